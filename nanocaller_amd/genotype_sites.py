"""Known-sites calling: the list of SNP positions a run is asked to genotype ("Genotyping a given list of sites").

`dct['genotype_sites']` / `params['genotype_sites']` is a VCF path (plain, gzipped or bgzipped) or a `{contig: positions}` dict;
`genotype_only` truthy makes the list the only source of candidates.  Without the keys the environment's NC_GENOTYPE_SITES /
NC_GENOTYPE_ONLY=1 are read, so the reference's `run(args)`, which builds the dicts itself, can drive the mode.  The candidate test
of generate_SNP_pileups.py:183 then reads `min_allele_freq <= alt_freq or v_pos in S` (or `v_pos in S` alone); the scan kernel
applies it (nc_snp_scan_set_sites), nothing downstream changes.

The indel half ("Genotyping a given list of indel sites") has keys of its own, `genotype_indel_sites` / `genotype_indel_only`
(NC_GENOTYPE_INDEL_SITES / NC_GENOTYPE_INDEL_ONLY=1): a listed column becomes a candidate of the indel window scan under its depth test
(nc_indel_set_sites, device pipeline only).  The SNP keys and their parser do not read indel lines and are not touched by it.

Neighbour sites given as a list ("Listed neighbour sites and background sampling"): `neighbor_sites` / `neighbor_only`
(NC_NEIGHBOR_SITES / NC_NEIGHBOR_ONLY=1), a `{contig: positions}` dict or a VCF of which the heterozygous single-base records count.  The
neighbour test of :173 / :177 then reads `frequency rule or v_pos in L` (or `v_pos in L` alone; nc_snp_scan_set_nbr_sites).  The two SNP lists
are independent: a listed neighbour is no candidate because of it, a position to genotype no neighbour.
"""
from __future__ import annotations

import os
import threading

import numpy as np

_EMPTY = np.zeros(0, np.int32)
_VCFS = {}                    # (path, size, mtime) -> ({contig: sorted unique int32 positions}, data lines skipped)
_LOCK = threading.Lock()


def parse_sites_vcf(path):
    """-> ({contig: sorted unique int32 POS}, n_skipped): every data line with a one-base REF contributes its POS, whatever its ALT;
    the others (indels, MNPs, malformed lines) are skipped and counted"""
    from .vcfio import read_vcf_gz
    _, recs = read_vcf_gz(path)
    by_contig, skipped = {}, 0
    for ln in recs:
        f = ln.split("\t", 5)
        if len(f) < 5 or len(f[3]) != 1 or not f[1].isdigit():
            skipped += bool(ln.strip())
            continue
        by_contig.setdefault(f[0], []).append(int(f[1]))
    lim = np.iinfo(np.int32).max
    out = {}
    for c, p in by_contig.items():
        a = np.unique(np.asarray(p, np.int64))
        out[c] = a[(a >= 1) & (a <= lim)].astype(np.int32)
    return out, skipped


def load_sites_vcf(path):
    """parse_sites_vcf, once per file (keyed by path, size and modification time)"""
    path = str(path)
    st = os.stat(path)
    key = (path, st.st_size, st.st_mtime_ns)
    with _LOCK:
        hit = _VCFS.get(key)
    if hit is None:
        hit = parse_sites_vcf(path)
        with _LOCK:
            for k in [k for k in _VCFS if k[0] == path]:
                del _VCFS[k]
            _VCFS[key] = hit
    return hit


def sites_for(dct, chrom):
    """-> (positions, only): the sorted unique int32 positions listed for `chrom` (None when no list is given at all) and whether
    the list alone decides.  A list that names no position of `chrom` is an empty array: in only mode that contig yields nothing."""
    src = dct.get("genotype_sites") if "genotype_sites" in dct else (os.environ.get("NC_GENOTYPE_SITES") or None)
    if src is None or (isinstance(src, str) and not src):
        return None, False
    only = bool(dct["genotype_only"]) if "genotype_only" in dct else os.environ.get("NC_GENOTYPE_ONLY") == "1"
    if isinstance(src, dict):
        p = src.get(chrom)
        if p is None:
            return _EMPTY, only
        a = np.unique(np.asarray(p).astype(np.int64, copy=False).ravel())
        return a[(a >= 1) & (a <= np.iinfo(np.int32).max)].astype(np.int32), only
    return load_sites_vcf(src)[0].get(chrom, _EMPTY), only


_NBR_VCFS = {}                # (path, size, mtime) -> {contig: sorted unique int32 positions}
_BASES = frozenset("AGTC")


def parse_neighbor_vcf(path):
    """-> {contig: sorted unique int32 POS} of the heterozygous single-base records, the test of the reference's training generator
    (misc/training/generate_SNP_pileups.py:135-144): REF one of A, G, T, C, the first sample's GT two different allele indices ('/' or '|'),
    both chosen alleles single bases.  A file without sample columns gives every record with a single-base REF and one single-base ALT."""
    from .vcfio import read_vcf_gz
    _, recs = read_vcf_gz(path)
    by_contig = {}
    for ln in recs:
        f = ln.rstrip("\r\n").split("\t")
        if len(f) < 5 or not f[1].isdigit() or f[3].upper() not in _BASES:
            continue
        alleles = [f[3].upper()] + [a.upper() for a in f[4].split(",")]
        if len(f) >= 10:
            fmt = f[8].split(":")
            if "GT" not in fmt:
                continue
            g = f[9].split(":")[fmt.index("GT")].replace("|", "/").split("/")
            if len(g) != 2 or not all(v.isdigit() for v in g) or g[0] == g[1] or max(int(g[0]), int(g[1])) >= len(alleles):
                continue
            chosen = (alleles[int(g[0])], alleles[int(g[1])])
        elif len(alleles) == 2:
            chosen = (alleles[0], alleles[1])
        else:
            continue
        if chosen[0] in _BASES and chosen[1] in _BASES:
            by_contig.setdefault(f[0], []).append(int(f[1]))
    lim = np.iinfo(np.int32).max
    out = {}
    for c, p in by_contig.items():
        a = np.unique(np.asarray(p, np.int64))
        out[c] = a[(a >= 1) & (a <= lim)].astype(np.int32)
    return out


def load_neighbor_vcf(path):
    """parse_neighbor_vcf, once per file (keyed by path, size and modification time)"""
    path = str(path)
    st = os.stat(path)
    key = (path, st.st_size, st.st_mtime_ns)
    with _LOCK:
        hit = _NBR_VCFS.get(key)
    if hit is None:
        hit = parse_neighbor_vcf(path)
        with _LOCK:
            for k in [k for k in _NBR_VCFS if k[0] == path]:
                del _NBR_VCFS[k]
            _NBR_VCFS[key] = hit
    return hit


def neighbor_sites_for(dct, chrom):
    """-> (positions, only): the neighbour sites listed for `chrom` as sorted unique int32 positions (None when no list is given at all) and
    whether the list alone decides (nc_snp_scan_set_nbr_sites).  dct['neighbor_sites']: a {contig: positions} dict or a
    VCF path (parse_neighbor_vcf); dct['neighbor_only']; without the keys NC_NEIGHBOR_SITES / NC_NEIGHBOR_ONLY=1.  A list that names no position
    of `chrom` is an empty array: in only mode no column of that contig is a neighbour, and a site needs min_nbr_sites listed neighbours in
    reach (its own column not counted), so that contig yields nothing."""
    src = dct.get("neighbor_sites") if "neighbor_sites" in dct else (os.environ.get("NC_NEIGHBOR_SITES") or None)
    if src is None or (isinstance(src, str) and not src):
        return None, False
    only = bool(dct["neighbor_only"]) if "neighbor_only" in dct else os.environ.get("NC_NEIGHBOR_ONLY") == "1"
    if isinstance(src, dict):
        p = src.get(chrom)
        if p is None:
            return _EMPTY, only
        a = np.unique(np.asarray(p).astype(np.int64, copy=False).ravel())
        return a[(a >= 1) & (a <= np.iinfo(np.int32).max)].astype(np.int32), only
    return load_neighbor_vcf(src).get(chrom, _EMPTY), only


LONG_INDEL = 10               # a listed indel is of the long-window class when an ALT differs from REF by more bases than this
_INDEL_VCFS = {}              # (path, size, mtime) -> {contig: (sorted unique int32 positions, uint8 is_long)}
_EMPTY_LONG = np.zeros(0, np.uint8)


def _indel_arrays(pos, is_long):
    """sorted unique int32 positions in [1, 2^31) with their class; a position listed with both classes is long"""
    pos = np.asarray(pos).astype(np.int64, copy=False).ravel()
    lng = np.zeros(pos.size, np.uint8) if is_long is None else (np.asarray(is_long).ravel() != 0).astype(np.uint8)
    if lng.size != pos.size:
        raise ValueError("genotype_indel_sites: %d positions with %d class flags" % (pos.size, lng.size))
    ok = (pos >= 1) & (pos <= np.iinfo(np.int32).max)
    pos, lng = pos[ok], lng[ok]
    u, inv = np.unique(pos, return_inverse=True)
    out = np.zeros(u.size, np.uint8)
    np.maximum.at(out, inv, lng)
    return u.astype(np.int32), out


def parse_indel_sites_vcf(path):
    """-> {contig: (sorted unique int32 POS, uint8 is_long)}: every data line with an ALT allele whose length differs from REF's (the test of
    indelCaller._non_snp) contributes its POS; the class is long when max |len(ALT_i) - len(REF)| > 10.  SNP lines are skipped."""
    from .vcfio import read_vcf_gz
    _, recs = read_vcf_gz(path)
    by_contig = {}
    for ln in recs:
        f = ln.split("\t", 5)
        if len(f) < 5 or not f[1].lstrip("-").isdigit():
            continue
        d = [abs(len(a) - len(f[3])) for a in f[4].split(",")]
        if not any(d):
            continue
        p, g = by_contig.setdefault(f[0], ([], []))
        p.append(int(f[1]))
        g.append(max(d) > LONG_INDEL)
    return {c: _indel_arrays(p, g) for c, (p, g) in by_contig.items()}


def load_indel_sites_vcf(path):
    """parse_indel_sites_vcf, once per file (keyed by path, size and modification time)"""
    path = str(path)
    st = os.stat(path)
    key = (path, st.st_size, st.st_mtime_ns)
    with _LOCK:
        hit = _INDEL_VCFS.get(key)
    if hit is None:
        hit = parse_indel_sites_vcf(path)
        with _LOCK:
            for k in [k for k in _INDEL_VCFS if k[0] == path]:
                del _INDEL_VCFS[k]
            _INDEL_VCFS[key] = hit
    return hit


def indel_list_given(dct):
    """whether a list of indel sites is given at all (the key, or the environment when the key is absent); reads no file"""
    src = dct.get("genotype_indel_sites") if "genotype_indel_sites" in dct else (os.environ.get("NC_GENOTYPE_INDEL_SITES") or None)
    return not (src is None or (isinstance(src, str) and not src))


def indel_sites_for(dct, chrom):
    """-> (positions, is_long, only): the sorted unique int32 columns listed for `chrom` with their class (None, None when no list is given at
    all) and whether the list alone decides.  dct['genotype_indel_sites']: a VCF path, {contig: positions} (all small) or {contig: (positions,
    is_long)}; dct['genotype_indel_only']; without the keys NC_GENOTYPE_INDEL_SITES / NC_GENOTYPE_INDEL_ONLY=1."""
    src = dct.get("genotype_indel_sites") if "genotype_indel_sites" in dct else (os.environ.get("NC_GENOTYPE_INDEL_SITES") or None)
    if src is None or (isinstance(src, str) and not src):
        return None, None, False
    only = bool(dct["genotype_indel_only"]) if "genotype_indel_only" in dct else os.environ.get("NC_GENOTYPE_INDEL_ONLY") == "1"
    if isinstance(src, dict):
        p = src.get(chrom)
        if p is None:
            return _EMPTY, _EMPTY_LONG, only
        if isinstance(p, tuple) and len(p) == 2 and np.ndim(p[0]) == 1:
            return _indel_arrays(p[0], p[1]) + (only,)
        return _indel_arrays(p, None) + (only,)
    p, g = load_indel_sites_vcf(src).get(chrom, (_EMPTY, _EMPTY_LONG))
    return p, g, only


def count_listed(sites, chunks, emitted_pos):
    """-> (listed, emitted): how many listed positions lie inside one of `chunks` ((start, end) inclusive), and how many of those are
    among `emitted_pos` (the positions that got a record).  listed - emitted positions failed a test of :161-170 or had no tensor."""
    if sites is None or sites.size == 0:
        return 0, 0
    inside = np.zeros(sites.size, bool)
    for a, b in chunks:
        inside[np.searchsorted(sites, a, "left"):np.searchsorted(sites, b, "right")] = True
    s = sites[inside]
    return int(s.size), int(np.isin(s, np.asarray(emitted_pos)).sum()) if s.size else 0


__all__ = ["parse_sites_vcf", "load_sites_vcf", "sites_for", "count_listed", "parse_neighbor_vcf", "load_neighbor_vcf", "neighbor_sites_for", "parse_indel_sites_vcf", "load_indel_sites_vcf", "indel_sites_for", "indel_list_given"]

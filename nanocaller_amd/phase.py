"""Read-based SNP phasing and read haplotagging on the GPU: the built-in replacement for the `whatshap phase` +
`whatshap haplotag` steps of phase_run (nanocaller_src/indelCaller.py:192-262).  DESIGN.md "Read-based phasing" states the
algorithm (an exact minimum-error-correction phaser, WhatsHap's model, every tie-break fixed) and its deviations from WhatsHap.

`phase_contig` phases one contig's het SNP calls from the reads of its resident pack (the SNP pass's `device_pack`: nothing is
decoded twice) and returns the phased records, the blocks and a haplotag table: per read NAME its 64-bit FNV-1a hash (the hash
the device ingest's record meta carries), HP and PS.  The indel pass takes HP / PS from such a table instead of the BAM's own tags
when a chunk carries `haplotags` (`TaggedBam`).  Opt-in: params['phaser'] = 'device', or NC_PHASER=device when params has no
'phaser' key (`device_phaser_selected`).  Behind it, params['phase_realign'] / NC_PHASE_REALIGN=1 (`phase_realign_selected`) selects the
alleles by local realignment (WhatsHap's `--reference` mode restated) instead of the pileup column's code; params['phase_distrust'] /
NC_PHASE_DISTRUST=1 (`phase_distrust_selected`) lets the phaser change genotypes and take homozygous calls (WhatsHap's `--distrust-genotypes
--include-homozygous` restated: `phase_contig(distrust=True)`); params['phase_weighted'] / NC_PHASE_WEIGHTED=1 (`phase_weighted_selected`) weighs every
allele by its base quality and leaves reads below a MAPQ floor out of the MEC (WhatsHap's weighted MEC restated: `phase_contig(weighted=True)`;
the qualities and MAPQs are read from the device ingest's record stream, so the contig has to take that route).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np

from .synth import FLAG_FILTER_DEFAULT, FLAG_FILTER_SUPPL, World

_CODE = {"A": 0, "G": 1, "T": 2, "C": 3}
_FNV_OFFSET = np.uint64(1469598103934665603)
_FNV_PRIME = np.uint64(1099511628211)


def _selected(params, key, env, on=None) -> bool:
    """params[key] (== `on`, or truthy where `on` is None); without that key, the environment's `env` == `on` (or '1')"""
    if key in params:
        return bool(params[key]) if on is None else params[key] == on
    return os.environ.get(env) == ("1" if on is None else on)


def device_phaser_selected(params) -> bool:
    """params['phaser'] == 'device'; without that key, the environment's NC_PHASER == 'device'"""
    return _selected(params, "phaser", "NC_PHASER", "device")


def phased_bam_selected(params) -> bool:
    """params['phased_bam'] truthy; without that key, the environment's NC_PHASED_BAM == '1' (phase_run writes <contig>.phased.bam behind
    the device phaser: bam_write.py)"""
    return _selected(params, "phased_bam", "NC_PHASED_BAM")


def phase_realign_selected(params) -> bool:
    """params['phase_realign'] truthy; without that key, the environment's NC_PHASE_REALIGN == '1' (the device phaser takes a read's allele
    at a site from a local realignment against both haplotypes instead of the code in the site's column: `phase_contig(realign=True)`)"""
    return _selected(params, "phase_realign", "NC_PHASE_REALIGN")


def phase_distrust_selected(params) -> bool:
    """params['phase_distrust'] truthy; without that key, the environment's NC_PHASE_DISTRUST == '1' (the device phaser may leave a site's called
    genotype at a price and takes the homozygous-ALT calls too: `phase_contig(distrust=True)`)"""
    return _selected(params, "phase_distrust", "NC_PHASE_DISTRUST")


def phase_weighted_selected(params) -> bool:
    """params['phase_weighted'] truthy; without that key, the environment's NC_PHASE_WEIGHTED == '1' (the device phaser weighs alleles by base
    quality and keeps reads below the MAPQ floor params['phase_mapq'] (default 20) out of the MEC: `phase_contig(weighted=True)`)"""
    return _selected(params, "phase_weighted", "NC_PHASE_WEIGHTED")


def name_hash(names) -> np.ndarray:
    """FNV-1a (64 bit) of every read name with its terminating NUL: the hash of the BAM record's read_name field, as the device
    ingest computes it (nc_ingest.hip, meta rows M_HASH_LO / M_HASH_HI)"""
    n = len(names)
    if n == 0:
        return np.zeros(0, np.uint64)
    enc = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in names]
    ln = np.fromiter((len(b) for b in enc), np.int64, n)
    w = int(ln.max()) + 1
    buf = np.zeros((n, w), np.uint8)
    flat = np.frombuffer(b"".join(enc), np.uint8)
    rows = np.repeat(np.arange(n), ln)
    cols = np.arange(flat.size) - np.repeat(np.cumsum(ln) - ln, ln)
    buf[rows, cols] = flat
    h = np.full(n, _FNV_OFFSET, np.uint64)
    with np.errstate(over="ignore"):
        for k in range(w):
            m = k <= ln                                                    # (k == len: the NUL byte)
            h[m] = (h[m] ^ buf[m, k].astype(np.uint64)) * _FNV_PRIME
    return h


@dataclass
class PhaseResult:
    records: list                      # VCF record lines, phased ones rewritten (GT with '|', FORMAT + ':PS')
    blocks: list                       # (first site position, last site position, PS, MEC cost) per block
    haplotags: dict                    # hash uint64 [n] ascending, hp uint8 [n], ps int32 [n]: tagged read names only
    sites: dict = field(default_factory=dict)    # pos, record index, h, phased, ps, called class gt_in and outcome gt_out per site
    reads: dict = field(default_factory=dict)    # kept reads: index into the World, name hash, group, side, hp, ps
    ms: dict = field(default_factory=dict)


def _sites(snp_records, phase_qual_score, homozygous):
    q = float(phase_qual_score)
    idx, pos, al, kind = [], [], [], []
    last = 0
    for i, ln in enumerate(snp_records):
        f = ln.rstrip("\n").split("\t")
        if len(f) < 10 or not float(f[5]) >= q:
            continue
        gt = f[9].split(":", 1)[0]
        alts = f[4].split(",")
        if gt == "0/1" and len(alts) == 1:
            a = (f[3], alts[0])
        elif gt == "1/2" and len(alts) == 2:
            a = (alts[0], alts[1])
        elif homozygous and gt == "1/1" and len(alts) == 1:
            a = (f[3], alts[0])
        else:
            continue
        if a[0] not in _CODE or a[1] not in _CODE or int(f[1]) <= last:
            continue
        last = int(f[1])
        idx.append(i)
        pos.append(last)
        al.append((_CODE[a[0]], _CODE[a[1]]))
        kind.append(gt)
    return (np.array(idx, np.int64), np.array(pos, np.int32), np.array(al, np.uint8).reshape(-1, 2), kind)


def het_sites(snp_records, phase_qual_score):
    """the records the phaser takes: QUAL >= phase_qual_score, GT 0/1 or 1/2, single-base alleles -> (record index, pos, alleles [n, 2], kind)"""
    return _sites(snp_records, phase_qual_score, False)


def distrust_sites(snp_records, phase_qual_score):
    """the records the phaser takes when it distrusts genotypes: het_sites' and GT 1/1 with one single-base ALT (alleles REF, ALT)
    -> (record index, pos, alleles [n, 2], kind, gt uint8 [n]: the called class, 0 het, 2 homozygous for the second allele)"""
    idx, pos, al, kind = _sites(snp_records, phase_qual_score, True)
    return idx, pos, al, kind, np.array([2 if k == "1/1" else 0 for k in kind], np.uint8)


def phased_record(line, h, ps):
    """one record with its GT phased (0/1 -> 0|1 when h = 0, 1|0 when h = 1; 1/2 -> 1|2 / 2|1) and PS appended"""
    f = line.rstrip("\n").split("\t")
    smp = f[9].split(":")
    a, b = smp[0].split("/")
    smp[0] = ("%s|%s" % (a, b)) if h == 0 else ("%s|%s" % (b, a))
    f[8] += ":PS"
    f[9] = ":".join(smp) + ":%d" % ps
    return "\t".join(f) + "\n"


def distrust_record(line, kind, outcome, h, phased, ps):
    """one record of a site of `distrust_sites` with the phaser's outcome written into its GT.  kind: the called GT; outcome 0 het (phased: GT
    with '|' by h and PS appended, a called 1/1 as 0|1 / 1|0), 1 / 2 homozygous for the site's first / second allele (0/1 -> 0/0 / 1/1,
    1/2 -> 1/1 / 2/2, 1/1 -> 0/0 / 1/1).  Every other byte of the record stays."""
    a, b = ("1", "2") if kind == "1/2" else ("0", "1")
    if outcome == 0 and phased:
        return phased_record(line if kind != "1/1" else _with_gt(line, "0/1"), h, ps)
    gt = "%s/%s" % ((a, b) if outcome == 0 else (a, a) if outcome == 1 else (b, b))
    return line if gt == kind else _with_gt(line, gt)


def _with_gt(line, gt):
    f = line.rstrip("\n").split("\t")
    f[9] = ":".join([gt] + f[9].split(":")[1:])
    return "\t".join(f) + "\n"


def kept_reads(world: World, supplementary):
    """the alignments the SNP pileup keeps (flag filter, htslib's depth cap), in pack order -> (World indices, start, end, slot_off)"""
    from .pack import pileup_depth_cap
    filt = FLAG_FILTER_SUPPL if supplementary else FLAG_FILTER_DEFAULT
    keep = pileup_depth_cap(world.read_start, world.read_end, np.ascontiguousarray((np.asarray(world.read_flag) & filt) == 0, np.uint8))
    kept = np.flatnonzero(keep)
    rs = np.ascontiguousarray(np.asarray(world.read_start)[kept], np.int32)
    re_ = np.ascontiguousarray(np.asarray(world.read_end)[kept], np.int32)
    slot = np.zeros(kept.size + 1, np.int64)
    np.cumsum(((re_.astype(np.int64) + 15) & ~15) - (rs.astype(np.int64) & ~15), out=slot[1:])     # (nc_pack_fill's slot layout)
    return kept, rs, re_, slot


def _ref_codes(fasta: str) -> np.ndarray:
    """uint8 [L]: A0 G1 T2 C3 in either letter case, 4 otherwise (position p at index p - 1)"""
    lut = np.full(256, 4, np.uint8)
    for k, b in enumerate("AGTC"):
        lut[ord(b)] = lut[ord(b.lower())] = k
    return lut[np.frombuffer(fasta.encode("ascii"), np.uint8)]


def _realign_inputs(sam_path, fasta_path, chrom, supplementary, device):
    """what nc_snp_phase_realign reads beside the sites: the contig's pack with its events and inserted bases, as the indel route loads them (from
    the BAM on the device where that route is open, else from the host decode), and the reference codes -> (pack, Engine.snp_phase's `realign`)"""
    import torch

    from . import _lib
    if not (isinstance(sam_path, str) and os.path.exists(sam_path)) or not fasta_path:
        raise _lib.NanoCallerHipError("phase_contig(realign=True) needs a BAM file and its FASTA: the alignments %r carry no inserted bases to rebuild "
                                      "the reads' query windows from (the column rule is not substituted)" % (sam_path,))
    from .indel_device import indel_pack_for, keep_flag
    dct = dict(fasta_path=fasta_path, supplementary=bool(supplementary))
    eng, dp, reads_c, ctg, _, _ = indel_pack_for(dct, [dict(chrom=chrom, sam_path=sam_path)], device)
    ix = dp.indel if ctg.get("device_ingest") else ctg[("dev_reads", keep_flag(dct), device)][1]
    if dp.events is None or dp.reads is None or ix is None:
        raise _lib.NanoCallerHipError("phase_contig(realign=True): the pack of %r, contig %s, carries no indel events / inserted bases" % (sam_path, chrom))
    key = ("phase_ref_code", device)
    if key not in ctg:
        # (a reference that took the device route, device_fasta.py: the same codes were made in HBM beside the letters)
        ctg[key] = ctg["ref_contig"].blind_codes if ctg.get("ref_contig") is not None else torch.from_numpy(_ref_codes(ctg["fasta"])).to(eng.device)
    return dp, (dp.codes, reads_c, dp.events["ev_pos"].numel(), ix["ins_bases"].numel(), ctg[key])


def _ingest_records(sam_path, fasta_path, chrom, supplementary, device):
    """the contig's pack as the device ingest makes it, with the record stream it was made from -> (pack, (raw uint8 device tensor, the kept
    reads' record offsets in pack order)).  The weighted model reads MAPQ and base qualities there and nowhere else: an input that does not take
    that route is refused, unit costs are not substituted."""
    from . import _lib
    from .indel_device import ingest_contig
    why = None
    if not (isinstance(sam_path, str) and os.path.exists(sam_path)) or not fasta_path:
        why = "the alignments %r are not a BAM file with its FASTA (a World or a registered key carries no record bytes)" % (sam_path,)
    else:
        di = ingest_contig(dict(fasta_path=fasta_path, supplementary=bool(supplementary)), sam_path, chrom, bool(supplementary), device)
        if di is None:
            why = ("%s does not take the device ingest route (NC_DEVICE_INGEST=0, no .bai / .csi beside it, or too large for HBM)" % sam_path)
        elif getattr(di[0], "records", None) is None:
            why = "the pack of %s, contig %s, does not carry its record stream" % (sam_path, chrom)
    if why:
        raise _lib.NanoCallerHipError("phase_contig(weighted=True): %s; MAPQ and base qualities exist only in the device ingest's record stream "
                                      "(unit costs are not substituted)" % why)
    dbam, rec_off = di[0].records
    return di[0], (dbam.raw[:dbam.raw_len], rec_off)


def phase_contig(sam_path, fasta_path, chrom, snp_records, phase_qual_score, supplementary=False, max_cov=15, device=0, realign=False, distrust=False,
                 distrust_cost=None, weighted=False, mapq_min=20, default_weight=30, w_max=93) -> PhaseResult:
    """Phase the het SNP calls `snp_records` (VCF lines of contig `chrom`) from the reads of `sam_path` (a BAM path, a World or a
    registered key) and haplotag the reads.  -> PhaseResult
    realign: a read's allele at a site comes from a local realignment of its bases against the reference window with either allele (DESIGN.md
    "Read-based phasing", the allele detectors) instead of the code in the site's column; needs a BAM file (the reads' inserted bases).
    distrust: the genotypes are not trusted (DESIGN.md "Read-based phasing", step 6b): the sites are `distrust_sites`', a site may come out het or
    homozygous for either allele, leaving its call costs `distrust_cost` allele errors (default 1; in weighted mode `default_weight`, one
    allele of default quality), and the records' GT follow the outcome.
    weighted: the weighted model (DESIGN.md "Read-based phasing", step 6c): an allele's flip costs min(its base quality, w_max) -- `default_weight`
    where the record has no quality --, reads with MAPQ < `mapq_min` are left out of the MEC and still tagged.  The qualities come from the device
    ingest's record stream: a World, a registered key, NC_DEVICE_INGEST=0 or a BAM without index raises NanoCallerHipError."""
    import torch

    from .engine import get_engine
    from .generate_SNP_pileups import _resolve, device_pack
    eng = get_engine(device)
    eng.use_torch_stream()
    wdp = quals = None
    if weighted:
        wdp, quals = _ingest_records(sam_path, fasta_path, chrom, supplementary, device)
    if distrust_cost is None:
        distrust_cost = max(1, int(default_weight)) if weighted else 1
    if distrust:
        rec_idx, pos, alleles, kind, gt_in = distrust_sites(snp_records, phase_qual_score)
        solve = dict(site_gt=gt_in, distrust_cost=distrust_cost)
    else:
        rec_idx, pos, alleles, kind = het_sites(snp_records, phase_qual_score)
        gt_in, solve = np.zeros(pos.size, np.uint8), {}
    ra = None
    if realign:
        dp, ra = _realign_inputs(sam_path, fasta_path, chrom, supplementary, device)
    world = _resolve(sam_path, chrom, fasta_path)
    if not realign:
        dp = wdp if weighted else device_pack(sam_path, fasta_path, chrom, bool(supplementary), None, device, by_name=True)[0]
    if weighted:
        if dp is not wdp:
            raise RuntimeError("phase_contig: the alleles and the qualities come from two packs")
        solve = dict(solve, bam_quals=quals + (int(mapq_min), int(default_weight), int(w_max)))
    kept, rs, re_, slot = kept_reads(world, supplementary)
    if dp.reads is not None:
        if dp.reads["n_reads"] != kept.size:
            raise RuntimeError("phase_contig: the pack holds %d reads, the flag filter keeps %d" % (dp.reads["n_reads"], kept.size))
        reads = (dp.codes, dp.reads["rd_start"], dp.reads["rd_end"], dp.reads["slot_off"])
    else:
        dev = eng.device
        reads = (dp.codes, torch.from_numpy(rs).to(dev), torch.from_numpy(re_).to(dev), torch.from_numpy(slot).to(dev))
    if int(slot[-1]) > dp.codes.numel():
        raise RuntimeError("phase_contig: the read table addresses %d code bytes, the pack holds %d" % (int(slot[-1]), dp.codes.numel()))
    from .pack import world_names
    names = world_names(world)
    if names is not None:
        hashes = name_hash([names[k] for k in kept.tolist()])
        uniq, group = np.unique(hashes, return_inverse=True)
    else:                                                               # no names: every alignment is its own read
        hashes = np.zeros(kept.size, np.uint64)
        uniq, group = np.zeros(kept.size, np.uint64), np.arange(kept.size)
    if realign:
        if dp.reads is None or ra[1].n_reads != kept.size:
            raise RuntimeError("phase_contig: the indel read table holds %d reads, the flag filter keeps %d" % (ra[1].n_reads, kept.size))
        r = eng.snp_phase(pos, alleles, group.astype(np.int32), len(uniq), max_cov=max_cov, realign=ra, **solve)
    else:
        r = eng.snp_phase(pos, alleles, group.astype(np.int32), len(uniq), max_cov=max_cov, reads=reads, **solve)
    out = list(snp_records)
    gt_out = r["site_gt"] if distrust else gt_in
    if distrust:
        for k, i in enumerate(rec_idx.tolist()):
            out[i] = distrust_record(snp_records[i], kind[k], int(gt_out[k]), int(r["site_h"][k]), bool(r["site_phased"][k]), int(r["site_ps"][k]))
    else:
        for k in np.flatnonzero(r["site_phased"]).tolist():
            out[int(rec_idx[k])] = phased_record(snp_records[int(rec_idx[k])], int(r["site_h"][k]), int(r["site_ps"][k]))
    blocks = [(int(pos[f]), int(pos[l_]), int(ps), int(c)) for f, l_, ps, c in zip(r["block_first"], r["block_last"], r["block_ps"], r["block_cost"])]
    tagged = r["group_hp"] != 0
    tags = dict(hash=np.ascontiguousarray(uniq[tagged] if names is not None else np.zeros(0, np.uint64)),
                hp=np.ascontiguousarray(r["group_hp"][tagged] if names is not None else np.zeros(0, np.uint8)),
                ps=np.ascontiguousarray(r["group_ps"][tagged] if names is not None else np.zeros(0, np.int32)))
    sites = dict(pos=pos, record=rec_idx, h=r["site_h"], phased=r["site_phased"], ps=r["site_ps"], block=r["site_block"], gt_in=gt_in, gt_out=gt_out)
    reads_out = dict(index=kept, hash=hashes, group=group, side=r["side"], hp=r["group_hp"][group], ps=r["group_ps"][group],
                     entry_off=r["entry_off"], entry_site=r["entry_site"], entry_allele=r["entry_allele"])
    if weighted:
        reads_out.update(entry_weight=r["entry_weight"], mapq=r["read_mapq"], ok=r["read_ok"])
    return PhaseResult(records=out, blocks=blocks, haplotags=tags, sites=sites, reads=reads_out, ms=r["ms"])


# ------------------------------------------------------------------------------------------- haplotag tables in the indel pass
def save_haplotags(path, tags):
    with open(path, "wb") as f:                                          # (an open file: np.savez would append '.npz' to a bare name)
        np.savez(f, hash=np.asarray(tags["hash"], np.uint64), hp=np.asarray(tags["hp"], np.uint8), ps=np.asarray(tags["ps"], np.int32))


_TABLES = {}


def load_haplotags(path):
    st = os.stat(path)
    key = (os.path.abspath(path), st.st_size, st.st_mtime_ns)
    if key not in _TABLES:
        _TABLES.clear()
        with np.load(path) as z:
            h, hp, ps = z["hash"].astype(np.uint64), z["hp"].astype(np.uint8), z["ps"].astype(np.int32)
        o = np.argsort(h, kind="stable")
        _TABLES[key] = (h[o], hp[o], ps[o])
    return _TABLES[key]


def tags_for_hashes(hashes, path):
    """(HP uint8, PS int32) per read-name hash from the table at `path`: names the table lacks are untagged (0, 0)"""
    h, hp, ps = load_haplotags(path)
    hashes = np.asarray(hashes, np.uint64)
    i = np.searchsorted(h, hashes)
    i = np.minimum(i, max(h.size - 1, 0))
    hit = (h[i] == hashes) if h.size else np.zeros(hashes.size, bool)
    return np.where(hit, hp[i] if h.size else 0, 0).astype(np.uint8), np.where(hit, ps[i] if h.size else 0, 0).astype(np.int32)


def tags_for_names(names, path):
    return tags_for_hashes(name_hash(names), path)


class TaggedBam(str):
    """The path of a BAM whose alignments take HP / PS from the haplotag table `tags` (by read name) instead of their own tags.
    It compares and hashes unequal to the bare path and to other tables, so every cache keyed by the source (decoded contig,
    resident pack, device-ingested contig) keeps the tagged and the untagged variant apart; file access sees the plain path."""

    def __new__(cls, path, tags):
        s = super().__new__(cls, path)
        s.tags = str(tags)
        return s

    def __eq__(self, other):
        return isinstance(other, TaggedBam) and str.__eq__(self, other) and self.tags == other.tags

    def __ne__(self, other):
        return not self.__eq__(other)

    def __hash__(self):
        return hash((str.__str__(self), self.tags))

    def __reduce__(self):
        return (TaggedBam, (str.__str__(self), self.tags))


def tagged_source(chunk):
    """chunk['sam_path'] as the indel pass reads it: a TaggedBam when the chunk carries `haplotags`"""
    sp = chunk["sam_path"]
    if chunk.get("haplotags") and isinstance(sp, str) and not isinstance(sp, TaggedBam):
        return TaggedBam(sp, chunk["haplotags"])
    return sp


def retag_decoded(d, sam_path):
    """a host decode (dict with names / hap / ps) of a TaggedBam: HP / PS overwritten in place from the table"""
    if isinstance(sam_path, TaggedBam):
        hp, ps = tags_for_names(d["names"], sam_path.tags)
        d["hap"][:] = hp
        d["ps"][:] = ps
    return d

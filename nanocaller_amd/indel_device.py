"""The Python side of the device-resident indel pipeline (nc_pipe.hip: pass 1 + 2 of get_indel_testing_candidates[_haploid] for all chunks of
a contig with no host code between the column decisions and the CNN input) and of the contig ingest that feeds it.

* `ingest_contig` / `indel_pack_for`: a contig's read pack WITH its indel sections, made on the device from the BAM file itself or from the host
  decode, cached one contig at a time (`_DEV_INGEST`; the host decode's cache is generate_indel_pileups._CONTIGS).
* `indel_sites_device` / `indel_sites_fetch`: nc_indel_sites_plan + _run + _fetch.
* `sites_to_tuples` (the per-chunk tuples of the reference's calls) and `sites_to_vcf_text` (the native genotype rules: VCF text without a Python
  object per site) of a run's sites.  What lays a `dct` and its chunks onto these calls is generate_indel_pileups.indel_sites_for_chunks.
* the small things every indel featuriser derives from its `dct`: `keep_flag`, `window_after_of`, `exclusion_mask`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .engine import get_engine
from .generate_SNP_pileups import _exclude_rows, device_pack
from .synth import FLAG_FILTER_DEFAULT, FLAG_FILTER_SUPPL


def keep_flag(dct):
    """the FLAG bits that keep an alignment out of the pileups (unmapped, secondary, qcfail, duplicate; supplementary unless dct['supplementary'])"""
    return FLAG_FILTER_SUPPL if dct.get("supplementary") else FLAG_FILTER_DEFAULT


def window_after_of(dct):
    """bases of a pass-2 read window behind its anchor (generate_indel_pileups.py:140-143)"""
    return 260 if dct["seq"] == "pacbio" else 160


def exclusion_mask(dct, chrom, dp):
    """dct['exclude_bed'] over the columns of the pack `dp` (uint8 on its device, 1 = excluded), or None without exclusions on `chrom`"""
    rows = _exclude_rows(dct, chrom)
    if not rows:
        return None
    m = np.zeros(dp.n_tiles * dp.tile_size, np.uint8)
    for (a, b) in rows:                                             # IntervalTree.overlaps(pos): a <= pos < b
        m[max(0, a - dp.tile_pos0):max(0, b - dp.tile_pos0)] = 1
    return torch.from_numpy(m).to(dp.ref_code.device)


TAIL_CAP = 272                 # query bases kept behind a read's last aligned base (>= the longest window, 260 + rounding)


def device_indel_reads(ctg, flag, dp, device):
    """The per-read inputs of the device pass 2 beyond the read pack: inserted bases of every insertion event, the bases that
    follow the last aligned one, PS tags (nc_indel_pack_build), uploaded once per (contig, flag filter).  -> (IndelReadsC, tensors)"""
    key = ("dev_reads", flag, device)
    if key in ctg and ctg[key][2] is not dp:                         # the pack was rebuilt (LRU eviction, release_contig): these pointers belong to the old one
        del ctg[key]
    if key not in ctg:
        L = _lib.lib()
        keep = ctg["keep"][flag]
        h = C.c_void_p()
        rc = L.nc_indel_pack_build(ctg["handle"], _lib.npp(keep), TAIL_CAP, C.byref(h))
        if rc != _lib.NC_OK:
            raise _lib.NanoCallerHipError("nc_indel_pack_build failed (%d)" % rc, status=rc)
        try:
            v = _lib.IndelPackArraysC()
            L.nc_indel_pack_view(h, C.byref(v))
            if dp.events is None or dp.reads is None or v.n_reads != dp.events["n_reads"] or v.n_reads != dp.reads["n_reads"]:
                # (NC_ERR_CAPACITY: the callers fall back to the host-assembled route)
                raise _lib.NanoCallerHipError("the contig's read pack carries no indel events / read table for %d kept reads" % v.n_reads,
                                              status=_lib.NC_ERR_CAPACITY)
            dev = get_engine(device).device

            def up(ptr, cnt, dt):
                a = np.frombuffer((C.c_char * (int(cnt) * np.dtype(dt).itemsize)).from_address(ptr), dt) if cnt and ptr else np.zeros(0, dt)
                a = a if a.size else np.zeros(4, dt)
                return torch.from_numpy(a.copy()).to(dev)
            t = dict(ins_off=up(v.ins_off, v.n_events + 1, np.int32), ins_bases=up(v.ins_bases, v.n_ins_bases, np.uint8),
                     tail_off=up(v.tail_off, v.n_reads + 1, np.int32), tail_bases=up(v.tail_bases, v.n_tail_bases, np.uint8),
                     read_ps=up(v.read_ps, v.n_reads, np.int32), read_flag=up(v.read_flag, v.n_reads, np.uint8))
        finally:
            L.nc_indel_pack_free(h)
        ev, rd = dp.events, dp.reads
        st = _lib.IndelReadsC(n_reads=rd["n_reads"], slot_off=rd["slot_off"].data_ptr(), rd_start=rd["rd_start"].data_ptr(), rd_end=rd["rd_end"].data_ptr(),
                              ev_off=ev["ev_off"].data_ptr(), ev_pos=ev["ev_pos"].data_ptr(), ev_len=ev["ev_len"].data_ptr(),
                              ins_off=t["ins_off"].data_ptr(), ins_bases=t["ins_bases"].data_ptr(), tail_off=t["tail_off"].data_ptr(),
                              tail_bases=t["tail_bases"].data_ptr(), read_ps=t["read_ps"].data_ptr(), read_hap=ev["read_hap"].data_ptr(),
                              read_flag=t["read_flag"].data_ptr())
        ctg[key] = (st, t, dp)                                       # dp: keeps the pack's tensors alive with the pointers
    return ctg[key][0]


def indel_sites_device(eng, dp, reads_c, chrom_len, chunks, *, mincov, maxcov, win_size, small_win_size, ins_t, del_t, window_after,
                       haploid=False, excl=None, fetch=True, impute=False, mates=None, scoring=None, sites=None, sites_long=None, sites_only=False,
                       downsample=None):
    """downsample: None, or (mode, seed) for this plan (Engine.set_downsample): with 'uniform' a read set deeper than maxcov is a seeded uniform
    sample; a shared-names table or impute is then refused (NC_ERR_UNSUPPORTED).
    nc_indel_sites_plan + _run (+ _fetch) for a list of (start, end) chunks of one contig -> dict: n, x (device float32
    [n, sets * 5, 128, 2]: the CNN input), and with fetch: pos / chunk / type / phase int32 [n], ref_len / alt_len int32 [n, sets],
    alt (uint8 codes, the ALT prefixes back to back in (site, set) order).  mates: indel_mate_table's (key, rec) when kept alignments share read
    names.  scoring: the star alignment's (gap open, gap extend, match, mismatch), default _lib.STAR_SCORING; nc_indel_sites_scoring refuses values
    the 16-bit aligners do not cover.  sites: indel columns to genotype (1-based, an array or an int32 device tensor; None: no list, every launch is
    the plain one), sites_long: their class (nonzero = long window; None: all small), sites_only: the list is the only source of candidates
    (nc_indel_set_sites); the fetched dict then also holds src, the listed column behind every site (0: none).  Raises NanoCallerHipError with
    .status."""
    L, check = eng.L, eng._check
    prm = _lib.IndelScanParamsC(mincov=int(mincov), win_size=int(win_size), small_win_size=int(small_win_size), ins_t=float(ins_t),
                                del_t=float(del_t), haploid=1 if haploid else 0, impute=1 if (impute and not haploid) else 0)
    starts = np.ascontiguousarray([c[0] for c in chunks], np.int32)
    ends = np.ascontiguousarray([c[1] for c in chunks], np.int32)
    pc = dp.c_struct()
    n, na = C.c_int32(), C.c_int64()
    S = 1 if haploid else 3
    # the list is checked and uploaded before the context borrows anything
    listed = sites is not None
    t_pos = t_long = None
    if listed:
        t_pos = sites if torch.is_tensor(sites) else torch.from_numpy(np.ascontiguousarray(sites, np.int32)).to(eng.device)
        if sites_long is not None:
            t_long = sites_long if torch.is_tensor(sites_long) else torch.from_numpy((np.asarray(sites_long) != 0).astype(np.uint8)).to(eng.device)
            if t_long.numel() != t_pos.numel():
                raise ValueError("indel_sites_device: %d listed columns with %d class flags" % (t_pos.numel(), t_long.numel()))
        if t_pos.dtype != torch.int32 or (t_long is not None and t_long.dtype != torch.uint8):
            raise ValueError("indel_sites_device: listed columns are int32, their classes uint8")
    check(L.nc_indel_sites_scoring(eng.ctx, *[int(v) for v in (_lib.STAR_SCORING if scoring is None else scoring)]), "nc_indel_sites_scoring")
    # alignments that share read names: the plan keys them by name from this table (none: no table, the plain kernels run).  The context borrows
    # the pointers of the table and of the list, so both are cleared again once the plan's and the run's launches are enqueued, whatever their
    # outcome -- that of the set calls included
    try:
        with eng.downsampling(downsample):
            check(L.nc_indel_set_mates(eng.ctx, int(mates[0].numel()) if mates else 0, C.c_void_p(mates[0].data_ptr()) if mates else None,
                                       C.c_void_p(mates[1].data_ptr()) if mates else None), "nc_indel_set_mates")
            if listed:
                ns = int(t_pos.numel())
                check(L.nc_indel_set_sites(eng.ctx, ns, C.c_void_p(t_pos.data_ptr()) if ns else None,
                                           C.c_void_p(t_long.data_ptr()) if (ns and t_long is not None) else None, 1 if sites_only else 0), "nc_indel_set_sites")
            check(L.nc_indel_sites_plan(eng.ctx, C.byref(pc), C.c_void_p(dp.ref_code.data_ptr()), dp.tile_pos0, dp.ref_code.numel(), int(chrom_len),
                                        C.byref(reads_c), C.c_void_p(excl.data_ptr()) if excl is not None else None, len(chunks), _lib.npp(starts),
                                        _lib.npp(ends), C.byref(prm), int(window_after), int(maxcov), C.byref(n), C.byref(na)), "nc_indel_sites_plan")
            N = n.value
            x = torch.empty((N, S * 5, 128, 2), dtype=torch.float32, device=eng.device)
            check(L.nc_indel_sites_run(eng.ctx, C.c_void_p(x.data_ptr())), "nc_indel_sites_run")
    finally:
        if mates:
            L.nc_indel_set_mates(eng.ctx, 0, None, None)
        if listed:
            L.nc_indel_set_sites(eng.ctx, 0, None, None, 0)
    out = dict(n=N, sets=S, x=x, n_alignments=na.value)
    if fetch:
        out.update(indel_sites_fetch(eng, N, S, src=listed))
    return out


def indel_sites_fetch(eng, N, S, src=False):
    """nc_indel_sites_fetch (+ _fetch_alt) of the last plan + run; src (a list was set): also the listed column behind every site"""
    L = eng.L
    pos, chunk, typ, phase = (np.empty(max(N, 1), np.int32) for _ in range(4))
    rl, al = np.empty((max(N, 1), S), np.int32), np.empty((max(N, 1), S), np.int32)
    nb = C.c_int64()
    eng._check(L.nc_indel_sites_fetch(eng.ctx, _lib.npp(pos), _lib.npp(chunk), _lib.npp(typ), _lib.npp(phase), _lib.npp(rl), _lib.npp(al), C.byref(nb)),
               "nc_indel_sites_fetch")
    alt = np.empty(max(int(nb.value), 1), np.uint8)
    if nb.value:
        eng._check(L.nc_indel_sites_fetch_alt(eng.ctx, _lib.npp(alt), int(nb.value)), "nc_indel_sites_fetch_alt")
    out = dict(pos=pos[:N], chunk=chunk[:N], type=typ[:N], phase=phase[:N], ref_len=rl[:N], alt_len=al[:N], alt=alt[:int(nb.value)])
    if src:
        sc = np.zeros(max(N, 1), np.int32)
        eng._check(L.nc_indel_sites_fetch_src(eng.ctx, _lib.npp(sc)), "nc_indel_sites_fetch_src")
        out["src"] = sc[:N]
    return out


MATE_RING_CAP = 64           # alignments of one read name that k_hap_depth_b, k_event_tiles and k_sets<.., true> walk (their `guard` loops)


def indel_mate_table(dp, read_ps):
    """nc_indel_set_mates' table of a pack whose kept alignments share read names (dp.mates: pack.mate_table's key / rec on the device), or None.
    The reference keys hap_reads_0 / hap_reads_1 and phase_dict by name (generate_indel_pileups.py:178-188): a name is in a hap set when ANY of its
    records carries that HP (in both when they disagree), and phase_dict[name] is the PS of its LAST record in file order, None (0 here) when that
    record has no HP.  read_ps: the pack's PS per kept read (device int32).  -> (key int64 [M], rec int32 [M, 8]) device tensors.
    A name with more than MATE_RING_CAP kept alignments is refused (NC_ERR_UNSUPPORTED): the kernels walk a ring that far and no further."""
    if getattr(dp, "mates", None) is None or dp.reads is None or dp.events is None:
        return None
    key, rec4 = dp.mates
    M = int(key.numel())
    if M == 0:
        return None
    K = int(dp.reads["n_reads"])
    r = torch.searchsorted(dp.reads["slot_off"][:K].contiguous(), key.contiguous())       # the member's index among the kept reads (slots are unique)
    if int((r >= K).any()) or not bool((dp.reads["slot_off"][r] == key).all()):
        raise _lib.NanoCallerHipError("indel_mate_table: the table of shared names is not this pack's")
    rec4 = rec4.view(-1, 4).cpu().numpy()
    hap = dp.events["read_hap"][r].cpu().numpy().astype(np.int32)
    ps = read_ps[r].cpu().numpy().astype(np.int32)
    idx = np.arange(M, dtype=np.int64)
    nxt = rec4[:, 2].astype(np.int64)
    if M < 2 or nxt.min() < 0 or nxt.max() >= M:
        raise _lib.NanoCallerHipError("indel_mate_table: the table of shared names is not this pack's")
    g, cur = idx.copy(), nxt.copy()                                 # the name's first member: the smallest index on the member's ring
    for _ in range(MATE_RING_CAP - 1):                              # (cur: one hop further per step, held once it is back at the member)
        g = np.minimum(g, cur)
        cur = np.where(cur != idx, nxt[cur], cur)
    if (cur != idx).any():
        raise _lib.NanoCallerHipError("indel_mate_table: a read name with more than %d kept alignments (the first: alignment %d of the kept ones)"
                                      % (MATE_RING_CAP, int(r[int(np.flatnonzero(cur != idx)[0])])), status=_lib.NC_ERR_UNSUPPORTED)
    bits = np.zeros(M, np.int32)
    np.bitwise_or.at(bits, g, np.where((hap == 1) | (hap == 2), 1 << (hap - 1).clip(0, 1), 0).astype(np.int32))
    last = np.zeros(M, np.int64)
    np.maximum.at(last, g, idx)
    rec = np.zeros((M, 8), np.int32)
    rec[:, :3] = rec4[:, :3]
    rec[:, 3] = r.cpu().numpy()
    rec[:, 4] = bits[g]
    rec[:, 5] = np.where(hap[last[g]] != 0, ps[last[g]], 0)
    return key.contiguous(), torch.from_numpy(rec).to(key.device)


_DEV_INGEST = {}              # one contig at a time: (BAM, contig, FASTA, flag filter, device, by name or not, file identity) -> (pack, nc_indel_reads, contig dict, indel_mate_table or None)


def ingest_contig(dct, sam_path, chrom, supp, device, by_name=False):
    """The contig's read pack WITH the indel sections, made on the device from the BAM file itself (device_bam.py: inflate, record walk, codes,
    events, inserted bases and tails in HBM) -- what decoded_contig + device_pack + device_indel_reads assemble on host threads.  None when the
    input cannot take that route (no .bai and no dct['build_index'] / NC_BUILD_INDEX=1 to make one, too large, NC_DEVICE_INGEST=0 / dct['device_ingest'] = False): the host route follows."""
    if not dct.get("device_ingest", os.environ.get("NC_DEVICE_INGEST", "1") != "0") or not isinstance(sam_path, str) or not os.path.exists(sam_path):
        return None
    st = os.stat(sam_path)
    key = (sam_path, chrom, dct["fasta_path"], supp, device, bool(by_name), st.st_size, st.st_mtime_ns)
    if key not in _DEV_INGEST:
        from .device_bam import DeviceIngestUnavailable, ensure_index, open_device_bam
        from .device_fasta import reference_for
        from .wire import indel_reads_struct
        _DEV_INGEST.clear()
        ensure_index(sam_path, dct, device)                              # (dct['build_index'] / NC_BUILD_INDEX=1: a BAM without index gets one)
        try:
            dbam = open_device_bam(sam_path, device, contigs=[chrom])
        except DeviceIngestUnavailable:
            return None
        # the letters as bytes, or (a bgzipped FASTA; a plain one with dct['device_fasta'] / NC_DEVICE_FASTA=1) the contig in HBM: the pack's
        # reference codes come from there, and the host's copy of the letters -- the windows' reference text -- is one D2H
        ref = reference_for(dct["fasta_path"], chrom, device, dct)
        dp = dbam.pack(dbam.prepare(chrom, ref, supplementary=supp, haplotags=getattr(sam_path, "tags", None), by_name=bool(by_name)), indel=True,
                       tail_cap=TAIL_CAP)
        ref_contig = ref if hasattr(ref, "scan_codes") else None
        if ref_contig is not None:
            try:
                fasta_b = ref_contig.host_letters()
            except DeviceIngestUnavailable:
                from .bam import read_fasta_bytes
                fasta_b, ref_contig = read_fasta_bytes(dct["fasta_path"], chrom), None
        else:
            fasta_b = ref
        _DEV_INGEST[key] = (dp, indel_reads_struct(dp), dict(fasta=fasta_b.decode("ascii"), fasta_b=fasta_b, device_ingest=True, ref_contig=ref_contig),
                            indel_mate_table(dp, dp.indel["read_ps"]) if by_name else None)
    return _DEV_INGEST[key]


def indel_pack_for(dct, chunks, device, by_name=False):
    """(engine, read pack with the indel sections, nc_indel_reads struct, contig dict, exclusion mask or None, table of shared names or None) of the
    chunks' BAM and contig: made on the device from the BAM file itself where that route is open (ingest_contig), else from the host decode.
    by_name (the device pipeline without impute_indel_phase): kept alignments that share a read name are not refused, and the last item is their
    table for nc_indel_set_mates (None without by_name or when no name is shared).  The device-ingested packs of the two settings are cached apart;
    the host decode's pack is one and the same (it always carries bit 3 and the name rings: by_name only lifts the refusal)."""
    chrom, sam_path = chunks[0]["chrom"], chunks[0]["sam_path"]
    supp = bool(dct.get("supplementary"))
    eng = get_engine(device)
    eng.use_torch_stream()
    di = ingest_contig(dct, sam_path, chrom, supp, device, by_name)
    if di is not None:
        dp, reads_c, ctg, mates = di
    else:
        from .generate_indel_pileups import contig_keep, decoded_contig
        ctg = decoded_contig(sam_path, chrom, dct["fasta_path"])
        flag = keep_flag(dct)
        contig_keep(ctg, flag)
        dp = device_pack(sam_path, dct.get("fasta_path"), chrom, supp, None, device, by_name=by_name)[0]
        reads_c = device_indel_reads(ctg, flag, dp, device)
        mates = None
        if by_name and getattr(dp, "mates", None) is not None:
            mk = ("dev_mates", flag, device)
            if mk not in ctg or ctg[mk][0] is not dp:
                ctg[mk] = (dp, indel_mate_table(dp, ctg[("dev_reads", flag, device)][1]["read_ps"]))
            mates = ctg[mk][1]
    return eng, dp, reads_c, ctg, exclusion_mask(dct, chrom, dp), mates


def imputed_chunk_mask(dct, chunks, device):
    """impute_indel_phase (generate_indel_pileups.py:278-304) on the device pipeline: which chunks hold a column that meets the rule's COLUMN-level
    predicate (:278-284; K7's col_type 2 on the resident pack).  A chunk without one takes no imputed anchor, and its `variants` are those of the flag
    off -- it runs on the device pipeline; the others (their read grouping needs the pileup strings, :285-304) take the host-assembled route."""
    eng, dp, _, _, excl, _ = indel_pack_for(dct, chunks, device)
    cols = eng.indel_scan_batch(dp, [(c["start"], c["end"]) for c in chunks], mincov=dct["mincov"], win_size=dct["win_size"],
                                small_win_size=dct["small_win_size"], ins_t=dct["ins_t"], del_t=dct["del_t"], excl=excl, haploid=False, impute=True)
    return [bool((ct == 2).any()) for ct in cols]


def device_part(fn, *args):
    """fn(*args) for a "device" part of generate_indel_pileups.plan_routes' plan, or None when the device pipeline met one of its capacity limits
    (sets of > 1024 alignment columns, chunks of > 130 kb, a pack without indel sections): the caller then redoes the part on the host-assembled
    route, and on that route only"""
    try:
        return fn(*args)
    except _lib.NanoCallerHipError as e:
        if e.status != _lib.NC_ERR_CAPACITY:
            raise
        return None


def sites_to_vcf_text(eng, r, probs, chrom, n_chunks, ctg, haploid):
    """the VCF record text of the device pipeline's sites `r` with their model probabilities, by the native genotype rules (nc_indel_vcf_format:
    no Python object per site) -> list of bytes, the records of each of the result's chunks"""
    N, S = r["n"], r["sets"]
    chrom = chrom.encode()
    cap = int(N) * (96 + len(chrom)) + 2 * int(np.maximum(r["ref_len"], 0).sum() + np.maximum(r["alt_len"], 0).sum()) * 2 + 4096
    buf = np.empty(cap, np.uint8)
    nb = C.c_int64()
    coff = np.empty(n_chunks + 1, np.int64)
    pos, chunk, phase = (np.ascontiguousarray(r[k], np.int32) for k in ("pos", "chunk", "phase"))
    rl, al = np.ascontiguousarray(r["ref_len"], np.int32), np.ascontiguousarray(r["alt_len"], np.int32)
    rc = eng.L.nc_indel_vcf_format(chrom, N, _lib.npp(pos), _lib.npp(chunk), n_chunks, _lib.npp(np.ascontiguousarray(probs, np.float32)), S,
                                   _lib.npp(rl), _lib.npp(al), _lib.npp(np.ascontiguousarray(r["alt"], np.uint8)), _lib.npp(phase), ctg["fasta_b"],
                                   len(ctg["fasta"]), 1 if haploid else 0, _lib.npp(buf), cap, C.byref(nb), _lib.npp(coff))
    if rc != _lib.NC_OK:
        raise _lib.NanoCallerHipError("nc_indel_vcf_format failed (%d)" % rc, status=rc)
    raw = buf[:nb.value].tobytes()
    co = coff.tolist()
    texts = [raw[a:b] for a, b in zip(co, co[1:])]
    if "src" in r:
        texts = _with_reference_calls(r, probs, chrom, texts, ctg, haploid)
    return texts


def reference_call_line(chrom, p, ref_base, prob, haploid):
    """The line of a listed indel column `p` whose site got no variant record: the model calls reference (diploid prob[0] > 0.95, haploid
    prob < 0.5: FILTER REF, Q = min(99, -10 log10(1e-6 + the probability of a variant))) or no allele was found (LOW, Q 0.00).  chrom: bytes."""
    if haploid:
        pv = float(np.asarray(prob).reshape(-1)[0])
        is_ref, q = pv < 0.5, pv
    else:
        p0 = float(np.asarray(prob).reshape(-1)[0])
        is_ref, q = p0 > 0.95, 1.0 - p0
    qv = min(99.0, -10.0 * float(np.log10(1e-6 + q))) if is_ref else 0.0
    return b"%s\t%d\t.\t%s\t.\t%.2f\t%s\t.\tGT:GQ\t./.:%.2f\n" % (chrom, p, ref_base, qv, b"REF" if is_ref else b"LOW", qv)


def _with_reference_calls(r, probs, chrom, texts, ctg, haploid):
    """nc_indel_vcf_format's text of every chunk + one reference_call_line per site whose anchor a listed column wrote (r['src'] > 0) and that got
    no record, merged by position.  A forced site the rules skipped by `pos <= prev` lies inside the previous record: no line, counted
    (r['genotype_inside']).  The lines never move the rules' `prev`: the rules ran before them.  Sets r['genotype_recorded']."""
    pos, chunk, src = r["pos"].tolist(), r["chunk"].tolist(), r["src"].tolist()
    fasta_b = ctg["fasta_b"]
    recorded, inside = set(), 0
    out = []
    k = 0
    for ci, text in enumerate(texts):
        lines = text.splitlines(keepends=True)
        rec = {}                                                     # a record's POS -> the `prev` it leaves: POS + its longest allele
        for ln in lines:
            f = ln.split(b"\t", 5)
            rec[int(f[1])] = int(f[1]) + max(len(f[3]), max(len(a) for a in f[4].split(b",")))
        extra, prev = [], 0
        while k < len(pos) and chunk[k] == ci:
            pj, sj = pos[k], src[k]
            if not pj > prev:
                inside += sj > 0
            elif pj in rec:
                prev = rec[pj]
                if sj > 0:
                    recorded.add((ci, sj))
            elif sj > 0:
                extra.append((sj, reference_call_line(chrom, sj, fasta_b[sj - 1:sj].upper(), probs[k], haploid)))
                recorded.add((ci, sj))
            k += 1
        if extra:
            keyed = [(int(ln.split(b"\t", 2)[1]), 0, i, ln) for i, ln in enumerate(lines)] + [(p, 1, i, ln) for i, (p, ln) in enumerate(extra)]
            text = b"".join(t[3] for t in sorted(keyed))
        out.append(text)
    r["genotype_recorded"] = len({s for _, s in recorded})
    r["genotype_inside"] = inside
    return out


def sites_to_tuples(r, n_chunks, fasta, haploid, device_x):
    """the per-chunk tuples get_indel_testing_candidates[_haploid] returns, from the arrays of the device pipeline"""
    N, S = r["n"], r["sets"]
    empty = ([], [], []) if haploid else ([], [], [], [], [], [])
    if N == 0:
        return [empty for _ in range(n_chunks)]
    x = r["x"] if device_x else r["x"].cpu().numpy().astype(np.float64)
    pos, chunk = r["pos"].tolist(), r["chunk"]
    rl, al = r["ref_len"].reshape(-1).tolist(), r["alt_len"].reshape(-1).tolist()
    alt_all = np.frombuffer(b"AGTCN", np.uint8)[r["alt"]].tobytes().decode("ascii")
    alleles, o = [], 0
    for k in range(N):
        p, row = pos[k], []
        for t in range(S):
            a, b = rl[k * S + t], al[k * S + t]
            if a < 0:
                row.append((None, None))
            else:
                row.append((fasta[p - 1:p - 1 + a], alt_all[o:o + b]))
            o += max(b, 0)
        alleles.append(row)
    phase = [v if v else None for v in r["phase"].tolist()]          # PS of set 0's first read; a read without the tag (imputed sets): None (:181-183,349)
    bounds = np.searchsorted(chunk, np.arange(n_chunks + 1))                       # sites are chunk-major
    out = []
    for ci in range(n_chunks):
        a, b = int(bounds[ci]), int(bounds[ci + 1])
        if a == b:
            out.append(empty)
        elif haploid:
            out.append((pos[a:b], x[a:b], [alleles[k][0] for k in range(a, b)]))
        else:
            out.append((pos[a:b], x[a:b, 0:5], x[a:b, 5:10], x[a:b, 10:15], alleles[a:b], phase[a:b]))
    return out

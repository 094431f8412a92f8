"""Host-side mirror of the reference's SNP caller (nanocaller_src/snpCaller.py).

Same entry points, `params` keys, model names, VCF text and output file names; the featurisation and
the CNN run on the MI355X through libnanocaller_hip.so.  Differences by design:

* one process per GPU instead of `cpu` worker processes; a worker takes ALL chunks of a contig as one
  device batch (the contig's alignments stay resident in HBM, scanned once);
* genotype rules (snpCaller.py:113-198) stay on the host: `snp_vcf_lines` / `snp_vcf_lines_haploid`;
* bcftools/bgzip are optional: records are written position-sorted and BGZF-compressed natively.
"""
from __future__ import annotations

import datetime
import os
import queue
import shutil
import struct
import sys
import zlib

import numpy as np
import torch

from . import _lib
from .engine import get_engine
from .generate_SNP_pileups import device_pack_for, release_contig
from .weights import Weights, get_haploid_SNP_model, get_SNP_model  # noqa: F401  (re-exported, same name as the reference)

num_to_base_map = {0: 'A', 1: 'G', 2: 'T', 3: 'C'}                 # snpCaller.py:14
_B = "AGTC"


def _qual(p, cap=99.0, mult=-10.0):
    """min(cap, mult*log10(1e-10 + 1 - p)) evaluated in float64 (numpy<2 scalar semantics)."""
    return min(cap, mult * np.log10(1e-10 + 1 - float(p)))


def snp_vcf_lines(chrom, pos, ref_idx, probs, dp, freq, fwd_dp, rev_dp):
    """Diploid genotype rules + VCF text (snpCaller.py:113-163).
    probs float32 [N,4] = class-1 probability of the A,G,T,C heads."""
    probs = np.asarray(probs, np.float32)
    order = np.argsort(probs, axis=1)                               # :118 (same call => same tie behaviour)
    k = np.sum(probs >= 0.5, axis=1)                                # :122
    out = []
    for j in range(len(pos)):
        pr = probs[j]
        info = 'PR=' + ','.join("{:.4f}".format(x) for x in pr[[0, 3, 1, 2]]) + ";FQ={:.4f}".format(freq[j])   # :127
        r = int(ref_idx[j])
        d = int(dp[j])
        ref_dp = (fwd_dp[j][r], rev_dp[j][r])
        p1, p2 = int(order[j, -1]), int(order[j, -2])
        head = '%s\t%d\t.\t%s\t' % (chrom, pos[j], _B[r])
        fmt = 'GT:DP:VF:AD:ADF:ADR'
        if k[j] >= 2:
            if p1 == r:                                             # :132
                a = (fwd_dp[j][p2], rev_dp[j][p2])
                out.append(head + '%s\t%.3f\t%s\t%s\t%s\t%s:%d:%.4f:%d,%d:%d,%d:%d,%d\n' % (
                    _B[p2], _qual(pr[p2]), 'PASS', info, fmt, '0/1', d, sum(a) / d, sum(ref_dp), sum(a), ref_dp[0], a[0],
                    ref_dp[1], a[1]))
            elif p2 == r and pr[p2] >= 0.5:                         # :138
                a = (fwd_dp[j][p1], rev_dp[j][p1])
                out.append(head + '%s\t%.3f\t%s\t%s\t%s\t%s:%d:%.4f:%d,%d:%d,%d:%d,%d\n' % (
                    _B[p1], _qual(pr[p2]), 'PASS', info, fmt, '0/1', d, sum(a) / d, sum(ref_dp), sum(a), ref_dp[0], a[0],
                    ref_dp[1], a[1]))
            elif p2 != r and p1 != r and pr[p2] >= 0.5:             # :143
                a1 = (fwd_dp[j][p1], rev_dp[j][p1])
                a2 = (fwd_dp[j][p2], rev_dp[j][p2])
                out.append(head + '%s,%s\t%.3f\t%s\t%s\t%s\t%s:%d:%.4f,%.4f:%d,%d,%d:%d,%d,%d:%d,%d,%d\n' % (
                    _B[p1], _B[p2], _qual(pr[p2]), 'PASS', info, fmt, '1/2', d, sum(a1) / d, sum(a2) / d, sum(ref_dp),
                    sum(a1), sum(a2), ref_dp[0], a1[0], a2[0], ref_dp[1], a1[1], a2[1]))
            # else: the reference writes nothing (k>=2 but the second allele is below 0.5 cannot happen)
        elif k[j] == 1 and r != p1 and pr[p1] >= 0.5:               # :150
            a = (fwd_dp[j][p1], rev_dp[j][p1])
            out.append(head + '%s\t%.3f\t%s\t%s\t%s\t%s:%d:%.4f:%d,%d:%d,%d:%d,%d\n' % (
                _B[p1], _qual(pr[p1]), 'PASS', info, fmt, '1/1', d, sum(a) / d, sum(ref_dp), sum(a), ref_dp[0], a[0],
                ref_dp[1], a[1]))
        elif k[j] == 1 and r == p1:                                 # :157
            out.append(head + '%s\t%.3f\t%s\t%s\t%s\t%s:%d:.:.:.:.\n' % ('.', _qual(pr[p1]), 'REF', info, fmt, './.', d))
        else:                                                       # :161
            out.append(head + '%s\t%.3f\t%s\t%s\t%s\t%s:%d:.:.:.:.\n' % ('.', 0, 'LOW', info, fmt, './.', d))
    return out


def snp_vcf_lines_haploid(chrom, pos, ref_idx, probs, dp, freq):
    """Haploid rules (snpCaller.py:184-198): arg-max of the 4-way softmax, PASS if it differs from ref."""
    probs = np.asarray(probs, np.float32)
    pred = np.argmax(probs, 1)
    out = []
    for j in range(len(pos)):
        pr = probs[j]
        p = int(pred[j])
        r = int(ref_idx[j])
        info = 'PR=' + ','.join("{:.4f}".format(x) for x in pr[[0, 3, 1, 2]]) + ";FQ={:.4f}".format(freq[j])
        out.append('%s\t%d\t.\t%s\t%s\t%.3f\t%s\t%s\tGT:DP:VF:AD:ADF:ADR\t%s:%d:%.4f:.:.:.\n' % (
            chrom, pos[j], _B[r], _B[p], _qual(pr[p], 999.0, -100.0), 'PASS' if p != r else 'REF', info, '1/1', int(dp[j]),
            freq[j]))
    return out


def argsort4(probs):
    """np.argsort(probs, axis=1) for [n, 4] float32 rows: the library sorts (threaded), numpy re-sorts only the rows that
    contain ties, so the result equals numpy's on this machine element for element (quirk E15)."""
    import ctypes as C
    L = _lib.lib()
    probs = np.ascontiguousarray(probs, np.float32)
    n = probs.shape[0]
    order = np.empty((n, 4), np.int32)
    ties = np.empty(max(n, 1), np.int64)
    nt = C.c_int64()
    rc = L.nc_argsort4(_lib.npp(probs), n, _lib.npp(order), C.byref(nt), _lib.npp(ties), ties.size)
    if rc != _lib.NC_OK:
        raise _lib.NanoCallerHipError("nc_argsort4 failed (%d)" % rc)
    if nt.value:
        t = ties[:nt.value]
        order[t] = np.argsort(probs[t], axis=1)
    return order


def snp_vcf_text(chrom, pos, ref_idx, probs, dp, freq, fwd_dp=None, rev_dp=None, haploid=False, as_array=False, out=None):
    """Same records as snp_vcf_lines / snp_vcf_lines_haploid, formatted by the library's native formatter
    (nc_snp_vcf_format); ties in the allele order resolve exactly as in the Python path (argsort4, E15).
    -> bytes, or with as_array=True a uint8 array (buffer protocol: file.write() takes it without another copy).
    `out`: optional uint8 scratch array to format into (reused by callers that write the text out immediately: saves the
    page faults of a fresh 400 B/record buffer per call)."""
    import ctypes as C
    L = _lib.lib()
    n = len(pos)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)          # noqa: E731
    probs = np.ascontiguousarray(probs, np.float32)
    order = None if haploid else argsort4(probs)
    pos_, ref_, dp_ = i32(pos), i32(ref_idx), i32(dp)
    freq_ = np.ascontiguousarray(freq, np.float64)
    fwd_ = None if haploid else i32(fwd_dp)
    rev_ = None if haploid else i32(rev_dp)
    cap = (400 + len(chrom)) * max(n, 1) + 1024
    if out is None or out.size < cap:
        out = np.empty(cap, np.uint8)
    cap = out.size
    nb = C.c_int64()
    rc = L.nc_snp_vcf_format(chrom.encode(), n, _lib.npp(pos_), _lib.npp(ref_), _lib.npp(probs), _lib.npp(order),
                             _lib.npp(dp_), _lib.npp(freq_), _lib.npp(fwd_), _lib.npp(rev_), 1 if haploid else 0,
                             _lib.npp(out), cap, C.byref(nb))
    if rc != _lib.NC_OK:
        raise _lib.NanoCallerHipError("nc_snp_vcf_format failed (%d)" % rc)
    return out[:nb.value] if as_array else out[:nb.value].tobytes()


VCF_HEADER = (                                                      # snpCaller.py:259-276
    '##fileformat=VCFv4.2\n'
    '##FILTER=<ID=PASS,Description="All filters passed">\n'
    '##FILTER=<ID=LOW,Description="All alleles have probability less than 50%.">\n'
    '##FILTER=<ID=REF,Description="Homozygous Reference. Only reference allele has greater than 50% probability. '
    'All alternative alleles having probability less than 50%.">\n'
    '{contigs}'
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth">\n'
    '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Allelic depths for the ref and alt alleles in the order listed">\n'
    '##FORMAT=<ID=ADF,Number=R,Type=Integer,Description="Allelic depths on forward strand for the ref and alt alleles in the order listed">\n'
    '##FORMAT=<ID=ADR,Number=R,Type=Integer,Description="Allelic depths on reverse strand for the ref and alt alleles in the order listed">\n'
    '##FORMAT=<ID=VF,Number=A,Type=Float,Description="Alternative allele frequency in the order listed">\n'
    '##INFO=<ID=PR,Number=4,Type=Float,Description="Probability of presence of alleles A, C, G and T, in the given order. '
    'Probability of each base is out of 1, independent of each other.">\n'
    '##INFO=<ID=FQ,Number=1,Type=Float,Description="Maximum frequency of non-reference base.">\n'
    '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}\n')


# keys of the `params` dict this module reads (all of them are in the dict NanoCaller:28-35 builds)
# (opt-in keys of this project that the reference's dict does not have are read with .get and are not listed: 'genotype_sites',
# 'genotype_only', 'neighbor_sites', 'neighbor_only', 'haploid_snp_model', 'gvcf', 'gvcf_error', 'gvcf_gq_bands', 'gvcf_writer'; tests/test_boundary.py holds this set
# to the reference's keys)
PARAM_KEYS = frozenset(['chunks_list', 'regions_list', 'sam_path', 'fasta_path', 'mincov', 'maxcov', 'min_allele_freq', 'min_nbr_sites',
                        'threshold', 'snp_model', 'vcf_path', 'prefix', 'sample', 'seq', 'supplementary', 'exclude_bed',
                        'suppress_progress', 'disable_coverage_normalization'])

_WEIGHTS = {}


def _weights(path):
    """parsed .ncw files, cached per path"""
    if path not in _WEIGHTS:
        _WEIGHTS[path] = Weights(path)
    return _WEIGHTS[path]


class PendingCall:
    """call_chunks(defer=True): everything is enqueued, the result copies may still be in flight; result() waits for them."""

    def __init__(self, finish):
        self._finish, self._res = finish, None

    def result(self):
        if self._finish is not None:
            self._res, self._finish = self._finish(), None
        return self._res


def call_chunks(params, chunks, device=0, dpk=None, defer=False, pipeline=None):
    """Run pileup featurisation + CNN for a list of chunks of ONE contig and ploidy on the GPU.
    `dpk`: alignments already resident in HBM (engine.DevicePack); default: packed from params['sam_path'].
    -> dict of host arrays (pos, chunk, ref, probs, gt, dp, freq, fwd_dp, rev_dp, chunk_depth).
    params['genotype_sites'] / params['genotype_only'] (genotype_sites.py; both optional): positions to genotype whatever their allele
    frequency; the result then counts them: genotype_listed = listed positions inside these chunks, genotype_emitted = those with a record.
    params['neighbor_sites'] / params['neighbor_only'] (genotype_sites.neighbor_sites_for; both optional): known heterozygous sites that are
    neighbour sites whatever their allele frequency, beside the frequency rule or instead of it.
    params['haploid_snp_model'] (optional; else NC_HAPLOID_SNP_MODEL): 'haploid' or an .ncw of kind KIND_SNP_HAP for haploid chunks; a file brings
    its own train_coverage for the coverage scale (weights.get_haploid_SNP_model; a missing file or another kind raises).
    params['downsample'] / params['downsample_seed'] (optional; else NC_DOWNSAMPLE / NC_DOWNSAMPLE_SEED; downsample.py): 'first' (the default) or
    'uniform' -- which reads a pileup deeper than maxcov keeps: the first maxcov in pileup order, or a seeded uniform sample (seed 812 unless given).
    Any other value raises ValueError, and so does 'uniform' on a contig whose kept alignments share read names.
    params['gvcf'] (optional; else NC_GVCF=1; gvcf.py): the result then carries 'gvcf', the per-column counts of the group's pack on the device
    (Engine.refconf_columns), from which caller() makes the reference-confidence blocks once the group's records are known.
    defer=True -> PendingCall: returns once the group's work is handed over; the caller starts the next group and collects result() afterwards.
    pipeline: None or False.  True asked for a removed path (a group's CNN enqueued inside the next call's scan; measured slower, 10.55 ->
    11.2 ms per contig: profiles/README.md, round 6) and raises."""
    if pipeline:
        raise ValueError("call_chunks(pipeline=True): the pipelined-CNN path (NC_PIPE_CNN=1) was removed")
    chrom = chunks[0]['chrom']
    ploidy = chunks[0]['ploidy']
    assert all(c['chrom'] == chrom and c['ploidy'] == ploidy for c in chunks)
    from .downsample import for_pack, resolve
    resolve(params)                                                  # (a bad value raises before any work)
    eng = get_engine(device)
    eng.use_torch_stream()
    if ploidy == 'diploid':
        path, train_cov = get_SNP_model(params['snp_model'])
        if path is None:
            print('Invalid SNP model name or path', flush=True)     # snpCaller.py:66-68
            sys.exit(1)
        kind = _lib.MODEL_SNP
    else:
        # the shipped CHM13 model with hap_train_coverage = 30 (snpCaller.py:73) unless params['haploid_snp_model'] names a trained file
        path, train_cov = get_haploid_SNP_model(params)
        kind = _lib.MODEL_SNP_HAP
    eng.load_weights(kind, _weights(path))
    if dpk is None:
        # a rank that owns only part of a contig (shard.shard_plan) decodes and uploads only its span +- the scan flank
        from .generate_SNP_pileups import contig_span
        dpk = device_pack_for(params, chrom, device, span=contig_span(params['sam_path'], chrom, chunks))
    # Results drain on a second stream while the GPU keeps computing: the candidate arrays right after the scan, the
    # featuriser's per-site arrays during the CNN, and every CNN batch's probabilities while the next batch runs.
    down = for_pack(params, dpk.mates, chrom)
    from .genotype_sites import count_listed, neighbor_sites_for, sites_for
    listed, only = sites_for(params, chrom)
    nbr_listed, nbr_only = neighbor_sites_for(params, chrom)
    spans = [(c['start'], c['end']) for c in chunks]
    sites = eng.snp_scan(dpk, spans, mincov=params['mincov'],
                         min_allele_freq=params['min_allele_freq'], threshold=params['threshold'],
                         haploid=(ploidy == 'haploid'), async_fetch=True, sites=listed, sites_only=only,
                         nbr_sites=nbr_listed, nbr_only=nbr_only)
    res = dict(chrom=chrom, ploidy=ploidy, n=0, genotype_listed=count_listed(listed, spans, ())[0], genotype_emitted=0)
    from . import gvcf
    if gvcf.enabled(params):
        # the per-column counts of the gVCF's reference-confidence blocks, behind the scan while the pack is resident (4 B per column, held until
        # the group's records are collected: gvcf.group_blocks)
        res['gvcf'] = eng.refconf_columns(dpk)
    if sites.n_sites == 0:
        eng.wait_copies()
        return PendingCall(lambda: res) if defer else res
    # the tensors stay on the device: int16 between featuriser and CNN (exact, half the HBM traffic) unless the exact-fp32
    # trunk, which reads the reference's float32 layout, has been selected
    exact = eng.exact_fp32
    eng.snp_featurize(dpk, sites, seq=params['seq'], maxcov=params['maxcov'], min_nbr_sites=params['min_nbr_sites'], int16=not exact, downsample=down)
    # default 1 never filters (:244), unless the neighbours come from a list alone (it then counts them, not the site's own column)
    all_valid = bool(sites.valid.all().item()) if params['min_nbr_sites'] > 1 or sites.nbr_only else True
    per_site = bool(params.get('disable_coverage_normalization'))
    scale, chunk_depth = eng.snp_scale(sites, len(chunks), train_cov, per_site=per_site, async_fetch=True)
    scan_copied = eng.copy_event()                                 # candidate arrays + chunk depths are on the host behind this
    # enqueued after the (short, latency-sensitive) scale kernel so that these copies run under the CNN, not beside it
    h_ref, h_fwd, h_rev, h_valid = eng.to_host_async([sites.ref_code, sites.fwd_dp, sites.rev_dp, None if all_valid else sites.valid])
    # range guard of the split-precision trunk (nc_cnn_range_watch): sites whose scaled tensor exceeds what the model's weights prove
    # safe for the fp16 range are marked and, in finish(), computed once more by the exact fp32 trunk
    flags = None if exact else torch.zeros(sites.n_sites, dtype=torch.uint8, device=eng.device)
    d_probs, d_gt, h_probs, h_gt = eng.snp_forward(kind, sites.x, sites.ref_code, scale, scale_mode=1 if per_site else 0, drain=True, range_flags=flags)
    h_nflag = None if exact else eng.to_host_async([flags.sum(dtype=torch.int32).reshape(1)])[0]
    drained = eng.copy_event()                                     # completes with this call's last result copy
    # host work that only needs the scan results runs under the CNN: freq = alt / n in float64 (:166)
    scan_copied.synchronize()
    freq = sites.alt.astype(np.float64) / sites.dp.astype(np.float64)

    def finish():
        drained.synchronize()
        n_rerun = int(h_nflag[0]) if h_nflag is not None else 0
        if n_rerun:
            idx = torch.nonzero(flags).squeeze(1)
            eng.use_torch_stream()
            eng.range_rerun(kind, sites.x, sites.ref_code, scale, 1 if per_site else 0, idx, d_probs, d_gt)
            ih = idx.cpu().numpy()
            h_probs[ih] = d_probs[idx].cpu().numpy()
            if h_gt is not None and d_gt is not None:
                h_gt[ih] = d_gt[idx].cpu().numpy()
        res['range_reruns'] = n_rerun
        out = dict(pos=sites.pos, chunk=sites.chunk, ref=h_ref, probs=h_probs, gt=h_gt, dp=sites.dp, alt=sites.alt,
                   fwd_dp=h_fwd, rev_dp=h_rev, freq=freq)
        if not all_valid:
            m = h_valid.astype(bool)
            out = {k: (v[m] if v is not None else None) for k, v in out.items()}
        # host arrays keep the device dtypes (int32 / float32)
        res.update(out, n=int(out['pos'].shape[0]), chunk_depth=chunk_depth)
        res['genotype_listed'], res['genotype_emitted'] = count_listed(listed, spans, out['pos'])
        return res
    return PendingCall(finish) if defer else finish()


def _prepare_wire(params, chrom, grp):
    """host half of a group's ingest, on a worker thread: decode the contig (or this rank's span of it) and build its wire pack
    in page-locked memory (what device_pack() does synchronously)"""
    from .generate_SNP_pileups import _check_supported, _exclude_rows, _resolve, contig_span
    from .wire import build_wire_from_world
    span = contig_span(params['sam_path'], chrom, grp)
    world = _resolve(params['sam_path'], chrom, params.get('fasta_path'), span)
    _check_supported(world, params['sam_path'], chrom, bool(params.get('supplementary')), by_name=True)
    kw = dict(pos_lo=span[0], pos_hi=span[1]) if span else {}
    return build_wire_from_world(world, supplementary=bool(params.get('supplementary')), exclude=_exclude_rows(params, chrom), **kw)


def _prepare_device(dbam, params, chrom, grp, ref=None):
    """host half of a group's ingest on the device route (device_bam.py), on a worker thread: the contig's reference sequence, which of its
    alignments the pileup keeps, the tile index -- from the per-record fields the device extracted when the file was loaded.  Alignments that
    share a read name are keyed by name (by_name=True: when name hashes repeat, one small launch on the context's own stream confirms the names)"""
    from .device_fasta import reference_for
    from .generate_SNP_pileups import _exclude_rows, span_of
    # (contig_span's rule, on the lengths the loader already holds: no second open of the BAM)
    span = span_of(grp, dbam.ref_lengths[dbam.ref_names.index(chrom)] if chrom in dbam.ref_names else 0)
    # (the letters as bytes, or -- a bgzipped FASTA, or a plain one with params['device_fasta'] / NC_DEVICE_FASTA=1 -- the contig on its way to HBM)
    ref = ref.result() if ref is not None else reference_for(params['fasta_path'], chrom, dbam.device, params)
    return dbam.prepare(chrom, ref, supplementary=bool(params.get('supplementary')), exclude=_exclude_rows(params, chrom), span=span, by_name=True)


def _plan_runs(params, keys, device):
    """-> (run_end, run_dev), per group of `keys` [(contig, ploidy)]: where its run of groups ends, and the run's contigs (None: host route).
    A file larger than HBM takes passes share by share: runs of contigs whose part of the file fits (device_bam.plan_shares;
    NC_DEVICE_INGEST_SHARE_GB of compressed BAM, default 12); a contig that alone does not fit is decoded by the host threads.  Where the
    device route cannot be taken at all, one run on the host route."""
    from .device_bam import DeviceIngestUnavailable, plan_shares
    run_end, run_dev = [len(keys)] * len(keys), [None] * len(keys)
    try:
        lim = os.environ.get('NC_DEVICE_INGEST_SHARE_GB')
        order = list(dict.fromkeys(k[0] for k in keys))
        share_of = {}
        for n_sh, (cs, fits) in enumerate(plan_shares(params['sam_path'], order, None if lim is None else int(float(lim) * (1 << 30)), device=device)):
            for c in cs:
                share_of[c] = (n_sh, tuple(cs) if fits else None)
        a0 = 0
        for j in range(1, len(keys) + 1):
            if j == len(keys) or share_of[keys[j][0]][0] != share_of[keys[a0][0]][0]:
                for q in range(a0, j):
                    run_end[q], run_dev[q] = j, share_of[keys[a0][0]][1]
                a0 = j
    except DeviceIngestUnavailable:
        pass
    return run_end, run_dev


class _Ingest:
    """Ingest pipeline of caller() (what bench.py's timed region does with its uploads): while the GPU runs group i, a host thread decodes the
    BAM records of group i + 1's contig and puts them into the reference-difference wire form (native code, the GIL is released); that pack
    then crosses PCIe on the upload stream through a ring of three device slots, under group i's kernels.
    Device route (device_bam.py; NC_DEVICE_INGEST=0 or params['device_ingest'] = False keeps the host threads' decode): the FILE crosses
    PCIe, is inflated and cut into records in HBM, and every group's pack is decoded there from the record stream; the worker threads only
    decide which alignments are kept and build the tile index.  Needs the .bai (_plan_runs: which groups take it).
    (alignments that share a read name -- a split read's records under dct['supplementary'], paired mates -- are keyed by NAME on both routes:
    pack.name_groups, fed by nc_decoded_name_groups on the host route and by nc_bam_name_groups on the device route)"""

    def __init__(self, params, keys, groups, device):
        from concurrent.futures import ThreadPoolExecutor
        self.params, self.keys, self.groups, self.device = params, keys, groups, device
        self.run_end, self.run_dev = [len(keys)] * len(keys), [None] * len(keys)
        if params.get('device_ingest', os.environ.get('NC_DEVICE_INGEST', '1') != '0') and params.get('fasta_path'):
            from .device_bam import ensure_index
            ensure_index(params['sam_path'], params, device)             # (params['build_index'] / NC_BUILD_INDEX=1: a BAM without index gets one)
            self.run_end, self.run_dev = _plan_runs(params, keys, device)
        # two groups ahead: the Python half of one pack's preparation (header parsing, the wire's index arrays, freeing the decoded
        # arrays: ~35 of ~58 ms per 3 Mb contig) runs beside the native decode of the next one, which releases the GIL
        self.ahead = max(1, int(os.environ.get('NC_INGEST_AHEAD', 2)))
        self.pool = ThreadPoolExecutor(max_workers=self.ahead)
        self.dbam = self.prepare = self.uploader = self.codes = None
        self.preps, self.refs, self.nxt = [], {}, 0                  # the next groups' packs, being prepared; reference letters on their way

    def _prepare_next(self, run_end):
        if self.nxt < run_end:
            k = self.keys[self.nxt]
            self.preps.append(self.pool.submit(self.prepare, k[0], self.groups[k]))
            self.nxt += 1

    def enter_run(self, i):
        """group i opens a run: the device route loads the run's share of the file (the previous share is dropped), the host route needs
        nothing; then the first preparations of the run are started"""
        from concurrent.futures import ThreadPoolExecutor
        from .device_bam import DeviceIngestUnavailable, open_device_bam, release as release_device_bam
        from .device_fasta import reference_for
        params, device, refs = self.params, self.device, self.refs
        # the previous share goes first: its DeviceBam is still referenced by the old `prepare` closure, and while it lives its stream buffer
        # cannot be re-used -- a second one next to it is ~2 x 108 GB for a genome-sized file (more than the card holds)
        self.dbam = self.prepare = None
        if i > 0 and self.run_dev[i - 1] is not None:
            get_engine(device).sync()
            release_device_bam(params['sam_path'])
        if self.run_dev[i] is not None:
            # the first contigs' reference letters are read while the file is loaded (the loader mostly waits: for its reader threads, for the GPU);
            # on the device route of the FASTA (device_fasta.py) that is the read of their byte ranges and their upload, on the upload stream
            ref_pool = ThreadPoolExecutor(max_workers=2)
            for k in self.keys[i:min(self.run_end[i], i + 3)]:
                refs.setdefault(k[0], ref_pool.submit(reference_for, params['fasta_path'], k[0], device, params))
            try:
                self.dbam = open_device_bam(params['sam_path'], device, contigs=list(self.run_dev[i]))
            except DeviceIngestUnavailable:
                pass                                                  # (includes: not enough free device / page-locked memory -- the host route needs neither)
            ref_pool.shutdown(wait=False)
        if self.dbam is not None:
            db = self.dbam
            self.prepare = lambda chrom, grp: _prepare_device(db, params, chrom, grp, refs.pop(chrom, None))   # noqa: E731
        else:
            self.prepare = lambda chrom, grp: _prepare_wire(params, chrom, grp)   # noqa: E731
            if self.uploader is None:
                from .wire import WireUploader
                self.uploader = WireUploader(get_engine(device))
        self.nxt = i
        while self.nxt < self.run_end[i] and len(self.preps) < self.ahead:
            self._prepare_next(self.run_end[i])

    def pack_for(self, i):
        """-> (group i's DevicePack, callable that releases its upload slot once the group's kernels are enqueued)"""
        if i == 0 or self.run_end[i - 1] == i:
            self.enter_run(i)
        wp = self.preps.pop(0).result()
        self._prepare_next(self.run_end[i])
        if self.dbam is not None:
            # one codes buffer for every group: all steps run on one stream, so group i + 1's decode is ordered behind group i's last reader
            if self.codes is None or self.codes.numel() < wp['codes_len']:
                self.codes = torch.empty(wp['codes_len'] + wp['codes_len'] // 8, dtype=torch.uint8, device=get_engine(self.device).device)
            return self.dbam.pack(wp, codes=self.codes), lambda: None
        tk = self.uploader.submit(wp)
        return self.uploader.expand(tk), lambda: self.uploader.release(tk)

    def close(self):
        self.pool.shutdown(wait=True)
        if self.dbam is not None:
            # the share of the file this worker had in HBM goes when the worker is done (the stages that follow -- phasing, the indel
            # callers -- need the memory; the loader's work buffers up to 16 GB stay for the next load)
            from .device_bam import release as release_device_bam
            from .device_fasta import release as release_device_fasta
            self.dbam = self.prepare = None
            release_device_bam(self.params['sam_path'])
            release_device_fasta(self.params['fasta_path'])              # (the last contig's FASTA image, where the reference took the device route)


class _Records:
    """Host pipeline of caller(): the genotype rules + record text of one (contig, ploidy) group are produced and written by a worker
    thread (the formatter is native code: the GIL is released) while the GPU already works on the next group."""

    def __init__(self, f, pool, counter_Q, gvcf_f=None):
        self.f, self.pool, self.counter_Q, self.scratch, self.pending, self.gvcf_f = f, pool, counter_Q, None, None, gvcf_f

    def emit(self, chrom, ploidy, r, grp, blocks=None, keep_text=False):
        """keep_text (the gVCF's device writer): -> the group's record lines as bytes; caller() merges them into the group's blocks on the device"""
        f = self.f
        text = b''
        if r['n']:
            need = (400 + len(chrom)) * r['n'] + 1024
            if self.scratch is None or self.scratch.size < need:
                self.scratch = np.empty(need + need // 4, np.uint8)
            text = snp_vcf_text(chrom, r['pos'], r['ref'], r['probs'], r['dp'], r['freq'], r['fwd_dp'], r['rev_dp'],
                                haploid=(ploidy != 'diploid'), as_array=True, out=self.scratch)
            f.write(text)
        f.flush()
        os.fsync(f.fileno())
        if blocks is not None:
            # the group's share of the gVCF: its variant lines, as they are, between the blocks the device cut at them
            from . import gvcf
            for piece in gvcf.splice(blocks[0], blocks[1], blocks[2], text, r['pos'] if r['n'] else []):
                self.gvcf_f.write(piece)
            self.gvcf_f.flush()
        for _ in grp:
            self.counter_Q.put(1)
        if keep_text:
            return text.tobytes() if r['n'] else b''                 # (a copy: the next group's lines overwrite the scratch)

    def wait(self):
        if self.pending is not None:
            return self.pending.result()                             # keeps the records in group order; re-raises errors

    def submit(self, chrom, ploidy, r, grp, blocks=None, keep_text=False):
        self.wait()
        self.pending = self.pool.submit(self.emit, chrom, ploidy, r, grp, blocks, keep_text)


def caller(params, chunks_Q, counter_Q, snp_files, device=0, worker_id=1):
    """Worker with the reference's signature (snpCaller.py:57): drains `chunks_Q`, writes
    <intermediate_snp_files_dir>/<prefix>.<worker>.snps.vcf.  Chunks are grouped per (contig, ploidy)
    and each group is one device batch."""
    from concurrent.futures import ThreadPoolExecutor
    curr_vcf_path = os.path.join(params['intermediate_snp_files_dir'], '%s.%d.snps.vcf' % (params['prefix'], worker_id))
    snp_files.append(curr_vcf_path)
    chunks = []
    while True:
        try:
            chunks.append(chunks_Q.get(block=False))
        except queue.Empty:
            break
        except Exception:
            if chunks_Q.empty():
                break
            raise
    groups = {}
    for c in chunks:
        groups.setdefault((c['chrom'], c['ploidy']), []).append(c)
    keys = list(groups)
    last_use = {chrom: i for i, (chrom, _) in enumerate(keys)}         # last group of every contig
    for k in keys:
        groups[k].sort(key=lambda c: c['start'])
    # BAM inputs take the ingest pipeline (_Ingest); NC_SERIAL_INGEST=1 keeps the round-2 behaviour (decode + upload inside call_chunks, the
    # GPU idle meanwhile)
    piped = isinstance(params['sam_path'], str) and os.path.exists(params['sam_path']) and not os.environ.get('NC_SERIAL_INGEST')
    depth = max(1, int(os.environ.get('NC_CALLER_DEPTH', 2 if piped else 1)))
    from contextlib import ExitStack
    from . import gvcf
    gvcf_cfg = gvcf.settings(params) if gvcf.enabled(params) else None          # (opt-in: <prefix>.<worker>.snps.g.vcf beside the worker's VCF)
    gvcf_dev = gvcf_cfg is not None and gvcf.writer(params) == 'device'          # (section 22: <prefix>.<worker>.snps.g.vcf.bgzf + .npz instead)
    with open(curr_vcf_path, 'wb') as f, ThreadPoolExecutor(max_workers=1) as pool, ExitStack() as stack:
        gvcf_f = stack.enter_context(open(gvcf.worker_path(params, worker_id), 'wb')) if gvcf_cfg and not gvcf_dev else None
        # the device writer's file writes run on the records thread, between two groups' records
        pieces = stack.enter_context(gvcf.PieceFile(gvcf.piece_path(params, worker_id), pool)) if gvcf_dev else None
        held_group = []                                              # the group whose records are being written: its pieces follow them
        records = _Records(f, pool, counter_Q, gvcf_f)
        ingest = _Ingest(params, keys, groups, device) if piped and keys else None
        in_flight = []                                               # groups whose kernels are queued and whose results have not been collected
        unrecorded = {}                                              # contig -> listed positions (params['genotype_sites']) inside its chunks that got no record

        def write_pieces():
            if held_group:
                held, chrom, ploidy, grp, pos = held_group.pop()
                text = records.wait()
                gvcf.group_pieces(get_engine(device), pieces, held, chrom, ploidy != 'diploid', [(c['start'], c['end']) for c in grp], text, pos, gvcf_cfg)
                pieces.flush()

        def collect():
            chrom, ploidy, call, grp, gi = in_flight.pop(0)
            r = call.result()
            if r.get('genotype_listed'):
                unrecorded[chrom] = unrecorded.get(chrom, 0) + r['genotype_listed'] - r['genotype_emitted']
            held, blocks = r.pop('gvcf', None), None
            if gvcf_dev:
                # the blocks, the merge with the group's lines and the compression run on the device once the records thread has formatted the
                # lines: the group before this one is due now, this one when the next is collected
                write_pieces()
                if held is not None:
                    held_group.append((held, chrom, ploidy, grp, r['pos'] if r['n'] else None))
            elif gvcf_cfg is not None and held is not None:
                # blocks and their text on the device, cut at the positions of the lines this group gets (PASS or not)
                blocks = gvcf.group_blocks(get_engine(device), held, chrom, ploidy != 'diploid', [(c['start'], c['end']) for c in grp],
                                           r['pos'] if r['n'] else None, gvcf_cfg)
            records.submit(chrom, ploidy, r, grp, blocks, keep_text=gvcf_dev and held is not None)
            if last_use[chrom] == gi:
                # a genome is walked contig by contig: drop the decoded alignments and the HBM pack of the one just finished (on an
                # ingest thread when there is one: unmapping ~100 MB takes 8 ms this thread would not be launching kernels)
                if ingest is not None:
                    ingest.pool.submit(release_contig, chrom)
                else:
                    release_contig(chrom)
        for i, (chrom, ploidy) in enumerate(keys):
            grp = groups[(chrom, ploidy)]
            if ingest is not None:
                dpk, done = ingest.pack_for(i)
                call = call_chunks(params, grp, device, dpk=dpk, defer=True)
                done()
            else:
                call = call_chunks(params, grp, device, defer=True)     # enqueued behind the previous group's CNN
            in_flight.append((chrom, ploidy, call, grp, i))
            # results are collected `depth` groups late: the copies that bring a group's results back run as kernels, and those wait for the NEXT
            # group's CNN (its persistent workgroups hold every CU) -- collecting group i - 1 right after enqueuing group i made the launching
            # thread wait out that CNN and only then prepare the next launch (6.3 ms a group for 4 ms of GPU work)
            while len(in_flight) > depth:
                collect()
        while in_flight:
            collect()
        records.wait()
        write_pieces()
        if not params.get('suppress_progress'):
            for chrom_, n_ in unrecorded.items():                    # (below mincov, a masked / non-AGTC / excluded reference base, no tensor)
                print('%s: %s: %d listed sites got no record (not eligible for a pileup).' % (str(datetime.datetime.now()), chrom_, n_), flush=True)
        if ingest is not None:
            ingest.close()


# ------------------------------------------------------------------ BGZF (so no bgzip binary is needed)
def bgzf_write(path, data: bytes):
    """BGZF file through the library's multi-threaded compressor (see vcfio.py)"""
    from . import vcfio
    vcfio.bgzf_write(path, data)


def _sort_key(line, order):
    f = line.split('\t', 2)
    return (order.get(f[0], 1 << 30), int(f[1]))


def call_manager(params, devices=None):
    """Same contract as snpCaller.call_manager (snpCaller.py:213-287): returns the PASS VCF path
    <vcf_path>/<prefix>.snps.vcf.gz (also writes <prefix>.unfiltered.snps.vcf.gz).
    Under torch.distributed (one process per GPU, e.g. torchrun) every rank calls this function: the chunk list
    is sharded over the ranks, each rank works on ITS GPU (engine.local_device: LOCAL_RANK, or devices[local rank]) and
    writes its own worker file, rank 0 merges (other ranks return the path)."""
    from . import gvcf, shard
    from .engine import local_device
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    if gvcf.enabled(params):
        gvcf.writer(params)                                           # (an unknown writer is refused before any work)
    if world > 1:                                                     # next to its GPU before anything page-locks memory or starts threads
        from .numa import bind_rank
        bind_rank(local_device(devices, rank))
    chunks_Q = queue.Queue()
    counter_Q = queue.Queue()
    snp_files = []
    from .device_bam import ensure_index
    ensure_index(params.get('sam_path'), params, local_device(devices, rank), collective=True)   # opt-in: rank 0 indexes a BAM that has no index, the others wait
    wts = shard.depth_weights(params.get('sam_path'), params['chunks_list']) if world > 1 else None      # balance by the alignments held
    for chunk in shard.shard_chunks(params['chunks_list'], rank, world, wts):
        chunks_Q.put(chunk)
    params['intermediate_snp_files_dir'] = os.path.join(params['vcf_path'], 'intermediate_snp_files')
    if rank == 0:
        if os.path.exists(params['intermediate_snp_files_dir']):
            shutil.rmtree(params['intermediate_snp_files_dir'])
        os.makedirs(params['intermediate_snp_files_dir'])
    shard.barrier()
    caller(params, chunks_Q, counter_Q, snp_files, device=local_device(devices, rank), worker_id=rank + 1)
    shard.barrier()
    all_path_ = os.path.join(params['vcf_path'], '%s.snps.vcf.gz' % params['prefix'])
    if rank != 0:
        shard.barrier()
        return all_path_
    snp_files = [os.path.join(params['intermediate_snp_files_dir'], '%s.%d.snps.vcf' % (params['prefix'], r + 1))
                 for r in range(world)]
    all_path = os.path.join(params['vcf_path'], '%s.unfiltered.snps.vcf.gz' % params['prefix'])
    pass_path = os.path.join(params['vcf_path'], '%s.snps.vcf.gz' % params['prefix'])
    if not params.get('suppress_progress'):
        print('\n%s: Combining SNP calls.' % str(datetime.datetime.now()))
    contigs = []
    for x in params['regions_list']:
        if x[0] not in contigs:
            contigs.append(x[0])
    header = VCF_HEADER.format(contigs=''.join('##contig=<ID=%s>\n' % c for c in contigs), sample=params['sample'])
    lines = []
    for fn in snp_files:
        with open(fn) as fd:
            lines.extend(fd.readlines())
    order = {c: i for i, c in enumerate(contigs)}
    keyed = []
    for ln in lines:                                                # CHROM, POS, REF, FILTER of every record
        f = ln.split('\t', 7)
        keyed.append((order.get(f[0], 1 << 30), int(f[1]), len(f[3]), f[6] == 'PASS', ln))
    keyed.sort(key=lambda k: (k[0], k[1]))                          # bcftools sort (:284); stable, keeps E3 duplicates
    from . import vcfio
    for path, recs in ((all_path, keyed), (pass_path, [k for k in keyed if k[3]])):     # bcftools view -f PASS (:285)
        body = ''.join(k[4] for k in recs).encode()
        vcfio.write_vcf_gz_with_csi(path, header, body, contigs, np.array([k[0] for k in recs], np.int64),
                                    np.array([k[1] for k in recs], np.int64), np.array([k[2] for k in recs], np.int64),
                                    np.array([len(k[4].encode()) for k in recs], np.int64))   # + <path>.csi (tabix -p vcf --csi)
    if gvcf.enabled(params):
        # <prefix>.snps.g.vcf.gz + .csi: every rank's blocks and variant lines (a block never spans two ranks' chunk runs)
        g_path = os.path.join(params['vcf_path'], '%s.snps.g.vcf.gz' % params['prefix'])
        if gvcf.writer(params) == 'device':                          # compressed pieces, concatenated (section 22)
            gvcf.merge_pieces([gvcf.piece_path(params, r + 1) for r in range(world)], g_path, contigs, params['sample'])
        else:
            gvcf.merge_worker_files([gvcf.worker_path(params, r + 1) for r in range(world)], g_path, contigs, params['sample'])
    shard.barrier()
    return pass_path

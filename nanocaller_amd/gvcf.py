"""gVCF output of the SNP caller: reference-confidence blocks between the variant records.

Opt-in: params['gvcf'] (or NC_GVCF=1 where the key is absent).  The per-column counts, the blocks and the blocks' record text are made on the
device (csrc/nc_refconf.hip through Engine.refconf_columns / refconf_blocks / refconf_text); this module holds what the host does: parameter
parsing, the three integer constants of the model, the header, the splice of a group's variant lines into its block text and the merge of the
workers' files.  `scores` and `block_line` state the PL rule and the line format in plain Python: the tests compare the device with them.

The model.  e = params['gvcf_error'] (default 0.1) is the per-read error rate; c_m = round(-10000 log10(1 - e)), c_x = round(-10000 log10 e),
c_h = round(-10000 log10 0.5).  A column with n pileup entries, ref of them the reference base and alt = n - ref has S00 = ref c_m + alt c_x,
S01 = n c_h, S11 = ref c_x + alt c_m; other = min(S01, S11) (haploid: S11); it is a no-call when n == 0 or S00 > other, else
GQ = min(99, (other - S00) // 1000); PL_g = min(9999, (S_g - min S) // 1000).  params['gvcf_gq_bands'] (default [0, 20, 40, 60, 80]): ascending
lower edges, the first one 0; a block is a maximal run of assessed columns of one band (no-call columns are a band of their own).
"""
from __future__ import annotations

import math
import os

import numpy as np

DEFAULT_ERROR = 0.1
DEFAULT_GQ_BANDS = (0, 20, 40, 60, 80)
MAX_BANDS = 16

HEADER_LINES = (
    '##ALT=<ID=*,Description="Any allele that is not the reference allele: a reference-confidence block">\n'
    '##INFO=<ID=END,Number=1,Type=Integer,Description="Last position of the reference-confidence block">\n'
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the smallest of the block\'s columns">\n'
    '##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description="Smallest depth (pileup entries, deletions included) of the block\'s columns">\n'
    '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods of the column with the block\'s smallest GQ, against <*>">\n')


def enabled(params) -> bool:
    """params['gvcf'] where the key is present, else NC_GVCF=1"""
    if 'gvcf' in params:
        return bool(params['gvcf'])
    return os.environ.get('NC_GVCF') == '1'


def constants(error=DEFAULT_ERROR):
    """(c_m, c_x, c_h) of the per-read error rate: the only floating-point step of the model"""
    e = float(error)
    if not 0.0 < e < 0.5:
        raise ValueError("gvcf_error must lie in (0, 0.5), got %r" % (error,))
    return tuple(int(round(-10000.0 * math.log10(x))) for x in (1.0 - e, e, 0.5))


def gq_bands(bands=None):
    """the validated list of lower edges"""
    b = [int(x) for x in (DEFAULT_GQ_BANDS if bands is None else bands)]
    if not 1 <= len(b) <= MAX_BANDS:
        raise ValueError("gvcf_gq_bands holds 1 to %d lower edges, got %d" % (MAX_BANDS, len(b)))
    if b[0] != 0:
        raise ValueError("gvcf_gq_bands must start at 0, got %d" % b[0])
    if any(y <= x for x, y in zip(b, b[1:])):
        raise ValueError("gvcf_gq_bands must ascend strictly: %r" % (b,))
    return b


def settings(params):
    """-> dict(error, bands, constants) of a params dict (raises on values the model refuses)"""
    error = float(params.get('gvcf_error', DEFAULT_ERROR))
    return dict(error=error, bands=gq_bands(params.get('gvcf_gq_bands')), constants=constants(error))


def scores(n, alt, consts, haploid=False):
    """-> (no_call, GQ, PL tuple) of a column with n entries, alt of them not the reference base"""
    c_m, c_x, c_h = consts
    n, alt = int(n), int(alt)
    ref = n - alt
    s00, s01, s11 = ref * c_m + alt * c_x, n * c_h, ref * c_x + alt * c_m
    s = (s00, s11) if haploid else (s00, s01, s11)
    other = min(s[1:])
    no_call = n == 0 or s00 > other
    gq = 0 if no_call else min(99, (other - s00) // 1000)
    m = min(s)
    return no_call, gq, tuple(min(9999, (x - m) // 1000) for x in s)


def band_of(gq, bands):
    """index of the last edge <= gq"""
    return int(np.searchsorted(np.asarray(bands), gq, side='right')) - 1


def block_line(chrom, start, end, ref_letter, min_dp, gq, n_at, alt_at, consts, haploid=False):
    """the record of one block (what nc_refconf_text writes on the device)"""
    no_call, _, pl = scores(n_at, alt_at, consts, haploid)
    gt = ('.' if no_call else '0') if haploid else ('./.' if no_call else '0/0')
    return '%s\t%d\t.\t%s\t<*>\t0\t.\tEND=%d\tGT:GQ:MIN_DP:PL\t%s:%d:%d:%s\n' % (chrom, start, ref_letter, end, gt, gq, min_dp, ','.join('%d' % x for x in pl))


def header(contigs, sample):
    """the SNP caller's header with the gVCF lines in front of the column line (snpCaller.VCF_HEADER itself is unchanged)"""
    from .snpCaller import VCF_HEADER
    h = VCF_HEADER.format(contigs=''.join('##contig=<ID=%s>\n' % c for c in contigs), sample=sample)
    at = h.index('#CHROM')
    return h[:at] + HEADER_LINES + h[at:]


def worker_path(params, worker_id):
    return os.path.join(params['intermediate_snp_files_dir'], '%s.%d.snps.g.vcf' % (params['prefix'], worker_id))


def splice(block_text, line_off, block_start, variant_text, variant_pos):
    """A group's block lines (uint8 array, byte offset of every line [n + 1], start of every block, ascending) with its variant lines (uint8 array or
    bytes, one line per position of variant_pos, ascending) put in position order.  The blocks are cut at the records, so every record falls
    between two blocks: a searchsorted on the block starts.  -> list of buffers to write in order"""
    bt = np.asarray(block_text, np.uint8)
    vt = np.frombuffer(variant_text, np.uint8) if isinstance(variant_text, (bytes, bytearray)) else np.asarray(variant_text, np.uint8)
    vpos = np.asarray(variant_pos, np.int64)
    if vpos.size == 0:
        return [bt]
    vend = np.flatnonzero(vt == 10) + 1
    if vend.size != vpos.size:
        raise ValueError("splice: %d variant lines for %d positions" % (vend.size, vpos.size))
    vbeg = np.concatenate([[0], vend[:-1]])
    at = np.searchsorted(np.asarray(block_start, np.int64), vpos, side='left')   # blocks in front of each record
    off = np.asarray(line_off, np.int64)
    out, done = [], 0
    # runs of records that share a gap between blocks go out as one piece
    first = np.flatnonzero(np.concatenate([[True], at[1:] != at[:-1]]))
    last = np.concatenate([first[1:], [vpos.size]]) - 1
    for a, b in zip(first.tolist(), last.tolist()):
        k = int(at[a])
        if k > done:
            out.append(bt[off[done]:off[k]])
            done = k
        out.append(vt[vbeg[a]:vend[b]])
    if done < off.size - 1:
        out.append(bt[off[done]:off[-1]])
    return out


def parse_line(line):
    """-> (chrom, pos, reference length the index covers): END - POS + 1 of a block, len(REF) of a variant record"""
    f = line.split('\t', 8)
    pos = int(f[1])
    if f[4] == '<*>' and f[7].startswith('END='):
        return f[0], pos, int(f[7][4:].split(';', 1)[0]) - pos + 1
    return f[0], pos, len(f[3])


def merge_worker_files(files, out_path, contigs, sample):
    """The workers' .snps.g.vcf files as one position-sorted <out_path> (BGZF) + .csi.  A block's index interval runs to its END; variant lines are
    copied as they are.  Every worker's lines of a contig are already in order and no block spans two workers' chunk runs, so a stable sort by
    (contig, position) is the merge.  -> number of records"""
    from . import vcfio
    order = {c: i for i, c in enumerate(contigs)}
    keyed = []
    for fn in files:
        if not os.path.exists(fn):
            continue
        with open(fn) as fd:
            for ln in fd:
                c, pos, rl = parse_line(ln)
                keyed.append((order.get(c, 1 << 30), pos, rl, ln))
    keyed.sort(key=lambda k: (k[0], k[1]))
    body = ''.join(k[3] for k in keyed).encode()
    vcfio.write_vcf_gz_with_csi(out_path, header(contigs, sample), body, list(contigs), np.array([k[0] for k in keyed], np.int64),
                                np.array([k[1] for k in keyed], np.int64), np.array([k[2] for k in keyed], np.int64),
                                np.array([len(k[3].encode()) for k in keyed], np.int64))
    return len(keyed)


def group_blocks(eng, held, chrom, haploid, spans, record_pos, cfg):
    """The blocks of one (contig, ploidy) group on the device: `held` = Engine.refconf_columns' result for the group's pack, spans = the group's
    chunk intervals, record_pos = positions of the lines the SNP caller wrote for the group (each cuts its column out).
    -> (text uint8 array, line_off int64 [n + 1], block starts int64 [n])"""
    words, ref_code, tile_pos0 = held
    pos = np.asarray(record_pos if record_pos is not None else [], np.int32).reshape(-1)
    cuts = np.stack([pos, pos], 1) if pos.size else None
    blocks = eng.refconf_blocks(words, tile_pos0, spans, cuts, error=cfg['error'], bands=cfg['bands'], haploid=haploid, device_out=True)
    text, off = eng.refconf_text(blocks, ref_code, tile_pos0, chrom, error=cfg['error'], haploid=haploid)
    start = blocks[:, 0].to('cpu').numpy().astype(np.int64) if blocks.shape[0] else np.zeros(0, np.int64)
    return text, off, start

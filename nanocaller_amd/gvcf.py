"""gVCF output of the SNP caller: reference-confidence blocks between the variant records.

Opt-in: params['gvcf'] (or NC_GVCF=1 where the key is absent).  The per-column counts, the blocks and the blocks' record text are made on the
device (csrc/nc_refconf.hip through Engine.refconf_columns / refconf_blocks / refconf_text); this module holds what the host does: parameter
parsing, the three integer constants of the model, the header, the splice of a group's variant lines into its block text and the merge of the
workers' files.  `scores` and `block_line` state the PL rule and the line format in plain Python: the tests compare the device with them.

params['gvcf_writer'] = 'device' (or NC_GVCF_WRITER=device where the key is absent) takes the splice, the compression and
the index to the device: `group_pieces` writes a group's lines as BGZF pieces (vcf_write.write_piece) to a `PieceFile`, `merge_pieces` concatenates
the workers' pieces and joins their index summaries.  The default, 'host', is the path above.

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


def writer(params) -> str:
    """'host' or 'device': params['gvcf_writer'] where the key is present, else NC_GVCF_WRITER, else 'host' (section 22).  Only read when the
    gVCF is on."""
    v = params['gvcf_writer'] if 'gvcf_writer' in params else os.environ.get('NC_GVCF_WRITER', 'host')
    if v not in ('host', 'device'):
        raise ValueError("gvcf_writer must be 'host' or 'device', got %r" % (v,))
    return v


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


# ------------------------------------------------------------------------------------------------------------ the device writer (section 22)
def piece_path(params, worker_id):
    return worker_path(params, worker_id) + '.bgzf'


def variant_lines(text):
    """-> (byte offset of every line int64 [n + 1], len(REF) of every line int64 [n]) of record lines (uint8 array)"""
    vt = np.asarray(text, np.uint8)
    vend = np.flatnonzero(vt == 10) + 1
    tabs = np.flatnonzero(vt == 9)
    first = np.searchsorted(tabs, np.concatenate([[0], vend[:-1]]))       # every line's first tab: CHROM's
    if vend.size and (first[-1] + 3 >= tabs.size or np.any(tabs[first + 3] >= vend)):
        raise ValueError("variant_lines: a line with fewer than five fields")
    return np.concatenate([[0], vend]).astype(np.int64), (tabs[first + 3] - tabs[first + 2] - 1).astype(np.int64)


def chunk_runs(spans):
    """maximal runs of abutting or overlapping intervals (both ends inclusive) -> [(start, end)], ascending"""
    out = []
    for s, e in sorted((int(s), int(e)) for s, e in spans):
        if out and s <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [tuple(x) for x in out]


PIECE_ARRAYS = (('run_bin', np.int32), ('run_vbeg', np.uint64), ('run_vend', np.uint64), ('win_min', np.uint64))


class PieceFile:
    """A worker's pieces: the file they are appended to and their summaries, which close() writes to the sidecar <path>.npz.  It is the file
    object write_piece writes to; with `pool` (a one-thread executor) a write runs there and write() returns once the write BEFORE it is done,
    which is what write_piece's two staging buffers need."""

    def __init__(self, path, pool=None):
        self.path, self.pool, self.f, self.offset, self.pieces, self.pending = path, pool, open(path, 'wb'), 0, [], None
        self.ms, self.merged_bytes = {}, 0                              # group_pieces' stage times and the bytes its merges wrote

    def write(self, buf):
        if self.pool is None:
            self.f.write(buf)
            return
        self.flush()
        self.pending = self.pool.submit(self.f.write, buf)

    def flush(self):
        if self.pending is not None:
            pending, self.pending = self.pending, None
            pending.result()

    def add(self, piece, contig, first, last):
        """file the summary of the piece write_piece has just written: its lines cover the 1-based positions first .. last of contig"""
        self.flush()
        self.pieces.append(dict(piece, contig=contig, first=int(first), last=int(last), offset=self.offset, file=self.path))
        self.offset += int(piece['bytes'])

    def close(self):
        self.flush()
        self.f.close()
        save_pieces(self.path + '.npz', self.pieces)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def save_pieces(path, pieces):
    """the summaries of a worker's pieces as one .npz: per piece contig, first and last position, file offset, length, lines, first window;
    the runs and the window minima of all pieces back to back with their bounds"""
    arrays = dict(contig=np.array([p['contig'] for p in pieces], dtype=str))
    for k in ('first', 'last', 'offset', 'bytes', 'lines', 'w0'):
        arrays[k] = np.array([int(p[k]) for p in pieces], np.int64)
    for which, names in (('run', PIECE_ARRAYS[:3]), ('win', PIECE_ARRAYS[3:])):
        arrays[which + '_ptr'] = np.concatenate([[0], np.cumsum([np.asarray(p[names[0][0]]).size for p in pieces])]).astype(np.int64)
        for k, dt in names:
            arrays[k] = np.concatenate([np.asarray(p[k], dt) for p in pieces]) if pieces else np.zeros(0, dt)
    with open(path, 'wb') as f:
        np.savez(f, **arrays)


def load_pieces(path, file):
    """-> the summaries save_pieces wrote, each with 'file' = the file its bytes are in"""
    with np.load(path) as z:
        a = {k: z[k] for k in z.files}
    out = []
    for i in range(a['first'].size):
        p = dict(contig=str(a['contig'][i]), file=file, **{k: int(a[k][i]) for k in ('first', 'last', 'offset', 'bytes', 'lines', 'w0')})
        for which, names in (('run', PIECE_ARRAYS[:3]), ('win', PIECE_ARRAYS[3:])):
            lo, hi = int(a[which + '_ptr'][i]), int(a[which + '_ptr'][i + 1])
            for k, _ in names:
                p[k] = a[k][lo:hi]
        out.append(p)
    return out


def group_pieces(eng, out, held, chrom, haploid, spans, variant_text, variant_pos, cfg, slab_members=4096):
    """The device twin of group_blocks + splice: the group's blocks and their text are made on the device as there, the group's variant lines
    (bytes or uint8 array, one line per position of variant_pos, ascending) are uploaded and merged in between (Engine.lines_merge: a block that
    starts where a record stands follows it, as splice's searchsorted has it), and one BGZF piece per maximal run of abutting or overlapping
    chunk intervals is written to `out` (a PieceFile) by vcf_write.write_piece.  -> the pieces' summaries (they are filed in `out` as well)."""
    import torch

    from . import vcf_write
    from .bgzf import event_timed
    words, ref_code, tile_pos0 = held
    dev = eng.device
    timed = event_timed(out.ms)                                         # (milliseconds per stage, summed over the groups: tools/bench_gvcf_write.py)
    pos = np.asarray(variant_pos if variant_pos is not None else [], np.int64).reshape(-1)
    cuts = np.stack([pos, pos], 1).astype(np.int32) if pos.size else None
    blocks = timed('blocks', lambda: eng.refconf_blocks(words, tile_pos0, spans, cuts, error=cfg['error'], bands=cfg['bands'], haploid=haploid, device_out=True))
    text, off = timed('text', lambda: eng.refconf_text(blocks, ref_code, tile_pos0, chrom, error=cfg['error'], haploid=haploid, device_out=True))
    a = b = None
    if blocks.shape[0]:
        beg = blocks[:, 0].to(torch.int64) - 1
        a = (text, off, beg, beg, blocks[:, 1].to(torch.int64))
    if pos.size:
        vt = np.frombuffer(variant_text, np.uint8) if isinstance(variant_text, (bytes, bytearray)) else np.asarray(variant_text, np.uint8)
        voff, ref_len = variant_lines(vt)
        if voff.size - 1 != pos.size:
            raise ValueError("group_pieces: %d variant lines for %d positions" % (voff.size - 1, pos.size))
        b = tuple(torch.from_numpy(np.array(x)).to(dev) for x in (vt, voff, pos - 1, pos - 1, pos - 1 + ref_len))
    m_text, m_off, m_beg, m_end, _ = timed('merge', lambda: eng.lines_merge(a, b))
    out.merged_bytes += int(m_text.numel())
    n = int(m_beg.numel())
    if n == 0:
        return []
    runs = chunk_runs(spans)
    edges = torch.tensor([[s - 1, e] for s, e in runs], dtype=torch.int64, device=dev).reshape(-1)
    at = torch.searchsorted(m_beg, edges)                               # the lines that begin inside each run
    ends = m_end[(at[1::2] - 1).clamp(min=0)]
    at, ends = at.cpu().numpy().reshape(-1, 2), ends.cpu().numpy()
    if int((at[:, 1] - at[:, 0]).sum()) != n or np.any(at[1:, 0] != at[:-1, 1]):
        raise ValueError("group_pieces: %s: lines outside the group's chunk intervals" % chrom)
    made = []
    for (l0, l1), last in zip(at.tolist(), ends.tolist()):
        if l1 > l0:
            piece = vcf_write.write_piece(eng, out, m_text, m_off[l0:l1 + 1], m_beg[l0:l1], m_end[l0:l1], slab_members=slab_members)
            for k, v in piece['ms'].items():
                out.ms[k] = out.ms.get(k, 0.0) + v
            out.add(piece, chrom, int(m_beg[l0].item()) + 1, last)
            made.append(out.pieces[-1])
    return made


class _Span:
    """`left` bytes of a file object from where it stands, as a file object for shutil.copyfileobj"""

    def __init__(self, f, left):
        self.f, self.left = f, left

    def read(self, size=-1):
        if self.left <= 0:
            return b''
        got = self.f.read(self.left if size is None or size < 0 else min(size, self.left))
        self.left -= len(got)
        return got


def merge_pieces(files, out_path, contigs, sample):
    """The workers' piece files (each with its sidecar <file>.npz) as one position-sorted <out_path> (BGZF) + .csi, without reading a line: the
    pieces sorted by (contig order, first position) are copied behind the header, which gets members of its own, and the index is their
    summaries joined (hts_index.csi_from_summaries).  Two pieces of a contig that overlap raise ValueError before anything is written.
    -> number of records"""
    import shutil

    from . import vcfio
    from .bgzf import BGZF_EOF
    from .hts_index import csi_from_summaries
    order = {c: i for i, c in enumerate(contigs)}
    pieces = []
    for fn in files:
        if os.path.exists(fn + '.npz'):
            pieces.extend(p for p in load_pieces(fn + '.npz', fn) if p['lines'])
    for p in pieces:
        if p['contig'] not in order:
            raise ValueError("merge_pieces: %s holds lines of contig %r, which the header does not name" % (p['file'], p['contig']))
    pieces.sort(key=lambda p: (order[p['contig']], p['first']))
    name = lambda p: '%s:%d-%d (%s, byte %d)' % (p['contig'], p['first'], p['last'], p['file'], p['offset'])  # noqa: E731
    for p, q in zip(pieces, pieces[1:]):
        if p['contig'] == q['contig'] and q['first'] <= p['last']:
            raise ValueError("merge_pieces: the pieces %s and %s overlap: the file would not be sorted" % (name(p), name(q)))
    hdr = header(contigs, sample).encode()
    comp, coff = vcfio.bgzf_compress(hdr)
    head = comp[:int(coff[-(-len(hdr) // vcfio.BGZF_BLOCK)])]            # the header's members, without the EOF block behind them
    per_ref = [[] for _ in contigs]
    handles = {}
    try:
        with open(out_path, 'wb') as f:
            f.write(head)
            at = int(head.size)
            for p in pieces:
                src = handles.get(p['file'])
                if src is None:
                    src = handles[p['file']] = open(p['file'], 'rb')
                src.seek(p['offset'])
                span = _Span(src, p['bytes'])
                shutil.copyfileobj(span, f, 1 << 22)
                if span.left:
                    raise ValueError("merge_pieces: %s ends inside the piece %s" % (p['file'], name(p)))
                per_ref[order[p['contig']]].append(dict(p, offset=at))
                at += p['bytes']
            f.write(BGZF_EOF)
    finally:
        for src in handles.values():
            src.close()
    vcfio.bgzf_write(out_path + '.csi', csi_from_summaries(len(contigs), per_ref, aux=vcfio.tabix_aux(contigs)))
    return sum(p['lines'] for p in pieces)

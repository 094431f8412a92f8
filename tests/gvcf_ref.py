"""The yardstick of the gVCF's reference-confidence blocks: a numpy restatement of the model, built from a world's arrays.

    columns(world, exclude)       per-position counts straight from the read-major codes: n (codes 0..4), per-base counts, the reference code
                                  with exclusions (oracle.ref_codes_with_exclusions: N and excluded intervals are "code >= 4")
    model(n, alt, ...)            no-call / GQ / band per column, integer arithmetic (Python-exact int64)
    blocks(...)                   maximal runs of open columns of one band -> int32 [k][6]: start, end, min n, min GQ, n and alt of the leftmost column
                                  that attains that GQ

tests/test_gvcf_ref.py ties `columns` to the CPU oracle's scan and proves the construction sharp; tests/test_gvcf_gpu.py compares the HIP path with it.
"""
import numpy as np

from nanocaller_amd import gvcf
from nanocaller_amd.synth import FLAG_FILTER_DEFAULT, FLAG_FILTER_SUPPL
from oracle import oracle

CONSTS = gvcf.constants(0.1)
BANDS = list(gvcf.DEFAULT_GQ_BANDS)
CLOSED = -2                                                           # a column's state: CLOSED, -1 no-call, else its band

_columns = {}


def columns(world, exclude=None, supplementary=False, key=None):
    """-> dict(rc uint8 [L], n int64 [L], cnt int64 [4][L], ref int64 [L], alt int64 [L], alt_max int64 [L]); index p - 1.  ref / alt are 0 where
    rc >= 4.  With `key`, computed once (callers must not modify it)."""
    if key is not None and key in _columns:
        return _columns[key]
    L = world.length
    rc = oracle.ref_codes_with_exclusions(world, exclude)
    filt = FLAG_FILTER_SUPPL if supplementary else FLAG_FILTER_DEFAULT
    keep = (np.asarray(world.read_flag) & filt) == 0
    s, e, off = np.asarray(world.read_start, np.int64), np.asarray(world.read_end, np.int64), np.asarray(world.read_off, np.int64)
    ln = e - s
    assert np.array_equal(ln, off[1:] - off[:-1])
    pos = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1] - s, ln)            # 1-based position of every code
    sel = np.repeat(keep, ln) & (pos >= 1) & (pos <= L)
    pos, code = pos[sel] - 1, np.asarray(world.codes)[sel]
    n = np.bincount(pos[code <= 4], minlength=L)[:L].astype(np.int64)
    cnt = np.stack([np.bincount(pos[code == b], minlength=L)[:L] for b in range(4)]).astype(np.int64)
    ok = rc < 4
    r = np.where(ok, rc, 0).astype(np.int64)
    ref = np.where(ok, cnt[r, np.arange(L)], 0)
    others = cnt.copy()
    others[r, np.arange(L)] = -1
    out = dict(rc=rc, n=n, cnt=cnt, ref=ref, alt=np.where(ok, n - ref, 0), alt_max=np.where(ok, others.max(0), 0))
    if key is not None:
        _columns[key] = out
    return out


def words(col, tile_pos0, npos):
    """what nc_refconf_columns writes for a pack grid that starts at tile_pos0: uint32 [npos]"""
    L = col["rc"].shape[0]
    w = np.full(npos, 0xFFFFFFFF, np.uint32)
    p = np.arange(tile_pos0, tile_pos0 + npos, dtype=np.int64)
    m = (p >= 1) & (p <= L)
    q = p[m] - 1
    w[m] = np.where(col["rc"][q] < 4, col["n"][q] | (col["alt"][q] << 16), 0xFFFFFFFF).astype(np.uint32)
    return w


def model(n, alt, consts=CONSTS, bands=BANDS, haploid=False):
    """-> (no_call bool, gq int64, band int64 with -1 for no-calls) per column"""
    c_m, c_x, c_h = (int(c) for c in consts)
    n, alt = np.asarray(n, np.int64), np.asarray(alt, np.int64)
    ref = n - alt
    s00, s01, s11 = ref * c_m + alt * c_x, n * c_h, ref * c_x + alt * c_m
    other = s11 if haploid else np.minimum(s01, s11)
    no_call = (n == 0) | (s00 > other)
    gq = np.where(no_call, 0, np.minimum(99, (other - s00) // 1000))
    band = np.where(no_call, -1, np.searchsorted(np.asarray(bands, np.int64), gq, side="right") - 1)
    return no_call, gq, band


def open_mask(n_cols, pos0, chunks, cuts, assessable):
    """open columns of a grid of n_cols columns whose first is position pos0: in the union of the chunks' [start, end], assessable (reference
    code < 4), in no cut interval"""
    p = np.arange(pos0, pos0 + n_cols, dtype=np.int64)
    region = np.zeros(n_cols, bool)
    for a, b in chunks:
        region |= (p >= a) & (p <= b)
    cut = np.zeros(n_cols, bool)
    for a, b in (cuts if cuts is not None else ()):
        cut |= (p >= a) & (p <= b)
    return region & np.asarray(assessable, bool) & ~cut


def blocks_of_words(w, pos0, chunks, cuts=None, consts=CONSTS, bands=BANDS, haploid=False):
    """blocks of a word array (uint32 [n_cols], n | alt << 16, all ones = not assessable) -> int32 [k][6]"""
    w = np.asarray(w).astype(np.uint32)
    ok = w != 0xFFFFFFFF
    n, alt = (w & 0xFFFF).astype(np.int64), (w >> 16).astype(np.int64)
    return blocks(np.where(ok, n, 0), np.where(ok, alt, 0), open_mask(w.size, pos0, chunks, cuts, ok), pos0, consts, bands, haploid)


def blocks(n, alt, is_open, pos0, consts=CONSTS, bands=BANDS, haploid=False):
    """maximal runs of consecutive open columns of one band"""
    n, alt = np.asarray(n, np.int64), np.asarray(alt, np.int64)
    _, gq, band = model(n, alt, consts, bands, haploid)
    state = np.where(is_open, band, CLOSED)
    before = np.concatenate([[CLOSED], state[:-1]])
    after = np.concatenate([state[1:], [CLOSED]])
    head = np.flatnonzero(is_open & (state != before))
    tail = np.flatnonzero(is_open & (state != after))
    assert head.size == tail.size
    if head.size == 0:
        return np.zeros((0, 6), np.int32)
    big = np.int64(1) << 62
    idx = np.arange(n.size, dtype=np.int64)
    dp = np.minimum.reduceat(np.where(is_open, n, big), head)
    key = np.minimum.reduceat(np.where(is_open, (gq << 32) | idx, big), head)
    at = key & 0xFFFFFFFF
    assert np.all((at >= head) & (at <= tail))
    return np.stack([head + pos0, tail + pos0, dp, key >> 32, n[at], alt[at]], 1).astype(np.int32)


def world_blocks(col, chunks, cuts=None, consts=CONSTS, bands=BANDS, haploid=False):
    """blocks of a world's columns (positions 1..L)"""
    L = col["rc"].shape[0]
    return blocks(col["n"], col["alt"], open_mask(L, 1, chunks, cuts, col["rc"] < 4), 1, consts, bands, haploid)


def lines(chrom, blk, ref_letters, consts=CONSTS, haploid=False):
    """the records of blocks through the Python formatter; ref_letters(pos) -> the reference letter"""
    return [gvcf.block_line(chrom, int(b[0]), int(b[1]), ref_letters(int(b[0])), int(b[2]), int(b[3]), int(b[4]), int(b[5]), consts, haploid) for b in blk]


def parse_block(line):
    """a block record back to (start, end, min_dp, gq, GT, PL tuple)"""
    f = line.rstrip("\n").split("\t")
    assert f[4] == "<*>" and f[7].startswith("END=") and f[8] == "GT:GQ:MIN_DP:PL"
    gt, gq, dp, pl = f[9].split(":")
    return int(f[1]), int(f[7][4:]), int(dp), int(gq), gt, tuple(int(x) for x in pl.split(","))


def tiles_crossed(blk, pos0, tile):
    """number of tile borders of a grid (first position pos0) that lie inside blocks"""
    a, b = (blk[:, 0].astype(np.int64) - pos0) // tile, (blk[:, 1].astype(np.int64) - pos0) // tile
    return int((b - a).sum())

"""htslib's binning index, read and written in one place: the .bai of SAMv1 5.2 and the CSIv1 of hts-specs (with the tabix auxiliary block
where the caller hands one in).  Host code, numpy only.

`index_bytes` is the one writer.  The BAM indexer (bam_index.index_bytes), the phased BAM's CSI (bam_write.csi_index) and the VCF's tabix
CSI (vcfio.csi_bytes) are calls into it.  `bai_linear_voffsets` / `csi_record_starts` read what the device BAM ingest wants of an index:
virtual offsets of record starts, per reference.
"""
from __future__ import annotations

import gzip
import struct

import numpy as np

_BIG = np.uint64(np.iinfo(np.uint64).max)


def reg2bin(beg, end, min_shift=14, depth=5):
    """hts_reg2bin for arrays of 0-based half-open intervals"""
    beg = np.asarray(beg, np.int64)
    end = np.asarray(end, np.int64) - 1
    out = np.zeros(beg.shape, np.int64)
    done = np.zeros(beg.shape, bool)
    s, t = min_shift, ((1 << (depth * 3)) - 1) // 7
    for lv in range(depth, 0, -1):
        hit = ~done & ((beg >> s) == (end >> s))
        out[hit] = t + (beg[hit] >> s)
        done |= hit
        s += 3
        t -= 1 << ((lv - 1) * 3)
    return out


def bin_first_window(bins, depth):
    """the first 2^min_shift window each bin covers"""
    out = np.zeros(bins.size, np.int64)
    for lv in range(depth + 1):
        t = ((1 << (3 * lv)) - 1) // 7
        m = (bins >= t) & (bins < t + (1 << (3 * lv)))
        out[m] = (bins[m] - t) << (3 * (depth - lv))
    return out


def linear_index(beg, end, vbeg, min_shift):
    """one reference: per 2^min_shift window the smallest virtual offset of a record that overlaps it; an empty window holds the uint64 maximum"""
    w0, w1 = beg >> min_shift, (end - 1) >> min_shift
    lin = np.full(int(w1.max()) + 1, _BIG, np.uint64)
    cnt = w1 - w0 + 1
    rows = np.repeat(np.arange(beg.size), cnt)
    win = w0[rows] + (np.arange(rows.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    np.minimum.at(lin, win, vbeg[rows])
    return lin


def bin_chunks(bins, vbeg, vend):
    """one reference: (bin ids ascending, first chunk of each, chunk counts, chunk begins, chunk ends).  The records of a bin stay in file
    order; adjacent ones -- the one begins where the other ends -- form one chunk."""
    o = np.argsort(bins, kind="stable")
    sb, svb, sve = bins[o], vbeg[o], vend[o]
    new = np.ones(sb.size, bool)
    new[1:] = (sb[1:] != sb[:-1]) | (svb[1:] != sve[:-1])
    starts = np.flatnonzero(new)
    ends = np.concatenate([starts[1:], [sb.size]]) - 1
    ub, first = np.unique(sb[starts], return_index=True)
    n_ch = np.diff(np.concatenate([first, [starts.size]]))
    return ub, first, n_ch, svb[starts], sve[ends]


def index_bytes(fmt, n_ref, refid, beg, end, unmapped, bins, vbeg, vend, min_shift=14, depth=5, aux=b"", pseudo_bin=True) -> bytes:
    """the .bai (fmt 'bai') or the uncompressed .csi (fmt 'csi'; `aux` = its auxiliary block) of a coordinate-sorted file from its records'
    arrays in file order: refID (below zero: unplaced), the 0-based span [beg, end) each is indexed under, flag & 4, bin (None: reg2bin of the
    span), virtual offsets of its first byte and of the byte behind it.  Per reference: the bins with their chunks, with `pseudo_bin` the
    pseudo-bin (virtual offsets of the reference's first and behind its last record; mapped and unmapped counts), and -- .bai -- the linear
    index, an empty window taking the offset of the window before it as samtools writes it, or -- .csi -- every bin's loffset = the linear
    index at the bin's first window, an empty one taking the next one's.  Behind the references, the number of unplaced records."""
    refid, beg, end = np.asarray(refid, np.int64), np.asarray(beg, np.int64), np.asarray(end, np.int64)
    vbeg, vend, unmapped = np.asarray(vbeg, np.uint64), np.asarray(vend, np.uint64), np.asarray(unmapped, bool)
    bins = reg2bin(beg, end, min_shift, depth) if bins is None else np.asarray(bins, np.int64)
    bai = fmt == "bai"
    out = [b"BAI\1" + struct.pack("<i", n_ref)] if bai else [b"CSI\1", struct.pack("<3i", min_shift, depth, len(aux)), aux, struct.pack("<i", n_ref)]
    # [a, b) of every reference's records in the (sorted) record list; the unplaced ones lie behind them
    edges = np.searchsorted(np.where(refid < 0, n_ref, refid), np.arange(n_ref + 1))
    for r in range(n_ref):
        a, b = int(edges[r]), int(edges[r + 1])
        summ = None if a == b else reference_summary(beg[a:b], end[a:b], unmapped[a:b], bins[a:b], vbeg[a:b], vend[a:b], min_shift)
        out.append(summary_bytes(fmt, summ, depth, pseudo_bin))
    out.append(struct.pack("<Q", int(refid.size - edges[n_ref])))
    return b"".join(out)


def reference_summary(beg, end, unmapped, bins, vbeg, vend, min_shift=14):
    """first half of index_bytes, one reference's records -> what its index stores: dict(bins ascending, first = the first chunk of each,
    n_chunks, chunk_beg, chunk_end, lin = the linear minima per 2^min_shift window from window 0 on, mapped, unmapped, vmin, vmax)"""
    ub, first, n_ch, cb, ce = bin_chunks(bins, vbeg, vend)
    n_un = int(np.count_nonzero(unmapped))
    return dict(bins=ub, first=first, n_chunks=n_ch, chunk_beg=cb, chunk_end=ce, lin=linear_index(beg, end, vbeg, min_shift),
                mapped=int(beg.size) - n_un, unmapped=n_un, vmin=int(vbeg.min()), vmax=int(vend.max()))


def summary_bytes(fmt, summ, depth=5, pseudo_bin=True) -> bytes:
    """second half of index_bytes: one reference's section of a .bai or .csi from its summary (None: a reference without records)"""
    bai = fmt == "bai"
    if summ is None:
        return struct.pack("<ii", 0, 0) if bai else struct.pack("<i", 0)
    meta_bin = ((1 << (depth * 3 + 3)) - 1) // 7 + 1
    ub, first, n_ch, cb, ce, lin = (summ[k] for k in ("bins", "first", "n_chunks", "chunk_beg", "chunk_end", "lin"))
    n_win = lin.size
    if bai:
        idx = np.maximum.accumulate(np.where(lin != _BIG, np.arange(n_win), -1))
        lin_out = np.where(idx >= 0, lin[np.maximum(idx, 0)], np.uint64(0))
    else:
        idx = np.where(lin != _BIG, np.arange(n_win), n_win)
        idx = np.minimum.accumulate(idx[::-1])[::-1]
        filled = np.concatenate([lin, [np.uint64(0)]])[idx]
        wdx = bin_first_window(ub, depth)
        loff = np.where(wdx < n_win, filled[np.minimum(wdx, n_win - 1)], np.uint64(0))
    chunks = np.empty(2 * cb.size, "<u8")
    chunks[0::2], chunks[1::2] = cb, ce
    blob = [struct.pack("<i", ub.size + bool(pseudo_bin))]
    for k in range(ub.size):
        s, n = int(first[k]), int(n_ch[k])
        blob.append(struct.pack("<Ii", int(ub[k]), n) if bai else struct.pack("<IQi", int(ub[k]), int(loff[k]), n))
        blob.append(chunks[2 * s:2 * (s + n)].tobytes())
    if pseudo_bin:
        blob.append(struct.pack("<Ii", meta_bin, 2) if bai else struct.pack("<IQi", meta_bin, 0, 2))
        blob.append(struct.pack("<QQQQ", summ["vmin"], summ["vmax"], summ["mapped"], summ["unmapped"]))
    if bai:
        blob.append(struct.pack("<i", n_win) + lin_out.astype("<u8").tobytes())
    return b"".join(blob)


def join_piece_summaries(pieces, min_shift=14):
    """One reference's summary (reference_summary's form) from the summaries of the BGZF pieces that hold its records, in file order.  A piece:
    dict(offset = where it starts in the file, lines, run_bin, run_vbeg, run_vend = its maximal runs of consecutive lines of one bin in file
    order, w0, win_min = its window minima from window w0 on), virtual offsets relative to the piece (Engine.lines_index).  The piece's file
    offset << 16 is added; bin_chunks then joins, per bin, the runs whose offsets meet: inside a piece none do (a run is maximal), across a piece
    border the last run of one piece and the first of the next when they share the bin and the pieces abut; shared windows take the minimum."""
    rb, vb, ve = [], [], []
    n_win = max(int(p["w0"]) + int(np.asarray(p["win_min"]).size) for p in pieces)
    lin = np.full(n_win, _BIG, np.uint64)
    for p in pieces:
        base = np.uint64(int(p["offset"]) << 16)
        rb.append(np.asarray(p["run_bin"], np.int64))
        vb.append(np.asarray(p["run_vbeg"], np.uint64) + base)
        ve.append(np.asarray(p["run_vend"], np.uint64) + base)
        wm = np.asarray(p["win_min"], np.uint64)
        w0 = int(p["w0"])
        lin[w0:w0 + wm.size] = np.minimum(lin[w0:w0 + wm.size], np.where(wm == _BIG, _BIG, wm + base))
    rb, vb, ve = np.concatenate(rb), np.concatenate(vb), np.concatenate(ve)
    ub, first, n_ch, cb, ce = bin_chunks(rb, vb, ve)
    return dict(bins=ub, first=first, n_chunks=n_ch, chunk_beg=cb, chunk_end=ce, lin=lin, mapped=sum(int(p["lines"]) for p in pieces), unmapped=0,
                vmin=int(vb.min()), vmax=int(ve.max()))


def csi_from_summaries(n_ref, pieces_of_ref, min_shift=14, depth=5, aux=b"", pseudo_bin=True) -> bytes:
    """the uncompressed .csi of a file made of BGZF pieces, without its records: pieces_of_ref[r] = the summaries of reference r's pieces in
    file order (join_piece_summaries; none: a reference without records).  Byte for byte what index_bytes writes from the records."""
    out = [b"CSI\1", struct.pack("<3i", min_shift, depth, len(aux)), aux, struct.pack("<i", n_ref)]
    for r in range(n_ref):
        ps = [p for p in pieces_of_ref[r] if int(p["lines"])]
        out.append(summary_bytes("csi", join_piece_summaries(ps, min_shift) if ps else None, depth, pseudo_bin))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------------ reading: record starts per reference
def bai_linear_voffsets(bai_path):
    """{reference index: uint64 array of the non-zero virtual offsets of its 16 kb windows} (SAM specification 5.2)"""
    with open(bai_path, "rb") as f:
        buf = f.read()
    if buf[:4] != b"BAI\1":
        raise ValueError("%s is not a BAI file" % bai_path)
    n_ref, = struct.unpack_from("<i", buf, 4)
    o, out = 8, {}
    for r in range(n_ref):
        n_bin, = struct.unpack_from("<i", buf, o)
        o += 4
        for _ in range(n_bin):
            _, n_chunk = struct.unpack_from("<Ii", buf, o)
            o += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", buf, o)
        o += 4
        iv = np.frombuffer(buf, np.uint64, n_intv, o)
        o += 8 * n_intv
        out[r] = np.unique(iv[iv != 0])
    return out


def csi_record_starts(csi_path):
    """the same from a CSI index (hts-specs CSIv1; the file is BGZF-compressed), which has no linear index: every bin's `loffset` and every
    chunk's begin are virtual offsets of record starts of that reference -- the leaf bins (16 kb with the default min_shift) make them as
    dense as a .bai's windows"""
    with open(csi_path, "rb") as f:
        buf = gzip.decompress(f.read())
    if buf[:4] != b"CSI\1":
        raise ValueError("%s is not a CSI file" % csi_path)
    _, depth, l_aux = struct.unpack_from("<3i", buf, 4)
    o = 16 + l_aux
    n_ref, = struct.unpack_from("<i", buf, o)
    o += 4
    meta_bin = ((1 << (depth * 3 + 3)) - 1) // 7 + 1                   # the pseudo-bin with the mapped / unmapped counts
    out = {}
    for r in range(n_ref):
        n_bin, = struct.unpack_from("<i", buf, o)
        o += 4
        starts = []
        for _ in range(n_bin):
            b, loff, n_chunk = struct.unpack_from("<IQi", buf, o)
            o += 16
            if b != meta_bin:
                starts.append(np.array([loff], np.uint64))
                starts.append(np.frombuffer(buf, np.uint64, 2 * n_chunk, o)[0::2])
            o += 16 * n_chunk
        v = np.concatenate(starts) if starts else np.zeros(0, np.uint64)
        out[r] = np.unique(v[v != 0])
    return out

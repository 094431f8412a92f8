"""The gVCF's device writer restated on the host: a BGZF piece made with zlib, and the two reductions of
nc_lines_index -- chunk runs and window minima -- in plain numpy / Python.  The tests compare nanocaller_amd.vcf_write.write_piece and
Engine.lines_index with these, and feed hts_index.csi_from_summaries and gvcf.merge_pieces with pieces made here, so those run without a GPU.
Nothing here calls hts_index: reg2bin and the reductions are written out from the CSIv1 text.
"""
import struct
import zlib

import numpy as np

from nanocaller_amd.bgzf import BGZF_BLOCK, member_table, scan_members

BIG = np.uint64(0xFFFFFFFFFFFFFFFF)


def reg2bin(beg, end, min_shift=14, depth=5):
    """hts-specs CSIv1, reg2bin: 0-based half-open [beg, end)"""
    end -= 1
    s, t = min_shift, ((1 << depth * 3) - 1) // 7
    for lv in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (lv - 1) * 3
    return 0


def members(data: bytes, level=6):
    """-> (the BGZF members of `data` cut every 0xff00 bytes, without an EOF block, as bytes; file offset of every member and, last, the length)"""
    out, foff = [], [0]
    for a in range(0, len(data), BGZF_BLOCK):
        chunk = data[a:a + BGZF_BLOCK]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        pay = z.compress(chunk) + z.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(pay) + 25) + pay +
                   struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        foff.append(foff[-1] + len(out[-1]))
    return b"".join(out), np.asarray(foff, np.int64)


def inflate_members(raw: bytes):
    """every member of `raw` inflated with zlib, its CRC-32 and ISIZE checked -> (the bytes, file offset of every member, inflated offset of every
    member and the total)"""
    out, foff, uoff, o = [], [], [0], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04" and raw[o + 12:o + 16] == b"BC\x02\x00", o
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        data = zlib.decompress(raw[o + 18:o + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        assert crc == zlib.crc32(data) and isize == len(data), o
        out.append(data)
        foff.append(o)
        uoff.append(uoff[-1] + len(data))
        o += bsize
    assert o == len(raw)
    return b"".join(out), np.asarray(foff + [o], np.int64), np.asarray(uoff, np.int64)


def piece_voffsets(q, foff):
    """virtual offsets, relative to the piece, of the bytes q of its text: a byte on a member border is the next member's first"""
    q = np.asarray(q, np.int64)
    return (foff[q // BGZF_BLOCK].astype(np.uint64) << np.uint64(16)) | (q % BGZF_BLOCK).astype(np.uint64)


def lines_index(beg, end, line_off, foff, min_shift=14, depth=5):
    """the summary Engine.lines_index gives for a piece: line_off [n + 1] relative to the piece's text, foff = members() offsets"""
    beg, end, off = (np.asarray(x, np.int64) for x in (beg, end, line_off))
    n = beg.size
    vb = piece_voffsets(off[:-1], foff)
    ve = np.concatenate([vb[1:], [np.uint64(int(foff[-1]) << 16)]])
    bins = [reg2bin(int(b), int(e), min_shift, depth) for b, e in zip(beg, end)]
    run_bin, run_vbeg, run_vend = [], [], []
    for i in range(n):
        if i == 0 or bins[i] != bins[i - 1]:
            run_bin.append(bins[i])
            run_vbeg.append(vb[i])
            run_vend.append(ve[i])
        else:
            run_vend[-1] = ve[i]
    w0, w1 = int(beg[0]) >> min_shift, int(end.max() - 1) >> min_shift
    win = np.full(w1 - w0 + 1, BIG, np.uint64)
    for i in range(n):
        a, b = (int(beg[i]) >> min_shift) - w0, (int(end[i] - 1) >> min_shift) - w0
        win[a:b + 1] = np.minimum(win[a:b + 1], vb[i])
    return dict(run_bin=np.asarray(run_bin, np.int32), run_vbeg=np.asarray(run_vbeg, np.uint64), run_vend=np.asarray(run_vend, np.uint64), w0=w0, win_min=win)


def write_piece(f, lines, beg, end, min_shift=14, depth=5):
    """vcf_write.write_piece on the host: `lines` (list of bytes) -> the same summary"""
    text = b"".join(lines)
    raw, foff = members(text)
    f.write(raw)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])])
    return dict(lines=len(lines), bytes=len(raw), text_bytes=len(text), members=foff.size - 1, **lines_index(beg, end, off, foff, min_shift, depth))


def file_voffsets(raw: bytes, header_len, line_len):
    """virtual offsets (first byte, byte behind) of the lines of a BGZF file whose text is a header of header_len bytes and then the lines,
    from the file's own members (bgzf.scan_members + member_table).  A position on a member border belongs to the next member; the end of the
    data is the EOF block."""
    coff, clen, isize, _ = scan_members(raw)
    mstart, ooff = member_table(coff, clen, isize)
    assert isize[-1] == 0 and isize[:-1].min() > 0, "one EOF block, at the end"
    u = header_len + np.concatenate([[0], np.cumsum(np.asarray(line_len, np.int64))])
    assert u[-1] == ooff[-1]
    m = np.minimum(np.searchsorted(ooff[1:], u, side="right"), mstart.size - 1)
    v = (mstart[m].astype(np.uint64) << np.uint64(16)) | (u - ooff[m]).astype(np.uint64)
    return v[:-1], v[1:]

"""Test tooling: a BAM index from first principles, in plain Python (SAMv1 sections 4.1, 4.2, 5.2, 5.3; hts-specs CSIv1).

  serial_chain      the record offsets of a BAM's inflated stream, by the chain p -> p + 4 + block_size from behind the header
  records           refID / pos / flag / reference span of those records and their virtual offsets
  build             the index content by brute force from the records; bai_bytes / csi_bytes serialise it
  parse_bai / parse_csi / query / records_of_chunks / overlapping   the region query of section 5.3 over an index FILE, and what it must return

`unmapped_placed`: a record with flag 4 that has a position (an unmapped mate placed with its partner) is indexed under the one base at its pos, in
the bins and in the linear index, as htslib's hts_idx_push does for every record with a refID -- the library's rule.  tests/bamio.py's writer
leaves such records out of both; False reproduces it."""
import struct

import numpy as np

from nanocaller_amd import vcfio

META_BAI = 37450


def members(path):
    """[(file offset, inflated size), ...] of every BGZF member, and the file's size"""
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            si, slen = raw[x:x + 2], struct.unpack_from("<H", raw, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", raw, x + 4)[0] + 1
            x += 4 + slen
        out.append((o, struct.unpack_from("<I", raw, o + bsize - 4)[0]))
        o += bsize
    return out, len(raw)


def header_len(stream):
    assert stream[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", stream, 4)
    n_ref, = struct.unpack_from("<i", stream, 8 + l_text)
    o, refs = 12 + l_text, []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, o)
        refs.append((stream[o + 4:o + 4 + l_name - 1].decode(), struct.unpack_from("<i", stream, o + 4 + l_name)[0]))
        o += 8 + l_name
    return o, refs


def serial_chain(path):
    """-> (inflated stream, reference list, offsets of all record starts)"""
    stream = vcfio.bgzf_read(path)
    p, refs = header_len(stream)
    offs = []
    while p < len(stream):
        bs, = struct.unpack_from("<i", stream, p)
        assert bs >= 32 and p + 4 + bs <= len(stream)
        offs.append(p)
        p += 4 + bs
    assert p == len(stream)
    return stream, refs, offs


class Voff:
    """stream offset <-> virtual offset; a position on a member boundary belongs to the first member that starts there"""

    def __init__(self, path):
        mem, self.file_size = members(path)
        self.foff = [m[0] for m in mem] + [self.file_size]
        self.ooff = [0]
        for m in mem:
            self.ooff.append(self.ooff[-1] + m[1])

    def of(self, x):
        import bisect
        k = bisect.bisect_left(self.ooff, x)
        if k < len(self.ooff) and self.ooff[k] == x:
            return self.foff[min(k, len(self.foff) - 1)] << 16
        return self.foff[k - 1] << 16 | (x - self.ooff[k - 1])

    def stream(self, v):
        return self.ooff[self.foff.index(v >> 16)] + (v & 0xffff)


def records(path):
    """-> (stream, refs, list of dict(off, refid, pos, flag, beg, end, vbeg, vend)): [beg, end) = the 0-based span the record is indexed under"""
    stream, refs, offs = serial_chain(path)
    vo = Voff(path)
    out = []
    for p in offs:
        bs, refid, pos, l_name, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", stream, p)
        c0 = p + 36 + l_name
        cig = struct.unpack_from("<%dI" % n_cig, stream, c0)
        if n_cig == 2 and cig[0] & 15 == 4 and cig[0] >> 4 == l_seq and cig[1] & 15 == 3:      # the real CIGAR is in the CG tag (4.2.2)
            a, e = c0 + 4 * n_cig + (l_seq + 1) // 2 + l_seq, p + 4 + bs
            k = stream.find(b"CGBI", a, e)
            if k >= 0:
                n, = struct.unpack_from("<I", stream, k + 4)
                cig = struct.unpack_from("<%dI" % n, stream, k + 8)
        rlen = sum(c >> 4 for c in cig if c & 15 in (0, 2, 3, 7, 8))
        beg = max(pos, 0)
        end = pos + (1 if (flag & 4) or rlen <= 0 else rlen)
        out.append(dict(off=p, refid=refid, pos=pos, flag=flag, beg=beg, end=max(end, beg + 1), vbeg=vo.of(p), vend=vo.of(p + 4 + bs)))
    return stream, refs, out


def reg2bin(beg, end, min_shift=14, depth=5):
    end -= 1
    s, t = min_shift, ((1 << (depth * 3)) - 1) // 7
    for lv in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << ((lv - 1) * 3)
    return 0


def build(refs, recs, min_shift=14, depth=5, unmapped_placed=True):
    """brute force -> dict(refs=[dict(bins={bin: [[vbeg, vend], ...]}, lin={window: voffset}, meta=(ref_beg, ref_end, n_mapped, n_unmapped) or
    None)], n_no_coor)"""
    out = [dict(bins={}, lin={}, meta=None) for _ in refs]
    n_no_coor = 0
    for r in recs:
        if r["refid"] < 0:
            n_no_coor += 1
            continue
        d = out[r["refid"]]
        m = d["meta"] or (r["vbeg"], r["vend"], 0, 0)
        un = bool(r["flag"] & 4)
        d["meta"] = (min(m[0], r["vbeg"]), max(m[1], r["vend"]), m[2] + (not un), m[3] + un)
        if un and not unmapped_placed:
            continue
        ch = d["bins"].setdefault(reg2bin(r["beg"], r["end"], min_shift, depth), [])
        if ch and ch[-1][1] == r["vbeg"]:
            ch[-1][1] = r["vend"]                                        # adjacent records of a bin: one chunk
        else:
            ch.append([r["vbeg"], r["vend"]])
        for w in range(r["beg"] >> min_shift, ((r["end"] - 1) >> min_shift) + 1):
            d["lin"][w] = min(d["lin"].get(w, r["vbeg"]), r["vbeg"])
    return dict(refs=out, n_no_coor=n_no_coor, min_shift=min_shift, depth=depth)


def linear_filled(lin):
    """the .bai linear index: an empty window takes the offset of the window before it (0 in front of the first)"""
    arr, last = [], 0
    for k in range((max(lin) + 1) if lin else 0):
        last = lin.get(k, last)
        arr.append(last)
    return arr


def bai_bytes(ix, pseudo_bin=True):
    out = b"BAI\1" + struct.pack("<i", len(ix["refs"]))
    for d in ix["refs"]:
        n_bin = len(d["bins"]) + (1 if pseudo_bin and d["meta"] else 0)
        out += struct.pack("<i", n_bin)
        for b in sorted(d["bins"]):
            out += struct.pack("<Ii", b, len(d["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in d["bins"][b])
        if pseudo_bin and d["meta"]:
            out += struct.pack("<Ii", META_BAI, 2) + struct.pack("<QQQQ", *d["meta"])
        lin = linear_filled(d["lin"])
        out += struct.pack("<i", len(lin)) + b"".join(struct.pack("<Q", v) for v in lin)
    return out + struct.pack("<Q", ix["n_no_coor"])


def _bin_first_window(b, depth):
    lv, t = 0, 0
    while b >= t + (1 << (3 * lv)):
        t += 1 << (3 * lv)
        lv += 1
    return (b - t) << (3 * (depth - lv))


def csi_bytes(ix, pseudo_bin=True):
    """uncompressed CSI; loffset = the linear index at the bin's first window, an empty window taking the next one's"""
    ms, depth = ix["min_shift"], ix["depth"]
    meta_bin = ((1 << (depth * 3 + 3)) - 1) // 7 + 1
    out = b"CSI\1" + struct.pack("<3i", ms, depth, 0) + struct.pack("<i", len(ix["refs"]))
    for d in ix["refs"]:
        if not d["bins"] and not (pseudo_bin and d["meta"]):
            out += struct.pack("<i", 0)
            continue
        n_win = (max(d["lin"]) + 1) if d["lin"] else 0
        lin = [d["lin"].get(k) for k in range(n_win)] + [None]
        for k in range(n_win - 1, -1, -1):
            if lin[k] is None:
                lin[k] = lin[k + 1]
        out += struct.pack("<i", len(d["bins"]) + (1 if pseudo_bin and d["meta"] else 0))
        for b in sorted(d["bins"]):
            w = _bin_first_window(b, depth)
            loff = lin[w] if w < n_win and lin[w] is not None else 0
            out += struct.pack("<IQi", b, loff, len(d["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in d["bins"][b])
        if pseudo_bin and d["meta"]:
            out += struct.pack("<IQi", meta_bin, 0, 2) + struct.pack("<QQQQ", *d["meta"])
    return out + struct.pack("<Q", ix["n_no_coor"])


# ------------------------------------------------------------------------------------------------------------ reading an index file, and the query
def parse_bai(buf):
    assert buf[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", buf, 4)
    o, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", buf, o)
        o += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, n_ch = struct.unpack_from("<Ii", buf, o)
            o += 8
            ch = [list(struct.unpack_from("<QQ", buf, o + 16 * k)) for k in range(n_ch)]
            o += 16 * n_ch
            if b == META_BAI:
                meta = tuple(ch[0] + ch[1])
            else:
                bins[b] = ch
        n_intv, = struct.unpack_from("<i", buf, o)
        lin = list(struct.unpack_from("<%dQ" % n_intv, buf, o + 4))
        o += 4 + 8 * n_intv
        refs.append(dict(bins=bins, lin=lin, meta=meta))
    n_no_coor = struct.unpack_from("<Q", buf, o)[0] if o + 8 <= len(buf) else None
    return dict(kind="bai", refs=refs, n_no_coor=n_no_coor, min_shift=14, depth=5)


def parse_csi(buf):
    """buf: the INFLATED content of a .csi"""
    assert buf[:4] == b"CSI\1"
    ms, depth, l_aux = struct.unpack_from("<3i", buf, 4)
    o = 16 + l_aux
    n_ref, = struct.unpack_from("<i", buf, o)
    o += 4
    meta_bin = ((1 << (depth * 3 + 3)) - 1) // 7 + 1
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", buf, o)
        o += 4
        bins, loff, meta = {}, {}, None
        for _ in range(n_bin):
            b, lo, n_ch = struct.unpack_from("<IQi", buf, o)
            o += 16
            ch = [list(struct.unpack_from("<QQ", buf, o + 16 * k)) for k in range(n_ch)]
            o += 16 * n_ch
            if b == meta_bin:
                meta = tuple(ch[0] + ch[1])
            else:
                bins[b], loff[b] = ch, lo
        refs.append(dict(bins=bins, loff=loff, meta=meta))
    n_no_coor = struct.unpack_from("<Q", buf, o)[0] if o + 8 <= len(buf) else None
    return dict(kind="csi", refs=refs, n_no_coor=n_no_coor, min_shift=ms, depth=depth)


def reg2bins(beg, end, min_shift=14, depth=5):
    """SAMv1 5.3 / CSIv1: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out, s, t = [], min_shift + depth * 3, 0
    for lv in range(depth + 1):
        out += list(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << (lv * 3)
    return out


def query(ix, tid, beg, end):
    """the chunks a reader has to scan for [beg, end) (0-based, half open): those of the region's bins that do not end at or before the
    linear-index cut-off"""
    d = ix["refs"][tid]
    ms, depth = ix["min_shift"], ix["depth"]
    if ix["kind"] == "bai":
        w = beg >> ms
        min_off = d["lin"][w] if w < len(d["lin"]) else (d["lin"][-1] if d["lin"] else 0)
    else:                                                                # the loffset of the smallest bin around `beg` that the index has
        b = ((1 << (depth * 3)) - 1) // 7 + (beg >> ms)
        min_off = 0
        while True:
            if b in d["loff"]:
                min_off = d["loff"][b]
                break
            if b == 0:
                break
            b = (b - 1) >> 3
    chunks = []
    for b in reg2bins(beg, end, ms, depth):
        chunks += [c for c in d["bins"].get(b, []) if c[1] > min_off]
    return sorted(chunks)


def records_of_chunks(vo, stream, chunks):
    """the record offsets a reader meets scanning the chunks"""
    got = set()
    for vb, ve in chunks:
        p, e = vo.stream(vb), vo.stream(ve)
        while p < e:
            got.add(p)
            p += 4 + struct.unpack_from("<i", stream, p)[0]
        assert p == e
    return got


def overlapping(recs, tid, beg, end, unmapped_placed=True):
    return {r["off"] for r in recs if r["refid"] == tid and r["beg"] < end and r["end"] > beg and (unmapped_placed or not r["flag"] & 4)}


def check_queries(path, index_file, seed=0, n=200, tids=None):
    """200 seeded random regions per reference + the contig ends: the query over `index_file`, its chunks read and the records filtered by
    overlap, returns exactly the brute-force overlap set (tids: only these references)"""
    import gzip
    stream, refs, recs = records(path)
    vo = Voff(path)
    raw = open(index_file, "rb").read()
    ix = parse_csi(gzip.decompress(raw)) if index_file.endswith(".csi") else parse_bai(raw)
    rng = np.random.default_rng(seed)
    by_off = {r["off"]: r for r in recs}
    for tid, (_, ln) in enumerate(refs):
        if tids is not None and tid not in tids:
            continue
        regions = [(0, 1), (max(0, ln - 1), ln), (0, ln)]
        for _ in range(n):
            a = int(rng.integers(0, max(1, ln)))
            regions.append((a, min(ln, a + int(rng.integers(1, 1 + max(1, ln // 4))))))
        for beg, end in regions:
            seen = records_of_chunks(vo, stream, query(ix, tid, beg, end))
            got = {o for o in seen if by_off[o]["refid"] == tid and by_off[o]["beg"] < end and by_off[o]["end"] > beg}
            assert got == overlapping(recs, tid, beg, end), (tid, beg, end)
    return ix

"""BAM records with a MAPQ field for the weighted phaser's tests: bamio.write_bam's record dicts plus `mapq` (default 60).  bamio.py writes
MAPQ 60 everywhere and stays as it is; the BGZF writer, the bins and the .csi writer are its own.
`record_bytes` is one record as it stands in the inflated stream (block_size first): the tests also hand such bytes to the kernel directly."""
import struct

import numpy as np

import bamio

_OPS = "MIDNSHP=X"


def _aux(tags):
    out = b""
    for k, v in tags.items():
        if isinstance(v, (list, tuple)):                                 # B,I (the CG tag)
            out += k.encode() + b"BI" + struct.pack("<I", len(v)) + b"".join(struct.pack("<I", x) for x in v)
        elif isinstance(v, str):
            out += k.encode() + b"Z" + v.encode() + b"\0"
        elif 0 <= v < 256:
            out += k.encode() + b"C" + struct.pack("<B", v)
        else:
            out += k.encode() + b"i" + struct.pack("<i", v)
    return out


def ref_span(cigar):
    return sum(n for op, n in cigar if op in "MDN=X")


def record_bytes(r, l_seq=None):
    """one alignment record: dict(name, flag, pos0, cigar [(op, len)], seq str, optional mapq, qual (bytes of len(seq); None: 0xff, absent),
    tags, tid).  l_seq: the value written into the l_seq field when it is to differ from len(seq) (a crafted record)"""
    name = r["name"].encode() + b"\0"
    seq = r["seq"]
    nib = bamio._NT16_LUT[np.frombuffer(seq.encode("ascii"), np.uint8)]
    if nib.size & 1:
        nib = np.append(nib, np.uint8(0))
    packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    qual = r["qual"] if r.get("qual") is not None else b"\xff" * len(seq)
    assert len(qual) == len(seq)
    pos0 = r["pos0"]
    body = struct.pack("<iiBBHHHiiii", r.get("tid", 0), pos0, len(name), r.get("mapq", 60), bamio.reg2bin(pos0, pos0 + max(1, ref_span(r["cigar"]))),
                       len(r["cigar"]), r["flag"], len(seq) if l_seq is None else l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", (n << 4) | _OPS.index(op)) for op, n in r["cigar"]) + packed + bytes(qual) + _aux(r.get("tags", {}))
    return struct.pack("<i", len(body)) + body


def record_stream(records):
    """the records back to back as the inflated stream holds them -> (uint8 array, int64 offsets of the records)"""
    chunks = [record_bytes(r) for r in records]
    off = np.zeros(len(chunks), np.int64)
    if len(chunks) > 1:
        off[1:] = np.cumsum([len(c) for c in chunks[:-1]])
    return np.frombuffer(b"".join(chunks), np.uint8).copy(), off


def write_bam(path, chrom, length, records, level=6):
    """coordinate-sorted records of one contig -> path, path.bai and path.csi"""
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n" % (chrom, length)
    w = bamio.BgzfWriter(path, level=level)
    w.write(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", len(chrom) + 1) + chrom.encode() + b"\0"
            + struct.pack("<i", length))
    w.flush()
    lin, spans = {}, []
    for r in records:
        beg, end = r["pos0"], r["pos0"] + max(1, ref_span(r["cigar"]))
        voff = w.tell()
        w.write(record_bytes(r))
        if not r["flag"] & 4:
            for win in range(beg >> 14, ((end - 1) >> 14) + 1):
                lin.setdefault(win, voff)
            spans.append((beg, end, voff, w.tell()))
    w.close()
    bamio.write_bam_csi(path + ".csi", [spans])
    with open(path + ".bai", "wb") as f:
        n_intv = (max(lin) + 1) if lin else 0
        arr, last = [], 0
        for k in range(n_intv):                                          # (empty windows take the previous offset, as samtools writes them)
            last = lin.get(k, last)
            arr.append(last)
        f.write(b"BAI\1" + struct.pack("<i", 1) + struct.pack("<i", 0) + struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", v) for v in arr))

"""The haplotagged BAM writer (nanocaller_amd/bam_write.py, csrc/nc_bamwrite.hip): the host pieces (header + @PG, gzip framing, CSI,
the PS type rule) on the CPU; on the GPU the device deflate against zlib, the re-tagged record stream byte for byte against a Python
restatement of the rule, region selection, a round trip through both readers, and phase_run's phased BAM end to end."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import bamio
from test_inflate_device import _run as _inflate_device

OPS = "MIDNSHP=X"


# ------------------------------------------------------------------------------------------------------------ test records
def aux(tag, ty, val):
    t = tag.encode() + ty.encode()
    if ty in "cCsSiIf":
        return t + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[ty], val)
    if ty == "A":
        return t + val.encode()
    if ty in "ZH":
        return t + val.encode() + b"\0"
    sub, vals = val                                                     # B array
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
    return t + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack("<" + fmt, v) for v in vals)


def record(name, flag, pos0, cigar, seq, qual, auxb, tid=0):
    rlen = sum(n for op, n in cigar if op in "MDN=X")
    nm = name.encode() + b"\0"
    nib = bamio._NT16_LUT[np.frombuffer(seq.encode(), np.uint8)]
    if nib.size & 1:
        nib = np.append(nib, np.uint8(0))
    packed = ((nib[0::2] << 4) | nib[1::2]).astype(np.uint8).tobytes()
    body = struct.pack("<iiBBHHHiiii", tid, pos0, len(nm), 60, bamio.reg2bin(pos0, pos0 + max(1, rlen)), len(cigar), flag, len(seq), -1, -1, 0) + \
        nm + b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for op, n in cigar) + packed + qual + auxb
    return struct.pack("<i", len(body)) + body, rlen


def write_raw_bam(path, refs, recs, text=None):
    """recs: (tid, pos0, rlen, record bytes) in coordinate order -> BAM + CSI (every record indexed, as htslib does)"""
    text = text if text is not None else "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    w = bamio.BgzfWriter(path, level=1)
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, ln in refs:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    w.write(hdr)
    w.flush()
    spans = [[] for _ in refs]
    for tid, pos0, rlen, rb in recs:
        v0 = w.tell()
        w.write(rb)
        spans[tid].append((pos0, pos0 + max(1, rlen), v0, w.tell()))
    w.close()
    bamio.write_bam_csi(path + ".csi", spans)
    return text


def split_aux(rb):
    """(fixed part without block_size, [(tag, field bytes)]) of one record"""
    body = rb[4:]
    l_name, n_cig, l_seq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<i", body, 16)[0]
    a = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    fields, p = [], a
    while p < len(body):
        ty = chr(body[p + 2])
        if ty in "AcC":
            sz = 1
        elif ty in "sS":
            sz = 2
        elif ty in "iIf":
            sz = 4
        elif ty in "ZH":
            sz = body.index(b"\0", p + 3) + 1 - (p + 3)
        else:
            es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[chr(body[p + 3])]
            sz = 5 + struct.unpack_from("<I", body, p + 4)[0] * es
        fields.append((body[p:p + 2], body[p:p + 3 + sz]))
        p += 3 + sz
    return body[:a], fields


def retag_expected(rb, name, table):
    """the rule of DESIGN.md section 13 restated: HP / PS / PC dropped, HP (C) and PS appended where the name is in the table"""
    from nanocaller_amd.bam_write import ps_tag
    fixed, fields = split_aux(rb)
    body = fixed + b"".join(f for t, f in fields if t not in (b"HP", b"PS", b"PC"))
    if name in table:
        hp, ps = table[name]
        body += b"HPC" + bytes([hp]) + ps_tag(ps)
    return struct.pack("<i", len(body)) + body


def bam_records(blob):
    """the records of an inflated BAM -> (header bytes, [record bytes])"""
    l_text, = struct.unpack_from("<i", blob, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", blob, o)
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", blob, o)[0]
    hdr, recs = blob[:o], []
    while o < len(blob):
        bs, = struct.unpack_from("<i", blob, o)
        recs.append(blob[o:o + 4 + bs])
        o += 4 + bs
    return hdr, recs


def ont_quals(rng, n):
    q = np.clip(rng.normal(18, 7, n), 2, 50).astype(np.uint8)
    runs = rng.random(n) < 0.3                                          # ONT qualities come in short runs
    q[1:][runs[1:]] = q[:-1][runs[1:]]
    return q.tobytes()


# ------------------------------------------------------------------------------------------------------------ CPU
def test_ps_type_rule():
    from nanocaller_amd.bam_write import ps_tag
    assert ps_tag(0) == b"PSC\0" and ps_tag(255) == b"PSC\xff"
    assert ps_tag(256) == b"PSS" + struct.pack("<H", 256) and ps_tag(65535) == b"PSS\xff\xff"
    assert ps_tag(65536) == b"PSI" + struct.pack("<I", 65536) and ps_tag(2 ** 31 - 1)[2:3] == b"I"
    assert ps_tag(-1) == b"PSc\xff" and ps_tag(-200)[2:3] == b"s" and ps_tag(-40000)[2:3] == b"i"


def test_header_and_pg():
    from nanocaller_amd.bam_write import add_pg, header_bytes
    t = add_pg("@HD\tVN:1.6\n@SQ\tSN:c\tLN:10\n")
    assert t.endswith("@PG\tID:nanocaller_amd\tPN:nanocaller_amd\n")
    t2 = add_pg("@HD\tVN:1.6\n@PG\tID:minimap2\tPN:minimap2\n@PG\tID:nanocaller_amd\tPN:nanocaller_amd\tPP:minimap2\n@PG\tID:samtools\tPN:samtools\tPP:nanocaller_amd\n")
    last = t2.rstrip("\n").split("\n")[-1]
    assert last == "@PG\tID:nanocaller_amd.1\tPN:nanocaller_amd\tPP:samtools"
    assert t2.count("\n") == 5
    hb = header_bytes(t, [("c", 10), ("d", 7)])
    assert hb[:4] == b"BAM\1" and struct.unpack_from("<i", hb, 4)[0] == len(t) and hb.endswith(b"\2\0\0\0d\0\7\0\0\0")


def test_header_read_back(tmp_path):
    from nanocaller_amd.bam_write import read_bam_header
    p = str(tmp_path / "h.bam")
    text = write_raw_bam(p, [("c1", 1000), ("c2", 500)], [])
    assert read_bam_header(p) == (text, [("c1", 1000), ("c2", 500)])


def test_gzip_member_assembly():
    from nanocaller_amd.bam_write import BGZF_EOF, bgzf_members, member_spans
    rng = np.random.default_rng(1)
    data = rng.integers(0, 4, 150_000).astype(np.uint8).tobytes()
    off, ln = member_spans(len(data))
    assert ln.tolist() == [0xff00, 0xff00, len(data) - 2 * 0xff00] and off.tolist() == [0, 0xff00, 2 * 0xff00]
    pays, crcs = [], []
    for o, n in zip(off, ln):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        pays.append(c.compress(data[o:o + n]) + c.flush())
        crcs.append(zlib.crc32(data[o:o + n]))
    blob = bgzf_members(pays, crcs, ln)
    assert blob.endswith(BGZF_EOF) and gzip.decompress(blob) == data
    o = 0
    for p in pays:                                                      # every member: BC field with BSIZE, then CRC and ISIZE
        assert blob[o:o + 4] == b"\x1f\x8b\x08\x04" and blob[o + 12:o + 16] == b"BC\2\0"
        assert struct.unpack_from("<H", blob, o + 16)[0] + 1 == len(p) + 26
        o += len(p) + 26
    assert len(blob) == o + 28


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_csi_equals_bamio_writer(tmp_path, seed):
    from nanocaller_amd.bam_write import csi_index, voffsets
    rng = np.random.default_rng(seed)
    n = 3000
    beg = np.sort(rng.integers(0, 2_000_000, n))
    beg[100:120] = beg[100]                                              # equal starts
    rl = rng.integers(1, 60_000, n)
    rl[::7] = rng.integers(1, 50, rl[::7].size)
    size = rng.integers(100, 40_000, n)                                 # records that span members
    pos = np.concatenate([[0], np.cumsum(size)])
    foff = np.concatenate([[0], np.cumsum(rng.integers(10_000, 30_000, pos[-1] // 0xff00 + 3))])
    hl = 3                                                              # header members in front
    vb, ve = voffsets(pos[:-1], hl, foff), voffsets(pos[1:], hl, foff)
    refs = 3
    tid = seed % refs
    got = csi_index(refs, tid, beg, beg + rl, vb, ve)
    spans = [[] for _ in range(refs)]
    spans[tid] = [(int(a), int(a + r), int(u), int(v)) for a, r, u, v in zip(beg, rl, vb, ve)]
    p = str(tmp_path / "x.csi")
    bamio.write_bam_csi(p, spans)
    assert got == gzip.decompress(open(p, "rb").read())
    assert csi_index(2, 0, beg[:0], beg[:0], vb[:0], ve[:0]) == b"CSI\1" + struct.pack("<3i", 14, 5, 0) + struct.pack("<iiiQ", 2, 0, 0, 0)


def test_voffsets_at_member_boundaries():
    from nanocaller_amd.bam_write import voffsets
    foff = np.array([0, 100, 250, 400], np.int64)
    v = voffsets(np.array([0, 5, 0xff00 - 1, 0xff00, 2 * 0xff00]), 1, foff)
    assert v.tolist() == [100 << 16, (100 << 16) | 5, (100 << 16) | 0xfeff, 250 << 16, 400 << 16]


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


def _deflate(eng, members):
    import torch
    from nanocaller_amd.bam_write import PAYLOAD_SLOT, deflate_members
    blob = b"".join(members)
    ln = np.array([len(m) for m in members], np.int32)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    d = torch.from_numpy(np.frombuffer(blob + b"\0" * 8, np.uint8).copy()).to(eng.device)
    pay, poff, clen, crc, st, _ = deflate_members(eng, d, off, ln)
    torch.cuda.synchronize()
    assert int(st.count_nonzero().item()) == 0
    c, cr, p = clen.cpu().numpy(), crc.cpu().numpy().view(np.uint32), pay.cpu().numpy()
    return [p[k * PAYLOAD_SLOT:k * PAYLOAD_SLOT + int(c[k])].tobytes() for k in range(len(members))], cr


def _zlib1(m):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return len(c.compress(m) + c.flush())


def _record_stream(rng, n, quals):
    out = []
    for k in range(n):
        L = int(rng.integers(200, 3000))
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, L))
        q = ont_quals(rng, L) if quals else b"\xff" * L
        rb, _ = record("read%06d" % k, 0, 1000 + 37 * k, [("M", L)], seq, q, aux("NM", "i", 3) + aux("RG", "Z", "grp1"))
        out.append(rb)
    return b"".join(out)


@pytest.mark.gpu
def test_deflate_member_classes(eng):
    rng = np.random.default_rng(3)
    ont = _record_stream(rng, 300, True)
    plain = _record_stream(rng, 300, False)
    text = ("@SQ\tSN:chr%d\tLN:%d\n" * 3000 % tuple(v for k in range(3000) for v in (k, 1000 + k))).encode()
    classes = dict(one=[b"\x07"], same=[b"\x41" * 0xff00], rand=[rng.integers(0, 256, 0xff00).astype(np.uint8).tobytes()],
                   text=[text[i:i + 0xff00] for i in range(0, 3 * 0xff00, 0xff00)],
                   plain=[plain[i:i + 0xff00] for i in range(0, 8 * 0xff00, 0xff00)],
                   ont=[ont[i:i + 0xff00] for i in range(0, 8 * 0xff00, 0xff00)],
                   edge=[ont[:0xff00 - 1], ont[5:5 + 0xff00], b"", b"ab", b"abcabcabcabcabcabc"])
    ratio = {}
    for name, members in classes.items():
        pays, crcs = _deflate(eng, members)
        for m, p, c in zip(members, pays, crcs):
            assert zlib.decompress(p, -15) == m, name
            assert int(c) == zlib.crc32(m), name
            assert len(p) <= len(m) + 5
        out, ooff, st = _inflate_device(pays, [len(m) for m in members])     # the writer's blocks through the reader's tables: both ours
        assert not st.any(), name
        for k, m in enumerate(members):
            assert out[ooff[k]:ooff[k] + len(m)].tobytes() == m, name
            assert out[ooff[k] + len(m):ooff[k] + len(m) + 3].tolist() == [0xEE] * 3, name
        ratio[name] = sum(map(len, pays)) / max(1, sum(_zlib1(m) for m in members))
    print("payload / zlib level 1:", {k: round(v, 3) for k, v in ratio.items()})
    pays, _ = _deflate(eng, classes["rand"])
    assert pays[0][0] & 7 == 1                                          # stored: incompressible bytes
    assert len(_deflate(eng, classes["same"])[0][0]) < 0xff00 // 10      # (measured 3,483 bytes: segments re-start matches)
    assert ratio["ont"] <= 1.15 and ratio["plain"] <= 1.5


def _retag_world(tmp_path, n=600, seed=5):
    """records of every aux type, old HP / PS / PC of several types, secondary / supplementary / unmapped, two contigs"""
    rng = np.random.default_rng(seed)
    refs = [("c1", 400_000), ("c2", 300_000)]
    recs, names, infos = [], [], []
    pos = 1000
    for k in range(n):
        tid = 0 if k < n * 2 // 3 else 1
        if k == n * 2 // 3:
            pos = 500
        pos += int(rng.integers(0, 600))
        name = "r%04d" % (k % (n - 50))                                 # some names twice: secondary / supplementary alignments
        L = int(rng.integers(50, 4000))
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, L))
        flag = [0, 16, 256, 2048, 1024, 512, 4][k % 7] if k % 5 == 0 else int(rng.choice([0, 16]))
        cig = [("S", 5), ("M", L - 5)] if flag != 4 else []
        ab = aux("NM", "C", 3) + aux("XA", "A", "q") + aux("xc", "c", -5) + aux("xs", "s", -300) + aux("xS", "S", 60000)
        ab += aux("xi", "i", -70000) + aux("xI", "I", 3_000_000_000) + aux("xf", "f", 1.5) + aux("RG", "Z", "g%d" % (k % 3)) + aux("xh", "H", "1AE3")
        ab += aux("ML", "B", ("C", list(rng.integers(0, 255, 20)))) + aux("xb", "B", ("s", [-1, 2, -3]))
        if k % 3 == 0:
            ab = aux("HP", ["C", "i", "s", "c"][k % 4], 1 + k % 2) + ab
        if k % 4 == 0:
            ab += aux("PS", ["i", "I", "S", "C"][(k // 4) % 4], 100 + k % 100)
        if k % 6 == 0:
            ab += aux("PC", ["i", "C"][k % 2], 20)
        if k % 11 == 0:                                                 # SAMv1 4.2.2: placeholder CIGAR, the real one in CG
            ab += aux("CG", "B", ("I", [(L - 5) << 4 | 0, 5 << 4 | 4]))
            cig = [("S", L), ("N", L - 5)]
        q = ont_quals(rng, L) if k % 9 else b"\xff" * L
        rb, rlen = record(name, flag, pos, cig, seq, q, ab, tid)
        recs.append((tid, pos, rlen, rb))
        names.append(name)
    p = str(tmp_path / "in.bam")
    text = write_raw_bam(p, refs, recs, text="@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:400000\n@SQ\tSN:c2\tLN:300000\n@PG\tID:minimap2\tPN:minimap2\n")
    uniq = sorted(set(names))
    pick = rng.random(len(uniq)) < 0.5
    ps_vals = rng.choice([7, 255, 256, 65535, 65536, 123_456_789], len(uniq))
    table = {nm: (int(1 + (i % 2)), int(ps_vals[i])) for i, nm in enumerate(uniq) if pick[i]}
    from nanocaller_amd.phase import name_hash
    keys = sorted(table)
    tags = dict(hash=name_hash(keys), hp=np.array([table[k][0] for k in keys], np.uint8), ps=np.array([table[k][1] for k in keys], np.int32))
    return p, refs, recs, names, text, table, tags


@pytest.mark.gpu
def test_retag_exact(eng, tmp_path):
    from nanocaller_amd.bam_write import add_pg, header_bytes, write_haplotagged_bam
    from nanocaller_amd.device_bam import release
    p, refs, recs, names, text, table, tags = _retag_world(tmp_path)
    out = str(tmp_path / "out.bam")
    release()
    r = write_haplotagged_bam(p, "c1", tags, out)
    blob = open(out, "rb").read()
    assert blob.endswith(bamio._BGZF_EOF)
    hdr, got = bam_records(gzip.decompress(blob))
    assert hdr == header_bytes(add_pg(text), refs)
    assert hdr[8:8 + len(text) + 60].decode().split("\n")[-2] == "@PG\tID:nanocaller_amd\tPN:nanocaller_amd\tPP:minimap2"
    want = [retag_expected(rb, nm, table) for (tid, _, _, rb), nm in zip(recs, names) if tid == 0]
    assert len(got) == len(want) == r["records"] and got == want
    assert b"".join(got) == b"".join(want)
    # the header in its own member(s), the records in members of exactly 0xff00 bytes
    sizes, o = [], 0
    while o < len(blob) - 28:
        bsize = struct.unpack_from("<H", blob, o + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", blob, o + bsize - 4)[0])
        o += bsize
    assert sizes[0] == len(hdr) and all(s == 0xff00 for s in sizes[1:-1]) and len(sizes) == r["members"]
    print("retag: %d records, %d tagged, %d members, ms %s" % (r["records"], r["tagged"], r["members"], r["ms"]))


@pytest.mark.gpu
def test_region_and_round_trip(eng, tmp_path):
    from nanocaller_amd.bam import read_bam
    from nanocaller_amd.bam_write import csi_index, write_haplotagged_bam
    from nanocaller_amd.device_bam import M_FLAG, M_HAP, M_POS, M_PS, DeviceBam, release
    from nanocaller_amd.phase import tags_for_names
    p, refs, recs, names, text, table, tags = _retag_world(tmp_path, seed=8)
    c1 = [(i, r) for i, r in enumerate(recs) if r[0] == 0]
    lo, hi = c1[len(c1) // 3][1][1] + 10, c1[2 * len(c1) // 3][1][1] + 10     # 1-based bounds inside the contig
    # placed-unmapped records right at both bounds
    extra = []
    for b in (lo - 1, hi - 1, lo - 2, hi):
        rb, _ = record("unm%d" % b, 4, b, [], "ACGT", b"\x10" * 4, aux("PS", "i", 5))
        extra.append((0, b, 0, rb))
    recs2 = sorted(recs + extra, key=lambda r: (r[0], r[1]))
    names2 = [struct.unpack_from("<%ds" % (r[3][12] - 1), r[3], 36)[0].decode() for r in recs2]
    bam2 = str(tmp_path / "in2.bam")
    write_raw_bam(bam2, refs, recs2, text=text)
    out = str(tmp_path / "reg.bam")
    release()
    res = write_haplotagged_bam(bam2, "c1", str(_save(tmp_path, tags)), out, start=lo, end=hi)
    _, got = bam_records(gzip.decompress(open(out, "rb").read()))
    sel = [(r, nm) for r, nm in zip(recs2, names2) if r[0] == 0 and r[1] < hi and r[1] + max(1, r[2]) > lo - 1]
    assert {"unm%d" % (lo - 1), "unm%d" % (hi - 1)} <= {nm for _, nm in sel} and "unm%d" % (lo - 2) not in {nm for _, nm in sel}
    assert "unm%d" % hi not in {nm for _, nm in sel}
    assert got == [retag_expected(r[3], nm, table) for r, nm in sel] and res["records"] == len(sel)
    # the index: bamio's writer on the written records' spans and virtual offsets
    blob = open(out, "rb").read()
    spans, voffs = [], _record_voffsets(blob)
    for (r, nm), (vb, ve) in zip(sel, voffs):
        spans.append((r[1], r[1] + max(1, r[2]), vb, ve))
    exp = str(tmp_path / "exp.csi")
    bamio.write_bam_csi(exp, [spans, []])
    assert gzip.decompress(open(out + ".csi", "rb").read()) == gzip.decompress(open(exp, "rb").read())
    assert csi_index(2, 0, [s[0] for s in spans], [s[1] for s in spans], [s[2] for s in spans], [s[3] for s in spans]) == \
        gzip.decompress(open(exp, "rb").read())
    # the host reader and the device ingest read it back: the input's alignments, HP / PS from the table
    fa = str(tmp_path / "r.fa")
    bamio.write_fasta(fa, "c1", "".join("ACGT"[i] for i in np.random.default_rng(0).integers(0, 4, 400_000)),
                      extra=[("c2", "A" * 300_000)])
    w = read_bam(out, fa, "c1", lo, hi)
    mapped = [nm for r, nm in sel if not r[3][18] & 0x4 and r[2] > 0]
    hp, ps = tags_for_names(list(w.names), _save(tmp_path, tags))
    assert list(w.names) == mapped and np.array_equal(w.meta["hap"], hp) and np.array_equal(w.meta["ps"], ps)
    db = DeviceBam(out, contigs=["c1"]).load()
    hp2, ps2 = tags_for_names([nm for _, nm in sel], _save(tmp_path, tags))
    assert db.n_rec == len(sel)
    assert np.array_equal(db.meta[M_POS], [r[1] for r, _ in sel]) and np.array_equal(db.meta[M_FLAG] & 0xffff, [struct.unpack_from("<H", r[3], 18)[0] for r, _ in sel])
    assert np.array_equal(db.meta[M_HAP], hp2) and np.array_equal(db.meta[M_PS], ps2)


def _save(tmp_path, tags):
    from nanocaller_amd.phase import save_haplotags
    p = str(tmp_path / "tags.npz")
    if not os.path.exists(p):
        save_haplotags(p, tags)
    return p


def _record_voffsets(blob):
    """(begin, end) virtual offsets of every record of a BGZF BAM, from its members, as htslib's bgzf_tell gives them while writing: a
    position at the end of a FULL member is the next member's start, any other position lies in the member that holds its bytes"""
    data, co, mo, isz, o = [], [], [], [], 0
    while o < len(blob):
        bsize = struct.unpack_from("<H", blob, o + 16)[0] + 1
        m = zlib.decompress(blob[o + 18:o + bsize - 8], -15)
        co.append(o)
        mo.append(sum(map(len, data)))
        isz.append(len(m))
        data.append(m)
        o += bsize
    raw = b"".join(data)
    live = [k for k in range(len(co)) if isz[k]]

    def v(q):
        k = live[int(np.searchsorted([mo[j] for j in live], q, side="right")) - 1]
        if q - mo[k] == isz[k] == 0xff00:
            return co[k + 1] << 16
        return (co[k] << 16) | (q - mo[k])
    hdr, recs = bam_records(raw)
    out, q = [], len(hdr)
    for rb in recs:
        out.append((v(q), v(q + len(rb))))
        q += len(rb)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ingest", ["0", "1"])
def test_phase_run_writes_the_phased_bam(tmp_path_factory, monkeypatch, ingest):
    """phaser='device' + phased_bam=True: <contig>.phased.bam + .csi; mode 'indels' on that BAM gives the indel VCF of the table route"""
    from nanocaller_amd import indelCaller
    from nanocaller_amd.phase import tags_for_names
    from test_phase_gpu import _indels, _snp_vcf
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
    monkeypatch.delenv("NC_PHASED_BAM", raising=False)
    d = str(tmp_path_factory.mktemp("pbam" + ingest))
    w = bamio.make_pass2_world(seed=41, length=150_000, depth=28)
    recs = bamio.world_to_records(w, None)
    untagged, fa = os.path.join(d, "untagged.bam"), os.path.join(d, "r.fa")
    bamio.write_bam(untagged, w.chrom, w.length, [dict(r, tags={}) for r in recs], write_csi=True)
    bamio.write_fasta(fa, w.chrom, w.ref)
    snp_vcf = _snp_vcf(untagged, fa, w.chrom, w.length, os.path.join(d, "snp"))
    _, table_route = _indels(untagged, fa, w.chrom, w.length, os.path.join(d, "dev"), "all", snp_vcf, phaser="device", phased_bam=True)
    ph = os.path.join(d, "dev", "intermediate_phase_files")
    bam = os.path.join(ph, "%s.phased.bam" % w.chrom)
    assert os.path.exists(bam) and os.path.exists(bam + ".csi")
    hp, ps = tags_for_names([r["name"] for r in recs], os.path.join(ph, "%s.haplotags.npz" % w.chrom))
    assert (hp > 0).mean() > 0.2
    _, from_bam = _indels(bam, fa, w.chrom, w.length, os.path.join(d, "re"), "indels")
    assert len(from_bam) > 20 and from_bam == table_route
    _, _ = _indels(untagged, fa, w.chrom, w.length, os.path.join(d, "off"), "all", snp_vcf, phaser="device")
    assert not os.path.exists(os.path.join(d, "off", "intermediate_phase_files", "%s.phased.bam" % w.chrom))

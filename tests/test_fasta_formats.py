"""Reference FASTA formats on the host (nanocaller_amd/fasta.py): a bgzip-compressed FASTA reads exactly as its plain twin, through the
.gzi or through the walked member map; only the covering members are inflated; files the readers must not accept are refused with a
message; plain files read as they always did.  Every comparison is exact equality."""
import gzip
import os
import struct

import numpy as np
import pytest

import fastaio
from nanocaller_amd import fasta
from nanocaller_amd._lib import NanoCallerHipError
from nanocaller_amd.bam import read_fasta, read_fasta_bytes


def plain_restated(path, chrom):
    """the plain reader of bam.py, word for word as it stood before .gz paths were told apart"""
    fai = path + ".fai"
    if os.path.exists(fai):
        for line in open(fai):
            f = line.rstrip("\n").split("\t")
            if f[0] == chrom:
                length, offset, lb, lw = int(f[1]), int(f[2]), int(f[3]), int(f[4])
                with open(path, "rb") as fh:
                    fh.seek(offset)
                    raw = fh.read(length + (length // lb + 1) * (lw - lb))
                return raw.replace(b"\n", b"").replace(b"\r", b"")[:length]
        raise KeyError(chrom)
    seq, on = [], False
    for line in open(path):
        if line.startswith(">"):
            if on:
                break
            on = line[1:].split()[0] == chrom
        elif on:
            seq.append(line.strip())
    if not seq:
        raise KeyError(chrom)
    return "".join(seq).encode("ascii")


TWINS = [dict(sizes=(0xff00,), gzi=True), dict(sizes=(0xff00,), gzi=False), dict(sizes=None, gzi=False), dict(sizes=None, gzi=True, levels=(0,)),
         dict(sizes=None, gzi=True, levels=(6, 0, 1, 9))]


def make_twin(fa, rng, sizes, gzi, levels=None):
    """the .gz twin of `fa`; sizes None: irregular members of 1 to 300 bytes"""
    if sizes is None:
        sizes = [int(x) for x in rng.integers(1, 301, 257)]
    return fastaio.bgzip_twin(fa, sizes=sizes, levels=levels, gzi=gzi)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """[(plain path, rows, {name: sequence})]: every line length x terminator, last line full / short, with / without a terminator at the end"""
    root = tmp_path_factory.mktemp("fasta_formats")
    rng = np.random.default_rng(11)
    out = []
    for lb in fastaio.LBS:
        for eol in ("\n", "\r\n"):
            for last_full, last_eol in ((True, False), (False, True)):
                p = str(root / ("lb%d_%s_%d%d.fa" % (lb, "lf" if eol == "\n" else "crlf", last_full, last_eol)))
                rows, seqs = fastaio.write_case_file(p, rng, lb, eol, last_full, last_eol)
                out.append((p, rows, seqs))
    for name, n, lb, eol in (("long", 200_003, 60, "\n"), ("long_crlf", 200_003, 61, "\r\n"), ("single", 5_000, 5_000, "\n")):
        p = str(root / (name + ".fa"))
        contigs = [("head a contig in front", fastaio.random_sequence(rng, 777)), (name + " the long one", fastaio.random_sequence(rng, n))]
        rows = fastaio.write_fasta_lines(p, contigs, lb, eol)
        out.append((p, rows, {h.split()[0]: s for h, s in contigs}))
    return out


def test_plain_reader_unchanged(cases):
    for p, rows, seqs in cases:
        for name, s in seqs.items():
            assert read_fasta_bytes(p, name) == plain_restated(p, name) == s.encode("ascii")
            assert read_fasta(p, name) == s
    # and without a .fai
    p, rows, seqs = cases[0]
    q = p + ".noindex.fa"
    with open(p, "rb") as f, open(q, "wb") as g:
        g.write(f.read())
    for name in seqs:
        assert read_fasta_bytes(q, name) == plain_restated(q, name)


@pytest.mark.parametrize("twin", range(len(TWINS)))
def test_bgzipped_equals_plain(cases, twin):
    rng = np.random.default_rng(100 + twin)
    for p, rows, seqs in cases:
        gz = make_twin(p, rng, **TWINS[twin])
        with open(gz, "rb") as f, open(p, "rb") as g:
            assert gzip.decompress(f.read()) == g.read()                 # the writer writes what gzip reads
        fasta.forget()
        for name in seqs:
            assert read_fasta_bytes(gz, name) == read_fasta_bytes(p, name)
        assert read_fasta(gz, rows[-1][0]) == seqs[rows[-1][0]]
        for ext in ("", ".fai", ".gzi"):
            if os.path.exists(gz + ext):
                os.remove(gz + ext)


def test_gzi_with_explicit_first_entry(cases, tmp_path):
    p, rows, seqs = cases[-3]
    with open(p, "rb") as f:
        data = f.read()
    gz = str(tmp_path / "x.fa.gz")
    ent = fastaio.write_bgzf(gz, data, sizes=(1000, 37))
    fastaio.write_gzi(gz + ".gzi", ent, explicit_first=True)
    fastaio.write_fai(gz + ".fai", rows)
    for name in seqs:
        assert read_fasta_bytes(gz, name) == seqs[name].encode("ascii")


def test_only_covering_members_are_inflated(tmp_path):
    rng = np.random.default_rng(3)
    contigs = [("a", fastaio.random_sequence(rng, 10_000)), ("b", fastaio.random_sequence(rng, 3_000)), ("c", fastaio.random_sequence(rng, 10_000))]
    p = str(tmp_path / "r.fa")
    rows = fastaio.write_fasta_lines(p, contigs, 60)
    with open(p, "rb") as f:
        data = f.read()
    for gzi in (True, False):
        gz = str(tmp_path / ("r%d.fa.gz" % gzi))
        ent = fastaio.write_bgzf(gz, data, sizes=(1000,))
        if gzi:
            fastaio.write_gzi(gz + ".gzi", ent)
        fastaio.write_fai(gz + ".fai", rows)
        for name, length, offset, lb, lw in rows:
            span = ((length - 1) // lb) * lw + (length - 1) % lb + 1
            want = (offset + span - 1) // 1000 - offset // 1000 + 1      # members of 1,000 bytes that hold [offset, offset + span)
            assert read_fasta_bytes(gz, name) == dict(contigs)[name].encode("ascii")
            assert fasta.LAST_HOST["members"] == want
            assert want < len(ent)
        # contig b lies inside members that also hold the end of a and the start of c: it starts and ends in the middle of members
        assert rows[1][2] % 1000 != 0


def _bgz(tmp_path, name="r.fa", n=5_000, lb=60, sizes=(700,)):
    rng = np.random.default_rng(9)
    contigs = [("a", fastaio.random_sequence(rng, n)), ("b", fastaio.random_sequence(rng, 999))]
    p = str(tmp_path / name)
    rows = fastaio.write_fasta_lines(p, contigs, lb)
    with open(p, "rb") as f:
        data = f.read()
    gz = p + ".gz"
    ent = fastaio.write_bgzf(gz, data, sizes=sizes)
    fastaio.write_fai(gz + ".fai", rows)
    return p, gz, ent, rows, data


def test_plain_gzip_is_refused(tmp_path):
    p, gz, ent, rows, data = _bgz(tmp_path)
    with open(gz, "wb") as f:
        f.write(gzip.compress(data))
    with pytest.raises(NanoCallerHipError, match="must be bgzip-compressed"):
        read_fasta_bytes(gz, "a")


def test_missing_fai_is_refused(tmp_path):
    p, gz, ent, rows, data = _bgz(tmp_path)
    os.remove(gz + ".fai")
    with pytest.raises(NanoCallerHipError, match="samtools faidx"):
        read_fasta_bytes(gz, "a")


def test_gzi_entry_off_a_member_start(tmp_path):
    p, gz, ent, rows, data = _bgz(tmp_path)
    bad = list(ent)
    bad[3] = (bad[3][0] + 1, bad[3][1])
    fastaio.write_gzi(gz + ".gzi", bad)
    with pytest.raises(NanoCallerHipError, match="not the start of a BGZF member"):
        read_fasta_bytes(gz, "a")


def test_gzi_descending(tmp_path):
    p, gz, ent, rows, data = _bgz(tmp_path)
    bad = list(ent)
    bad[2], bad[3] = bad[3], bad[2]
    fastaio.write_gzi(gz + ".gzi", bad)
    with pytest.raises(NanoCallerHipError, match="not in file order"):
        read_fasta_bytes(gz, "a")


def test_gzi_entry_outside_the_file(tmp_path):
    p, gz, ent, rows, data = _bgz(tmp_path)
    fastaio.write_gzi(gz + ".gzi", list(ent) + [(os.path.getsize(gz) + 5, len(data) + 5)])
    with pytest.raises(NanoCallerHipError, match="lies outside"):
        read_fasta_bytes(gz, "a")


@pytest.mark.parametrize("gzi", [True, False])
def test_flipped_payload_byte_fails_crc(tmp_path, gzi):
    # stored members: a flipped payload byte leaves the deflate stream valid, only the CRC-32 tells
    rng = np.random.default_rng(9)
    contigs = [("a", fastaio.random_sequence(rng, 5_000))]
    p = str(tmp_path / "s.fa")
    rows = fastaio.write_fasta_lines(p, contigs, 60)
    with open(p, "rb") as f:
        data = f.read()
    gz = p + ".gz"
    ent = fastaio.write_bgzf(gz, data, sizes=(700,), level=0)
    fastaio.write_fai(gz + ".fai", rows)
    if gzi:
        fastaio.write_gzi(gz + ".gzi", ent)
    assert read_fasta_bytes(gz, "a") == contigs[0][1].encode("ascii")
    raw = bytearray(open(gz, "rb").read())
    at = ent[2][0] + 18 + 5 + 100                                        # inside the third member's stored bytes
    raw[at] ^= 0x01
    with open(gz, "wb") as f:
        f.write(bytes(raw))
    os.utime(gz, ns=(1, 1))                                              # (the member map is keyed by path, mtime and size)
    with pytest.raises(NanoCallerHipError, match="CRC-32"):
        read_fasta_bytes(gz, "a")


def test_fai_with_wrong_linewidth(tmp_path):
    p, gz, ent, rows, data = _bgz(tmp_path)
    fastaio.write_fai(gz + ".fai", [(n, ln, off, lb, lw + 1) for n, ln, off, lb, lw in rows])     # claims \r\n
    with pytest.raises(NanoCallerHipError, match="does not describe this file"):
        read_fasta_bytes(gz, "a")
    fastaio.write_fai(gz + ".fai", [(n, ln, off, lb, lw + 2) for n, ln, off, lb, lw in rows])
    with pytest.raises(NanoCallerHipError, match="neither 1"):
        read_fasta_bytes(gz, "a")
    fastaio.write_fai(gz + ".fai", [(n, ln, off, 0, 1) for n, ln, off, lb, lw in rows])
    with pytest.raises(NanoCallerHipError, match="not a line length"):
        read_fasta_bytes(gz, "a")
    fastaio.write_fai(gz + ".fai", [(n, ln, off + 10**6, lb, lw) for n, ln, off, lb, lw in rows])  # points behind the file
    with pytest.raises(NanoCallerHipError, match="does not describe this file"):
        read_fasta_bytes(gz, "a")


def test_span_formula():
    e = fasta.FaiEntry("x", 120, 7, 60, 61)
    assert e.span == 121                                                  # two full lines: the terminator behind the last is not part of it
    assert fasta.FaiEntry("x", 121, 7, 60, 61).span == 123
    assert fasta.FaiEntry("x", 1, 7, 60, 62).span == 1
    assert fasta.FaiEntry("x", 5000, 7, 5000, 5001).span == 5000


def test_gzi_layout(tmp_path):
    """the writer's .gzi is the format htslib documents: uint64 count, then (compressed, uncompressed) uint64 pairs, first member left out"""
    p, gz, ent, rows, data = _bgz(tmp_path)
    fastaio.write_gzi(gz + ".gzi", ent)
    buf = open(gz + ".gzi", "rb").read()
    n, = struct.unpack_from("<Q", buf)
    assert n == len(ent) - 1 and len(buf) == 8 + 16 * n
    assert struct.unpack_from("<QQ", buf, 8) == ent[1]
    mm = fasta.member_map(gz)
    assert mm.from_gzi and mm.mstart.tolist() == [c for c, _ in ent] and mm.ustart.tolist() == [u for _, u in ent]
    os.remove(gz + ".gzi")
    mm = fasta.member_map(gz)
    assert not mm.from_gzi and mm.mstart.tolist()[:len(ent)] == [c for c, _ in ent] and mm.ustart.tolist()[:len(ent)] == [u for _, u in ent]

"""Test tooling: FASTA / .fai / bgzip / .gzi WRITERS (htslib's faidx and bgzf formats, SAMv1 4.1), independent of the product's own compressor
and parsers: plain Python + zlib.  The BGZF writer cuts its members where the caller says, so member boundaries can fall anywhere in a
contig: mid-line, between \\r and \\n, inside a header."""
import struct
import zlib

import numpy as np

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_fasta_lines(path, contigs, lb, eol="\n", last_eol=True, with_fai=True):
    """contigs: [(header line without '>', sequence str)] written with `lb` bases per line and `eol` behind every line; last_eol=False leaves
    the terminator behind the file's last line out.  -> [(name, length, offset, lb, lw)], also written to <path>.fai"""
    rows, out = [], bytearray()
    e = eol.encode("ascii")
    for k, (header, seq) in enumerate(contigs):
        out += b">" + header.encode("ascii") + e
        rows.append((header.split()[0], len(seq), len(out), lb, lb + len(e)))
        s = seq.encode("ascii")
        for i in range(0, len(s), lb):
            out += s[i:i + lb] + e
        if k == len(contigs) - 1 and not last_eol and s:
            del out[len(out) - len(e):]
    with open(path, "wb") as f:
        f.write(bytes(out))
    if with_fai:
        write_fai(path + ".fai", rows)
    return rows


def write_fai(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write("%s\t%d\t%d\t%d\t%d\n" % tuple(r))


def bgzf_member(raw, level=6):
    """one BGZF member of `raw` (<= 65,536 bytes... 0xff00 for level 0, whose stored form grows by 5 bytes per 65,535)"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(raw) + co.flush()
    assert len(comp) + 25 < 65536, "member too large"
    return struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(comp) + 25) + comp + \
        struct.pack("<II", zlib.crc32(raw) & 0xffffffff, len(raw))


def write_bgzf(path, data, sizes=(0xff00,), level=6, levels=None, eof=True):
    """`data` as BGZF members of sizes[0], sizes[1], ... bytes (the list is cycled; every size >= 1); levels: a list cycled the same way
    (0 = stored members).  -> [(compressed offset, uncompressed offset)] of every member, the first included"""
    ent, out, u, k = [], bytearray(), 0, 0
    while u < len(data):
        n = int(sizes[k % len(sizes)])
        assert n >= 1
        lv = level if levels is None else levels[k % len(levels)]
        ent.append((len(out), u))
        out += bgzf_member(data[u:u + n], lv)
        u += n
        k += 1
    if eof:
        out += BGZF_EOF
    with open(path, "wb") as f:
        f.write(bytes(out))
    return ent


def write_gzi(path, entries, explicit_first=False):
    """entries as write_bgzf returns them; the (0, 0) of the first member is left out, as bgzip does, unless explicit_first"""
    ent = [e for e in entries if explicit_first or e != (0, 0)]
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(ent)))
        for c, u in ent:
            f.write(struct.pack("<QQ", c, u))


def random_sequence(rng, n, soft=True):
    """letters with everything a reference holds: upper-case ACGT, lower-case (soft-masked) runs, N runs, IUPAC letters and '*'"""
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    if soft and n >= 8:
        for _ in range(max(1, n // 400)):
            a = int(rng.integers(0, n))
            b = min(n, a + int(rng.integers(1, 40)))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                s[a:b] |= 0x20                                           # lower case
            elif kind == 1:
                s[a:b] = ord("N") if rng.integers(0, 2) else ord("n")
            else:
                s[a:b] = np.frombuffer(b"RYKMSWBDHVryn*", np.uint8)[rng.integers(0, 14, b - a)]
    return s.tobytes().decode("ascii")


def bgzip_twin(fa_path, sizes=(0xff00,), level=6, levels=None, gzi=True, fai_rows=None):
    """<fa_path>.gz beside a plain FASTA: the same bytes as BGZF, the same .fai, a .gzi when asked -> the .gz path"""
    with open(fa_path, "rb") as f:
        data = f.read()
    gz = fa_path + ".gz"
    ent = write_bgzf(gz, data, sizes, level, levels)
    if gzi:
        write_gzi(gz + ".gzi", ent)
    with open(fa_path + ".fai") as f, open(gz + ".fai", "w") as g:
        g.write(f.read())
    return gz


LBS = (1, 7, 15, 16, 17, 60, 61, 64)


def case_lengths(lb):
    """the contig lengths at which a reader can go wrong for lines of `lb` bases"""
    return sorted({n for n in (1, lb - 1, lb, lb + 1, 2 * lb, 4095, 4096, 4097) if n >= 1})


def write_case_file(path, rng, lb, eol, last_full, last_eol):
    """one FASTA with a contig of every length of case_lengths(lb), each behind a header of another length (so that the offsets of the first
    bases are odd and even), and a last contig whose last line is full / short, with / without a terminator at the end of the file.
    -> (rows, {name: sequence})"""
    lens = case_lengths(lb) + [3 * lb if last_full else 3 * lb + (lb + 1) // 2]
    contigs = [("c%d %s" % (k, "x" * (5 * k + (k & 1))), random_sequence(rng, n)) for k, n in enumerate(lens)]
    rows = write_fasta_lines(path, contigs, lb, eol, last_eol=last_eol)
    return rows, {h.split()[0]: s for h, s in contigs}

"""Reference FASTA formats (host side): .fai, bgzip-compressed FASTA (.fa.gz + .fai + optional .gzi), and the host reader of the latter.

The reference reads its FASTA through pysam.FastaFile, which accepts a plain file or a bgzipped one (how GRCh38 is commonly distributed).
`bam.read_fasta_bytes` hands every path that ends in .gz to `read_fasta_bytes` here; plain files keep the reader in bam.py.  The device
route (device_fasta.py, csrc/nc_fasta.hip) uses the same index parsers and the same member map.

A .fai row is name, length, offset, linebases (lb), linewidth (lw): the contig's bytes in the UNCOMPRESSED file are [offset, offset + span),
span = ((length - 1) // lb) * lw + (length - 1) % lb + 1 -- the last line may be short or full, and nothing is assumed about a terminator
behind it.  A .gzi is uint64 n, then n pairs (compressed offset of a BGZF member, uncompressed offset of its first byte), little endian;
the member at (0, 0) is implicit.  Without a .gzi the member map is made once per file by walking the member headers (nc_bgzf_scan) and
kept in memory: nothing is written beside the user's file.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import NamedTuple

import numpy as np

from . import bgzf
from ._lib import NanoCallerHipError

BGZF_MAGIC = b"\x1f\x8b\x08\x04"
LAST_HOST = {}                # what the most recent host read of a bgzipped contig touched: members inflated, compressed bytes read


class FaiEntry(NamedTuple):
    name: str
    length: int
    offset: int
    linebases: int
    linewidth: int

    @property
    def span(self):
        """bytes from the contig's first base to its last, terminators between them included"""
        if self.length <= 0:
            return 0
        return ((self.length - 1) // self.linebases) * self.linewidth + (self.length - 1) % self.linebases + 1


_FAI = {}                     # (path, mtime, size) -> {contig: FaiEntry}
_MAPS = {}                    # (path, mtime, size) of the .fa.gz -> MemberMap


def _file_key(path):
    st = os.stat(path)
    return (os.path.abspath(path), st.st_mtime_ns, st.st_size)


def read_fai(fai_path):
    """{contig: FaiEntry} of a .fai (the five columns of samtools faidx), parsed once per version of the file.  Rows the readers cannot walk
    are refused here: linebases < 1, or a line terminator (linewidth - linebases) that is neither \\n nor \\r\\n."""
    key = _file_key(fai_path)
    if key not in _FAI:
        out = {}
        with open(fai_path) as f:
            for no, line in enumerate(f, 1):
                t = line.rstrip("\r\n").split("\t")
                if len(t) < 5:
                    if not line.strip():
                        continue
                    raise NanoCallerHipError("%s, line %d: a .fai row has five columns (name, length, offset, linebases, linewidth)" % (fai_path, no))
                try:
                    e = FaiEntry(t[0], int(t[1]), int(t[2]), int(t[3]), int(t[4]))
                except ValueError:
                    raise NanoCallerHipError("%s, line %d: not a .fai row" % (fai_path, no))
                if e.length < 0 or e.offset < 0:
                    raise NanoCallerHipError("%s, line %d: negative length / offset" % (fai_path, no))
                if e.linebases < 1:
                    raise NanoCallerHipError("%s, line %d (%s): linebases %d is not a line length" % (fai_path, no, e.name, e.linebases))
                if e.linewidth - e.linebases not in (1, 2):
                    raise NanoCallerHipError("%s, line %d (%s): linewidth %d - linebases %d is neither 1 (\\n) nor 2 (\\r\\n)"
                                             % (fai_path, no, e.name, e.linewidth, e.linebases))
                out.setdefault(e.name, e)
        _FAI.clear()
        _FAI[key] = out
    return _FAI[key]


def fai_entry(fasta_path, chrom):
    """the .fai row of `chrom` (<fasta_path>.fai); KeyError for an unknown contig, NanoCallerHipError when there is no index"""
    fai = fasta_path + ".fai"
    if not os.path.exists(fai):
        raise NanoCallerHipError("%s has no index %s beside it: make one with `samtools faidx %s`" % (fasta_path, fai, fasta_path))
    e = read_fai(fai).get(chrom)
    if e is None:
        raise KeyError(chrom)
    return e


def is_bgzf(path):
    """gzip magic + FEXTRA + a BC subfield: what bgzip writes (the test generate_SNP_pileups._exclude_rows makes for BED files)"""
    with open(path, "rb") as f:
        head = f.read(18)
    return len(head) == 18 and head[:4] == BGZF_MAGIC and head[12:14] == b"BC"


def check_bgzf(path):
    """a .gz reference must be bgzip output (random access needs the members); plain gzip is refused, as pysam refuses it"""
    if not is_bgzf(path):
        with open(path, "rb") as f:
            gz = f.read(2) == b"\x1f\x8b"
        raise NanoCallerHipError("%s is %s: a compressed reference must be bgzip-compressed (`bgzip %s`, then `samtools faidx`)"
                                 % (path, "plain gzip, not BGZF" if gz else "not a gzip file", os.path.splitext(path)[0]))


class MemberMap(NamedTuple):
    """file offset of every BGZF member and the uncompressed offset of its first byte (both ascending, both start at 0)"""
    mstart: np.ndarray        # int64 [n]
    ustart: np.ndarray        # int64 [n]
    file_bytes: int
    from_gzi: bool

    def covering(self, u0, u1):
        """the members that hold the uncompressed bytes [u0, u1): (index of the first, file offset where it starts, file offset behind the
        last, uncompressed offset of the first's first byte)"""
        i = int(np.searchsorted(self.ustart, u0, side="right")) - 1
        j = int(np.searchsorted(self.ustart, max(u0 + 1, u1), side="left"))          # first member that starts at or behind u1
        hi = int(self.mstart[j]) if j < self.mstart.size else self.file_bytes
        return i, int(self.mstart[i]), hi, int(self.ustart[i])


def read_gzi(gzi_path, gz_path):
    """the member map from a .gzi, every entry validated against the file: strictly ascending, inside the file, BGZF magic at the compressed offset"""
    file_bytes = os.path.getsize(gz_path)
    with open(gzi_path, "rb") as f:
        buf = f.read()
    if len(buf) < 8:
        raise NanoCallerHipError("%s is not a .gzi (shorter than its entry count)" % gzi_path)
    n, = struct.unpack_from("<Q", buf, 0)
    if len(buf) < 8 + 16 * n:
        raise NanoCallerHipError("%s announces %d entries and holds %d" % (gzi_path, n, (len(buf) - 8) // 16))
    ent = np.frombuffer(buf, "<u8", 2 * n, 8).reshape(n, 2)
    if n and int(ent.max()) >= 1 << 62:
        raise NanoCallerHipError("%s: an entry lies outside %s" % (gzi_path, gz_path))
    ent = ent.astype(np.int64)
    if n and ent[0, 0] == 0 and ent[0, 1] == 0:                         # (bgzip leaves the first member out; an explicit one is tolerated)
        ent = ent[1:]
    c = np.concatenate([[0], ent[:, 0]]).astype(np.int64)
    u = np.concatenate([[0], ent[:, 1]]).astype(np.int64)
    if np.any(np.diff(c) <= 0) or np.any(np.diff(u) <= 0):
        k = int(np.flatnonzero((np.diff(c) <= 0) | (np.diff(u) <= 0))[0])
        raise NanoCallerHipError("%s: entry %d (%d, %d) does not ascend from (%d, %d): the index is not in file order"
                                 % (gzi_path, k, c[k + 1], u[k + 1], c[k], u[k]))
    if c[-1] + 28 > file_bytes:
        raise NanoCallerHipError("%s: entry (%d, %d) lies outside %s (%d bytes)" % (gzi_path, c[-1], u[-1], gz_path, file_bytes))
    fd = os.open(gz_path, os.O_RDONLY)
    try:
        for k in range(c.size):
            head = os.pread(fd, 18, int(c[k]))
            if len(head) < 18 or head[:4] != BGZF_MAGIC or head[12:14] != b"BC":
                raise NanoCallerHipError("%s: entry %d points at byte %d of %s, which is not the start of a BGZF member" % (gzi_path, k, c[k], gz_path))
    finally:
        os.close(fd)
    return MemberMap(c, u, file_bytes, True)


def scan_members(data, base=0):
    """the whole BGZF members of `data` (bytes-like) -> (payload offset into data, payload length, inflated size, bytes scanned)"""
    try:
        return bgzf.scan_members(data)
    except bgzf.ScanError as e:
        raise NanoCallerHipError("not a BGZF member at byte %d (nc_bgzf_scan: %d)" % (base + e.pos, e.rc))


def walk_members(gz_path, piece=64 << 20):
    """the member map of a file without .gzi: the member headers, walked piece by piece (the file is read once, never held whole)"""
    file_bytes = os.path.getsize(gz_path)
    ms, us, pos, u = [], [], 0, 0
    with open(gz_path, "rb") as f:
        rest = b""
        while True:
            got = f.read(piece)
            buf = rest + got
            if not buf:
                break
            try:
                coff, clen, isize, nxt = scan_members(buf, pos)
            except NanoCallerHipError as e:
                raise NanoCallerHipError("%s: %s" % (gz_path, e))
            if coff.size:
                start, uo = bgzf.member_table(coff, clen, isize)
                ms.append(start + pos)
                us.append(uo[:-1] + u)
                u += int(uo[-1])
            if not got:
                if nxt != len(buf):
                    raise NanoCallerHipError("%s does not end with a whole BGZF member" % gz_path)
                break
            if nxt == 0 and len(buf) > (1 << 17):
                raise NanoCallerHipError("%s: no BGZF member at byte %d" % (gz_path, pos))
            rest, pos = buf[nxt:], pos + nxt
    if not ms:
        raise NanoCallerHipError("%s holds no BGZF member" % gz_path)
    return MemberMap(np.concatenate(ms), np.concatenate(us), file_bytes, False)


def member_map(gz_path):
    """MemberMap of a bgzipped file: from <path>.gzi when there is one, else walked once per version of the file (kept in memory)"""
    key = _file_key(gz_path)
    gzi = gz_path + ".gzi"
    if os.path.exists(gzi):
        key = key + _file_key(gzi)
    if key not in _MAPS:
        check_bgzf(gz_path)
        m = read_gzi(gzi, gz_path) if os.path.exists(gzi) else walk_members(gz_path)
        for k in [k for k in _MAPS if k[0] == key[0]]:
            del _MAPS[k]
        _MAPS[key] = m
    return _MAPS[key]


def read_member_bytes(gz_path, lo, hi):
    with open(gz_path, "rb") as f:
        f.seek(lo)
        buf = f.read(hi - lo)
    if len(buf) != hi - lo:
        raise NanoCallerHipError("short read of %s" % gz_path)
    return buf


def inflate_range(gz_path, u0, u1):
    """uncompressed bytes [u0, u1) of a bgzipped file with zlib: only the members that hold them are read and inflated, each checked against
    its CRC-32 and ISIZE"""
    mm = member_map(gz_path)
    if u1 <= u0:
        return b""
    i, lo, hi, ubase = mm.covering(u0, u1)
    buf = read_member_bytes(gz_path, lo, hi)
    coff, clen, isize, _ = scan_members(buf, lo)
    out, have, got0, n_inf = [], ubase, None, 0
    for k in range(coff.size):
        if have >= u1:
            break
        c, size = int(coff[k]), int(isize[k])
        if have + size > u0:                                             # (a .gzi that leaves members out makes the range begin early)
            try:
                data = zlib.decompress(buf[c:c + int(clen[k])], -15)
            except zlib.error as e:
                raise NanoCallerHipError("%s: the BGZF member at byte %d is not a valid deflate stream (%s)" % (gz_path, lo + c - 18, e))
            crc, = struct.unpack_from("<I", buf, c + int(clen[k]))
            if len(data) != size:
                raise NanoCallerHipError("%s: the BGZF member at byte %d inflates to %d bytes, its ISIZE says %d" % (gz_path, lo + c - 18, len(data), size))
            if zlib.crc32(data) != crc:
                raise NanoCallerHipError("%s: the BGZF member at byte %d fails its CRC-32" % (gz_path, lo + c - 18))
            n_inf += 1
            if got0 is None:
                got0 = have
            out.append(data)
        have += size
    LAST_HOST.clear()
    LAST_HOST.update(members=n_inf, compressed_bytes=hi - lo)
    if have < u1 or got0 is None:
        raise NanoCallerHipError("%s ends %d bytes before the contig does: the .fai does not describe this file" % (gz_path, u1 - have))
    got = b"".join(out)
    return got[u0 - got0:u1 - got0]


def strip_lines(raw, e: FaiEntry, path):
    """the letters of contig `e` from its bytes [offset, offset + span): terminators out, and the same checks the device decoder makes --
    every terminator slot between two lines of the contig holds \\n / \\r\\n, no base byte lies outside 0x21..0x7e"""
    lb, lw, n = e.linebases, e.linewidth, e.length
    if len(raw) != e.span:
        raise NanoCallerHipError("%s, contig %s: the .fai does not describe this file (%d of %d bytes)" % (path, e.name, len(raw), e.span))
    a = np.frombuffer(raw, np.uint8)
    nfull = (n - 1) // lb
    body = a[:nfull * lw].reshape(nfull, lw)
    term = np.frombuffer(b"\n" if lw - lb == 1 else b"\r\n", np.uint8)
    if nfull and not np.array_equal(body[:, lb:], np.broadcast_to(term, (nfull, lw - lb))):
        raise NanoCallerHipError("%s, contig %s: the .fai does not describe this file (a line does not end where linebases %d / linewidth %d say)"
                                 % (path, e.name, lb, lw))
    letters = np.concatenate([body[:, :lb].reshape(-1), a[nfull * lw:]])
    if letters.size and (int(letters.min()) < 0x21 or int(letters.max()) > 0x7e):
        raise NanoCallerHipError("%s, contig %s: the .fai does not describe this file (a control byte among the bases)" % (path, e.name))
    return letters.tobytes()


def read_fasta_bytes(path, chrom):
    """the letters of `chrom` from a bgzip-compressed FASTA (<path>.fai, optionally <path>.gzi), on the host"""
    check_bgzf(path)
    e = fai_entry(path, chrom)
    if e.length == 0:
        return b""
    return strip_lines(inflate_range(path, e.offset, e.offset + e.span), e, path)


def forget():
    """drop the parsed indexes and member maps"""
    _FAI.clear()
    _MAPS.clear()

"""BGZF (SAMv1 4.1) as the BAM, FASTA and VCF file paths share it: the members of a file image, their framing, virtual offsets, the batched
inflate on the device, and the BAM header that sits in a file's leading members.

Host side (numpy, zlib): `scan_members` is the one caller of nc_bgzf_scan, `member_table` the one place that turns its answer into member
starts and inflated offsets.  Device side (torch, imported where it is used): `inflate_members` is the batched nc_inflate_device +
nc_bgzf_crc_device loop of the BAM indexer and the FASTA reader.  DeviceBam.load keeps its own two-stream pipeline (device_bam.py) and takes
from here the scan, the token workspace's size and the error for members that do not inflate.  The switches (NC_BGZF_CRC, ...) and the
buffer pools stay in device_bam.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import _lib
from ._lib import NanoCallerHipError

BGZF_BLOCK = 0xff00             # uncompressed bytes of every member but the last (htslib's BGZF_BLOCK_SIZE)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ------------------------------------------------------------------------------------------------------------ host: the members of a file image
class ScanError(NanoCallerHipError):
    """nc_bgzf_scan refused the bytes: `rc` its status, `pos` where it stopped; the callers word the message"""

    def __init__(self, rc, pos):
        super().__init__("not a BGZF member at byte %d (nc_bgzf_scan: %d)" % (pos, rc))
        self.rc, self.pos = rc, pos


def _host_ptr(a, at=0):
    """pointer to element `at` of a contiguous numpy array (the loader scans once per piece it has read: ndarray.ctypes costs it tens of
    microseconds a time)"""
    assert a.flags.c_contiguous
    return C.c_void_p(a.__array_interface__["data"][0] + at * a.itemsize)


def scan_members(buf, pos=0, out=None, out_at=0):
    """the whole BGZF members of buf[pos:] (bytes-like or a uint8 array) -> (payload offset into buf, payload length, inflated size, where the
    scan stopped: behind the last whole member).  out = (int64, int32, int32) arrays of the caller's: the members are written there from
    element `out_at` on -- nothing is copied -- and the three results are views of them."""
    arr = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, np.uint8)
    if out is None:
        cap = (arr.size - pos) // 26 + 16                                # (a member is 28 bytes at least)
        out = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap, np.int32)
    k, nxt = C.c_int64(), C.c_int64()
    rc = _lib.lib().nc_bgzf_scan(_host_ptr(arr), arr.size, pos, out[0].size - out_at, *(_host_ptr(a, out_at) for a in out), C.byref(k), C.byref(nxt))
    if rc != _lib.NC_OK:
        raise ScanError(rc, int(nxt.value))
    k = out_at + int(k.value)
    return out[0][out_at:k], out[1][out_at:k], out[2][out_at:k], int(nxt.value)


def member_table(coff, clen, isize):
    """(offset of every member's first byte [n], offset of every member's first inflated byte and, last, the inflated total [n + 1]) of members
    scanned back to back from offset 0 on"""
    mstart = np.zeros(coff.size, np.int64)
    mstart[1:] = coff[:-1] + clen[:-1] + 8
    ooff = np.zeros(coff.size + 1, np.int64)
    np.cumsum(isize, out=ooff[1:])
    return mstart, ooff


def member_spans(n_bytes, base=0, block=BGZF_BLOCK):
    """(offsets, lengths) of the members that cut n_bytes bytes from `base` on into pieces of `block` (the last may be shorter)"""
    k = -(-int(n_bytes) // block)
    off = base + np.arange(k, dtype=np.int64) * block
    ln = np.full(k, block, np.int32)
    if k:
        ln[-1] = int(n_bytes) - (k - 1) * block
    return off, ln


def bgzf_members(payloads, crcs, isizes, eof=True) -> bytes:
    """gzip members with the BC extra field (SAMv1 4.1) around raw-deflate payloads, + the EOF block"""
    out = []
    for p, c, n in zip(payloads, crcs, isizes):
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(p) + 25) + bytes(p) +
                   struct.pack("<II", int(c) & 0xffffffff, int(n)))
    if eof:
        out.append(BGZF_EOF)
    return b"".join(out)


def virtual_offsets(stream_pos, member_foff, first_member=0, block=BGZF_BLOCK):
    """virtual offsets (SAMv1 4.1.1) of positions in a stream that starts at member `first_member` and is cut into members of `block`
    bytes; member_foff = file offset of every member (and of the EOF block behind them).  A position at a member boundary is the start of the
    next member, as htslib's bgzf_tell gives it after a full block."""
    q = np.asarray(stream_pos, np.int64)
    return (member_foff[first_member + q // block].astype(np.uint64) << np.uint64(16)) | (q % block).astype(np.uint64)


# ------------------------------------------------------------------------------------------------------------ host: the BAM header
def _parse_bam_header(path, data, coff, clen):
    """the header from the leading members (inflated with zlib: a few kilobytes); None when the members seen so far do not hold all of it"""
    got, k = b"", 0

    def need(n):
        nonlocal got, k
        while len(got) < n:
            if k >= len(coff):
                raise EOFError
            c = int(coff[k])
            got += zlib.decompress(data[c:c + int(clen[k])].tobytes(), -15)
            k += 1
    try:
        need(12)
        if got[:4] != b"BAM\1":
            raise NanoCallerHipError("%s is not a BAM file" % path)
        l_text, = struct.unpack_from("<i", got, 4)
        need(12 + l_text)
        n_ref, = struct.unpack_from("<i", got, 8 + l_text)
        o = 12 + l_text
        names, lengths = [], []
        for _ in range(n_ref):
            need(o + 4)
            l_name, = struct.unpack_from("<i", got, o)
            need(o + 8 + l_name)
            names.append(got[o + 4:o + 4 + l_name - 1].decode("ascii"))
            lengths.append(struct.unpack_from("<i", got, o + 4 + l_name)[0])
            o += 8 + l_name
    except EOFError:
        return None
    return got[8:8 + l_text].split(b"\0", 1)[0].decode("ascii", "replace"), names, lengths, o


def bam_header(path):
    """(header text, reference names, reference lengths, header_len = where the first record starts in the inflated stream) of a BAM file.
    The head of the file is read, more of it while the header goes on (it may span many members)."""
    file_bytes, want = os.path.getsize(path), 1 << 20
    while True:
        with open(path, "rb") as f:
            head = np.frombuffer(f.read(min(want, file_bytes)), np.uint8)
        try:
            coff, clen, _, _ = scan_members(head)
        except ScanError as e:
            raise NanoCallerHipError("%s is not a BGZF file (nc_bgzf_scan: %d)" % (path, e.rc))
        hdr = _parse_bam_header(path, head, coff, clen)
        if hdr is not None:
            return hdr
        if head.size >= file_bytes:
            raise NanoCallerHipError("%s: truncated BAM header" % path)
        want *= 8


# ------------------------------------------------------------------------------------------------------------ device: inflate
def _vp(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off)


def token_workspace(dev, name, batch):
    """the token workspace of `batch` members per nc_inflate_device call (256 KB each, 16 MB per 64 members), from device_bam's pool of work
    buffers under `name`"""
    import torch

    from . import device_bam
    return device_bam._work_buffer(dev, name, ((batch + 63) // 64) << 22, torch.int32)


def inflate_members(eng, d_comp, d64, d32, n, d_out, batch, tok_name, events=None):
    """Inflate `n` members of the file image d_comp into d_out, at most `batch` per launch, and check their CRC-32s (device_bam.CHECK_CRC):
    d64 = [payload offsets | output offsets], d32 = [payload lengths | inflated sizes], n of each -> int32 status per member (0: good,
    7: CRC-32).  events: three timing events, recorded before the first inflate, behind the last and behind the last CRC pass."""
    import torch

    from . import device_bam
    L, dev = _lib.lib(), eng.device
    status = torch.zeros(max(1, n), dtype=torch.int32, device=dev)
    batch = min(batch, max(64, (n + 63) // 64 * 64))
    d_tok = token_workspace(dev, tok_name, batch)
    d_ntok = torch.zeros(batch, dtype=torch.int32, device=dev)
    for a in range(0, n, batch):
        k = min(batch, n - a)
        args = (k, _vp(d_comp), _vp(d64, 8 * a), _vp(d32, 4 * a), _vp(d_out), _vp(d64, 8 * (n + a)), _vp(d32, 4 * (n + a)), _vp(status, 4 * a))
        if events and a == 0:
            events[0].record()
        eng._check(L.nc_inflate_device(eng.ctx, *args, _vp(d_tok), _vp(d_ntok)), "nc_inflate_device")
        if events and a + batch >= n:
            events[1].record()
        if device_bam.CHECK_CRC:
            eng._check(L.nc_bgzf_crc_device(eng.ctx, *args), "nc_bgzf_crc_device")
    if events:
        events[2].record()
    return status[:n]


def bad_members_error(path, statuses):
    """the error of a BAM whose members did not all inflate (`statuses`: the status tensors of its inflate calls), None when they did"""
    bad = sum(int(st.count_nonzero().item()) for st in statuses)
    if not bad:
        return None
    crc = sum(int((st == 7).sum().item()) for st in statuses)
    return NanoCallerHipError("%s: %d BGZF members are not valid deflate streams of their announced size%s"
                              % (path, bad - crc, (", %d fail their CRC-32" % crc) if crc else ""))


def event_timed(ms):
    """-> timed(what, fn): fn() with its time on the current stream, by events, added to ms[what] (milliseconds)"""
    import torch

    def timed(what, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        ms[what] = ms.get(what, 0.0) + e0.elapsed_time(e1)
        return r
    return timed

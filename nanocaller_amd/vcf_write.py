"""Text lines to a BGZF piece on the GPU: the lines are compressed where they were made and only the compressed
members cross to the host; with them goes the piece's share of the CSI index, reduced on the device to what the index stores.

A piece is a run of whole BGZF members without the EOF block: it starts a member of its own, so pieces concatenate into a file in any order the
caller finds right, and an index over the file is the pieces' summaries joined (hts_index.csi_from_summaries).  `write_piece` is all there is:

  text --member_spans--> members of 0xff00 bytes --nc_bgzf_deflate_device / nc_bgzf_crc32_device / nc_bgzf_assemble_device, in slabs of at most
  `slab_members` members--> the slab's file image --D2H into one of two page-locked buffers--> f.write, while the next slab compresses
  lines + member offsets --nc_lines_index--> chunk runs and window minima, virtual offsets relative to the piece

Payload slots and the file image are sized by the slab, not by the text; the text is not copied (the members' offsets point into it).
"""
from __future__ import annotations

import time

import numpy as np

from . import _lib
from .bgzf import BGZF_EOF, member_spans

PAYLOAD_SLOT = 65536            # room for one member's payload on the device (a stored block is 65,285 bytes at most)
MEMBER_MAX = PAYLOAD_SLOT + 26  # ... and for the member around it in the file image
STAGES = ("deflate", "crc", "assemble", "d2h", "index")


def _pinned_pair(eng, nbytes):
    """the engine's two page-locked staging buffers, grown to nbytes each (page-locking is slow: they are kept)"""
    import torch
    have = getattr(eng, "_vcf_write_pinned", None)
    if have is None or have[0].numel() < nbytes:
        have = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        eng._vcf_write_pinned = have
    return have


def write_piece(eng, f, text, line_off, beg, end, *, slab_members=4096, min_shift=14, depth=5) -> dict:
    """Write the lines text[line_off[0] : line_off[n]] (device tensors: text uint8, line_off int64 [n + 1] offsets into text, beg / end int64
    [n] = the 0-based half-open interval each line is indexed under, ends and begins ascending) to the binary file object `f` as one BGZF piece.
    -> dict(lines, bytes = the piece's length in the file, text_bytes, members, run_bin, run_vbeg, run_vend, w0, win_min (Engine.lines_index:
    virtual offsets relative to the piece), ms = milliseconds per stage, by events; 'write' by the clock)."""
    import torch
    dev = eng.device
    n = int(beg.numel())
    if int(line_off.numel()) != n + 1 or int(end.numel()) != n:
        raise ValueError("write_piece: %d lines need %d offsets and %d ends" % (n, n + 1, n))
    slab_members = int(slab_members)
    if slab_members < 1:
        raise ValueError("write_piece: slab_members must be at least 1")
    u0, u1 = (int(x) for x in line_off[[0, n]].tolist())
    nbytes = u1 - u0
    ms = dict.fromkeys(STAGES + ("write",), 0.0)
    if n == 0 or nbytes <= 0:
        return dict(lines=0, bytes=0, text_bytes=0, members=0, run_bin=np.zeros(0, np.int32), run_vbeg=np.zeros(0, np.uint64),
                    run_vend=np.zeros(0, np.uint64), w0=0, win_min=np.zeros(0, np.uint64), ms=ms)
    ioff, ilen = member_spans(nbytes, base=u0)
    nm = int(ioff.size)
    S = min(slab_members, nm)
    d_ioff, d_ilen = torch.from_numpy(ioff).to(dev), torch.from_numpy(ilen).to(dev)
    pay = torch.empty(S * PAYLOAD_SLOT, dtype=torch.uint8, device=dev)
    poff = torch.arange(S, dtype=torch.int64, device=dev) * PAYLOAD_SLOT
    clen, crc, st = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(3))
    slab_foff = torch.empty(S + 1, dtype=torch.int64, device=dev)
    image = torch.empty(S * MEMBER_MAX + len(BGZF_EOF), dtype=torch.uint8, device=dev)
    foff = torch.empty(nm + 1, dtype=torch.int64, device=dev)            # the piece's members, for the index
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    host = _pinned_pair(eng, S * MEMBER_MAX)
    events = []                                                          # (stage, start, stop), resolved at the end

    def stage(what, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        events.append((what, e0, e1))
        return e1

    def flush(pending):
        if pending is not None:
            buf, size, done = pending
            done.synchronize()
            t0 = time.perf_counter()
            f.write(memoryview(buf.numpy())[:size])
            ms["write"] += (time.perf_counter() - t0) * 1e3

    base, pending = 0, None
    for turn, a in enumerate(range(0, nm, S)):
        k = min(S, nm - a)
        io, il = d_ioff[a:a + k], d_ilen[a:a + k]
        stage("deflate", lambda: eng.bgzf_deflate(text, io, il, pay, poff[:k], clen[:k], st[:k]))
        stage("crc", lambda: eng.bgzf_crc32(text, io, il, crc[:k]))
        stage("assemble", lambda: eng.bgzf_assemble(pay, poff[:k], clen[:k], crc[:k], il, slab_foff[:k + 1]))
        bad += st[:k].count_nonzero()
        flush(pending)                                                   # the slab before this one goes to the file while this one compresses
        size = int(slab_foff[k].item())                                  # (the trailing EOF block behind it is not copied)
        stage("assemble", lambda: eng.bgzf_assemble(pay, poff[:k], clen[:k], crc[:k], il, slab_foff[:k + 1], image))
        foff[a:a + k] = slab_foff[:k] + base
        buf = host[turn & 1]
        done = stage("d2h", lambda: buf[:size].copy_(image[:size], non_blocking=True))
        pending = (buf, size, done)
        base += size
    foff[nm] = base
    if int(bad.item()):
        raise _lib.NanoCallerHipError("nc_bgzf_deflate_device: %d of %d members failed" % (int(bad.item()), nm))
    flush(pending)
    box = {}
    stage("index", lambda: box.update(eng.lines_index(beg, end, line_off, u0, foff, min_shift=min_shift, depth=depth)))
    for what, e0, e1 in events:
        e1.synchronize()
        ms[what] += e0.elapsed_time(e1)
    return dict(lines=n, bytes=base, text_bytes=nbytes, members=nm, ms=ms, **box)

"""The haplotagged BAM of phase_run, written on the GPU: the built-in replacement for `whatshap haplotag --tag-supplementary | samtools view
-b -1 --write-index` (nanocaller_src/indelCaller.py:243-246) behind the device phaser (phase.py).  DESIGN.md section 13 states the rule.

`write_haplotagged_bam` takes the contig's inflated record stream as the device ingest holds it (device_bam.open_device_bam: a contig the
phaser has just loaded is neither read nor inflated again) and, all in HBM (csrc/nc_bamwrite.hip):

  records overlapping the region --nc_bam_retag_sizes / nc_bam_retag--> the record stream, HP / PS / PC dropped, HP + PS from the haplotag
  table appended --nc_bgzf_deflate_device--> one raw-deflate payload per 0xff00 bytes --nc_bgzf_crc32_device--> CRC-32s
  --nc_bgzf_assemble_device--> the BGZF file image --D2H--> the file

The CSI index is assembled here from the records' virtual offsets (numpy) and compressed on the device as well.  There is no host
compression on this path: without the device route (no index beside the input, a contig too large for HBM) it raises.
"""
from __future__ import annotations

import os
import struct
import time

import numpy as np

from . import _lib
from .bgzf import BGZF_BLOCK, BGZF_EOF, bam_header, bgzf_members, event_timed, member_spans, virtual_offsets
from .hts_index import index_bytes

PAYLOAD_SLOT = 65536            # room for one member's payload on the device (a stored block is 65,285 bytes at most)
PG_NAME = "nanocaller_amd"
CSI_MIN_SHIFT, CSI_DEPTH = 14, 5


# ------------------------------------------------------------------------------------------------------------ host pieces
def ps_tag(v) -> bytes:
    """the PS aux field as pysam's set_tag types an integer (WhatsHap's haplotag): the smallest of C / S / I that holds it (c / s / i
    below zero).  nc_bamwrite.hip's ps_type is the same rule."""
    v = int(v)
    if v >= 0:
        ty, fmt = ("C", "<B") if v <= 0xff else ("S", "<H") if v <= 0xffff else ("I", "<I")
    else:
        ty, fmt = ("c", "<b") if v >= -0x80 else ("s", "<h") if v >= -0x8000 else ("i", "<i")
    return b"PS" + ty.encode() + struct.pack(fmt, v)


def read_bam_header(path):
    """(header text, [(name, length), ...]) of a BAM file"""
    text, names, lengths, _ = bam_header(path)
    return text, list(zip(names, lengths))


def add_pg(text, cl=None):
    """the header text with one @PG line appended: ID unique in the header (nanocaller_amd, else nanocaller_amd.1, .2, ...),
    PN:nanocaller_amd, PP = the ID of the last @PG line before it when there is one"""
    lines = [ln for ln in text.split("\n") if ln]
    ids, last = set(), None
    for ln in lines:
        if ln.startswith("@PG\t"):
            for f in ln.split("\t")[1:]:
                if f.startswith("ID:"):
                    ids.add(f[3:])
                    last = f[3:]
    pid, k = PG_NAME, 0
    while pid in ids:
        k += 1
        pid = "%s.%d" % (PG_NAME, k)
    pg = "@PG\tID:%s\tPN:%s" % (pid, PG_NAME) + ("\tPP:%s" % last if last is not None else "") + ("\tCL:%s" % cl if cl else "")
    return "".join(ln + "\n" for ln in lines) + pg + "\n"


def header_bytes(text, refs):
    """the BAM header (SAMv1 4.2): magic, l_text, text, the reference list"""
    t = text.encode("ascii")
    out = [b"BAM\1", struct.pack("<i", len(t)), t, struct.pack("<i", len(refs))]
    for name, ln in refs:
        nb = name.encode("ascii") + b"\0"
        out.append(struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln))
    return b"".join(out)


def voffsets(stream_pos, first_member, member_foff, block=BGZF_BLOCK):
    """bgzf.virtual_offsets of positions in a record stream that starts at member `first_member`"""
    return virtual_offsets(stream_pos, member_foff, first_member, block)


def csi_index(n_ref, tid, beg, end, vbeg, vend, min_shift=CSI_MIN_SHIFT, depth=CSI_DEPTH) -> bytes:
    """CSIv1 index content (uncompressed, no auxiliary data) of a BAM whose records are all on reference `tid`: record k spans
    [beg[k], end[k]) (0-based) and occupies virtual offsets [vbeg[k], vend[k]).  Per bin its chunks (adjacent records merged) and
    `loffset` = the smallest virtual offset of a record overlapping the bin's first window (empty windows take the next window's), as
    samtools index -c writes them; no pseudo-bin"""
    n = len(beg)
    return index_bytes("csi", n_ref, np.full(n, tid), beg, end, np.zeros(n, bool), None, vbeg, vend, min_shift, depth, pseudo_bin=False)


def load_table(haplotags):
    """(hash uint64 ascending, hp uint8, ps int32) of a haplotag table: a path (phase.save_haplotags) or a dict of that form"""
    if isinstance(haplotags, (str, os.PathLike)):
        from .phase import load_haplotags
        return load_haplotags(str(haplotags))
    h = np.asarray(haplotags["hash"], np.uint64)
    o = np.argsort(h, kind="stable")
    return h[o], np.asarray(haplotags["hp"], np.uint8)[o], np.asarray(haplotags["ps"], np.int32)[o]


# ------------------------------------------------------------------------------------------------------------ device pieces
def deflate_members(eng, data, ioff, ilen, crc=True, ms=None):
    """BGZF payloads of the members data[ioff[b] : ioff[b] + ilen[b]] (data: a device uint8 tensor) -> (payload buffer, payload offsets,
    clen, crc, status) device tensors.  ms: dict that gets 'deflate' and 'crc' (ms, by events)"""
    import torch
    dev = eng.device
    n = int(len(ioff))
    d_ioff = torch.from_numpy(np.ascontiguousarray(ioff, np.int64)).to(dev)
    d_ilen = torch.from_numpy(np.ascontiguousarray(ilen, np.int32)).to(dev)
    pay = torch.empty(max(1, n) * PAYLOAD_SLOT, dtype=torch.uint8, device=dev)
    poff = torch.arange(n, dtype=torch.int64, device=dev) * PAYLOAD_SLOT
    clen = torch.zeros(n, dtype=torch.int32, device=dev)
    d_crc = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    eng.bgzf_deflate(data, d_ioff, d_ilen, pay, poff, clen, st)
    ev[1].record()
    if crc:
        eng.bgzf_crc32(data, d_ioff, d_ilen, d_crc)
    ev[2].record()
    if ms is not None:
        ev[2].synchronize()
        ms["deflate"] = ms.get("deflate", 0.0) + ev[0].elapsed_time(ev[1])
        ms["crc"] = ms.get("crc", 0.0) + ev[1].elapsed_time(ev[2])
    return pay, poff, clen, d_crc, st, d_ilen


def bgzf_compress_device(eng, data: bytes) -> bytes:
    """a small byte string (a header, an index) as a BGZF file: members of BGZF_BLOCK bytes compressed on the device, framed here"""
    import torch
    eng.use_torch_stream()
    raw = np.frombuffer(bytes(data), np.uint8)
    d = torch.from_numpy(raw.copy()).to(eng.device) if raw.size else torch.zeros(1, dtype=torch.uint8, device=eng.device)
    off, ln = member_spans(raw.size)
    pay, poff, clen, crc, st, _ = deflate_members(eng, d, off, ln)
    if int(st.count_nonzero().item()):
        raise _lib.NanoCallerHipError("nc_bgzf_deflate_device: status %s" % st.cpu().numpy().tolist())
    c, cr, p = clen.cpu().numpy(), crc.cpu().numpy().view(np.uint32), pay.cpu().numpy()
    return bgzf_members([p[k * PAYLOAD_SLOT:k * PAYLOAD_SLOT + int(c[k])] for k in range(off.size)], cr, ln)


def write_haplotagged_bam(sam_path, chrom, haplotags, out_path, start=None, end=None, device=0) -> dict:
    """Write `out_path` (BAM) and `out_path`.csi: the records of contig `chrom` of `sam_path` that overlap [start, end] (1-based,
    inclusive; None: the contig's bounds), in input order and whatever their flags, with HP / PS / PC dropped and, where the read name is
    in `haplotags` (phase.save_haplotags' table: a path or a dict), HP and PS appended.  -> dict of counts and milliseconds per stage"""
    import torch

    from .device_bam import M_POS, M_RLEN, DeviceIngestUnavailable, ensure_index, open_device_bam
    t_all = time.perf_counter()
    ms = {}
    ensure_index(sam_path, None, device)                                # (NC_BUILD_INDEX=1: an input without index gets one)
    try:
        db = open_device_bam(sam_path, device, contigs=[chrom])
    except DeviceIngestUnavailable as e:
        raise _lib.NanoCallerHipError("write_haplotagged_bam: %s cannot be re-tagged on the device (%s); there is no host writer" % (sam_path, e))
    eng = db.eng
    eng.use_torch_stream()
    dev = eng.device
    tid = db.ref_names.index(chrom)
    length = db.ref_lengths[tid]
    beg1 = 1 if start is None else max(1, int(start))
    end1 = length if end is None else int(end)
    a, b = db.tid_range.get(tid, (0, 0))
    pos = db.meta[M_POS, a:b].astype(np.int64)
    span = np.maximum(1, db.meta[M_RLEN, a:b]).astype(np.int64)
    sel = np.flatnonzero((pos < end1) & (pos + span > beg1 - 1))        # what an htslib region query returns
    n = int(sel.size)
    text, refs = read_bam_header(sam_path)
    hdr = header_bytes(add_pg(text), refs)
    hl = len(hdr)
    th, thp, tps = load_table(haplotags)

    timed = event_timed(ms)
    # ---- re-tag
    d_rec = torch.from_numpy(np.ascontiguousarray(db.rec_off[a + sel], np.int64)).to(dev)
    d_hash = torch.from_numpy(np.ascontiguousarray(th).view(np.int64)).to(dev)
    d_hp = torch.from_numpy(np.ascontiguousarray(thp)).to(dev)
    d_ps = torch.from_numpy(np.ascontiguousarray(tps)).to(dev)
    d_size = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    d_tag = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(1, dtype=torch.int32, device=dev)
    timed("retag", lambda: eng.bam_retag_sizes(db.raw, d_rec, d_hash, d_ps, d_size, d_tag, d_out_off, d_st))
    st = int(d_st.item())
    if st:
        raise _lib.NanoCallerHipError("%s, contig %s: records with malformed %s (nc_bam_retag_sizes status %d)"
                                      % (sam_path, chrom, "aux data" if st & 2 else "fixed fields", st))
    out_off = d_out_off.cpu().numpy()
    total = int(out_off[-1])
    stream = torch.empty(hl + total + 8, dtype=torch.uint8, device=dev)
    stream[:hl].copy_(torch.from_numpy(np.frombuffer(hdr, np.uint8).copy()))
    timed("retag", lambda: eng.bam_retag(db.raw, d_rec, d_hp, d_ps, d_tag, d_out_off, stream, out_byte_off=hl))
    # ---- members: the header's, flushed before the first record, then the records' as one stream
    ho, hln = member_spans(hl)
    ro, rln = member_spans(total, base=hl)
    ioff, ilen = np.concatenate([ho, ro]), np.concatenate([hln, rln])
    nm = int(ioff.size)
    pay, poff, clen, crc, dst, d_ilen = deflate_members(eng, stream, ioff, ilen, ms=ms)
    d_foff = torch.empty(nm + 1, dtype=torch.int64, device=dev)
    timed("assemble", lambda: eng.bgzf_assemble(pay, poff, clen, crc, d_ilen, d_foff))
    if int(dst.count_nonzero().item()):
        raise _lib.NanoCallerHipError("nc_bgzf_deflate_device: %d members failed" % int(dst.count_nonzero().item()))
    foff = d_foff.cpu().numpy()
    fsize = int(foff[-1]) + len(BGZF_EOF)
    file = torch.empty(fsize, dtype=torch.uint8, device=dev)
    timed("assemble", lambda: eng.bgzf_assemble(pay, poff, clen, crc, d_ilen, d_foff, file))
    t0 = time.perf_counter()
    host = torch.empty(fsize, dtype=torch.uint8, pin_memory=True)
    host.copy_(file)
    ms["d2h"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    with open(out_path, "wb") as f:
        f.write(memoryview(host.numpy()))
    ms["write"] = (time.perf_counter() - t0) * 1e3
    # ---- index
    t0 = time.perf_counter()
    vb = voffsets(out_off[:-1], ho.size, foff)
    ve = voffsets(out_off[1:], ho.size, foff)
    csi = csi_index(len(refs), tid, pos[sel], pos[sel] + span[sel], vb, ve)
    with open(out_path + ".csi", "wb") as f:
        f.write(bgzf_compress_device(eng, csi))
    ms["index"] = (time.perf_counter() - t0) * 1e3
    del stream, pay, file
    return dict(records=n, tagged=int((d_tag[:n] >= 0).sum().item()) if n else 0, inflated_bytes=hl + total, header_bytes=hl, bytes_out=fsize, members=nm, ms=ms, seconds=time.perf_counter() - t_all)

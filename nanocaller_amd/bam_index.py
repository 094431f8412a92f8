"""The index of an unindexed BAM, built on the GPU: the built-in replacement for `samtools index` in front of the device ingest
(device_bam.py needs a .bai / .csi; the reference needs one for pysam's fetch / pileup).  DESIGN.md section 6, "Indexing an unindexed BAM".

  file, piece by piece of whole BGZF members --H2D--> nc_inflate_device + nc_bgzf_crc_device --> the record stream of the piece, behind the
  bytes of the record the piece before ended in --nc_bamidx_candidates / _chain / _collect / _verify--> record offsets (proved; else
  nc_bamidx_serial) --nc_bam_meta + nc_bamidx_fields--> refID, span, bin, virtual offsets, sort check --D2H (36 B per record)-->
  [host, numpy: bins with chunks, linear index, pseudo-bins] --> .bai, or .csi compressed on the device

Between pieces travel the chain's carry (the offset of the first record that is not whole yet; its bytes are copied in front of the next piece)
and the sort state (refID and pos of the last record).  Nothing else is kept in HBM, so the size of the file does not matter.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import time

import numpy as np

from . import _lib

BAI_MAX_LEN = 1 << 29            # the longest reference a .bai (min_shift 14, depth 5) can address
MIN_SHIFT = 14
PIECE_BYTES = 128 << 20          # compressed bytes per piece (at most eight times that inflated, beside the 4/16 of it the chain's tables take)
INFLATE_BATCH = 4096             # members per nc_inflate_device call (256 KB of token workspace each)
LAST_INDEX = {}                  # the most recent build_index: seconds per stage, pieces, records, `serial_pieces` = pieces the proof sent to the serial walk
_STATUS_TEXT = [(2, "a record with a block_size below 32"), (4, "a record whose fixed fields overrun its block_size"),
                (8, "the record chain does not end where the data ends (the file stops inside a record, or the first record's offset is wrong)"),
                (16, "a record whose refID is not in the header's reference list"),
                (32, "the file is not coordinate-sorted (refID order broken, pos decreasing inside a contig, or a placed record behind the unplaced ones); "
                     "sort it first -- samtools index refuses such a file as well"),
                (64, "a record outside the BGZF member table")]


def status_error(path, st):
    err = _lib.NanoCallerHipError("%s cannot be indexed: %s (status %d)" % (path, "; ".join(t for b, t in _STATUS_TEXT if st & b) or "corrupt records", st))
    err.status = int(st)
    return err


def _vp(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off)


# ------------------------------------------------------------------------------------------------------------ device: one piece
def chain_piece(eng, d_buf, length, first, n_ref, d_ref_len, last=False, stats=None):
    """record starts of the piece d_buf[0, length) (uint8 device tensor, at least 16 bytes longer) from the record start `first` on
    -> (device int64 tensor of the offsets, their number, the carry, NC_BAMIDX_* status bits).  stats['serial_pieces'] counts the pieces whose
    speculative chain the proof did not accept."""
    import torch
    L, dev = _lib.lib(), eng.device
    if length >= 1 << 31:
        raise _lib.NanoCallerHipError("a piece of %d inflated bytes: more than 2^31 (choose a smaller piece_bytes)" % length)
    if d_buf.numel() < length + 16:
        raise ValueError("the piece's buffer must be readable 16 bytes past its length")
    n_words = -(-length // 4096) * 64
    words = torch.empty(n_words, dtype=torch.int64, device=dev)
    cnt = torch.empty(n_words, dtype=torch.int32, device=dev)
    eng._check(L.nc_bamidx_candidates(eng.ctx, _vp(d_buf), length, d_buf.numel(), n_ref, _vp(d_ref_len) if n_ref else None, _vp(words), _vp(cnt)),
               "nc_bamidx_candidates")
    incl = torch.cumsum(cnt, 0, dtype=torch.int32)
    rank = incl - cnt
    n_cand = int(incl[-1].item())
    res = torch.zeros(3, dtype=torch.int64, device=dev)
    n_rec, out = 0, torch.empty(1, dtype=torch.int64, device=dev)
    if n_cand:
        pos = torch.empty(n_cand, dtype=torch.int64, device=dev)
        jump = torch.empty(2 * (n_cand + 1), dtype=torch.int32, device=dev)
        mark = torch.empty(n_cand + 1, dtype=torch.int32, device=dev)
        eng._check(L.nc_bamidx_chain(eng.ctx, _vp(d_buf), length, first, _vp(words), _vp(rank), n_cand, _vp(pos), _vp(jump), _vp(mark)), "nc_bamidx_chain")
        mrank = torch.cumsum(mark[:n_cand], 0, dtype=torch.int32)
        n_rec = int(mrank[-1].item())
        out = torch.empty(max(1, n_rec), dtype=torch.int64, device=dev)
        eng._check(L.nc_bamidx_collect(eng.ctx, n_cand, _vp(pos), _vp(mark), _vp(mrank), _vp(out)), "nc_bamidx_collect")
    eng._check(L.nc_bamidx_verify(eng.ctx, _vp(d_buf), length, first, n_rec, _vp(out), int(bool(last)), _vp(res)), "nc_bamidx_verify")
    r = res.cpu().numpy()
    if stats is not None:
        stats["candidates"] = stats.get("candidates", 0) + n_cand
    if int(r[0]) & 1:                                                    # not proved: the exact serial chain
        if stats is not None:
            stats["serial_pieces"] = stats.get("serial_pieces", 0) + 1
        eng._check(L.nc_bamidx_serial(eng.ctx, _vp(d_buf), length, first, int(bool(last)), None, _vp(res)), "nc_bamidx_serial")
        n_rec = int(res[2].item())
        out = torch.empty(max(1, n_rec), dtype=torch.int64, device=dev)
        eng._check(L.nc_bamidx_serial(eng.ctx, _vp(d_buf), length, first, int(bool(last)), _vp(out), _vp(res)), "nc_bamidx_serial")
        r = res.cpu().numpy()
    return out, n_rec, int(r[1]), int(r[0]) & ~1


def _inflate_piece(eng, comp, coff, clen, isize, d_buf, out_off):
    """the members of the compressed bytes `comp` (numpy) -> d_buf[out_off:], CRC-32s checked; -> number of bad members"""
    import torch
    from .device_bam import CHECK_CRC, _work_buffer
    L, dev = _lib.lib(), eng.device
    n = int(coff.size)
    padded = np.zeros(comp.size + 64, np.uint8)
    padded[:comp.size] = comp
    d_comp = torch.from_numpy(padded).to(dev)
    ooff = np.zeros(n, np.int64)
    np.cumsum(isize[:-1], out=ooff[1:])
    ooff += out_off
    d64 = torch.from_numpy(np.concatenate([coff.astype(np.int64), ooff])).to(dev)
    d32 = torch.from_numpy(np.concatenate([clen.astype(np.int32), isize.astype(np.int32)])).to(dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    batch = min(INFLATE_BATCH, (n + 63) // 64 * 64)
    d_tok = _work_buffer(dev, "idx_tok", ((batch + 63) // 64) << 22, torch.int32)
    d_ntok = torch.zeros(batch, dtype=torch.int32, device=dev)
    for a in range(0, n, batch):
        k = min(batch, n - a)
        args = (k, _vp(d_comp), _vp(d64, 8 * a), _vp(d32, 4 * a), _vp(d_buf), _vp(d64, 8 * (n + a)), _vp(d32, 4 * (n + a)), _vp(status, 4 * a))
        eng._check(L.nc_inflate_device(eng.ctx, *args, _vp(d_tok), _vp(d_ntok)), "nc_inflate_device")
        if CHECK_CRC:
            eng._check(L.nc_bgzf_crc_device(eng.ctx, *args), "nc_bgzf_crc_device")
    return status


# ------------------------------------------------------------------------------------------------------------ host: the index from the records' arrays
def _ref_runs(refid, n_ref):
    """[a, b) of every reference's records in the (sorted) record list, and the number of unplaced ones"""
    key = np.where(refid < 0, n_ref, refid).astype(np.int64)
    edges = np.searchsorted(key, np.arange(n_ref + 1))
    return edges, int(refid.size - edges[n_ref])


def _ref_tables(beg, end, bins, vbeg, vend, min_shift):
    """one reference: (bin ids ascending, first chunk of each, chunk counts, chunk begins, chunk ends, linear index with the empty windows
    still at the uint64 maximum)"""
    w0, w1 = beg >> min_shift, (end - 1) >> min_shift
    n_win = int(w1.max()) + 1
    big = np.uint64(np.iinfo(np.uint64).max)
    lin = np.full(n_win, big, np.uint64)
    cnt = w1 - w0 + 1
    rows = np.repeat(np.arange(beg.size), cnt)
    win = w0[rows] + (np.arange(rows.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    np.minimum.at(lin, win, vbeg[rows])
    o = np.argsort(bins, kind="stable")                                  # the records of a bin in file order; adjacent ones form one chunk
    sb, svb, sve = bins[o], vbeg[o], vend[o]
    new = np.ones(sb.size, bool)
    new[1:] = (sb[1:] != sb[:-1]) | (svb[1:] != sve[:-1])
    starts = np.flatnonzero(new)
    ends = np.concatenate([starts[1:], [sb.size]]) - 1
    ub, first = np.unique(sb[starts], return_index=True)
    n_ch = np.diff(np.concatenate([first, [starts.size]]))
    return ub, first, n_ch, svb[starts], sve[ends], lin


def _chunks_blob(cb, ce):
    c = np.empty(2 * cb.size, np.uint64)
    c[0::2], c[1::2] = cb, ce
    return c.astype("<u8").tobytes()


def index_bytes(fmt, n_ref, refid, beg, end, unmapped, bins, vbeg, vend, min_shift=MIN_SHIFT, depth=5) -> bytes:
    """the .bai (SAMv1 5.2) or the uncompressed .csi (hts-specs CSIv1, no auxiliary data) of a coordinate-sorted BAM from its records' arrays
    in file order: refID, the 0-based span [beg, end) each is indexed under, flag & 4, bin, virtual offsets of its first byte and of the byte
    behind it.  Per reference: the bins with their chunks, the pseudo-bin (virtual offsets of the reference's first and behind its last record;
    mapped and unmapped counts), and -- .bai -- the linear index, an empty window taking the offset of the window before it as samtools writes
    it, or -- .csi -- every bin's loffset = the linear index at the bin's first window, an empty one taking the next one's."""
    from .bam_write import _bin_first_window
    refid, beg, end = np.asarray(refid, np.int64), np.asarray(beg, np.int64), np.asarray(end, np.int64)
    vbeg, vend, bins = np.asarray(vbeg, np.uint64), np.asarray(vend, np.uint64), np.asarray(bins, np.int64)
    unmapped = np.asarray(unmapped, bool)
    bai = fmt == "bai"
    out = [b"BAI\1" + struct.pack("<i", n_ref)] if bai else [b"CSI\1", struct.pack("<3i", min_shift, depth, 0), struct.pack("<i", n_ref)]
    meta_bin = ((1 << (depth * 3 + 3)) - 1) // 7 + 1
    big = np.uint64(np.iinfo(np.uint64).max)
    edges, n_no_coor = _ref_runs(refid, n_ref)
    for r in range(n_ref):
        a, b = int(edges[r]), int(edges[r + 1])
        if a == b:
            out.append(struct.pack("<ii", 0, 0) if bai else struct.pack("<i", 0))
            continue
        ub, first, n_ch, cb, ce, lin = _ref_tables(beg[a:b], end[a:b], bins[a:b], vbeg[a:b], vend[a:b], min_shift)
        n_win = lin.size
        if bai:
            idx = np.where(lin != big, np.arange(n_win), -1)
            idx = np.maximum.accumulate(idx)
            lin_out = np.where(idx >= 0, lin[np.maximum(idx, 0)], np.uint64(0))
            loff = None
        else:
            idx = np.where(lin != big, np.arange(n_win), n_win)
            idx = np.minimum.accumulate(idx[::-1])[::-1]
            filled = np.concatenate([lin, [np.uint64(0)]])[idx]
            wdx = _bin_first_window(ub, depth)
            loff = np.where(wdx < n_win, filled[np.minimum(wdx, n_win - 1)], np.uint64(0))
        blob = [struct.pack("<i", ub.size + 1)]
        for k in range(ub.size):
            s = int(first[k])
            head = struct.pack("<Ii", int(ub[k]), int(n_ch[k])) if bai else struct.pack("<IQi", int(ub[k]), int(loff[k]), int(n_ch[k]))
            blob.append(head + _chunks_blob(cb[s:s + n_ch[k]], ce[s:s + n_ch[k]]))
        n_un = int(np.count_nonzero(unmapped[a:b]))
        pseudo = struct.pack("<QQQQ", int(vbeg[a:b].min()), int(vend[a:b].max()), b - a - n_un, n_un)
        blob.append((struct.pack("<Ii", meta_bin, 2) if bai else struct.pack("<IQi", meta_bin, 0, 2)) + pseudo)
        if bai:
            blob.append(struct.pack("<i", n_win) + lin_out.astype("<u8").tobytes())
        out.append(b"".join(blob))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------------ the file
def read_header(path):
    """(reference names, reference lengths, offset of the first record in the inflated stream) of a BAM file; the header may span many members"""
    from .device_bam import DeviceBam
    probe = DeviceBam.__new__(DeviceBam)
    probe.path, probe.file_bytes = path, os.path.getsize(path)
    probe._read_header()
    return list(probe.ref_names), list(probe.ref_lengths), int(probe.header_len)


def scan_records(path, device=0, piece_bytes=None, depth=5, keep_offsets=False):
    """The device half of build_index: the file through HBM piece by piece -> dict of per-record numpy arrays in file order (refid, flag, bin,
    beg, end, vbeg, vend; with keep_offsets also `offset`, every record's offset in the inflated stream) and LAST_INDEX's counters and stage
    times.  Raises NanoCallerHipError (with .status, NC_BAMIDX_* bits) for a file that is corrupt or not coordinate-sorted."""
    import torch

    from .device_bam import META_COLS
    from .engine import get_engine
    t_all = time.perf_counter()
    names, lengths, first_record = read_header(path)
    n_ref = len(names)
    piece_bytes = int(piece_bytes or PIECE_BYTES)
    eng, L = get_engine(device), _lib.lib()
    eng.use_torch_stream()
    dev = eng.device
    d_ref_len = torch.from_numpy(np.asarray(lengths or [0], np.int32)).to(dev)
    stats = dict(pieces=0, serial_pieces=0, candidates=0, members=0)
    ms = dict(inflate=0.0, chain=0.0, fields=0.0)
    cols = []                                                            # per piece: (refid, flag, bin, beg, end, vbeg, vend, offset)
    mem_ooff, mem_foff = np.zeros(0, np.int64), np.zeros(0, np.int64)   # the members from the carry's on: first byte in the inflated stream / in the file
    g_total, g_carry = 0, first_record                          # inflated bytes so far; stream offset of the first record that is not indexed yet
    tail = None                                                          # its bytes, when some of them are inflated already (device tensor)
    has_prev, prev_refid, prev_pos = 0, 0, 0
    file_size, base, leftover, seen_last = os.path.getsize(path), 0, b"", False

    def timed(what, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        ms[what] += e0.elapsed_time(e1)
        return r
    with open(path, "rb") as f:
        while not seen_last:
            chunk = f.read(piece_bytes)
            buf = np.frombuffer(leftover + chunk, np.uint8)
            if buf.size == 0:
                raise _lib.NanoCallerHipError("%s does not end with a whole BGZF member" % path)
            cap = buf.size // 28 + 16
            coff, clen, isize = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap, np.int32)
            k, nxt = C.c_int64(), C.c_int64()
            rc = L.nc_bgzf_scan(_lib.npp(buf), buf.size, 0, cap, _lib.npp(coff), _lib.npp(clen), _lib.npp(isize), C.byref(k), C.byref(nxt))
            if rc != _lib.NC_OK:
                raise _lib.NanoCallerHipError("%s is not a BGZF file (nc_bgzf_scan: %d at byte %d)" % (path, rc, base))
            k, nxt = int(k.value), int(nxt.value)
            if k == 0:
                if not chunk:
                    raise _lib.NanoCallerHipError("%s does not end with a whole BGZF member" % path)
                leftover = buf.tobytes()
                continue
            coff, clen, isize = coff[:k], clen[:k], isize[:k]
            seen_last = base + nxt == file_size
            n_inf = int(isize.sum(dtype=np.int64))
            mstart = np.empty(k, np.int64)
            mstart[0] = 0
            mstart[1:] = coff[:-1] + clen[:-1] + 8
            oo = np.zeros(k, np.int64)
            np.cumsum(isize[:-1], out=oo[1:])
            mem_ooff, mem_foff = np.concatenate([mem_ooff, oo + g_total]), np.concatenate([mem_foff, mstart + base])
            g0, g1 = g_total, g_total + n_inf
            stats["pieces"] += 1
            stats["members"] += k
            if g_carry < g1:                                             # (else: the header, or one long record, goes on behind this piece)
                t_len = int(tail.numel()) if tail is not None else 0
                assert t_len == max(0, g0 - g_carry)
                length = t_len + n_inf
                d_buf = torch.empty(length + 64, dtype=torch.uint8, device=dev)
                d_buf[length:].zero_()
                if t_len:
                    d_buf[:t_len].copy_(tail)
                status = timed("inflate", lambda: _inflate_piece(eng, buf[:nxt], coff, clen, isize, d_buf, t_len))
                bad = int(status.count_nonzero().item())
                if bad:
                    crc = int((status == 7).sum().item())
                    raise _lib.NanoCallerHipError("%s: %d BGZF members are not valid deflate streams of their announced size%s"
                                                  % (path, bad - crc, (", %d fail their CRC-32" % crc) if crc else ""))
                stream_base = g0 - t_len
                first = g_carry - stream_base
                d_out, n_rec, carry, st = timed("chain", lambda: chain_piece(eng, d_buf, length, first, n_ref, d_ref_len, seen_last, stats))
                if st:
                    raise status_error(path, st)
                if n_rec:
                    d_moo = torch.from_numpy(np.concatenate([mem_ooff, [g1]])).to(dev)
                    d_mfo = torch.from_numpy(np.concatenate([mem_foff, [base + nxt]])).to(dev)
                    d_meta = torch.empty((META_COLS, n_rec), dtype=torch.int32, device=dev)
                    d_voff = torch.empty((2, n_rec), dtype=torch.int64, device=dev)
                    d_fld = torch.empty((3, n_rec), dtype=torch.int32, device=dev)
                    d_st = torch.zeros(1, dtype=torch.int32, device=dev)

                    def fields():
                        eng._check(L.nc_bam_meta(eng.ctx, _vp(d_buf), n_rec, _vp(d_out), _vp(d_meta), _vp(d_st)), "nc_bam_meta")
                        eng._check(L.nc_bamidx_fields(eng.ctx, _vp(d_buf), n_rec, _vp(d_out), stream_base, _vp(d_meta), n_ref, int(d_moo.numel()) - 1,
                                                      _vp(d_moo), _vp(d_mfo), has_prev, prev_refid, prev_pos, MIN_SHIFT, depth, _vp(d_voff), _vp(d_fld),
                                                      _vp(d_st)), "nc_bamidx_fields")
                    timed("fields", fields)
                    st = int(d_st.item())
                    if st:
                        raise status_error(path, st)
                    meta, voff, fld = d_meta[:3].cpu().numpy(), d_voff.cpu().numpy().view(np.uint64), d_fld.cpu().numpy()
                    cols.append((meta[0], meta[2], fld[0], fld[1], fld[2], voff[0], voff[1],
                                 d_out[:n_rec].cpu().numpy() + stream_base if keep_offsets else None))
                    has_prev, prev_refid, prev_pos = 1, int(meta[0][-1]), int(meta[1][-1])
                g_carry = stream_base + carry
                tail = d_buf[carry:length].clone() if carry < length else None
                del d_buf
            elif seen_last and g_carry > g1:
                raise status_error(path, 8)
            m0 = mem_ooff.size
            if tail is not None:                                         # the first member that starts at the carry, else the one that holds it
                m0 = int(np.searchsorted(mem_ooff, g_carry, side="left"))
                if m0 == mem_ooff.size or mem_ooff[m0] != g_carry:
                    m0 -= 1
            mem_ooff, mem_foff = mem_ooff[m0:], mem_foff[m0:]            # the members before the carry's are done with
            g_total, base, leftover = g1, base + nxt, buf[nxt:].tobytes()
    cat = lambda j, dt: np.concatenate([c[j] for c in cols]).astype(dt) if cols else np.zeros(0, dt)   # noqa: E731
    rec = dict(refid=cat(0, np.int64), flag=cat(1, np.int64), bin=cat(2, np.int64), beg=cat(3, np.int64), end=cat(4, np.int64), vbeg=cat(5, np.uint64),
               vend=cat(6, np.uint64))
    if keep_offsets:
        rec["offset"] = cat(7, np.int64)
    LAST_INDEX.clear()
    LAST_INDEX.update(stats, records=int(rec["refid"].size), inflated_bytes=g_total, inflate_s=ms["inflate"] * 1e-3, chain_s=ms["chain"] * 1e-3,
                      fields_s=ms["fields"] * 1e-3, scan_s=time.perf_counter() - t_all)
    return rec


def build_index(path, fmt=None, device=0, piece_bytes=None):
    """Write the index of the coordinate-sorted BAM `path` beside it and return its path: <path>.bai, or <path>.csi (min_shift 14; depth 5, or 6
    for a reference beyond 2^29) with fmt='csi' or when a reference is longer than 2^29.  piece_bytes: compressed bytes per piece."""
    from .bam_write import bgzf_compress_device
    from .engine import get_engine
    t_all = time.perf_counter()
    names, lengths, _ = read_header(path)
    n_ref, longest = len(names), max(lengths) if lengths else 0
    if fmt is None:
        fmt = "csi" if longest > BAI_MAX_LEN else "bai"
    if fmt not in ("bai", "csi"):
        raise ValueError("fmt must be 'bai' or 'csi'")
    if fmt == "bai" and longest > BAI_MAX_LEN:
        raise ValueError("%s has a reference of %d bases: a .bai addresses 2^29, ask for fmt='csi'" % (path, longest))
    depth = 5
    while fmt == "csi" and (1 << (MIN_SHIFT + 3 * depth)) < longest:
        depth += 1
    rec = scan_records(path, device, piece_bytes, depth)
    eng = get_engine(device)
    t0 = time.perf_counter()
    data = index_bytes(fmt, n_ref, rec["refid"], rec["beg"], rec["end"], (rec["flag"] & 4) != 0, rec["bin"], rec["vbeg"], rec["vend"], MIN_SHIFT, depth)
    if fmt == "csi":
        data = bgzf_compress_device(eng, data)
    out = path + "." + fmt
    tmp = "%s.tmp%d" % (out, os.getpid())
    try:
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, out)
    except OSError as e:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise _lib.NanoCallerHipError("the index of %s cannot be written beside it (%s): index it where the directory is writable, or run without "
                                      "build_index (the host route needs no index)" % (path, e))
    LAST_INDEX.update(format=fmt, depth=depth, assemble_s=time.perf_counter() - t0, seconds=time.perf_counter() - t_all)
    return out

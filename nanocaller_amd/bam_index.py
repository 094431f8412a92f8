"""The index of an unindexed BAM, built on the GPU: the built-in replacement for `samtools index` in front of the device ingest
(device_bam.py needs a .bai / .csi; the reference needs one for pysam's fetch / pileup).  DESIGN.md section 6, "Indexing an unindexed BAM".

  file, piece by piece of whole BGZF members --H2D--> nc_inflate_device + nc_bgzf_crc_device --> the record stream of the piece, behind the
  bytes of the record the piece before ended in --nc_bamidx_candidates / _chain / _collect / _verify--> record offsets (proved; else
  nc_bamidx_serial) --nc_bam_meta + nc_bamidx_fields--> refID, span, bin, virtual offsets, sort check --D2H (36 B per record)-->
  [host, numpy, hts_index.index_bytes: bins with chunks, linear index, pseudo-bins] --> .bai, or .csi compressed on the device

Between pieces travel the chain's carry (the offset of the first record that is not whole yet; its bytes are copied in front of the next piece)
and the sort state (refID and pos of the last record).  Nothing else is kept in HBM, so the size of the file does not matter.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _lib, bgzf
from .hts_index import index_bytes           # (the writer of both formats; importable from here as before)

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
    return _lib.NanoCallerHipError("%s cannot be indexed: %s (status %d)" % (path, "; ".join(t for b, t in _STATUS_TEXT if st & b) or "corrupt records", st),
                                   status=int(st))


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


def _inflate_piece(eng, comp, coff, clen, isize, ooff, d_buf, out_off):
    """the members of the compressed bytes `comp` (numpy; ooff: bgzf.member_table's inflated offsets) -> d_buf[out_off:], CRC-32s checked;
    -> status per member"""
    import torch
    dev = eng.device
    padded = np.zeros(comp.size + 64, np.uint8)
    padded[:comp.size] = comp
    d_comp = torch.from_numpy(padded).to(dev)
    d64 = torch.from_numpy(np.concatenate([coff, ooff[:-1] + out_off])).to(dev)
    d32 = torch.from_numpy(np.concatenate([clen, isize])).to(dev)
    return bgzf.inflate_members(eng, d_comp, d64, d32, int(coff.size), d_buf, INFLATE_BATCH, "idx_tok")


# ------------------------------------------------------------------------------------------------------------ the file
def read_header(path):
    """(reference names, reference lengths, offset of the first record in the inflated stream) of a BAM file; the header may span many members"""
    return bgzf.bam_header(path)[1:]


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
    timed = bgzf.event_timed(ms)
    with open(path, "rb") as f:
        while not seen_last:
            chunk = f.read(piece_bytes)
            buf = np.frombuffer(leftover + chunk, np.uint8)
            if buf.size == 0:
                raise _lib.NanoCallerHipError("%s does not end with a whole BGZF member" % path)
            try:
                coff, clen, isize, nxt = bgzf.scan_members(buf)
            except bgzf.ScanError as e:
                raise _lib.NanoCallerHipError("%s is not a BGZF file (nc_bgzf_scan: %d at byte %d)" % (path, e.rc, base))
            k = int(coff.size)
            if k == 0:
                if not chunk:
                    raise _lib.NanoCallerHipError("%s does not end with a whole BGZF member" % path)
                leftover = buf.tobytes()
                continue
            seen_last = base + nxt == file_size
            mstart, oo = bgzf.member_table(coff, clen, isize)
            n_inf = int(oo[-1])
            mem_ooff, mem_foff = np.concatenate([mem_ooff, oo[:-1] + g_total]), np.concatenate([mem_foff, mstart + base])
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
                status = timed("inflate", lambda: _inflate_piece(eng, buf[:nxt], coff, clen, isize, oo, d_buf, t_len))
                err = bgzf.bad_members_error(path, [status])
                if err:
                    raise err
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

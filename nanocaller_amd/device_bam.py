"""BAM -> read pack on the device (csrc/nc_inflate.hip, csrc/nc_ingest.hip).

The reference reads alignments through pysam / htslib (generate_SNP_pileups.py:134-164).  The host route of this package inflates and
decodes them on worker threads (bam.py, nc_bam.cpp), diffs them against the reference and sends the difference over PCIe (wire.py).  Here
the FILE crosses PCIe as it is -- a BAM is already a compressed form of the pack -- and everything else happens in HBM:

  file image (page-locked) --H2D--> BGZF payloads --nc_inflate_device--> record stream --nc_bam_walk (.bai entries as chain starts)-->
  record offsets --nc_bam_meta--> per-record fields --D2H (48 B per record)--> [host: which reads are kept, tile index] --H2D-->
  nc_bam_codes --> the position-addressed codes of the pack

Which reads the pileup keeps (flag filter, htslib's depth cap, the unsupported-input checks) and the tile index are decided on the host
from the per-record fields with the same functions the host route uses, so a `DevicePack` made here is byte for byte the one
`wire.upload_wire(build_wire_from_world(bam.read_bam(...)))` makes (tests/test_device_bam.py); `pack(indel=True)` adds the indel path's sections.
Needs an index beside the file: a .bai's linear index, or a .csi's bin offsets and chunk begins, cut the record chain into independent walks.
A file without one is indexed here, on the GPU, by `build_index` (bam_index.py) -- the callers do so when asked (`ensure_index`).
"""
from __future__ import annotations

import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, bgzf, hts_index
from .engine import DevicePack, get_engine
from .pack import mate_table, name_groups, pileup_depth_cap
from .synth import FLAG_FILTER_DEFAULT, FLAG_FILTER_SUPPL

META_COLS = 12
(M_REFID, M_POS, M_FLAG, M_RLEN, M_LSEQ, M_HASSEQ, M_HAP, M_PS, M_HASH_LO, M_HASH_HI, M_NCIG, M_CIGD) = range(META_COLS)
CHECK_CRC = os.environ.get("NC_BGZF_CRC", "1") != "0"     # CRC-32 of every inflated member on the device (NC_BGZF_CRC=0: lengths only, as in round 4)
TRACE_LOAD = os.environ.get("NC_LOAD_TRACE") == "1"
LZ_SERIAL = os.environ.get("NC_LZ_SERIAL", "0") == "1"     # the match resolution behind the Huffman kernel on ONE stream instead of beside the next batch's
INFLATE_BATCH = int(os.environ.get("NC_INFLATE_BATCH", 28672))   # members per nc_inflate_device call: one full round of k_huff (256 CUs x 7 workgroups x 16 lanes); 7.5 GB of token workspace each, two in flight
POOL_MAX = 16 << 30              # buffers up to this size stay allocated between loads (larger ones go back to the allocator after use)
MAX_RESIDENT = 96 << 30          # upper bound of the inflated bytes kept in HBM at once; resident_limit() lowers it to what the device has free


def resident_limit(device=0):
    """inflated bytes one share of a file may take on `device`: the loader holds the stream (sized 8 x + 12.5 % of the compressed bytes), the file
    image (1/8 of the stream) and <= 8 GB of tokens; the read packs, the indel pipeline's workspaces and the CNN's need room beside them (two token workspaces of 7.5 GB at the default batch) -- half of
    what is free now (plus what this module's own pools already hold), at most MAX_RESIDENT"""
    try:
        free, _total = torch.cuda.mem_get_info(device)
        # blocks torch's caching allocator holds but has handed back (a released share larger than POOL_MAX lands there) are invisible to
        # mem_get_info and are served to the next torch.empty all the same: they count as free
        free += max(0, torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device))
    except Exception:
        return MAX_RESIDENT
    pooled = sum(t[0].numel() for k, t in _RAW_POOL.items() if k == device) + sum(t.numel() * t.element_size() for k, t in _WORK_POOL.items() if k[0] == device)
    # (the pools' tensors are torch allocations: part of memory_allocated, so they are added back here as the loader re-uses them)
    return int(max(1 << 30, min(MAX_RESIDENT, (free + pooled) // 2)))


LAST_LOAD = {}                   # seconds per stage of the most recent DeviceBam construction + load() (bench.py reports them)


class DeviceIngestUnavailable(RuntimeError):
    """the input cannot take the device route (no .bai, too large): the caller falls back to the host route"""


def _bai_path(path):
    """the index beside the BAM: .bai, else .csi (None: the device route is not available)"""
    for ext in (".bai", ".csi"):
        for p in (path + ext, os.path.splitext(path)[0] + ext):
            if os.path.exists(p):
                return p
    return None


_BAI = {}


def bai_linear_voffsets(bai_path):
    """{reference index: uint64 array of the non-zero virtual offsets of its 16 kb windows} (SAM specification 5.2); parsed once per file"""
    st = os.stat(bai_path)
    key = (os.path.abspath(bai_path), st.st_size, st.st_mtime_ns)
    if key not in _BAI:
        _BAI.clear()
        _BAI[key] = (hts_index.csi_record_starts if bai_path.endswith(".csi") else hts_index.bai_linear_voffsets)(bai_path)
    return _BAI[key]


class DeviceBam:
    """One BAM file: inflated and indexed in HBM by `load()`, then `prepare()` (host half, thread-safe) + `pack()` (device half) per contig."""

    def __init__(self, path, device=0, threads=None, contigs=None):
        """contigs: only these are wanted (a rank's share of a genome): the part of the file from the first record of the first of them to the
        first record behind the last is read and inflated, nothing else"""
        self.path, self.device = path, device
        self.eng = get_engine(device)
        bai = _bai_path(path)
        if bai is None:
            raise DeviceIngestUnavailable("%s: no .bai / .csi beside it" % path)
        self.lin = bai_linear_voffsets(bai)
        from .bam import rank_threads
        self.threads = threads or rank_threads()
        self.file_bytes = os.path.getsize(path)
        _, self.ref_names, self.ref_lengths, self.header_len = bgzf.bam_header(path)
        self.B0, self.B1, self.tids = 0, self.file_bytes, None
        if contigs is not None:
            unknown = [c for c in contigs if c not in self.ref_names]
            if unknown:
                raise ValueError("%s has no contig %r" % (path, unknown[0]))
            self.tids = sorted({self.ref_names.index(c) for c in contigs})
            have = [t for t in self.tids if t in self.lin and self.lin[t].size]
            if have:
                self.B0 = int(self.lin[have[0]][0] >> np.uint64(16))
                later = [t for t in sorted(self.lin) if t > have[-1] and self.lin[t].size]
                if later:                                                # through the member that holds the next contig's first record
                    self.B1 = min(self.file_bytes, int(self.lin[later[0]][0] >> np.uint64(16)) + 65536 + 1024)
            else:
                self.B1 = 0                                              # none of them has an alignment
        self.n_bytes = self.B1 - self.B0
        if self.n_bytes * 8 > resident_limit(device):                    # (the loader reserves eight times the compressed size for the inflated stream)
            raise DeviceIngestUnavailable("%s (%.1f GB to load): more than is kept in HBM at once" % (path, self.n_bytes / 1e9))
        self.loaded = False

    def voffset_to_stream(self, voff):
        """virtual offsets (coffset << 16 | uoffset) -> offsets into the inflated stream"""
        voff = np.asarray(voff, np.uint64)
        co = (voff >> np.uint64(16)).astype(np.int64) - self.B0          # (member offsets are relative to the part of the file that was read)
        m = np.searchsorted(self.mstart, co)
        if m.size and (m.max() >= len(self.mstart) or not np.array_equal(self.mstart[m], co)):
            raise _lib.NanoCallerHipError("%s: an index entry does not point at a BGZF member" % self.path)
        return self.ooff[m] + (voff & np.uint64(0xffff)).astype(np.int64)

    # ------------------------------------------------------------------ the file, once
    def load(self):
        """The file -> HBM, inflated: worker threads read it into page-locked memory piece by piece; as soon as the pieces read so far hold
        INFLATE_BATCH more whole members their bytes are copied (copy stream) and inflated (compute stream) -- the GPU works while the rest
        of the file is still being read.  Then the record walk and the per-record fields."""
        if self.loaded:
            return self
        import time
        eng, L, dev = self.eng, _lib.lib(), self.eng.device
        eng.use_torch_stream()
        vp = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)   # noqa: E731
        t_start = time.perf_counter()
        n = self.n_bytes
        self.host_buf = torch.empty(n + 64, dtype=torch.uint8, pin_memory=True)
        t_pin = time.perf_counter() - t_start
        data = self.host_buf.numpy()
        data[n:] = 0
        view = memoryview(data)
        piece = max(32 << 20, -(-n // 64))
        fd = os.open(self.path, os.O_RDONLY)

        def read_piece(a):                                               # (buffer offsets; the file's are B0 higher)
            b_, o = min(n, a + piece), a
            while o < b_:
                got = os.preadv(fd, [view[o:b_]], self.B0 + o)
                if got <= 0:
                    raise IOError("short read of %s" % self.path)
                o += got
            return b_
        # half the rank's thread budget, at most eight: with the whole budget reading, the caller's other threads (reference letters, the launching
        # thread) push the process over its CPU quota and the scheduler throttles all of them for the rest of the period (measured: 22 -> 270 ms)
        pool = ThreadPoolExecutor(max_workers=max(2, min(self.threads // 2, 8)))
        futures = [pool.submit(read_piece, a) for a in range(0, n, piece)]
        raw_cap = n * 8 + (64 << 20)                                     # the inflated size is known only at the end: room for eight-fold
        # the stream's buffer is kept from load to load (share after share of a genome-sized file, run after run of a bench): a fresh multi-gigabyte
        # request that misses the allocator's cache makes it release and re-acquire device memory, which was seen to take > 100 ms
        import weakref
        pooled = _RAW_POOL.get(dev.index)
        if pooled is not None and pooled[0].numel() >= raw_cap and pooled[1]() in (None, self):
            self.raw = pooled[0]
        else:
            self.raw = torch.empty(raw_cap + raw_cap // 8, dtype=torch.uint8, device=dev)
        if self.raw.numel() <= POOL_MAX:
            _RAW_POOL[dev.index] = (self.raw, weakref.ref(self))
        else:
            _RAW_POOL.pop(dev.index, None)
        d_file = _work_buffer(dev, "file", n + 64, torch.uint8)
        cap = n // 1024 + 4096
        stage64 = torch.empty(2 * cap, dtype=torch.int64, pin_memory=True)    # [coff | ooff] of every member, page-locked: the batches' uploads are async
        stage32 = torch.empty(2 * cap, dtype=torch.int32, pin_memory=True)    # [clen | isize]
        coff, ooff = stage64.numpy()[:cap], stage64.numpy()[cap:]
        clen, isize = stage32.numpy()[:cap], stage32.numpy()[cap:]
        # two token workspaces: the Huffman kernel of batch i + 1 (compute stream) runs beside the match resolution of batch i (its own stream)
        # (256 KB of tokens per member: a small file gets small workspaces -- and, should its members be unusually short, more batches)
        batch = min(INFLATE_BATCH, max(64, (n // 4096 + 63) // 64 * 64))
        toks = [(bgzf.token_workspace(dev, "tok%d" % k_, batch), torch.zeros(batch, dtype=torch.int32, device=dev), [None])
                for k_ in range(2)]
        t_alloc = time.perf_counter() - t_start
        copy_stream, lz_stream = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        compute = torch.cuda.current_stream(dev)
        lz_stream.wait_stream(compute)                                   # (the output buffer's allocation)
        n_batches = [0]
        n_mem, m0, scan_pos, total, statuses, keep = 0, 0, 0, 0, [], []
        traces = []

        pending = []                                                     # the batch whose bytes are on their way and whose kernels are not enqueued yet

        def kernels():
            """the inflate of the pending batch.  It is enqueued AFTER the next batch's copy: a host-to-device copy submitted while k_huff runs was
            seen to start only when that kernel ended (batch i + 1's 20 ms of PCIe behind batch i's 27 ms of Huffman decoding instead of under them)"""
            if not pending:
                return
            k, d64, d32, ev, tr, t_host, nbytes = pending.pop()

            def mark(stream, what):
                if tr is not None:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record(stream)
                    tr.append((what, e))
            compute.wait_event(ev)
            st = torch.zeros(k, dtype=torch.int32, device=dev)
            d_tok, d_ntok, lz_done = toks[n_batches[0] & 1]
            n_batches[0] += 1
            if lz_done[0] is not None:
                compute.wait_event(lz_done[0])                           # the workspace's previous tokens have been resolved
            args = (k, vp(d_file), vp(d64[0]), vp(d32[0]), vp(self.raw), vp(d64[1]), vp(d32[1]), vp(st), vp(d_tok), vp(d_ntok))
            mark(compute, "huff0")
            eng._check(L.nc_inflate_device_phase(eng.ctx, 1, *args), "nc_inflate_device_phase")
            mark(compute, "huff1")
            huffed = torch.cuda.Event()
            huffed.record(compute)
            with torch.cuda.stream(compute if LZ_SERIAL else lz_stream):
                (compute if LZ_SERIAL else lz_stream).wait_event(huffed)
                eng.use_torch_stream()
                mark(compute if LZ_SERIAL else lz_stream, "lz0")
                eng._check(L.nc_inflate_device_phase(eng.ctx, 2, *args), "nc_inflate_device_phase")
                mark(compute if LZ_SERIAL else lz_stream, "lz1")
                if CHECK_CRC:                                            # what htslib does for every block it inflates: the member's CRC-32 against its trailer
                    eng._check(L.nc_bgzf_crc_device(eng.ctx, *args[:8]), "nc_bgzf_crc_device")
                mark(compute if LZ_SERIAL else lz_stream, "crc1")
                lz_done[0] = torch.cuda.Event()
                lz_done[0].record(compute if LZ_SERIAL else lz_stream)
            if tr is not None:
                traces.append((t_host, k, nbytes, tr))
            eng.use_torch_stream()
            statuses.append(st)
            keep.append((d64, d32))                                      # (allocated on the copy stream, read on the compute stream: alive until the sync)

        def launch(m1):
            nonlocal m0
            a_byte = int(coff[m0 - 1]) + int(clen[m0 - 1]) + 8 if m0 else 0   # (from the batch's first member; the headers ride along)
            b_byte = int(coff[m1 - 1]) + int(clen[m1 - 1]) + 8
            k = m1 - m0
            tr = [] if TRACE_LOAD else None
            with torch.cuda.stream(copy_stream):
                if tr is not None:                                       # (NC_LOAD_TRACE=1: where a load's time goes, by events)
                    e = torch.cuda.Event(enable_timing=True)
                    e.record(copy_stream)
                    tr.append(("copy0", e))
                d_file[a_byte:b_byte].copy_(self.host_buf[a_byte:b_byte], non_blocking=True)
                if tr is not None:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record(copy_stream)
                    tr.append(("copy1", e))
                d64 = stage64[m0:m1].to(dev, non_blocking=True), stage64[cap + m0:cap + m1].to(dev, non_blocking=True)
                d32 = stage32[m0:m1].to(dev, non_blocking=True), stage32[cap + m0:cap + m1].to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            kernels()                                                    # the batch before this one
            pending.append((k, d64, d32, ev, tr, time.perf_counter() - t_start, b_byte - a_byte))
            m0 = m1
        try:
            t_wait = t_launch = 0.0
            for fut in futures:
                tw = time.perf_counter()
                avail = fut.result()
                t_wait += time.perf_counter() - tw
                while True:
                    try:
                        new, _, _, nxt = bgzf.scan_members(data[:avail], scan_pos, (coff, clen, isize), n_mem)   # straight into the page-locked arrays
                    except bgzf.ScanError as e:
                        raise _lib.NanoCallerHipError("%s is not a BGZF file (nc_bgzf_scan: %d at byte %d)" % (self.path, e.rc, scan_pos))
                    k = int(new.size)
                    if k:
                        ooff[n_mem] = total
                        if k > 1:
                            np.cumsum(isize[n_mem:n_mem + k - 1], out=ooff[n_mem + 1:n_mem + k])
                            ooff[n_mem + 1:n_mem + k] += total
                        total = int(ooff[n_mem + k - 1]) + int(isize[n_mem + k - 1])
                    n_mem += k
                    scan_pos = nxt
                    if n_mem < cap or scan_pos >= avail:
                        break
                    raise DeviceIngestUnavailable("%s: more BGZF members than planned for" % self.path)
                if total + 64 > raw_cap:
                    raise DeviceIngestUnavailable("%s inflates more than eight-fold" % self.path)
                tw = time.perf_counter()
                while n_mem - m0 >= batch:
                    launch(m0 + batch)
                t_launch += time.perf_counter() - tw
            if scan_pos != n and self.B1 == self.file_bytes:
                raise _lib.NanoCallerHipError("%s does not end with a whole BGZF member" % self.path)
            while n_mem > m0:
                launch(min(n_mem, m0 + batch))
            kernels()
        finally:
            pool.shutdown(wait=True)
            os.close(fd)
        LAST_LOAD.clear()
        LAST_LOAD["read_scan_enqueue"] = time.perf_counter() - t_start
        LAST_LOAD["of_which_page_locked_alloc"] = t_pin
        LAST_LOAD["of_which_allocations"], LAST_LOAD["of_which_waiting_for_readers"], LAST_LOAD["of_which_enqueue"] = t_alloc, t_wait, t_launch
        t0 = time.perf_counter()
        self.coff, self.clen, self.isize = coff[:n_mem].copy(), clen[:n_mem].copy(), isize[:n_mem].copy()
        self.mstart, self.ooff = bgzf.member_table(self.coff, self.clen, self.isize)   # file offset / inflated offset of every member (+ the total)
        lz_stream.synchronize()
        err = bgzf.bad_members_error(self.path, statuses)                # (also: the inflate is done)
        if err:
            raise err
        compute.wait_stream(lz_stream)
        if traces:
            e0 = traces[0][3][0][1]
            for t_host, k_, nb_, tr_ in traces:
                print("  batch of %d members, %.0f MB, enqueued at %.1f ms: " % (k_, nb_ / 1e6, t_host * 1e3) + ", ".join("%s %.1f" % (w, e0.elapsed_time(e)) for w, e in tr_), flush=True)
        del toks, d_file, keep, statuses
        self.host_buf = None
        LAST_LOAD["inflate_wait"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        self.n_rec = 0
        self.meta = np.zeros((META_COLS, 0), np.int32)
        self.rec_off = np.zeros(0, np.int64)
        seeds, tids = [], []
        # chain starts: the linear index entries of every contig
        for tid in (sorted(self.lin) if self.tids is None else self.tids):
            v = self.lin.get(tid, np.zeros(0, np.uint64))
            if v.size:
                seeds.append(self.voffset_to_stream(v))
                tids.append(np.full(v.size, tid, np.int32))
        if seeds:
            seed, tid = np.concatenate(seeds), np.concatenate(tids)
            if np.any(np.diff(seed) <= 0):
                raise _lib.NanoCallerHipError("%s: the index entries are not in file order" % self.path)
            d_seed, d_tid = torch.from_numpy(seed).to(dev), torch.from_numpy(tid).to(dev)
            d_cnt = torch.zeros(seed.size, dtype=torch.int64, device=dev)
            d_status = torch.zeros(1, dtype=torch.int32, device=dev)
            eng._check(L.nc_bam_walk(eng.ctx, vp(self.raw), total, seed.size, vp(d_seed), vp(d_tid), None, vp(d_cnt), vp(d_status)), "nc_bam_walk")
            d_first = torch.cumsum(d_cnt, 0) - d_cnt
            self.n_rec = int(d_cnt.sum().item())
            self.d_rec_off = torch.empty(max(1, self.n_rec), dtype=torch.int64, device=dev)
            eng._check(L.nc_bam_walk(eng.ctx, vp(self.raw), total, seed.size, vp(d_seed), vp(d_tid), vp(d_first), vp(self.d_rec_off), vp(d_status)), "nc_bam_walk")
            d_meta = torch.empty((META_COLS, max(1, self.n_rec)), dtype=torch.int32, device=dev)
            eng._check(L.nc_bam_meta(eng.ctx, vp(self.raw), self.n_rec, vp(self.d_rec_off), vp(d_meta), vp(d_status)), "nc_bam_meta")
            self.meta = d_meta.cpu().numpy()[:, :self.n_rec]
            self.rec_off = self.d_rec_off.cpu().numpy()[:self.n_rec]
            st = int(d_status.item())
            if st:
                raise _lib.NanoCallerHipError("%s: corrupt BAM records or index (status %d)" % (self.path, st))
        # the records of a contig are one run of the record list (coordinate-sorted file)
        refid = self.meta[M_REFID]
        self.tid_range = {}
        if self.n_rec:
            cut = np.flatnonzero(np.diff(refid)) + 1
            lo = np.concatenate([[0], cut])
            hi = np.concatenate([cut, [self.n_rec]])
            for a, b in zip(lo.tolist(), hi.tolist()):
                t = int(refid[a])
                if t in self.tid_range:
                    raise _lib.NanoCallerHipError("%s is not coordinate-sorted (contig %d appears twice)" % (self.path, t))
                self.tid_range[t] = (a, b)
        LAST_LOAD["walk_meta"] = time.perf_counter() - t0
        LAST_LOAD["members"], LAST_LOAD["records"], LAST_LOAD["inflated_bytes"] = n_mem, self.n_rec, total
        self.raw_len = total
        self.loaded = True
        return self

    def fetch_names(self, recs):
        """read names of the records `recs` (indices into the record list): a D2H of a few bytes each (the duplicate-name check's slow path)"""
        out = []
        for r in np.asarray(recs).tolist():
            o = int(self.rec_off[r])
            head = self.raw[o + 4:o + 4 + 32].cpu().numpy()
            l_name = int(head[8])
            out.append(self.raw[o + 36:o + 36 + l_name - 1].cpu().numpy().tobytes().decode("ascii", "replace"))
        return out

    # ------------------------------------------------------------------ one contig: the host's decisions
    def prepare(self, chrom, ref, supplementary=False, exclude=None, span=None, tile_size=2048, haplotags=None, by_name=False):
        """host half (numpy + native, no GPU call: may run on a worker thread).  ref: the contig's sequence (str / bytes), or a
        device_fasta.DeviceContig: then no letters are staged and pack() takes the scan's reference codes from it.  haplotags: path of a haplotag
        table (phase.save_haplotags) whose HP / PS replace the records' own tags, by read-name hash.  -> dict for pack()
        by_name (the SNP route): kept alignments that share a read name are not refused but keyed by name as the host route keys them
        (pack.name_groups -> mate_table: bit 3 and the name's strand in the tile entries, `mates` in the result).  When, and only when, name
        hashes repeat among the kept alignments, THIS call then touches the GPU: one nc_bam_name_groups launch on the context's own stream and
        one copy of 4 bytes per candidate back, both waited for here.  It stays safe on a worker thread -- the launch stream and the
        context's state are left alone -- but it is no longer host work only."""
        if not self.loaded:
            raise RuntimeError("DeviceBam.load() first")
        if chrom not in self.ref_names:
            raise ValueError("%s has no contig %r" % (self.path, chrom))
        tid = self.ref_names.index(chrom)
        length = self.ref_lengths[tid]
        beg1, end1 = (1, length) if span is None else (max(1, int(span[0])), int(span[1]))
        a, b = self.tid_range.get(tid, (0, 0))
        m = self.meta[:, a:b]
        pos, rlen, flag = m[M_POS], m[M_RLEN], m[M_FLAG]
        # the alignments nc_bam_decode(tid, beg1, end1) returns
        sel = (pos < end1) & ((flag & 0x4) == 0) & (rlen > 0) & (pos.astype(np.int64) + rlen > beg1 - 1)
        idx = np.flatnonzero(sel)
        start = (pos[idx] + 1).astype(np.int32)
        end = (start + rlen[idx]).astype(np.int32)
        flag = flag[idx]
        # inputs the library does not reproduce (generate_SNP_pileups._check_supported)
        mask = 0x704 if supplementary else 0xF04
        kept_for_check = (flag & mask) == 0
        n_skip = int(np.count_nonzero(kept_for_check & ((flag & _lib.FLAG_REFSKIP) != 0)))
        h = (m[M_HASH_LO][idx].astype(np.uint32).astype(np.uint64) | (m[M_HASH_HI][idx].astype(np.uint32).astype(np.uint64) << np.uint64(32)))
        n_dup = 0 if by_name else self._same_name_overlaps(h, start, end, kept_for_check, a + idx, any_pair=bool(supplementary))
        if n_skip or n_dup:
            what = []
            if n_skip:
                what.append("%d alignments with a reference skip (CIGAR N) would enter the pileup; the reference's code table has no entry for "
                            "their '>' / '<' symbols (generate_SNP_pileups.py:104)" % n_skip)
            if n_dup:
                what.append("%d pairs of kept alignments carry the same read name%s; the reference's per-column dicts hold one entry per name "
                            "(generate_SNP_pileups.py:175,185,208): the host route (NC_DEVICE_INGEST=0) keys them by name" % (n_dup, "" if supplementary else " and overlap on the reference"))
            raise _lib.NanoCallerHipError("%s, contig %s: %s -- NC_ERR_UNSUPPORTED" % (self.path, chrom, "; ".join(what)), status=_lib.NC_ERR_UNSUPPORTED)
        filt = FLAG_FILTER_SUPPL if supplementary else FLAG_FILTER_DEFAULT
        keep = pileup_depth_cap(start, end, np.ascontiguousarray((flag & filt) == 0, np.uint8))
        if haplotags:
            from .phase import tags_for_hashes
            hap, ps = tags_for_hashes(h, haplotags)
        else:
            hap, ps = m[M_HAP][idx].astype(np.uint8), m[M_PS][idx]
        strand = np.ascontiguousarray(((flag & 0x10) != 0).astype(np.uint8) | ((hap & 3) << 1))
        mates = None
        if by_name:
            # every kept alignment whose name occurs more than once, overlapping or not, under both filters: what the host route does
            gid = self._name_gid(h, (flag & filt) == 0, a + idx)
            nxt, gstrand = name_groups(None, flag, keep, gid=gid) if gid is not None else (None, None)
            if nxt is not None:
                strand = np.ascontiguousarray(gstrand | ((nxt >= 0).astype(np.uint8) << 3) | ((hap & 3) << 1))   # (as pack.pack_reads builds it)
                mates = mate_table(nxt, keep, start, end)
        # tile index + slot layout (nc_pack_plan / nc_pack_fill, index only: what wire.build_wire does)
        L = _lib.lib()
        ref_contig = ref if hasattr(ref, "scan_codes") else None        # a device_fasta.DeviceContig: the letters are in HBM already
        ref_bytes = np.zeros(0, np.uint8) if ref_contig is not None else np.frombuffer(ref.encode("ascii") if isinstance(ref, str) else ref, np.uint8)
        Lref = int(ref_contig.length) if ref_contig is not None else int(ref_bytes.shape[0])
        pos_lo = 1 if span is None else max(1, int(span[0]))
        pos_hi = max(pos_lo, Lref if span is None else min(Lref, int(span[1])))
        codes_len, n_ent = C.c_int64(), C.c_int64()
        tile_pos0, n_tiles = C.c_int32(), C.c_int32()
        n = int(idx.size)
        rc = L.nc_pack_plan(n, _lib.npp(start), _lib.npp(end), _lib.npp(keep), tile_size, pos_lo, pos_hi, C.byref(codes_len), C.byref(tile_pos0),
                            C.byref(n_tiles), C.byref(n_ent))
        if rc != _lib.NC_OK:
            raise _lib.NanoCallerHipError("nc_pack_plan failed (%d)" % rc)
        tile_off = np.empty(n_tiles.value + 1, np.int32)
        tile_ent = np.empty(max(1, n_ent.value), _lib.TILE_ENTRY_DTYPE)
        rc = L.nc_pack_fill(n, _lib.npp(start), _lib.npp(end), None, None, _lib.npp(strand), _lib.npp(keep), tile_size, tile_pos0.value,
                            n_tiles.value, None, codes_len.value, _lib.npp(tile_off), _lib.npp(tile_ent), n_ent.value)
        if rc != _lib.NC_OK:
            raise _lib.NanoCallerHipError("nc_pack_fill (index) failed (%d)" % rc)
        kk = np.flatnonzero(keep)
        ks, ke = start[kk], end[kk]
        size = ((ke.astype(np.int64) + 15) & ~15) - (ks.astype(np.int64) & ~15)
        slot = np.zeros(kk.size, np.int64)
        if kk.size:
            np.cumsum(size[:-1], out=slot[1:])
        mk = m[:, idx[kk]]
        ncig = mk[M_NCIG].astype(np.int64) | np.where(mk[M_HASSEQ] != 0, 0, 1 << 31)
        # everything the device half uploads, back to back in ONE page-locked buffer (a pageable source makes the copy wait for the GPU to
        # finish what is queued before it -- the previous contig's CNN -- and the launching thread with it)
        ga, gb = max(1, tile_pos0.value), min(Lref, tile_pos0.value + n_tiles.value * tile_size - 1)
        parts = dict(rec=np.ascontiguousarray(self.rec_off[a + idx[kk]]), slot=slot, cigd=np.ascontiguousarray(mk[M_CIGD]),
                     ncig=ncig.astype(np.uint32).view(np.int32), start=np.ascontiguousarray(ks), rd_end=np.ascontiguousarray(ke),
                     slot_off=np.concatenate([slot, [int(size.sum())]]).astype(np.int64), read_hap=np.ascontiguousarray(hap[kk]),
                     read_ps=np.ascontiguousarray(ps[kk], np.int32), read_flag=np.ascontiguousarray((mk[M_LSEQ] == 0).astype(np.uint8)), tile_off=tile_off,
                     tile_ent=tile_ent.view(np.uint8).reshape(-1), ref_letters=ref_bytes[ga - 1:gb] if gb >= ga and ref_contig is None else ref_bytes[:0])
        if mates is not None:
            parts.update(mate_key=mates[0], mate_rec=np.ascontiguousarray(mates[1]).reshape(-1))
        sections, total_b = {}, 0
        for k, v in parts.items():
            sections[k] = (total_b, v.dtype, int(v.size))
            total_b += (v.nbytes + 255) & ~255
        staged = torch.empty(max(256, total_b), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        host = staged.numpy()
        for k, v in parts.items():
            o = sections[k][0]
            host[o:o + v.nbytes] = v.view(np.uint8).reshape(-1)
        return dict(chrom=chrom, n_kept=int(kk.size), staged=staged, sections=sections, ref_span=(ga, gb), ref_contig=ref_contig, exclude=list(exclude or ()),
                    codes_len=int(codes_len.value), tile_size=tile_size,
                    tile_pos0=int(tile_pos0.value), n_tiles=int(n_tiles.value), n_entries=int(n_ent.value), pos_lo=pos_lo, pos_hi=pos_hi,
                    n_reads=n, read_start=start, read_end=end, read_flag=flag, keep=keep, mates=mates)

    def _name_gid(self, h, keep, recs):
        """nc_decoded_name_groups' answer from the record stream: per alignment the first kept alignment (file order) of its read name when
        another kept one carries it, else -1; None when no name hash repeats among the kept alignments (no launch).  The candidates -- kept
        alignments whose hash occurs more than once -- go to nc_bam_name_groups sorted by (hash, file order); the names themselves are
        compared there, so two names with one hash stay apart."""
        k = np.flatnonzero(keep)
        if k.size < 2:
            return None
        _, inv, cnt = np.unique(h[k], return_inverse=True, return_counts=True)
        cand = k[cnt[inv] > 1]
        if cand.size == 0:
            return None
        cand = cand[np.argsort(h[cand], kind="stable")]
        dev = self.eng.device
        d_gid = torch.empty(cand.size, dtype=torch.int32, device=dev)
        d_status = torch.empty(1, dtype=torch.int32, device=dev)
        d_off = torch.from_numpy(np.ascontiguousarray(self.rec_off[recs[cand]])).to(dev)      # (blocking copies: complete when the call is made)
        d_hash = torch.from_numpy(h[cand].view(np.int64)).to(dev)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        rc = _lib.lib().nc_bam_name_groups(self.eng.ctx, vp(self.raw), self.raw_len, int(cand.size), vp(d_off), vp(d_hash), vp(d_gid), vp(d_status))
        if rc != _lib.NC_OK:
            raise _lib.NanoCallerHipError("%s: nc_bam_name_groups failed (%d)%s" % (self.path, rc, ": corrupt BAM records" if rc == _lib.NC_ERR_ARG else ""))
        g = d_gid.cpu().numpy()
        gid = np.full(h.size, -1, np.int32)
        m = g >= 0
        gid[cand[m]] = cand[g[m]]
        return gid

    def _same_name_overlaps(self, h, start, end, keep, recs, any_pair=False):
        """bam.same_name_overlaps on name hashes; hash-equal pairs are confirmed on the names themselves.  any_pair: count every pair of kept
        alignments that share a name, overlapping or not (under dct['supplementary'] the reference looks neighbour columns up by NAME: the host
        route keys such records by name, pack.name_groups; this route does not)"""
        k = np.flatnonzero(keep)
        if k.size < 2:
            return 0
        hk = h[k]
        u, inv, cnt = np.unique(hk, return_inverse=True, return_counts=True)
        cand = k[cnt[inv] > 1]                                            # kept alignments whose name (hash) occurs more than once
        if cand.size == 0:
            return 0
        names = self.fetch_names(recs[cand])
        last, n = {}, 0
        for r, nm in zip(cand.tolist(), names):
            e = last.get(nm)
            if e is not None and (any_pair or int(start[r]) < e):
                n += 1
            last[nm] = max(int(end[r]), e or 0)
        return n

    def _ref_lut(self):
        if getattr(self, "_lut", None) is None:
            lut = np.full(256, 4, np.uint8)                              # upper-case AGTC are scanned; soft-masked / other letters are not (quirk E4)
            for i, ch in enumerate("AGTC"):
                lut[ord(ch)] = i
            self._lut = torch.from_numpy(lut).to(self.eng.device)
        return self._lut

    # ------------------------------------------------------------------ one contig: the slots, in HBM
    def pack(self, prep, codes=None, indel=False, tail_cap=272) -> DevicePack:
        """device half: uploads the (small) arrays of prepare() and decodes the kept reads into `codes` (allocated when None).  indel=True: the
        pack also carries the indel path's sections (events, inserted bases, tails: what wire.build_wire(events=..., indel_extra=...) uploads on
        the host route), made from the record stream by nc_bam_indel_reads"""
        eng, L, dev = self.eng, _lib.lib(), self.eng.device
        eng.use_torch_stream()
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        dbuf = prep["staged"].to(dev, non_blocking=True)
        tdt = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}

        def sec(k):
            o, dt, cnt = prep["sections"][k]
            return dbuf[o:o + cnt * np.dtype(dt).itemsize].view(tdt[np.dtype(dt)])
        n = prep["codes_len"]
        if codes is None:
            codes = torch.empty(n, dtype=torch.uint8, device=dev)
        codes = codes[:n]
        codes.fill_(7)                                                   # NC_CODE_ABSENT
        if prep["n_kept"]:
            eng._check(L.nc_bam_codes(eng.ctx, vp(self.raw), prep["n_kept"], vp(sec("rec")), vp(sec("slot")), vp(sec("cigd")), vp(sec("ncig")), vp(sec("start")),
                                      vp(codes)), "nc_bam_codes")
        # the scan's reference codes on the tile grid, from the contig's letters (wire.ref_wire_from_string + nc_wire_expand's rule, in HBM: the
        # 9 MB table passes of a contig kept a worker thread -- and the interpreter lock the launching thread needs -- busy for milliseconds)
        ref_len, t0 = prep["n_tiles"] * prep["tile_size"], prep["tile_pos0"]
        ga, gb = prep["ref_span"]
        if prep.get("ref_contig") is not None:                           # the same codes straight from the FASTA image in HBM (nc_fasta_decode)
            try:
                ref_code = prep["ref_contig"].scan_codes(t0, ref_len, ga, gb)
            except DeviceIngestUnavailable:                              # no room for the image: the host reader's letters, as below
                from .bam import read_fasta_bytes
                letters = np.frombuffer(read_fasta_bytes(prep["ref_contig"].owner.path, prep["chrom"]), np.uint8)[max(0, ga - 1):max(0, gb)]
                ref_code = torch.full((ref_len,), 4, dtype=torch.uint8, device=dev)
                if gb >= ga:
                    ref_code[ga - t0:gb - t0 + 1] = self._ref_lut()[torch.from_numpy(letters.copy()).to(dev).to(torch.int32)]
        else:
            ref_code = torch.full((ref_len,), 4, dtype=torch.uint8, device=dev)
            if gb >= ga:
                ref_code[ga - t0:gb - t0 + 1] = self._ref_lut()[sec("ref_letters").to(torch.int32)]
        for (a, b) in prep["exclude"]:                                   # tree.overlaps(pos): a <= pos < b (generate_SNP_pileups.py:116-119,161)
            lo, hi = max(1, int(a)) - t0, max(1, int(b)) - t0
            if hi > max(lo, 0):
                ref_code[max(lo, 0):min(hi, ref_len)] = 4
        dp = DevicePack(codes=codes, tile_off=sec("tile_off"), tile_ent=sec("tile_ent"), ref_code=ref_code, tile_size=prep["tile_size"],
                        tile_pos0=prep["tile_pos0"], n_tiles=prep["n_tiles"], n_entries=prep["n_entries"], pos_lo=prep["pos_lo"], pos_hi=prep["pos_hi"])
        dp.records = (self, sec("rec"))
        if prep.get("mates") is not None:                                # prepare(by_name=True): the featuriser's table of the shared names (nc_snp_set_mates)
            dp.mates = (sec("mate_key"), sec("mate_rec").view(-1, 4))
        if indel:
            K = prep["n_kept"]
            i32 = lambda n_: torch.zeros(max(int(n_), 4), dtype=torch.int32, device=dev)   # noqa: E731
            u8 = lambda n_: torch.zeros(max(int(n_), 4), dtype=torch.uint8, device=dev)    # noqa: E731
            counts = torch.zeros((3, max(K, 1)), dtype=torch.int32, device=dev)
            args = (vp(self.raw), K, vp(sec("rec")), vp(sec("cigd")), vp(sec("ncig")), int(tail_cap))
            eng._check(L.nc_bam_indel_reads(eng.ctx, *args, vp(counts), None, None, None, None, None, None, None, None), "nc_bam_indel_reads")
            offs = torch.zeros((3, K + 1), dtype=torch.int64, device=dev)
            if K:
                torch.cumsum(counts[:, :K], 1, out=offs[:, 1:])
            n_ev, n_ins, n_tail = (int(x) for x in offs[:, K].tolist())
            if max(n_ev, n_ins, n_tail) > 2**31 - 2:
                raise _lib.NanoCallerHipError("more than 2^31 indel events / inserted bases in one contig")
            o32 = offs.to(torch.int32)
            ev_pos, ev_len, ins_off, ins_bases, tail_bases = i32(n_ev), i32(n_ev), i32(n_ev + 1), u8(n_ins), u8(n_tail)
            if K:
                eng._check(L.nc_bam_indel_reads(eng.ctx, *args, None, vp(o32[0]), vp(o32[1]), vp(o32[2]), vp(ev_pos), vp(ev_len), vp(ins_off), vp(ins_bases),
                                                vp(tail_bases)), "nc_bam_indel_reads")
            ins_off[n_ev] = n_ins
            z = lambda t: t if t.numel() else torch.zeros(4, dtype=t.dtype, device=dev)   # noqa: E731
            dp.events = dict(n_reads=K, ev_off=o32[0].contiguous(), ev_pos=ev_pos[:max(n_ev, 1)], ev_len=ev_len[:max(n_ev, 1)], read_hap=z(sec("read_hap")))
            dp.reads = dict(n_reads=K, rd_start=z(sec("start")), rd_end=z(sec("rd_end")), slot_off=sec("slot_off"))
            dp.indel = dict(ins_off=ins_off[:n_ev + 1], ins_bases=ins_bases, tail_off=o32[2].contiguous(), tail_bases=tail_bases, read_ps=z(sec("read_ps")),
                            read_flag=z(sec("read_flag")))
        return dp


def contig_spans(path):
    """{contig: (lo, hi)} = the bytes of the BAM file that hold its records, from the .bai alone: the member of its first record to the member of
    the next contig's first record (inclusive: a record straddles members); contigs without alignments are absent.  Raises
    DeviceIngestUnavailable when there is no .bai."""
    bai = _bai_path(path)
    if bai is None:
        raise DeviceIngestUnavailable("%s: no .bai / .csi beside it" % path)
    lin, file_bytes = bai_linear_voffsets(bai), os.path.getsize(path)
    names = bgzf.bam_header(path)[1]
    with_reads = [t for t in sorted(lin) if lin[t].size and t < len(names)]
    out = {}
    for k, t in enumerate(with_reads):
        hi = min(file_bytes, int(lin[with_reads[k + 1]][0] >> np.uint64(16)) + 65536 + 1024) if k + 1 < len(with_reads) else file_bytes
        out[names[t]] = (int(lin[t][0] >> np.uint64(16)), hi)
    return out, names


def plan_shares(path, contigs, limit_bytes=None, device=None):
    """`contigs` (in the order they will be called) cut into runs whose part of the file -- first record of the run's first contig to the first
    record behind its last -- stays under `limit_bytes` of compressed BAM (default: what DeviceBam accepts), so that a genome-sized file
    passes through HBM share by share.  -> list of (contigs of the share, fits): fits False = that contig alone is too large (host route).
    Raises DeviceIngestUnavailable when there is no .bai."""
    spans, names = contig_spans(path)
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    limit = (resident_limit(device) // 8) if limit_bytes is None else int(limit_bytes)
    shares, cur, lo, hi = [], [], None, None
    for c in contigs:
        if c not in names:
            raise ValueError("%s has no contig %r" % (path, c))
        sp = spans.get(c)
        if sp is None:                                                   # no alignments: rides along
            cur.append(c)
            continue
        if sp[1] - sp[0] > limit:
            if cur:
                shares.append((cur, True))
            shares.append(([c], False))
            cur, lo, hi = [], None, None
            continue
        nlo, nhi = (sp[0], sp[1]) if lo is None else (min(lo, sp[0]), max(hi, sp[1]))
        if cur and lo is not None and nhi - nlo > limit:
            shares.append((cur, True))
            cur, nlo, nhi = [], sp[0], sp[1]
        cur.append(c)
        lo, hi = nlo, nhi
    if cur:
        shares.append((cur, True))
    return shares


def build_index(path, fmt=None, device=0, piece_bytes=None):
    """Index the coordinate-sorted BAM `path` on the GPU and write <path>.bai (fmt='csi', or a reference longer than 2^29: <path>.csi) beside
    it -> the index's path.  The file streams through HBM in pieces of whole BGZF members (`piece_bytes` of compressed bytes each), so its size
    does not matter; an unsorted or corrupt file raises NanoCallerHipError (bam_index.py)."""
    from .bam_index import build_index as _build
    return _build(path, fmt=fmt, device=device, piece_bytes=piece_bytes)


def build_index_selected(params=None) -> bool:
    """params['build_index'] truthy; without that key, the environment's NC_BUILD_INDEX == '1': a BAM without index is indexed once
    (build_index) instead of taking the host route"""
    if params is not None and "build_index" in params:
        return bool(params["build_index"])
    return os.environ.get("NC_BUILD_INDEX") == "1"


def ensure_index(path, params=None, device=0, collective=False):
    """the opt-in of the callers: a BAM file without index gets one when build_index_selected(params).  collective: every rank of a
    torch.distributed run calls this at the same point -- rank 0 builds, the others wait at shard.barrier().  Without the opt-in, or for
    an input that is no file, nothing happens."""
    if not (isinstance(path, str) and os.path.exists(path)) or not build_index_selected(params):
        return None
    rank0 = True
    if collective:
        import torch.distributed as dist
        rank0 = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
    try:
        if _bai_path(path) is None and rank0:
            build_index(path, device=device)
    finally:
        if collective:
            from . import shard
            shard.barrier()
    return _bai_path(path)


_OPEN = {}
_RAW_POOL = {}               # device index -> (buffer of the inflated stream, weak reference to the DeviceBam that is using it)
_WORK_POOL = {}              # (device index, name) -> the loader's work buffers (file image in HBM, token workspaces), kept from load to load


def _work_buffer(dev, name, numel, dtype):
    """a buffer of the loader that lives only during load(): the same allocation every time (grown when a larger file comes).  Handing
    these back to the framework's allocator let it cut them up for other requests in between; the next load then had to get ~9 GB of fresh
    device memory, which was measured at 240 ms"""
    t = _WORK_POOL.get((dev.index, name))
    if t is None or t.numel() < numel or t.dtype != dtype:
        _WORK_POOL.pop((dev.index, name), None)
        t = torch.empty(numel, dtype=dtype, device=dev)
        if numel * t.element_size() <= POOL_MAX:
            _WORK_POOL[(dev.index, name)] = t
    return t[:numel]


def open_device_bam(path, device=0, contigs=None) -> DeviceBam:
    """the loaded DeviceBam of (path, device) holding at least `contigs` (None: the whole file), cached by path + size + mtime"""
    st = os.stat(path)
    want = None if contigs is None else frozenset(contigs)
    ident = (os.path.abspath(path), st.st_size, st.st_mtime_ns, device)
    for k, db in list(_OPEN.items()):
        if k[:4] == ident and (k[4] is None or (want is not None and want <= k[4])):
            return db.load()
        if k[0] == ident[0] and k[3] == device:
            del _OPEN[k]                                                # another version of the file, or another share of it
    db = _OPEN[ident + (want,)] = DeviceBam(path, device, contigs=None if want is None else sorted(want))
    try:
        return db.load()
    except (torch.cuda.OutOfMemoryError, MemoryError) as e:             # device or page-locked memory: the host route needs neither
        _OPEN.pop(ident + (want,), None)
        release(path, buffers=True)
        raise DeviceIngestUnavailable("%s: %s" % (path, str(e).splitlines()[0] if str(e) else type(e).__name__))
    except RuntimeError as e:
        if "out of memory" in str(e).lower() or "hipErrorOutOfMemory" in str(e):
            _OPEN.pop(ident + (want,), None)
            release(path, buffers=True)
            raise DeviceIngestUnavailable("%s: %s" % (path, str(e).splitlines()[0]))
        raise


def release(path=None, buffers=False):
    """forget the loaded files (of `path`, or all); buffers=True also gives the pooled stream buffers back"""
    for k in [k for k in _OPEN if path is None or k[0] == os.path.abspath(path)]:
        del _OPEN[k]
    if buffers:
        _RAW_POOL.clear()
        _WORK_POOL.clear()
        from . import device_fasta
        device_fasta.release()                                           # the FASTA images and contigs kept in HBM go with the other pools

"""Device engine: drives libnanocaller_hip.so from Python.

PyTorch is used only as plumbing -- device memory (tensors), the current HIP stream and, for multi-GPU
runs, torch.distributed rendezvous.  All arithmetic of the hot path runs in the library's HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .pack import HostPack
from .weights import Weights


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def sample_thresholds(keep):
    """probabilities in [0, 1) -> the uint32 thresholds of nc_snp_scan_set_sampling: a column is kept when its 32-bit hash is below
    floor(keep * 2^32), that is with probability floor(keep * 2^32) / 2^32 over the hash values"""
    return np.floor(np.asarray(keep, np.float64) * 4294967296.0).astype(np.uint32)


@dataclass
class DevicePack:
    codes: torch.Tensor
    tile_off: torch.Tensor
    tile_ent: torch.Tensor      # uint8 view of the 16-byte entries
    ref_code: torch.Tensor
    tile_size: int
    tile_pos0: int
    n_tiles: int
    n_entries: int
    pos_lo: int
    pos_hi: int
    events: dict | None = None    # device tensors ev_off / ev_pos / ev_len / read_hap (indel scan inputs)
    reads: dict | None = None     # device tensors rd_start / rd_end / slot_off of the kept reads (device pass 2: tile entry -> read)
    indel: dict | None = None     # device tensors ins_off / ins_bases / tail_off / tail_bases / read_ps / read_flag (device pass 2)
    mates: tuple | None = None    # (key int64 [M], rec int32 [M, 4]) device tensors: alignments that share read names (nc_snp_set_mates)
    records: tuple | None = None  # (DeviceBam, int64 device tensor): a pack the device ingest made -- the owner of the inflated record stream and
                                  # the kept reads' record offsets in it, in pack order (the weighted phaser reads MAPQ and qualities there)

    def c_struct(self) -> _lib.ReadPackC:
        return _lib.ReadPackC(codes_len=self.codes.numel(), codes=self.codes.data_ptr(), tile_size=self.tile_size,
                              tile_pos0=self.tile_pos0, n_tiles=self.n_tiles, tile_off=self.tile_off.data_ptr(),
                              tile_ent=self.tile_ent.data_ptr(), n_entries=self.n_entries)

    @property
    def nbytes(self):
        return self.codes.numel() + self.tile_off.numel() * 4 + self.tile_ent.numel() + self.ref_code.numel()


@dataclass
class SnpSites:
    """Results of scan + featurize for a batch of chunks (device tensors unless noted)."""
    n_sites: int
    n_nbr: int
    pos: np.ndarray            # host int32 [N]
    chunk: np.ndarray          # host int32 [N]
    dp: np.ndarray             # host int32 [N]   pileup entries incl. deletions
    alt: np.ndarray            # host int32 [N]   max non-reference base count
    x: torch.Tensor | None = None          # f32 [N,5,41,5]
    ref_code: torch.Tensor | None = None   # i32 [N]
    fwd_dp: torch.Tensor | None = None     # i32 [N,4]
    rev_dp: torch.Tensor | None = None
    depth: torch.Tensor | None = None      # i32 [N]
    valid: torch.Tensor | None = None      # u8 [N]
    nbr_only: bool = False                 # the scan took its neighbours from a list alone: the featuriser's min_nbr_sites counts them, not the site


class _PinnedPool:
    """Page-locked host blocks for result arrays.  hipHostMalloc costs milliseconds, so blocks are reused -- but only
    when no numpy view handed out from a block is alive any more (tracked with a weak reference), so results of
    earlier calls stay valid for as long as the caller keeps them."""

    def __init__(self):
        self.blocks = []                                  # [uint8 pinned tensor, weakref to the numpy array handed out]

    def get(self, shape, dtype):
        """-> (torch tensor view, numpy array) over the same pinned memory"""
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        best = None
        for b in self.blocks:
            if (b[1] is None or b[1]() is None) and b[0].numel() >= nbytes and (best is None or b[0].numel() < best[0].numel()):
                best = b
        if best is None:
            cap = max(4096, nbytes + nbytes // 4)
            best = [torch.empty(cap, dtype=torch.uint8, pin_memory=True), None]
            self.blocks.append(best)
        t = best[0][:nbytes].view(dtype).view(shape)
        arr = t.numpy()
        best[1] = weakref.ref(arr)
        return t, arr


class Engine:
    """One engine per GPU (one process per GPU in multi-GPU runs).  Not thread-safe."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise _lib.NanoCallerHipError("no ROCm device visible: the NanoCaller HIP path has no CPU fallback")
        self.L = _lib.lib()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        rc = self.L.nc_ctx_create(device, C.byref(ctx))
        if rc != _lib.NC_OK:
            raise _lib.NanoCallerHipError("nc_ctx_create(device=%d) failed with status %d" % (device, rc))
        self.ctx = ctx
        self._loaded = {}
        self._pinned = _PinnedPool()
        self.x_int16 = self.exact_fp32 = False              # the library's defaults (set_tensor_format / set_cnn_precision)
        self.use_torch_stream()

    def close(self):
        if getattr(self, "ctx", None):
            self.L.nc_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != _lib.NC_OK:
            msg = self.L.nc_last_error(self.ctx)
            raise _lib.NanoCallerHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""), status=rc)

    def use_torch_stream(self):
        """The library's kernels go to torch's current stream of this thread.  Where that is the legacy default stream, the thread is first moved to
        this engine's own torch stream: torch's kernels (fills, reductions, copies) and the library's then share ONE hardware queue.  On the default
        stream the library used a stream of its own beside it, and every torch kernel in a pass cost two cross-queue hand-overs (~0.4 ms of idle GPU
        per 11 ms contig pass: bench.py 56.0 -> 58.2 M sites/s; `rocprofv3 --kernel-trace` timelines by tools/one_pass.py).  Work the caller has
        already enqueued on the default stream is waited for.  NC_ONE_QUEUE=0: the old arrangement."""
        s = torch.cuda.current_stream(self.device)
        if s.cuda_stream == 0 and os.environ.get("NC_ONE_QUEUE", "1") != "0":
            if getattr(self, "_tstream", None) is None:
                self._tstream = torch.cuda.Stream(device=self.device)
            self._tstream.wait_stream(s)
            torch.cuda.set_stream(self._tstream)
            s = self._tstream
        self._check(self.L.nc_ctx_set_stream(self.ctx, C.c_void_p(s.cuda_stream)), "nc_ctx_set_stream")

    def _adopt_thread(self):
        """get_engine() from a thread that meets this engine for the first time: a thread on the legacy default stream is moved to the engine's own torch
        stream (one hardware queue); the CONTEXT's launch stream is left alone (get_engine used to call use_torch_stream(), which rewrites
        the shared ctx->stream -- a worker thread could retarget another thread's launches between its `with torch.cuda.stream(...)` and its kernel).
        Only an explicit use_torch_stream() retargets the context."""
        s = torch.cuda.current_stream(self.device)
        if s.cuda_stream == 0 and os.environ.get("NC_ONE_QUEUE", "1") != "0" and getattr(self, "_tstream", None) is not None:
            self._tstream.wait_stream(s)
            torch.cuda.set_stream(self._tstream)

    def set_cnn_precision(self, exact_fp32: bool):
        """False (default): fp16x3 split-precision trunk; True: exact fp32 MFMA trunk."""
        self._check(self.L.nc_set_cnn_precision(self.ctx, 1 if exact_fp32 else 0), "nc_set_cnn_precision")
        self.exact_fp32 = bool(exact_fp32)

    def set_tensor_format(self, int16: bool):
        """The engine's default tensor format: what snp_featurize(int16=None) writes and what trunk_info() reports for -- int16 (exact: every
        entry is a small integer; half the bytes) instead of the reference's float32.  snp_forward does not read it: a tensor's dtype says
        which it is."""
        self._check(self.L.nc_set_tensor_format(self.ctx, 1 if int16 else 0), "nc_set_tensor_format")
        self.x_int16 = bool(int16)

    def set_downsample(self, mode='first', seed=812):
        """Which reads a pileup deeper than maxcov keeps in the next snp_featurize / indel_sites_device calls (nc_set_downsample): 'first' (or 0,
        the default: the first maxcov in pileup order) or 'uniform' (or 1: the seeded uniform sample of nanocaller_amd.downsample)."""
        from .downsample import MODES
        m = MODES.get(mode, mode) if isinstance(mode, str) else mode
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
            raise ValueError("set_downsample: mode is 'first' or 'uniform', not %r" % (mode,))
        self._check(self.L.nc_set_downsample(self.ctx, int(m), int(seed) & 0xffffffff), "nc_set_downsample")

    @contextmanager
    def downsampling(self, downsample):
        """`downsample` = None (nothing is set) or (mode, seed): set for the calls inside, and cleared afterwards whatever their outcome"""
        if downsample is None:
            yield
            return
        try:
            self.set_downsample(*downsample)
            yield
        finally:
            self.L.nc_set_downsample(self.ctx, 0, 0)

    @contextmanager
    def _snp_state(self, int16=None, exact_fp32=None, range_flags=None):
        """The context's tensor format, CNN precision (None: as they stand) and range watch (nc_cnn_range_watch; None: none) for ONE library
        call; what was there before is put back, also when the call raises.  The only place that saves and restores this state."""
        was_i16, was_exact = self.x_int16, self.exact_fp32
        try:
            if int16 is not None and bool(int16) != was_i16:
                self.set_tensor_format(int16)
            if exact_fp32 is not None and bool(exact_fp32) != was_exact:
                self.set_cnn_precision(exact_fp32)
            if range_flags is not None:
                self._check(self.L.nc_cnn_range_watch(self.ctx, C.c_void_p(range_flags.data_ptr())), "nc_cnn_range_watch")
            yield
        finally:
            if range_flags is not None:                              # (no watch outlives a call: there was none before)
                self.L.nc_cnn_range_watch(self.ctx, None)
            if self.exact_fp32 != was_exact:
                self.set_cnn_precision(was_exact)
            if self.x_int16 != was_i16:
                self.set_tensor_format(was_i16)

    TRUNK_KERNELS = {0: "k4_conv12", 2: "k5_trunk_p3", 3: "k5_trunk_lin"}

    def trunk_info(self, int16=None):
        """-> (v_mfma_f32_16x16x32_f16 instructions per site, kernel name) of the SNP trunk a snp_forward launches in the current precision mode for
        int16 (True) or float32 (False) tensors; None: for the engine's default format.  k5_trunk_p3 13 x 24 + 10 x 27 + 8 x 18 = 726, k5_trunk_lin
        (int16 tensors) 613"""
        n, k = C.c_int32(), C.c_int32()
        with self._snp_state(int16=int16):
            self._check(self.L.nc_snp_trunk_info(self.ctx, C.byref(n), C.byref(k)), "nc_snp_trunk_info")
        return int(n.value), self.TRUNK_KERNELS[int(k.value)]

    def trunk_mfma_per_site(self) -> int:
        return self.trunk_info()[0]

    def enable_timing(self, on=True, trunk_only=False):
        """HIP-event timers: all stages, or (trunk_only) just the trunk kernel's launches, whose events ride on the
        kernel's dispatch packets and leave the stream undisturbed"""
        self._check(self.L.nc_enable_timing(self.ctx, (2 if trunk_only else 1) if on else 0), "nc_enable_timing")

    def last_ms(self, which):
        ms = C.c_float()
        self._check(self.L.nc_last_kernel_ms(self.ctx, which, C.byref(ms)), "nc_last_kernel_ms")
        return float(ms.value)

    def timing_sums(self):
        """-> (sum_ms float64 [6], count int64 [6]) over the calls since enable_timing(True): 0 scan, 1 featurize, 2 CNN
        stage, 3 indel, 4 trunk kernel launches (summed), 5 number of trunk launches."""
        sums, cnt = np.zeros(6, np.float64), np.zeros(6, np.int64)
        self._check(self.L.nc_timing_sums(self.ctx, _lib.npp(sums), _lib.npp(cnt)), "nc_timing_sums")
        return sums, cnt

    # ------------------------------------------------------------------ data movement
    def upload(self, hp: HostPack) -> DevicePack:
        dev = self.device
        ent_bytes = np.frombuffer(hp.tile_ent.tobytes(), np.uint8) if hp.tile_ent.size else np.zeros(16, np.uint8)
        dp = DevicePack(codes=torch.from_numpy(hp.codes).to(dev), tile_off=torch.from_numpy(hp.tile_off).to(dev),
                        tile_ent=torch.from_numpy(ent_bytes.copy()).to(dev), ref_code=torch.from_numpy(hp.ref_code).to(dev),
                        tile_size=hp.tile_size, tile_pos0=hp.tile_pos0, n_tiles=hp.n_tiles,
                        n_entries=int(hp.tile_ent.shape[0]), pos_lo=hp.pos_lo, pos_hi=hp.pos_hi)
        if hp.mates is not None:
            dp.mates = (torch.from_numpy(hp.mates[0]).to(dev), torch.from_numpy(hp.mates[1]).to(dev))
        if hp.ev_off is not None:
            z = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt) if a.size else np.zeros(1, dt)).to(dev)   # noqa: E731
            dp.events = dict(n_reads=int(hp.read_hap.shape[0]), ev_off=z(hp.ev_off, np.int32), ev_pos=z(hp.ev_pos, np.int32),
                             ev_len=z(hp.ev_len, np.int32), read_hap=z(hp.read_hap, np.uint8))
        return dp

    def load_weights(self, kind: int, w: Weights):
        if self._loaded.get(kind) == w.path:
            return
        if w.kind != kind:
            raise ValueError("weights %s are of kind %d, expected %d" % (w.path, w.kind, kind))
        flat = np.ascontiguousarray(w.flat, np.float32)
        self._check(self.L.nc_load_weights(self.ctx, kind, _lib.npp(flat), flat.size), "nc_load_weights")
        self._loaded[kind] = w.path

    # ------------------------------------------------------------------ K1
    def snp_scan(self, dp: DevicePack, chunks, *, mincov, min_allele_freq, threshold, haploid=False, async_fetch=False, sites=None,
                 sites_only=False, nbr_sites=None, nbr_only=False, sample=None) -> SnpSites:
        """chunks: list of (start, end) inclusive, same contig, ascending.
        sites (known-sites calling, nc_snp_scan_set_sites): 1-based positions of the contig (int array, or an int32 device tensor), any order,
        duplicates allowed -- a listed column that passes every other test is a candidate whatever its allele frequency; sites_only: the list
        alone decides (with no position in it, nothing is a candidate).  The list is cleared when the scan's kernels are enqueued.
        nbr_sites / nbr_only (nc_snp_scan_set_nbr_sites): the same for the neighbour rule -- a listed column that passes every other test is a
        neighbour site whatever its allele frequency; nbr_only: the list alone decides (with no position in it, no column is a neighbour), and
        snp_featurize then keeps a site that has min_nbr_sites such neighbours in reach, its own column not counted: a site none of the listed
        sites reaches has no tensor, with no position for the contig nothing has.
        sample = (seed, keep) (nc_snp_scan_set_sampling): keep = six probabilities in [0, 1), one per 5 % bin of the alternative allele
        frequency (the last one: 25 % and above); a column under the candidate test is a candidate with that probability, decided by a hash of
        its position and the seed.  Both are cleared with the list."""
        def on_device(s):
            if isinstance(s, torch.Tensor):
                d = s.to(device=self.device, dtype=torch.int32).contiguous()
            else:
                a = np.asarray(s).astype(np.int64, copy=False).ravel()
                a = a[(a >= 1) & (a <= np.iinfo(np.int32).max)]          # (no contig has other positions)
                d = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.device)
            d.record_stream(torch.cuda.current_stream(self.device))
            return d
        d_sites = on_device(sites) if sites is not None else None
        d_nbr = on_device(nbr_sites) if nbr_sites is not None else None
        threshold = [float(threshold[0]), float(threshold[1])]
        if sites_only and (d_sites is None or d_sites.numel() == 0):
            min_allele_freq = 2.0                                    # alt <= n: no column passes the frequency test, none is listed
        if nbr_only and (d_nbr is None or d_nbr.numel() == 0):
            threshold[0] = 2.0                                       # the same for the neighbour rule: t0 <= alt_freq never holds
        keep6 = None
        if sample is not None:
            seed, keep = sample
            keep = np.asarray(keep, np.float64).ravel()
            if keep.size != 6 or not np.all((keep >= 0.0) & (keep < 1.0)):
                raise ValueError("snp_scan: sample = (seed, keep) needs six probabilities in [0, 1)")
            keep6 = np.ascontiguousarray(sample_thresholds(keep))
            seed = int(seed) & 0xFFFFFFFF
        cs = np.ascontiguousarray([c[0] for c in chunks], np.int32)
        ce = np.ascontiguousarray([c[1] for c in chunks], np.int32)
        scan_lo = max(1, int(cs.min()) - _lib.FLANK)
        scan_hi = int(ce.max()) + _lib.FLANK
        if scan_lo < dp.pos_lo or min(scan_hi, dp.pos_hi) < scan_lo:
            pass  # the pack simply has no data there
        params = _lib.ScanParamsC(mincov=int(mincov), min_allele_freq=float(min_allele_freq), nbr_t0=float(threshold[0]),
                                  nbr_t1=float(threshold[1]), haploid=1 if haploid else 0)
        pc = dp.c_struct()
        listed = d_sites is not None and d_sites.numel() > 0
        listed_nbr = d_nbr is not None and d_nbr.numel() > 0
        try:
            if listed:
                self._check(self.L.nc_snp_scan_set_sites(self.ctx, int(d_sites.numel()), _ptr(d_sites), 1 if sites_only else 0), "nc_snp_scan_set_sites")
            if listed_nbr:
                self._check(self.L.nc_snp_scan_set_nbr_sites(self.ctx, int(d_nbr.numel()), _ptr(d_nbr), 1 if nbr_only else 0), "nc_snp_scan_set_nbr_sites")
            if keep6 is not None:
                self._check(self.L.nc_snp_scan_set_sampling(self.ctx, seed, _lib.npp(keep6)), "nc_snp_scan_set_sampling")
            self._check(self.L.nc_snp_scan_begin(self.ctx, C.byref(pc), _ptr(dp.ref_code), dp.tile_pos0, dp.ref_code.numel(), scan_lo,
                                                 scan_hi, C.byref(params), len(chunks), _lib.npp(cs), _lib.npp(ce)), "nc_snp_scan_begin")
        finally:
            if listed:                                               # the context never carries a list or a table into a later call
                self.L.nc_snp_scan_set_sites(self.ctx, 0, None, 0)
            if listed_nbr:
                self.L.nc_snp_scan_set_nbr_sites(self.ctx, 0, None, 0)
            if keep6 is not None:
                self.L.nc_snp_scan_set_sampling(self.ctx, 0, None)
        n_nbr, n_cand, n_sites = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.L.nc_snp_scan_end(self.ctx, C.byref(n_nbr), C.byref(n_cand), C.byref(n_sites)), "nc_snp_scan_end")
        N = n_sites.value
        # pinned host buffers (cached by torch's host allocator): the four copies run at PCIe speed, one sync
        hb, h = self._pinned.get((4, max(N, 1)), torch.int32)
        ptr = [C.c_void_p(hb[i].data_ptr()) for i in range(4)]
        if async_fetch:
            # copies go to the copy stream NOW: they run in the host's turn-around before the featuriser is launched (issued behind
            # that launch they collide with the featuriser and spill into the kernels after it: measured, worse)
            self._check(self.L.nc_snp_scan_fetch_async(self.ctx, self._copy_stream_ptr(), None, ptr[0], ptr[1], ptr[2], ptr[3]),
                        "nc_snp_scan_fetch_async")
        else:
            self._check(self.L.nc_snp_scan_fetch(self.ctx, None, ptr[0], ptr[1], ptr[2], ptr[3]), "nc_snp_scan_fetch")
        return SnpSites(n_sites=N, n_nbr=n_nbr.value, pos=h[0, :N], chunk=h[1, :N], dp=h[2, :N], alt=h[3, :N], nbr_only=bool(nbr_only))

    def fetch_nbr_sites(self, n_nbr) -> np.ndarray:
        out = np.empty(n_nbr, np.int32)
        self._check(self.L.nc_snp_scan_fetch(self.ctx, _lib.npp(out), None, None, None, None), "nc_snp_scan_fetch")
        return out

    # ------------------------------------------------------------------ reference-confidence blocks (csrc/nc_refconf.hip; gvcf.py)
    REFCONF_TILE = 4096                                              # columns per workgroup of the blocks kernels (the tests put borders on it)

    @staticmethod
    def _refconf_params(error, bands, haploid):
        from . import gvcf
        c_m, c_x, c_h = gvcf.constants(error)
        b = gvcf.gq_bands(bands)
        prm = _lib.RefconfParamsC(c_m=c_m, c_x=c_x, c_h=c_h, haploid=1 if haploid else 0, n_bands=len(b))
        for k, v in enumerate(b):
            prm.band[k] = v
        return prm

    def refconf_columns(self, dp: DevicePack):
        """-> (words, ref_code, tile_pos0): one int32 (the bits of a uint32: n | alt << 16, all ones where the reference code is >= 4) per column of
        the pack's tile grid, the grid's reference codes (a copy: packs of an ingest pipeline share one buffer) and the grid's first position.
        Enqueued on the context's stream while the pack is resident; nothing later needs the pack."""
        npos = dp.n_tiles * dp.tile_size
        if dp.ref_code.numel() < npos:
            raise ValueError("refconf_columns: the pack's reference codes hold %d columns, its tile grid %d" % (dp.ref_code.numel(), npos))
        words = torch.empty(npos, dtype=torch.int32, device=self.device)
        pc = dp.c_struct()
        self._check(self.L.nc_refconf_columns(self.ctx, C.byref(pc), _ptr(dp.ref_code), dp.tile_pos0, npos, _ptr(words)), "nc_refconf_columns")
        return words, dp.ref_code[:npos].clone(), dp.tile_pos0

    def refconf_blocks(self, words, dpk, chunks, cuts, *, error, bands, haploid=False, device_out=False):
        """The blocks of `words` (refconf_columns, or any int32 / uint32-bits device tensor of that form, a multiple of 16 long) -> int32 [n][6]:
        start, end, min n, min GQ, n and alt of the leftmost column with that GQ (host array; device_out: a device tensor).
        dpk: the pack (its tile_pos0 places column 0) or that position itself, a multiple of 16; chunks: (start, end) inclusive intervals whose union
        is the region; cuts: None or an int array [k][2] of inclusive intervals (host or device) whose columns belong to no block."""
        tile_pos0 = int(getattr(dpk, "tile_pos0", dpk))
        prm = self._refconf_params(error, bands, haploid)
        cs = np.ascontiguousarray([c[0] for c in chunks], np.int32)
        ce = np.ascontiguousarray([c[1] for c in chunks], np.int32)
        d_cs = d_ce = None
        n_cut = 0
        if cuts is not None and len(cuts):
            d_cuts = cuts if isinstance(cuts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cuts, np.int32).reshape(-1, 2))
            d_cuts = d_cuts.to(device=self.device, dtype=torch.int32)
            d_cs, d_ce = d_cuts[:, 0].contiguous(), d_cuts[:, 1].contiguous()
            n_cut = int(d_cs.numel())
        nb = C.c_int64()
        self._check(self.L.nc_refconf_blocks(self.ctx, _ptr(words), tile_pos0, int(words.numel()), len(chunks), _lib.npp(cs), _lib.npp(ce), n_cut,
                                             _ptr(d_cs), _ptr(d_ce), C.byref(prm), C.byref(nb)), "nc_refconf_blocks")
        n = int(nb.value)
        if device_out:
            out = torch.empty((n, 6), dtype=torch.int32, device=self.device)
            self._check(self.L.nc_refconf_fetch(self.ctx, _ptr(out) if n else None), "nc_refconf_fetch")
            return out
        out = np.empty((n, 6), np.int32)
        self._check(self.L.nc_refconf_fetch(self.ctx, _lib.npp(out) if n else None), "nc_refconf_fetch")
        return out

    def refconf_text(self, blocks, ref_code, tile_pos0, chrom, *, error, haploid=False, device_out=False):
        """The records of `blocks` (refconf_blocks; host array or device tensor) written on the device -> (text uint8 host array, byte offset of
        every line int64 [n + 1] host array); device_out: the two device tensors instead.  ref_code: the grid's reference codes (device uint8,
        index 0 = tile_pos0)."""
        prm = self._refconf_params(error, None, haploid)
        d_blocks = blocks if isinstance(blocks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(blocks, np.int32).reshape(-1, 6))
        d_blocks = d_blocks.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(d_blocks.shape[0])
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        nbytes = C.c_int64()
        args = (self.ctx, n, _ptr(d_blocks) if n else None, _ptr(ref_code), int(tile_pos0), int(ref_code.numel()), str(chrom).encode(), C.byref(prm), _ptr(off))
        self._check(self.L.nc_refconf_text(*args, None, 0, C.byref(nbytes)), "nc_refconf_text")
        text = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=self.device)
        self._check(self.L.nc_refconf_text(*args, _ptr(text), int(nbytes.value), None), "nc_refconf_text")
        if device_out:
            return text[:int(nbytes.value)], off
        return text[:int(nbytes.value)].cpu().numpy(), off.cpu().numpy()

    # ------------------------------------------------------------------ text lines (csrc/nc_vcfwrite.hip)
    def lines_merge(self, a, b):
        """The stable merge by key of two lists of lines, each a tuple of device tensors (text uint8, line_off int64 [n + 1] from 0, key int64 [n]
        ascending, beg int64 [n], end int64 [n]) or None for an empty list; at equal keys b's lines go first (nc_lines_merge)
        -> (text, line_off [na + nb + 1], beg, end, src int32: a's line i is i, b's line j is na + j), device tensors."""
        dev = self.device

        def norm(lst):
            if lst is None or int(lst[2].numel()) == 0:
                return 0, 0, (None,) * 5
            text, off, key, beg, end = lst
            n = int(key.numel())
            if int(off.numel()) != n + 1 or int(beg.numel()) != n or int(end.numel()) != n:
                raise ValueError("lines_merge: %d keys need %d offsets and %d begins and ends" % (n, n + 1, n))
            t = (text.contiguous(),) + tuple(x.to(device=dev, dtype=torch.int64).contiguous() for x in (off, key, beg, end))
            return n, int(text.numel()), t
        na, ba, A = norm(a)
        nb, bb, B = norm(b)
        n, nbytes = na + nb, ba + bb
        out = torch.empty(max(16, nbytes), dtype=torch.uint8, device=dev)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        beg, end = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        src = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.zeros(3, dtype=torch.int32, device=dev)
        self._check(self.L.nc_lines_merge(self.ctx, na, *(_ptr(x) for x in A), nb, *(_ptr(x) for x in B), nbytes, _ptr(out), _ptr(off),
                                          _ptr(beg) if n else None, _ptr(end) if n else None, _ptr(src) if n else None, _ptr(st)), "nc_lines_merge")
        bad = st.cpu().numpy()
        if bad.any():
            raise ValueError("lines_merge: %s" % "; ".join(w for w, x in zip(("the texts do not hold the bytes their offsets say", "a list's line offsets descend",
                                                                             "a list's keys descend"), bad) if x))
        return out[:nbytes], off, beg, end, src

    def lines_index(self, beg, end, line_off, u0, foff, *, min_shift=14, depth=5):
        """A BGZF piece's share of a CSI index (nc_lines_index): its n lines in file order (device int64 tensors: 0-based beg / end [n], line_off
        [n + 1] with the piece's text starting at offset u0), foff = device int64 [members + 1], where every member starts in the piece and the
        piece's length.  -> dict(run_bin int32, run_vbeg, run_vend uint64: the chunk runs; w0, win_min uint64: the window minima from window w0
        on), host arrays; virtual offsets are relative to the piece.  Raises ValueError where the ends or begins do not ascend."""
        n = int(beg.numel())
        if n == 0:
            return dict(run_bin=np.zeros(0, np.int32), run_vbeg=np.zeros(0, np.uint64), run_vend=np.zeros(0, np.uint64), w0=0, win_min=np.zeros(0, np.uint64))
        work = torch.empty(n + (n + 4095) // 4096 + 8, dtype=torch.int32, device=self.device)
        info = (C.c_int64 * 4)()
        args = (self.ctx, n, _ptr(beg), _ptr(end), _ptr(line_off), int(u0), int(foff.numel()) - 1, _ptr(foff), int(min_shift), int(depth), _ptr(work), info)
        self._check(self.L.nc_lines_index(*args, None, None, None, None), "nc_lines_index")
        if info[3]:
            raise ValueError("lines_index: %s" % "; ".join(w for k, w in enumerate(("the lines' ends do not ascend", "the lines' begins do not ascend",
                                                                                    "an empty interval, or line offsets that do not fit the members")) if info[3] >> k & 1))
        n_runs, w0, n_win = int(info[0]), int(info[1]), int(info[2])
        out = torch.empty(4 * n_runs + 8 * (2 * n_runs + n_win), dtype=torch.uint8, device=self.device)    # one buffer, one copy back
        v = out[:8 * (2 * n_runs + n_win)].view(torch.int64)
        rb = out[8 * (2 * n_runs + n_win):].view(torch.int32)
        self._check(self.L.nc_lines_index(*args, _ptr(rb), _ptr(v[:n_runs]), _ptr(v[n_runs:2 * n_runs]), _ptr(v[2 * n_runs:])), "nc_lines_index")
        h = out.cpu().numpy()
        hv = h[:8 * (2 * n_runs + n_win)].view(np.uint64)
        return dict(run_bin=h[8 * (2 * n_runs + n_win):].view(np.int32).copy(), run_vbeg=hv[:n_runs].copy(), run_vend=hv[n_runs:2 * n_runs].copy(),
                    w0=w0, win_min=hv[2 * n_runs:].copy())

    # ------------------------------------------------------------------ K2-K4
    def snp_featurize(self, dp: DevicePack, sites: SnpSites, *, seq, maxcov, min_nbr_sites=1, int16=None, downsample=None) -> SnpSites:
        """downsample: None, or (mode, seed) for this call (set_downsample; downsample.resolve(params) gives it): with 'uniform' a pileup deeper
        than maxcov keeps a seeded uniform sample, and a pack with shared read names is refused (NC_ERR_UNSUPPORTED).
        int16: sites.x as int16 (True) or as the reference's float32 (False); None: the engine's default (set_tensor_format).
        min_nbr_sites: the reference's test of :244, which counts the site's own column; for sites of a scan in neighbour only mode
        (sites.nbr_only) it counts the listed neighbours alone, so the kernel is asked for one column more."""
        if sites.nbr_only:
            min_nbr_sites = int(min_nbr_sites) + 1
        N = sites.n_sites
        dev = self.device
        want16 = self.x_int16 if int16 is None else bool(int16)
        # alignments that share read names are keyed by name in the int16-tensor kernel only: it runs, float32 tensors are its cast (exact)
        i16 = want16 or dp.mates is not None
        # one allocation carved into the six outputs (this sits between the scan's totals and the featuriser's launch: the GPU idles)
        xb = N * 1025 * (2 if i16 else 4)
        a16 = lambda v: (v + 15) & ~15     # noqa: E731
        o_ref = a16(xb); o_fwd = a16(o_ref + 4 * N); o_rev = a16(o_fwd + 16 * N); o_dep = a16(o_rev + 16 * N); o_val = a16(o_dep + 4 * N)
        buf = torch.empty(o_val + N + 16, dtype=torch.uint8, device=dev)
        sites.x = buf[:xb].view(torch.int16 if i16 else torch.float32).view(N, 5, 41, 5)
        sites.ref_code = buf[o_ref:o_ref + 4 * N].view(torch.int32)
        sites.fwd_dp = buf[o_fwd:o_fwd + 16 * N].view(torch.int32).view(N, 4)
        sites.rev_dp = buf[o_rev:o_rev + 16 * N].view(torch.int32).view(N, 4)
        sites.depth = buf[o_dep:o_dep + 4 * N].view(torch.int32)
        sites.valid = buf[o_val:o_val + N]
        pc = dp.c_struct()
        if dp.mates is not None:                                     # alignments that share read names: the featuriser keys them by name
            self._check(self.L.nc_snp_set_mates(self.ctx, int(dp.mates[0].numel()), _ptr(dp.mates[0]), _ptr(dp.mates[1])), "nc_snp_set_mates")
        try:
            with self._snp_state(int16=i16), self.downsampling(downsample):
                self._check(self.L.nc_snp_featurize(self.ctx, C.byref(pc), _ptr(dp.ref_code), dp.tile_pos0, dp.ref_code.numel(),
                                                    _lib.SEQ_MODES[seq], int(maxcov), int(min_nbr_sites), _ptr(sites.x),
                                                    _ptr(sites.ref_code), _ptr(sites.fwd_dp), _ptr(sites.rev_dp), _ptr(sites.depth),
                                                    _ptr(sites.valid)), "nc_snp_featurize")
        finally:
            if dp.mates is not None:
                self.L.nc_snp_set_mates(self.ctx, 0, None, None)
        if not want16 and i16:
            sites.x = sites.x.to(torch.float32)
        return sites

    def snp_scale(self, sites: SnpSites, n_chunks, train_coverage, per_site=False, async_fetch=False):
        """-> (scale f64 [N] device tensor, chunk_depth float64 host [n_chunks]).  async_fetch: the chunk depths arrive in
        pinned memory through the copy stream (valid after wait_copies() / a later copy_event()), and the compute stream
        is not synchronised between the featuriser and the CNN."""
        scale = torch.empty(sites.n_sites, dtype=torch.float64, device=self.device)
        if not async_fetch:
            cd = np.zeros(n_chunks, np.float64)
            self._check(self.L.nc_snp_scale(self.ctx, _ptr(sites.depth), _ptr(sites.valid), float(train_coverage),
                                            1 if per_site else 0, _ptr(scale), _lib.npp(cd)), "nc_snp_scale")
            return scale, cd
        hb, cd = self._pinned.get((max(int(n_chunks), 1),), torch.float64)
        self._check(self.L.nc_snp_scale(self.ctx, _ptr(sites.depth), _ptr(sites.valid), float(train_coverage),
                                        1 if per_site else 0, _ptr(scale), None), "nc_snp_scale")
        self._check(self.L.nc_snp_chunk_depth_async(self.ctx, self._copy_stream_ptr(), C.c_void_p(hb.data_ptr())), "nc_snp_chunk_depth_async")
        return scale, cd[:int(n_chunks)]

    # ------------------------------------------------------------------ K5 / K9
    def x_limit(self, kind) -> float:
        """largest |scaled input value| for which the loaded model's weights prove that the split-precision trunk stays inside the
        fp16 range (nc_cnn_x_limit)"""
        v = C.c_float()
        self._check(self.L.nc_cnn_x_limit(self.ctx, kind, C.byref(v)), "nc_cnn_x_limit")
        return float(v.value)

    def snp_forward_guarded(self, kind, x, ref_code, scale, scale_mode=0):
        """snp_forward on the split-precision trunk with its range guard closed: sites whose scaled tensor exceeds x_limit are re-run
        on the exact fp32 trunk.  -> (probs, gt, number of re-run sites); synchronous (tests, small batches; call_chunks does the same
        asynchronously)."""
        n = int(x.shape[0])
        flags = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.device)
        probs, gt = self.snp_forward(kind, x, ref_code, scale, scale_mode, range_flags=flags)
        idx = torch.nonzero(flags[:n]).squeeze(1)
        if idx.numel():
            self.range_rerun(kind, x, ref_code, scale, scale_mode, idx, probs, gt)
        return probs, gt, int(idx.numel())

    def range_rerun(self, kind, x, ref_code, scale, scale_mode, idx, probs, gt):
        """the sites `idx` (device int64) once more on the exact fp32 MFMA trunk; their rows of probs / gt (device tensors) are replaced"""
        xs = x[idx].to(torch.float32).contiguous()                   # the exact trunk reads the reference's float32 layout
        with self._snp_state(exact_fp32=True):
            p2, g2 = self.snp_forward(kind, xs, ref_code[idx].contiguous(), scale[idx].contiguous() if scale is not None else None, scale_mode,
                                      want_gt=gt is not None)
        probs[idx] = p2
        if gt is not None and g2 is not None:
            gt[idx] = g2

    def snp_forward(self, kind, x, ref_code, scale, scale_mode=0, want_gt=True, drain=False, range_flags=None):
        """-> (probs, gt) device tensors; with drain=True also (probs_host, gt_host) numpy arrays in pinned memory that
        the copy stream fills batch by batch while the next batch computes (wait_copies() before reading them).
        x: int16 tensors (the featuriser's exact short form) or the reference's float32 layout -- its dtype says which, the engine's default
        format plays no part.
        range_flags (uint8 device tensor [n], zeroed): the split-precision trunk marks the sites whose scaled tensor exceeds the
        model's x_limit (nc_cnn_range_watch)."""
        if x.dtype not in (torch.int16, torch.float32):
            raise ValueError("snp_forward: tensors of dtype %s (int16 or float32 expected)" % x.dtype)
        n = int(x.shape[0])
        probs = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        gt = torch.empty((n, 2), dtype=torch.float32, device=self.device) if (want_gt and kind == _lib.MODEL_SNP) else None
        with self._snp_state(int16=x.dtype == torch.int16, range_flags=range_flags):
            if not drain:
                self._check(self.L.nc_snp_forward(self.ctx, kind, n, _ptr(x), _ptr(ref_code), _ptr(scale), int(scale_mode),
                                                  _ptr(probs), _ptr(gt)), "nc_snp_forward")
                return probs, gt
            hp, hp_np = self._pinned.get((n, 4), torch.float32)
            hg, hg_np = self._pinned.get((n, 2), torch.float32) if gt is not None else (None, None)
            self._check(self.L.nc_snp_forward_drain(self.ctx, kind, n, _ptr(x), _ptr(ref_code), _ptr(scale), int(scale_mode),
                                                    _ptr(probs), _ptr(gt), self._copy_stream_ptr(), C.c_void_p(hp.data_ptr()),
                                                    C.c_void_p(hg.data_ptr()) if hg is not None else None), "nc_snp_forward_drain")
            return probs, gt, hp_np, hg_np

    def indel_forward(self, kind, x):
        n = int(x.shape[0])
        nout = 4 if kind == _lib.MODEL_INDEL else 1
        probs = torch.empty((n, nout), dtype=torch.float32, device=self.device)
        self._check(self.L.nc_indel_forward(self.ctx, kind, n, _ptr(x), _ptr(probs)), "nc_indel_forward")
        return probs

    def snp_phase(self, site_pos, site_alleles, read_group, n_groups, *, max_cov=15, reads=None, csr=None, realign=None, site_gt=None,
                  distrust_cost=1, weights=None, bam_quals=None) -> dict:
        """Read-based phasing + haplotags (nc_snp_phase_*, nc_haplotag_run) -> dict of host arrays (see nc_phase_arrays).
        reads: (codes, rd_start, rd_end, slot_off) device tensors of a resident pack's kept reads (alleles gathered on the device);
        csr: (entry_off int64, entry_site int32, entry_allele uint8) host arrays instead;
        realign: (codes, IndelReadsC, n_events, n_ins_bases, ref_code) -- the pack's codes, its read table with the events and the inserted
        bases, and the contig's reference codes [length] (device uint8, position p at p - 1, 4 = not a base): alleles by local
        realignment (nc_snp_phase_realign).
        site_gt: the called class per site (uint8: 0 het, 1 / 2 homozygous for the first / second allele) -- the genotypes are not trusted
        (nc_snp_phase_solve_gt with the price `distrust_cost` of leaving a call) and the result gains `site_gt`, the outcome per site.
        The weighted model (an allele's flip costs its weight, reads may be barred from selection), either of
        weights: (entry_weight uint8 [n_entries] in 0..93, read_ok uint8 [n_reads]) host arrays, either None = all 1 (nc_snp_phase_set_weights);
        bam_quals: (raw, rec_off, mapq_min, default_weight, w_max) -- the device ingest's inflated record stream (uint8 device tensor), the kept
        reads' record offsets in the reads' order (int64 device tensor): base qualities capped at w_max as weights, read_ok = MAPQ >= mapq_min
        (nc_snp_phase_weights_from_bam).
        The result then gains `entry_weight`, `read_mapq` and `read_ok`."""
        pos = np.ascontiguousarray(site_pos, np.int32)
        h = self._phase_open(pos, site_alleles, reads, csr, realign)
        try:
            self._phase_weigh(h, weights, bam_quals)
            if site_gt is None:
                self._check(self.L.nc_snp_phase_solve(self.ctx, h, int(max_cov)), "nc_snp_phase_solve")
            else:
                gt = np.ascontiguousarray(site_gt, np.uint8)
                if gt.shape != pos.shape:
                    raise ValueError("snp_phase: site_gt holds %d classes for %d sites" % (gt.size, pos.size))
                self._check(self.L.nc_snp_phase_solve_gt(self.ctx, h, int(max_cov), _lib.npp(gt), int(distrust_cost)), "nc_snp_phase_solve_gt")
            grp = np.ascontiguousarray(read_group, np.int32)
            self._check(self.L.nc_haplotag_run(self.ctx, h, int(n_groups), _lib.npp(grp)), "nc_haplotag_run")
            return self._phase_result(h, with_gt=site_gt is not None, with_weights=weights is not None or bam_quals is not None)
        finally:
            self.L.nc_snp_phase_free(h)

    def _phase_open(self, pos, site_alleles, reads, csr, realign):
        """the phasing handle of snp_phase's `realign=`, `reads=` or `csr=` (the caller frees it)"""
        L, h = self.L, C.c_void_p()
        if realign is not None or reads is not None:
            al = np.ascontiguousarray(site_alleles, np.uint8).reshape(-1, 2)
            torch.cuda.current_stream(self.device).synchronize()            # (the pack's upload may still be in flight on torch's stream)
        if realign is not None:
            codes, reads_c, n_events, n_ins, ref_code = realign
            rc = L.nc_snp_phase_realign(self.ctx, _ptr(codes), codes.numel(), C.byref(reads_c), int(n_events), int(n_ins), _ptr(ref_code),
                                        int(ref_code.numel()), pos.size, _lib.npp(pos), _lib.npp(al), C.byref(h))
            self._check(rc, "nc_snp_phase_realign")
        elif reads is not None:
            codes, rs, re_, so = reads
            rc = L.nc_snp_phase_gather(self.ctx, _ptr(codes), codes.numel(), int(rs.numel()), _ptr(rs), _ptr(re_), _ptr(so), pos.size, _lib.npp(pos),
                                       _lib.npp(al), C.byref(h))
            self._check(rc, "nc_snp_phase_gather")
        else:
            off, site, allele = (np.ascontiguousarray(a, t) for a, t in zip(csr, (np.int64, np.int32, np.uint8)))
            self._check(L.nc_snp_phase_load(self.ctx, off.size - 1, pos.size, _lib.npp(pos), _lib.npp(off), _lib.npp(site), _lib.npp(allele),
                                            C.byref(h)), "nc_snp_phase_load")
        return h

    def _phase_view(self, h):
        v = _lib.PhaseArraysC()
        self.L.nc_snp_phase_view(h, C.byref(v))
        return v

    def _phase_weigh(self, h, weights, bam_quals):
        """the weighted model on the handle, from snp_phase's `weights=` or `bam_quals=`"""
        if weights is not None and bam_quals is not None:
            raise ValueError("snp_phase: weights= and bam_quals= are two sources of the same weights")
        if weights is None and bam_quals is None:
            return
        v = self._phase_view(h)
        if weights is not None:
            ew, ok = (None if a is None else np.ascontiguousarray(a, np.uint8) for a in weights)
            if (ew is not None and ew.size != v.n_entries) or (ok is not None and ok.size != v.n_reads):
                raise ValueError("snp_phase: weights= holds %s weights / %s flags for %d entries / %d reads"
                                 % (None if ew is None else ew.size, None if ok is None else ok.size, v.n_entries, v.n_reads))
            self._check(self.L.nc_snp_phase_set_weights(self.ctx, h, None if ew is None else _lib.npp(ew), None if ok is None else _lib.npp(ok)),
                        "nc_snp_phase_set_weights")
        else:
            raw, rec_off, mapq_min, default_weight, w_max = bam_quals
            if rec_off.dtype != torch.int64 or rec_off.numel() != v.n_reads or raw.dtype != torch.uint8:
                raise ValueError("snp_phase: bam_quals= needs a uint8 record stream and %d int64 record offsets, one per read" % v.n_reads)
            torch.cuda.current_stream(self.device).synchronize()
            self._check(self.L.nc_snp_phase_weights_from_bam(self.ctx, h, _ptr(raw), int(raw.numel()), _ptr(rec_off), int(mapq_min), int(default_weight),
                                                             int(w_max)), "nc_snp_phase_weights_from_bam")

    def _phase_result(self, h, with_gt, with_weights) -> dict:
        """snp_phase's result: copies of the handle's arrays"""
        L, v = self.L, self._phase_view(h)

        def a(ptr, n, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), (n,)).copy() if n and ptr else np.zeros(0, dt)
        R, S, nb, ng = v.n_reads, v.n_sites, v.n_blocks, v.n_groups
        extra = {}
        if with_gt:
            g = C.c_void_p()
            L.nc_snp_phase_genotypes(h, C.byref(g))
            extra = dict(site_gt=a(g, S, np.uint8))
        if with_weights:
            pw, pm, po = C.c_void_p(), C.c_void_p(), C.c_void_p()
            L.nc_snp_phase_weights(h, C.byref(pw), C.byref(pm), C.byref(po))
            extra.update(entry_weight=a(pw, v.n_entries, np.uint8), read_mapq=a(pm, R, np.uint8), read_ok=a(po, R, np.uint8))
        return dict(entry_off=a(v.entry_off, R + 1, np.int64), entry_site=a(v.entry_site, v.n_entries, np.int32),
                    entry_allele=a(v.entry_allele, v.n_entries, np.uint8), side=a(v.read_side, R, np.int8),
                    site_block=a(v.site_block, S, np.int32), site_h=a(v.site_h, S, np.uint8), site_phased=a(v.site_phased, S, np.uint8).astype(bool),
                    site_ps=a(v.site_ps, S, np.int32), block_first=a(v.block_first, nb, np.int32), block_last=a(v.block_last, nb, np.int32),
                    block_ps=a(v.block_ps, nb, np.int32), block_cost=a(v.block_cost, nb, np.int64), group_hp=a(v.group_hp, ng, np.uint8),
                    group_ps=a(v.group_ps, ng, np.int32), ms=dict(zip(("gather", "select", "dp", "haplotag"), list(v.ms))), **extra)

    # ---- writing BAM (csrc/nc_bamwrite.hip; bam_write.py).  Device tensors in and out, on the context's stream.
    def bam_retag_sizes(self, raw, rec_off, thash, tps, new_size, tag_idx, out_off, status, raw_byte_off=0):
        """new size, table row and output offset of every record (nc_bam_retag_sizes); thash int64 tensor of the uint64 hashes, ascending"""
        self._check(self.L.nc_bam_retag_sizes(self.ctx, C.c_void_p(raw.data_ptr() + raw_byte_off), int(rec_off.numel()), _ptr(rec_off),
                                              _ptr(thash) if thash.numel() else None, _ptr(tps) if tps.numel() else None, int(thash.numel()),
                                              _ptr(new_size), _ptr(tag_idx), _ptr(out_off), _ptr(status)), "nc_bam_retag_sizes")

    def bam_retag(self, raw, rec_off, thp, tps, tag_idx, out_off, out, out_byte_off=0, raw_byte_off=0):
        """the re-tagged records at out + out_byte_off + out_off[i] (nc_bam_retag)"""
        self._check(self.L.nc_bam_retag(self.ctx, C.c_void_p(raw.data_ptr() + raw_byte_off), int(rec_off.numel()), _ptr(rec_off),
                                        _ptr(thp) if thp.numel() else None, _ptr(tps) if tps.numel() else None, _ptr(tag_idx), _ptr(out_off),
                                        C.c_void_p(out.data_ptr() + out_byte_off)), "nc_bam_retag")

    def bgzf_deflate(self, data, ioff, ilen, out, ooff, clen, status, crc=None):
        """raw-deflate payload of every member data[ioff[b] : ioff[b] + ilen[b]] at out[ooff[b]:], clen[b] bytes (nc_bgzf_deflate_device);
        crc: also their CRC-32s"""
        self._check(self.L.nc_bgzf_deflate_device(self.ctx, int(ioff.numel()), _ptr(data), _ptr(ioff), _ptr(ilen), _ptr(out), _ptr(ooff), _ptr(clen),
                                                  _ptr(crc), _ptr(status)), "nc_bgzf_deflate_device")

    def bgzf_crc32(self, data, ioff, ilen, crc):
        self._check(self.L.nc_bgzf_crc32_device(self.ctx, int(ioff.numel()), _ptr(data), _ptr(ioff), _ptr(ilen), _ptr(crc)), "nc_bgzf_crc32_device")

    def bgzf_assemble(self, pay, poff, clen, crc, isize, foff, file=None):
        """member offsets foff [n + 1] in the BGZF file image; with `file`, the image itself (nc_bgzf_assemble_device)"""
        self._check(self.L.nc_bgzf_assemble_device(self.ctx, int(clen.numel()), _ptr(pay), _ptr(poff), _ptr(clen), _ptr(crc), _ptr(isize), _ptr(foff),
                                                   _ptr(file)), "nc_bgzf_assemble_device")

    def fasta_decode(self, raw, first, length, linebases, linewidth, *, letters=None, scan=None, scan_pos0=1, ga=1, gb=None, blind=None, status=None,
                     raw_len=None):
        """one contig of the FASTA file image `raw` (uint8 device tensor; `first`, `length`, `linebases`, `linewidth`: its .fai columns) to
        `letters` [length], `scan` (the scan's codes, entry p - scan_pos0 for p in [ga, gb], 4 elsewhere) and `blind` [length], each a uint8 device
        tensor or None (nc_fasta_decode, on the context's stream; returns when they are complete).  A file the .fai does not describe raises."""
        if status is None:
            status = torch.empty(1, dtype=torch.int32, device=self.device)
        rc = self.L.nc_fasta_decode(self.ctx, _ptr(raw), int(raw.numel() if raw_len is None else raw_len), int(first), int(length), int(linebases),
                                    int(linewidth), _ptr(letters), _ptr(scan), int(scan_pos0), 0 if scan is None else int(scan.numel()), int(ga),
                                    int(length if gb is None else gb), _ptr(blind), _ptr(status))
        self._check(rc, "nc_fasta_decode")

    def indel_scan(self, dp: DevicePack, start, end, *, mincov, win_size, small_win_size, ins_t, del_t, excl=None, haploid=False, impute=False):
        """K7 -> int8 [end-start+1] per-column decision (-1 none, 0 long-window rule, 1 small-window rule, 2 impute_indel_phase
        candidate when impute=True)."""
        if dp.events is None:
            raise ValueError("this read pack carries no indel events / haplotype tags")
        ev = dp.events
        evc = _lib.IndelEventsC(n_reads=ev["n_reads"], ev_off=ev["ev_off"].data_ptr(), ev_pos=ev["ev_pos"].data_ptr(),
                                ev_len=ev["ev_len"].data_ptr(), read_hap=ev["read_hap"].data_ptr())
        prm = _lib.IndelScanParamsC(mincov=int(mincov), win_size=int(win_size), small_win_size=int(small_win_size),
                                    ins_t=float(ins_t), del_t=float(del_t), haploid=1 if haploid else 0, impute=1 if impute else 0)
        lo = max(1, int(start))
        out = np.empty(int(end) - lo + 1, np.int8)
        pc = dp.c_struct()
        self._check(self.L.nc_indel_scan(self.ctx, C.byref(pc), C.byref(evc), _ptr(excl), lo, int(end), C.byref(prm),
                                         _lib.npp(out)), "nc_indel_scan")
        return out

    def indel_scan_batch(self, dp: DevicePack, chunks, *, mincov, win_size, small_win_size, ins_t, del_t, excl=None, haploid=False, impute=False):
        """K7 for a list of (start, end) chunks of one contig -> list of int8 arrays (one per chunk); ascending chunk lists run in
        the same kernel launches (chunk = a grid dimension)."""
        if dp.events is None:
            raise ValueError("this read pack carries no indel events / haplotype tags")
        ev = dp.events
        evc = _lib.IndelEventsC(n_reads=ev["n_reads"], ev_off=ev["ev_off"].data_ptr(), ev_pos=ev["ev_pos"].data_ptr(),
                                ev_len=ev["ev_len"].data_ptr(), read_hap=ev["read_hap"].data_ptr())
        prm = _lib.IndelScanParamsC(mincov=int(mincov), win_size=int(win_size), small_win_size=int(small_win_size),
                                    ins_t=float(ins_t), del_t=float(del_t), haploid=1 if haploid else 0, impute=1 if impute else 0)
        starts = np.ascontiguousarray([c[0] for c in chunks], np.int32)
        ends = np.ascontiguousarray([c[1] for c in chunks], np.int32)
        ncol = ends.astype(np.int64) - np.maximum(starts, 1) + 1
        off = np.zeros(len(chunks) + 1, np.int64)
        np.cumsum(ncol, out=off[1:])
        out = np.empty(int(off[-1]), np.int8)
        pc = dp.c_struct()
        self._check(self.L.nc_indel_scan_batch(self.ctx, C.byref(pc), C.byref(evc), _ptr(excl), len(chunks), _lib.npp(starts),
                                               _lib.npp(ends), C.byref(prm), _lib.npp(out), _lib.npp(off)), "nc_indel_scan_batch")
        return [out[off[k]:off[k + 1]] for k in range(len(chunks))]

    def star_msa_tensor(self, read_sets, refs, *, open_=None, extend=None, match=None, mismatch=None, max_cols=None, want_rows=False, cns_as_str=False):
        """Device star alignment (nc_star_msa_tensor) of many read sets at once + the rows -> tensor kernel.
        read_sets[s]: list of read strings, refs[s]: reference window string.
        -> (x f32 [S,5,128,2] device, cns list of uint8 arrays (or, cns_as_str, AGTC strings) with gaps removed, n_cols int32 [S]
            [, rows list of uint8 [n_reads, n_cols], ref_rows list of uint8 [n_cols]])"""
        S = len(read_sets)
        if S == 0:
            x = torch.empty((0, 5, 128, 2), dtype=torch.float32, device=self.device)
            return (x, [], np.zeros(0, np.int32)) + (([], []) if want_rows else ())
        n_reads = np.fromiter(map(len, read_sets), np.int64, S)
        set0 = np.zeros(S + 1, np.int32)
        np.cumsum(n_reads, out=set0[1:])
        flat = [q for rs in read_sets for q in rs]
        rlen = np.fromiter(map(len, flat), np.int64, len(flat))
        read_off = np.zeros(len(flat) + 1, np.int32)
        np.cumsum(rlen, out=read_off[1:])
        reflen = np.fromiter(map(len, refs), np.int64, S)
        ref_off = np.zeros(S + 1, np.int32)
        np.cumsum(reflen, out=ref_off[1:])
        raw_reads, raw_refs = "".join(flat).encode(), "".join(refs).encode()
        # every read base can at most add one column to its set
        per_set = np.zeros(S, np.int64)
        nz = n_reads > 0
        if len(flat):
            per_set[nz] = np.add.reduceat(rlen, set0[:-1][nz])
        cap = reflen + per_set
        mc = int(max_cols) if max_cols else int(cap.max())
        return self.star_msa_tensor_flat(S, raw_reads, read_off, set0, raw_refs, ref_off, mc, open_=open_, extend=extend, match=match,
                                         mismatch=mismatch, want_rows=want_rows, cns_as_str=cns_as_str, _n_reads=n_reads, _cap=cap)

    def star_msa_tensor_flat(self, S, reads, read_off, set_read0, refs, ref_off, max_cols, *, open_=None, extend=None, match=None, mismatch=None,
                             want_rows=False, cns_as_str=False, _n_reads=None, _cap=None, al_dup=None):
        """The same on flat host buffers (what nc_indel_pass2_sets produces): `reads` / `refs` bytes objects or raw pointers
        (ints / c_void_p), read_off / set_read0 / ref_off int32 arrays or pointers.  al_dup (int32 array or pointer, optional):
        nc_pass2_arrays.al_dup -- alignments that repeat an earlier one are not computed again."""
        open_, extend, match, mismatch = [d if v is None else v for v, d in zip((open_, extend, match, mismatch), _lib.STAR_SCORING)]
        x = torch.empty((S, 5, 128, 2), dtype=torch.float32, device=self.device)
        mc = int(max_cols)
        cns = np.empty((S, mc), np.uint8)
        ncols = np.empty(S, np.int32)
        ptr = lambda a: _lib.npp(a) if isinstance(a, np.ndarray) else a      # noqa: E731
        rows = rr = roff = rroff = None
        if want_rows:
            roff = np.zeros(S + 1, np.int64)
            np.cumsum(_n_reads * _cap, out=roff[1:])
            rroff = np.zeros(S + 1, np.int64)
            np.cumsum(_cap, out=rroff[1:])
            rows, rr = np.empty(max(int(roff[-1]), 1), np.uint8), np.empty(max(int(rroff[-1]), 1), np.uint8)
        self._check(self.L.nc_star_msa_tensor_dup(self.ctx, S, reads, ptr(read_off), ptr(set_read0), refs, ptr(ref_off),
                                                  int(open_), int(extend), int(match), int(mismatch), mc, _ptr(x), _lib.npp(cns), _lib.npp(ncols),
                                                  _lib.npp(rows), _lib.npp(roff), _lib.npp(rr), _lib.npp(rroff), ptr(al_dup)), "nc_star_msa_tensor")
        if int(ncols.max()) > mc and not want_rows:
            # the caller's column bound was an estimate (consensus columns beyond it are cut): once more with the real maximum
            return self.star_msa_tensor_flat(S, reads, read_off, set_read0, refs, ref_off, int(ncols.max()), open_=open_, extend=extend,
                                             match=match, mismatch=mismatch, cns_as_str=cns_as_str, al_dup=al_dup)
        # consensus with the gap symbols removed
        if cns_as_str:
            # natively (worker threads): the [S, mc] matrix of a contig arm is tens of megabytes, numpy masks over it cost more than the alignments
            cut = np.empty(S + 1, np.int64)
            flat = np.empty(max(S * mc, 1), np.uint8)
            self._check(self.L.nc_consensus_strings(_lib.npp(cns), S, mc, _lib.npp(ncols), _lib.npp(flat), _lib.npp(cut)), "nc_consensus_strings")
            cl = cut.tolist()
            big = flat[:cl[-1]].tobytes().decode("ascii")
            out_cns = [big[a:b] for a, b in zip(cl, cl[1:])]
        else:
            keep = (np.arange(mc, dtype=np.int32)[None, :] < np.minimum(ncols, mc)[:, None]) & (cns != 4)
            cnt = keep.sum(1)
            cut = np.zeros(S + 1, np.int64)
            np.cumsum(cnt, out=cut[1:])
            flat_cns = cns[keep]
            out_cns = [flat_cns[cut[k]:cut[k + 1]] for k in range(S)]
        if not want_rows:
            return x, out_cns, ncols
        out_rows = [rows[roff[s]:roff[s] + int(_n_reads[s]) * int(ncols[s])].reshape(int(_n_reads[s]), int(ncols[s])) for s in range(S)]
        out_rr = [rr[rroff[s]:rroff[s] + int(ncols[s])] for s in range(S)]
        return x, out_cns, ncols, out_rows, out_rr

    def indel_tensor(self, rows_list, ref_rows_list):
        """rows_list[s]: uint8 [n_rows, n_cols] aligned symbols 0..4; ref_rows_list[s]: uint8 [n_cols].
        -> (x f32 [S,5,128,2] device, cns list of uint8 arrays with gaps removed)"""
        S = len(rows_list)
        dev = self.device
        n_rows = np.array([r.shape[0] for r in rows_list], np.int32)
        n_cols = np.array([r.shape[1] for r in rows_list], np.int32)
        row_off = np.zeros(S, np.int64)
        ref_off = np.zeros(S, np.int64)
        if S:
            np.cumsum((n_rows.astype(np.int64) * n_cols)[:-1], out=row_off[1:])
            np.cumsum(n_cols.astype(np.int64)[:-1], out=ref_off[1:])
        max_cols = max(128, int(n_cols.max()) if S else 128)
        rows = np.concatenate([np.ascontiguousarray(r, np.uint8).ravel() for r in rows_list]) if S else np.zeros(1, np.uint8)
        refs = np.concatenate([np.ascontiguousarray(r, np.uint8).ravel() for r in ref_rows_list]) if S else np.zeros(1, np.uint8)
        t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
        d_rows, d_refs, d_ro, d_fo, d_nr, d_nc = t(rows), t(refs), t(row_off), t(ref_off), t(n_rows), t(n_cols)
        x = torch.empty((S, 5, 128, 2), dtype=torch.float32, device=dev)
        cns = torch.empty((S, max_cols), dtype=torch.uint8, device=dev)
        self._check(self.L.nc_indel_tensor(self.ctx, S, _ptr(d_rows), _ptr(d_ro), _ptr(d_nr), _ptr(d_nc), _ptr(d_refs),
                                           _ptr(d_fo), max_cols, _ptr(x), _ptr(cns)), "nc_indel_tensor")
        cns_h = cns.cpu().numpy()
        out = []
        for s in range(S):
            row = cns_h[s, :n_cols[s]]
            out.append(row[row != 4])
        return x, out

    def to_host(self, tensors):
        """Copy device tensors to (cached) pinned host memory with ONE synchronisation; -> list of numpy views
        that own their pinned storage through the returned arrays' base tensors."""
        outs = []
        for t in tensors:
            if t is None:
                outs.append(None)
                continue
            h, h_np = self._pinned.get(t.shape, t.dtype)
            h.copy_(t, non_blocking=True)
            outs.append(h_np)
        torch.cuda.current_stream(self.device).synchronize()
        return outs

    # ------------------------------------------------------------------ copy stream (results drain overlapping compute)
    def _copy_stream(self):
        if getattr(self, "_cstream", None) is None:
            self._cstream = torch.cuda.Stream(device=self.device)
        return self._cstream

    def _copy_stream_ptr(self):
        return C.c_void_p(self._copy_stream().cuda_stream)

    def to_host_async(self, tensors):
        """Enqueue D2H copies of device tensors on the copy stream, ordered after everything already enqueued on the
        compute stream; -> list of numpy views of pinned memory, valid after wait_copies()."""
        cs = self._copy_stream()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        cs.wait_event(ev)
        outs = []
        with torch.cuda.stream(cs):
            for t in tensors:
                if t is None:
                    outs.append(None)
                    continue
                h, h_np = self._pinned.get(t.shape, t.dtype)
                t = t.contiguous()
                # small blocks go by copy kernel, bulk by the copy engine (see nc_d2h_async)
                self._check(self.L.nc_d2h_async(self.ctx, C.c_void_p(cs.cuda_stream), C.c_void_p(h.data_ptr()), C.c_void_p(t.data_ptr()),
                                                t.numel() * t.element_size()), "nc_d2h_async")
                t.record_stream(cs)
                outs.append(h_np)
        return outs

    def copy_event(self):
        """event that completes when the copies enqueued so far on the copy stream are done"""
        ev = torch.cuda.Event()
        ev.record(self._copy_stream())
        return ev

    def wait_copies(self):
        self._copy_stream().synchronize()

    def sync(self):
        torch.cuda.synchronize(self.device)


_engines = {}


def get_engine(device: int = 0) -> Engine:
    if device not in _engines:
        _engines[device] = Engine(device)
    else:
        _engines[device]._adopt_thread()                 # (a thread that meets the engine for the first time is moved to its stream; ctx->stream untouched)
    return _engines[device]


def local_device(devices=None, rank=0) -> int:
    """GPU of this process: one process per GPU.  `devices` (a sequence) is indexed by the local rank; by default the local
    rank itself (LOCAL_RANK from torchrun, else the global rank) modulo the number of visible devices."""
    local = int(os.environ.get("LOCAL_RANK", rank))
    if devices:
        return int(devices[local % len(devices)])
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    return local % n if n > 0 else 0

"""The reference FASTA on the device (csrc/nc_fasta.hip; formats: fasta.py).

The reference reads its FASTA through pysam.FastaFile, plain or bgzip-compressed.  Here a contig's part of the FILE crosses PCIe as it is --
the bytes [offset, offset + span) of a plain file, the covering BGZF members of a bgzipped one -- and everything else happens in HBM:

  file range (page-locked) --H2D, upload stream--> [ .gz: nc_inflate_device + nc_bgzf_crc_device ] --nc_fasta_decode--> letters (as they
  stand) / the scan's reference codes on a pack's tile grid (upper-case AGTC, quirk E4) / the phaser's case-blind codes

`DeviceFasta.contig(chrom)` is the host half: index lookup, file read, upload.  It launches nothing and may run on a worker thread (the callers
pre-fetch the next contigs with it).  The kernels run when the contig is first USED, on the thread that uses it and on the context's stream,
as every other launch of a pass: `scan_codes`, `letters`, `blind_codes`, `host_letters`.  The decoder checks the file against the .fai where
it reads it; a member that does not inflate to its announced size or fails its CRC-32 raises and names the member.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, bgzf, fasta
from .device_bam import DeviceIngestUnavailable
from .engine import get_engine

INFLATE_BATCH = 4096          # members per nc_inflate_device call (256 KB of token workspace each)
LAST_CONTIG = {}              # seconds per stage of the most recent contig (tools/bench_fasta.py reports them)


def wanted(fasta_path, params=None):
    """does this reference take the device route?  A bgzipped file always (where the caller's device route is in play at all); a plain file only
    when asked: params['device_fasta'] truthy, or NC_DEVICE_FASTA=1 when the key is absent"""
    if not isinstance(fasta_path, str) or not fasta_path:
        return False
    if fasta_path.endswith(".gz"):
        return True
    if params is not None and "device_fasta" in params:
        return bool(params["device_fasta"])
    return os.environ.get("NC_DEVICE_FASTA") == "1"


def _oom(e):
    return isinstance(e, (torch.cuda.OutOfMemoryError, MemoryError)) or "out of memory" in str(e).lower() or "hipErrorOutOfMemory" in str(e)


class DeviceContig:
    """One contig of a DeviceFasta: `length`, and on the device `letters`, `blind_codes`, `scan_codes(tile_pos0, n, ga, gb)`."""

    def __init__(self, owner, entry, first, image_len, staged, upload_done, members=None):
        self.owner, self.entry, self.chrom, self.length = owner, entry, entry.name, int(entry.length)
        self.first, self.image_len = int(first), int(image_len)
        self._staged, self._upload_done, self._members = staged, upload_done, members
        self._image = self._letters = self._blind = None

    # ------------------------------------------------------------------ the image in HBM (first use, launching thread)
    def image(self):
        """the uncompressed bytes that hold the contig, in HBM (uint8 [image_len]; the contig's first base at `first`)"""
        if self._image is not None:
            return self._image
        eng = self.owner.eng
        eng.use_torch_stream()
        dev = eng.device
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(self._upload_done)
        for t in self._staged.values():
            t.record_stream(cur)
        try:
            if self._members is None:
                self._image = self._staged["file"][:self.image_len]
            else:
                self._image = self._inflate(eng, dev)
        except (RuntimeError, MemoryError) as e:
            if _oom(e):
                raise DeviceIngestUnavailable("%s, contig %s: %s" % (self.owner.path, self.chrom, str(e).splitlines()[0] if str(e) else type(e).__name__))
            raise
        self._staged = None
        return self._image

    def _inflate(self, eng, dev):
        """the covering members -> the uncompressed bytes (nc_inflate_device + nc_bgzf_crc_device on the context's stream)"""
        m = self._members
        n = int(m["n"])
        raw = torch.empty(self.image_len + 64, dtype=torch.uint8, device=dev)
        timed = self.owner.timed
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        status = bgzf.inflate_members(eng, self._staged["file"], self._staged["m64"], self._staged["m32"], n, raw, INFLATE_BATCH, "fa_tok", ev)
        st = status.cpu().numpy()
        if timed:
            # (with several batches the inflate figure covers the CRCs of all but the last batch as well)
            LAST_CONTIG.update(inflate=ev[0].elapsed_time(ev[1]) * 1e-3, crc=ev[1].elapsed_time(ev[2]) * 1e-3)
        bad = np.flatnonzero(st)
        if bad.size:
            b = int(bad[0])
            why = "fails its CRC-32" if int(st[b]) == 7 else "is not a valid deflate stream of its announced size (status %d)" % int(st[b])
            raise _lib.NanoCallerHipError("%s: the BGZF member at byte %d %s%s" % (self.owner.path, int(m["file_off"][b]), why,
                                                                                   "" if bad.size == 1 else " (and %d more members)" % (bad.size - 1)))
        return raw[:self.image_len]

    def _decode(self, **out):
        e = self.entry
        self.owner.eng.fasta_decode(self.image(), self.first, e.length, e.linebases, e.linewidth, **out)

    # ------------------------------------------------------------------ the three forms
    def _letters_and_blind(self):
        if self._letters is None:
            dev = self.owner.eng.device
            try:
                letters = torch.empty(self.length, dtype=torch.uint8, device=dev)
                blind = torch.empty(self.length, dtype=torch.uint8, device=dev)
            except (RuntimeError, MemoryError) as e:
                if _oom(e):
                    raise DeviceIngestUnavailable("%s, contig %s: %s" % (self.owner.path, self.chrom, str(e).splitlines()[0]))
                raise
            self._decode(letters=letters, blind=blind)
            self._letters, self._blind = letters, blind

    @property
    def letters(self):
        """uint8 [length]: the contig's bytes as they stand, case preserved"""
        self._letters_and_blind()
        return self._letters

    @property
    def blind_codes(self):
        """uint8 [length]: A0 G1 T2 C3 in either case, else 4 (phase._ref_codes)"""
        self._letters_and_blind()
        return self._blind

    def scan_codes(self, tile_pos0, n, ga=1, gb=None, out=None):
        """uint8 [n]: entry p - tile_pos0 = A0 G1 T2 C3 for an upper-case letter at a position p in [ga, gb], 4 everywhere else (DeviceBam._ref_lut's
        rule on the pack's tile grid)"""
        if out is None:
            out = torch.empty(int(n), dtype=torch.uint8, device=self.owner.eng.device)
        self._decode(scan=out[:int(n)], scan_pos0=int(tile_pos0), ga=int(ga), gb=self.length if gb is None else int(gb))
        return out[:int(n)]

    def host_letters(self):
        """the letters on the host: one copy into page-locked memory -> bytes"""
        t = self.letters
        h = torch.empty(self.length, dtype=torch.uint8, pin_memory=True)
        h.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.owner.eng.device).synchronize()
        return h.numpy().tobytes()


class DeviceFasta:
    """One FASTA file (plain + .fai, or bgzipped + .fai [+ .gzi]) for one device.  `contig(chrom)` -> DeviceContig."""

    def __init__(self, path, device=0):
        self.path, self.device = path, device
        self.eng = get_engine(device)
        self.gz = path.endswith(".gz")
        self.timed = False
        if self.gz:
            fasta.check_bgzf(path)
        if not os.path.exists(path + ".fai"):
            if self.gz:
                fasta.fai_entry(path, "")                                # raises with the samtools faidx hint
            raise DeviceIngestUnavailable("%s: no .fai beside it" % path)
        self.file_bytes = os.path.getsize(path)
        self._upload = None
        self._last = None

    def _upload_stream(self):
        if self._upload is None:
            self._upload = torch.cuda.Stream(device=self.eng.device)
        return self._upload

    def contig(self, chrom) -> DeviceContig:
        """host half (no launch: may run on a worker thread): the contig's byte range into page-locked memory and on its way to the device"""
        last = self._last
        if last is not None and last.chrom == chrom:
            return last
        import time
        t0 = time.perf_counter()
        e = fasta.fai_entry(self.path, chrom)
        if e.length < 1:
            raise _lib.NanoCallerHipError("%s: contig %s is empty" % (self.path, chrom))
        members = None
        if self.gz:
            mm = fasta.member_map(self.path)
            _, lo, hi, ubase = mm.covering(e.offset, e.offset + e.span)
        else:
            lo, hi, ubase = e.offset, e.offset + e.span, e.offset
            if hi > self.file_bytes:
                raise _lib.NanoCallerHipError("%s, contig %s: the .fai does not describe this file (the contig ends %d bytes behind it)"
                                              % (self.path, chrom, hi - self.file_bytes))
        n = hi - lo
        try:
            host = torch.empty(n + 64, dtype=torch.uint8, pin_memory=True)
        except (RuntimeError, MemoryError) as ex:
            if _oom(ex):
                raise DeviceIngestUnavailable("%s: %s" % (self.path, str(ex).splitlines()[0] if str(ex) else type(ex).__name__))
            raise
        data = host.numpy()
        data[n:] = 0
        view = memoryview(data)
        fd = os.open(self.path, os.O_RDONLY)
        try:
            o = 0
            while o < n:
                got = os.preadv(fd, [view[o:n]], lo + o)
                if got <= 0:
                    raise _lib.NanoCallerHipError("short read of %s" % self.path)
                o += got
        finally:
            os.close(fd)
        t_read = time.perf_counter() - t0
        hosts = {"file": host}
        image_len = n
        if self.gz:
            coff, clen, isize, _ = fasta.scan_members(data[:n], lo)
            need = e.offset + e.span - ubase                             # uncompressed bytes from the first member's first to the contig's last
            ooff = bgzf.member_table(coff, clen, isize)[1]
            k = int(np.searchsorted(ooff, need, side="left"))           # members that hold them
            if k > coff.size or ooff[min(k, coff.size)] < need:
                raise _lib.NanoCallerHipError("%s ends %d bytes before contig %s does: the .fai does not describe this file"
                                              % (self.path, need - int(ooff[-1]), chrom))
            m64 = torch.empty(2 * k, dtype=torch.int64, pin_memory=True)
            m32 = torch.empty(2 * k, dtype=torch.int32, pin_memory=True)
            m64.numpy()[:k], m64.numpy()[k:] = coff[:k], ooff[:k]
            m32.numpy()[:k], m32.numpy()[k:] = clen[:k], isize[:k]
            hosts.update(m64=m64, m32=m32)
            image_len = int(ooff[k])
            members = dict(n=k, file_off=lo + coff[:k] - 18)
        dev = self.eng.device
        up = self._upload_stream()
        t1 = time.perf_counter()
        try:
            with torch.cuda.stream(up):
                if self.timed:
                    begun = torch.cuda.Event(enable_timing=True)
                    begun.record(up)
                staged = {name: h.to(dev, non_blocking=True) for name, h in hosts.items()}
                done = torch.cuda.Event(enable_timing=self.timed)
                done.record(up)
        except (RuntimeError, MemoryError) as ex:
            if _oom(ex):
                raise DeviceIngestUnavailable("%s: %s" % (self.path, str(ex).splitlines()[0] if str(ex) else type(ex).__name__))
            raise
        c = DeviceContig(self, e, e.offset - ubase, image_len, staged, done, members)
        c._hosts = hosts                                                 # (page-locked sources: alive until the copies are done)
        if self.timed:
            done.synchronize()
            LAST_CONTIG.clear()
            LAST_CONTIG.update(file_read=t_read, h2d=begun.elapsed_time(done) * 1e-3, bytes_read=n, enqueue=time.perf_counter() - t1)
        self._last = c
        return c


_OPEN = {}


def open_device_fasta(path, device=0) -> DeviceFasta:
    """the DeviceFasta of (path, device), cached by path + size + mtime (of the file and its .fai)"""
    st = os.stat(path)
    fai = os.stat(path + ".fai") if os.path.exists(path + ".fai") else None
    key = (os.path.abspath(path), device, st.st_size, st.st_mtime_ns, fai and (fai.st_size, fai.st_mtime_ns))
    if key not in _OPEN:
        for k in [k for k in _OPEN if k[:2] == key[:2]]:
            del _OPEN[k]
        _OPEN[key] = DeviceFasta(path, device)
    return _OPEN[key]


def device_contig(fasta_path, chrom, device=0):
    """DeviceFasta(...).contig(chrom): the form the callers pre-fetch"""
    return open_device_fasta(fasta_path, device).contig(chrom)


def reference_for(fasta_path, chrom, device=0, params=None):
    """what DeviceBam.prepare takes as `ref`: the contig on the device where the reference takes that route (`wanted`), else -- also when page-locked
    or device memory is short -- its letters as bytes from the host readers.  No launch: may run on a worker thread."""
    if wanted(fasta_path, params):
        try:
            return device_contig(fasta_path, chrom, device)
        except DeviceIngestUnavailable:
            pass
    from .bam import read_fasta_bytes
    return read_fasta_bytes(fasta_path, chrom)


def release(path=None):
    """forget the open files (of `path`, or all) and the contigs they hold in HBM"""
    for k in [k for k in _OPEN if path is None or k[0] == os.path.abspath(path)]:
        del _OPEN[k]

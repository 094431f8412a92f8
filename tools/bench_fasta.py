"""What the reference FASTA costs on the from-BAM route, host against device (device_fasta.py, csrc/nc_fasta.hip), on a chr20-sized contig
(64,444,167 bp) and a chr1-sized one (248,956,422 bp), 60-base lines; medians of five, the routes interleaved:

  (a) host        bam.read_fasta_bytes + DeviceBam.prepare's staging of the letters into page-locked memory + their upload + pack()'s torch gather
                  (the unchanged default for a plain file)
  (b) device      DeviceFasta.contig on the plain file (file read, H2D) + scan_codes (k_fasta_decode)
  (c) device .gz  the same on the bgzipped twin, with the stages apart: file read, H2D, inflate, CRC, k_fasta_decode
  (d) host .gz    fasta.read_fasta_bytes on the bgzipped twin (zlib, one thread)

+ k_fasta_decode alone with all three outputs against its 1 + 3 bytes per base, and the wall time of snpCaller.caller from tools/ont_like_bam.py's
BAM with the reference on route (a) and on route (b).  Test tooling: the files are synthetic and written here (the bgzipped twin by the library's
multi-threaded compressor), page cache warm.

    python tools/bench_fasta.py --out profiles/device_fasta.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nanocaller_amd import device_bam, device_fasta, fasta, vcfio  # noqa: E402
from nanocaller_amd.bam import read_fasta_bytes  # noqa: E402
from nanocaller_amd.engine import get_engine  # noqa: E402

TILE = 2048


def write_contig(tmp, name, n, seed, lb=60):
    """a plain FASTA of one contig (random ACGT, soft-masked and N runs) + .fai, and its bgzipped twin + .fai + .gzi"""
    rng = np.random.default_rng(seed)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    for a in rng.integers(0, n, n // 20_000).tolist():
        s[a:a + 300] |= 0x20
    s[:10_000] = ord("N")
    header = (">%s synthetic\n" % name).encode()
    nfull = n // lb
    body = np.empty((nfull, lb + 1), np.uint8)
    body[:, :lb] = s[:nfull * lb].reshape(nfull, lb)
    body[:, lb] = 10
    data = header + body.tobytes() + (s[nfull * lb:].tobytes() + b"\n" if n % lb else b"")
    fa = os.path.join(tmp, name + ".fa")
    with open(fa, "wb") as f:
        f.write(data)
    row = "%s\t%d\t%d\t%d\t%d\n" % (name, n, len(header), lb, lb + 1)
    gz = fa + ".gz"
    coff = np.asarray(vcfio.bgzf_write(gz, data), np.int64)
    for p in (fa, gz):
        with open(p + ".fai", "w") as f:
            f.write(row)
    with open(gz + ".gzi", "wb") as f:                                   # (compressed, uncompressed) offset of every member but the first
        ent = np.stack([coff[1:], np.arange(1, coff.size, dtype=np.int64) * 0xff00], 1)
        ent = ent[ent[:, 1] < len(data)]
        f.write(np.array([ent.shape[0]], "<u8").tobytes() + ent.astype("<u8").tobytes())
    return fa, gz, os.path.getsize(gz)


def host_route(eng, lut, fa, name):
    """(a): what the unchanged route does with a contig's reference on its way into a pack"""
    t0 = time.perf_counter()
    ref = np.frombuffer(read_fasta_bytes(fa, name), np.uint8)
    t1 = time.perf_counter()
    staged = torch.empty(ref.size, dtype=torch.uint8, pin_memory=True)  # prepare(): the letters into the page-locked staging buffer
    staged.numpy()[:] = ref
    t2 = time.perf_counter()
    ref_len = (ref.size + TILE) // TILE * TILE
    d = staged.to(eng.device, non_blocking=True)                         # pack(): upload + gather
    ref_code = torch.full((ref_len,), 4, dtype=torch.uint8, device=eng.device)
    ref_code[0:ref.size] = lut[d.to(torch.int32)]
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return dict(total=t3 - t0, read_fasta_bytes=t1 - t0, staging=t2 - t1, upload_gather=t3 - t2), ref_code


def device_route(eng, path, name, timed=False):
    """(b) / (c)"""
    device_fasta.release()
    fasta.forget()
    t0 = time.perf_counter()
    df = device_fasta.open_device_fasta(path, eng.device.index)
    df.timed = timed
    c = df.contig(name)
    t1 = time.perf_counter()
    ref_len = (c.length + TILE) // TILE * TILE
    c.image()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ref_code = c.scan_codes(1, ref_len, 1, c.length)
    e1.record()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    out = dict(total=t3 - t0, contig_host_half=t1 - t0, image=t2 - t1, scan_codes_call=t3 - t2, k_fasta_scan=e0.elapsed_time(e1) * 1e-3)
    if timed:
        out.update({k: v for k, v in device_fasta.LAST_CONTIG.items()})
    return out, ref_code, c


def med(rows):
    return {k: round(statistics.median(r[k] for r in rows), 5) for k in rows[0]}


def bench_contig(eng, tmp, name, n, seed, reps=5):
    fa, gz, gz_bytes = write_contig(tmp, name, n, seed)
    lut = np.full(256, 4, np.uint8)
    for i, ch in enumerate("AGTC"):
        lut[ord(ch)] = i
    lut = torch.from_numpy(lut).to(eng.device)
    rows = dict(a=[], b=[], c=[], d=[])
    same = True
    host_route(eng, lut, fa, name)                                       # warm: first launches, the page cache, the allocators' pools
    device_route(eng, gz, name)
    for _ in range(reps):
        r, want = host_route(eng, lut, fa, name)
        rows["a"].append(r)
        r, got, _ = device_route(eng, fa, name)
        rows["b"].append(r)
        same = same and torch.equal(got, want)
        r, got, c = device_route(eng, gz, name, timed=True)
        rows["c"].append(r)
        same = same and torch.equal(got, want)
        del got, want
        t0 = time.perf_counter()
        fasta.forget()
        fasta.read_fasta_bytes(gz, name)
        rows["d"].append(dict(total=time.perf_counter() - t0))
    # the kernel alone, all three outputs: 1 byte read + 3 written per base
    letters = torch.empty(n, dtype=torch.uint8, device=eng.device)
    blind = torch.empty(n, dtype=torch.uint8, device=eng.device)
    scan = torch.empty((n + TILE) // TILE * TILE, dtype=torch.uint8, device=eng.device)
    e = c.entry
    ks = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.fasta_decode(c.image(), c.first, e.length, e.linebases, e.linewidth, letters=letters, scan=scan, blind=blind)
        e1.record()
        torch.cuda.synchronize()
        ks.append(e0.elapsed_time(e1) * 1e-3)
    k = statistics.median(ks[1:])
    del letters, blind, scan, c
    device_fasta.release()
    return dict(bases=n, linebases=60, plain_bytes=os.path.getsize(fa), gz_bytes=gz_bytes, outputs_identical=bool(same),
                a_host_plain=med(rows["a"]), b_device_plain=med(rows["b"]), c_device_gz=med(rows["c"]), d_host_gz_zlib=med(rows["d"]),
                k_fasta_decode_all_outputs=dict(seconds=round(k, 6), bytes_per_base="1 read + 3 written (+ the line terminators read)",
                                                gb_s=round(4 * n / k / 1e9, 1)))


def bench_from_bam(eng, n_contigs=2, L=9_000_000):
    """snpCaller.caller from the ONT-like BAM: the reference on the host route (default for a plain file) and on the device route"""
    import queue
    import shutil

    import bamio
    import ont_like_bam
    from nanocaller_amd import generate_SNP_pileups as gsp
    from nanocaller_amd import snpCaller
    from nanocaller_amd.utils import get_chunks
    tmp = tempfile.mkdtemp(prefix="nc_bench_fasta_bam_")
    bam, refs, fa_seqs, _ = ont_like_bam.make_files(eng, tmp, n_contigs, L, depth=30.0, seed0=7000, level=1)
    fa = os.path.join(tmp, "b.fa")
    bamio.write_fasta(fa, fa_seqs[0][0], fa_seqs[0][1], extra=fa_seqs[1:])
    del fa_seqs
    regions = [(n, 1, ln, "diploid") for n, ln in refs]
    base = dict(regions_list=regions, sam_path=bam, fasta_path=fa, mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6],
                snp_model="ONT-HG002", cpu=16, prefix="t", sample="S", seq="ont", supplementary=False, exclude_bed=None, suppress_progress=True,
                disable_coverage_normalization=False)
    times, texts = dict(host=[], device=[]), {}
    for rep in range(6):                                                 # the first run of either route is the warm-up
        for tag in ("host", "device"):
            gsp.release_contig()
            device_bam.release()
            device_fasta.release()
            d = os.path.join(tmp, "%s%d" % (tag, rep))
            os.makedirs(d)
            params = dict(base, chunks_list=get_chunks(regions, 16), vcf_path=d, intermediate_snp_files_dir=d, device_fasta=(tag == "device"))
            q = queue.Queue()
            for c in params["chunks_list"]:
                q.put(c)
            files = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            snpCaller.caller(params, q, queue.Queue(), files, device=eng.device.index)
            torch.cuda.synchronize()
            if rep:
                times[tag].append(time.perf_counter() - t0)
            texts[tag] = open(files[0], "rb").read()
    gsp.release_contig()
    device_bam.release(buffers=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return dict(workload="%d contigs of %d bp, ONT-like 30x BAM (tools/ont_like_bam.py) + plain FASTA -> snpCaller.caller -> worker VCF" % (n_contigs, L),
                a_host_fasta_s=round(statistics.median(times["host"]), 4), b_device_fasta_s=round(statistics.median(times["device"]), 4),
                runs=dict(host=[round(t, 4) for t in times["host"]], device=[round(t, 4) for t in times["device"]]),
                records=texts["host"].count(b"\n"), vcf_identical=texts["host"] == texts["device"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_fasta.json"))
    ap.add_argument("--skip-from-bam", action="store_true")
    ap.add_argument("--skip-chr1", action="store_true")
    a = ap.parse_args()
    eng = get_engine(0)
    eng.use_torch_stream()
    out = dict(device=torch.cuda.get_device_name(0), note="medians of five, routes interleaved, files written moments before (page cache warm)")

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    with tempfile.TemporaryDirectory(prefix="nc_bench_fasta_") as tmp:
        out["chr20_sized"] = bench_contig(eng, tmp, "chr20", 64_444_167, 20)
        print(json.dumps(out["chr20_sized"]), flush=True)
        save()
        if not a.skip_chr1:
            out["chr1_sized"] = bench_contig(eng, tmp, "chr1", 248_956_422, 1)
            print(json.dumps(out["chr1_sized"]), flush=True)
            save()
    device_bam.release(buffers=True)
    if not a.skip_from_bam:
        out["from_bam"] = bench_from_bam(eng)
        print(json.dumps(out["from_bam"]), flush=True)
        save()


if __name__ == "__main__":
    main()

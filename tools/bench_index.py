"""Indexing an unindexed BAM on the GPU (device_bam.build_index, csrc/nc_bamindex.hip) on tools/ont_like_bam.py's file -> profiles/index_build.json

  build_index          wall time of the whole call (file read, H2D, inflate + CRC, chain, fields, D2H, numpy assembly, write) and its device
                       stages by events, .bai and .csi
  chain vs one lane    the record boundaries of one piece of the inflated stream in HBM: nc_bamidx_candidates / _chain / _collect / _verify
                       (bam_index.chain_piece, prefix sums and host synchronisations included) against nc_bam_walk with ONE seed, count pass +
                       fill pass, as the ingest would have to walk the stream without an index; same piece, same output
  snpCaller.caller     on the file WITHOUT index: with params['build_index'] (the index is deleted before every run, so every run builds it)
                       against the host-thread route the callers take without the opt-in, and against the run on the indexed file

Medians over the runs after a warm-up run of each route, routes interleaved; the file was written moments before (page cache warm)."""
import argparse
import ctypes as C
import json
import os
import queue
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch   # noqa: E402

from nanocaller_amd import _lib, bam_index, device_bam   # noqa: E402
from nanocaller_amd.engine import get_engine   # noqa: E402

CHAIN_PIECE = 1 << 30            # bytes of the inflated stream the chain comparison runs on


def _drop_index(bam):
    for ext in (".bai", ".csi"):
        if os.path.exists(bam + ext):
            os.unlink(bam + ext)


def bench_build(bare, reps):
    out = {}
    for fmt in ("bai", "csi"):
        rows = []
        for rep in range(reps + 1):
            _drop_index(bare)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_bam.build_index(bare, fmt=fmt)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if rep:
                rows.append(dict(bam_index.LAST_INDEX, wall_s=wall))
        med = lambda k: round(statistics.median(r[k] for r in rows), 4)   # noqa: E731
        out[fmt] = dict(wall_s=med("wall_s"), inflate_s=med("inflate_s"), chain_s=med("chain_s"), fields_s=med("fields_s"), assemble_s=med("assemble_s"),
                        runs_wall_s=[round(r["wall_s"], 4) for r in rows], pieces=rows[0]["pieces"], serial_pieces=rows[0]["serial_pieces"],
                        members=rows[0]["members"], records=rows[0]["records"], candidates=rows[0]["candidates"], inflated_bytes=rows[0]["inflated_bytes"],
                        index_bytes=os.path.getsize(bare + "." + fmt))
    _drop_index(bare)
    return out


def bench_chain(eng, indexed, reps):
    """one piece of the stream, resident: the parallel chain against the one-seed walk"""
    L, dev = _lib.lib(), eng.device
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    db = device_bam.DeviceBam(indexed, dev.index).load()
    names, lengths, first = bam_index.read_header(indexed)
    n = int(min(db.raw_len, CHAIN_PIECE))
    buf = db.raw[:n + 64]
    d_len = torch.tensor(lengths, dtype=torch.int32, device=dev)
    seed = torch.tensor([first], dtype=torch.int64, device=dev)
    tid = torch.tensor([int(db.meta[0][0])], dtype=torch.int32, device=dev)
    t_chain, t_walk, same = [], [], None
    for rep in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        stats = {}
        e[0].record()
        out, n_rec, carry, st = bam_index.chain_piece(eng, buf, n, first, len(names), d_len, last=False, stats=stats)
        e[1].record()
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        e[2].record()
        eng._check(L.nc_bam_walk(eng.ctx, vp(buf), n, 1, vp(seed), vp(tid), None, vp(cnt), vp(status)), "nc_bam_walk")
        k = int(cnt.item())
        walked = torch.empty(max(1, k), dtype=torch.int64, device=dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        eng._check(L.nc_bam_walk(eng.ctx, vp(buf), n, 1, vp(seed), vp(tid), vp(zero), vp(walked), vp(status)), "nc_bam_walk")
        e[3].record()
        e[3].synchronize()
        if rep:
            t_chain.append(e[0].elapsed_time(e[1]) * 1e-3)
            t_walk.append(e[2].elapsed_time(e[3]) * 1e-3)
        # (the one-seed walk stops where the next contig's records begin; the chain does not)
        same = bool(st == 0 and stats.get("serial_pieces", 0) == 0 and k <= n_rec and torch.equal(out[:k], walked[:k]))
    res = dict(piece_bytes=n, records_chain=n_rec, records_one_seed_walk=k, candidates=stats["candidates"], offsets_identical=same,
               chain_s=round(statistics.median(t_chain), 5), one_seed_walk_s=round(statistics.median(t_walk), 5),
               runs=dict(chain=[round(t, 5) for t in t_chain], one_seed_walk=[round(t, 5) for t in t_walk]))
    res["walk_over_chain"] = round(res["one_seed_walk_s"] / res["chain_s"], 2)
    del db, buf
    device_bam.release(buffers=True)
    return res


def bench_caller(eng, indexed, bare, fa, refs, tmp, reps, host_reps):
    from nanocaller_amd import generate_SNP_pileups as gsp
    from nanocaller_amd import snpCaller
    from nanocaller_amd.utils import get_chunks
    regions = [(n, 1, ln, "diploid") for n, ln in refs]
    base = dict(regions_list=regions, fasta_path=fa, mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6],
                snp_model="ONT-HG002", cpu=16, prefix="t", sample="S", seq="ont", supplementary=False, exclude_bed=None, suppress_progress=True,
                disable_coverage_normalization=False)
    routes = dict(indexed=(indexed, {}, reps), unindexed_build_index=(bare, dict(build_index=True), reps), unindexed_host_route=(bare, {}, host_reps))
    times, texts = {k: [] for k in routes}, {}
    for rep in range(max(reps, host_reps) + 1):
        for tag, (bam, extra, n) in routes.items():
            if rep > n:
                continue
            gsp.release_contig()
            device_bam.release()
            _drop_index(bare)
            d = os.path.join(tmp, "%s%d" % (tag, rep))
            os.makedirs(d)
            params = dict(base, sam_path=bam, chunks_list=get_chunks(regions, 16), vcf_path=d, intermediate_snp_files_dir=d, **extra)
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
            shutil.rmtree(d, ignore_errors=True)
    gsp.release_contig()
    device_bam.release(buffers=True)
    _drop_index(bare)
    sites = sum(1 for ln in texts["indexed"].split(b"\n") if ln and not ln.startswith(b"#"))
    out = dict(reference_bases=sum(ln for _, ln in refs), candidate_sites=sites, vcf_identical=len(set(texts.values())) == 1)
    for tag in routes:
        s = statistics.median(times[tag])
        out[tag] = dict(seconds=round(s, 4), m_candidate_sites_s=round(sites / s / 1e6, 3), runs=[round(t, 4) for t in times[tag]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build.json"))
    ap.add_argument("--contigs", type=int, default=2)
    ap.add_argument("--length", type=int, default=9_000_000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=1, help="timed runs of the host-thread route (each takes about a minute at the default size)")
    a = ap.parse_args()
    import bamio
    import ont_like_bam
    eng = get_engine(0)
    eng.use_torch_stream()
    tmp = tempfile.mkdtemp(prefix="nc_bench_index_")
    indexed, refs, fa_seqs, fstats = ont_like_bam.make_files(eng, tmp, a.contigs, a.length, depth=30.0, seed0=7000, level=1)
    fa = os.path.join(tmp, "b.fa")
    bamio.write_fasta(fa, fa_seqs[0][0], fa_seqs[0][1], extra=fa_seqs[1:])
    del fa_seqs
    bare = os.path.join(tmp, "bare.bam")
    os.link(indexed, bare)                                               # the same file under a name that has no index beside it
    out = dict(device=torch.cuda.get_device_name(0), workload="%d contigs of %d bp, ONT-like 30x BAM (tools/ont_like_bam.py), %d bytes, %d reads"
               % (a.contigs, a.length, fstats["bam_bytes"], fstats["reads"]), note=__doc__.strip().splitlines()[-1])

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    try:
        out["build_index"] = bench_build(bare, a.reps)
        print(json.dumps(out["build_index"]), flush=True)
        save()
        out["chain_vs_one_seed_walk"] = bench_chain(eng, indexed, a.reps)
        print(json.dumps(out["chain_vs_one_seed_walk"]), flush=True)
        save()
        out["snp_caller"] = bench_caller(eng, indexed, bare, fa, refs, tmp, a.reps, a.host_reps)
        print(json.dumps(out["snp_caller"]), flush=True)
        save()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

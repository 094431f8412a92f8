#!/usr/bin/env python3
"""Cost of the gVCF's reference-confidence blocks (csrc/nc_refconf.hip) on the chr20-sized synthetic contig bench.py uses, and bench.py's headline
on this build against the parent commit with the option off.

    python tools/bench_gvcf.py [--parent DIR] [--pairs K] [--length L] [--reps N] [--out profiles/gvcf.json]

In one process, on an HBM-resident pack, device events around each step, the device drained between repetitions:

    scan            k_scan (timer 0 of the library), the plain scan of this build
    columns         nc_refconf_columns on the same pack: it streams the same bytes and counts two planes instead of five
    blocks          nc_refconf_blocks + nc_refconf_fetch into device memory (a host clock: the call waits for the count), default bands, no cuts
    text            nc_refconf_text, both calls (offsets, then bytes), and the copy of the text to the host, each on its own
    blocks_per_column, text_bytes

--parent DIR: a built checkout of the parent commit.  bench.py --gpus 1 --steps S --warmup W runs in a fresh child process for this build and for
the parent, K pairs, alternating; `headline_by_process` holds every process's value in the order run, so that the two builds are compared against
the parent's own run-to-run spread.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p90_ms=float(a[(9 * len(a)) // 10]), reps=int(a.size))


def steps(args):
    import numpy as np
    import torch
    from nanocaller_amd import gvcf
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_device_workload
    from nanocaller_amd.utils import get_chunks
    eng = get_engine(0)
    L = args.length
    pack, info = make_device_workload(eng, L, depth=30.0, tech="ont", seed=4811)
    spans = [(c["start"], c["end"]) for c in get_chunks([("chr20", 1, L, "diploid")], cpu=16)]
    kw = dict(error=gvcf.DEFAULT_ERROR, bands=list(gvcf.DEFAULT_GQ_BANDS))
    out = {"workload": "chr20-sized synthetic ONT 30x contig (bench.py's), %d bp, pack resident in HBM" % L, "pileup_entries": int(info["pileup_entries"])}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return r, a.elapsed_time(b)

    scan, cols, blocks, text_off, text_bytes, text_copy = [], [], [], [], [], []
    eng.enable_timing(True)
    for i in range(args.warmup + args.reps):
        eng.snp_scan(pack, spans, mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])
        eng.sync()
        held, ms_c = events(lambda: eng.refconf_columns(pack))
        words, ref_code, pos0 = held
        t0 = time.perf_counter()
        blk = eng.refconf_blocks(words, pos0, spans, None, device_out=True, **kw)
        ms_b = (time.perf_counter() - t0) * 1e3
        prm = eng._refconf_params(kw["error"], None, False)
        import ctypes as C
        n = int(blk.shape[0])
        off = torch.empty(n + 1, dtype=torch.int64, device=eng.device)
        nbytes = C.c_int64()
        a = (eng.ctx, n, C.c_void_p(blk.data_ptr()), C.c_void_p(ref_code.data_ptr()), int(pos0), int(ref_code.numel()), b"chr20", C.byref(prm), C.c_void_p(off.data_ptr()))
        t0 = time.perf_counter()
        eng._check(eng.L.nc_refconf_text(*a, None, 0, C.byref(nbytes)), "nc_refconf_text")
        ms_o = (time.perf_counter() - t0) * 1e3
        txt = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=eng.device)
        t0 = time.perf_counter()
        eng._check(eng.L.nc_refconf_text(*a, C.c_void_p(txt.data_ptr()), int(nbytes.value), None), "nc_refconf_text")
        ms_t = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = txt.cpu()
        ms_h = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            scan.append(eng.last_ms(0)); cols.append(ms_c); blocks.append(ms_b); text_off.append(ms_o); text_bytes.append(ms_t); text_copy.append(ms_h)
        out.update(n_blocks=n, columns=int(words.numel()), blocks_per_column=n / float(L), text_bytes=int(nbytes.value))
        del held, words, ref_code, blk, off, txt, host
    eng.enable_timing(False)
    out.update(scan=stats(scan), columns_kernel=stats(cols), blocks=stats(blocks), text_offsets=stats(text_off), text_write=stats(text_bytes),
               text_to_host=stats(text_copy))
    out["columns_over_scan"] = out["columns_kernel"]["median_ms"] / out["scan"]["median_ms"]
    return out


def headline(tree, args):
    env = dict(os.environ, PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("NC_GVCF", None)
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.bench_warmup)],
                       env=env, cwd=tree, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    if p.returncode != 0:
        raise SystemExit("bench.py (%s) failed with status %d" % (tree, p.returncode))
    return float(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])["value"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent", help="a built checkout of the parent commit (bench.py's headline is measured on both builds)")
    ap.add_argument("--pairs", type=int, default=3, help="with --parent: pairs of bench.py processes (parent, this build), alternating")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gvcf.json"))
    ap.add_argument("--steps-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps_child:
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(steps(args)), flush=True)
        return
    # the steps in a child of their own: one process holds the GPU at a time
    cmd = [sys.executable, os.path.abspath(__file__), "--steps-child", "--length", str(args.length), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    if p.returncode != 0:
        raise SystemExit("the steps' child failed with status %d" % p.returncode)
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    if args.parent:
        by = {"parent": [], "this": []}
        for _ in range(args.pairs):
            by["parent"].append(headline(os.path.abspath(args.parent), args))
            by["this"].append(headline(ROOT, args))
            print("headline so far", by, file=sys.stderr, flush=True)
        res["headline_by_process"] = dict(by, what="bench.py --gpus 1 --steps %d --warmup %d, sites/s of each process in the order run, gvcf off" % (args.steps, args.bench_warmup))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

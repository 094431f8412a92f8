#!/usr/bin/env python3
"""What the uniform sample above maxcov (nc_set_downsample) costs and what it changes.

    python tools/bench_downsample.py [--length L] [--reps N] [--out profiles/downsample.json]

On one GPU, on HBM-resident synthetic packs, by the library's stage timers (HIP events around the kernels):

    snp_30x      nc_snp_featurize (timer 1) on the chr20-sized 30x contig bench.py uses, option off against on.  Nothing exceeds maxcov = 160 there:
                 the difference is the price of the sampled form where it samples nothing.
    indel_30x    the indel plan + run (nc_indel_sites_plan + _run, host clock around the call and the wait for the device: the pipeline has no
                 single stage timer) on the 30x indel workload, option off against on.
    snp_deep     nc_snp_featurize on an amplicon-like contig of 20 kb at 2,000x, first against uniform: every site draws a sample (the counting pass,
                 the radix select over ~2,000 keys, the membership tests).
    bias         on that deep contig, per policy: the mean number of neighbour columns left and right of the site that a sampled read covers, read off
                 the tensors (a read counts at a column where it has a base: the column's four base counts over the four centre-base rows), and the
                 mean number of neighbour columns a site has on either side.  The first maxcov reads in coordinate order are those that start
                 furthest left: their right side is the short one.

The select alone (nc_sample_threshold at n = 10^3 .. 10^5) has no entry point of its own and is not timed here; snp_deep holds it at n ~ 2,000.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(a[len(a) // 10]), p90_ms=float(a[(9 * len(a)) // 10]), reps=int(a.size))


def coverage_sides(x):
    """x int16 [N, 5, 41, 5] -> (mean neighbour columns a sampled read covers left, right; mean neighbour columns present left, right)"""
    import torch
    c = x[:, 1:, :, :4].abs().to(torch.int64).sum(dim=(1, 3))            # [N, 41]: reads with a base at the column
    ns = c[:, 20].clamp(min=1).to(torch.float64)
    present = x[:, 0, :, :4].abs().sum(dim=2) > 0                         # the column has a reference one-hot: it exists
    left, right = c[:, :20].sum(dim=1).to(torch.float64) / ns, c[:, 21:].sum(dim=1).to(torch.float64) / ns
    return (float(left.mean()), float(right.mean()), float(present[:, :20].sum(dim=1).double().mean()), float(present[:, 21:].sum(dim=1).double().mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=812)
    ap.add_argument("--skip-indel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downsample.json"))
    a = ap.parse_args()
    import torch
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_device_workload, make_indel_device_workload
    from nanocaller_amd.utils import get_chunks
    eng = get_engine(0)
    eng.enable_timing(True)
    out = dict(device=torch.cuda.get_device_name(0), length=a.length, maxcov=160, seed=a.seed)
    skw = dict(mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])

    def featurize(pack, spans, label, modes):
        sites = eng.snp_scan(pack, spans, **skw)
        res = {}
        for name, down in modes:
            ms = []
            for i in range(a.warmup + a.reps):
                eng.snp_featurize(pack, sites, seq="ont", maxcov=160, int16=True, downsample=down)
                eng.sync()
                if i >= a.warmup:
                    ms.append(eng.last_ms(1))
            res[name] = dict(stats(ms), sites=int(sites.n_sites), mean_site_depth=float(sites.depth.double().mean()))
            if label == "snp_deep":
                cl, cr, pl, pr = coverage_sides(sites.x)
                res[name].update(read_covers_left=cl, read_covers_right=cr, columns_left=pl, columns_right=pr)
            print(label, name, res[name], flush=True)
        out[label] = res

    L = a.length
    pack, _ = make_device_workload(eng, L, depth=30.0, tech="ont", seed=4811)
    spans = [(c["start"], c["end"]) for c in get_chunks([("chr20", 1, L, "diploid")], cpu=16)]
    featurize(pack, spans, "snp_30x", [("off", None), ("on", ("uniform", a.seed)), ("off_again", None)])
    del pack
    torch.cuda.empty_cache()
    deep, _ = make_device_workload(eng, 20_000, depth=2000.0, tech="ont", seed=4812)
    featurize(deep, [(1, 20_000)], "snp_deep", [("first", None), ("uniform", ("uniform", a.seed))])
    del deep
    torch.cuda.empty_cache()
    if not a.skip_indel:
        Li = min(L, 10_000_000)
        ipack, reads_c, _ = make_indel_device_workload(eng, Li, depth=28.0, seed=31)
        chunks = [(s, min(Li, s + 100_000)) for s in range(1, Li, 100_000)]
        res = {}
        for name, down in (("off", None), ("on", ("uniform", a.seed)), ("off_again", None)):
            ms = []
            for i in range(a.warmup + a.reps):
                eng.sync()
                t0 = time.perf_counter()
                r = gip.indel_sites_device(eng, ipack, reads_c, Li, chunks, mincov=4, maxcov=160, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6,
                                           window_after=160, fetch=False, downsample=down)
                eng.sync()
                if i >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            res[name] = dict(stats(ms), sites=int(r["n"]), length=Li)
            print("indel_30x", name, res[name], flush=True)
        out["indel_30x"] = res
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of genotyping a given list of indel sites (nc_indel_set_sites) on the chr20-sized synthetic indel workload resident in HBM.

    python tools/bench_genotype_indel.py [--parent DIR] [--alternate K] [--length L] [--reps N] [--out profiles/genotype_indel_sites.json]

nc_indel_sites_stage_ms of every pass (timing mode: HIP events around the stages, one stream): the plan stage (K7, k_listed, anchors, read sets)
and the whole pass (the six stages summed), 40 passes after 8 warm-up ones, median and p10-p90:

    plain                      this build without a list (the launches of the parent commit)
    parent_plain               the parent commit, plain: DIR is a built checkout of it (--parent), measured by the same child code
    add_1e3 / _1e4 / _1e5      add mode with that many random columns of the contig listed (every fourth of the long class)
    only_1e3 / _1e4 / _1e5     only mode with the same lists

Every configuration set runs in a fresh child process of this script (one GPU process at a time), the parent's with DIR first on the module
path.  --alternate K: K more (parent, this build) pairs of processes that time the plain pass alone.  The plain pass launches the kernels the
parent launches, so the two builds may differ by run-to-run spread only: `plain_check` says whether the p10-p90 ranges of the two builds'
processes overlap (plan stage and whole pass), and the exit status is 1 when they do not.  The listed runs report their cost; nothing is
demanded of them.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(a[len(a) // 10]), p90_ms=float(a[(9 * len(a)) // 10]), reps=int(a.size))


def child(args):
    import numpy as np
    import torch
    from nanocaller_amd import _lib
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_indel_device_workload
    eng = get_engine(0)
    L = args.length
    pack, reads_c, info = make_indel_device_workload(eng, L, depth=30.0, seed=812)
    chunks = [(s, min(L, s + 100_000)) for s in range(1, L, 100_000)]
    kw = dict(mincov=4, maxcov=160, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6, window_after=160)
    rng = np.random.Generator(np.random.PCG64(17))
    out = {}

    def timed(label, **skw):
        eng.enable_timing(True)
        plan, whole, n, forced = [], [], 0, None
        ms = np.zeros(6, np.float32)
        for i in range(args.warmup + args.reps):
            last = i == args.warmup + args.reps - 1
            r = gip.indel_sites_device(eng, pack, reads_c, L, chunks, fetch=last and bool(skw), **kw, **skw)
            torch.cuda.synchronize()
            eng.L.nc_indel_sites_stage_ms(eng.ctx, _lib.npp(ms), None)
            if i >= args.warmup:
                plan.append(float(ms[0]))
                whole.append(float(ms.sum()))
            n = r["n"]
            if "src" in r:
                forced = int((r["src"] > 0).sum())
        eng.enable_timing(False)
        out[label] = dict(plan=stats(plan), whole=stats(whole), sites=int(n))
        if forced is not None:
            out[label]["sites_from_listed_columns"] = forced
        print(label, out[label], file=sys.stderr, flush=True)

    timed("plain")
    if not args.plain_only:
        for n in (1_000, 10_000, 100_000):
            p = np.unique(rng.integers(1, L + 1, size=n)).astype(np.int32)
            t_pos = torch.from_numpy(p).to(eng.device)
            t_long = torch.from_numpy((p % 4 == 0).astype(np.uint8)).to(eng.device)
            timed("add_1e%d" % round(np.log10(n)), sites=t_pos, sites_long=t_long)
            timed("only_1e%d" % round(np.log10(n)), sites=t_pos, sites_long=t_long, sites_only=True)
        timed("plain_again")                                          # the plain pass once more, last: drift over the run
    out["workload"] = dict(reads=int(info["n_reads"]), events=int(info["n_events"]), chunks=len(chunks), tile_size=int(pack.tile_size))
    out["device"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(tree, args, plain_only):
    env = dict(os.environ, PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--length", str(args.length), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd + (["--plain-only"] if plain_only else []), env=env, cwd=tree, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    if p.returncode != 0:
        raise SystemExit("child (%s) failed with status %d" % (tree, p.returncode))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def overlap(a, b, key):
    """the p10-p90 ranges of two lists of per-process stats overlap"""
    lo_a, hi_a = min(s[key]["p10_ms"] for s in a), max(s[key]["p90_ms"] for s in a)
    lo_b, hi_b = min(s[key]["p10_ms"] for s in b), max(s[key]["p90_ms"] for s in b)
    return dict(parent=[lo_a, hi_a], this=[lo_b, hi_b], overlap=bool(lo_a <= hi_b and lo_b <= hi_a))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent", help="a built checkout of the parent commit (its plain pass is measured too)")
    ap.add_argument("--alternate", type=int, default=2, help="with --parent: this many more (parent, this build) pairs of plain-pass processes")
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genotype_indel_sites.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.getcwd())
        return child(args)
    res = {"what": "chr20-sized synthetic ONT 30x indel workload, %d bp in 100 kb chunks, resident in HBM; nc_indel_sites_stage_ms per pass "
                       "(timing mode, stages on one stream), %d passes after %d warm-up ones" % (args.length, args.reps, args.warmup),
           "length": args.length, "passes": args.reps, "warmup": args.warmup}
    parent, this = [], []
    if args.parent:
        parent.append(run_child(os.path.abspath(args.parent), args, True)["plain"])
        res["parent_plain"] = parent[0]
    full = run_child(ROOT, args, False)
    res.update(full)
    this.append(full["plain"])
    if args.parent:
        for _ in range(args.alternate):                               # processes of the two builds in turn: the order does not decide
            parent.append(run_child(os.path.abspath(args.parent), args, True)["plain"])
            this.append(run_child(ROOT, args, True)["plain"])
        res["plain_by_process"] = dict(parent=parent, this=this, what="the plain pass of each process, in the order run (parent, this, parent, ...)")
        res["plain_check"] = dict(plan=overlap(parent, this, "plan"), whole=overlap(parent, this, "whole"),
                                  what="p10-p90 of the plain pass over the processes of either build; passes when the ranges overlap")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if args.parent and not (res["plain_check"]["plan"]["overlap"] and res["plain_check"]["whole"]["overlap"]):
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

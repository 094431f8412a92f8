#!/usr/bin/env python3
"""Scan time with listed neighbour sites and background sampling (nc_snp_scan_set_nbr_sites, nc_snp_scan_set_sampling) on the chr20-sized
synthetic contig bench.py uses.

    python tools/bench_neighbors.py [--parent DIR] [--alternate K] [--length L] [--reps N] [--out profiles/neighbor_sites.json]

Timer 0 of the library (nc_last_kernel_ms: HIP events around the scan kernel; with a list also around the bitmap's memset and k_site_bits) on an
HBM-resident pack, one scan per repetition, the device drained between repetitions:

    plain                          the plain scan of this build (k_scan<.., false, false>)
    parent_plain                   the plain scan of the parent commit: DIR is a built checkout of it (--parent), measured by the same child code
    nbr_1e3 / nbr_1e5 / nbr_1e6    the opt-in form, k_scan<.., false, true>, with 10^3 / 10^5 / 10^6 random positions as listed neighbours (add mode)
    sample_1e4 / sample_1e6        ... with a sampling table that keeps about 10^4 / 10^6 columns under the candidate threshold (one probability
                                   in every bin: the count over the contig's length)
    both_1e5_1e6                   ... with 10^5 listed neighbours and the 10^6 table
    genotype_listed_1e5            k_scan<.., true, false>, the known-sites form, with 10^5 positions: what the new form is compared with
    plain_again                    the plain scan once more, last: drift over the run

Every configuration runs in a fresh child process of this script (one GPU process at a time), the parent's with DIR first on the module path.
--alternate K: after that, K more pairs of processes (parent, this build) that time the plain scan alone -- the medians of one process lie closer
together than those of two processes of the same build, so the two builds are compared over processes (`plain_by_process`).
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
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_device_workload
    from nanocaller_amd.utils import get_chunks
    eng = get_engine(0)
    L = args.length
    pack, info = make_device_workload(eng, L, depth=30.0, tech="ont", seed=4811)
    chunks = get_chunks([("chr20", 1, L, "diploid")], cpu=16)
    spans = [(c["start"], c["end"]) for c in chunks]
    kw = dict(mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])
    rng = np.random.Generator(np.random.PCG64(11))
    out = {}

    def timed(label, **skw):
        eng.enable_timing(True)
        ms, n, nb = [], 0, 0
        for i in range(args.warmup + args.reps):
            s = eng.snp_scan(pack, spans, **kw, **skw)
            eng.sync()
            if i >= args.warmup:
                ms.append(eng.last_ms(0))
            n, nb = s.n_sites, s.n_nbr
        eng.enable_timing(False)
        out[label] = dict(stats(ms), sites_emitted=int(n), neighbours=int(nb))
        print(label, out[label], file=sys.stderr, flush=True)

    def positions(n):
        return torch.from_numpy(rng.integers(1, L + 1, size=n).astype(np.int32)).to(eng.device)

    def table(count):
        return (17, [min(0.5, count / L)] * 6)

    timed("plain")
    if not args.plain_only:
        for label, n in (("nbr_1e3", 1_000), ("nbr_1e5", 100_000), ("nbr_1e6", 1_000_000)):
            timed(label, nbr_sites=positions(n))
        timed("sample_1e4", sample=table(1e4))
        timed("sample_1e6", sample=table(1e6))
        timed("both_1e5_1e6", nbr_sites=positions(100_000), sample=table(1e6))
        timed("genotype_listed_1e5", sites=positions(100_000))
        timed("plain_again")
    out["pileup_entries"] = int(info["pileup_entries"])
    out["tiles"] = dict(tile_size=int(pack.tile_size), n_tiles=int(pack.n_tiles), bitmap_bytes=int(pack.n_tiles) * int(pack.tile_size) // 8)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(tree, args, plain_only):
    env = dict(os.environ, PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--length", str(args.length), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd + (["--plain-only"] if plain_only else []), env=env, cwd=tree, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    if p.returncode != 0:
        raise SystemExit("child (%s) failed with status %d" % (tree, p.returncode))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent", help="a built checkout of the parent commit (its plain scan is measured too)")
    ap.add_argument("--alternate", type=int, default=0, help="with --parent: this many more (parent, this build) pairs of plain-scan processes")
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_sites.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.getcwd())
        return child(args)
    res = {"workload": "chr20-sized synthetic ONT 30x contig (bench.py's), %d bp, pack resident in HBM; timer 0 per scan" % args.length}
    if args.parent:
        res["parent_plain"] = run_child(os.path.abspath(args.parent), args, True)["plain"]
    res.update(run_child(ROOT, args, False))
    if args.parent:                                                   # once more after this build's run: the order of the two does not decide
        res["parent_plain_after"] = run_child(os.path.abspath(args.parent), args, True)["plain"]
    if args.parent and args.alternate:
        by = {"parent": [res["parent_plain"]["median_ms"], res["parent_plain_after"]["median_ms"]], "this": [res["plain"]["median_ms"]]}
        for _ in range(args.alternate):
            by["parent"].append(run_child(os.path.abspath(args.parent), args, True)["plain"]["median_ms"])
            by["this"].append(run_child(ROOT, args, True)["plain"]["median_ms"])
        res["plain_by_process"] = dict(by, what="median scan ms of each process, in the order run")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Step times of the haploid SNP and indel trainers (csrc/nc_train_hap.hip, csrc/nc_train_hap_indel.hip) and the float32 noise figures their
tests' bounds are made of.

    python tools/bench_train_haploid.py [--batches 1024 4096] [--indel_batches 256 1024] [--reps 40] [--warmup 8] [--out profiles/haploid_train.json]
    python tools/bench_train_haploid.py --noise  # CPU only: the float32-against-float64 table of tests/hap_train_ref.py

Per batch size, on random integer tensors (-8..8) and the shipped CHM13 weights, timed as tools/bench_train.py times the diploid trainer (its
`timed`: HIP events on the engine's stream around each call, one call per repetition, the device drained between repetitions; median, min,
10th and 90th percentile):

    step, loss_grad, forward_exact, forward_split_precision, stages_median_ms, workspace_bytes_per_site     as in tools/bench_train.py
    diploid_same_session    tools/bench_train.py's own measurement of SnpTrainer at the same batch, taken in this process right after
    step_over_diploid_step  the ratio of the two medians

The haploid indel trainer (indel_batch_N) is measured the same way on tests/hap_indel_train_ref.py's pipeline-like tensors, beside
tools/bench_train_indel.py's measurement of the diploid indel trainer in the same process.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_train  # noqa: E402
import bench_train_indel  # noqa: E402


def noise_table():
    """the float32 restatement against the float64 one on the tests' inputs: {case: largest per-tensor error, largest loss error, bound}"""
    import hap_train_ref as R
    out = {}
    for wn in R.WEIGHT_SETS:
        for case in R.SIZES + ("17s",):
            g, l = R.measure_noise(wn, case)
            out["grad %s n=%s" % (wn, case)] = dict(tensor_err=g, loss_err=l, bound=R.grad_bound(wn, case))
        out["trajectory %s, 5 steps n=64" % wn] = dict(tensor_err=R.measure_traj_noise(wn), bound=R.traj_bound(wn))
        out["forward %s n=300" % wn] = dict(tensor_err=R.measure_forward_noise(wn), bound=R.forward_bound(wn))
    I = R.indel
    for wn in I.WEIGHT_SETS:
        for n in I.SIZES:
            g, l = I.measure_noise(wn, n)
            out["indel grad %s n=%s" % (wn, n)] = dict(tensor_err=g, loss_err=l, bound=I.grad_bound(wn, n))
        out["indel trajectory %s, 5 steps n=64" % wn] = dict(tensor_err=I.measure_traj_noise(wn), bound=I.traj_bound(wn))
        out["indel forward %s n=130" % wn] = dict(tensor_err=I.measure_forward_noise(wn), bound=I.forward_bound(wn))
    return out


def bench(args):
    import numpy as np
    import torch
    from nanocaller_amd import _lib
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.train_haploid import HaploidSnpTrainer
    from nanocaller_amd.weights import Weights, get_SNP_model
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_SNP_HAP, Weights(get_SNP_model("haploid")[0]))
    res = {}
    for n in args.batches:
        rng = np.random.default_rng(n)
        x = torch.from_numpy(rng.integers(-8, 9, (n, 5, 41, 5)).astype(np.float32)).to(eng.device)
        ref = torch.from_numpy((np.arange(n) % 4).astype(np.int32)).to(eng.device)
        lab = torch.from_numpy(rng.integers(0, 4, n).astype(np.uint8)).to(eng.device)
        tr = HaploidSnpTrainer(0, "haploid", lr=1e-6, max_batch=n)
        mask = tr.draw_mask(n)
        r = dict(step=bench_train.timed(lambda: tr.step(x, ref, lab, mask=mask), args.reps, args.warmup),
                 loss_grad=bench_train.timed(lambda: tr.loss_grad(x, ref, lab, mask, 0.5, want_grad=False), args.reps, args.warmup))
        with eng._snp_state(exact_fp32=True):
            r["forward_exact"] = bench_train.timed(lambda: eng.snp_forward(_lib.MODEL_SNP_HAP, x, ref, None), args.reps, args.warmup)
        r["forward_split_precision"] = bench_train.timed(lambda: eng.snp_forward(_lib.MODEL_SNP_HAP, x, ref, None), args.reps, args.warmup)
        tr.stage_ms(True)
        rows = []
        for _ in range(args.reps):
            tr.loss_grad(x, ref, lab, mask, 0.5, want_grad=False)
            rows.append(tr.stage_ms(True))
        tr.stage_ms(False)
        r["stages_median_ms"] = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
        info = tr.info()
        r["workspace_bytes_per_site"] = info["workspace_bytes"] / info["slice_sites"]
        r["step_over_forward_exact"] = r["step"]["median_ms"] / r["forward_exact"]["median_ms"]
        r["sites_per_s"] = n / r["step"]["median_ms"] * 1e3
        res["snp_batch_%d" % n] = r
        print("haploid SNP batch", n, json.dumps(r), file=sys.stderr, flush=True)
        tr.close()
    dip = bench_train.bench(args)                                       # the diploid trainer, same process, same batches
    for n in args.batches:
        r, d = res["snp_batch_%d" % n], dip["batch_%d" % n]
        r["diploid_same_session"] = dict(step=d["step"], loss_grad=d["loss_grad"], stages_median_ms=d["stages_median_ms"])
        r["step_over_diploid_step"] = r["step"]["median_ms"] / d["step"]["median_ms"]
    return res


def bench_indel(args):
    import hap_indel_train_ref as I
    import numpy as np
    import torch
    from nanocaller_amd import _lib
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.train_haploid import HaploidIndelTrainer
    from nanocaller_amd.weights import Weights, get_indel_model
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_INDEL_HAP, Weights(get_indel_model("haploid")))
    timed = bench_train.timed
    res = {}
    for n in args.indel_batches:
        x, lab, _ = I.make_inputs(n)
        x, lab = torch.from_numpy(x).to(eng.device), torch.from_numpy(lab).to(eng.device)
        tr = HaploidIndelTrainer(0, "haploid", lr=1e-6, max_batch=n)
        mask = tr.draw_mask(n)
        r = dict(step=timed(lambda: tr.step(x, lab, mask=mask), args.reps, args.warmup),
                 loss_grad=timed(lambda: tr.loss_grad(x, lab, mask, 0.5, want_grad=False), args.reps, args.warmup))
        with eng._snp_state(exact_fp32=True):
            r["forward_exact"] = timed(lambda: eng.indel_forward(_lib.MODEL_INDEL_HAP, x), args.reps, args.warmup)
        r["forward_split_precision"] = timed(lambda: eng.indel_forward(_lib.MODEL_INDEL_HAP, x), args.reps, args.warmup)
        tr.stage_ms(True)
        rows = []
        for _ in range(args.reps):
            tr.loss_grad(x, lab, mask, 0.5, want_grad=False)
            rows.append(tr.stage_ms(True))
        tr.stage_ms(False)
        r["stages_median_ms"] = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
        info = tr.info()
        r["workspace_bytes_per_site"] = info["workspace_bytes"] / info["slice_sites"]
        r["step_over_forward_exact"] = r["step"]["median_ms"] / r["forward_exact"]["median_ms"]
        r["sites_per_s"] = n / r["step"]["median_ms"] * 1e3
        res["indel_batch_%d" % n] = r
        print("haploid indel batch", n, json.dumps(r), file=sys.stderr, flush=True)
        tr.close()
    if args.no_diploid:
        return res
    dargs = argparse.Namespace(batches=args.indel_batches, reps=args.reps, warmup=args.warmup)
    dip = bench_train_indel.bench(dargs)                                # the diploid indel trainer, same process, same batches
    for n in args.indel_batches:
        r, d = res["indel_batch_%d" % n], dip["batch_%d" % n]
        r["diploid_same_session"] = dict(step=d["step"], loss_grad=d["loss_grad"], stages_median_ms=d["stages_median_ms"])
        r["step_over_diploid_step"] = r["step"]["median_ms"] / d["step"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--indel_batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--only_indel", action="store_true", help="the haploid indel trainer alone (with --no_diploid: without the diploid one beside it)")
    ap.add_argument("--no_diploid", action="store_true")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--noise", action="store_true", help="CPU only: print the float32 noise table and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haploid_train.json"))
    args = ap.parse_args()
    noise = noise_table()
    if args.noise:
        for k, v in noise.items():
            print("%-40s %.2e  losses %s  bound %.1e" % (k, v["tensor_err"], "%.2e" % v["loss_err"] if "loss_err" in v else "-", v["bound"]))
        return
    res = {"workload": "SNP: random integer tensors in -8..8, shipped CHM13 haploid SNP weights; indel: pipeline-like tensors of "
                       "tests/hap_indel_train_ref.py, shipped CHM13 haploid indel weights; keep 0.5; HIP events around one call, 1x MI355X; the "
                       "diploid figures are tools/bench_train.py's / bench_train_indel.py's measurement in the same process",
           "float32_noise": noise}
    if not args.only_indel:
        res.update(bench(args))
    res.update(bench_indel(args))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "float32_noise"}))


if __name__ == "__main__":
    main()

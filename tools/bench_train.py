#!/usr/bin/env python3
"""Step time of the SNP trainer (csrc/nc_train.hip) and the float32 noise figures its tests' bounds are made of.

    python tools/bench_train.py [--batches 1024 4096] [--reps 40] [--warmup 8] [--out profiles/snp_train.json]
    python tools/bench_train.py --noise          # CPU only: the float32-against-float64 table of tests/snp_train_ref.py

Per batch size, on random integer tensors (-8..8) and the shipped ONT-HG002 weights, HIP events on the engine's stream around each call, one
call per repetition, the device drained between repetitions; median, min, 10th and 90th percentile over the repetitions:

    step            SnpTrainer.step: forward with stored activations, backward, slab sum + Adam, the six losses back on the host
    loss_grad       the same without the Adam kernel
    forward_exact   Engine.snp_forward of the same sites on the exact-fp32 inference trunk (nc_set_cnn_precision(ctx, 1))
    stages          the step's split (nc_train_stage_ms: events between the stage groups of one loss_grad, median over the repetitions)
    workspace_bytes_per_site
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(a[len(a) // 10]), p90_ms=float(a[(9 * len(a)) // 10]), reps=int(a.size))


def noise_table():
    """the float32 restatement against the float64 one on the tests' inputs: {case: largest per-tensor error | largest loss error}"""
    import numpy as np
    import snp_train_ref as R
    import torch
    from nanocaller_amd.train import xavier_init
    from nanocaller_amd.weights import Weights, get_SNP_model
    W = {"ONT-HG002": Weights(get_SNP_model("ONT-HG002")[0]).flat, "xavier3": xavier_init(3)}
    out = {}
    for wn, w in W.items():
        for case in (1, 3, 17, 64, 300, "17s") + ((4160,) if wn == "xavier3" else ()):
            n = 17 if case == "17s" else case
            x, ref, lab, mask = R.make_inputs(n)
            sc = np.linspace(0.5, 2.0, n) if case == "17s" else None
            l64, g64 = R.loss_grad(w, x, ref, lab, mask, 0.5, scale=sc)
            l32, g32 = R.loss_grad(w, x, ref, lab, mask, 0.5, scale=sc, dtype=torch.float32)
            e = R.rel_errors(g32, g64)
            worst = max(e, key=e.get)
            out["grad %s n=%s" % (wn, case)] = dict(tensor_err=e[worst], tensor=worst, loss_err=float((np.abs(l32 - l64) / np.abs(l64)).max()),
                                                    bound=R.grad_bound(wn, case))
        x, ref, lab, _ = R.make_inputs(64)
        masks = [R.make_inputs(64, seed=50 + t)[3] for t in range(5)]
        l64, w64 = R.trajectory(w, x, ref, lab, masks, 0.5, R.TRAJ_LR)
        l32, w32 = R.trajectory(w, x, ref, lab, masks, 0.5, R.TRAJ_LR, dtype=torch.float32)
        w0 = np.asarray(w, np.float64)
        e = R.rel_errors(w32 - w0, w64 - w0)
        worst = max(e, key=e.get)
        out["trajectory %s, 5 steps n=64" % wn] = dict(tensor_err=e[worst], tensor=worst, loss_err=float((np.abs(l32 - l64) / np.abs(l64)).max()),
                                                       bound=R.TRAJ_BOUND)
    return out


def timed(fn, reps, warmup):
    import torch
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return stats(ms)


def bench(args):
    import numpy as np
    import torch
    from nanocaller_amd import _lib
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.train import SnpTrainer
    from nanocaller_amd.weights import Weights, get_SNP_model
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_SNP, Weights(get_SNP_model("ONT-HG002")[0]))
    res = {}
    for n in args.batches:
        rng = np.random.default_rng(n)
        x = torch.from_numpy(rng.integers(-8, 9, (n, 5, 41, 5)).astype(np.float32)).to(eng.device)
        ref = torch.from_numpy((np.arange(n) % 4).astype(np.int32)).to(eng.device)
        lab = torch.from_numpy(rng.integers(0, 2, (n, 5)).astype(np.uint8)).to(eng.device)
        tr = SnpTrainer(0, "ONT-HG002", lr=1e-6, max_batch=n)
        mask = tr.draw_mask(n)
        r = dict(step=timed(lambda: tr.step(x, ref, lab, mask=mask), args.reps, args.warmup),
                 loss_grad=timed(lambda: tr.loss_grad(x, ref, lab, mask, 0.5, want_grad=False), args.reps, args.warmup))
        with eng._snp_state(exact_fp32=True):
            r["forward_exact"] = timed(lambda: eng.snp_forward(_lib.MODEL_SNP, x, ref, None), args.reps, args.warmup)
        r["forward_split_precision"] = timed(lambda: eng.snp_forward(_lib.MODEL_SNP, x, ref, None), args.reps, args.warmup)
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
        res["batch_%d" % n] = r
        print("batch", n, json.dumps(r), file=sys.stderr, flush=True)
        tr.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--noise", action="store_true", help="CPU only: print the float32 noise table and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snp_train.json"))
    args = ap.parse_args()
    noise = noise_table()
    if args.noise:
        for k, v in noise.items():
            print("%-40s %.2e (%s)  losses %.2e  bound %.1e" % (k, v["tensor_err"], v["tensor"], v["loss_err"], v["bound"]))
        return
    res = {"workload": "random integer tensors in -8..8, ONT-HG002 weights, keep 0.5; HIP events around one call, 1x MI355X",
           "float32_noise": noise}
    res.update(bench(args))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "float32_noise"}))


if __name__ == "__main__":
    main()

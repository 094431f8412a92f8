#!/usr/bin/env python3
"""Step time of the indel trainer (csrc/nc_train_indel.hip) and the float32 noise figures its tests' bounds are made of.

    python tools/bench_train_indel.py [--batches 256 1024] [--reps 40] [--warmup 8] [--out profiles/indel_train.json]
    python tools/bench_train_indel.py --noise     # CPU only: the float32-against-float64 table of tests/indel_train_ref.py

Per batch size, on the tests' pipeline-like tensors (indel_train_ref.make_inputs) and the shipped ONT-HG002 indel weights, HIP events on the
engine's stream around each call, one call per repetition, the device drained between repetitions; median, min, 10th and 90th percentile
over the repetitions:

    step            IndelTrainer.step: forward with stored activations, backward, slab sum + Adam, the two losses back on the host
    loss_grad       the same without the Adam kernel
    forward_exact   Engine.indel_forward of the same sites on the exact-fp32 inference trunk (nc_set_cnn_precision(ctx, 1))
    stages          the step's split (nc_indel_train_stage_ms: events between the stage groups of one loss_grad, median over the repetitions)
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
    """the float32 restatement against the float64 one on the tests' inputs: {case: largest per-tensor error | largest loss error | bound}"""
    import indel_train_ref as R
    m = R.measure_noise()
    out = {}
    for key, err in m["grad"].items():
        wn, n = key.split("/")
        out["grad %s n=%s" % (wn, n)] = dict(tensor_err=err, tensor=m["worst_tensor"][key], loss_err=m["loss"][key], bound=R.grad_bound(wn, int(n)))
    for wn, t in m["traj"].items():
        out["trajectory %s, 5 steps n=64" % wn] = dict(tensor_err=t["dw"], tensor=t["worst_tensor"], loss_err=t["losses"], bound=R.traj_bound(wn),
                                                       torch_eps_tensor_err=t["torch_eps_dw"])
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
    import indel_train_ref as R
    import numpy as np
    import torch
    from nanocaller_amd import _lib
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.train_indel import IndelTrainer
    from nanocaller_amd.weights import Weights, get_indel_model
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_INDEL, Weights(get_indel_model("ONT-HG002")))
    res = {}
    for n in args.batches:
        xh, labh, _ = R.make_inputs(n)
        x, lab = torch.from_numpy(xh).to(eng.device), torch.from_numpy(labh).to(eng.device)
        tr = IndelTrainer(0, "ONT-HG002", lr=1e-6, max_batch=n)
        mask = tr.draw_mask(n)
        r = dict(step=timed(lambda: tr.step(x, lab, mask=mask), args.reps, args.warmup),
                 loss_grad=timed(lambda: tr.loss_grad(x, lab, mask, 0.5, want_grad=False), args.reps, args.warmup))
        with eng._snp_state(exact_fp32=True):
            r["forward_exact"] = timed(lambda: eng.indel_forward(_lib.MODEL_INDEL, x), args.reps, args.warmup)
        r["forward_split_precision"] = timed(lambda: eng.indel_forward(_lib.MODEL_INDEL, x), args.reps, args.warmup)
        r["train_forward"] = timed(lambda: tr.forward(x), args.reps, args.warmup)
        tr.stage_ms(True)
        rows = []
        for _ in range(args.reps):
            tr.loss_grad(x, lab, mask, 0.5, want_grad=False)
            rows.append(tr.stage_ms(True))
        tr.stage_ms(False)
        r["stages_median_ms"] = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
        info = tr.info()
        r["slice_sites"] = info["slice_sites"]
        r["workspace_bytes_per_site"] = info["workspace_bytes"] / info["slice_sites"]
        r["step_over_forward_exact"] = r["step"]["median_ms"] / r["forward_exact"]["median_ms"]
        r["sites_per_s"] = n / r["step"]["median_ms"] * 1e3
        res["batch_%d" % n] = r
        print("batch", n, json.dumps(r), file=sys.stderr, flush=True)
        tr.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--noise", action="store_true", help="CPU only: print the float32 noise table and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indel_train.json"))
    args = ap.parse_args()
    noise = noise_table()
    if args.noise:
        for k, v in noise.items():
            print("%-42s %.2e (%s)  losses %.2e  bound %.1e" % (k, v["tensor_err"], v["tensor"], v["loss_err"], v["bound"]))
        return
    res = {"workload": "pipeline-like tensors (indel_train_ref.make_inputs), ONT-HG002 indel weights, keep 0.5; HIP events around one call, 1x MI355X",
           "float32_noise": noise}
    res.update(bench(args))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "float32_noise"}))


if __name__ == "__main__":
    main()

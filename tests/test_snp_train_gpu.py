"""The SNP trainer on the device (csrc/nc_train.hip, nanocaller_amd/train.py) against the float64 restatement of tests/snp_train_ref.py.

Inputs (snp_train_ref.make_inputs): integer tensors in -8..8, all four reference bases, both classes in every label column, a seeded 0/1
mask.  Weight sets: the shipped ONT-HG002 and Xavier-uniform from seed 3.  Batch sizes 1, 3, 17, 64, 300: one site, a partial 16-site MFMA
tile, a tile boundary, a full slab of four tiles, several workgroups' slabs (4160 in one test: more than one workspace slice).
Every comparison is per parameter tensor, never global, and its bound is 10 x the float32-against-float64 error of the restatement itself on the
same inputs (the figures stand next to the constants in snp_train_ref.py).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import snp_train_ref as R  # noqa: E402
from nanocaller_amd import _lib, train  # noqa: E402
from nanocaller_amd.weights import Weights, get_SNP_model  # noqa: E402

pytestmark = pytest.mark.gpu
KEEP = 0.5
SIZES = (1, 3, 17, 64, 300)


@functools.lru_cache(None)
def weights(wname):
    return Weights(get_SNP_model("ONT-HG002")[0]).flat if wname == "ONT-HG002" else train.xavier_init(3)


@functools.lru_cache(None)
def reference(wname, n, scaled=False):
    """-> (inputs, scale, float64 losses, float64 gradient); computed once and shared"""
    x, ref, lab, mask = R.make_inputs(n)
    scale = np.linspace(0.5, 2.0, n) if scaled else None
    l6, g = R.loss_grad(weights(wname), x, ref, lab, mask, KEEP, scale=scale)
    return (x, ref, lab, mask), scale, l6, g


@functools.lru_cache(None)
def trainer(wname, max_batch=300):
    return train.SnpTrainer(0, weights(wname), lr=R.TRAJ_LR, gamma=R.GAMMA, keep=KEEP, seed=0, max_batch=max_batch)


def precheck(wname, n):
    """no dead layer, no head saturated on every site: otherwise an error there would not show"""
    (x, ref, lab, mask), _, _, g = reference(wname, n)
    for name, off, size, _ in R.segments():
        assert np.linalg.norm(g[off:off + size]) > 0, name
    out = R.forward(R.split(weights(wname)), x, ref, None, mask, KEEP)
    p = np.concatenate([out["probs"].numpy(), out["gt"].numpy()[:, 1:]], 1)
    if n >= 3:
        assert (np.minimum(p, 1 - p) > 1e-6).any(0).all(), "a head is saturated on all sites"


def compare(wname, case, l6, grad, want_l6, want_g, what):
    bound = R.grad_bound(wname, case)
    e = R.rel_errors(grad, want_g)
    le = np.abs(np.asarray(l6, np.float64) - want_l6) / np.abs(want_l6)
    worst = max(e, key=e.get)
    print("%s %s %s: largest per-tensor error %.2e (%s), losses %.2e, bound %.1e" % (what, wname, case, e[worst], worst, le.max(), bound))
    assert le.max() <= bound, dict(zip(R.LOSS_KEYS, le))
    assert e[worst] <= bound, {k: v for k, v in e.items() if v > bound}


def device_loss_grad(tr, inputs, scale=None, keep=KEEP):
    x, ref, lab, mask = inputs
    losses, grad = tr.loss_grad(x, ref, lab, mask, keep, scale)
    return np.array([losses[k] for k in R.LOSS_KEYS]), grad


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("wname", ["ONT-HG002", "xavier3"])
def test_gradient(wname, n):
    precheck(wname, n)
    inputs, _, want_l6, want_g = reference(wname, n)
    l6, grad = device_loss_grad(trainer(wname), inputs)
    compare(wname, n, l6, grad.cpu().numpy(), want_l6, want_g, "gradient")


@pytest.mark.parametrize("wname", ["ONT-HG002", "xavier3"])
def test_gradient_with_coverage_scale(wname):
    inputs, scale, want_l6, want_g = reference(wname, 17, True)
    l6, grad = device_loss_grad(trainer(wname), inputs, scale)
    compare(wname, "17s", l6, grad.cpu().numpy(), want_l6, want_g, "gradient, scaled input")


def test_gradient_over_two_slices():
    """4160 sites = one workspace slice of 4096 and a second of one slab: the slices' gradients are accumulated"""
    inputs, _, want_l6, want_g = reference("xavier3", 4160)
    tr = train.SnpTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=4160)
    assert tr.info()["slice_sites"] == 4096
    l6, grad = device_loss_grad(tr, inputs)
    compare("xavier3", 4160, l6, grad.cpu().numpy(), want_l6, want_g, "gradient, two slices")
    tr.close()


@pytest.mark.parametrize("wname", ["ONT-HG002", "xavier3"])
def test_forward(wname):
    from nanocaller_amd.engine import get_engine
    from oracle import oracle
    n = 300
    x, ref, _, _ = R.make_inputs(n)
    scale = np.linspace(0.5, 2.0, n)
    tr = trainer(wname)
    for sc in (None, scale):
        probs, gt = tr.forward(x, ref, sc)
        ep, eg = oracle.snp_forward(weights(wname), x, ref, np.ones(n) if sc is None else sc, precision="f64")
        err = max(float(np.abs(probs.cpu().numpy() - ep).max()), float(np.abs(gt.cpu().numpy() - eg).max()))
        print("training forward against the oracle (%s, scale %s): %.2e" % (wname, sc is not None, err))
        assert err < 1e-4
    # against the inference path in exact-fp32 mode: two float32 evaluations of the same function
    eng = get_engine(0)
    path = os.path.join(str(_tmp()), "w_%s.ncw" % wname)
    train.write_ncw(path, 0, 30.0, train.blob_tensors(weights(wname)))
    eng.load_weights(_lib.MODEL_SNP, Weights(path))
    dx = torch.from_numpy(x).to(eng.device)
    dref = torch.from_numpy(ref).to(eng.device)
    dsc = torch.from_numpy(scale).to(eng.device)
    with eng._snp_state(exact_fp32=True):
        p2, g2 = eng.snp_forward(_lib.MODEL_SNP, dx, dref, dsc)
    probs, gt = tr.forward(x, ref, scale)
    err = max(float((probs - p2).abs().max()), float((gt - g2).abs().max()))
    print("training forward against Engine.snp_forward, exact fp32 (%s): %.2e" % (wname, err))
    assert err <= R.grad_bound(wname, 300)


_TMP = []


def _tmp():
    import tempfile
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory())
    return _TMP[0].name


def test_determinism():
    inputs, _, _, _ = reference("ONT-HG002", 300)
    tr = trainer("ONT-HG002")
    _, g1 = device_loss_grad(tr, inputs)
    _, g2 = device_loss_grad(tr, inputs)
    assert torch.equal(g1, g2)
    tr2 = train.SnpTrainer(0, weights("ONT-HG002"), gamma=R.GAMMA, max_batch=300)
    _, g3 = device_loss_grad(tr2, inputs)
    assert torch.equal(g1, g3)
    tr2.close()


def test_padding_contributes_nothing():
    """17 sites in a 64-site workspace that a 64-site batch of NaN tensors has filled with NaN (activations, gradients, slabs) give the
    bits of 17 sites in a workspace of their own"""
    inputs, _, _, _ = reference("xavier3", 17)
    x64, ref64, lab64, mask64 = R.make_inputs(64)
    big = train.SnpTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=64)
    l_nan, g_nan = device_loss_grad(big, (np.full_like(x64, np.nan), ref64, lab64, mask64))
    assert np.isnan(l_nan).any() and bool(torch.isnan(g_nan).any())
    _, g_big = device_loss_grad(big, inputs)
    small = train.SnpTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=17)
    _, g_small = device_loss_grad(small, inputs)
    assert not bool(torch.isnan(g_big).any())
    assert torch.equal(g_big, g_small)
    big.close()
    small.close()


@pytest.mark.parametrize("wname", ["ONT-HG002", "xavier3"])
def test_trajectory(wname):
    """five Adam steps at n = 64 with fixed masks"""
    x, ref, lab, _ = R.make_inputs(64)
    masks = [R.make_inputs(64, seed=50 + t)[3] for t in range(5)]
    want_l, want_w = R.trajectory(weights(wname), x, ref, lab, masks, KEEP, R.TRAJ_LR)
    tr = train.SnpTrainer(0, weights(wname), lr=R.TRAJ_LR, gamma=R.GAMMA, keep=KEEP, max_batch=64)
    for t, mask in enumerate(masks):
        got = tr.step(x, ref, lab, mask=mask)
        le = np.abs(np.array([got[k] for k in R.LOSS_KEYS]) - want_l[t]) / np.abs(want_l[t])
        print("step %d: losses %.2e" % (t + 1, le.max()))
        assert le.max() <= R.TRAJ_BOUND, (t, dict(zip(R.LOSS_KEYS, le)))
    assert tr.info()["steps"] == 5
    w0 = np.asarray(weights(wname), np.float64)
    e = R.rel_errors(tr.get_weights().astype(np.float64) - w0, want_w - w0)
    worst = max(e, key=e.get)
    print("trajectory %s: largest per-tensor error of delta w %.2e (%s), bound %.1e" % (wname, e[worst], worst, R.TRAJ_BOUND))
    assert e[worst] <= R.TRAJ_BOUND, {k: v for k, v in e.items() if v > R.TRAJ_BOUND}
    tr.close()


def test_end_to_end_on_a_synthetic_world():
    """a world of 50,000 bases: the smallest multiple of 10,000 at which the labelling rule keeps at least 200 sites with both GT classes
    (found with the oracle's candidates on the CPU: 40,000 -> 165 sites, 50,000 -> 231)"""
    from nanocaller_amd import snpCaller
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth import make_world
    world = make_world(seed=7, length=50_000, depth=20, read_len_scale=0.4)
    params = dict(sam_path=world, fasta_path=None, mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6],
                  seq="ont", supplementary=False, exclude_bed=None, disable_coverage_normalization=False)
    ex = train.snp_training_examples(params, neg_ratio=2.0, seed=0)
    x, ref, lab, pos, depth = ex[world.chrom]
    n = int(x.shape[0])
    assert n >= 200 and n == lab.shape[0] == pos.shape[0] and lab[:, 4].min() == 0 and lab[:, 4].max() == 1
    truth = train.world_truth(world)
    assert all(lab[i, 4] == truth[int(p)][0] for i, p in enumerate(pos) if int(p) in truth)
    tr = train.SnpTrainer(0, None, lr=1e-3, seed=1, max_batch=n)
    before = tr.evaluate(x, ref, lab)["cost"]
    for _ in range(30):
        tr.step(x, ref, lab)
    ev = tr.evaluate(x, ref, lab)
    print("end to end: %d sites, cost %.4f -> %.4f after 30 steps, accuracies GT %.2f all %.2f" % (n, before, ev["cost"], ev["acc_GT"], ev["acc_all"]))
    assert ev["cost"] < before
    path = tr.save(os.path.join(_tmp(), "model-30.ncw"), depth)
    w = Weights(path)
    assert w.kind == 0 and abs(w.train_coverage - depth) < 1e-3 and np.array_equal(w.flat, tr.get_weights())
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_SNP, w)
    p2, g2 = eng.snp_forward(_lib.MODEL_SNP, x, ref, None)
    assert float((p2 - ev["probs"]).abs().max()) < 1e-4 and float((g2 - ev["gt"]).abs().max()) < 1e-4
    r = snpCaller.call_chunks(dict(params, snp_model=path), [dict(chrom=world.chrom, start=1, end=50_000, ploidy="diploid")])
    assert r["n"] > 200 and r["probs"].shape == (r["n"], 4) and np.isfinite(r["probs"]).all()
    tr.close()


def test_rejected_kinds():
    from nanocaller_amd.engine import get_engine
    eng = get_engine(0)
    for kind in (_lib.MODEL_SNP_HAP, _lib.MODEL_INDEL, _lib.MODEL_INDEL_HAP):
        h = C.c_void_p()
        assert eng.L.nc_train_create(eng.ctx, kind, 64, C.byref(h)) == _lib.NC_ERR_UNSUPPORTED and not h.value
        assert b"diploid SNP" in eng.L.nc_last_error(eng.ctx)
        with pytest.raises(ValueError):
            train.SnpTrainer(0, None, kind=kind)
    with pytest.raises(ValueError):
        train.SnpTrainer(0, "haploid")
    tr = train.SnpTrainer(0, weights("xavier3"), max_batch=1)
    with pytest.raises(_lib.NanoCallerHipError):                       # no gradient to step with
        tr.adam_step()
    tr.close()


@pytest.mark.parametrize("wrong", ["x", "mask", "labels", "ref_code"])
def test_misshapen_inputs_refused(wrong):
    """a tensor, mask, label array or reference-code array of the wrong shape raises ValueError before the device call, which would read
    n sites of each; the trainer then still takes a correct step on 3 sites"""
    x, ref, lab, mask = R.make_inputs(3)
    bad = dict(x=np.asarray(x), ref_code=np.asarray(ref), labels=np.asarray(lab), mask=np.asarray(mask))
    assert bad["x"].shape == (3, 5, 41, 5) and bad["mask"].shape == (3, 48) and bad["labels"].shape == (3, 5) and bad["ref_code"].shape == (3,)
    bad[wrong] = {"x": bad["x"][..., :4], "mask": bad["mask"][:, :32], "labels": bad["labels"][:, 0], "ref_code": bad["ref_code"][:2]}[wrong]
    tr = train.SnpTrainer(0, weights("xavier3"), max_batch=8)
    with pytest.raises(ValueError):
        tr.step(bad["x"], bad["ref_code"], bad["labels"], mask=bad["mask"])
    assert tr.info()["steps"] == 0
    losses = tr.step(x, ref, lab, mask=mask)
    assert tr.info()["steps"] == 1 and np.isfinite([losses[k] for k in R.LOSS_KEYS]).all()
    assert not np.array_equal(tr.get_weights(), weights("xavier3"))
    tr.close()


def test_train_snp_model_from_files():
    """the file route (truth VCF + confident BED) gives the planted-truth route's examples inside the intervals, and train_snp_model writes
    one loadable model per epoch"""
    from nanocaller_amd.synth import make_world
    world = make_world(seed=7, length=50_000, depth=20, read_len_scale=0.4)
    params = dict(sam_path=world, fasta_path=None, mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6],
                  seq="ont", supplementary=False, exclude_bed=None, disable_coverage_normalization=False)
    truth = train.world_truth(world)
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for p in sorted(truth):
        _, a, b = truth[p]
        r = world.ref[p - 1].upper()
        alts = [c for c in dict.fromkeys(("AGTC"[a], "AGTC"[b])) if c != r]
        al = [r] + alts
        lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%d/%d" % (world.chrom, p, r, ",".join(alts) or ".", al.index("AGTC"[a]), al.index("AGTC"[b])))
    vcf, bed = os.path.join(_tmp(), "truth.vcf"), os.path.join(_tmp(), "conf.bed")
    open(vcf, "w").write("\n".join(lines) + "\n")
    open(bed, "w").write("%s\t0\t30000\n%s\t35000\t50000\n" % (world.chrom, world.chrom))
    assert train.parse_truth_vcf(open(vcf).read(), world.chrom) == truth
    whole = train.snp_training_examples(params, neg_ratio=None)[world.chrom]
    files = train.snp_training_examples(dict(params, chrom_list=[(world.chrom, 1, 50_000)]), vcf, bed, neg_ratio=None)[world.chrom]
    inside = (whole[3] <= 30000) | (whole[3] > 35000)
    assert np.array_equal(files[3], whole[3][inside]) and np.array_equal(files[2], whole[2][inside])
    assert torch.equal(files[0], whole[0][torch.from_numpy(inside).to(whole[0].device)])
    out = os.path.join(_tmp(), "models")
    hist = train.train_snp_model(dict(params, truth_vcf=vcf, confident_bed=bed, chrom_list=[(world.chrom, 1, 50_000)], out_dir=out, epochs=3, batch=64,
                                      seed=2))
    assert [os.path.basename(h["path"]) for h in hist] == ["model-1.ncw", "model-2.ncw", "model-3.ncw"] and hist[2]["train_cost"] < hist[0]["train_cost"]
    w = Weights(hist[2]["path"])
    assert w.kind == 0 and 10 < w.train_coverage < 30 and np.isfinite(w.flat).all() and 0 <= hist[2]["val_acc_GT"] <= 1

"""CPU-only checks of the haploid SNP trainer's reference computation (tests/hap_train_ref.py), of the labelling rule
(nanocaller_amd/train_haploid.py) and of the callers' haploid-model keys (nanocaller_amd/weights.py): the restatement is pinned to the oracle's
forward, its gradient to finite differences, its Adam to the written-out formula; no listed case is saturated; each mistake the device
comparison is meant to catch breaks that comparison when made in the restatement itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hap_train_ref as R  # noqa: E402
from nanocaller_amd import _lib, train_haploid, weights  # noqa: E402
from nanocaller_amd.weights import KIND_SNP_HAP, get_SNP_model  # noqa: E402


def test_forward_pinned_to_oracle():
    from oracle import oracle
    w = R.weights("haploid")
    x, ref, _, _ = R.make_inputs(17)
    scale = np.linspace(0.5, 2.0, 17)
    for sc in (None, scale):
        out = R.forward(R.split(w), x, ref, sc)
        ep = oracle.snp_hap_forward(w, x, ref, np.ones(17) if sc is None else sc, precision="f64")
        ep = ep[0] if isinstance(ep, tuple) else ep                      # (probs, no GT output)
        # the oracle computes in float64 but hands its results back as float32 arrays: the agreement asked for is 1e-9, on top of the
        # half ulp of float32 below 1 (2^-25 = 3e-8) that this rounding of the oracle's output costs
        assert ep.shape == (17, 4)
        assert np.abs(out["probs"].numpy() - ep.astype(np.float64)).max() < 2.0 ** -25 + 1e-9


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_no_listed_case_is_saturated(wname):
    """every (weight set, n) of the device comparisons, with the mask and without, the scaled case and the trajectory's five masks at their
    initial weights: the label's softmax probability stays more than 1e-4 away from 0 and from 1"""
    w = R.weights(wname)
    lo, hi = 1.0, 0.0
    for case in R.SIZES + ("17s",):
        n = 17 if case == "17s" else case
        x, ref, lab, mask = R.make_inputs(n)
        scale = np.linspace(0.5, 2.0, n) if case == "17s" else None
        for m, keep in ((mask, R.KEEP), (None, 1.0)):
            lp = R.label_probs(w, x, ref, lab, m, keep, scale)
            assert lp.min() > R.SATURATED and lp.max() < 1 - R.SATURATED, (wname, case, keep, lp.min(), lp.max())
            lo, hi = min(lo, lp.min()), max(hi, lp.max())
    x, ref, lab, _ = R.make_inputs(64)
    for t in range(5):
        lp = R.label_probs(w, x, ref, lab, R.make_inputs(64, seed=50 + t)[3], R.KEEP)
        assert lp.min() > R.SATURATED and lp.max() < 1 - R.SATURATED
    print("%s: label probabilities within [%.2e, 1 - %.2e]" % (wname, lo, 1 - hi))


def test_inputs_hold_every_class():
    for n in R.SIZES[2:]:
        _, ref, lab, _ = R.make_inputs(n)
        assert set(lab.tolist()) == {0, 1, 2, 3} and set(ref.tolist()) == {0, 1, 2, 3} and (lab != ref).any() and (lab == ref).any()


def test_gradient_against_finite_differences():
    w = train_haploid.xavier_init(KIND_SNP_HAP, 3).astype(np.float64)
    x, ref, lab, mask = R.make_inputs(3)
    _, g = R.loss_grad(w, x, ref, lab, mask, 0.5)
    rng = np.random.default_rng(5)

    def cost(wv):
        p = R.split(wv)
        return R.cost(p, R.forward(p, x, ref, None, mask, 0.5), lab)["cost"].item()

    worst = 0.0
    for name, off, size, _ in R.segments():
        for i in rng.choice(size, min(5, size), replace=False):
            h = 1e-6                                                    # (small: at inputs in -1..1 a conv1 pre-activation lies within 1e-5 of SELU's kink)
            wp, wm = w.copy(), w.copy()
            wp[off + i] += h
            wm[off + i] -= h
            fd = (cost(wp) - cost(wm)) / (2 * h)
            err = abs(fd - g[off + i]) / max(abs(g[off + i]), 1e-3 * np.abs(g[off:off + size]).max())
            worst = max(worst, err)
            assert err < 1e-6, (name, int(i), fd, g[off + i])
    print("finite differences: worst relative error %.2e" % worst)


def test_adam_is_tensorflows_form():
    g = [np.array([0.5, -2.0, 1e-4, 0.0]), np.array([0.25, 1.0, -1e-4, 3.0]), np.array([-0.5, 0.5, 2e-4, -3.0])]
    w = np.array([1.0, -1.0, 0.5, 2.0])
    m, v = np.zeros(4), np.zeros(4)
    w2, m2, v2 = w.copy(), m.copy(), v.copy()
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    for t in range(1, 4):
        w, m, v = R.adam_step(w, m, v, g[t - 1], t, lr, b1, b2, eps)
        for i in range(4):                                              # the written-out formula, entry by entry
            lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            m2[i] = b1 * m2[i] + (1 - b1) * g[t - 1][i]
            v2[i] = b2 * v2[i] + (1 - b2) * g[t - 1][i] ** 2
            w2[i] -= lr_t * m2[i] / (np.sqrt(v2[i]) + eps)
        assert np.allclose(w, w2, rtol=1e-14, atol=0) and np.allclose(m, m2, rtol=1e-14) and np.allclose(v, v2, rtol=1e-14)
    w1, _, _ = R.adam_step(np.zeros(1), np.zeros(1), np.zeros(1), np.array([1e-8]), 1, 1.0)
    assert abs(-w1[0] - 1e-8 / (1e-8 + 1e-8 / np.sqrt(1 - 0.999))) < 1e-12


@pytest.fixture(scope="module")
def probe_cases():
    out = {}
    for wname in R.WEIGHT_SETS:
        w = R.weights(wname)
        x, ref, lab, mask = R.make_inputs(64)
        out[wname] = (w, x, ref, lab, mask, R.loss_grad(w, x, ref, lab, mask, R.KEEP))
    return out


def _breaks(wname, l2, g, want):
    """what test_gradient of the device tests asserts, as a predicate"""
    e = R.rel_errors(g, want[1])
    le = np.abs(l2 - want[0]) / np.abs(want[0])
    bound = R.grad_bound(wname, 64)
    return max(e.values()) > bound or le.max() > bound


# a probe that a weight set cannot see is left out for that set by name, with the reason
PROBES_BLIND = {
    ("xavier3", "reg_bias"): "Xavier initialisation has zero biases: regularising them adds nothing to the cost or its gradient",
}


@pytest.mark.parametrize("variant", ["no_reg", "reg_bias", "mask_first", "no_inv_keep", "no_fc3_selu", "no_onehot", "acgt"])
@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_probe_sharpness(probe_cases, wname, variant):
    w, x, ref, lab, mask, want = probe_cases[wname]
    assert not _breaks(wname, *R.loss_grad(w, x, ref, lab, mask, R.KEEP), want)
    l2, g = R.loss_grad(w, x, ref, lab, mask, R.KEEP, variant=variant)
    e = R.rel_errors(g, want[1])
    print(wname, variant, "largest per-tensor error %.2e (%s)" % (max(e.values()), max(e, key=e.get)))
    if (wname, variant) in PROBES_BLIND:
        assert not _breaks(wname, l2, g, want), "the reason given for leaving this probe out no longer holds"
        return
    assert _breaks(wname, l2, g, want), variant


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_probe_sharpness_adam_eps(wname):
    """torch's eps placement breaks the trajectory comparison of the device tests on the shipped weights.  On xavier(3) it is left out: every
    gradient entry there is far above eps, the two placements differ by 6.5e-3 of delta w, and float32 itself by 7.0e-4, so the bound of ten
    times that does not separate them (asserted, so that the reason stays true)."""
    w = R.weights(wname)
    x, ref, lab, _ = R.make_inputs(64)
    masks = [R.make_inputs(64, seed=50 + t)[3] for t in range(5)]
    _, w_tf = R.trajectory(w, x, ref, lab, masks, R.KEEP, R.TRAJ_LR)
    _, w_torch = R.trajectory(w, x, ref, lab, masks, R.KEEP, R.TRAJ_LR, torch_eps=True)
    w0 = np.asarray(w, np.float64)
    worst = max(R.rel_errors(w_torch - w0, w_tf - w0).values())
    print("%s: torch's eps placement moves delta w by %.2e, bound %.1e" % (wname, worst, R.traj_bound(wname)))
    assert (worst > R.traj_bound(wname)) == (wname == "haploid")


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_measured_noise_is_what_the_bounds_say(wname):
    """the float32 figures behind the bounds, measured again: the gradient cases of R.PINNED_CASES (the module says why n = 300 and 4160 are
    one machine's), the trajectory and the forward.  (The float32 sums depend a little on how many threads torch's kernels split them over.)"""
    for case in R.PINNED_CASES:
        worst, _ = R.measure_noise(wname, case)
        print("%s %s: float32 against float64 %.2e (table %.2e)" % (wname, case, worst, R.GRAD_F32_NOISE[(wname, case)]))
        assert 0.3 * R.GRAD_F32_NOISE[(wname, case)] <= worst <= 3 * R.GRAD_F32_NOISE[(wname, case)], case
    traj = R.measure_traj_noise(wname)
    print("%s: five-step trajectory: %.2e" % (wname, traj))
    assert 0.3 * R.TRAJ_F32_NOISE[wname] <= traj <= 3 * R.TRAJ_F32_NOISE[wname]
    fwd = R.measure_forward_noise(wname)
    print("%s: forward at n = 300: %.2e" % (wname, fwd))
    assert 0.3 * R.FWD_F32_NOISE[wname] <= fwd <= 3 * R.FWD_F32_NOISE[wname]
    assert set(R.GRAD_F32_NOISE) == {(s, c) for s in R.WEIGHT_SETS for c in R.SIZES + ("17s",)}


VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
    "c1\t10\t.\tA\tG\t.\tPASS\t.\tGT\t0/1",          # het: the site is dropped
    "c1\t20\t.\tT\tC\t.\tPASS\t.\tGT:DP\t1|1:30",     # hom alt -> C
    "c1\t25\t.\tG\tT\t.\tPASS\t.\tGT\t1",             # haploid genotype -> T
    "c1\t30\t.\tG\tA,T\t.\tPASS\t.\tGT\t1/2",         # two alts: dropped
    "c1\t33\t.\tG\tA,T\t.\tPASS\t.\tGT\t2/2",         # the second alt on both copies -> T
    "c1\t40\t.\tA\tAT\t.\tPASS\t.\tGT\t1/1",          # insertion: dropped
    "c1\t50\t.\tC\tT\t.\tPASS\t.\tGT\t./.",           # no call: dropped
    "c1\t60\t.\tC\tT\t.\tPASS\t.\tGT\t0/0",           # hom ref is no statement about a variant: dropped
    "c1\t70\t.\tC\tT\t.\tPASS\t.\tGT\t1/1",           # outside the BED
    "c2\t12\t.\tA\tC\t.\tPASS\t.\tGT\t1/1",
])
BED = "c1\t0\t45\nc1\t55\t65\nc2\t0\t100\n"


def test_snp_labelling_rule():
    A = train_haploid.AMBIGUOUS
    truth = train_haploid.parse_haploid_truth_vcf(VCF, "c1")
    assert truth == {10: A, 20: 3, 25: 2, 30: A, 33: 2, 40: A, 50: A, 60: A, 70: 2}
    iv = train_haploid.parse_bed(BED, "c1")
    pos = np.array([5, 10, 12, 20, 25, 30, 33, 36, 40, 46, 58, 60, 62, 70])
    ref = np.array([0, 0, 1, 2, 1, 1, 1, 0, 0, 2, 1, 3, 2, 3])
    idx, lab, dropped = train_haploid.label_haploid_sites(pos, ref, truth, iv, neg_ratio=None)
    # 10 (het), 30, 40, 60 are ambiguous; 46 and 70 are outside the intervals; 12 takes c1's own truth, not c2's record at 12
    assert pos[idx].tolist() == [5, 12, 20, 25, 33, 36, 58, 62]
    assert lab.tolist() == [0, 1, 3, 2, 2, 0, 1, 2] and lab.dtype == np.uint8
    assert dropped == dict(outside_bed=2, ambiguous=4, negatives_subsampled=0)
    # three truth sites (20, 25, 33), five others: neg_ratio 1 keeps three of them, the same ones for the same seed
    i1, l1, d1 = train_haploid.label_haploid_sites(pos, ref, truth, iv, neg_ratio=1.0, seed=3)
    i2, _, _ = train_haploid.label_haploid_sites(pos, ref, truth, iv, neg_ratio=1.0, seed=3)
    assert i1.tolist() == i2.tolist() and len(i1) == 6 and {20, 25, 33} <= set(pos[i1].tolist()) and d1["negatives_subsampled"] == 2
    want = dict(zip(pos[idx].tolist(), lab.tolist()))
    assert all(l1[j] == want[int(pos[i])] for j, i in enumerate(i1))
    everywhere = train_haploid.label_haploid_sites(pos, ref, truth, None, neg_ratio=None)
    assert len(everywhere[0]) == 10 and everywhere[2]["outside_bed"] == 0 and everywhere[2]["ambiguous"] == 4


def test_xavier_init_and_blob_tensors():
    w = train_haploid.xavier_init(KIND_SNP_HAP, 3)
    assert w.shape == (108308,) and w.dtype == np.float32 and np.array_equal(w, train_haploid.xavier_init(KIND_SNP_HAP, 3))
    assert not np.array_equal(w, train_haploid.xavier_init(KIND_SNP_HAP, 4))
    for name, off, size, is_kernel in R.segments():
        assert (np.abs(w[off:off + size]).max() > 0) == is_kernel, name
    t = dict(train_haploid.blob_tensors(w))
    lim = np.sqrt(6.0 / (20 + 4))
    assert t["fc3.k"].shape == (20, 4) and t["fc2.k"].shape == (48, 16) and np.abs(t["fc3.k"]).max() <= lim
    assert np.array_equal(np.concatenate([a.ravel() for _, a in train_haploid.blob_tensors(w)]), w)


def test_refusals_before_any_allocation(tmp_path, monkeypatch):
    """a file of another kind, a wrong name and a blob of the wrong size raise before the engine is asked for: get_engine is never reached"""
    from nanocaller_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: pytest.fail("the device was touched"))
    with pytest.raises(ValueError, match="kind 0"):
        train_haploid.HaploidSnpTrainer(0, "ONT-HG002")
    with pytest.raises(ValueError):
        train_haploid.HaploidSnpTrainer(0, "no-such-model")
    with pytest.raises(ValueError):
        train_haploid.HaploidSnpTrainer(0, np.zeros(109370, np.float32))
    dip = str(tmp_path / "indel_hap.ncw")
    weights.write_ncw(dip, weights.KIND_INDEL_HAP, 30.0, train_haploid.blob_tensors(np.zeros(158185, np.float32), weights.KIND_INDEL_HAP))
    with pytest.raises(ValueError, match="kind 3"):
        train_haploid.HaploidSnpTrainer(0, dip)
    # (the C entry point's own refusals need a context: tests/test_hap_train_gpu.py::test_refusals)
    assert "nc_hap_train_create" in _lib.EXPORTS and "nc_hap_train_adam" in _lib.EXPORTS


def test_caller_keys(tmp_path, monkeypatch):
    monkeypatch.delenv("NC_HAPLOID_SNP_MODEL", raising=False)
    monkeypatch.delenv("NC_HAPLOID_INDEL_MODEL", raising=False)
    builtin = get_SNP_model("haploid")[0]
    # absent: what the callers had hard-wired, the shipped file and the constant 30
    assert weights.get_haploid_SNP_model({}) == (builtin, 30) and weights.get_haploid_SNP_model(None) == (builtin, 30)
    assert weights.get_haploid_SNP_model(dict(haploid_snp_model="haploid")) == (builtin, 30)
    assert weights.get_haploid_indel_model({}) == weights.get_indel_model("haploid") == weights.get_haploid_indel_model(dict(haploid_indel_model="haploid"))
    snp = str(tmp_path / "snp_hap.ncw")
    weights.write_ncw(snp, KIND_SNP_HAP, 21.5, train_haploid.blob_tensors(train_haploid.xavier_init(KIND_SNP_HAP, 1)))
    ind = str(tmp_path / "indel_hap.ncw")
    weights.write_ncw(ind, weights.KIND_INDEL_HAP, 30.0, train_haploid.blob_tensors(np.zeros(158185, np.float32), weights.KIND_INDEL_HAP))
    # a file: its own train_coverage
    assert weights.get_haploid_SNP_model(dict(haploid_snp_model=snp)) == (snp, 21.5)
    assert weights.get_haploid_indel_model(dict(haploid_indel_model=ind)) == ind
    # the environment is read only without the key
    monkeypatch.setenv("NC_HAPLOID_SNP_MODEL", snp)
    monkeypatch.setenv("NC_HAPLOID_INDEL_MODEL", ind)
    assert weights.get_haploid_SNP_model({}) == (snp, 21.5) and weights.get_haploid_SNP_model(dict(haploid_snp_model="haploid")) == (builtin, 30)
    assert weights.get_haploid_indel_model({}) == ind
    # a given key is never ignored: a missing file, a file of another kind and a diploid model's name raise
    for bad, exc in ((str(tmp_path / "missing.ncw"), FileNotFoundError), (ind, ValueError), ("ONT-HG002", ValueError), (get_SNP_model("ONT-HG002")[0], ValueError)):
        with pytest.raises(exc):
            weights.get_haploid_SNP_model(dict(haploid_snp_model=bad))
    for bad, exc in ((str(tmp_path / "missing.ncw"), FileNotFoundError), (snp, ValueError), ("ONT-HG002", ValueError)):
        with pytest.raises(exc):
            weights.get_haploid_indel_model(dict(haploid_indel_model=bad))
    monkeypatch.setenv("NC_HAPLOID_SNP_MODEL", str(tmp_path / "missing.ncw"))
    with pytest.raises(FileNotFoundError):
        weights.get_haploid_SNP_model({})


# ------------------------------------------------------------------ the haploid indel model
I = R.indel


def test_indel_forward_pinned_to_oracle():
    from oracle import oracle
    w = I.weights("haploid")
    x, _, _ = I.make_inputs(17)
    ep = oracle.indel_forward(w, x, precision="f64")
    assert ep.shape == (17, 1)
    # (1e-9 on top of the half ulp of float32 that the oracle's float32 output array costs)
    assert np.abs(I.sigmoids(w, x) - ep.reshape(-1).astype(np.float64)).max() < 2.0 ** -25 + 1e-9


@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_no_listed_case_is_saturated(wname):
    """every (weight set, n) of the device comparisons, with the mask and without, and the trajectory's five masks at their initial weights:
    the sigmoid of every site stays more than 1e-4 away from 0 and from 1"""
    w = I.weights(wname)
    lo, hi = 1.0, 0.0
    cases = [I.make_inputs(n) for n in I.SIZES]
    runs = [(x, m, I.KEEP) for x, _, m in cases] + [(x, None, 1.0) for x, _, _ in cases]
    runs += [(cases[3][0], I.make_inputs(64, seed=50 + t)[2], I.KEEP) for t in range(5)]
    for x, m, keep in runs:
        p = I.sigmoids(w, x, m, keep)
        assert p.min() > I.SATURATED and p.max() < 1 - I.SATURATED, (wname, x.shape[0], keep, p.min(), p.max())
        lo, hi = min(lo, p.min()), max(hi, p.max())
    print("%s: sigmoids within [%.2e, 1 - %.2e]" % (wname, lo, 1 - hi))
    for n in I.SIZES[1:]:
        assert set(I.make_inputs(n)[1].tolist()) == {0, 1}


def test_indel_gradient_against_finite_differences():
    w = train_haploid.xavier_init(weights.KIND_INDEL_HAP, 3).astype(np.float64)
    x, lab, mask = I.make_inputs(3)
    _, g = I.loss_grad(w, x, lab, mask, 0.5)
    rng = np.random.default_rng(5)

    def cost(wv):
        p = I.split(wv)
        return I.cost(p, I.forward(p, x, mask, 0.5), lab)["cost"].item()

    for name, off, size, _ in I.segments():
        for i in rng.choice(size, min(5, size), replace=False):
            h = 1e-6
            wp, wm = w.copy(), w.copy()
            wp[off + i] += h
            wm[off + i] -= h
            fd = (cost(wp) - cost(wm)) / (2 * h)
            err = abs(fd - g[off + i]) / max(abs(g[off + i]), 1e-3 * np.abs(g[off:off + size]).max())
            assert err < 1e-6, (name, int(i), fd, g[off + i])
    assert I.adam_step is not None and np.allclose(I.adam_step(np.ones(2), np.zeros(2), np.zeros(2), np.array([0.5, -2.0]), 1, 0.01)[0],
                                                   R.adam_step(np.ones(2), np.zeros(2), np.zeros(2), np.array([0.5, -2.0]), 1, 0.01)[0], rtol=0, atol=0)


@pytest.fixture(scope="module")
def indel_probe_cases():
    out = {}
    for wname in I.WEIGHT_SETS:
        w = I.weights(wname)
        x, lab, mask = I.make_inputs(64)
        out[wname] = (w, x, lab, mask, I.loss_grad(w, x, lab, mask, I.KEEP))
    return out


def _indel_breaks(wname, l2, g, want):
    e = I.rel_errors(g, want[1])
    le = np.abs(l2 - want[0]) / np.abs(want[0])
    bound = I.grad_bound(wname, 64)
    return max(e.values()) > bound or le.max() > bound


INDEL_PROBES_BLIND = {
    ("xavier3", "reg_bias"): "Xavier initialisation has zero biases: regularising them adds nothing to the cost or its gradient",
}


@pytest.mark.parametrize("variant", ["no_reg", "reg_bias", "mask_first", "no_inv_keep", "inverted", "bce_1mp"])
@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_probe_sharpness(indel_probe_cases, wname, variant):
    w, x, lab, mask, want = indel_probe_cases[wname]
    assert not _indel_breaks(wname, *I.loss_grad(w, x, lab, mask, I.KEEP), want)
    l2, g = I.loss_grad(w, x, lab, mask, I.KEEP, variant=variant)
    e = I.rel_errors(g, want[1])
    print(wname, variant, "largest per-tensor error %.2e (%s), bound %.1e" % (max(e.values()), max(e, key=e.get), I.grad_bound(wname, 64)))
    assert _indel_breaks(wname, l2, g, want) == ((wname, variant) not in INDEL_PROBES_BLIND), variant


@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_probe_sharpness_adam_eps(wname):
    """torch's eps placement breaks the trajectory comparison of the device tests, on both weight sets"""
    w = I.weights(wname)
    x, lab, _ = I.make_inputs(64)
    masks = [I.make_inputs(64, seed=50 + t)[2] for t in range(5)]
    _, w_tf = I.trajectory(w, x, lab, masks, I.KEEP, I.TRAJ_LR)
    _, w_torch = I.trajectory(w, x, lab, masks, I.KEEP, I.TRAJ_LR, torch_eps=True)
    w0 = np.asarray(w, np.float64)
    worst = max(I.rel_errors(w_torch - w0, w_tf - w0).values())
    print("%s: torch's eps placement moves delta w by %.2e, bound %.1e" % (wname, worst, I.traj_bound(wname)))
    assert worst > I.traj_bound(wname)


@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_measured_noise_is_what_the_bounds_say(wname):
    """every case of the table measured again (the cases are small), and the trajectory figure"""
    for n in I.SIZES:
        worst, _ = I.measure_noise(wname, n)
        print("%s n = %d: float32 against float64 %.2e (table %.2e)" % (wname, n, worst, I.GRAD_F32_NOISE[(wname, n)]))
        assert 0.3 * I.GRAD_F32_NOISE[(wname, n)] <= worst <= 3 * I.GRAD_F32_NOISE[(wname, n)]
    traj = I.measure_traj_noise(wname)
    assert 0.3 * I.TRAJ_F32_NOISE[wname] <= traj <= 3 * I.TRAJ_F32_NOISE[wname]
    fwd = I.measure_forward_noise(wname)
    assert 0.3 * I.FWD_F32_NOISE[wname] <= fwd <= 3 * I.FWD_F32_NOISE[wname]
    assert set(I.GRAD_F32_NOISE) == {(s, c) for s in I.WEIGHT_SETS for c in I.SIZES}


INDEL_VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
    "c1\t1000\t.\tA\tAT\t.\tPASS\t.\tGT\t1",                         # an indel, haploid genotype
    "c1\t1500\t.\tA\tG\t.\tPASS\t.\tGT\t1",                          # a SNP: not a record of the rule
    "c1\t2000\t.\tACGTACGTACGTA\tA\t.\tPASS\t.\tGT:DP\t1|1:30",      # an indel, long
    "c1\t4000\t.\tAT\tA\t.\tPASS\t.\tGT\t0/0",                       # says there is no indel: no record
    "c1\t5000\t.\tAT\tA\t.\tPASS\t.\tGT\t./.",                       # an indel without a usable genotype
    "c1\t6000\t.\tAT\tA\t.\tPASS\t.\tGT\t1/1",                       # outside the BED
    "c2\t1000\t.\tA\tAC\t.\tPASS\t.\tGT\t1",
])


def test_indel_labelling_rule():
    from nanocaller_amd.train_indel import CLASS_UNKNOWN
    tp, tc, tl = train_haploid.parse_haploid_truth_indels(INDEL_VCF, "c1")
    assert tp.tolist() == [1000, 2000, 4000, 5000, 6000] and tc.tolist() == [1, 1, 0, CLASS_UNKNOWN, 1] and tl.tolist() == [0, 1, 0, 0, 0]
    iv = train_haploid.parse_bed("c1\t0\t5500\nc1\t7000\t9000\n", "c1")
    pos = np.array([100,      # no record in [100, 228): 0
                    960,      # record 1000 at offset 40: inside the reach -> 1
                    959,      # record 1000 at offset 41: only beyond 40 -> dropped
                    1000,     # offset 0 -> 1
                    873,      # offset 127, the window's last column: beyond 40 -> dropped
                    872,      # offset 128: outside the window -> 0
                    1990,     # -> 1
                    3990,     # a 0/0 record: no record -> 0
                    4990,     # a record without a usable genotype -> dropped
                    5990,     # an indel, but outside the BED
                    7500])    # inside the second interval, no record -> 0
    idx, lab, dropped = train_haploid.label_haploid_indel_sites(pos, tp, tc, iv, neg_ratio=None)
    assert pos[idx].tolist() == [100, 960, 1000, 872, 1990, 3990, 7500] and lab.tolist() == [0, 1, 1, 0, 1, 0, 0] and lab.dtype == np.uint8
    assert dropped == dict(outside_bed=1, beyond_reach=2, no_genotype=1, negatives_subsampled=0) and set(dropped) == set(train_haploid.INDEL_DROP_KEYS)
    idx2, lab2, _ = train_haploid.label_haploid_indel_sites(pos, tp, tc, None, neg_ratio=None)
    assert pos[idx2].tolist() == [100, 960, 1000, 872, 1990, 3990, 5990, 7500] and lab2[6] == 1
    # three class-1 sites, four class-0 sites: neg_ratio 0.5 keeps one of them, the same one for the same seed
    i1, l1, d1 = train_haploid.label_haploid_indel_sites(pos, tp, tc, iv, neg_ratio=0.5, seed=3)
    i2, _, _ = train_haploid.label_haploid_indel_sites(pos, tp, tc, iv, neg_ratio=0.5, seed=3)
    assert i1.tolist() == i2.tolist() and len(i1) == 4 and int((l1 == 0).sum()) == 1 and d1["negatives_subsampled"] == 3
    i0, l0, _ = train_haploid.label_haploid_indel_sites(pos, np.zeros(0, np.int64), np.zeros(0, np.uint8), iv, neg_ratio=2.0)
    assert len(i0) == 10 and not l0.any()


def test_indel_xavier_init_and_refusals(tmp_path, monkeypatch):
    w = train_haploid.xavier_init(weights.KIND_INDEL_HAP, 3)
    assert w.shape == (I.NPAR,) and w.dtype == np.float32 and not np.array_equal(w, train_haploid.xavier_init(weights.KIND_INDEL_HAP, 4))
    for name, off, size, is_kernel in I.segments():
        assert (np.abs(w[off:off + size]).max() > 0) == is_kernel, name
    t = dict(train_haploid.blob_tensors(w, weights.KIND_INDEL_HAP))
    assert t["fc1.k"].shape == (4464, 32) and t["fc3.k"].shape == (24, 1)
    assert np.array_equal(np.concatenate([a.ravel() for _, a in train_haploid.blob_tensors(w, weights.KIND_INDEL_HAP)]), w)
    from nanocaller_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: pytest.fail("the device was touched"))
    for bad in ("ONT-HG002", "no-such-model", get_SNP_model("haploid")[0], np.zeros(634420, np.float32)):
        with pytest.raises(ValueError):
            train_haploid.HaploidIndelTrainer(0, bad)
    assert "nc_hap_indel_train_create" in _lib.EXPORTS and "nc_hap_indel_train_adam" in _lib.EXPORTS

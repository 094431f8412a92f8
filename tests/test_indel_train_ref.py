"""CPU-only checks of the indel trainer's reference computation (tests/indel_train_ref.py) and of the labelling rule
(nanocaller_amd/train_indel.py): the restatement is pinned to the oracle's forward, its gradient to finite differences, its Adam to the
written-out formula; each mistake the device comparison is meant to catch breaks that comparison when made in the restatement itself."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import indel_train_ref as R  # noqa: E402
from nanocaller_amd import train_indel  # noqa: E402

KEEP = 0.5
WNAMES = ["ONT-HG002", "xavier3"]


def test_weight_sets():
    assert np.array_equal(R.weight_set("xavier3"), train_indel.xavier_init(3))
    assert R.weight_set("ONT-HG002").shape == (R.NPAR,) == R.weight_set("xavier3").shape
    assert R.segments()[-1][1] + R.segments()[-1][2] == R.NPAR and len(R.segments()) == 16


def test_inputs_look_like_the_pipelines():
    x, lab, mask = R.make_inputs(17)
    assert x.shape == (17, 15, 128, 2) and x.dtype == np.float32 and lab.dtype == np.uint8 and mask.shape == (17, 32)
    g = x.reshape(17, 3, 5, 128, 2).astype(np.float64)
    ch1 = g[..., 1]
    assert set(np.unique(ch1)) == {0.0, 1.0} and set(np.unique(ch1.sum(2))) == {0.0, 1.0}       # a one-hot reference row, or none
    assert np.abs((g[..., 0] + ch1).sum(2) - 1.0).max() < 1e-6 and (g[..., 0] + ch1).min() > -1e-7  # a distribution over the five rows
    assert set(lab[:4].tolist()) == {0, 1, 2, 3} and set(np.unique(mask)) == {0, 1}
    assert all(np.array_equal(a, b) for a, b in zip(R.make_inputs(17), R.make_inputs(17)))


@pytest.mark.parametrize("wname", WNAMES)
def test_forward_pinned_to_oracle(wname):
    from oracle import oracle
    w = R.weight_set(wname)
    x, _, _ = R.make_inputs(17)
    out = R.forward(R.split(w), x)
    ep = oracle.indel_forward(w, x, precision="f64")
    # the oracle computes in float64 but hands its results back as float32 arrays: the agreement asked for is 1e-9, on top of the
    # half ulp of float32 below 1 (2^-25 = 3e-8) that this rounding of the oracle's output costs
    assert np.abs(out["probs"].numpy() - ep.astype(np.float64)).max() < 2.0 ** -25 + 1e-9


def test_gradient_against_finite_differences():
    w = R.weight_set("xavier3").astype(np.float64)
    x, lab, mask = R.make_inputs(3)
    _, g = R.loss_grad(w, x, lab, mask, KEEP)
    rng = np.random.default_rng(5)

    def cost(wv):
        p = R.split(wv)
        return R.cost(p, R.forward(p, x, mask, KEEP), lab)["cost"].item()

    worst = 0.0
    for name, off, size, _ in R.segments():
        for i in rng.choice(size, min(4, size), replace=False):
            # SELU has a kink at zero, and a bias moves every pre-activation of its channel: a step of 1e-5 carries a few of the 280,000
            # across it (errors of 1e-3); with 1e-6 none crosses and the rounding of the cost (1e-16 / 1e-6) is still far below the bound
            h = 1e-6
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


# the size each weight set is probed at: xavier(3)'s n = 64 figure holds a SELU branch flip (indel_train_ref.py), which makes its bound 15 times
# wider than ONT-HG002's and too wide to see a regulariser of gamma = 1e-5 (5.7e-05 on the gradient, 5.3e-04 on the cost against 7.1e-04)
PROBE_N = {"ONT-HG002": 64, "xavier3": 17}


@pytest.fixture(scope="module")
def probe_case():
    out = {}
    for wname in WNAMES:
        w = R.weight_set(wname)
        x, lab, mask = R.make_inputs(PROBE_N[wname])
        out[wname] = (w, x, lab, mask, R.loss_grad(w, x, lab, mask, KEEP))
    return out


def _breaks(wname, l2, g, want):
    """what test_gradient of the device tests asserts, as a predicate"""
    e = R.rel_errors(g, want[1])
    le = np.abs(l2 - want[0]) / np.abs(want[0])
    bound = R.grad_bound(wname, PROBE_N[wname])
    return max(e.values()) > bound or le.max() > bound


# (xavier(3) has zero biases: regularising them changes nothing there)
PROBES = [(w, v) for w in WNAMES for v in ("no_reg", "reg_bias", "mask_first", "no_scale", "swap12") if (w, v) != ("xavier3", "reg_bias")]


@pytest.mark.parametrize("wname,variant", PROBES)
def test_probe_sharpness(probe_case, wname, variant):
    w, x, lab, mask, want = probe_case[wname]
    assert not _breaks(wname, *R.loss_grad(w, x, lab, mask, KEEP), want)
    l2, g = R.loss_grad(w, x, lab, mask, KEEP, variant=variant)
    e = R.rel_errors(g, want[1])
    print(wname, variant, "largest per-tensor error %.2e (%s), bound %.1e" % (max(e.values()), max(e, key=e.get), R.grad_bound(wname, PROBE_N[wname])))
    assert _breaks(wname, l2, g, want), variant


def test_probe_sharpness_adam_eps():
    """torch's eps placement breaks the trajectory comparison of the device tests on ONT-HG002 (on xavier(3) every gradient is far above eps
    and the two placements give the same steps within float32's own figure: indel_train_ref.py says so beside the constants)"""
    w = R.weight_set("ONT-HG002")
    x, lab, _ = R.make_inputs(64)
    masks = [R.make_inputs(64, seed=50 + t)[2] for t in range(5)]
    _, w_tf = R.trajectory(w, x, lab, masks, KEEP, R.TRAJ_LR)
    _, w_torch = R.trajectory(w, x, lab, masks, KEEP, R.TRAJ_LR, torch_eps=True)
    w0 = np.asarray(w, np.float64)
    assert max(R.rel_errors(w_torch - w0, w_tf - w0).values()) > R.traj_bound("ONT-HG002")


def test_measured_noise_is_what_the_bounds_say():
    """the float32 figure behind grad_bound, measured again at n = 64 (the other cases: tools/bench_train_indel.py --noise)"""
    w = R.weight_set("ONT-HG002")
    x, lab, mask = R.make_inputs(64)
    l64, g64 = R.loss_grad(w, x, lab, mask, KEEP)
    l32, g32 = R.loss_grad(w, x, lab, mask, KEEP, dtype=torch.float32)
    worst = max(R.rel_errors(g32, g64).values())
    print("float32 against float64 at n = 64: %.2e" % worst)
    # (the float32 sums depend a little on how many threads torch's kernels split them over)
    assert 0.3 * R.GRAD_F32_NOISE[("ONT-HG002", 64)] <= worst <= 3 * R.GRAD_F32_NOISE[("ONT-HG002", 64)]


@pytest.mark.parametrize("wname", WNAMES)
def test_no_dead_tensor_and_no_saturated_output(wname):
    """the device test's precheck, on the CPU at its largest size"""
    w = R.weight_set(wname)
    x, lab, mask = R.make_inputs(130)
    _, g = R.loss_grad(w, x, lab, mask, KEEP)
    for name, off, size, _ in R.segments():
        assert np.linalg.norm(g[off:off + size]) > 0, name
    p = R.forward(R.split(w), x, mask, KEEP)["probs"].numpy()
    assert (np.minimum(p, 1 - p) > 1e-6).any(0).all()


VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
    "c1\t1000\t.\tA\tAT\t.\tPASS\t.\tGT\t0/1",                       # class 2
    "c1\t1500\t.\tA\tG\t.\tPASS\t.\tGT\t0/1",                        # a SNP: not a record of the rule
    "c1\t2000\t.\tACGTACGTACGTA\tA\t.\tPASS\t.\tGT:DP\t1|1:30",      # class 1, long (12 bases deleted)
    "c1\t3000\t.\tA\tAT,ATT\t.\tPASS\t.\tGT\t1/2",                   # class 3
    "c1\t3020\t.\tAT\tA\t.\tPASS\t.\tGT\t1|0",                       # class 2, 20 behind the class-3 record
    "c1\t4000\t.\tAT\tA\t.\tPASS\t.\tGT\t0/0",                       # class 0
    "c1\t5000\t.\tAT\tA\t.\tPASS\t.\tGT\t./.",                       # an indel without a usable genotype
    "c1\t6000\t.\tAT\tA\t.\tPASS\t.\tGT\t1/1",                       # outside the BED
    "c2\t1000\t.\tA\tAC\t.\tPASS\t.\tGT\t0/1",
])
BED = "c1\t0\t5500\nc1\t7000\t9000\nc2\t0\t100\n"


def test_labelling_rule():
    tp, tc, tl = train_indel.parse_truth_indels(VCF, "c1")
    assert tp.tolist() == [1000, 2000, 3000, 3020, 4000, 5000, 6000]
    assert tc.tolist() == [2, 1, 3, 2, 0, train_indel.CLASS_UNKNOWN, 1] and tl.tolist() == [0, 1, 0, 0, 0, 0, 0]
    iv = train_indel.parse_bed(BED, "c1")
    pos = np.array([100,      # no record in [100, 228): class 0
                    960,      # record 1000 at offset 40: inside the reach, class 2
                    959,      # record 1000 at offset 41: one class, but only beyond 40 -> ambiguous
                    1000,     # offset 0
                    873,      # record 1000 at offset 127: the last column of the window, beyond 40 -> ambiguous
                    872,      # record 1000 at offset 128: outside the window -> class 0
                    1990,     # class 1
                    2990,     # 3000 (class 3) and 3020 (class 2) -> two classes -> ambiguous
                    3010,     # only 3020 -> class 2
                    3990,     # a 0/0 record within reach: class 0
                    4990,     # a record without a usable genotype -> ambiguous
                    5990,     # class 1 but outside the BED
                    7500])    # inside the second interval, no record
    idx, lab, dropped = train_indel.label_sites(pos, tp, tc, iv, neg_ratio=None)
    assert pos[idx].tolist() == [100, 960, 1000, 872, 1990, 3010, 3990, 7500]
    assert lab.tolist() == [0, 2, 2, 0, 1, 2, 0, 0]
    assert dropped == dict(outside_bed=1, ambiguous=4, negatives_subsampled=0)
    # without a BED the site at 5990 is kept with its class
    idx2, lab2, d2 = train_indel.label_sites(pos, tp, tc, None, neg_ratio=None)
    assert pos[idx2].tolist() == [100, 960, 1000, 872, 1990, 3010, 3990, 5990, 7500] and lab2[7] == 1 and d2["outside_bed"] == 0
    # four labelled sites (960, 1000, 1990, 3010) and four class-0 sites: neg_ratio 0.5 keeps two of them, the same for the same seed
    i1, l1, d1 = train_indel.label_sites(pos, tp, tc, iv, neg_ratio=0.5, seed=3)
    i2, _, _ = train_indel.label_sites(pos, tp, tc, iv, neg_ratio=0.5, seed=3)
    assert i1.tolist() == i2.tolist() and len(i1) == 6 and int((l1 == 0).sum()) == 2 and d1["negatives_subsampled"] == 2
    assert {960, 1000, 1990, 3010} <= set(pos[i1].tolist()) and np.all(np.diff(i1) > 0)
    seeds = {tuple(train_indel.label_sites(pos, tp, tc, iv, neg_ratio=0.5, seed=s)[0].tolist()) for s in range(8)}
    assert len(seeds) > 1
    assert len(train_indel.label_sites(pos, tp, tc, iv, neg_ratio=2.0)[0]) == 8           # fewer class-0 sites than the ratio allows: all kept
    # no truth at all: everything inside the BED is class 0 and nothing is subsampled
    i0, l0, _ = train_indel.label_sites(pos, np.zeros(0, np.int64), np.zeros(0, np.uint8), iv, neg_ratio=2.0)
    assert len(i0) == 12 and not l0.any()


def test_world_truth_is_the_planted_sites():
    from nanocaller_amd.synth import add_indels, make_world
    w = add_indels(make_world(seed=7, length=20_000, depth=12, read_len_scale=0.3), seed=7, het_rate=1 / 300.0)
    pos, cls, lng = train_indel.world_truth(w)
    assert pos.size > 20 and np.all(np.diff(pos) > 0) and set(cls.tolist()) == {2} and 0 < lng.sum() < lng.size
    ev_pos = w.meta["events"][1]
    assert np.isin(pos, ev_pos).mean() > 0.9                                               # (a site no read carries is planted all the same)
    with pytest.raises(ValueError):
        train_indel.world_truth(make_world(seed=7, length=5_000, depth=5))


def test_xavier_init_and_blob_tensors():
    w = train_indel.xavier_init(3)
    assert w.shape == (R.NPAR,) and w.dtype == np.float32 and not np.array_equal(w, train_indel.xavier_init(4))
    for name, off, size, is_kernel in R.segments():
        assert (np.abs(w[off:off + size]).max() > 0) == is_kernel, name
    t = dict(train_indel.blob_tensors(w))
    lim = np.sqrt(6.0 / (19344 + 32))
    assert t["fc1.k"].shape == (19344, 32) and np.abs(t["fc1.k"]).max() <= lim and np.abs(t["fc1.k"]).max() > 0.99 * lim
    assert np.array_equal(np.concatenate([a.ravel() for _, a in train_indel.blob_tensors(w)]), w)


def test_refusals_before_any_allocation():
    """the haploid kind and weight files of another kind raise ValueError without touching the device"""
    from nanocaller_amd.weights import KIND_INDEL_HAP, WEIGHT_DIR, SNP_MODEL_FILES
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, None, kind=KIND_INDEL_HAP)
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, "haploid")
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, os.path.join(WEIGHT_DIR, SNP_MODEL_FILES["ONT-HG002"]))
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, "no-such-model")
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, np.zeros(10, np.float32))

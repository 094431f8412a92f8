"""CPU-only checks of the SNP trainer's reference computation (tests/snp_train_ref.py) and of the labelling rule (nanocaller_amd/train.py):
the restatement is pinned to the oracle's forward, its gradient to finite differences, its Adam to the written-out formula; each mistake the
device comparison is meant to catch breaks that comparison when made in the restatement itself."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import snp_train_ref as R  # noqa: E402
from nanocaller_amd import train  # noqa: E402
from nanocaller_amd.weights import Weights, get_SNP_model  # noqa: E402


def _weights(name):
    return Weights(get_SNP_model(name)[0]).flat


@pytest.mark.parametrize("model", ["ONT-HG002", "CCS-HG002"])
def test_forward_pinned_to_oracle(model):
    from oracle import oracle
    w = _weights(model)
    x, ref, _, _ = R.make_inputs(17)
    scale = np.linspace(0.5, 2.0, 17)
    for sc in (None, scale):
        out = R.forward(R.split(w), x, ref, sc)
        ep, eg = oracle.snp_forward(w, x, ref, np.ones(17) if sc is None else sc, precision="f64")
        # the oracle computes in float64 but hands its results back as float32 arrays: the agreement asked for is 1e-9, on top of the
        # half ulp of float32 below 1 (2^-25 = 3e-8) that this rounding of the oracle's output costs
        assert np.abs(out["probs"].numpy() - ep.astype(np.float64)).max() < 2.0 ** -25 + 1e-9
        assert np.abs(out["gt"].numpy() - eg.astype(np.float64)).max() < 2.0 ** -25 + 1e-9


def test_gradient_against_finite_differences():
    w = train.xavier_init(3).astype(np.float64)
    x, ref, lab, mask = R.make_inputs(3)
    _, g = R.loss_grad(w, x, ref, lab, mask, 0.5)
    rng = np.random.default_rng(5)

    def cost(wv):
        p = R.split(wv)
        return R.cost(p, R.forward(p, x, ref, None, mask, 0.5), lab)["cost"].item()

    worst = 0.0
    for name, off, size, _ in R.segments():
        for i in rng.choice(size, min(5, size), replace=False):
            h = 1e-5
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
        for i in range(4):                                              # the issue's formula, entry by entry
            lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            m2[i] = b1 * m2[i] + (1 - b1) * g[t - 1][i]
            v2[i] = b2 * v2[i] + (1 - b2) * g[t - 1][i] ** 2
            w2[i] -= lr_t * m2[i] / (np.sqrt(v2[i]) + eps)
        assert np.allclose(w, w2, rtol=1e-14, atol=0) and np.allclose(m, m2, rtol=1e-14) and np.allclose(v, v2, rtol=1e-14)
    # first step of TF's form: |dw| = lr |g| / (|g| + eps sqrt(1 - b2)) -- not lr |g| / (|g| + eps), torch's
    w1, _, _ = R.adam_step(np.zeros(1), np.zeros(1), np.zeros(1), np.array([1e-8]), 1, 1.0)
    assert abs(-w1[0] - 1e-8 / (1e-8 + 1e-8 / np.sqrt(1 - 0.999))) < 1e-12


@pytest.fixture(scope="module")
def probe_case():
    w = _weights("ONT-HG002")
    x, ref, lab, mask = R.make_inputs(64)
    return w, x, ref, lab, mask, R.loss_grad(w, x, ref, lab, mask, 0.5)


def _breaks(l6, g, want):
    """what test_gradient of the device tests asserts, as a predicate"""
    e = R.rel_errors(g, want[1])
    le = np.abs(l6 - want[0]) / np.abs(want[0])
    bound = R.grad_bound("ONT-HG002", 64)
    return max(e.values()) > bound or le.max() > bound


@pytest.mark.parametrize("variant", ["no_jacobian", "no_reg", "reg_bias", "mask_first"])
def test_probe_sharpness(probe_case, variant):
    w, x, ref, lab, mask, want = probe_case
    assert not _breaks(*R.loss_grad(w, x, ref, lab, mask, 0.5), want)
    l6, g = R.loss_grad(w, x, ref, lab, mask, 0.5, variant=variant)
    e = R.rel_errors(g, want[1])
    print(variant, "largest per-tensor error %.2e (%s)" % (max(e.values()), max(e, key=e.get)))
    assert _breaks(l6, g, want), variant


def test_probe_sharpness_adam_eps():
    """torch's eps placement breaks the trajectory comparison of the device tests"""
    for w in (_weights("ONT-HG002"), train.xavier_init(3)):
        x, ref, lab, _ = R.make_inputs(64)
        masks = [R.make_inputs(64, seed=50 + t)[3] for t in range(5)]
        _, w_tf = R.trajectory(w, x, ref, lab, masks, 0.5, R.TRAJ_LR)
        _, w_torch = R.trajectory(w, x, ref, lab, masks, 0.5, R.TRAJ_LR, torch_eps=True)
        w0 = np.asarray(w, np.float64)
        assert max(R.rel_errors(w_torch - w0, w_tf - w0).values()) > R.TRAJ_BOUND


def test_measured_noise_is_what_the_bounds_say():
    """the float32 figure behind GRAD_BOUND, measured again at n = 64 (the other cases: tools/bench_train.py --noise)"""
    w = _weights("ONT-HG002")
    x, ref, lab, mask = R.make_inputs(64)
    l64, g64 = R.loss_grad(w, x, ref, lab, mask, 0.5)
    l32, g32 = R.loss_grad(w, x, ref, lab, mask, 0.5, dtype=torch.float32)
    worst = max(R.rel_errors(g32, g64).values())
    print("float32 against float64 at n = 64: %.2e" % worst)
    # (the float32 sums depend a little on how many threads torch's kernels split them over)
    assert 0.3 * R.GRAD_F32_NOISE[("ONT-HG002", 64)] <= worst <= 3 * R.GRAD_F32_NOISE[("ONT-HG002", 64)]


VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1",
    "c1\t10\t.\tA\tG\t.\tPASS\t.\tGT\t0/1",          # het: ref A, alt G
    "c1\t20\t.\tT\tC\t.\tPASS\t.\tGT:DP\t1|1:30",     # hom alt
    "c1\t30\t.\tG\tA,T\t.\tPASS\t.\tGT\t1/2",         # two alts
    "c1\t40\t.\tA\tAT\t.\tPASS\t.\tGT\t0/1",          # insertion: skipped
    "c1\t50\t.\tC\tT\t.\tPASS\t.\tGT\t./.",           # no call: skipped
    "c1\t60\t.\tC\tT\t.\tPASS\t.\tGT\t0/0",           # hom ref
    "c1\t70\t.\tC\tT\t.\tPASS\t.\tGT\t1/0",           # outside the BED
    "c2\t10\t.\tA\tC\t.\tPASS\t.\tGT\t0/1",
])
BED = "c1\t0\t35\nc1\t55\t65\nc2\t0\t100\n"


def test_labelling_rule():
    truth = train.parse_truth_vcf(VCF, "c1")
    assert truth == {10: (1, 0, 1), 20: (0, 3, 3), 30: (1, 0, 2), 60: (0, 3, 3), 70: (1, 2, 3)}
    iv = train.parse_bed(BED, "c1")
    assert iv == [(0, 35), (55, 65)]
    # BED intervals are 0-based half-open: position 35 is inside [0, 35), 36 is not; 56 is the first position of [55, 65)
    assert train.in_bed(iv, [1, 35, 36, 55, 56, 65, 66]).tolist() == [True, True, False, False, True, True, False]
    pos = np.array([5, 10, 12, 20, 25, 30, 33, 36, 58, 60, 62, 70])
    ref = np.array([0, 0, 1, 2, 3, 1, 2, 0, 1, 3, 2, 3])
    idx, lab = train.label_sites(pos, ref, truth, iv, neg_ratio=None)
    assert pos[idx].tolist() == [5, 10, 12, 20, 25, 30, 33, 58, 60, 62]                     # 36 and 70 are outside the intervals
    want = {5: [1, 0, 0, 0, 0], 10: [1, 1, 0, 0, 1], 12: [0, 1, 0, 0, 0], 20: [0, 0, 0, 1, 0], 25: [0, 0, 0, 1, 0], 30: [1, 0, 1, 0, 1],
            33: [0, 0, 1, 0, 0], 58: [0, 1, 0, 0, 0], 60: [0, 0, 0, 1, 0], 62: [0, 0, 1, 0, 0]}
    assert {int(p): r.tolist() for p, r in zip(pos[idx], lab)} == want
    # four truth sites are kept (10, 20, 30, 60); six others: neg_ratio 1 keeps four of them, the same ones for the same seed
    i1, l1 = train.label_sites(pos, ref, truth, iv, neg_ratio=1.0, seed=3)
    i2, _ = train.label_sites(pos, ref, truth, iv, neg_ratio=1.0, seed=3)
    assert i1.tolist() == i2.tolist() and len(i1) == 8 and {10, 20, 30, 60} <= set(pos[i1].tolist())
    assert all(l1[j].tolist() == want[int(pos[i])] for j, i in enumerate(i1))
    assert len(train.label_sites(pos, ref, truth, iv, neg_ratio=0.5)[0]) == 6
    assert len(train.label_sites(pos, ref, truth, None, neg_ratio=None)[0]) == 12


def test_xavier_init_and_blob_tensors():
    w = train.xavier_init(3)
    assert w.shape == (109370,) and w.dtype == np.float32 and np.array_equal(w, train.xavier_init(3)) and not np.array_equal(w, train.xavier_init(4))
    for name, off, size, is_kernel in R.segments():
        seg = w[off:off + size]
        assert (np.abs(seg).max() > 0) == is_kernel, name
    t = dict(train.blob_tensors(w))
    lim = np.sqrt(6.0 / (1728 + 48))
    assert t["fc1.k"].shape == (1728, 48) and np.abs(t["fc1.k"]).max() <= lim and np.abs(t["fc1.k"]).max() > 0.99 * lim
    assert np.array_equal(np.concatenate([a.ravel() for _, a in train.blob_tensors(w)]), w)

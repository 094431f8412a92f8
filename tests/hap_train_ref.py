"""The reference computation of the haploid trainers' tests (the haploid indel model's half is tests/hap_indel_train_ref.py, imported below as
`indel`): the haploid SNP model (the deployed forward, model_architect_SNP_haploid.py:33-53:
the diploid trunk through fc1, dropout behind fc1's SELU, fc2, fc3 on [fc2 | reference one-hot] WITH its SELU, softmax over the four SELU
outputs), the training loss (batch mean of the 4-way cross-entropy of the site's base + gamma * sum over the kernels of |W|^2 / 2) and Adam in
TensorFlow's form, in float64 (or float32) with torch autograd on the CPU.  Test code: the trainer itself never calls torch.nn.

`variant` switches one deliberate mistake on (tests/test_hap_train_ref.py::test_probe_sharpness shows the comparison sees each):
  no_reg       no regulariser
  reg_bias     the regulariser also over the biases
  mask_first   the dropout mask before fc1's SELU instead of behind it
  no_inv_keep  kept units not multiplied by 1 / keep
  no_fc3_selu  the backward pass skips SELU' of fc3 (the forward keeps its SELU)
  no_onehot    the reference one-hot's rows of fc3's kernel get no gradient
  acgt         the label's classes read in A, C, G, T order instead of A, G, T, C
"""
import numpy as np
import torch
import torch.nn.functional as F

from nanocaller_amd.weights import KIND_SNP_HAP, LAYER_SPECS

import hap_indel_train_ref as indel  # noqa: F401  (the haploid indel model's reference: tests use it as R.indel)

SPECS = LAYER_SPECS[KIND_SNP_HAP]
LOSS_KEYS = ("cost", "CE")
GAMMA = 1e-3
KEEP = 0.5
SIZES = (1, 3, 17, 64, 300, 4160)
WEIGHT_SETS = ("haploid", "xavier3")
SATURATED = 1e-4              # a label probability this close to 0 or 1: the relative error of its gradient means nothing

# ---- bounds of the device comparisons (tests/test_hap_train_gpu.py), set by measurement, not by what the device gives: the same restatement
# evaluated in float32 on the CPU against float64, on the inputs of make_inputs() (keep 0.5) and both weight sets.  Per case: the largest
# relative L2 error over the 16 parameter tensors.  "17s": n = 17 with a coverage scale of 0.5 .. 2.  tools/bench_train_haploid.py --noise
# prints this table; profiles/haploid_train.json keeps it.  The bound of a case is 10 x its figure: the margin is for a different summation
# order over sites and taps.  It also bounds the losses (their own float32 error is 1e-8 .. 8e-7).  Most cases sit at 5e-7 to 4e-6; the
# outliers (n = 300 and 4160) are float32 itself, as in tests/snp_train_ref.py: a conv1 pre-activation within rounding of zero lands on the
# other branch of the SELU, whose derivatives differ by a factor 1.67.
GRAD_F32_NOISE = {
    ("haploid", 1): 1.77e-6, ("haploid", 3): 4.19e-6, ("haploid", 17): 5.92e-7, ("haploid", 64): 1.27e-6, ("haploid", 300): 1.18e-5,
    ("haploid", 4160): 1.13e-5, ("haploid", "17s"): 4.54e-7,
    ("xavier3", 1): 4.72e-7, ("xavier3", 3): 8.87e-7, ("xavier3", 17): 2.88e-6, ("xavier3", 64): 1.67e-6, ("xavier3", 300): 1.70e-6,
    ("xavier3", 4160): 3.72e-4, ("xavier3", "17s"): 1.29e-6,
}

# The table is one machine's (the CPU these tests were written on, torch's default thread count).  The cases up to n = 64 and "17s" are
# re-measured by test_measured_noise_is_what_the_bounds_say wherever the suite runs; n = 300 and 4160 are not: their figures are one or a few
# SELU branch flips, and which pre-activations flip moves with the number of threads the float32 sums are split over (the same case measured
# on another machine: 4.4e-6 at n = 300 on CHM13, profiles/haploid_train.json).
PINNED_CASES = (1, 3, 17, 64, "17s")

# the forward's own figure: the largest |p_f32 - p_f64| over the probabilities at n = 300, plain, with the coverage scale and with the mask
FWD_F32_NOISE = {"haploid": 5.76e-7, "xavier3": 1.10e-6}

# five Adam steps at n = 64, lr 1e-3, fixed masks: per-tensor ||dw_f32 - dw_f64|| / ||dw_f64||, the largest over the tensors, per weight set
TRAJ_F32_NOISE = {"haploid": 1.81e-4, "xavier3": 6.99e-4}
TRAJ_LR = 1e-3


def grad_bound(wname, case):
    return 10 * GRAD_F32_NOISE[(wname, case)]


def traj_bound(wname):
    return 10 * TRAJ_F32_NOISE[wname]


def forward_bound(wname):
    return 10 * FWD_F32_NOISE[wname]


def weights(wname):
    """the two weight sets of the comparisons: the shipped CHM13 file and Xavier-uniform from seed 3"""
    from nanocaller_amd import train_haploid
    from nanocaller_amd.weights import Weights, get_SNP_model
    if wname == "haploid":
        return Weights(get_SNP_model("haploid")[0]).flat
    assert wname == "xavier3", wname
    return train_haploid.xavier_init(KIND_SNP_HAP, 3)


def segments():
    """-> [(tensor name, offset, size, is_kernel)] of the 16 parameter tensors in blob order"""
    out, off = [], 0
    for name, shp in SPECS:
        nk = int(np.prod(shp))
        out.append((name + ".k", off, nk, True))
        out.append((name + ".b", off + nk, shp[-1], False))
        off += nk + shp[-1]
    return out


def split(flat, dtype=torch.float64, requires_grad=False):
    """canonical blob -> dict name -> (kernel, bias) torch tensors"""
    p, off = {}, 0
    flat = np.asarray(flat)
    for name, shp in SPECS:
        nk = int(np.prod(shp))
        k = torch.tensor(flat[off:off + nk].reshape(shp), dtype=dtype, requires_grad=requires_grad)
        b = torch.tensor(flat[off + nk:off + nk + shp[-1]], dtype=dtype, requires_grad=requires_grad)
        p[name] = (k, b)
        off += nk + shp[-1]
    return p


def join(p, grad=False):
    parts = []
    for name, _ in SPECS:
        for t in p[name]:
            parts.append((t.grad if grad else t.detach()).reshape(-1))
    return torch.cat(parts).numpy()


def _conv(x, kb, padding=0, stride=1):
    k, b = kb
    return F.conv2d(x, k.permute(3, 2, 0, 1), b, stride=stride, padding=padding)


class _SeluForwardOnly(torch.autograd.Function):
    """SELU whose backward pass forgets its derivative (the no_fc3_selu probe)"""

    @staticmethod
    def forward(ctx, x):
        return F.selu(x)

    @staticmethod
    def backward(ctx, g):
        return g


def forward(p, x, ref_code, scale=None, mask=None, keep=1.0, variant=None):
    """x [n,5,41,5], ref_code [n] -> dict a ([n,4] SELU outputs of fc3, the softmax's logits), probs [n,4]"""
    dtype = p["fc1"][0].dtype
    x = torch.as_tensor(np.asarray(x), dtype=dtype).clone()
    if scale is not None:
        x[:, 1:, :, :4] = x[:, 1:, :, :4] * torch.as_tensor(np.asarray(scale), dtype=dtype).reshape(-1, 1, 1, 1)
    n = x.shape[0]
    xin = x.permute(0, 3, 1, 2)
    a1 = F.selu(torch.cat([_conv(xin, p["conv1_1"], (0, 2)), _conv(xin, p["conv1_2"], (2, 0)), _conv(xin, p["conv1_3"], (2, 2))], 1))
    a2 = F.selu(_conv(a1, p["conv2"], 0, (1, 2)))
    a3 = F.selu(_conv(a2, p["conv3"], 0, (1, 2)))
    flat = a3.permute(0, 2, 3, 1).reshape(n, -1)                       # H, W, C order
    mk = None
    if mask is not None and keep != 1.0:
        mk = torch.as_tensor(np.asarray(mask), dtype=dtype) / (1.0 if variant == "no_inv_keep" else keep)
    pre = flat @ p["fc1"][0] + p["fc1"][1]
    if variant == "mask_first" and mk is not None:
        f1m = F.selu(pre * mk)
    else:
        f1m = F.selu(pre)
        if mk is not None:
            f1m = f1m * mk
    fc2 = F.selu(f1m @ p["fc2"][0] + p["fc2"][1])
    onehot = F.one_hot(torch.as_tensor(np.asarray(ref_code)).long(), 4).to(dtype)
    k3, b3 = p["fc3"]
    if variant == "no_onehot":
        k3 = torch.cat([k3[:16], k3[16:].detach()], 0)
    z = torch.cat([fc2, onehot], 1) @ k3 + b3
    a = _SeluForwardOnly.apply(z) if variant == "no_fc3_selu" else F.selu(z)
    return dict(a=a, probs=torch.softmax(a, 1))


ACGT_OF_AGTC = (0, 3, 1, 2)   # the acgt probe: a label written A0 G1 T2 C3 read as an index into A, C, G, T (1 -> C = 3, 2 -> G = 1, 3 -> T = 2)


def cost(p, out, labels, gamma=GAMMA, variant=None):
    """labels [n] = the site's base A0 G1 T2 C3 -> dict cost, CE (torch scalars)"""
    lab = torch.as_tensor(np.asarray(labels)).long()
    if variant == "acgt":
        lab = torch.tensor(ACGT_OF_AGTC)[lab]
    r = {"CE": F.cross_entropy(out["a"], lab)}
    reg = 0.0
    if variant != "no_reg":
        for name, _ in SPECS:
            reg = reg + 0.5 * (p[name][0] ** 2).sum()
            if variant == "reg_bias":
                reg = reg + 0.5 * (p[name][1] ** 2).sum()
    r["cost"] = r["CE"] + gamma * reg
    return r


def loss_grad(w_flat, x, ref_code, labels, mask=None, keep=1.0, gamma=GAMMA, scale=None, dtype=torch.float64, variant=None):
    """-> (cost, CE float64 [2], gradient blob float64 [108308])"""
    p = split(w_flat, dtype, requires_grad=True)
    c = cost(p, forward(p, x, ref_code, scale, mask, keep, variant), labels, gamma, variant)
    c["cost"].backward()
    return np.array([c[k].item() for k in LOSS_KEYS]), join(p, grad=True).astype(np.float64)


def label_probs(w_flat, x, ref_code, labels, mask=None, keep=1.0, scale=None):
    """the softmax probability of each site's label, float64 [n]: the quantity the no-saturation condition is about"""
    out = forward(split(w_flat), x, ref_code, scale, mask, keep)
    return out["probs"].detach().numpy()[np.arange(len(labels)), np.asarray(labels, np.int64)]


def adam_step(w, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, torch_eps=False):
    """step t (1-based) of Adam in TensorFlow's form; torch_eps: torch's placement, eps added to sqrt(v / (1 - beta2^t))"""
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    if torch_eps:
        w = w - lr / (1 - beta1 ** t) * m / (np.sqrt(v / (1 - beta2 ** t)) + eps)
    else:
        w = w - lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m / (np.sqrt(v) + eps)
    return w, m, v


def trajectory(w_flat, x, ref_code, labels, masks, keep, lr, gamma=GAMMA, dtype=torch.float64, torch_eps=False):
    """len(masks) Adam steps -> (losses [steps][2], final weights float64)"""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    w = np.asarray(w_flat).astype(np_dt)
    m, v = np.zeros_like(w), np.zeros_like(w)
    losses = []
    for t, mask in enumerate(masks, 1):
        l2, g = loss_grad(w, x, ref_code, labels, mask, keep, gamma, dtype=dtype)
        losses.append(l2)
        w, m, v = adam_step(w, m, v, g.astype(np_dt), np_dt(t), np_dt(lr), np_dt(0.9), np_dt(0.999), np_dt(1e-8), torch_eps)
        w, m, v = w.astype(np_dt), m.astype(np_dt), v.astype(np_dt)
    return np.array(losses), w.astype(np.float64)


def rel_errors(got, want):
    """per parameter tensor ||got - want||_2 / ||want||_2 -> dict name -> float"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return {name: float(np.linalg.norm(got[o:o + k] - want[o:o + k]) / np.linalg.norm(want[o:o + k])) for name, o, k, _ in segments()}


def make_inputs(n, seed=11, keep=KEEP):
    """integer tensors drawn as tests/snp_train_ref.py draws them, but in -1..1, all four reference bases, all four bases among the labels
    (n >= 4), a seeded 0/1 mask.  The range is what keeps every listed case unsaturated: this model's softmax sits on SELU outputs, which
    have no upper limit, and at -8..8 (the diploid tests' range) Xavier weights push the label's probability to 3e-7 and to 1 - 5e-6 at
    n = 4160; at -2..2 the closest is 1.2e-4, at -1..1 2.8e-4 from 0 and 4.4e-3 from 1 over all cases of both weight sets
    (tests/test_hap_train_ref.py::test_no_listed_case_is_saturated proves it)."""
    rng = np.random.default_rng(seed + 1000 * n)
    x = rng.integers(-1, 2, (n, 5, 41, 5)).astype(np.float32)
    ref = (np.arange(n) % 4).astype(np.int32)
    labels = rng.integers(0, 4, n).astype(np.uint8)
    if n >= 4:
        labels[:4] = (1, 2, 3, 0)                                       # (never the site's own reference base, which is arange % 4)
    mask = (rng.random((n, 48)) < keep).astype(np.uint8)
    return x, ref, labels, mask


def measure_noise(wname, case):
    """the float32-against-float64 figure of one case of GRAD_F32_NOISE -> (largest per-tensor error, largest loss error)"""
    n = 17 if case == "17s" else case
    x, ref, lab, mask = make_inputs(n)
    scale = np.linspace(0.5, 2.0, n) if case == "17s" else None
    w = weights(wname)
    l64, g64 = loss_grad(w, x, ref, lab, mask, KEEP, scale=scale)
    l32, g32 = loss_grad(w, x, ref, lab, mask, KEEP, scale=scale, dtype=torch.float32)
    return max(rel_errors(g32, g64).values()), float((np.abs(l32 - l64) / np.abs(l64)).max())


def measure_traj_noise(wname):
    x, ref, lab, _ = make_inputs(64)
    masks = [make_inputs(64, seed=50 + t)[3] for t in range(5)]
    w = weights(wname)
    _, w64 = trajectory(w, x, ref, lab, masks, KEEP, TRAJ_LR)
    _, w32 = trajectory(w, x, ref, lab, masks, KEEP, TRAJ_LR, dtype=torch.float32)
    w0 = np.asarray(w, np.float64)
    return max(rel_errors(w32 - w0, w64 - w0).values())


def measure_forward_noise(wname, n=300):
    """the figure of FWD_F32_NOISE: float32 against float64 probabilities, the largest over the three forms the device test runs"""
    w = weights(wname)
    x, ref, _, mask = make_inputs(n)
    worst = 0.0
    for sc, m, keep in ((None, None, 1.0), (np.linspace(0.5, 2.0, n), None, 1.0), (None, mask, KEEP)):
        p64 = forward(split(w), x, ref, sc, m, keep)["probs"].numpy()
        p32 = forward(split(w, torch.float32), x, ref, sc, m, keep)["probs"].numpy().astype(np.float64)
        worst = max(worst, float(np.abs(p32 - p64).max()))
    return worst

"""The reference computation of the indel trainer's tests: the diploid indel model (the deployed forward, model_architect_indel.py:28-48: three
conv1 branches, conv2, conv3, fc1, dropout behind fc1's SELU, fc2, fc3, softmax), the training loss (misc/training/model_architect_indel.py:
101-126) and Adam in TensorFlow's form, in float64 (or float32) with torch autograd on the CPU.  Test code: the trainer itself never calls
torch.nn.

`variant` switches one deliberate mistake on (tests/test_indel_train_ref.py::test_probe_sharpness shows the comparison sees each):
  no_reg       no regulariser
  reg_bias     the regulariser also over the biases
  mask_first   the dropout mask before fc1's SELU instead of behind it
  no_scale     kept units are not multiplied by 1 / keep
  swap12       classes 1 and 2 swapped in the one-hot label
(trajectory(torch_eps=True): Adam with torch's eps placement)
"""
import numpy as np
import torch
import torch.nn.functional as F

from nanocaller_amd.weights import KIND_INDEL, LAYER_SPECS

SPECS = LAYER_SPECS[KIND_INDEL]
LOSS_KEYS = ("cost", "CE")
GAMMA = 1e-5
NPAR = 634420

# ---- bounds of the device comparisons (tests/test_indel_train_gpu.py), set by measurement, not by what the device gives:
# the same restatement evaluated in float32 on the CPU against float64, on the inputs of make_inputs() (keep 0.5) and both weight sets.  Per
# case: the largest relative L2 error over the 16 parameter tensors (the two losses are always closer: 5.1e-08 .. 1.5e-06, below the tensors'
# figure of the same case).  measure_noise() computes this table, tools/bench_train_indel.py --noise prints it, profiles/indel_train.json
# keeps it.  The worst tensor is a convolution's in every case (conv1's biases and kernels at the small sizes, conv2.k / conv3.k at n = 130).
# Two figures are float32 itself, not summation order: at n = 64 on xavier(3) one conv2 pre-activation, and at n = 130 on xavier(3) one conv3
# pre-activation, lands on the other branch of the SELU in float32, and the branches' derivatives differ by a factor 1.67 (counted: that one
# flip among the 6.0 million pre-activations of n = 64, 12.2 million of n = 130; 38 and 72 lie within 1e-6 of zero there, 31 at n = 130
# on ONT-HG002, none at n = 3).  No output is saturated in any case (the device test's precheck asserts it).
# The bound of a case is 10 x its figure: the margin is for a different summation order over sites and taps.  It also bounds the losses.
GRAD_F32_NOISE = {
    ("ONT-HG002", 1): 4.06e-6, ("ONT-HG002", 3): 2.72e-5, ("ONT-HG002", 17): 1.57e-5, ("ONT-HG002", 64): 4.66e-6, ("ONT-HG002", 130): 2.15e-5,
    ("xavier3", 1): 1.15e-6, ("xavier3", 3): 8.97e-7, ("xavier3", 17): 2.32e-6, ("xavier3", 64): 7.10e-5, ("xavier3", 130): 5.59e-4,
}


def grad_bound(wname, case):
    return 10 * GRAD_F32_NOISE[(wname, case)]


# five Adam steps at n = 64, lr 1e-3, fixed masks: per-tensor ||dw_f32 - dw_f64|| / ||dw_f64||, largest: ONT-HG002 4.74e-04 (fc2.b), xavier(3)
# 7.47e-03 (fc2.k); the two losses over the five steps, largest relative error: 9.9e-07 / 9.9e-04.  Both figures are a few entries, not a
# spread: one entry holds 67 % of fc2.b's squared error on ONT-HG002 (every other tensor there is below 2.9e-04) and 53 % of fc2.k's on
# xavier(3).  On xavier(3) the float32 run leaves the float64 one as a whole in the fifth step: the losses agree to 3.6e-06 over four steps
# and to 9.9e-04 in the fifth, and all sixteen tensors end between 2.0e-04 and 7.5e-03 (Adam divides by sqrt(v), so an entry whose gradient
# changes sign under float32 noise moves by a full lr the other way).
# (Adam with torch's eps placement: 4.6e-01 on ONT-HG002, whose gradients are of eps's size; 2.6e-03 on xavier(3), whose gradients are far above
# eps, so that probe is sharp on ONT-HG002 only.)
TRAJ_F32_NOISE = {"ONT-HG002": 4.74e-4, "xavier3": 7.47e-3}
TRAJ_LR = 1e-3


def traj_bound(wname):
    return 10 * TRAJ_F32_NOISE[wname]


def segments():
    """-> [(tensor name, offset, size, is_kernel)] of the 16 parameter tensors in blob order"""
    out, off = [], 0
    for name, shp in SPECS:
        nk = int(np.prod(shp))
        out.append((name + ".k", off, nk, True))
        out.append((name + ".b", off + nk, shp[-1], False))
        off += nk + shp[-1]
    return out


def xavier(seed):
    """what train_indel.xavier_init gives, restated: Xavier-uniform kernels, zero biases"""
    rng = np.random.default_rng(seed)
    parts = []
    for _, shp in SPECS:
        rf = int(np.prod(shp[:-2]))
        lim = np.sqrt(6.0 / (rf * shp[-2] + rf * shp[-1]))
        parts.append(rng.uniform(-lim, lim, int(np.prod(shp))).astype(np.float32))
        parts.append(np.zeros(shp[-1], np.float32))
    return np.concatenate(parts)


def weight_set(wname):
    from nanocaller_amd.weights import Weights, get_indel_model
    return Weights(get_indel_model("ONT-HG002")).flat if wname == "ONT-HG002" else xavier(3)


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


def forward(p, x, mask=None, keep=1.0, variant=None):
    """x [n,15,128,2] -> dict z ([n,4] logits), probs [n,4]"""
    dtype = p["fc1"][0].dtype
    x = torch.as_tensor(np.asarray(x), dtype=dtype)
    n = x.shape[0]
    xin = x.permute(0, 3, 1, 2)
    a1 = F.selu(torch.cat([_conv(xin, p["conv1_1"], (0, 2)), _conv(xin, p["conv1_2"], (2, 0)), _conv(xin, p["conv1_3"], (2, 2))], 1))
    a2 = F.selu(_conv(a1, p["conv2"], 0, (1, 2)))
    a3 = F.selu(_conv(a2, p["conv3"], 0, (1, 2)))
    flat = a3.permute(0, 2, 3, 1).reshape(n, -1)                       # H, W, C order
    mk = None
    if mask is not None and keep != 1.0:
        mk = torch.as_tensor(np.asarray(mask), dtype=dtype)
        if variant != "no_scale":
            mk = mk / keep
    pre = flat @ p["fc1"][0] + p["fc1"][1]
    if variant == "mask_first" and mk is not None:
        f1m = F.selu(pre * mk)
    else:
        f1m = F.selu(pre)
        if mk is not None:
            f1m = f1m * mk
    fc2 = F.selu(f1m @ p["fc2"][0] + p["fc2"][1])
    z = fc2 @ p["fc3"][0] + p["fc3"][1]
    return dict(z=z, probs=torch.softmax(z, 1))


def cost(p, out, labels, gamma=GAMMA, variant=None):
    """labels [n] classes 0..3 -> dict cost, CE (torch scalars)"""
    lab = torch.as_tensor(np.asarray(labels)).long()
    if variant == "swap12":
        lab = torch.tensor([0, 2, 1, 3])[lab]
    ce = F.cross_entropy(out["z"], lab)
    reg = 0.0
    if variant != "no_reg":
        for name, _ in SPECS:
            reg = reg + 0.5 * (p[name][0] ** 2).sum()
            if variant == "reg_bias":
                reg = reg + 0.5 * (p[name][1] ** 2).sum()
    return dict(cost=ce + gamma * reg, CE=ce)


def loss_grad(w_flat, x, labels, mask=None, keep=1.0, gamma=GAMMA, dtype=torch.float64, variant=None):
    """-> (cost and CE float64 [2], gradient blob float64 [634420])"""
    p = split(w_flat, dtype, requires_grad=True)
    c = cost(p, forward(p, x, mask, keep, variant), labels, gamma, variant)
    c["cost"].backward()
    return np.array([c[k].item() for k in LOSS_KEYS]), join(p, grad=True).astype(np.float64)


def adam_step(w, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, torch_eps=False):
    """step t (1-based) of Adam in TensorFlow's form; torch_eps: torch's placement, eps added to sqrt(v / (1 - beta2^t))"""
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    if torch_eps:
        w = w - lr / (1 - beta1 ** t) * m / (np.sqrt(v / (1 - beta2 ** t)) + eps)
    else:
        w = w - lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) * m / (np.sqrt(v) + eps)
    return w, m, v


def trajectory(w_flat, x, labels, masks, keep, lr, gamma=GAMMA, dtype=torch.float64, torch_eps=False):
    """len(masks) Adam steps -> (losses [steps][2], final weights float64)"""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    w = np.asarray(w_flat).astype(np_dt)
    m, v = np.zeros_like(w), np.zeros_like(w)
    losses = []
    for t, mask in enumerate(masks, 1):
        l2, g = loss_grad(w, x, labels, mask, keep, gamma, dtype=dtype)
        losses.append(l2)
        w, m, v = adam_step(w, m, v, g.astype(np_dt), np_dt(t), np_dt(lr), np_dt(0.9), np_dt(0.999), np_dt(1e-8), torch_eps)
        w, m, v = w.astype(np_dt), m.astype(np_dt), v.astype(np_dt)
    return np.array(losses), w.astype(np.float64)


def rel_errors(got, want):
    """per parameter tensor ||got - want||_2 / ||want||_2 -> dict name -> float"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return {name: float(np.linalg.norm(got[o:o + k] - want[o:o + k]) / np.linalg.norm(want[o:o + k])) for name, o, k, _ in segments()}


def make_inputs(n, seed=11, keep=0.5):
    """Tensors that look like the pipeline's: in each of the three row groups and every column, channel 1 is a one-hot reference row (all zero
    in a tenth of the columns) and channel 0 a distribution over the five rows minus channel 1; labels with all four classes once n >= 4;
    a seeded 0/1 mask [n][32].  -> (x float32 [n,15,128,2], labels uint8 [n], mask uint8 [n,32])"""
    rng = np.random.default_rng(seed + 1000 * n)
    ref_row = rng.integers(0, 5, (n, 3, 128))
    ch1 = (np.arange(5)[None, None, :, None] == ref_row[:, :, None, :]).astype(np.float64)
    ch1 *= (rng.random((n, 3, 1, 128)) >= 0.1)
    dist = rng.random((n, 3, 5, 128)) ** 4                              # peaked: most of a column's reads agree
    dist /= dist.sum(2, keepdims=True)
    x = np.stack([dist - ch1, ch1], -1).reshape(n, 15, 128, 2).astype(np.float32)
    labels = rng.integers(0, 4, n).astype(np.uint8)
    if n >= 4:
        labels[:4] = np.arange(4)
    mask = (rng.random((n, 32)) < keep).astype(np.uint8)
    return x, labels, mask


def measure_noise(sizes=(1, 3, 17, 64, 130), wnames=("ONT-HG002", "xavier3"), keep=0.5):
    """the float32-against-float64 table behind GRAD_F32_NOISE and TRAJ_F32_NOISE (CPU only) -> dict"""
    out = {"grad": {}, "loss": {}, "worst_tensor": {}}
    for wname in wnames:
        w = weight_set(wname)
        for n in sizes:
            x, lab, mask = make_inputs(n)
            l64, g64 = loss_grad(w, x, lab, mask, keep)
            l32, g32 = loss_grad(w, x, lab, mask, keep, dtype=torch.float32)
            e = rel_errors(g32, g64)
            worst = max(e, key=e.get)
            key = "%s/%s" % (wname, n)
            out["grad"][key], out["worst_tensor"][key] = e[worst], worst
            out["loss"][key] = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
    out["traj"] = {}
    for wname in wnames:
        w = weight_set(wname)
        x, lab, _ = make_inputs(64)
        masks = [make_inputs(64, seed=50 + t)[2] for t in range(5)]
        l64, w64 = trajectory(w, x, lab, masks, keep, TRAJ_LR)
        l32, w32 = trajectory(w, x, lab, masks, keep, TRAJ_LR, dtype=torch.float32)
        lt, wt = trajectory(w, x, lab, masks, keep, TRAJ_LR, torch_eps=True)
        w0 = np.asarray(w, np.float64)
        e, et = rel_errors(w32 - w0, w64 - w0), rel_errors(wt - w0, w64 - w0)
        worst = max(e, key=e.get)
        out["traj"][wname] = dict(dw=e[worst], worst_tensor=worst, losses=float(np.max(np.abs(l32 - l64) / np.abs(l64))), torch_eps_dw=max(et.values()))
    return out

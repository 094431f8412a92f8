"""The reference computation of the haploid indel trainer's tests (tests/hap_train_ref.py has the haploid SNP model's and imports this module as
`indel`): the deployed forward (model_architect_indels_haploid.py:29-48: [5][128][2] -> conv1 24 -> conv2 -> conv3 -> 4,464 -> fc1 32, dropout
behind its SELU -> fc2 24 -> fc3 1 -> sigmoid), the training loss (batch mean of the binary cross-entropy, from the logit, + gamma * sum over
the kernels of |W|^2 / 2) and Adam in TensorFlow's form, in float64 (or float32) with torch autograd on the CPU.

`variant` switches one deliberate mistake on (tests/test_hap_train_ref.py::test_indel_probe_sharpness shows the comparison sees each):
  no_reg       no regulariser
  reg_bias     the regulariser also over the biases
  mask_first   the dropout mask before fc1's SELU instead of behind it
  no_inv_keep  kept units not multiplied by 1 / keep
  inverted     the label inverted (1 = no indel)
  bce_1mp      the cross-entropy of 1 - p: the sigmoid of -z
"""
import numpy as np
import torch
import torch.nn.functional as F

from nanocaller_amd.weights import KIND_INDEL_HAP, LAYER_SPECS

SPECS = LAYER_SPECS[KIND_INDEL_HAP]
NPAR = 158185
LOSS_KEYS = ("cost", "CE")
GAMMA = 1e-5
KEEP = 0.5
SIZES = (1, 3, 17, 64, 130)
WEIGHT_SETS = ("haploid", "xavier3")
SATURATED = 1e-4              # a sigmoid this close to 0 or 1: the relative error of its gradient means nothing

# ---- bounds of the device comparisons (tests/test_hap_train_gpu.py), set by measurement, not by what the device gives: the same restatement
# evaluated in float32 on the CPU against float64, on the inputs of make_inputs() (keep 0.5) and both weight sets.  Per case: the largest
# relative L2 error over the 16 parameter tensors.  The bound of a case is 10 x its figure (the margin is for a different summation order
# over sites and taps) and also bounds the losses.  One machine's figures: they move with the number of threads the CPU sums are split over.
GRAD_F32_NOISE = {
    ("haploid", 1): 2.01e-6, ("haploid", 3): 4.59e-6, ("haploid", 17): 1.24e-5, ("haploid", 64): 5.28e-6, ("haploid", 130): 3.97e-6,
    ("xavier3", 1): 5.92e-7, ("xavier3", 3): 1.71e-6, ("xavier3", 17): 1.48e-6, ("xavier3", 64): 1.08e-6, ("xavier3", 130): 2.96e-6,
}

# the forward's own figure: the largest |p_f32 - p_f64| over the sigmoids at n = 130, plain and with the mask
FWD_F32_NOISE = {"haploid": 2.19e-6, "xavier3": 3.31e-7}

# five Adam steps at n = 64, lr 1e-3, fixed masks: per-tensor ||dw_f32 - dw_f64|| / ||dw_f64||, the largest over the tensors, per weight set
TRAJ_F32_NOISE = {"haploid": 3.94e-5, "xavier3": 1.22e-4}
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
    from nanocaller_amd.weights import Weights, get_indel_model
    if wname == "haploid":
        return Weights(get_indel_model("haploid")).flat
    assert wname == "xavier3", wname
    return train_haploid.xavier_init(KIND_INDEL_HAP, 3)


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
    """x [n,5,128,2] -> dict z ([n] logits), probs [n]"""
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
        mk = torch.as_tensor(np.asarray(mask), dtype=dtype) / (1.0 if variant == "no_inv_keep" else keep)
    pre = flat @ p["fc1"][0] + p["fc1"][1]
    if variant == "mask_first" and mk is not None:
        f1m = F.selu(pre * mk)
    else:
        f1m = F.selu(pre)
        if mk is not None:
            f1m = f1m * mk
    fc2 = F.selu(f1m @ p["fc2"][0] + p["fc2"][1])
    z = (fc2 @ p["fc3"][0] + p["fc3"][1]).reshape(n)
    return dict(z=z, probs=torch.sigmoid(z))


def cost(p, out, labels, gamma=GAMMA, variant=None):
    """labels [n], 1 = indel -> dict cost, CE (torch scalars); the cross-entropy is softplus(z) - y z"""
    y = torch.as_tensor(np.asarray(labels)).to(out["z"].dtype)
    if variant == "inverted":
        y = 1 - y
    z = -out["z"] if variant == "bce_1mp" else out["z"]
    r = {"CE": (F.softplus(z) - y * z).mean()}
    reg = 0.0
    if variant != "no_reg":
        for name, _ in SPECS:
            reg = reg + 0.5 * (p[name][0] ** 2).sum()
            if variant == "reg_bias":
                reg = reg + 0.5 * (p[name][1] ** 2).sum()
    r["cost"] = r["CE"] + gamma * reg
    return r


def loss_grad(w_flat, x, labels, mask=None, keep=1.0, gamma=GAMMA, dtype=torch.float64, variant=None):
    """-> (cost, CE float64 [2], gradient blob float64 [158185])"""
    p = split(w_flat, dtype, requires_grad=True)
    c = cost(p, forward(p, x, mask, keep, variant), labels, gamma, variant)
    c["cost"].backward()
    return np.array([c[k].item() for k in LOSS_KEYS]), join(p, grad=True).astype(np.float64)


def sigmoids(w_flat, x, mask=None, keep=1.0):
    """the sigmoid of every site, float64 [n]: the quantity the no-saturation condition is about"""
    return forward(split(w_flat), x, mask, keep)["probs"].detach().numpy()


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


def make_inputs(n, seed=11, keep=KEEP):
    """Tensors that look like the haploid pipeline's, as tests/indel_train_ref.py draws them with one row group instead of three: in every
    column channel 1 is a one-hot reference row (all zero in a tenth of the columns) and channel 0 a distribution over the five rows minus
    channel 1; both labels once n >= 2; a seeded 0/1 mask [n][32].  -> (x float32 [n,5,128,2], labels uint8 [n], mask uint8 [n,32])"""
    rng = np.random.default_rng(seed + 1000 * n)
    ref_row = rng.integers(0, 5, (n, 128))
    ch1 = (np.arange(5)[None, :, None] == ref_row[:, None, :]).astype(np.float64)
    ch1 *= (rng.random((n, 1, 128)) >= 0.1)
    dist = rng.random((n, 5, 128)) ** 4                                 # peaked: most of a column's reads agree
    dist /= dist.sum(1, keepdims=True)
    x = np.stack([dist - ch1, ch1], -1).astype(np.float32)
    labels = rng.integers(0, 2, n).astype(np.uint8)
    if n >= 2:
        labels[:2] = (1, 0)
    mask = (rng.random((n, 32)) < keep).astype(np.uint8)
    return x, labels, mask


def measure_noise(wname, n):
    """the float32-against-float64 figure of one case of GRAD_F32_NOISE -> (largest per-tensor error, largest loss error)"""
    x, lab, mask = make_inputs(n)
    w = weights(wname)
    l64, g64 = loss_grad(w, x, lab, mask, KEEP)
    l32, g32 = loss_grad(w, x, lab, mask, KEEP, dtype=torch.float32)
    return max(rel_errors(g32, g64).values()), float((np.abs(l32 - l64) / np.abs(l64)).max())


def measure_traj_noise(wname):
    x, lab, _ = make_inputs(64)
    masks = [make_inputs(64, seed=50 + t)[2] for t in range(5)]
    w = weights(wname)
    _, w64 = trajectory(w, x, lab, masks, KEEP, TRAJ_LR)
    _, w32 = trajectory(w, x, lab, masks, KEEP, TRAJ_LR, dtype=torch.float32)
    w0 = np.asarray(w, np.float64)
    return max(rel_errors(w32 - w0, w64 - w0).values())


def measure_forward_noise(wname, n=130):
    """the figure of FWD_F32_NOISE: float32 against float64 sigmoids, plain and with the mask"""
    w = weights(wname)
    x, _, mask = make_inputs(n)
    worst = 0.0
    for m, keep in ((None, 1.0), (mask, KEEP)):
        p64 = forward(split(w), x, m, keep)["probs"].detach().numpy()
        p32 = forward(split(w, torch.float32), x, m, keep)["probs"].detach().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(p32 - p64).max()))
    return worst

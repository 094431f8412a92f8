"""The reference computation of the SNP trainer's tests: the diploid SNP model (the deployed forward, model_architect.py:36-64: softmax
outputs of the allele heads into fc3, dropout behind fc1's SELU), the training loss (misc/training/model_architect.py:130-145) and Adam in
TensorFlow's form, in float64 (or float32) with torch autograd on the CPU.  Test code: the trainer itself never calls torch.nn.

`variant` switches one deliberate mistake on (tests/test_snp_train_ref.py::test_probe_sharpness shows the comparison sees each):
  no_jacobian  the allele heads reach fc3 detached: the GT loss does not flow through their softmaxes
  no_reg       no regulariser
  reg_bias     the regulariser also over the biases
  mask_first   the dropout mask before fc1's SELU instead of behind it
"""
import numpy as np
import torch
import torch.nn.functional as F

from nanocaller_amd.weights import KIND_SNP, LAYER_SPECS

SPECS = LAYER_SPECS[KIND_SNP]
LOSS_KEYS = ("cost", "GT", "A", "G", "T", "C")
GAMMA = 1e-3

# ---- bounds of the device comparisons (tests/test_snp_train_gpu.py), set by measurement, not by what the device gives:
# the same restatement evaluated in float32 on the CPU against float64, on the inputs of make_inputs() (keep 0.5) and both weight sets.  Per
# case: the largest relative L2 error over the 28 parameter tensors (the six loss terms are always closer: 1.4e-07 .. 5.2e-05, below the
# tensors' figure of the same case).  "17s": n = 17 with a coverage scale of 0.5 .. 2.  tools/bench_train.py --noise prints this table;
# profiles/snp_train.json keeps it.
# Most cases sit at 1e-6 to 3e-6.  The outliers are float32 itself, not summation order: at n = 1 on ONT-HG002 the A head is nearly saturated
# (margin 2.5e-4), so p - label cancels; at n = 300 on ONT-HG002 and at n = 4160 one conv1 pre-activation within 1e-6 of zero lands on the
# other branch of the SELU in float32, and the branches' derivatives differ by a factor 1.67 (counted: one such flip among the 3 million conv1
# activations at n = 300; twelve more pre-activations lie within 1e-6 of zero there, none in the smaller cases).
# The bound of a case is 10 x its figure: the margin is for a different summation order over sites and taps.  It also bounds the losses.
GRAD_F32_NOISE = {
    ("ONT-HG002", 1): 5.28e-5, ("ONT-HG002", 3): 2.48e-6, ("ONT-HG002", 17): 1.17e-6, ("ONT-HG002", 64): 2.97e-6, ("ONT-HG002", 300): 2.87e-4,
    ("xavier3", 1): 5.00e-6, ("xavier3", 3): 2.25e-5, ("xavier3", 17): 1.44e-6, ("xavier3", 64): 1.77e-6, ("xavier3", 300): 1.93e-6,
    ("ONT-HG002", "17s"): 1.99e-6, ("xavier3", "17s"): 7.42e-6, ("xavier3", 4160): 1.12e-4,
}


def grad_bound(wname, case):
    return 10 * GRAD_F32_NOISE[(wname, case)]


# five Adam steps at n = 64, lr 1e-3, fixed masks: per-tensor ||dw_f32 - dw_f64|| / ||dw_f64||, largest: ONT-HG002 3.8e-05 (G.b), xavier(3) 1.4e-05 (fc1.k);
# the six losses over the five steps, largest relative error: 5.4e-07 / 1.4e-06.  (Adam with torch's eps placement: 1.7e-01 / 3.9e-03.)
TRAJ_F32_NOISE = 3.8e-5
TRAJ_BOUND = 10 * TRAJ_F32_NOISE
TRAJ_LR = 1e-3


def segments():
    """-> [(tensor name, offset, size, is_kernel)] of the 28 parameter tensors in blob order"""
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


def forward(p, x, ref_code, scale=None, mask=None, keep=1.0, variant=None):
    """x [n,5,41,5], ref_code [n] -> dict z (four [n,2] logits), g ([n,2] GT logits), probs [n,4], gt [n,2], acts"""
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
        mk = torch.as_tensor(np.asarray(mask), dtype=dtype) / keep
    pre = flat @ p["fc1"][0] + p["fc1"][1]
    if variant == "mask_first" and mk is not None:
        f1m = F.selu(pre * mk)
    else:
        f1m = F.selu(pre)
        if mk is not None:
            f1m = f1m * mk
    fa = F.selu(f1m @ p["fa"][0] + p["fa"][1])
    onehot = F.one_hot(torch.as_tensor(np.asarray(ref_code)).long(), 4).to(dtype)
    z, sm = [], []
    for h, name in enumerate("AGTC"):
        zh = torch.cat([fa, onehot[:, h:h + 1]], 1) @ p[name][0] + p[name][1]
        z.append(zh)
        sm.append(torch.softmax(zh, 1))
    fc2 = F.selu(f1m @ p["fc2"][0] + p["fc2"][1])
    heads_in = [s.detach() for s in sm] if variant == "no_jacobian" else sm
    fc3 = F.selu(torch.cat([fc2] + heads_in, 1) @ p["fc3"][0] + p["fc3"][1])
    g = fc3 @ p["GT"][0] + p["GT"][1]
    return dict(z=z, g=g, probs=torch.stack([s[:, 1] for s in sm], 1), gt=torch.softmax(g, 1))


def cost(p, out, labels, gamma=GAMMA, variant=None):
    """labels [n,5] = classes of A, G, T, C, GT -> dict of the six terms (torch scalars)"""
    lab = torch.as_tensor(np.asarray(labels)).long()
    r = {name: F.cross_entropy(out["z"][h], lab[:, h]) for h, name in enumerate("AGTC")}
    r["GT"] = F.cross_entropy(out["g"], lab[:, 4])
    reg = 0.0
    if variant != "no_reg":
        for name, _ in SPECS:
            reg = reg + 0.5 * (p[name][0] ** 2).sum()
            if variant == "reg_bias":
                reg = reg + 0.5 * (p[name][1] ** 2).sum()
    r["cost"] = r["A"] + r["G"] + r["T"] + r["C"] + r["GT"] + gamma * reg
    return r


def loss_grad(w_flat, x, ref_code, labels, mask=None, keep=1.0, gamma=GAMMA, scale=None, dtype=torch.float64, variant=None):
    """-> (six losses float64 [6] in LOSS_KEYS order, gradient blob float64 [109370])"""
    p = split(w_flat, dtype, requires_grad=True)
    c = cost(p, forward(p, x, ref_code, scale, mask, keep, variant), labels, gamma, variant)
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


def trajectory(w_flat, x, ref_code, labels, masks, keep, lr, gamma=GAMMA, dtype=torch.float64, torch_eps=False):
    """len(masks) Adam steps -> (losses [steps][6], final weights float64)"""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    w = np.asarray(w_flat).astype(np_dt)
    m, v = np.zeros_like(w), np.zeros_like(w)
    losses = []
    for t, mask in enumerate(masks, 1):
        l6, g = loss_grad(w, x, ref_code, labels, mask, keep, gamma, dtype=dtype)
        losses.append(l6)
        w, m, v = adam_step(w, m, v, g.astype(np_dt), np_dt(t), np_dt(lr), np_dt(0.9), np_dt(0.999), np_dt(1e-8), torch_eps)
        w, m, v = w.astype(np_dt), m.astype(np_dt), v.astype(np_dt)
    return np.array(losses), w.astype(np.float64)


def rel_errors(got, want):
    """per parameter tensor ||got - want||_2 / ||want||_2 -> dict name -> float"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return {name: float(np.linalg.norm(got[o:o + k] - want[o:o + k]) / np.linalg.norm(want[o:o + k])) for name, o, k, _ in segments()}


def make_inputs(n, seed=11, keep=0.5):
    """integer tensors in -8..8, all four reference bases, both classes in every label column (n >= 2), a seeded 0/1 mask"""
    rng = np.random.default_rng(seed + 1000 * n)
    x = rng.integers(-8, 9, (n, 5, 41, 5)).astype(np.float32)
    ref = (np.arange(n) % 4).astype(np.int32)
    labels = rng.integers(0, 2, (n, 5)).astype(np.uint8)
    if n >= 2:
        labels[0], labels[1] = 0, 1
    mask = (rng.random((n, 48)) < keep).astype(np.uint8)
    return x, ref, labels, mask

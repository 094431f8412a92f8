"""Synthetic, unsaturated probes of the four CNNs (a helper module, not a conftest).

The shipped checkpoints saturate (1 - 3 % of their outputs lie in (0.1, 0.9)) and carry many dead weights, so a kernel with one tap
or one packed row wrong can stay inside the product's 1e-4 contract.  The probes here are weight blobs drawn from seeds, in which every
element is distinct and matters, with inputs on which the float64 oracle's outputs stay in the steep part of the sigmoid / softmax:
  synthetic_blob   the blob of a kind ("dense": N(0, g / fan_in) kernels; "wide": magnitudes log-uniform over 2^-20 .. 2^0)
  layer_view       one layer's kernel (or bias) inside a flat blob
  write_probe      the blob as an .ncw file of its own (the engine caches loaded weights by path)
  mutations        the catalogue of single-weight errors a probe must see (tests/test_cnn_probe_ref.py proves that it does)
  snp_inputs / indel_inputs, oracle_forward, tolerance, x_limit_bound
Nothing here opens the GPU."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from nanocaller_amd.weights import KIND_INDEL, KIND_INDEL_HAP, KIND_SNP, KIND_SNP_HAP, LAYER_SPECS, n_params, write_ncw

KINDS = (KIND_SNP, KIND_SNP_HAP, KIND_INDEL, KIND_INDEL_HAP)
KIND_NAMES = {KIND_SNP: "snp", KIND_SNP_HAP: "snp_hap", KIND_INDEL: "indel", KIND_INDEL_HAP: "indel_hap"}
RECIPES = ("dense", "wide")
TRUNK = ("conv1_1", "conv1_2", "conv1_3", "conv2", "conv3", "fc1")

# Gain g of a layer's kernel: its elements have variance g / fan_in.  The trunk keeps g = 1 (SELU's fixed point: unit-variance
# activations); the layers behind fc1 are damped so that the logits stay small.  A two-way softmax (diploid SNP) leaves (0.1, 0.9) at a
# logit difference of 2.2, a four-way one (haploid SNP, diploid indel) already when one logit lies 1.1 below the others, hence
# the smaller gains there.  Tuned on the float64 oracle alone (test_cnn_probe_ref.py asserts the outcome).
HEAD_GAIN = {
    KIND_SNP: {"fa": 0.5, "A": 0.2, "G": 0.2, "T": 0.2, "C": 0.2, "fc2": 0.5, "fc3": 0.5, "GT": 0.2},
    KIND_SNP_HAP: {"fc2": 0.5, "fc3": 0.07},
    KIND_INDEL: {"fc2": 0.5, "fc3": 0.07},
    KIND_INDEL_HAP: {"fc2": 0.5, "fc3": 0.5},
}
BIAS_VAR = 0.1
HEAD_BIAS_VAR = {KIND_SNP: 0.1, KIND_SNP_HAP: 0.01, KIND_INDEL: 0.01, KIND_INDEL_HAP: 0.1}


def _offsets(kind):
    out, off = {}, 0
    for name, shape in LAYER_SPECS[kind]:
        nk = int(np.prod(shape))
        out[name] = (off, shape)
        off += nk + shape[-1]
    return out


def layer_view(flat, kind, name, bias=False):
    """the kernel of layer `name` (Keras layout: HWIO / [in, out]) inside the flat blob, as a view; bias=True: its bias, which follows it"""
    off, shape = _offsets(kind)[name]
    nk = int(np.prod(shape))
    return flat[off + nk:off + nk + shape[-1]] if bias else flat[off:off + nk].reshape(shape)


def synthetic_blob(kind, seed, recipe):
    """float32 blob [n_params(kind)] in the canonical order (every layer: kernel, then bias)"""
    assert recipe in RECIPES
    rng = np.random.default_rng([seed, kind, RECIPES.index(recipe)])
    flat = np.zeros(n_params(kind), np.float32)
    for name, shape in LAYER_SPECS[kind]:
        fan_in = int(np.prod(shape[:-1]))
        head = name in HEAD_GAIN[kind]
        g = HEAD_GAIN[kind][name] if head else 1.0
        if head:
            # The layers behind fc1 (scalar fp32 code, not split) are probed element by element, so none of their weights may be dead in either
            # recipe: a unit whose few outgoing weights are all near zero hides every weight in front of it.  Magnitudes uniform in
            # (0.5, 1.5) x sqrt(g / fan_in) / 1.04 (the same variance), random signs.
            k = rng.uniform(0.5, 1.5, size=shape) * rng.choice([-1.0, 1.0], size=shape) * np.sqrt(g / (fan_in * (13.0 / 12.0)))
        elif recipe == "dense":
            k = rng.normal(0.0, np.sqrt(g / fan_in), size=shape)
        else:
            # magnitudes down to 2^-20 of the layer's largest: in and below fp16's subnormals once the load-time scale is applied;
            # rescaled to the variance the dense recipe gives the layer's outputs (sum of squares over fan_in = g per output unit)
            k = np.exp2(rng.uniform(-20.0, 0.0, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
            k *= np.sqrt(g / (fan_in * np.mean(k * k)))
        k = k.astype(np.float32).ravel()
        while True:                                                    # every element distinct in float32 too: a repeat moves up by one ulp
            first = np.zeros(k.size, bool)
            first[np.unique(k, return_index=True)[1]] = True
            if first.all():
                break
            k[~first] = np.nextafter(k[~first], np.float32(np.inf))
        layer_view(flat, kind, name)[...] = k.reshape(shape)
        layer_view(flat, kind, name, bias=True)[...] = rng.normal(0.0, np.sqrt(HEAD_BIAS_VAR[kind] if head else BIAS_VAR), size=shape[-1])
    return flat


def write_probe(tmp_path, kind, blob, train_cov=48.0, tag="probe"):
    """the blob as `<tmp_path>/<tag>_<kind>.ncw` -> path.  Every probe needs a path of its own: Engine.load_weights skips a load whose
    path equals the loaded one."""
    path = os.path.join(str(tmp_path), "%s_%s.ncw" % (tag, KIND_NAMES[kind]))
    assert not os.path.exists(path), path
    tensors = []
    for name, shape in LAYER_SPECS[kind]:
        tensors.append((name + ".k", layer_view(blob, kind, name)))
        tensors.append((name + ".b", layer_view(blob, kind, name, bias=True)))
    write_ncw(path, kind, train_cov, tensors)
    return path


def rescaled(blob, kind, f1, f2=1.0):
    """the blob with its conv1 kernels x f1, conv2's x f2 and fc1's / (f1 f2): the activations of conv1 - conv3 grow (and with them
    the range bound of the split-precision kernels shrinks) while fc1's pre-activations, up to SELU's negative branch and the biases, stay"""
    out = blob.copy()
    for name in ("conv1_1", "conv1_2", "conv1_3"):
        layer_view(out, kind, name)[...] *= np.float32(f1)
    layer_view(out, kind, "conv2")[...] *= np.float32(f2)
    layer_view(out, kind, "fc1")[...] /= np.float32(f1 * f2)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def snp_inputs(seed, n, hi):
    """n distinct SNP site tensors with the structure of SURVEY Appendix A -- row 0 the one-hot reference, rows 1..4 integer counts in
    [-hi, hi] on channels 0..3 and 0 / 1 flags on channel 4 --, a quarter of them one saturated plane (every read the same base);
    ref_code = the centre column's base (all four occur); per-site coverage scales that bring the counts to |x| of order 1.
    -> (x float32 [n,5,41,5], ref_code int32 [n], scale float64 [n])"""
    rng = np.random.default_rng([seed, n, hi, 1])
    x = np.zeros((n, 5, 41, 5), np.float32)
    ref = rng.integers(0, 4, size=(n, 41))
    if n >= 4:
        ref[:4, 20] = np.arange(4)
    x[np.arange(n)[:, None], 0, np.arange(41)[None, :], ref] = 1
    x[:, 1:, :, :4] = rng.integers(-hi, hi + 1, size=(n, 4, 41, 4))
    x[:, 1:, :, 4] = rng.integers(0, 2, size=(n, 4, 41))
    k = np.arange(n) % 4 == 3
    b = rng.integers(0, 4, size=n)
    for s in np.nonzero(k)[0]:
        x[s, 1:, :, :4] = 0
        x[s, 1 + b[s], :, b[s]] = hi
        x[s, 1 + (b[s] + 1) % 4, :, (b[s] + 2) % 4] = rng.integers(-hi, hi + 1, size=41)     # (keeps these sites distinct)
    scale = rng.uniform(0.5, 2.0, size=n) / hi
    return x, ref[:, 20].astype(np.int32), scale.astype(np.float64)


def indel_inputs(seed, n, rows):
    """n dense indel tensors [rows][128][2] (rows = 15 diploid, 5 haploid) of frequencies, |x| <= 1, the bounds and 0 included"""
    rng = np.random.default_rng([seed, n, rows, 2])
    x = rng.uniform(-1.0, 1.0, size=(n, rows, 128, 2)).astype(np.float32)
    edge = rng.integers(0, 16, size=x.shape)
    x[edge == 0] = 1.0
    x[edge == 1] = -1.0
    x[edge == 2] = 0.0
    return x


def probe_inputs(kind, seed, n, hi=30):
    """the input tuple of a kind as oracle_forward takes it: (x, ref_code, scale) with counts up to `hi`, or (x,) of an indel kind"""
    return snp_inputs(seed, n, hi) if kind in (KIND_SNP, KIND_SNP_HAP) else (indel_inputs(seed, n, 15 if kind == KIND_INDEL else 5),)


# ---------------------------------------------------------------------------------------------------------------- the reference
def _threads():
    return max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count() or 1))


def oracle_forward(kind, blob, inputs, precision="f64", scale_mode=0):
    """every output of the oracle's forward as one float32 array [n][k]: diploid SNP probs | gt (k = 6), haploid SNP 4, indel 4 / 1.
    Sites are independent, so they are spread over a few threads (the oracle is C behind ctypes)."""
    from oracle import oracle
    n = int(inputs[0].shape[0])

    def part(sl):
        if kind == KIND_SNP:
            p, g = oracle.snp_forward(blob, inputs[0][sl], inputs[1][sl], inputs[2][sl], scale_mode=scale_mode, precision=precision)
            return np.concatenate([p, g], axis=1)
        if kind == KIND_SNP_HAP:
            return oracle.snp_hap_forward(blob, inputs[0][sl], inputs[1][sl], inputs[2][sl], scale_mode=scale_mode, precision=precision)
        return oracle.indel_forward(blob, inputs[0][sl], precision=precision)
    oracle.lib()
    nt = min(_threads(), n)
    cuts = [n * i // nt for i in range(nt + 1)]
    with ThreadPoolExecutor(nt) as pool:
        return np.concatenate(list(pool.map(part, [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])])), axis=0)


def tolerance(ref32, ref64):
    """what a kernel may differ from the float64 oracle by, from the reference alone: 8 x the float32 oracle's own error on the same blob and
    inputs (4 x: the split drops the lo x lo products, 2^-22 against fp32's 2^-24 per product; 2 x: another accumulation order), floor 1e-6
    (the oracle returns float32)"""
    return max(8.0 * float(np.abs(ref32.astype(np.float64) - ref64.astype(np.float64)).max()), 1e-6)


def x_limit_bound(kind, blob):
    """nc_load_weights' range bound of the split-precision kernels (csrc/nc_cnn.hip cnn_x_limit) restated in float64: the largest input
    magnitude X for which the L1 norms of conv1 - conv3 prove every clamped activation below 6e4"""
    snp = kind in (KIND_SNP, KIND_SNP_HAP)
    def l1(name):
        k = layer_view(blob, kind, name).astype(np.float64)
        return np.abs(k.reshape(-1, k.shape[-1])).sum(0).max()
    def bmax(name):
        return float(np.abs(layer_view(blob, kind, name, bias=True).astype(np.float64)).max())
    L1, B1 = max(l1("conv1_1"), l1("conv1_2"), l1("conv1_3")), max(bmax("conv1_1"), bmax("conv1_2"), bmax("conv1_3"))
    L2, B2, L3, B3 = l1("conv2"), bmax("conv2"), l1("conv3"), bmax("conv3")
    LAM = 1.0507009873554805
    LA, CAP = LAM * 1.6732632423543772, 60000.0 * 0.999

    def worst(X):
        a1 = max(LAM * (L1 * X + B1), LA)
        a2 = max(LAM * (L2 * a1 + B2), LA)
        a3 = max(LAM * (L3 * a2 + B3), LA)
        return max(a1, a2, a3) if snp else max(a1, a2)
    lo, hi = 0.0, 1e6
    if worst(0.0) >= CAP:
        return 0.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if worst(mid) < CAP:
            lo = mid
        else:
            hi = mid
    return float(np.float32(lo))


# ---------------------------------------------------------------------------------------------------------------- mutations
def _edges(n, marks):
    """first, last and both sides of the tile borders `marks` of an axis of length n"""
    return sorted({0, n - 1} | {m + d for m in marks for d in (-1, 0) if 0 < m < n})


def mutations(kind):
    """The catalogue: a list of tuples, applied by `mutate`.
      ("zero", layer, index)            one kernel element set to 0
      ("zero_max", layer)               the layer's largest element set to 0 (its place depends on the blob; in a "wide" layer the elements at
                                        fixed places are mostly too small for their loss to show, this one never is)
      ("swap", layer, axis, a, b)       two slices of the kernel exchanged (axis 2 of a conv = input channels, the last axis = output channels,
                                        axis 0 of fc1 = its rows)
      ("bias", layer, i)                bias element + 0.01
      ("fp16",)                         conv and fc1 kernels rounded to fp16: what a split that loses its lo half computes
    Zeroings sit at the first and last index of every axis and on both sides of the kernels' tile borders: the 16-wide MFMA output tiles,
    the K groups of 8 / 16 / 32 input channels, fc1's rows in groups of 32 and its last rows, and for the indel conv2 the end of its
    K = 6 x 24 = 144 (padded to 160 in the kernel) and the K = 127 | 128 border inside it.  Head matrices are covered element by element."""
    snp = kind in (KIND_SNP, KIND_SNP_HAP)
    spec = dict(LAYER_SPECS[kind])
    out = []
    for name in TRUNK:
        shape = spec[name]
        mid = tuple(s // 2 for s in shape)
        if len(shape) == 4:
            marks = [(), (), (8, 16, 32), (16, 32, 48)]
            out.append(("zero", name, tuple(0 for _ in shape)))
            out.append(("zero", name, tuple(s - 1 for s in shape)))
            for ax in range(4):
                for i in _edges(shape[ax], marks[ax]):
                    out.append(("zero", name, mid[:ax] + (i,) + mid[ax + 1:]))
            cin, cout = shape[2], shape[3]
            out.append(("swap", name, 2, cin - 2, cin - 1))
            out.append(("swap", name, 3, cout // 2 - 1, cout // 2))
        else:
            rows, cols = shape
            for r in _edges(rows, (16, 32, 64, rows - 32, rows - 1)):
                out.append(("zero", name, (r, cols // 2)))
            for c in _edges(cols, (16, 32)):
                out.append(("zero", name, (rows // 2, c)))
            out += [("zero", name, (0, 0)), ("zero", name, (rows - 1, cols - 1))]
            out += [("swap", name, 0, 0, 64), ("swap", name, 0, rows - 2, rows - 1), ("swap", name, 1, cols // 2 - 1, cols // 2)]
        out.append(("zero_max", name))
        out.append(("bias", name, shape[-1] - 1))
    if snp:
        out.append(("zero", "conv3", (1, 2, 31, 63)))                   # (the issue's examples)
        out.append(("zero", "conv1_3", (4, 4, 4, 15)))
        out.append(("zero", "conv2", (1, 2, 47, 31)))
        out.append(("swap", "conv2", 2, 46, 47))
    else:
        # conv2's K index = (tap, channel) flattened: 127 | 128 = tap 5, channels 7 | 8; 143 = the last real one before the padding
        out += [("zero", "conv2", (1, 2, 7, 16)), ("zero", "conv2", (1, 2, 8, 16)), ("zero", "conv2", (1, 2, 23, 31)), ("zero", "conv2", (1, 2, 23, 0))]
    for name, shape in LAYER_SPECS[kind]:
        if name in TRUNK:
            continue
        for i in range(shape[0]):
            for j in range(shape[1]):
                out.append(("zero", name, (i, j)))
        if shape[1] > 1:
            out.append(("swap", name, 1, 0, shape[1] - 1))
        out.append(("swap", name, 0, 0, shape[0] - 1))
        out.append(("bias", name, shape[1] // 2))                       # (a middle unit: fc3 of the diploid SNP model keeps units deep in SELU's flat branch)
    out.append(("fp16",))
    seen, uniq = set(), []
    for m in out:
        if m not in seen:
            seen.add(m)
            uniq.append(m)
    return uniq


def is_head(m):
    return m[0] != "fp16" and m[1] not in TRUNK


def substitute(m):
    """what replaces a ("zero", layer, index) whose loss the float64 oracle does not show at 10 x the tolerance (an element that happens
    to be small; most of a "wide" layer): the same element takes a wrong weight of the layer's rms size and the opposite sign, which
    is what a kernel that reads another tap in its place computes.  It is a different mutation and carries its own name."""
    assert m[0] == "zero"
    return ("wrong",) + tuple(m[1:])


def mutate(blob, kind, m):
    """a copy of the blob with mutation m applied"""
    out = blob.copy()
    if m[0] == "fp16":
        for name in TRUNK:
            k = layer_view(out, kind, name)
            k[...] = k.astype(np.float16).astype(np.float32)
        return out
    if m[0] == "bias":
        layer_view(out, kind, m[1], bias=True)[m[2]] += np.float32(0.01)
        return out
    k = layer_view(out, kind, m[1])
    if m[0] == "zero_max":
        k[np.unravel_index(np.argmax(np.abs(k)), k.shape)] = 0.0
    elif m[0] == "zero":
        k[m[2]] = 0.0
    elif m[0] == "wrong":
        rms = float(np.sqrt(np.mean(np.square(k, dtype=np.float64))))
        k[m[2]] = -rms if float(k[m[2]]) >= 0 else rms
    else:
        _, _, ax, a, b = m
        ia, ib = [slice(None)] * k.ndim, [slice(None)] * k.ndim
        ia[ax], ib[ax] = a, b
        tmp = k[tuple(ia)].copy()
        k[tuple(ia)] = k[tuple(ib)]
        k[tuple(ib)] = tmp
    return out

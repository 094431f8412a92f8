"""The synthetic CNN probes (tests/cnn_probe.py) are sharp: proven on the float64 oracle alone, without a GPU, so that the GPU comparison
of tests/test_cnn_synthetic_gpu.py cannot hide a wrong kernel behind a weak probe.  For every model kind and both weight recipes:
  * at least 99 % of the oracle's outputs on the probe inputs lie in (0.1, 0.9) and all of them in (0.01, 0.99): an error in a logit is
    not swallowed by a saturated sigmoid / softmax;
  * every mutation of the catalogue -- single kernel elements zeroed at the first / last index of every axis and on both sides of the kernels'
    tile borders, channel / row swaps, a bias, every element of every head matrix, the conv + fc1 weights rounded to fp16 -- moves the
    oracle's output by at least 10 x the tolerance the GPU test grants a kernel on the same blob and inputs
    (max(8 x |oracle_f32 - oracle_f64|, 1e-6)); a zeroing that does not is replaced by a wrong weight at the same index, under its own name,
    and every layer keeps a true zeroing that does."""
import numpy as np
import pytest

import cnn_probe as P
from nanocaller_amd.weights import LAYER_SPECS, Weights, n_params

SEEDS = (0, 1, 2)
CASES = [(k, r) for k in P.KINDS for r in P.RECIPES]
IDS = ["%s-%s" % (P.KIND_NAMES[k], r) for k, r in CASES]
SNP = (P.KIND_SNP, P.KIND_SNP_HAP)


def _input_sets(kind, seed, n_snp=256, n_indel=64):
    if kind in SNP:
        return [("counts <= %d" % hi, P.snp_inputs(seed, n_snp, hi)) for hi in (30, 160)]
    return [("frequencies", P.probe_inputs(kind, seed, n_indel))]


def test_blob_layout_and_file_route(tmp_path):
    for kind in P.KINDS:
        blob = P.synthetic_blob(kind, 5, "dense")
        assert blob.dtype == np.float32 and blob.size == n_params(kind)
        assert np.array_equal(blob, P.synthetic_blob(kind, 5, "dense")) and not np.array_equal(blob, P.synthetic_blob(kind, 6, "dense"))
        w = Weights(P.write_probe(tmp_path, kind, blob))
        assert w.kind == kind and np.array_equal(w.flat, blob)
        off = 0
        for name, shape in LAYER_SPECS[kind]:                           # kernel, then bias, in the canonical order
            k, b = P.layer_view(blob, kind, name), P.layer_view(blob, kind, name, bias=True)
            assert k.shape == tuple(shape) and b.shape == (shape[-1],)
            assert np.shares_memory(k, blob) and np.array_equal(k.ravel(), blob[off:off + k.size])
            assert np.array_equal(b, blob[off + k.size:off + k.size + b.size])
            assert np.array_equal(w.t[name + ".k"], k) and np.array_equal(w.t[name + ".b"], b)
            assert np.unique(k).size == k.size, (kind, name)            # every element distinct: a permutation changes the layer
            off += k.size + b.size
        assert off == blob.size


def test_wide_recipe_reaches_below_the_fp16_subnormals():
    """the split packs a weight as fp16 hi + lo of w x S, S <= 1024 (H3Scale): the smallest magnitudes of a "wide" layer lie more than 2^-14 / 1024
    below its largest, i.e. their hi halves are fp16 subnormals or vanish.  This concerns the split layers only -- conv1_3, conv2, conv3, fc1;
    the 1x5 and 5x1 kernels of the indel models (80 elements) are too few to be sure of the span and are left out, and the layers behind fc1
    are drawn densely in both recipes (cnn_probe.synthetic_blob)."""
    for kind in P.KINDS:
        blob = P.synthetic_blob(kind, 0, "wide")
        for name in P.TRUNK:
            a = np.abs(P.layer_view(blob, kind, name))
            if a.size >= 400:
                assert a.min() < a.max() * 2.0 ** -16 and a.min() > 0, (kind, name)


def test_catalogue_covers_every_layer():
    for kind in P.KINDS:
        muts = P.mutations(kind)
        assert len(set(muts)) == len(muts) and ("fp16",) in muts
        for name, shape in LAYER_SPECS[kind]:
            ops = {m[0] for m in muts if len(m) > 1 and m[1] == name}
            assert {"zero", "swap", "bias"} <= ops and ("zero_max" in ops) == (name in P.TRUNK), (kind, name)
            zeroed = {m[2] for m in muts if m[0] == "zero" and m[1] == name}
            assert tuple(0 for _ in shape) in zeroed and tuple(s - 1 for s in shape) in zeroed, (kind, name)
            if name not in P.TRUNK:
                assert len(zeroed) == int(np.prod(shape)), (kind, name)  # heads: element by element (the ref-base rows included)
        z = lambda layer: {m[2] for m in muts if m[0] == "zero" and m[1] == layer}   # noqa: E731
        assert {i[2] for i in z("conv2")} >= {7, 8, 15, 16}                          # K-group borders of the input channels
        assert {i[3] for i in z("conv2")} >= {15, 16} and {i[3] for i in z("conv3")} >= {15, 16, 31, 32}
        rows = LAYER_SPECS[kind][5][1][0]
        assert {i[0] for i in z("fc1")} >= {0, 15, 16, 31, 32, rows - 2, rows - 1}
        if kind not in SNP:
            assert {(1, 2, 7), (1, 2, 8), (1, 2, 23)} <= {i[:3] for i in z("conv2")}  # K = 127 | 128 and the last K before the padding to 160


@pytest.mark.parametrize("kind,recipe", CASES, ids=IDS)
def test_oracle_outputs_stay_unsaturated(kind, recipe):
    for seed in SEEDS:
        blob = P.synthetic_blob(kind, seed, recipe)
        for what, inp in _input_sets(kind, seed):
            for mode in ((0, 1) if kind in SNP else (0,)):
                out = P.oracle_forward(kind, blob, inp, "f64", scale_mode=mode).astype(np.float64)
                mid = float(np.mean((out > 0.1) & (out < 0.9)))
                print("%s %s seed %d, %s, scale_mode %d: %.2f %% in (0.1, 0.9), range %.4f .. %.4f" %
                      (P.KIND_NAMES[kind], recipe, seed, what, mode, 100 * mid, out.min(), out.max()))
                assert mid >= 0.99, (seed, what, mid)
                assert out.min() > 0.01 and out.max() < 0.99, (seed, what, out.min(), out.max())


@pytest.mark.parametrize("kind,recipe", CASES, ids=IDS)
def test_every_mutation_moves_the_oracle_by_ten_tolerances(kind, recipe):
    """Every mutation is applied as the catalogue names it and must move the float64 oracle by >= 10 x the tolerance of the same blob and
    inputs -- for the SNP kinds on the counts <= 30 and on the counts <= 160 inputs alike.  The replacement rule: a ("zero", ...) that does
    not reach it (the element happens to be small; most elements of a "wide" layer) is replaced by cnn_probe.substitute's "wrong" weight at
    the same index, which must reach it; and every layer keeps at least one true zeroing of a non-zero element that reaches it."""
    blob = P.synthetic_blob(kind, 0, recipe)
    n_head = 8                                  # (the layers behind fc1, element by element: many mutations, so fewer sites -- a smaller maximum)
    sets = []
    for what, inp in _input_sets(kind, 0, n_snp=48, n_indel=24):
        ref64 = P.oracle_forward(kind, blob, inp, "f64")
        sets.append((what, inp, ref64, P.tolerance(P.oracle_forward(kind, blob, inp, "f32"), ref64)))

    def moved(m, si, head):
        what, inp, ref64, tol = sets[si]
        got = P.oracle_forward(kind, P.mutate(blob, kind, m), tuple(a[:n_head] for a in inp) if head else inp, "f64")
        return float(np.abs(got.astype(np.float64) - (ref64[:n_head] if head else ref64)).max()) / tol

    weak, least, n_zero, n_sub, true_zero = [], {}, 0, 0, set()
    for m in P.mutations(kind):
        head = P.is_head(m) and m[0] == "zero"
        which = (0,) if P.is_head(m) else range(len(sets))           # (the heads see the trunk through fc1's 48 / 32 outputs only: one input set)
        r = min(moved(m, si, head) for si in which)
        if m[0] in ("zero", "zero_max"):
            n_zero += 1
            if r >= 10:
                if m[0] == "zero":
                    assert float(P.layer_view(blob, kind, m[1])[m[2]]) != 0.0
                true_zero.add(m[1])
            elif m[0] == "zero":
                n_sub += 1
                m = P.substitute(m)
                r = min(moved(m, si, head) for si in which)
        key = m[0] if m[0] == "fp16" else "%s %s" % (m[0], m[1])
        least[key] = min(least.get(key, np.inf), r)
        if not r >= 10:
            weak.append((m, r))
    print("%s %s: tol %s; %d of %d zeroings replaced by a wrong weight; least max|dp| / tol per layer and kind of mutation: %s" %
          (P.KIND_NAMES[kind], recipe, ", ".join("%.2e" % t[3] for t in sets), n_sub, n_zero, ", ".join("%s %.0f" % kv for kv in least.items())))
    assert not weak, weak[:10]
    assert true_zero == {name for name, _ in LAYER_SPECS[kind]}, sorted({name for name, _ in LAYER_SPECS[kind]} - true_zero)

"""Every CNN kernel route against the float64 oracle on synthetic, unsaturated weights (tests/cnn_probe.py; tests/test_cnn_probe_ref.py
proves on the oracle alone that one wrong tap, row or bias of such a blob moves the output by >= 10 x the tolerance used here).

Routes: SNP / haploid SNP  k4_conv12 + k3_fc1 (exact fp32), k5_trunk_p3 + k6_fc1_h3 on float32 and on int16 tensors (NC_TRUNK_LIN=0),
k5_trunk_lin + k6_fc1_h3 on int16 tensors, each with k_snp_heads / k_snp_hap_heads, both scale modes, probs and gt;
indel / haploid indel  k10_indel_trunk_h3 and the exact fp32 convolutions, each with k3_fc1 and k_indel_heads.
Three seeds per kind and recipe ("dense", "wide"), 1, 63, 257 and 1300 distinct sites.

Tolerance, per case and from the reference alone: max(8 x max|oracle_f32 - oracle_f64|, 1e-6) on the same blob and the same sites
(cnn_probe.tolerance: 4 x for the split's dropped lo x lo products, 2 x for another accumulation order; 1e-6: the oracle returns float32).

Measured on the MI355X, per kind and route, over the three seeds, both count ranges, both scale modes and the four site counts: the largest
max|dp| against the float64 oracle, the span of the run-time tolerances of those cases, and the largest error / tolerance of any one case.
  kind       route                          max|dp|   tol                  worst err / tol   (dense | wide)
  snp        k4_conv12 (fp32)               3.6e-07 | 4.2e-07   1.0e-06 .. 3.3e-06   0.13 | 0.13
  snp        k5_trunk_p3, float32 tensors   2.4e-07 | 3.0e-07   1.0e-06 .. 3.8e-06   0.09 | 0.11
  snp        k5_trunk_p3, int16 tensors     2.4e-07 | 3.0e-07   1.0e-06 .. 3.8e-06   0.09 | 0.11
  snp        k5_trunk_lin                   2.4e-07 | 2.4e-07   1.0e-06 .. 3.3e-06   0.12 | 0.08
  snp_hap    k4_conv12 (fp32)               1.8e-07 | 1.5e-07   1.0e-06 .. 1.9e-06   0.13 | 0.13
  snp_hap    k5_trunk_p3, float32 tensors   1.8e-07 | 1.2e-07   1.0e-06 .. 1.9e-06   0.11 | 0.09
  snp_hap    k5_trunk_p3, int16 tensors     1.8e-07 | 1.2e-07   1.0e-06 .. 1.9e-06   0.11 | 0.09
  snp_hap    k5_trunk_lin                   1.5e-07 | 1.5e-07   1.0e-06 .. 1.9e-06   0.12 | 0.12
  indel      k10_indel_trunk_h3             2.7e-07 | 3.3e-07   1.0e-06 .. 3.6e-06   0.10 | 0.12
  indel      fp32 convolutions              3.0e-07 | 3.3e-07   1.0e-06 .. 5.0e-06   0.10 | 0.15
  indel_hap  k10_indel_trunk_h3             2.7e-07 | 3.0e-07   1.0e-06 .. 4.3e-06   0.18 | 0.08
  indel_hap  fp32 convolutions              3.6e-07 | 4.2e-07   1.0e-06 .. 4.3e-06   0.13 | 0.10
  indel / indel_hap, fall-back to fp32 (x_limit 0.498): 1.2e-07 / 1.8e-07 (tol 1.4e-06 / 2.2e-06), default == exact mode bit for bit
  snp / snp_hap, partial re-run (127 of 257 sites flagged, all three split routes, both modes): 1.8e-07 / 8.9e-08 (tol 1.9e-06 / 1.0e-06)
The split-precision routes are as close to the oracle as the exact ones: no route needed more than a fifth of its tolerance.
(Each run prints its own figures.)

Two routes no shipped model reaches: the indel trunk's fall-back to the fp32 kernels when the weights' range bound does not cover
|x| <= 1, and a guarded SNP forward in which only some sites are re-run on the exact trunk."""
import contextlib
import os

import numpy as np
import pytest
import torch

import cnn_probe as P

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
COUNTS = ((1, 1299), (63, 600), (257, 900), (1300, 0))               # (sites, first site in the pool of 1300 distinct ones)
POOL = 1300
SNP = (P.KIND_SNP, P.KIND_SNP_HAP)
# (name, exact fp32, int16 tensors, NC_TRUNK_LIN, kernel)
SNP_ROUTES = (("fp32", True, False, None, "k4_conv12"), ("p3 f32", False, False, "0", "k5_trunk_p3"), ("p3 i16", False, True, "0", "k5_trunk_p3"),
              ("lin i16", False, True, None, "k5_trunk_lin"))


@pytest.fixture(scope="module")
def eng():
    """the shared engine; afterwards it forgets which files it holds, so that the next module's load_weights loads its model again instead
    of meeting a probe's (deleted) path or, by chance, an equal one"""
    from nanocaller_amd.engine import get_engine
    e = get_engine(0)
    yield e
    _restore(e)
    e._loaded.clear()


@contextlib.contextmanager
def _route(eng, exact, lin_env):
    """the engine on one SNP route (which tensors it takes is the tensors' dtype: _snp_run); the defaults restored afterwards"""
    old = os.environ.get("NC_TRUNK_LIN")
    try:
        if lin_env is None:
            os.environ.pop("NC_TRUNK_LIN", None)
        else:
            os.environ["NC_TRUNK_LIN"] = lin_env
        eng.set_cnn_precision(exact)
        yield
    finally:
        _restore(eng)
        if old is None:
            os.environ.pop("NC_TRUNK_LIN", None)
        else:
            os.environ["NC_TRUNK_LIN"] = old


def _restore(eng):
    eng.set_cnn_precision(False)
    eng.L.nc_cnn_range_watch(eng.ctx, None)


def _load(eng, tmp_path, kind, blob, tag):
    from nanocaller_amd.weights import Weights
    w = Weights(P.write_probe(tmp_path, kind, blob, tag=tag))           # (through the file: every probe has a path of its own)
    assert np.array_equal(w.flat, blob)
    eng.load_weights(kind, w)
    xl = eng.x_limit(kind)
    assert abs(xl - P.x_limit_bound(kind, blob)) <= 1e-5 * xl + 1e-6, (xl, P.x_limit_bound(kind, blob))
    return xl


def _snp_run(eng, kind, x, rc, scale, mode, i16):
    """-> outputs [n][6 | 4] as the oracle_forward of cnn_probe lays them out (probs | gt)"""
    dev = eng.device
    xd = torch.from_numpy(np.ascontiguousarray(x.astype(np.int16) if i16 else x)).to(dev)
    p, g = eng.snp_forward(kind, xd, torch.from_numpy(rc).to(dev), torch.from_numpy(scale).to(dev), mode)
    assert (g is not None) == (kind == P.KIND_SNP)
    return np.concatenate([p.cpu().numpy(), g.cpu().numpy()], axis=1) if g is not None else p.cpu().numpy()


def _report(what, err, tol):
    print("%-58s max|dp| %.2e   tol %.2e" % (what, err, tol))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("recipe", P.RECIPES)
@pytest.mark.parametrize("kind", SNP, ids=lambda k: P.KIND_NAMES[k])
def test_snp_routes_equal_the_oracle_on_unsaturated_weights(eng, tmp_path, kind, recipe, seed):
    blob = P.synthetic_blob(kind, seed, recipe)
    try:
        xl = _load(eng, tmp_path, kind, blob, "%s%d" % (recipe, seed))
        bad = []
        for hi in (30, 160):
            x, rc, scale = P.snp_inputs(seed, POOL, hi)
            assert np.unique(x.reshape(POOL, -1), axis=0).shape[0] == POOL and set(rc.tolist()) == {0, 1, 2, 3}
            assert float(np.abs(x).max()) == hi and float((np.abs(x[:, 1:, :, :4]).max(axis=(1, 2, 3)) * scale).max()) < min(xl, 2.01)   # inside the proven range
            for mode in (0, 1):
                r64 = P.oracle_forward(kind, blob, (x, rc, scale), "f64", scale_mode=mode)
                r32 = P.oracle_forward(kind, blob, (x, rc, scale), "f32", scale_mode=mode)
                for name, exact, i16, lin_env, kernel in SNP_ROUTES:
                    with _route(eng, exact, lin_env):
                        assert eng.trunk_info(int16=i16)[1] == kernel, (name, eng.trunk_info(int16=i16))
                        worst = (0.0, 0.0)
                        for n, s0 in COUNTS:
                            sl = slice(s0, s0 + n)
                            got = _snp_run(eng, kind, x[sl], rc[sl], scale[sl], mode, i16)
                            tol = P.tolerance(r32[sl], r64[sl])
                            err = float(np.abs(got.astype(np.float64) - r64[sl]).max())
                            worst = max(worst, (err / tol, err, tol))
                            if not err <= tol:
                                bad.append((name, hi, mode, n, err, tol))
                        _report("%s %s seed %d %s counts<=%d mode %d" % (P.KIND_NAMES[kind], recipe, seed, name, hi, mode), worst[1], worst[2])
        assert not bad, bad
    finally:
        _restore(eng)


def _indel_run(eng, kind, x, exact):
    eng.set_cnn_precision(exact)
    return eng.indel_forward(kind, torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)).cpu().numpy()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("recipe", P.RECIPES)
@pytest.mark.parametrize("kind", (P.KIND_INDEL, P.KIND_INDEL_HAP), ids=lambda k: P.KIND_NAMES[k])
def test_indel_routes_equal_the_oracle_on_unsaturated_weights(eng, tmp_path, kind, recipe, seed):
    blob = P.synthetic_blob(kind, seed, recipe)
    try:
        xl = _load(eng, tmp_path, kind, blob, "%s%d" % (recipe, seed))
        assert xl >= 1.0                                                # the default mode takes k10_indel_trunk_h3
        x, = P.probe_inputs(kind, seed, POOL)
        assert np.abs(x).max() == 1.0
        r64, r32 = P.oracle_forward(kind, blob, (x,), "f64"), P.oracle_forward(kind, blob, (x,), "f32")
        bad, full = [], {}
        for name, exact in (("k10_indel_trunk_h3", False), ("fp32 convolutions", True)):
            worst = (0.0, 0.0)
            for n, s0 in COUNTS:
                sl = slice(s0, s0 + n)
                got = _indel_run(eng, kind, x[sl], exact)
                tol = P.tolerance(r32[sl], r64[sl])
                err = float(np.abs(got.astype(np.float64) - r64[sl]).max())
                worst = max(worst, (err / tol, err, tol))
                if not err <= tol:
                    bad.append((name, n, err, tol))
                if n == POOL:
                    full[exact] = got
            _report("%s %s seed %d %s" % (P.KIND_NAMES[kind], recipe, seed, name), worst[1], worst[2])
        assert not np.array_equal(full[False], full[True])              # two routes indeed
        assert not bad, bad
    finally:
        _restore(eng)


@pytest.mark.parametrize("kind", (P.KIND_INDEL, P.KIND_INDEL_HAP), ids=lambda k: P.KIND_NAMES[k])
def test_indel_model_outside_the_range_bound_takes_the_fp32_kernels(eng, tmp_path, kind):
    """conv1 and conv2 scaled up (fc1 down by as much) until the bound on the clamped activations no longer covers |x| <= 1: the default
    mode must run the exact kernels, i.e. give the exact mode's result bit for bit, and that result is the oracle's"""
    base = P.synthetic_blob(kind, 0, "dense")
    f = np.sqrt(2.0 * P.x_limit_bound(kind, base))
    blob = P.rescaled(base, kind, f, f)
    try:
        xl = _load(eng, tmp_path, kind, blob, "fallback")
        assert 0.0 < xl < 1.0, xl
        x, = P.probe_inputs(kind, 7, 257)
        r64, r32 = P.oracle_forward(kind, blob, (x,), "f64"), P.oracle_forward(kind, blob, (x,), "f32")
        tol = P.tolerance(r32, r64)
        default, exact = _indel_run(eng, kind, x, False), _indel_run(eng, kind, x, True)
        err = float(np.abs(default.astype(np.float64) - r64).max())
        _report("%s fall-back to fp32 (x_limit %.3f)" % (P.KIND_NAMES[kind], xl), err, tol)
        assert np.array_equal(default, exact)
        assert err <= tol, (err, tol)
    finally:
        _restore(eng)


def _expected_flags(x, scale, mode, x_limit, lin):
    """the sites the range guard must flag, as the kernels compute it in float32: k5_trunk_p3 looks at every entry after scaling (rows 1..4,
    channels 0..3: x * float(s), or float(double(x) * s) in scale mode 1); k5_trunk_lin at max|count| * float(s) and the unscaled entries.
    (k5_trunk_lin's further conditions -- counts beyond 2048, scales outside (0, 64], 1 / s beyond fp16 -- hold for none of these sites.)"""
    xl = np.float32(x_limit)
    s32 = scale.astype(np.float32)
    cnt = x[:, 1:, :, :4]
    if lin:
        amax = np.abs(cnt).max(axis=(1, 2, 3)).astype(np.float32) * s32
    elif mode == 0:
        amax = np.abs(cnt * s32[:, None, None, None]).max(axis=(1, 2, 3))
    else:
        amax = np.abs((cnt.astype(np.float64) * scale[:, None, None, None]).astype(np.float32)).max(axis=(1, 2, 3))
    unscaled = np.float32(max(np.abs(x[:, 0]).max(), np.abs(x[:, 1:, :, 4]).max()))
    assert unscaled <= xl and scale.max() <= 64.0 and scale.min() > 1.0 / 60000.0 and np.abs(x).max() <= 2048
    return ~(amax <= xl)


@pytest.mark.parametrize("kind", SNP, ids=lambda k: P.KIND_NAMES[k])
def test_guarded_snp_forward_reruns_exactly_the_sites_beyond_the_bound(eng, tmp_path, kind):
    """conv1 scaled up (fc1 down) until x_limit falls inside the probe's scaled inputs (0.5 .. 2): only the sites beyond it are re-run"""
    base = P.synthetic_blob(kind, 0, "dense")
    blob = P.rescaled(base, kind, P.x_limit_bound(kind, base) / 1.2)
    try:
        xl = _load(eng, tmp_path, kind, blob, "partial")
        assert 1.0 < xl < 1.5, xl
        n = 257
        x, rc, scale = P.snp_inputs(3, n, 30)
        dev = eng.device
        rcd, sd = torch.from_numpy(rc).to(dev), torch.from_numpy(scale).to(dev)
        for mode in (0, 1):
            r64 = P.oracle_forward(kind, blob, (x, rc, scale), "f64", scale_mode=mode)
            tol = P.tolerance(P.oracle_forward(kind, blob, (x, rc, scale), "f32", scale_mode=mode), r64)
            with _route(eng, True, None):
                exact = _snp_run(eng, kind, x, rc, scale, mode, False)
            for name, _, i16, lin_env, kernel in SNP_ROUTES[1:]:
                with _route(eng, False, lin_env):
                    assert eng.trunk_info(int16=i16)[1] == kernel
                    unguarded = _snp_run(eng, kind, x, rc, scale, mode, i16)
                    xd = torch.from_numpy(np.ascontiguousarray(x.astype(np.int16) if i16 else x)).to(dev)
                    flags = torch.zeros(n, dtype=torch.uint8, device=dev)
                    eng.snp_forward(kind, xd, rcd, sd, mode, range_flags=flags)
                    flagged = flags.cpu().numpy().astype(bool)
                    pg, gg, n_rerun = eng.snp_forward_guarded(kind, xd, rcd, sd, mode)
                    guarded = np.concatenate([pg.cpu().numpy(), gg.cpu().numpy()], axis=1) if gg is not None else pg.cpu().numpy()
                assert 0 < n_rerun < n, (name, mode, n_rerun)
                assert n_rerun == int(flagged.sum())
                assert np.array_equal(flagged, _expected_flags(x, scale, mode, xl, kernel == "k5_trunk_lin")), (name, mode)
                assert np.array_equal(guarded[flagged], exact[flagged]), (name, mode)          # the exact kernel's rows, bit for bit
                assert np.array_equal(guarded[~flagged], unguarded[~flagged]), (name, mode)     # the split run's rows, bit for bit
                err = float(np.abs(guarded.astype(np.float64) - r64).max())
                _report("%s partial re-run %s mode %d (%d of %d sites)" % (P.KIND_NAMES[kind], name, mode, n_rerun, n), err, tol)
                assert err <= tol, (name, mode, err, tol)
    finally:
        _restore(eng)

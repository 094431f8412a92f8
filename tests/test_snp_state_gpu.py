"""The SNP step's per-call choices are call arguments: snp_featurize(int16=...) says which tensors it writes, snp_forward reads the format off the
tensor's dtype, and whatever a call changes in the context (tensor format, CNN precision, range watch: Engine._snp_state) is back as it was when
the call returns or raises.  One chunk of the ONT test world (a few hundred sites)."""
import numpy as np
import pytest
import torch

from nanocaller_amd import _lib
from nanocaller_amd.weights import Weights, get_SNP_model

from util import load_snp_case, load_world

pytestmark = pytest.mark.gpu

KIND = _lib.MODEL_SNP
SPAN = [(20_000, 60_000)]
SCAN = dict(mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    e = get_engine(0)
    path, _ = get_SNP_model("ONT-HG002")
    e.load_weights(KIND, Weights(path))
    e.set_cnn_precision(exact_fp32=False)
    e.set_tensor_format(int16=False)
    yield e
    e.set_cnn_precision(exact_fp32=False)
    e.set_tensor_format(int16=False)


def _featurize(eng, dpk, **kw):
    sites = eng.snp_scan(dpk, SPAN, **SCAN)
    return eng.snp_featurize(dpk, sites, seq="ont", maxcov=160, **kw)


@pytest.fixture(scope="module")
def world_tensors(eng):
    """-> (DevicePack, x int16, x float32, ref_code, scale) of the chunk; shared, never written to"""
    from nanocaller_amd.pack import pack_world
    dpk = eng.upload(pack_world(load_world("ont")))
    s16 = _featurize(eng, dpk, int16=True)
    s32 = _featurize(eng, dpk, int16=False)
    scale, _ = eng.snp_scale(s32, 1, get_SNP_model("ONT-HG002")[1])
    assert 100 < s16.n_sites == s32.n_sites < 2000
    return dpk, s16.x, s32.x, s32.ref_code, scale


def _state(eng):
    return eng.x_int16, eng.exact_fp32, eng.trunk_info()


def test_the_featurisers_formats_hold_the_same_values(eng, world_tensors):
    _, x16, x32, _, _ = world_tensors
    assert x16.dtype == torch.int16 and x32.dtype == torch.float32 and x16.shape == x32.shape
    assert torch.equal(x16.to(torch.float32), x32)


@pytest.mark.parametrize("fmt", ["int16", "float32"])
def test_forward_reads_the_format_off_the_dtype(eng, world_tensors, fmt):
    """the engine's default format plays no part: the same tensor gives the same bits whatever set_tensor_format last said"""
    _, x16, x32, rc, scale = world_tensors
    x = x16 if fmt == "int16" else x32
    got = []
    try:
        for default16 in (False, True):
            eng.set_tensor_format(int16=default16)
            p, g = eng.snp_forward(KIND, x, rc, scale)
            assert _state(eng)[0] == default16
            got.append((p.clone(), g.clone()))
    finally:
        eng.set_tensor_format(int16=False)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert bool(torch.isfinite(got[0][0]).all()) and 0.0 <= float(got[0][0].min()) and float(got[0][0].max()) <= 1.0


def test_default_format_is_the_featurisers_default(eng, world_tensors):
    dpk, x16, x32, _, _ = world_tensors
    try:
        assert _featurize(eng, dpk).x.dtype == torch.float32
        eng.set_tensor_format(int16=True)
        s = _featurize(eng, dpk)
        assert s.x.dtype == torch.int16 and torch.equal(s.x, x16)
        s = _featurize(eng, dpk, int16=False)                               # the argument wins
        assert s.x.dtype == torch.float32 and torch.equal(s.x, x32) and eng.x_int16 is True
    finally:
        eng.set_tensor_format(int16=False)


def test_a_pack_with_mates_gives_float32_tensors_with_the_int16_routes_values(eng):
    """alignments that share read names are keyed by name in the int16 kernel only: float32 tensors are its result, cast"""
    from nanocaller_amd.wire import build_wire_from_world, upload_wire
    world, dct, region, _, gold = load_snp_case("ont_mates")
    dpk = upload_wire(eng, build_wire_from_world(world, supplementary=True))
    assert dpk.mates is not None
    out = {}
    for key, kw in (("default", {}), ("float32", dict(int16=False)), ("int16", dict(int16=True))):
        before = _state(eng)
        sites = eng.snp_scan(dpk, [(region["start"], region["end"])], mincov=dct["mincov"], min_allele_freq=dct["min_allele_freq"], threshold=dct["threshold"])
        eng.snp_featurize(dpk, sites, seq=dct["seq"], maxcov=dct["maxcov"], min_nbr_sites=dct["min_nbr_sites"], **kw)
        assert _state(eng) == before == (False, False, eng.trunk_info())
        out[key] = sites.x
    assert out["default"].dtype == out["float32"].dtype == torch.float32 and out["int16"].dtype == torch.int16
    assert torch.equal(out["default"], out["int16"].to(torch.float32)) and torch.equal(out["float32"], out["default"])
    assert np.array_equal(out["default"].cpu().numpy(), gold["mat"])          # the reference's tensors (float32 in the golden)


@pytest.mark.parametrize("default16", [False, True])
def test_every_call_leaves_the_state_as_it_found_it(eng, world_tensors, default16):
    """each call is given tensors of the format the engine's default is NOT, so that it has to change the context and put it back"""
    dpk, x16, x32, rc, scale = world_tensors
    x = x32 if default16 else x16
    n = int(x.shape[0])
    try:
        eng.set_tensor_format(int16=default16)
        before = _state(eng)
        assert before[:2] == (default16, False) and before[2][1] == ("k5_trunk_lin" if default16 else "k5_trunk_p3")
        _featurize(eng, dpk, int16=not default16)
        assert _state(eng) == before
        flags = torch.zeros(n, dtype=torch.uint8, device=eng.device)
        probs, gt = eng.snp_forward(KIND, x, rc, scale, range_flags=flags)
        assert _state(eng) == before
        eng.snp_forward_guarded(KIND, x, rc, scale)
        assert _state(eng) == before
        eng.range_rerun(KIND, x, rc, scale, 0, torch.arange(0, n, 7, device=eng.device), probs, gt)
        assert _state(eng) == before
        assert eng.trunk_info(int16=not default16)[1] == ("k5_trunk_p3" if default16 else "k5_trunk_lin")
        assert _state(eng) == before
    finally:
        eng.set_tensor_format(int16=False)


def test_an_error_return_leaves_the_state_as_it_was(eng, world_tensors):
    """error RETURNS of the library, answered before any launch: not an SNP model kind (NC_ERR_ARG), int16 tensors for the exact fp32 trunk
    (NC_ERR_STATE)"""
    _, x16, x32, rc, scale = world_tensors
    n = int(x16.shape[0])
    before = _state(eng)
    assert before[:2] == (False, False)
    flags = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    with pytest.raises(_lib.NanoCallerHipError, match="not an SNP model kind"):
        eng.snp_forward(_lib.MODEL_INDEL, x16, rc, scale, range_flags=flags)
    assert _state(eng) == before
    # (the watch went with the failed call: a forward far beyond x_limit marks nothing in `flags`)
    eng.snp_forward(KIND, x32, rc, scale * (2.0 * eng.x_limit(KIND)))
    assert int(flags.sum().item()) == 0
    try:
        eng.set_cnn_precision(exact_fp32=True)
        exact = _state(eng)
        assert exact[:2] == (False, True) and exact[2][1] == "k4_conv12"
        with pytest.raises(_lib.NanoCallerHipError, match="split-precision trunk only"):
            eng.snp_forward(KIND, x16, rc, scale)
        assert _state(eng) == exact
    finally:
        eng.set_cnn_precision(exact_fp32=False)
    assert _state(eng) == before


def test_a_tensor_of_another_dtype_is_refused_before_any_library_call(eng, world_tensors, monkeypatch):
    _, _, x32, rc, scale = world_tensors

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)
    x64 = x32[:8].to(torch.float64)
    monkeypatch.setattr(eng, "L", NoLibrary())
    for x in (x64, x32[:8].to(torch.float16), x32[:8].to(torch.int32)):
        with pytest.raises(ValueError, match="int16 or float32"):
            eng.snp_forward(KIND, x, rc[:8], scale[:8])


@pytest.mark.parametrize("fmt", ["int16", "float32"])
def test_the_guarded_forward_reruns_exactly_the_rows_beyond_the_limit(eng, world_tensors, fmt):
    """a few rows get one count that, scaled, lies beyond x_limit: the guard marks exactly those, the exact fp32 trunk computes them again, and
    the whole result is the exact trunk's within the 1e-4 of test_cnn_range.py (the re-run rows: its bits)"""
    _, x16, _, rc, scale = world_tensors
    xl = eng.x_limit(KIND)
    n = int(x16.shape[0])
    rows = [3, 17, n - 1]
    x_h = x16.cpu().numpy().copy()
    s_h = scale.cpu().numpy().copy()
    for k in rows:
        x_h[k, 2, 5, 1] = int(xl / 1.5) + 2
        s_h[k] = 1.5
    amax = np.abs(x_h[:, 1:, :, :4]).max(axis=(1, 2, 3)).astype(np.float32) * s_h.astype(np.float32)
    assert sorted(np.flatnonzero(amax > np.float32(xl)).tolist()) == rows        # on the host: these rows and no others leave the proven range
    x32 = torch.from_numpy(x_h.astype(np.float32)).to(eng.device)
    x = torch.from_numpy(x_h).to(eng.device) if fmt == "int16" else x32
    sd = torch.from_numpy(s_h).to(eng.device)
    try:
        eng.set_cnn_precision(exact_fp32=True)
        pe, ge = eng.snp_forward(KIND, x32, rc, sd)
    finally:
        eng.set_cnn_precision(exact_fp32=False)
    flags = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    eng.snp_forward(KIND, x, rc, sd, range_flags=flags)
    assert torch.nonzero(flags).flatten().tolist() == rows
    pg, gg, n_rerun = eng.snp_forward_guarded(KIND, x, rc, sd)
    assert n_rerun == len(rows)
    assert float((pg - pe).abs().max()) < 1e-4 and float((gg - ge).abs().max()) < 1e-4
    assert torch.equal(pg[rows], pe[rows]) and torch.equal(gg[rows], ge[rows])

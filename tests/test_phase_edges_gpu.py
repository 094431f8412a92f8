"""GPU: the device phaser at the ends of its input space (instances of tests/phase_edges.py; tests/test_phase_edges_ref.py shows that each reaches
its edge) -- k_hp_dp's 16-bit relative costs at exactly 65,535 (solved, equal to the restatements) and at 65,536 (NC_ERR_CAPACITY, nothing left
behind in the context), a handle whose second solve fails (it refuses nc_haplotag_run and views as unsolved), every (continuing, leaving) pair of
slot transitions on interleaved slots in more blocks than the device has compute units, and k_hp_quals on CIGAR operations beyond 65,535 bases.
Every comparison is exact.

Measured on an MI355X (`ms` of the result, printed by test_range_at_the_edge_solves), k_hp_dp's part of the solve: the 65,535-column unit members
109 ms (plain) and 125 ms (genotype-aware) -- 1.7 - 1.9 us per column at four states --, the 705-column weighted members 3.2 - 3.6 ms, the
fifteen-read members 8.1 - 8.4 ms for 102 columns of 2^15 states; the haplotagger 24 ms on the two 65,535-entry reads."""
import ctypes as C

import numpy as np
import pytest

import phase_edges as E
from phase_w_ref import flat_weights
from test_phase_gpu import _assert_equal_to_restatement, _csr, eng  # noqa: F401
from test_phase_gt_gpu import _assert_equal as _assert_equal_gt
from test_phase_w_gpu import _assert_equal as _assert_equal_w
from test_phase_w_gpu import _expected_weights

pytestmark = pytest.mark.gpu

NC_ERR_STATE = -5                # include/nanocaller_hip.h


@pytest.fixture(scope="module")
def members():
    return E.range_members()


def _solve(eng, t, form, **kw):  # noqa: F811
    w, ok, gt = E.form_arguments(form, t["weights"], t["read_ok"], t["gt"])
    if w is not None:
        kw["weights"] = (flat_weights(w), ok)
    if gt is not None:
        kw.update(site_gt=gt, distrust_cost=t["G"])
    return eng.snp_phase(t["pos"], None, t["groups"], int(t["groups"].max()) + 1, max_cov=t["max_cov"], csr=_csr(t["reads"]), **kw)


def _assert_restatement(got, t, form):
    """the comparison helper of the form's own test module: the arrays key by key, block cost and haplotags included"""
    w, ok, gt = E.form_arguments(form, t["weights"], t["read_ok"], t["gt"])
    if w is not None:
        return _assert_equal_w(got, t["reads"], w, ok, t["pos"], t["groups"], t["max_cov"], gt, t["G"])
    if gt is not None:
        return _assert_equal_gt(got, t["reads"], t["pos"], t["groups"], gt, t["G"], t["max_cov"])
    return _assert_equal_to_restatement(got, t["reads"], t["pos"], t["groups"], t["max_cov"])


def _assert_closed_form(got, t, with_gt):
    """a two_reads member against its closed form (the restatements' solve: tests/test_phase_edges_ref.py), the same keys"""
    ref, hp, ps = E.two_reads_closed_form(t)
    for k in ("side", "site_block", "site_h", "site_phased", "site_ps") + (("site_gt",) if with_gt else ()):
        assert np.array_equal(got[k], ref[k]), k
    assert [tuple(int(v) for v in b) for b in zip(got["block_first"], got["block_last"], got["block_ps"], got["block_cost"])] == ref["blocks"]
    assert np.array_equal(got["group_hp"], hp) and np.array_equal(got["group_ps"], ps)


def _same_arrays(a, b):
    assert set(a) == set(b)
    for k in a:
        if k != "ms":
            assert np.array_equal(a[k], b[k]), k


CASES = [(name, form) for name in ("weighted", "unit", "fifteen") for form in (("ff", "Gf") if name == "unit" else ("fW", "GW"))]


@pytest.mark.parametrize("name,form", CASES)
def test_range_at_the_edge_solves(eng, members, name, form):  # noqa: F811
    t, forms, spread = members[name + "-edge"]
    assert form in forms and spread == E.EDGE
    got = _solve(eng, t, form)
    print("%s %s: %d sites, spread %d, ms %s" % (name, form, t["n_sites"], spread, got["ms"]))
    if name == "unit":
        _assert_closed_form(got, t, form[0] == "G")
    else:
        _assert_restatement(got, t, form)
        if name == "weighted":
            _assert_closed_form(got, t, form[0] == "G")
    assert got["site_phased"].all() and got["block_cost"].size == 1


@pytest.mark.parametrize("name,form", CASES)
def test_range_one_beyond_is_refused(eng, members, name, form):  # noqa: F811
    from nanocaller_amd import _lib
    t, forms, spread = members[name + "-over"]
    assert form in forms and spread == E.EDGE + 1
    with pytest.raises(_lib.NanoCallerHipError, match="65535") as e:
        _solve(eng, t, form)
    assert e.value.status == _lib.NC_ERR_CAPACITY


@pytest.mark.parametrize("name,form", [("weighted", "fW"), ("fifteen", "GW"), ("unit", "ff")])
def test_range_after_a_refusal_the_edge_solves_as_before(eng, members, name, form):  # noqa: F811
    from nanocaller_amd import _lib
    t = members[name + "-edge"][0]
    before = _solve(eng, t, form)
    with pytest.raises(_lib.NanoCallerHipError) as e:
        _solve(eng, members[name + "-over"][0], form)
    assert e.value.status == _lib.NC_ERR_CAPACITY
    _same_arrays(_solve(eng, t, form), before)


@pytest.fixture(scope="module")
def transitions():
    return E.transition_instance()[0]


@pytest.mark.parametrize("form", E.FORMS)
def test_transitions_equal_the_restatements(eng, transitions, form):  # noqa: F811
    t = transitions
    got = _solve(eng, t, form)
    ref = _assert_restatement(got, t, form)
    assert len(ref["blocks"]) > 256 and ref["accepted"].all() and (got["group_hp"] > 0).sum() > 1000


@pytest.mark.parametrize("w_max,default_weight,mapq_min", [(93, 30, 20), (50, 7, 0)])
def test_qualities_of_long_operation_records(eng, w_max, default_weight, mapq_min):  # noqa: F811
    import bamio_w
    import torch
    recs = E.long_op_records()
    pos, reads = E.long_op_csr(recs)
    raw, off = bamio_w.record_stream(recs)
    groups = np.arange(len(recs), dtype=np.int32)
    got = eng.snp_phase(pos, None, groups, len(recs), csr=_csr(reads),
                        bam_quals=(torch.from_numpy(raw).to(eng.device), torch.from_numpy(off).to(eng.device), mapq_min, default_weight, w_max))
    want = _expected_weights(recs, reads, pos, default_weight, w_max)
    k = 0
    for r, rd in zip(recs, reads):                                       # record by record, so that a failure names its CIGAR
        assert np.array_equal(got["entry_weight"][k:k + len(rd)], want[k:k + len(rd)]), r["name"]
        k += len(rd)
    mapq = np.array([r["mapq"] for r in recs], np.uint8)
    assert np.array_equal(got["read_mapq"], mapq) and np.array_equal(got["read_ok"], (mapq >= mapq_min).astype(np.uint8))
    assert (want == default_weight).sum() > 20 and (want == w_max).any() and len(set(want.tolist())) > 30
    weights, k = [], 0
    for rd in reads:
        weights.append(want[k:k + len(rd)].tolist())
        k += len(rd)
    ref = _assert_equal_w(got, reads, weights, got["read_ok"], pos, groups)
    assert sum(b[3] for b in ref["blocks"]) > 1000                       # the solve's costs are sums of those weights


def test_a_failed_second_solve_leaves_the_handle_unsolved(eng, members):  # noqa: F811
    """the C ABI on one handle: a solve that fails after one that succeeded must not leave the first one's `solved` behind"""
    from nanocaller_amd import _lib
    L, ctx = eng.L, eng.ctx
    t = members["weighted-over"][0]
    real = flat_weights(t["weights"])
    grp = np.ascontiguousarray(t["groups"], np.int32)
    gt = np.ascontiguousarray(t["gt"], np.uint8)

    def tag(h):
        return L.nc_haplotag_run(ctx, h, 2, _lib.npp(grp))

    def assert_unsolved(h):
        assert tag(h) == NC_ERR_STATE
        v = eng._phase_view(h)
        assert v.n_blocks == 0 and v.n_groups == 0 and v.n_reads == 2 and v.n_entries == real.size and v.entry_off
        for k in ("read_side", "site_block", "site_h", "site_phased", "site_ps", "block_first", "block_last", "block_ps", "block_cost"):
            assert not getattr(v, k), k
        g = C.c_void_p()
        assert L.nc_snp_phase_genotypes(h, C.byref(g)) == _lib.NC_OK and not g.value

    def assert_solved(h):
        assert tag(h) == _lib.NC_OK
        v = eng._phase_view(h)
        assert v.n_blocks == 1 and v.read_side and v.site_h and v.block_ps and v.group_hp

    # a setter between the solves: unit weights solve (spread 705), the real weights overflow
    h = eng._phase_open(t["pos"], None, None, _csr(t["reads"]), None)
    try:
        assert L.nc_snp_phase_set_weights(ctx, h, None, None) == _lib.NC_OK
        assert L.nc_snp_phase_solve(ctx, h, 15) == _lib.NC_OK
        assert_solved(h)
        assert L.nc_snp_phase_set_weights(ctx, h, _lib.npp(real), None) == _lib.NC_OK
        assert L.nc_snp_phase_solve(ctx, h, 15) == _lib.NC_ERR_CAPACITY
        assert_unsolved(h)
    finally:
        L.nc_snp_phase_free(h)
    # no setter between the solves: unit costs solve; with the weights set, one read (max_cov 1: no split state) solves, and both reads overflow
    # in the plain and in the genotype-aware solve
    h = eng._phase_open(t["pos"], None, None, _csr(t["reads"]), None)
    try:
        assert L.nc_snp_phase_solve(ctx, h, 15) == _lib.NC_OK
        assert_solved(h)
        assert L.nc_snp_phase_set_weights(ctx, h, _lib.npp(real), None) == _lib.NC_OK
        assert tag(h) == NC_ERR_STATE                                    # (the setter itself asks for a new solve)
        assert L.nc_snp_phase_solve(ctx, h, 1) == _lib.NC_OK
        assert_solved(h)
        assert L.nc_snp_phase_solve(ctx, h, 15) == _lib.NC_ERR_CAPACITY
        assert b"65535" in L.nc_last_error(ctx)
        assert_unsolved(h)
        assert L.nc_snp_phase_solve(ctx, h, 1) == _lib.NC_OK
        assert_solved(h)
        assert L.nc_snp_phase_solve_gt(ctx, h, 15, _lib.npp(gt), t["G"]) == _lib.NC_ERR_CAPACITY
        assert_unsolved(h)
        assert L.nc_snp_phase_solve_gt(ctx, h, 1, _lib.npp(gt), t["G"]) == _lib.NC_OK
        assert_solved(h)
        g = C.c_void_p()
        assert L.nc_snp_phase_genotypes(h, C.byref(g)) == _lib.NC_OK and g.value
    finally:
        L.nc_snp_phase_free(h)

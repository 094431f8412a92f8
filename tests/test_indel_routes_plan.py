"""generate_indel_pileups.plan_routes: which chunks of a list take the device pipeline and which the host-assembled route.  CPU, no engine: the
split's chunk mask is passed in, and every other case is decided from the arguments alone."""
import numpy as np
import pytest

from nanocaller_amd import _lib
from nanocaller_amd import generate_indel_pileups as gip
from nanocaller_amd.synth import World

DCT = dict(seq="ont", fasta_path="r.fa", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6, supplementary=False,
           exclude_bed=None, impute_indel_phase=False)
IMPUTE = dict(DCT, impute_indel_phase=True)


def _chunks(spans, sam_path="reads.bam"):
    return [dict(chrom="chrT", start=a, end=b, sam_path=sam_path) for a, b in spans]


FOUR = _chunks([(1, 10_000), (10_001, 20_000), (20_001, 30_000), (30_001, 40_000)])


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    """the plan is made without the library (the one case that scans, route="split" without a mask, is a GPU test's)"""
    def boom(*a, **k):
        raise AssertionError("plan_routes called the library")
    monkeypatch.setattr(_lib, "lib", boom)


def test_default_is_one_device_part():
    assert gip.plan_routes(DCT, FOUR, False) == [("device", [0, 1, 2, 3], DCT)]
    assert gip.plan_routes(IMPUTE, FOUR, False) == [("device", [0, 1, 2, 3], IMPUTE)]      # the device pipeline groups the reads itself
    assert gip.plan_routes(DCT, FOUR, False)[0][2] is DCT


def test_route_host_sends_everything_to_the_host():
    for dct, haploid in ((DCT, False), (DCT, True), (IMPUTE, False)):
        assert gip.plan_routes(dct, FOUR, haploid, route="host") == [("host", [0, 1, 2, 3], dct)]


def test_alignments_that_are_not_a_bam_path_go_to_the_host():
    z = np.zeros(0, np.int32)
    w = World(chrom="chrT", ref="ACGT", read_start=z, read_end=z, read_flag=z, read_off=np.zeros(1, np.int64), codes=np.zeros(0, np.uint8))
    for route in (None, "split"):
        assert gip.plan_routes(IMPUTE, _chunks([(1, 2), (3, 4)], sam_path=w), False, route=route) == [("host", [0, 1], IMPUTE)]


def test_nested_chunks_go_to_the_host():
    """sorted by (start, end) their ends do not ascend: the device plan takes no such list"""
    assert gip.plan_routes(DCT, _chunks([(1, 5000), (1000, 3000)]), False) == [("host", [0, 1], DCT)]
    assert gip.plan_routes(DCT, _chunks([(1000, 3000), (1, 5000)]), False) == [("host", [0, 1], DCT)]
    # out of order, but monotone once sorted; overlapping, but ends ascending: the device takes them
    assert gip.plan_routes(DCT, _chunks([(5001, 9000), (1, 5000)]), False) == [("device", [0, 1], DCT)]
    assert gip.plan_routes(DCT, _chunks([(1, 5000), (1000, 6000)]), False) == [("device", [0, 1], DCT)]


def test_haploid_with_impute_indel_phase_is_one_device_part_with_the_dct_unchanged():
    for route in (None, "split"):
        plan = gip.plan_routes(IMPUTE, FOUR, True, route=route, mask=[True, False, True, False])
        assert plan == [("device", [0, 1, 2, 3], IMPUTE)] and plan[0][2] is IMPUTE


def test_split_sends_the_masked_chunks_to_the_host_and_the_rest_to_the_device_with_the_flag_off():
    plan = gip.plan_routes(IMPUTE, FOUR, False, route="split", mask=[True, True, False, False])
    assert [(k, idx) for k, idx, _ in plan] == [("device", [2, 3]), ("host", [0, 1])]
    assert plan[0][2] == dict(IMPUTE, impute_indel_phase=False) and plan[1][2] is IMPUTE
    assert IMPUTE["impute_indel_phase"] is True                                            # the caller's dct is not written to
    # the mask is per chunk in the order given, whatever that order is
    back = FOUR[::-1]
    plan = gip.plan_routes(IMPUTE, back, False, route="split", mask=[False, False, True, True])
    assert [(k, idx) for k, idx, _ in plan] == [("device", [0, 1]), ("host", [2, 3])]
    # nothing masked: one device part, still with the flag off (no chunk has a column for the rule)
    plan = gip.plan_routes(IMPUTE, FOUR, False, route="split", mask=[False] * 4)
    assert plan == [("device", [0, 1, 2, 3], dict(IMPUTE, impute_indel_phase=False))]


def test_split_with_every_chunk_masked_is_all_host():
    assert gip.plan_routes(IMPUTE, FOUR, False, route="split", mask=[True] * 4) == [("host", [0, 1, 2, 3], IMPUTE)]


def test_split_without_the_flag_plans_as_the_default():
    assert gip.plan_routes(DCT, FOUR, False, route="split", mask=[True] * 4) == gip.plan_routes(DCT, FOUR, False)


def test_an_unknown_route_is_a_value_error():
    for route in ("nonsense", "device", True, 0):
        with pytest.raises(ValueError):
            gip.plan_routes(DCT, FOUR, False, route=route)
    with pytest.raises(ValueError):
        gip.get_indel_testing_candidates_batch(DCT, FOUR, route="nonsense")


def test_the_retired_environment_switches_change_nothing(monkeypatch):
    """the six process-wide switches the routes once hung on, at the values that used to turn something: the plan does not read them"""
    want = [gip.plan_routes(d, FOUR, h) for d in (DCT, IMPUTE) for h in (False, True)]
    for name, value in (("INDEL_HOST_PASS2", "1"), ("IMPUTE_SPLIT", "0"), ("IMPUTE_DEVICE", "0"), ("INDEL_PY_RULES", "1"), ("MSA_NO_DEDUP", "1"),
                        ("KEEP_GC", "1")):
        monkeypatch.setenv("NC_" + name, value)
    assert [gip.plan_routes(d, FOUR, h) for d in (DCT, IMPUTE) for h in (False, True)] == want
    assert want[0] == [("device", [0, 1, 2, 3], DCT)] and want[2] == [("device", [0, 1, 2, 3], IMPUTE)]

"""The host-side planning of snpCaller.caller, without a GPU and without an engine: which groups form a run on the device ingest route
(_plan_runs, a pure function of device_bam.plan_shares' answer), the span rule a rank's partial contig is decoded by (generate_SNP_pileups.span_of,
shared by contig_span and the device route's _prepare_device), and call_chunks' refusal of the removed pipelined-CNN path."""
import pytest

from nanocaller_amd import _lib, device_bam, snpCaller
from nanocaller_amd import generate_SNP_pileups as gsp

KEYS = [("a", "diploid"), ("a", "haploid"), ("b", "diploid"), ("c", "diploid"), ("d", "diploid"), ("e", "diploid")]


def test_plan_runs_follows_the_shares(monkeypatch):
    asked = []

    def shares(path, order, limit, device=0):
        asked.append((path, list(order), limit, device))
        return [(["a", "b"], True), (["c"], False), (["d", "e"], True)]
    monkeypatch.setattr(device_bam, "plan_shares", shares)
    monkeypatch.delenv("NC_DEVICE_INGEST_SHARE_GB", raising=False)
    run_end, run_dev = snpCaller._plan_runs(dict(sam_path="x.bam"), KEYS, 3)
    assert run_end == [3, 3, 3, 4, 6, 6]
    assert run_dev == [("a", "b")] * 3 + [None] + [("d", "e")] * 2
    assert asked == [("x.bam", ["a", "b", "c", "d", "e"], None, 3)]          # every contig once, in the groups' order; no limit of its own
    monkeypatch.setenv("NC_DEVICE_INGEST_SHARE_GB", "0.5")
    snpCaller._plan_runs(dict(sam_path="x.bam"), KEYS, 0)
    assert asked[-1][2] == 1 << 29


def test_plan_runs_without_the_device_route(monkeypatch):
    def shares(*a, **k):
        raise device_bam.DeviceIngestUnavailable("no index")
    monkeypatch.setattr(device_bam, "plan_shares", shares)
    run_end, run_dev = snpCaller._plan_runs(dict(sam_path="x.bam"), KEYS, 0)
    assert run_end == [len(KEYS)] * len(KEYS) and run_dev == [None] * len(KEYS)
    assert snpCaller._plan_runs(dict(sam_path="x.bam"), [], 0) == ([], [])


def _chunks(*spans):
    return [dict(chrom="c", start=a, end=b, ploidy="diploid") for a, b in spans]


def test_span_rule():
    F = _lib.FLANK
    assert F == 50_000
    L = 10_000_000
    assert gsp.span_of(_chunks((3_000_000, 3_100_000), (3_100_000, 3_250_000)), L) == (3_000_000 - F, 3_250_000 + F)     # extent +- flank
    assert gsp.span_of(_chunks((3_100_000, 3_250_000), (3_000_000, 3_100_000)), L) == (3_000_000 - F, 3_250_000 + F)     # (any order)
    assert gsp.span_of(_chunks((1, 100_000)), L) == (1, 100_000 + F)                                                     # clipped at 1 ...
    assert gsp.span_of(_chunks((9_000_000, L)), L) == (9_000_000 - F, L)                                                 # ... and at the length
    assert gsp.span_of(_chunks((9_000_000, L + 500)), L) == (9_000_000 - F, L)
    # None from 90 % of the contig on: lo = 1, hi = end + F covers end + F bases
    assert gsp.span_of(_chunks((1, 9_000_000 - F - 1)), L) == (1, 8_999_999)
    assert gsp.span_of(_chunks((1, 9_000_000 - F)), L) is None
    assert gsp.span_of(_chunks((1, L)), L) is None
    assert gsp.span_of(_chunks((1, 1000)), 0) is None                        # (a contig the file does not know: length 0)


def test_span_rule_is_contig_spans(tmp_path, monkeypatch):
    """the values of test_gpu_parity's split-contig test: a 420 kb contig, chunks 150,000 .. 260,000"""
    from nanocaller_amd import bam

    class FakeBam:
        def __init__(self, path):
            pass

        def get_reference_length(self, chrom):
            return 420_000

        def close(self):
            pass
    monkeypatch.setattr(bam, "BamFile", FakeBam)
    path = str(tmp_path / "s.bam")
    open(path, "wb").close()
    for chunks in (_chunks((150_000, 200_000), (200_000, 260_000)), _chunks((1, 200_000), (200_000, 420_000)), _chunks((30_000, 60_000))):
        assert gsp.contig_span(path, "c", chunks) == gsp.span_of(chunks, 420_000)
    assert gsp.span_of(_chunks((150_000, 200_000), (200_000, 260_000)), 420_000) == (100_000, 310_000)
    assert gsp.contig_span(object(), "c", _chunks((1, 10))) is None          # (not a file: the whole contig)


def test_call_chunks_refuses_the_removed_pipelined_path(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(snpCaller, "get_engine", no_engine)
    with pytest.raises(ValueError, match="pipelined-CNN"):
        snpCaller.call_chunks({}, _chunks((1, 10)), pipeline=True)
    assert not hasattr(snpCaller, "_PENDING_CNN") and not hasattr(snpCaller, "flush_pending_cnn")

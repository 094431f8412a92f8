"""CPU-only: bench.py reports counter traffic only from passes taken on the kernel sources it runs (tools/build_tag.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_traffic_records_of_another_build_are_refused():
    import bench
    from build_tag import INDEL_SOURCES, TRUNK_SOURCES, build_tag
    for name, sources in (("trunk_traffic.json", TRUNK_SOURCES), ("indel_traffic.json", INDEL_SOURCES)):
        rec = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert len(rec.get("build_tag", "")) == 16 and rec["build_tag_of"] == list(sources)
        ok, note = bench.traffic_build_check(dict(rec, build_tag=build_tag(sources)), sources)
        assert ok and note is None
        ok, note = bench.traffic_build_check(dict(rec, build_tag="0" * 16), sources)
        assert not ok and "another build" in note
        ok, note = bench.traffic_build_check({k: v for k, v in rec.items() if k != "build_tag"}, sources)      # a record from before the tags
        assert not ok


def test_dump_outputs_writes_float_arrays_and_samples_rows_over_the_limit(tmp_path):
    """bench.py --dump-outputs: every array of a call_chunks result as <name>.npy, float32 / float64 holding the values exactly; over
    the size limit the per-site arrays keep the same seeded rows (sample_rows.npy), and two dumps of one result are identical"""
    import numpy as np
    import bench
    n = 1000
    rng = np.random.default_rng(1)
    res = dict(chrom="chr20", ploidy="diploid", n=n, range_reruns=0, pos=np.sort(rng.integers(1, 64_000_000, n)).astype(np.int32),
               probs=rng.random((n, 4), dtype=np.float32), dp=rng.integers(0, 200, n).astype(np.int32), freq=rng.random(n),
               ref=rng.integers(0, 4, n).astype(np.uint8), chunk_depth=np.arange(7, dtype=np.float32))
    names = bench.dump_outputs(res, str(tmp_path / "a"))
    assert names == ["chunk_depth", "dp", "freq", "pos", "probs", "ref"]
    for k in names:
        v = np.load(str(tmp_path / "a" / (k + ".npy")))
        assert v.dtype in (np.float32, np.float64) and np.array_equal(v, res[k]), k
    assert np.load(str(tmp_path / "a" / "pos.npy")).dtype == np.float64           # positions past 2^24: float32 would round them
    limit = 20_000
    names = bench.dump_outputs(res, str(tmp_path / "b"), limit=limit)
    assert "sample_rows" in names
    rows = np.load(str(tmp_path / "b" / "sample_rows.npy")).astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    total = 0
    for k in names:
        v = np.load(str(tmp_path / "b" / (k + ".npy")))
        total += v.nbytes
        if k not in ("sample_rows", "chunk_depth"):
            assert np.array_equal(v, res[k][rows]), k
    assert total <= limit
    bench.dump_outputs(res, str(tmp_path / "c"), limit=limit)
    for k in names:
        assert np.array_equal(np.load(str(tmp_path / "b" / (k + ".npy"))), np.load(str(tmp_path / "c" / (k + ".npy"))))

"""CPU: the BAM index helper (tests/bam_index_ref.py) on its own, against the indexes tests/bamio.py writes and the spec-derived fixture; and
the library's numpy assembly (nanocaller_amd/bam_index.index_bytes) against the helper's byte for byte."""
import gzip
import os

import numpy as np
import pytest

from tests import bam_index_ref as ref
from tests import bamio

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def world_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("ixref")
    w = bamio.make_bam_world()
    bam = str(d / "w.bam")
    recs = bamio.world_to_records(w, np.random.default_rng(2))
    bamio.write_bam(bam, w.chrom, w.length, recs, other_refs=[("other", 5000)], write_bai=False)
    # The writer notes a record's end BEFORE it flushes its last block, a reader (and the helper) sees the end of the data as the start of the
    # EOF member.  A Z tag on the last record makes the records fill their last member exactly: then the writer flushes first and both agree.
    stream = ref.vcfio.bgzf_read(bam)
    fill = -(len(stream) - ref.header_len(stream)[0]) % 0xff00
    recs[-1] = dict(recs[-1], tags=dict(recs[-1].get("tags", {}), ZP="x" * ((fill - 4) % 0xff00)))
    bamio.write_bam(bam, w.chrom, w.length, recs, other_refs=[("other", 5000)], write_csi=True)
    stream, refs, recs = ref.records(bam)
    assert len(recs) > 200 and any(r["flag"] & 4 for r in recs)
    return bam, refs, recs


def test_linear_index_equals_the_writers(world_bam):
    bam, refs, recs = world_bam
    ix = ref.build(refs, recs, unmapped_placed=False)                    # (the writer leaves placed unmapped records out)
    theirs = ref.parse_bai(open(bam + ".bai", "rb").read())
    assert [ref.linear_filled(d["lin"]) for d in ix["refs"]] == [d["lin"] for d in theirs["refs"]]
    assert len(theirs["refs"][0]["lin"]) == 2 and theirs["refs"][1]["lin"] == []


def test_csi_equals_the_writers(world_bam):
    bam, refs, recs = world_bam
    ix = ref.build(refs, recs, unmapped_placed=False)
    assert ref.csi_bytes(ix, pseudo_bin=False) == gzip.decompress(open(bam + ".csi", "rb").read())


def test_region_query_on_the_spec_fixture():
    ix = ref.check_queries(os.path.join(G, "spec.bam"), os.path.join(G, "spec.bam.bai"))
    assert ix["n_no_coor"] == 3 and sum(len(d["bins"]) for d in ix["refs"]) > 3
    # and the helper's own index of that file: the same bins and chunks, the same pseudo-bins, the fixture's linear index where it has an entry
    stream, refs, recs = ref.records(os.path.join(G, "spec.bam"))
    mine = ref.build(refs, recs)
    for a, b in zip(mine["refs"], ix["refs"]):
        assert a["bins"] == b["bins"] and a["meta"] == b["meta"]
        assert all(v == 0 or v == a["lin"][w] for w, v in enumerate(b["lin"])) and len(b["lin"]) == (max(a["lin"]) + 1 if a["lin"] else 0)
    assert mine["n_no_coor"] == 3


def test_region_query_on_the_helpers_own_files(world_bam, tmp_path):
    """the query over what bai_bytes / csi_bytes serialise, placed unmapped records included"""
    bam, refs, recs = world_bam
    ix = ref.build(refs, recs)
    p = str(tmp_path / "w.bam")
    os.symlink(bam, p)
    open(p + ".bai", "wb").write(ref.bai_bytes(ix))
    open(p + ".csi", "wb").write(gzip.compress(ref.csi_bytes(ix)))
    for ext in (".bai", ".csi"):
        got = ref.check_queries(p, p + ext)
        assert got["refs"][0]["meta"] == ix["refs"][0]["meta"] and got["n_no_coor"] == 0


def test_library_assembly_equals_the_helper(world_bam):
    """bam_index.index_bytes (numpy, from per-record arrays as the device makes them) == the brute-force serialisation"""
    from nanocaller_amd.bam_index import index_bytes
    bam, refs, recs = world_bam
    recs = recs + [dict(off=0, refid=-1, pos=-1, flag=4, beg=0, end=1, vbeg=recs[-1]["vend"], vend=recs[-1]["vend"] + 40)]
    col = lambda k: np.array([r[k] for r in recs])   # noqa: E731
    for depth in (5, 6):
        bins = np.array([ref.reg2bin(r["beg"], r["end"], 14, depth) for r in recs])
        ix = ref.build(refs, recs, depth=depth)
        args = (len(refs), col("refid"), col("beg"), col("end"), (col("flag") & 4) != 0, bins, col("vbeg").astype(np.uint64), col("vend").astype(np.uint64))
        assert index_bytes("csi", *args, 14, depth) == ref.csi_bytes(ix)
        if depth == 5:
            assert index_bytes("bai", *args) == ref.bai_bytes(ix)
    assert ix["n_no_coor"] == 1

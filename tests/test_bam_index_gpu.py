"""GPU: indexing an unindexed BAM on the device (csrc/nc_bamindex.hip, nanocaller_amd/bam_index.py, device_bam.build_index).

The record offsets the device finds without chain starts are the serial chain's, entry for entry, on files whose records lie anywhere relative to
the BGZF members, are longer than a member, carry bytes that look like records, or reach the serial fallback; the .bai / .csi written from them
are the brute-force index of tests/bam_index_ref.py byte for byte and answer the region query of SAMv1 5.3 exactly; the device ingest makes the
same pack from them as from the writer's own index; corrupt and unsorted files come back as a status; the callers take the device route on an
unindexed file when asked, and only then."""
import gzip
import os
import queue
import shutil
import struct

import numpy as np
import pytest

from nanocaller_amd import _lib
from tests import bam_index_ref as ref
from tests import bamio

pytestmark = pytest.mark.gpu
ST_BLOCK_SIZE, ST_TRUNCATED, ST_UNSORTED = 2, 8, 32


def _reblock(src, dst, block=0xff00, per_record=False, stream=None):
    """the same inflated stream in members of `block` bytes, or (per_record) flushed behind the header and behind every record, as htslib writes"""
    stream = ref.vcfio.bgzf_read(src) if stream is None else stream
    w = bamio.BgzfWriter(dst, block=block)
    if per_record:
        p = ref.header_len(stream)[0]
        w.write(stream[:p])
        w.flush()
        while p < len(stream):
            n = 4 + struct.unpack_from("<i", stream, p)[0]
            w.write(stream[p:p + n])
            w.flush()
            p += n
    else:
        w.write(stream)
    w.close()
    return dst


def _small(i, pos0, tid=0, n=40):
    return dict(name="s%d" % i, flag=0, pos0=pos0, cigar=[("M", n)], seq="ACGT" * (n // 4), tid=tid)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (BAM without index, piece_bytes or None)"""
    d = tmp_path_factory.mktemp("bamidx")
    p = lambda n: str(d / (n + ".bam"))   # noqa: E731
    rng = np.random.default_rng(11)
    w = bamio.make_bam_world()
    recs = bamio.world_to_records(w, np.random.default_rng(2))
    out = {"world": w, "fa": str(d / "ref.fa"), "recs": recs, "dir": d}
    bamio.write_fasta(out["fa"], w.chrom, w.ref)
    bamio.write_bam(p("a"), w.chrom, w.length, recs, write_bai=False)                                   # a. members of 0xff00: records straddle them
    out["a"] = (p("a"), None)
    out["b512"] = (_reblock(p("a"), p("b512"), 512), None)                                              # b. members far shorter than a record
    out["b4096"] = (_reblock(p("a"), p("b4096"), 4096), None)
    out["c"] = (_reblock(p("a"), p("c"), per_record=True), None)                                        # c. members aligned with records
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, 70_000))                                        # d. a record longer than 64 KiB
    long_recs = [_small(0, 50), dict(name="long", flag=0, pos0=100, cigar=[("M", 70_000)], seq=seq, qual=bytes(rng.integers(0, 94, 70_000, dtype=np.uint8))),
                 _small(1, 200), _small(2, 90_000)]
    bamio.write_bam(p("d"), "c0", 100_000, long_recs, write_bai=False)
    out["d"] = (p("d"), None)
    bamio.write_bam(p("tmp"), "c0", 100_000, [_small(7, 1000), _small(8, 1010), _small(9, 1020)], write_bai=False)   # e. the decoy
    s = ref.vcfio.bgzf_read(p("tmp"))
    three = s[ref.header_len(s)[0]:]
    three += b"\0" * (-len(three) % 4)
    decoy = dict(_small(3, 120, n=400), tags={"ZD": list(struct.unpack("<%dI" % (len(three) // 4), three))})
    bamio.write_bam(p("e"), "c0", 100_000, [_small(0, 50), decoy, _small(1, 200), _small(2, 300)], write_bai=False)
    out["e"] = (p("e"), None)
    unplaced = [dict(name="u%d" % i, flag=4, pos0=-1, cigar=[], seq="ACGTACGTAC", tid=-1) for i in range(3)]      # f. an empty contig, unplaced records
    f_recs = [_small(i, 100 + 700 * i) for i in range(30)] + [_small(100 + i, 50 + 900 * i, tid=2) for i in range(20)] + unplaced
    bamio.write_bam(p("f"), "c0", 40_000, f_recs, other_refs=[("c1", 5000), ("c2", 40_000)], write_bai=False)
    out["f"] = (p("f"), None)
    bamio.write_bam(p("g"), w.chrom, w.length, recs[:120], other_refs=[("sq%04d" % i, 1000 + i) for i in range(3000)], write_bai=False)   # g. a long header
    out["g"] = (p("g"), None)
    bamio.write_bam(p("h"), "c0", 1000, [], write_bai=False)                                            # h. no records
    out["h"] = (p("h"), None)
    out["i"] = (p("a"), 30_000)                                                                         # i. pieces that end inside records
    out["i512"] = (out["b512"][0], 3_000)
    out["g_pieces"] = (p("g"), 20_000)                                                                  # (the header alone spans pieces)
    beyond = recs + [dict(_small(5, w.length + 100), name="beyond")]                                    # the fallback: a pos behind its reference's end
    bamio.write_bam(p("fallback"), w.chrom, w.length, beyond, write_bai=False)
    out["fallback"] = (p("fallback"), None)
    return out


CASES = ["a", "b512", "b4096", "c", "d", "e", "f", "g", "h", "i", "i512", "g_pieces", "fallback"]


@pytest.mark.parametrize("case", CASES)
def test_record_offsets_and_index(files, case):
    from nanocaller_amd import bam_index, device_bam
    src, piece = files[case]
    bam = str(files["dir"] / ("ix_%s.bam" % case))
    shutil.copyfile(src, bam)
    stream, refs, offs = ref.serial_chain(bam)
    got = bam_index.scan_records(bam, 0, piece, keep_offsets=True)
    assert got["offset"].tolist() == offs                                # the serial chain, entry for entry
    st = dict(bam_index.LAST_INDEX)
    assert st["records"] == len(offs) and (st["serial_pieces"] >= 1) == (case == "fallback"), st
    if piece:
        assert st["pieces"] > 3
    if case == "e":
        assert st["candidates"] >= len(offs) + 3                         # the decoy's records passed the predicate and were not taken
    if case == "d":
        assert max(np.diff(offs + [len(stream)])) > 65536
    if case == "g":
        assert offs[0] > 0xff00
    stream, refs, recs = ref.records(bam)
    ix = ref.build(refs, recs)
    tids = [0, 1, 2, len(refs) - 1] if len(refs) > 3 else None
    bai = device_bam.build_index(bam, piece_bytes=piece)
    assert bai == bam + ".bai" and not [f for f in os.listdir(os.path.dirname(bam)) if ".tmp" in f]
    mine = ref.parse_bai(open(bai, "rb").read())
    assert [d["lin"] for d in mine["refs"]] == [ref.linear_filled(d["lin"]) for d in ix["refs"]]
    assert [d["meta"] for d in mine["refs"]] == [d["meta"] for d in ix["refs"]] and mine["n_no_coor"] == ix["n_no_coor"]
    assert open(bai, "rb").read() == ref.bai_bytes(ix)
    ref.check_queries(bam, bai, seed=3, tids=tids)
    os.unlink(bai)
    csi = device_bam.build_index(bam, fmt="csi", piece_bytes=piece)
    assert csi == bam + ".csi" and gzip.decompress(open(csi, "rb").read()) == ref.csi_bytes(ix)
    got = ref.check_queries(bam, csi, seed=4, tids=tids)
    assert [d["meta"] for d in got["refs"]] == [d["meta"] for d in ix["refs"]] and got["n_no_coor"] == ix["n_no_coor"]
    if case == "f":
        assert ix["n_no_coor"] == 3 and ix["refs"][1]["meta"] is None and ix["refs"][2]["meta"][2] == 20


def _pack_arrays(bam, fa, chrom):
    import torch
    from nanocaller_amd import device_bam
    from nanocaller_amd.bam import read_fasta
    device_bam.release()
    db = device_bam.DeviceBam(bam, 0).load()
    dp = db.pack(db.prepare(chrom, read_fasta(fa, chrom)), indel=True)
    torch.cuda.synchronize()
    out = [dp.codes, dp.tile_off, dp.tile_ent.view(torch.uint8), dp.ref_code, dp.events["ev_pos"], dp.events["ev_len"], dp.indel["ins_bases"],
           dp.indel["tail_bases"]]
    out = [t.cpu().numpy().copy() for t in out] + [db.rec_off.copy()]
    device_bam.release()
    return out


@pytest.mark.parametrize("fmt", ["bai", "csi"])
def test_the_ingest_makes_the_same_pack_from_the_built_index(files, fmt):
    from nanocaller_amd import device_bam
    w, d = files["world"], files["dir"]
    theirs, mine = str(d / ("theirs_%s.bam" % fmt)), str(d / ("mine_%s.bam" % fmt))
    bamio.write_bam(theirs, w.chrom, w.length, files["recs"], write_bai=fmt == "bai", write_csi=fmt == "csi")
    shutil.copyfile(theirs, mine)
    assert device_bam.build_index(mine, fmt=fmt) == mine + "." + fmt
    a, b = _pack_arrays(theirs, files["fa"], w.chrom), _pack_arrays(mine, files["fa"], w.chrom)
    assert len(a[-1]) > 200
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------- refusals: a status, never a fault
def _rewrite(files, name, stream):
    return _reblock(None, str(files["dir"] / (name + ".bam")), stream=stream)


def _refused(bam, bit, piece=None):
    from nanocaller_amd import device_bam
    with pytest.raises(_lib.NanoCallerHipError) as e:
        device_bam.build_index(bam, piece_bytes=piece)
    assert e.value.status & bit, e.value
    assert not os.path.exists(bam + ".bai")
    return str(e.value)


@pytest.mark.parametrize("piece", [None, 30_000])
def test_unsorted_files_are_refused(files, piece):
    w, recs, d = files["world"], list(files["recs"]), files["dir"]
    k = next(k for k in range(150, len(recs) - 1) if recs[k]["pos0"] < recs[k + 1]["pos0"])
    recs[k], recs[k + 1] = recs[k + 1], recs[k]                          # positions swapped (across a piece boundary or not: the sort state travels)
    bam = str(d / ("unsorted_pos_%s.bam" % piece))
    bamio.write_bam(bam, w.chrom, w.length, recs, write_bai=False)
    assert "not coordinate-sorted" in _refused(bam, ST_UNSORTED, piece)
    bam = str(d / ("unsorted_contig_%s.bam" % piece))                    # contig order swapped
    bamio.write_bam(bam, "c0", 40_000, [_small(i, 100 * i, tid=1) for i in range(400)] + [_small(900 + i, 100 * i) for i in range(400)],
                    other_refs=[("c1", 40_000)], write_bai=False)
    _refused(bam, ST_UNSORTED, piece)
    bam = str(d / ("unsorted_unplaced_%s.bam" % piece))                  # a placed record behind an unplaced one
    bamio.write_bam(bam, "c0", 40_000, [_small(0, 10), dict(name="u", flag=4, pos0=-1, cigar=[], seq="ACGT", tid=-1), _small(1, 20)], write_bai=False)
    _refused(bam, ST_UNSORTED, piece)


def test_corrupt_streams_are_refused(files):
    import torch
    from nanocaller_amd import bam_index
    from nanocaller_amd.engine import get_engine
    stream, refs, offs = ref.serial_chain(files["a"][0])
    k = len(offs) // 2
    bad = bytearray(stream)
    bad[offs[k]:offs[k] + 4] = struct.pack("<i", 8)                      # a block_size of 8
    for piece in (None, 30_000):
        _refused(_rewrite(files, "bs8_%s" % piece, bytes(bad)), ST_BLOCK_SIZE, piece)
        _refused(_rewrite(files, "cut_%s" % piece, stream[:offs[-1] + 20]), ST_TRUNCATED, piece)   # the stream ends inside the last record
    # the kernels themselves, on the stream in HBM: from a record in the middle on; from an offset that is no record start
    eng = get_engine(0)
    eng.use_torch_stream()
    d_buf = torch.zeros(len(stream) + 64, dtype=torch.uint8, device=eng.device)
    d_buf[:len(stream)] = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(eng.device)
    d_len = torch.tensor([ln for _, ln in refs], dtype=torch.int32, device=eng.device)
    stats = {}
    out, n, carry, st = bam_index.chain_piece(eng, d_buf, len(stream), offs[k], len(refs), d_len, last=True, stats=stats)
    assert st == 0 and carry == len(stream) and out[:n].cpu().numpy().tolist() == offs[k:] and stats.get("serial_pieces", 0) == 0
    j = next(j for j in range(len(offs) - 1) if offs[j + 1] - offs[j] < 8192)          # (its block_size read one byte late is below 32)
    out, n, carry, st = bam_index.chain_piece(eng, d_buf, len(stream), offs[j] + 1, len(refs), d_len, last=True)
    assert st != 0
    # a piece cut inside a record: the carry is that record's start, nothing is read behind the cut
    cut = offs[k] + 30
    out, n, carry, st = bam_index.chain_piece(eng, d_buf, cut, offs[0], len(refs), d_len, last=False)
    assert st == 0 and carry == offs[k] and out[:n].cpu().numpy().tolist() == offs[:k]
    out, n, carry, st = bam_index.chain_piece(eng, d_buf, cut, offs[0], len(refs), d_len, last=True)
    assert st == ST_TRUNCATED


# ------------------------------------------------------------------------------------------------- end to end: the opt-in of the callers
def _snp_run(bam, fa, w, d, **extra):
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp, snpCaller
    gsp.release_contig()
    device_bam.release()
    del gsp.DECODES[:]
    os.makedirs(d)
    chunks = [dict(chrom=w.chrom, start=s, end=min(w.length, s + 15_000), ploidy="diploid") for s in range(1, w.length, 15_000)]
    params = dict(chunks_list=chunks, regions_list=[(w.chrom, 1, w.length, "diploid")], sam_path=bam, fasta_path=fa, mincov=4, maxcov=160,
                  min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=2, vcf_path=d, prefix="t", sample="S",
                  seq="ont", supplementary=False, exclude_bed=None, suppress_progress=True, disable_coverage_normalization=False,
                  intermediate_snp_files_dir=d, **extra)
    q = queue.Queue()
    for c in chunks:
        q.put(c)
    out = []
    snpCaller.caller(params, q, queue.Queue(), out)
    return open(out[0], "rb").read(), bool(gsp.DECODES)


def _has_index(bam):
    return os.path.exists(bam + ".bai") or os.path.exists(bam + ".csi")


def test_snp_caller_indexes_an_unindexed_bam_when_asked(files, tmp_path, monkeypatch):
    monkeypatch.delenv("NC_BUILD_INDEX", raising=False)
    monkeypatch.delenv("NC_DEVICE_INGEST", raising=False)
    w, fa = files["world"], files["fa"]
    indexed, bare = str(tmp_path / "indexed.bam"), str(tmp_path / "bare.bam")
    bamio.write_bam(indexed, w.chrom, w.length, files["recs"])
    shutil.copyfile(indexed, bare)
    want, host = _snp_run(indexed, fa, w, str(tmp_path / "o1"))
    assert not host and want.count(b"\n") > 20
    # without the opt-in: the host route, and no file appears
    got, host = _snp_run(bare, fa, w, str(tmp_path / "o2"))
    assert host and not _has_index(bare)
    monkeypatch.setenv("NC_DEVICE_INGEST", "0")
    today, host = _snp_run(indexed, fa, w, str(tmp_path / "o3"))
    monkeypatch.delenv("NC_DEVICE_INGEST")
    assert host and got == today
    got, host = _snp_run(bare, fa, w, str(tmp_path / "o4"), build_index=False)
    assert host and not _has_index(bare)
    # with it: the index is built once and the device route gives the indexed file's output byte for byte
    got, host = _snp_run(bare, fa, w, str(tmp_path / "o5"), build_index=True)
    assert not host and os.path.exists(bare + ".bai") and got == want
    stamp = os.stat(bare + ".bai").st_mtime_ns
    got, host = _snp_run(bare, fa, w, str(tmp_path / "o6"), build_index=True)
    assert not host and got == want and os.stat(bare + ".bai").st_mtime_ns == stamp


def test_an_index_that_cannot_be_written_is_an_error(files, tmp_path):
    from nanocaller_amd import device_bam
    bam = str(tmp_path / "x.bam")
    shutil.copyfile(files["a"][0], bam)
    os.mkdir("%s.bai.tmp%d" % (bam, os.getpid()))                        # a directory where the index's temporary file would go
    with pytest.raises(_lib.NanoCallerHipError, match="cannot be written beside it"):
        device_bam.ensure_index(bam, dict(build_index=True))
    assert not _has_index(bam)
    assert device_bam.ensure_index(bam, dict(build_index=False)) is None and device_bam.ensure_index(bam, {}) is None


def _indel_run(bam, fa, w, d, **extra):
    from nanocaller_amd import device_bam, generate_indel_pileups as gip, indelCaller
    from nanocaller_amd.generate_SNP_pileups import release_contig
    release_contig()
    device_bam.release()
    gip._DEV_INGEST.clear()
    os.makedirs(d)
    params = dict(seq="ont", fasta_path=fa, win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6, supplementary=False,
                  exclude_bed=None, impute_indel_phase=False, indel_model="ONT-HG002", intermediate_indel_files_dir=d, prefix="t", **extra)
    jobs = queue.Queue()
    for s in range(1, w.length, 10_000):
        jobs.put(("indel", dict(chrom=w.chrom, start=s, end=min(w.length, s + 10_000), sam_path=bam, ploidy="diploid")))
    return open(indelCaller.indel_run(params, {}, jobs, queue.Queue(), [], aligner="device")).read()


def test_indel_caller_indexes_an_unindexed_bam_when_asked(files, tmp_path, monkeypatch):
    from nanocaller_amd import device_bam
    monkeypatch.delenv("NC_BUILD_INDEX", raising=False)
    monkeypatch.delenv("NC_DEVICE_INGEST", raising=False)
    w, fa = files["world"], files["fa"]
    indexed, bare = str(tmp_path / "indexed.bam"), str(tmp_path / "bare.bam")
    bamio.write_bam(indexed, w.chrom, w.length, files["recs"])
    shutil.copyfile(indexed, bare)
    opened = []
    real = device_bam.open_device_bam
    monkeypatch.setattr(device_bam, "open_device_bam", lambda *a, **k: (opened.append(a[0]), real(*a, **k))[1])
    from nanocaller_amd import generate_indel_pileups as gip
    want = _indel_run(indexed, fa, w, str(tmp_path / "o1"))
    assert want.count("\n") > 10 and set(opened) == {indexed} and [k[0] for k in gip._DEV_INGEST] == [indexed]
    _indel_run(bare, fa, w, str(tmp_path / "o2"))                         # without the opt-in: the host decode, and no file appears
    assert not _has_index(bare) and not gip._DEV_INGEST
    got = _indel_run(bare, fa, w, str(tmp_path / "o3"), build_index=True)
    assert got == want and os.path.exists(bare + ".bai") and [k[0] for k in gip._DEV_INGEST] == [bare]


def test_weighted_phasing_on_an_unindexed_bam(tmp_path, monkeypatch):
    """phase_contig(weighted=True) reads qualities from the device ingest's record stream: without index it raises as before, with
    NC_BUILD_INDEX=1 it indexes the file and gives the indexed file's result"""
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import kept_reads, phase_contig
    from phase_gt_ref import world_calls
    from phase_realign_ref import make_realign_world
    monkeypatch.delenv("NC_BUILD_INDEX", raising=False)
    monkeypatch.setenv("NC_DEVICE_INGEST", "1")
    w = make_realign_world(93, length=30_000, depth=12.0)
    rng = np.random.default_rng(93)
    recs = bamio.world_to_records(w, None)
    for r in recs:
        r["tags"] = {}
        r["qual"] = bytes(rng.integers(0, 94, len(r["seq"]), dtype=np.uint8))
    indexed, bare, fa = str(tmp_path / "indexed.bam"), str(tmp_path / "bare.bam"), str(tmp_path / "r.fa")
    bamio.write_bam(indexed, w.chrom, w.length, recs)
    shutil.copyfile(indexed, bare)
    bamio.write_fasta(fa, w.chrom, w.ref)
    vcf = world_calls(w, kept_reads(w, False)[0], third_every=7)
    release_contig()
    want = phase_contig(indexed, fa, w.chrom, vcf, 10, False, weighted=True)
    release_contig()
    with pytest.raises(_lib.NanoCallerHipError, match="device ingest"):
        phase_contig(bare, fa, w.chrom, vcf, 10, False, weighted=True)
    assert not _has_index(bare)
    monkeypatch.setenv("NC_BUILD_INDEX", "1")
    release_contig()
    got = phase_contig(bare, fa, w.chrom, vcf, 10, False, weighted=True)
    assert os.path.exists(bare + ".bai") and got.records == want.records and len(want.records) > 10
    assert np.array_equal(got.reads["hp"], want.reads["hp"]) and np.array_equal(got.reads["ps"], want.reads["ps"])
    release_contig()

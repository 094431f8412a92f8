"""GPU: alignments that share a read name on the device BAM ingest (device_bam.DeviceBam.prepare(by_name=True); csrc/nc_ingest_names.hip).  The
names are confirmed in HBM by nc_bam_name_groups; from there the pack is the host route's byte for byte (pack.name_groups / mate_table: bit 3 and
the name's strand in the tile entries, the featuriser's table), and the SNP entry points answer what the oracle keyed by name answers."""
import copy
import ctypes as C
import queue

import numpy as np
import pytest

from nanocaller_amd import _lib
from tests import bamio

pytestmark = pytest.mark.gpu


def _share_names(w, seed, n_groups=16, reach=6_000, primary=False, apart=False):
    """some alignments of `w` renamed to another alignment's name (overlapping it, or within `reach`; apart=True: only ones that do NOT overlap
    it) and flagged supplementary; primary=True: they stay primary records (paired-end mates: kept by the default filter too); every third
    name gets three records"""
    rng = np.random.default_rng(seed)
    w = copy.copy(w)
    names, flag = list(w.names), w.read_flag.copy()
    s, e = w.read_start, w.read_end
    plain = [r for r in range(w.n_reads) if int(flag[r]) in (0, 16)]
    used, made = set(), 0
    for r1 in rng.permutation(plain).tolist():
        if made >= n_groups:
            break
        if r1 in used:
            continue
        cand = [r for r in plain if r != r1 and r not in used and int(s[r]) < int(e[r1]) + reach and int(s[r1]) < int(e[r]) + reach
                and not (apart and int(s[r]) < int(e[r1]) and int(s[r1]) < int(e[r]))]
        if not cand:
            continue
        pick = [cand[int(rng.integers(0, len(cand)))]]
        if made % 3 == 2 and len(cand) > 1:
            pick.append([c for c in cand if c != pick[0]][0])
        used.add(r1)
        for r2 in pick:
            used.add(r2)
            names[r2] = names[r1]
            flag[r2] = (0 if primary else 0x800) | (16 if rng.random() < 0.5 else 0)
        made += 1
    w.names, w.read_flag = names, flag
    return w


def _first_occurrence(names):
    """the grouping nc_bam_name_groups must return: per entry the index of the first entry with its name, -1 for a name that occurs once"""
    first, gid = {}, [-1] * len(names)
    for i, nm in enumerate(names):
        q = first.setdefault(nm, i)
        if q != i:
            gid[q] = gid[i] = q
    return gid


def _write(tmp_path, w, tag="m", seed=2):
    bam, fa = str(tmp_path / (tag + ".bam")), str(tmp_path / (tag + ".fa"))
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, np.random.default_rng(seed)))
    bamio.write_fasta(fa, w.chrom, w.ref)
    return bam, fa


def _name_groups(db, recs, hashes, rec_off=None, raw_len=None):
    """nc_bam_name_groups on records `recs` of a loaded DeviceBam with the given hashes -> (status code, gid)"""
    import torch
    dev = db.eng.device
    off = np.ascontiguousarray(db.rec_off[recs] if rec_off is None else rec_off, np.int64)
    d_off, d_hash = torch.from_numpy(off).to(dev), torch.from_numpy(np.ascontiguousarray(hashes, np.uint64).view(np.int64)).to(dev)
    d_gid, d_status = torch.full((len(off),), -7, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rc = _lib.lib().nc_bam_name_groups(db.eng.ctx, vp(db.raw), db.raw_len if raw_len is None else raw_len, len(off), vp(d_off), vp(d_hash), vp(d_gid), vp(d_status))
    return rc, d_gid.cpu().numpy().tolist(), int(d_status.item())


def test_kernel_groups_by_the_names_themselves(tmp_path):
    from nanocaller_amd import device_bam
    from nanocaller_amd.device_bam import M_HASH_HI, M_HASH_LO, DeviceBam
    ref = "ACGT" * 1500
    long_a = "L" * 254
    long_b = "L" * 200 + "l" + "L" * 53                                 # 254 bytes as well, another name
    names = ["ov", "tri", "far", "lastA", "ov", "pre", "tri", "x", long_a, "lastB", "prefix", "mid-0123456789abcdeX-tail", "tri", long_b,
             "read/0123456789abcdef", "mid-0123456789abcdeY-tail", "alone", "read/0123456789abcdef", long_a, "y", "read/0123456789abcdeg", "far"]
    # (records of different sizes: the names start on every byte of a dword; "ov" overlaps itself, "far" does not)
    recs = [dict(name=nm, flag=16 * (k % 2), pos0=40 + 50 * k, cigar=[("M", 60 + k)], seq=ref[40 + 50 * k:100 + 51 * k], tags={}) for k, nm in enumerate(names)]
    recs[4]["pos0"], recs[4]["seq"] = 60, ref[60:60 + 64]
    recs.sort(key=lambda r: r["pos0"])
    names = [r["name"] for r in recs]
    bam = str(tmp_path / "n.bam")
    bamio.write_bam(bam, "chrT", len(ref), recs)
    db = DeviceBam(bam, 0).load()
    assert db.n_rec == len(names) and db.fetch_names(range(db.n_rec)) == names
    h = db.meta[M_HASH_LO].astype(np.uint32).astype(np.uint64) | (db.meta[M_HASH_HI].astype(np.uint32).astype(np.uint64) << np.uint64(32))
    # the true hashes: the records whose hash occurs more than once, sorted by (hash, file order)
    _, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
    cand = np.flatnonzero(cnt[inv] > 1)
    cand = cand[np.argsort(h[cand], kind="stable")]
    assert cand.size == 11                                                # ov 2, far 2, tri 3, the 254-byte name 2, read/...f 2
    rc, gid, st = _name_groups(db, cand, h[cand])
    assert rc == _lib.NC_OK and st == 0
    assert gid == _first_occurrence([names[r] for r in cand]) and -1 not in gid
    # every hash forced equal: one run that holds every name -- the collision path
    every = np.arange(db.n_rec)
    rc, gid, st = _name_groups(db, every, np.full(db.n_rec, 12345, np.uint64))
    assert rc == _lib.NC_OK and st == 0
    assert gid == _first_occurrence(names)
    assert sorted(names[i] for i, g in enumerate(gid) if g == -1) == sorted(["lastA", "lastB", "pre", "prefix", "x", "y", "alone", long_b, "mid-0123456789abcdeX-tail",
                                                                             "mid-0123456789abcdeY-tail", "read/0123456789abcdeg"])
    # a run longer than one wave (the records four times over): members behind the first 64 find the leaders of the earlier ones
    four = np.tile(every, 4)
    rc, gid, st = _name_groups(db, four, np.full(four.size, 99, np.uint64))
    assert rc == _lib.NC_OK and four.size > 64
    assert gid == _first_occurrence([names[r] for r in four]) and -1 not in gid
    # two runs side by side, the second one cut by the end of the candidates
    rc, gid, st = _name_groups(db, every, np.r_[np.full(9, 5, np.uint64), np.full(db.n_rec - 9, 6, np.uint64)])
    assert rc == _lib.NC_OK and gid == _first_occurrence(names[:9]) + [g + 9 if g >= 0 else -1 for g in _first_occurrence(names[9:])]
    # a record offset that does not lie inside the stream: an error return through the status word, no fault
    for bad in (db.raw_len + 100, db.raw_len - 10, -4):
        off = db.rec_off[every].copy()
        off[7] = bad
        rc, _, st = _name_groups(db, every, np.full(db.n_rec, 1, np.uint64), rec_off=off)
        assert rc == _lib.NC_ERR_ARG and st != 0, bad
    rc, _, st = _name_groups(db, every, np.full(db.n_rec, 1, np.uint64), raw_len=int(db.rec_off[-1]) + 40)      # the last record's name ends behind the stream
    assert rc == _lib.NC_ERR_ARG and st != 0
    assert _lib.lib().nc_bam_name_groups(db.eng.ctx, None, 0, 0, None, None, None, None) == _lib.NC_OK          # no candidates: nothing to do
    device_bam.release()


def _host_pack(eng, bam, fa, chrom, supplementary):
    from nanocaller_amd.bam import read_bam
    from nanocaller_amd.wire import build_wire_from_world, upload_wire
    world = read_bam(bam, fa, chrom)
    return upload_wire(eng, build_wire_from_world(world, supplementary=supplementary)), world


def _assert_same_pack(got, want):
    import torch
    torch.cuda.synchronize()
    for f in ("tile_size", "tile_pos0", "n_tiles", "n_entries", "pos_lo", "pos_hi"):
        assert getattr(got, f) == getattr(want, f), f
    assert np.array_equal(got.tile_off.cpu().numpy(), want.tile_off.cpu().numpy())
    assert np.array_equal(got.tile_ent.cpu().numpy().view(np.uint8).reshape(-1), want.tile_ent.cpu().numpy().view(np.uint8).reshape(-1)[:got.tile_ent.numel()])
    assert np.array_equal(got.ref_code.cpu().numpy(), want.ref_code.cpu().numpy())
    assert np.array_equal(got.codes.cpu().numpy(), want.codes.cpu().numpy())
    assert (got.mates is None) == (want.mates is None)
    if want.mates is not None:
        assert np.array_equal(got.mates[0].cpu().numpy(), want.mates[0].cpu().numpy())
        assert np.array_equal(got.mates[1].cpu().numpy().reshape(-1, 4), want.mates[1].cpu().numpy().reshape(-1, 4))


@pytest.mark.parametrize("supplementary", [True, False])
def test_by_name_pack_is_the_host_routes_pack(tmp_path, supplementary):
    from nanocaller_amd import device_bam
    from nanocaller_amd.bam import read_fasta
    from nanocaller_amd.device_bam import DeviceBam
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.pack import pack_world
    w = _share_names(bamio.make_bam_world(seed=21, length=60_000, depth=14), seed=5, n_groups=16, primary=not supplementary)
    bam, fa = _write(tmp_path, w)
    eng = get_engine(0)
    want, world = _host_pack(eng, bam, fa, w.chrom, supplementary)
    db = DeviceBam(bam, 0).load()
    prep = db.prepare(w.chrom, read_fasta(fa, w.chrom), supplementary=supplementary, by_name=True)
    got = db.pack(prep)
    _assert_same_pack(got, want)
    # ... and pack_reads' on the host decode: the flagged entries carry bit 3 and the NAME's strand
    hp = pack_world(world, supplementary=supplementary)
    key, rec = hp.mates
    assert key.size >= 32 and np.array_equal(prep["mates"][0], key) and np.array_equal(prep["mates"][1], rec)
    ent = got.tile_ent.cpu().numpy().view(_lib.TILE_ENTRY_DTYPE)
    assert np.array_equal(ent["base_flag"], hp.tile_ent["base_flag"]) and int(((ent["base_flag"] & 8) != 0).sum()) >= key.size
    # without by_name nothing changed: the same file is refused with the words the indel route depends on
    with pytest.raises(_lib.NanoCallerHipError) as e:
        db.prepare(w.chrom, read_fasta(fa, w.chrom), supplementary=supplementary)
    assert e.value.status == _lib.NC_ERR_UNSUPPORTED and "same read name" in str(e.value) and "NC_DEVICE_INGEST=0" in str(e.value)
    device_bam.release()


def test_a_member_the_depth_cap_drops_leaves_its_names_ring(tmp_path):
    from nanocaller_amd import device_bam
    from nanocaller_amd.bam import read_fasta
    from nanocaller_amd.device_bam import DeviceBam
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.pack import PILEUP_MAX_DEPTH
    rng = np.random.default_rng(3)
    ref = "".join("ACGT"[i] for i in rng.integers(0, 4, 6_000))
    rec = lambda name, p0, ln, flag=0: dict(name=name, flag=flag, pos0=p0, cigar=[("M", ln)], seq=ref[p0:p0 + ln], tags={})   # noqa: E731
    recs = [rec("s", 100, 900)]                                          # alive at column 501 ...
    recs += [rec("d%d" % k, 500, 30, 16 * (k & 1)) for k in range(PILEUP_MAX_DEPTH + 5)]
    recs.append(rec("s", 500, 40, 16))                                   # ... where its second record arrives behind more than max_depth others
    recs += [rec("t", 2_000, 300), rec("u", 2_050, 300, 16), rec("t", 2_100, 300, 16), rec("t", 2_600, 200)]
    bam, fa = str(tmp_path / "d.bam"), str(tmp_path / "d.fa")
    bamio.write_bam(bam, "chrD", len(ref), recs)
    bamio.write_fasta(fa, "chrD", ref)
    eng = get_engine(0)
    want, world = _host_pack(eng, bam, fa, "chrD", False)
    db = DeviceBam(bam, 0).load()
    prep = db.prepare("chrD", read_fasta(fa, "chrD"), by_name=True)
    second = PILEUP_MAX_DEPTH + 6
    assert prep["read_start"][second] == 501 and prep["keep"][second] == 0 and prep["keep"][0] == 1       # dropped by the cap; the survivor is kept
    got = db.pack(prep)
    _assert_same_pack(got, want)
    key, mrec = prep["mates"]
    assert key.size == 3 and mrec[:, 0].tolist() == [2_001, 2_101, 2_601]                                   # "t" alone: "s" is one alignment again
    ent = got.tile_ent.cpu().numpy().view(_lib.TILE_ENTRY_DTYPE)
    assert not (ent["base_flag"][ent["start"] == 101] & 8).any() and (ent["base_flag"][ent["start"] == 2_001] & 8).all()
    device_bam.release()


def _dct(bam, fa, supplementary, **kw):
    return dict(sam_path=bam, fasta_path=fa, exclude_bed=None, threshold=[0.3, 0.7], supplementary=supplementary, mincov=4, maxcov=160, min_allele_freq=0.15,
                min_nbr_sites=1, seq="ont", **kw)


def _same_tuple(out, exp):
    assert len(out[0]) == len(exp[0]) > 50
    assert np.array_equal(out[0], exp[0]) and np.array_equal(np.asarray(out[2]), np.asarray(exp[2]))
    assert np.array_equal(out[6], exp[6]) and np.array_equal(out[7], exp[7]) and float(out[5]) == float(exp[5])


def test_snp_entry_points_take_the_device_route_and_equal_the_oracle_by_name(tmp_path):
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp, snpCaller
    from nanocaller_amd.engine import DevicePack
    from oracle import oracle
    w = _share_names(bamio.make_bam_world(seed=21, length=60_000, depth=14), seed=5, n_groups=16)
    bam, fa = _write(tmp_path, w)
    dct = _dct(bam, fa, True, device_ingest=True)
    region = dict(chrom=w.chrom, start=5_000, end=55_000, ploidy="diploid")
    gsp.release_contig()
    device_bam.release()
    device_bam.LAST_LOAD.clear()
    del gsp.DECODES[:]
    out = gsp.get_snp_testing_candidates(dct, region)
    exp = oracle.get_snp_testing_candidates(w, dct, region)
    _same_tuple(out, exp)
    res = snpCaller.call_chunks(dict(dct, snp_model="ONT-HG002", disable_coverage_normalization=False), [region])
    assert res["n"] == len(exp[0]) and np.array_equal(res["pos"], exp[0])
    assert np.array_equal(res["fwd_dp"], np.asarray(exp[6], res["fwd_dp"].dtype)) and np.array_equal(res["rev_dp"], np.asarray(exp[7], res["rev_dp"].dtype))
    # the contig came through the device ingest: the file was loaded into HBM, nothing was decoded on the host, the cached pack has no World
    assert device_bam.LAST_LOAD.get("records", 0) >= w.n_reads and gsp.DECODES == []
    entry = [v for k, v in gsp._PACKS.d.items() if k[0] == bam]
    assert entry and all(isinstance(v[0], DevicePack) and v[0].mates is not None and v[1] is None for v in entry)
    plain = copy.copy(w)
    plain.names = None
    per_alignment = oracle.get_snp_testing_candidates(plain, dct, region)
    assert not np.array_equal(np.asarray(per_alignment[2]), np.asarray(exp[2]))          # (the test is about something)
    gsp.release_contig()
    device_bam.release()


def test_mates_that_do_not_overlap_give_one_answer_on_both_routes(tmp_path, monkeypatch):
    """ADVICE: with `supplementary` off the device route used to count only OVERLAPPING same-name pairs and let non-overlapping mates pass as
    independent reads, so one BAM gave different tensors with NC_DEVICE_INGEST=0 and without"""
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp
    from nanocaller_amd.bam import same_name_overlaps
    from oracle import oracle
    w = _share_names(bamio.make_bam_world(seed=23, length=60_000, depth=14), seed=9, n_groups=16, primary=True, apart=True)
    keep = (w.read_flag & 0xF04) == 0
    assert same_name_overlaps(w.names, w.read_start, w.read_end, keep) == 0 and len(set(w.names)) <= w.n_reads - 16
    bam, fa = _write(tmp_path, w)
    region = dict(chrom=w.chrom, start=5_000, end=55_000, ploidy="diploid")
    exp = oracle.get_snp_testing_candidates(w, _dct(bam, fa, False), region)
    plain = copy.copy(w)
    plain.names = None
    per_alignment = oracle.get_snp_testing_candidates(plain, _dct(bam, fa, False), region)
    assert not np.array_equal(np.asarray(per_alignment[2]), np.asarray(exp[2]))          # by name and per alignment differ on this world
    gsp.release_contig()
    device_bam.release()
    del gsp.DECODES[:]
    dev = gsp.get_snp_testing_candidates(_dct(bam, fa, False, device_ingest=True), region)
    assert gsp.DECODES == []
    gsp.release_contig()
    monkeypatch.setenv("NC_DEVICE_INGEST", "0")
    host = gsp.get_snp_testing_candidates(_dct(bam, fa, False), region)
    assert [d[:2] for d in gsp.DECODES] == [(bam, w.chrom)]
    _same_tuple(dev, exp)
    _same_tuple(host, exp)
    for a, b in zip(dev, host):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    gsp.release_contig()
    device_bam.release()


def test_a_name_on_two_contigs_is_two_names(tmp_path):
    from nanocaller_amd import device_bam
    from nanocaller_amd.device_bam import DeviceBam
    rng = np.random.default_rng(4)
    refs = ["".join("ACGT"[i] for i in rng.integers(0, 4, 3_000)) for _ in range(2)]
    rec = lambda tid, name, p0, ln=200, flag=0: dict(tid=tid, name=name, flag=flag, pos0=p0, cigar=[("M", ln)], seq=refs[tid][p0:p0 + ln], tags={})   # noqa: E731
    recs = [rec(0, "a%d" % k, 20 * k) for k in range(12)] + [rec(0, "both", 300), rec(0, "pair", 320), rec(0, "pair", 900, flag=16)]
    recs += [rec(1, "b%d" % k, 20 * k) for k in range(12)] + [rec(1, "both", 310, flag=16)]
    recs.sort(key=lambda r: (r["tid"], r["pos0"]))
    bam = str(tmp_path / "t.bam")
    bamio.write_bam(bam, "c0", 3_000, recs, other_refs=[("c1", 3_000)])
    db = DeviceBam(bam, 0).load()
    p0 = db.prepare("c0", refs[0], by_name=True)
    assert p0["mates"] is not None and p0["mates"][1][:, 0].tolist() == [321, 901] and p0["mates"][1][:, 2].tolist() == [1, 0]
    p1 = db.prepare("c1", refs[1], by_name=True)
    assert p1["mates"] is None and p1["n_kept"] == 13 and db.pack(p1).mates is None
    device_bam.release()


def test_the_caller_takes_split_reads_through_the_device_ingest(tmp_path, monkeypatch):
    """snpCaller.caller with dct['supplementary'] no longer gives the device route up for such a file: nothing is decoded on the host, and the
    worker file is the host route's byte for byte"""
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp, snpCaller
    w = _share_names(bamio.make_bam_world(seed=21, length=60_000, depth=14), seed=5, n_groups=16)
    bam, fa = _write(tmp_path, w)
    chunks = [dict(chrom=w.chrom, start=s, end=min(w.length, s + 30_000), ploidy="diploid") for s in range(1, w.length, 30_000)]
    outs = {}
    for tag, env in (("device", None), ("host", "0")):
        if env is None:
            monkeypatch.delenv("NC_DEVICE_INGEST", raising=False)
        else:
            monkeypatch.setenv("NC_DEVICE_INGEST", env)
        gsp.release_contig()
        device_bam.release()
        del gsp.DECODES[:]
        d = tmp_path / tag
        d.mkdir()
        params = dict(chunks_list=chunks, regions_list=[(w.chrom, 1, w.length, "diploid")], sam_path=bam, fasta_path=fa, mincov=4, maxcov=160,
                      min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=2, vcf_path=str(d), prefix="t",
                      sample="S", seq="ont", supplementary=True, exclude_bed=None, suppress_progress=True,
                      disable_coverage_normalization=False, intermediate_snp_files_dir=str(d))
        q = queue.Queue()
        for c in chunks:
            q.put(c)
        files = []
        snpCaller.caller(params, q, queue.Queue(), files)
        outs[tag] = open(files[0], "rb").read()
        assert (gsp.DECODES == []) == (tag == "device")
    assert outs["device"] == outs["host"] and outs["device"].count(b"\n") > 50
    gsp.release_contig()

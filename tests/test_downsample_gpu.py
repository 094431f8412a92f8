"""The uniform sample above maxcov on the device (nc_set_downsample; csrc/nc_sample.h) against the yardsticks of
tests/downsample_ref.py.  Every world, maxcov and seed used here is shown by tests/test_downsample_ref.py, on the host, to hold sites at which the
uniform sample is not the first maxcov reads; the comparisons below count such sites and ask for the same minimum.

SNP: the tensor of a site deeper than maxcov equals the oracle's on the sub-world of the sampled reads; fwd_dp / rev_dp are those of the full world;
site_depth is min(n, maxcov); sites of depth <= maxcov equal the plain form's bit for bit, in the same launch.
Indel: set s of an anchor whose set is deeper than maxcov equals x[0] of oracle.indel_site_ref on the records of the set's sample (haploid=True,
mincov=1, maxcov large, band=True), its allele likewise; the phase set is that of the unsampled pileup's first HP 1 read.  (`only HP 1 exceeds` can
only mean `of the two haplotype sets`: the `all` set holds both, so it exceeds maxcov whenever one of them does.)"""
import numpy as np
import pytest

import downsample_ref as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


_packs = {}


def _pack(eng, world, key):
    if key not in _packs:
        from nanocaller_amd.wire import build_wire_from_world, upload_wire
        _packs[key] = upload_wire(eng, build_wire_from_world(world))
    return _packs[key]


def _run(eng, world, key, listed, maxcov, downsample, int16=True, mincov=1, region=None):
    """scan with `listed` as the only candidates + featurise -> dict of host arrays"""
    import torch
    dpk = _pack(eng, world, key)
    lo, hi = region or (1, world.length - 1)
    sites = eng.snp_scan(dpk, [(lo, hi)], mincov=mincov, min_allele_freq=0.15, threshold=[0.3, 0.7], sites=np.asarray(listed), sites_only=True)
    eng.snp_featurize(dpk, sites, seq="ont", maxcov=maxcov, min_nbr_sites=1, int16=int16, downsample=downsample)
    torch.cuda.synchronize()
    assert sites.x.dtype == (torch.int16 if int16 else torch.float32)
    return dict(pos=np.asarray(sites.pos).copy(), x=sites.x.cpu().numpy(), fwd=sites.fwd_dp.cpu().numpy(), rev=sites.rev_dp.cpu().numpy(),
                depth=sites.depth.cpu().numpy(), valid=sites.valid.cpu().numpy(), ref=sites.ref_code.cpu().numpy())


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


_nbr = {}


def _check(world, key, got, plain, seed, maxcov, need_sharp, mincov=1):
    """every site of `got` (the sampled form) against its yardstick; -> the sharp sites seen"""
    if key not in _nbr:
        _nbr[key] = D.world_nbr(world, mincov)
    rc, nbr = _nbr[key]
    assert np.array_equal(got["pos"], plain["pos"]) and got["valid"].all()
    sharp = []
    for i, v in enumerate(got["pos"].tolist()):
        n = D.pileup(world, v).size
        if n <= maxcov:                                              # the same launch leaves these what the plain form makes them
            assert np.array_equal(got["x"][i], plain["x"][i]), v
        mat, fwd, rev, dep = D.snp_yardstick(world, rc, nbr, v, seed, maxcov)
        assert np.array_equal(got["x"][i].astype(np.float32), mat), "tensor of site %d (depth %d, maxcov %d) differs from the sampled sub-world's" % (v, n, maxcov)
        assert np.array_equal(got["fwd"][i], fwd) and np.array_equal(got["rev"][i], rev), v
        assert np.array_equal(got["fwd"][i], plain["fwd"][i]) and np.array_equal(got["rev"][i], plain["rev"][i])
        assert got["depth"][i] == dep == min(n, maxcov) and got["ref"][i] == plain["ref"][i]
        if D.sharp(seed, v, 0, n, maxcov):
            sharp.append(v)                                          # (a sharp sample may still count the same bases: the yardstick decides)
    assert len(sharp) >= need_sharp, (len(sharp), need_sharp)
    return sharp


# ---------------------------------------------------------------------------------------------------------------- the setter
def test_setter_and_refusals(eng):
    from nanocaller_amd import _lib
    L = eng.L
    assert L.nc_set_downsample(eng.ctx, 1, 812) == 0 and L.nc_set_downsample(eng.ctx, 0, 0) == 0
    for bad in (2, -1, 7):
        assert L.nc_set_downsample(eng.ctx, bad, 812) == _lib.NC_ERR_ARG
    with pytest.raises(ValueError):
        eng.set_downsample("sometimes")
    eng.set_downsample("uniform", 5)
    eng.set_downsample("first")
    # a shared-names table with the uniform sample is refused, never served by the first-maxcov cut; the state is cleared afterwards
    from util import load_snp_case
    from nanocaller_amd.wire import build_wire_from_world, upload_wire
    world, dct, region, _, _ = load_snp_case("ont_mates")
    dpk = upload_wire(eng, build_wire_from_world(world, supplementary=dct["supplementary"]))
    assert dpk.mates is not None
    sites = eng.snp_scan(dpk, [(region["start"], region["end"])], mincov=dct["mincov"], min_allele_freq=dct["min_allele_freq"], threshold=dct["threshold"])
    assert sites.n_sites > 0
    with pytest.raises(_lib.NanoCallerHipError) as ei:
        eng.snp_featurize(dpk, sites, seq=dct["seq"], maxcov=8, downsample=("uniform", 812))
    assert ei.value.status == _lib.NC_ERR_UNSUPPORTED and "share read names" in str(ei.value)
    eng.snp_featurize(dpk, sites, seq=dct["seq"], maxcov=8)                          # (cleared: the plain call runs)
    from nanocaller_amd import generate_SNP_pileups as gsp
    with pytest.raises(ValueError, match="share read names"):
        gsp.get_snp_testing_candidates(dict(dct, sam_path=world, fasta_path=None, downsample="uniform", maxcov=8), region)


# ---------------------------------------------------------------------------------------------------------------- SNP: the staircase
@pytest.mark.parametrize("maxcov,int16,pairs", [(m, True, True) for m in D.STAIR_MAXCOVS_PAIRS] + [(m, True, True) for m in D.STAIR_MAXCOVS_WALK] +
                         [(160, False, True), (160, True, False)])
def test_staircase_every_depth_around_maxcov(eng, monkeypatch, maxcov, int16, pairs):
    """maxcov <= 255 with int16 tensors: k_featurize_pairs; maxcov >= 256, float32 tensors or NC_FEAT_PAIRS=0: k_featurize"""
    if not pairs:
        monkeypatch.setenv("NC_FEAT_PAIRS", "0")
    w, seed = D.staircase_world(), D.stair_seed(maxcov)
    listed = D.stair_sites()
    plain = _run(eng, w, "stair", listed, maxcov, None, int16)
    first = _run(eng, w, "stair", listed, maxcov, ("first", seed), int16)
    assert _same(plain, first)                                       # mode 0: today's output, whole
    got = _run(eng, w, "stair", listed, maxcov, ("uniform", seed), int16)
    again = _run(eng, w, "stair", listed, maxcov, ("uniform", seed), int16)
    assert _same(got, again)                                         # two runs, bit for bit
    assert {D.stair_col(d) for d in (maxcov - 1, maxcov, maxcov + 1) if d >= 1} <= set(got["pos"].tolist())
    sharp = _check(w, "stair", got, plain, seed, maxcov, 20)
    assert D.stair_col(maxcov + 1) in sharp
    assert _same(plain, _run(eng, w, "stair", listed, maxcov, None, int16))           # nothing is left set


def test_another_seed_gives_other_sets(eng):
    w, maxcov = D.staircase_world(), 64
    listed = D.stair_sites()
    plain = _run(eng, w, "stair", listed, maxcov, None)
    a = _run(eng, w, "stair", listed, maxcov, ("uniform", 812))
    b = _run(eng, w, "stair", listed, maxcov, ("uniform", 4242))
    deep = np.array([D.pileup(w, int(v)).size > maxcov for v in a["pos"]])
    differ = (a["x"] != b["x"]).any(axis=(1, 2, 3))
    assert not differ[~deep].any() and differ[deep].sum() >= 0.9 * deep.sum()
    _check(w, "stair", b, plain, 4242, maxcov, 20)                    # the yardstick follows the seed


def test_sample_over_several_steps_and_tile_edges(eng):
    w = D.mixed_world()
    listed, edges = D.mixed_sites(w)
    plain = _run(eng, w, "mixed", listed, D.MIXED_MAXCOV, None, mincov=4)
    got = _run(eng, w, "mixed", listed, D.MIXED_MAXCOV, ("uniform", D.SEED), mincov=4)
    dpk = _packs["mixed"]
    assert (int(dpk.tile_pos0), int(dpk.tile_size)) == D.tile_grid(w)
    sharp = _check(w, "mixed", got, plain, D.SEED, D.MIXED_MAXCOV, 20, mincov=4)
    assert set(edges) <= set(sharp)


@pytest.mark.parametrize("name", ["ont", "deep"])
def test_golden_worlds_at_maxcov_8(eng, name):
    w, listed = D.golden_sites(name)
    lo, hi = D.GOLDEN_REGION[name]
    key = "golden_" + name
    if key not in _nbr:
        from oracle import oracle
        rc = oracle.ref_codes_with_exclusions(w)
        _nbr[key] = (rc, oracle.snp_scan(w, rc, lo, hi, "diploid", 4, 0.15, [0.3, 0.7])[0])
    plain = _run(eng, w, key, listed, 8, None, mincov=4, region=(lo, hi))
    got = _run(eng, w, key, listed, 8, ("uniform", D.SEED), mincov=4, region=(lo, hi))
    assert np.array_equal(got["pos"], listed)
    _check(w, key, got, plain, D.SEED, 8, 20, mincov=4)


# ---------------------------------------------------------------------------------------------------------------- indel
@pytest.fixture(scope="module")
def indel_files(tmp_path_factory):
    import bamio
    d = tmp_path_factory.mktemp("downsample_indel")
    out = {}
    for wname in ("listed", "deep"):
        h = D.indel_host(wname)
        w = h["w"]
        bam, fa = str(d / (wname + ".bam")), str(d / (wname + ".fa"))
        bamio.write_bam(bam, w.chrom, w.length, h["all_recs"])
        bamio.write_fasta(fa, w.chrom, w.ref)
        out[wname] = (bam, fa)
    return out


def _indel_dct(files, name, maxcov, downsample=None, seed=D.SEED, **kw):
    from test_indel_pipeline import _params
    case = D.INDEL_CASES[name]
    w = D.indel_world(case["world"])
    d = _params(files[case["world"]][1], maxcov=maxcov, **dict(D.INDEL_BASE, **kw))
    cols, is_long = D.indel_listed(case)
    d["genotype_indel_sites"] = {w.chrom: (cols, is_long)}
    d["genotype_indel_only"] = True
    if downsample is not None:
        d.update(downsample=downsample, downsample_seed=seed)
    return d, [dict(chrom=w.chrom, start=a, end=b, sam_path=files[case["world"]][0]) for a, b in case["chunks"]]


def _indel_run(files, name, maxcov, downsample=None, seed=D.SEED):
    from nanocaller_amd import generate_indel_pileups as gip
    d, chunks = _indel_dct(files, name, maxcov, downsample, seed)
    r, _, order = gip.indel_sites_for_chunks(d, chunks, 0, D.INDEL_CASES[name]["haploid"])
    assert order == list(range(len(chunks)))
    r["xh"] = r.pop("x").cpu().numpy()
    return r


def _indel_same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("pos", "chunk", "type", "phase", "ref_len", "alt_len", "alt", "xh"))


def _indel_check(files, name, maxcov, seed=D.SEED, need_sharp=10):
    import oracle_pool
    from util import device_alleles, oracle_alleles
    haploid = D.INDEL_CASES[name]["haploid"]
    S = 1 if haploid else 3
    plain = _indel_run(files, name, maxcov)
    got = _indel_run(files, name, maxcov, "uniform", seed)
    assert _indel_same(got, _indel_run(files, name, maxcov, "uniform", seed))                    # two runs, bit for bit
    # the kept / dropped decision of every anchor is what it was, and what the set sizes say
    expect = [(ci, an, t) for ci, an, t in D.indel_anchors(name) if D.indel_kept(name, an)]
    for r in (plain, got):
        assert list(zip(r["chunk"].tolist(), r["pos"].tolist(), r["type"].tolist())) == expect
    tasks, where, n_sharp = [], [], {0: 0, 1: 0, 2: 0}
    for k, an in enumerate(got["pos"].tolist()):
        gx, px = got["xh"][k].reshape(S, 5, 128, 2), plain["xh"][k].reshape(S, 5, 128, 2)
        for t, (s, ids) in enumerate(D.indel_sets(name, an)):
            if not D.sharp(seed, an, s, ids.size, maxcov):           # not sampled, or the sample is the first maxcov: the plain plan's set, bit for bit
                assert np.array_equal(gx[t], px[t]) and device_alleles(got, k)[t] == device_alleles(plain, k)[t], (an, s)
            if ids.size > maxcov:
                tasks.append(D.indel_set_task(name, an, s, ids, seed, maxcov))
                where.append((k, t, s, an))
        if not haploid:                                              # PS: the unsampled pileup's first HP 1 read
            assert int(got["phase"][k]) == int(plain["phase"][k]) == D.indel_first_hp1_ps(name, an), an
    for (k, t, s, an), ob in zip(where, oracle_pool.map_sites(tasks)):
        assert ob is not None, an
        assert np.array_equal(got["xh"][k].reshape(S, 5, 128, 2)[t], ob["x"][0]), "set %d of the anchor %d differs from its sample's tensor" % (s, an)
        assert device_alleles(got, k)[t] == oracle_alleles(ob["cns"][:1], ob["win"], int(got["type"][k]))[0], (an, s)
        n_sharp[s] += D.sharp(seed, an, s, D.indel_sets(name, an)[t][1].size, maxcov)
    assert all(n_sharp[s] >= need_sharp for s in ((0,) if haploid else (0, 1, 2))), n_sharp
    return plain, got


@pytest.mark.parametrize("maxcov", D.INDEL_MAXCOVS)
def test_indel_sets_equal_their_samples_diploid(indel_files, maxcov):
    """anchors where one haplotype set, the other, only `all` and all three sets exceed maxcov; sets of maxcov and maxcov + 1 reads (the host test
    counts them)"""
    plain, got = _indel_check(indel_files, "dip", maxcov)
    assert not np.array_equal(plain["xh"], got["xh"])


@pytest.mark.parametrize("maxcov", D.INDEL_MAXCOVS)
def test_indel_sets_equal_their_samples_haploid(indel_files, maxcov):
    _indel_check(indel_files, "hap", maxcov)


def test_indel_sample_crosses_a_step_of_the_tile(indel_files):
    _, got = _indel_check(indel_files, "deep", 8)
    assert sum(1 for an in got["pos"].tolist() if D.indel_spans_a_step("deep", an, 8)) >= 5


def test_indel_nothing_sampled_and_mode_first_are_the_plain_plan(indel_files):
    plain = _indel_run(indel_files, "dip", 160)
    assert _indel_same(plain, _indel_run(indel_files, "dip", 160, "uniform"))                    # no set exceeds 160: the sampled form changes nothing
    assert _indel_same(_indel_run(indel_files, "dip", 8), _indel_run(indel_files, "dip", 8, "first"))
    assert not _indel_same(_indel_run(indel_files, "dip", 8, "uniform", 812), _indel_run(indel_files, "dip", 8, "uniform", 4242))


def test_indel_refusals(eng, indel_files):
    from nanocaller_amd import _lib, indel_device
    from nanocaller_amd import generate_indel_pileups as gip
    d, chunks = _indel_dct(indel_files, "dip", 8, "uniform", impute_indel_phase=True)
    with pytest.raises(ValueError, match="impute_indel_phase"):
        gip.indel_sites_for_chunks(d, chunks, 0, False)
    d.pop("genotype_indel_sites"), d.pop("genotype_indel_only")
    eng2, dp, reads_c, ctg, excl, mates = gip.indel_pack_for(d, chunks, 0, by_name=False)
    kw = dict(mincov=4, maxcov=8, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6, window_after=160, excl=excl)
    with pytest.raises(_lib.NanoCallerHipError) as ei:
        indel_device.indel_sites_device(eng2, dp, reads_c, len(ctg["fasta"]), [(1_000, 6_000)], impute=True, downsample=("uniform", 812), **kw)
    assert ei.value.status == _lib.NC_ERR_UNSUPPORTED and "impute_indel_phase" in str(ei.value)
    r = indel_device.indel_sites_device(eng2, dp, reads_c, len(ctg["fasta"]), [(1_000, 6_000)], impute=True, **kw)      # (cleared: the plain plan runs)
    assert r["n"] > 0
    with pytest.raises(ValueError):
        gip.indel_sites_for_chunks(dict(d, impute_indel_phase=False, downsample="sometimes"), chunks, 0, False)


# ---------------------------------------------------------------------------------------------------------------- through the callers
def test_snp_call_chunks_with_and_without_the_key(eng):
    """snpCaller.call_chunks at maxcov = 8: without the key and with 'first' the same arrays; with 'uniform' the probabilities are those of the
    existing CNN on the yardstick's tensors (the bound of the smoke test: 1e-4 against the float64 oracle), which the plain run's are not"""
    from nanocaller_amd import snpCaller
    from nanocaller_amd.weights import Weights, get_SNP_model
    from oracle import oracle
    w, listed = D.golden_sites("ont")
    lo, hi = D.GOLDEN_REGION["ont"]
    params = dict(sam_path=w, fasta_path=None, mincov=4, maxcov=8, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002",
                  seq="ont", supplementary=False, exclude_bed=None, disable_coverage_normalization=False)
    chunks = [dict(chrom=w.chrom, start=lo, end=hi, ploidy="diploid")]
    plain = snpCaller.call_chunks(params, chunks)
    first = snpCaller.call_chunks(dict(params, downsample="first", downsample_seed=5), chunks)
    got = snpCaller.call_chunks(dict(params, downsample="uniform"), chunks)
    keys = ("pos", "ref", "probs", "gt", "dp", "freq", "fwd_dp", "rev_dp")
    assert all(np.array_equal(plain[k], first[k]) for k in keys)
    assert all(np.array_equal(plain[k], got[k]) for k in ("pos", "ref", "dp", "freq", "fwd_dp", "rev_dp"))
    pos = [int(v) for v in got["pos"]]
    assert len(pos) >= 20 and set(listed.tolist()) <= set(pos)
    rc = oracle.ref_codes_with_exclusions(w)
    nbr = oracle.snp_scan(w, rc, lo, hi, "diploid", 4, 0.15, [0.4, 0.6])[0]
    yard = [D.snp_yardstick(w, rc, nbr, v, D.SEED, 8) for v in pos]
    mats, depth = np.stack([y[0] for y in yard]), float(np.mean([y[3] for y in yard]))
    path, cov = get_SNP_model("ONT-HG002")
    ep, _ = oracle.snp_forward(Weights(path).flat, mats, np.asarray(got["ref"], np.int32), np.full(len(pos), cov / depth), precision="f64")
    err = np.abs(got["probs"] - ep).max(axis=1)
    print("max |dp| against the yardstick: uniform %.2e, plain %.2e" % (err.max(), np.abs(plain["probs"] - ep).max()))
    assert err.max() < 1e-4
    assert (np.abs(plain["probs"] - ep).max(axis=1) > 1e-3).sum() >= 20
    with pytest.raises(ValueError):
        snpCaller.call_chunks(dict(params, downsample="sometimes"), chunks)


def test_indel_records_with_and_without_the_key(eng, indel_files):
    """the indel step's record text (device pipeline -> K9 -> native rules) at maxcov = 8: without the key and with 'first' the same bytes; with
    'uniform' the probabilities behind the records are the existing CNN's on the sampled plan's tensors, whose sets the tests above hold to the
    yardstick"""
    import torch
    from nanocaller_amd import _lib
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.weights import Weights, get_indel_model
    eng.load_weights(_lib.MODEL_INDEL, Weights(get_indel_model("ONT-HG002")))

    def text(downsample):
        d, chunks = _indel_dct(indel_files, "dip", 8, downsample)
        counts = {}
        return gip.indel_chunks_vcf_text(d, chunks, 0, False, _lib.MODEL_INDEL, counts), counts
    plain, _ = text(None)
    assert plain == text("first")[0] and sum(len(t) for t in plain) > 0
    got, counts = text("uniform")
    assert got != plain
    r = _indel_run(indel_files, "dip", 8, "uniform")
    probs = eng.indel_forward(_lib.MODEL_INDEL, torch.from_numpy(r["xh"]).to(eng.device)).cpu().numpy()
    assert np.array_equal(counts["pos"], r["pos"]) and np.array_equal(counts["probs"], probs)


def test_device_ingest_and_host_decoded_pack_give_equal_tensors(eng, tmp_path):
    """the mixed world written to a BAM: the pack the device ingest builds and the pack of the host-decoded records hold the same entries in the same
    order, so the same sites draw the same samples"""
    import copy

    import bamio
    from nanocaller_amd.bam import read_bam
    from nanocaller_amd.device_bam import DeviceBam
    from nanocaller_amd.wire import build_wire_from_world, upload_wire
    w = copy.copy(D.mixed_world())
    R = w.n_reads
    w.meta = dict(events=(np.zeros(R + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)), hap=np.zeros(R, np.int8), ps=np.zeros(R, np.int32))
    bam, fa = str(tmp_path / "m.bam"), str(tmp_path / "m.fa")
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, None))
    bamio.write_fasta(fa, w.chrom, w.ref)
    db = DeviceBam(bam, 0).load()
    _packs["ingest_device"] = db.pack(db.prepare(w.chrom, w.ref))
    _packs["ingest_host"] = upload_wire(eng, build_wire_from_world(read_bam(bam, fa, w.chrom)))
    listed, _ = D.mixed_sites(w)
    try:
        a = _run(eng, w, "ingest_device", listed, D.MIXED_MAXCOV, ("uniform", D.SEED), mincov=4)
        b = _run(eng, w, "ingest_host", listed, D.MIXED_MAXCOV, ("uniform", D.SEED), mincov=4)
        plain = _run(eng, w, "ingest_host", listed, D.MIXED_MAXCOV, None, mincov=4)
    finally:
        _packs.pop("ingest_device"), _packs.pop("ingest_host")
    assert _same(a, b) and a["pos"].size >= 20
    sharp = [i for i, v in enumerate(a["pos"].tolist()) if D.sharp(D.SEED, v, 0, D.pileup(w, v).size, D.MIXED_MAXCOV)]
    assert len(sharp) >= 20 and (a["x"][sharp] != plain["x"][sharp]).any(axis=(1, 2, 3)).sum() >= 15


def test_indel_plan_refuses_a_shared_names_table(eng, tmp_path):
    """nc_indel_sites_plan with a shared-names table (nc_indel_set_mates) and the uniform sample: NC_ERR_UNSUPPORTED from the library, ValueError
    from the Python layer; the state is cleared and the name-keyed plan runs afterwards"""
    import bamio
    import test_indel_mates as tim
    from nanocaller_amd import _lib, indel_device
    from nanocaller_amd import generate_indel_pileups as gip
    w = bamio.world_from_arrays(tim.Z, "w_")
    w.names = ["r%07d" % i for i in tim.Z["w_name_id"]]
    bam, fa = str(tmp_path / "m.bam"), str(tmp_path / "m.fa")
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, None))
    bamio.write_fasta(fa, w.chrom, w.ref)
    dct = dict(tim.DCT, fasta_path=fa, maxcov=8)
    chunks = [dict(chrom=w.chrom, start=1, end=4_001, sam_path=bam)]
    eng2, dp, reads_c, ctg, excl, mates = gip.indel_pack_for(dct, chunks, 0, by_name=True)
    assert mates is not None
    kw = dict(mincov=dct["mincov"], maxcov=8, win_size=dct["win_size"], small_win_size=dct["small_win_size"], ins_t=dct["ins_t"], del_t=dct["del_t"],
              window_after=160, excl=excl, mates=mates)
    with pytest.raises(_lib.NanoCallerHipError) as ei:
        indel_device.indel_sites_device(eng2, dp, reads_c, len(ctg["fasta"]), [(1, 4_001)], downsample=("uniform", 812), **kw)
    assert ei.value.status == _lib.NC_ERR_UNSUPPORTED and "share read names" in str(ei.value)
    assert indel_device.indel_sites_device(eng2, dp, reads_c, len(ctg["fasta"]), [(1, 4_001)], **kw)["n"] > 0
    with pytest.raises(ValueError, match="share read names"):
        gip.indel_sites_for_chunks(dict(dct, downsample="uniform"), chunks, 0, False)


# ---------------------------------------------------------------------------------------------------------------- through the files
def _snp_params(bam, fa, out, chrom, length, **kw):
    from nanocaller_amd.utils import get_chunks
    regions = ((chrom, 1, length, "diploid"),)
    return dict(chunks_list=get_chunks(regions, 2), regions_list=regions, sam_path=bam, fasta_path=fa, mincov=4, maxcov=8, min_allele_freq=0.15,
                min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=2, vcf_path=out, prefix="t", sample="S", seq="ont", supplementary=False,
                exclude_bed=None, suppress_progress=True, phase_qual_score=10, verbose=False, disable_coverage_normalization=False, **kw)


def _file_records(path):
    import gzip
    return [ln for ln in gzip.open(path, "rt") if not ln.startswith("#")]


def test_snp_files_with_and_without_the_key(indel_files, tmp_path, monkeypatch):
    """snpCaller.call_manager (caller, the records thread, the merge) on a small BAM at maxcov = 8.  Without the key, with 'first' and with
    NC_DOWNSAMPLE=first the records are the same bytes, and they are the oracle pipeline's with its first-maxcov cut (what the parent wrote); with the
    key -- in the dict, or from the environment -- the records are those of the existing CNN and rules on the yardstick's tensors."""
    import os
    from nanocaller_amd import snpCaller
    from nanocaller_amd.bam import read_bam
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.weights import Weights, get_SNP_model
    from oracle import oracle
    bam, fa = indel_files["listed"]
    w = D.indel_world("listed")
    monkeypatch.delenv("NC_DOWNSAMPLE", raising=False)
    monkeypatch.delenv("NC_DOWNSAMPLE_SEED", raising=False)

    def run(tag, **kw):
        out = str(tmp_path / tag)
        os.makedirs(out)
        release_contig()
        sp = _snp_params(bam, fa, out, w.chrom, w.length, **kw)
        snpCaller.call_manager(sp)
        return _file_records(os.path.join(out, "t.unfiltered.snps.vcf.gz")), sp
    plain, sp = run("plain")
    assert plain == run("first", downsample="first", downsample_seed=3)[0]
    got, _ = run("uniform", downsample="uniform")
    monkeypatch.setenv("NC_DOWNSAMPLE", "uniform")
    assert got == run("env")[0]
    monkeypatch.delenv("NC_DOWNSAMPLE")
    assert got != plain and len(plain) >= 20
    world = read_bam(bam, fa, w.chrom)
    rc = oracle.ref_codes_with_exclusions(world)
    wd, cov = Weights(get_SNP_model("ONT-HG002")[0]), get_SNP_model("ONT-HG002")[1]
    dct = dict(threshold=[0.4, 0.6], mincov=4, maxcov=8, min_allele_freq=0.15, min_nbr_sites=1, seq="ont")
    exp_plain, exp_uni, n_sharp = [], [], 0
    for c in sp["chunks_list"]:
        pos, ref, mat, dp, freq, depth, fwd, rev = oracle.get_snp_testing_candidates(world, dct, c)
        if not len(pos):
            continue
        r1 = np.argmax(ref, 1).astype(np.int32)
        exp_plain += snpCaller.snp_vcf_lines(c["chrom"], pos, r1, oracle.snp_forward(wd.flat, mat, r1, cov / depth)[0], dp, freq, fwd, rev)
        nbr = oracle.snp_scan(world, rc, c["start"], c["end"], "diploid", 4, 0.15, [0.4, 0.6])[0]
        yard = [D.snp_yardstick(world, rc, nbr, int(v), D.SEED, 8) for v in pos]
        n_sharp += sum(D.sharp(D.SEED, int(v), 0, D.pileup(world, int(v)).size, 8) for v in pos)
        ymat, ydepth = np.stack([y[0] for y in yard]), float(np.mean([y[3] for y in yard]))
        assert ydepth == depth
        exp_uni += snpCaller.snp_vcf_lines(c["chrom"], pos, r1, oracle.snp_forward(wd.flat, ymat, r1, cov / ydepth)[0], dp, freq, fwd, rev)
    assert n_sharp >= 20
    for rec, exp in ((plain, exp_plain), (got, exp_uni)):
        exp = sorted(exp, key=lambda ln: int(ln.split("\t")[1]))
        assert len(rec) == len(exp)
        for g, e in zip(rec, exp):
            gf, ef = g.split("\t"), e.split("\t")
            assert gf[:5] == ef[:5] and gf[6] == ef[6] and gf[9].split(":")[:2] == ef[9].split(":")[:2], (g, e)


def test_indel_files_with_and_without_the_key(indel_files, tmp_path, monkeypatch):
    """indelCaller.call_manager(mode='indels') (caller, indel_run, the merge) on the haplotagged small BAM at maxcov = 8.  Without the key and with
    'first' the same records; with the key the records are the text of the sampled device plan (whose sets the tests above hold to the yardstick)
    through the existing CNN and rules, chunk by chunk."""
    import os
    from nanocaller_amd import _lib, indelCaller
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.utils import get_chunks
    bam, fa = indel_files["listed"]
    w = D.indel_world("listed")
    monkeypatch.delenv("NC_DOWNSAMPLE", raising=False)
    monkeypatch.delenv("NC_DOWNSAMPLE_SEED", raising=False)
    regions = ((w.chrom, 1, w.length, "diploid"),)

    def params(out, **kw):
        return dict(chunks_list=get_chunks(regions, 2, max_chunk_size=100000), mode="indels", snp_vcf=None, regions_list=regions, sam_path=bam,
                    fasta_path=fa, mincov=4, maxcov=8, indel_model="ONT-HG002", cpu=2, vcf_path=out, prefix="t", sample="S", seq="ont", del_t=0.6,
                    ins_t=0.4, impute_indel_phase=False, supplementary=False, exclude_bed=None, win_size=40, small_win_size=4, enable_whatshap=False,
                    suppress_progress=True, phase_qual_score=10, verbose=False, **kw)

    def run(tag, **kw):
        out = str(tmp_path / tag)
        os.makedirs(out)
        files = indelCaller.call_manager(params(out, **kw))
        return _file_records(files["indels"])
    plain = run("plain")
    assert plain == run("first", downsample="first") and len(plain) >= 10
    got = run("uniform", downsample="uniform")
    assert got != plain
    ip = params(str(tmp_path))
    chunks = [dict(c, sam_path=bam) for c in ip["chunks_list"]]
    texts = gip.indel_chunks_vcf_text(dict(ip, downsample="uniform"), chunks, 0, False, _lib.MODEL_INDEL)
    exp = [ln for t in texts for ln in t.decode("ascii").splitlines(True) if indelCaller._non_snp(ln)]
    assert sorted(got, key=lambda ln: int(ln.split("\t")[1])) == sorted(exp, key=lambda ln: int(ln.split("\t")[1]))

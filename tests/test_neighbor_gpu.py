"""Listed neighbour sites and background sampling on the GPU (nc_snp_scan_set_nbr_sites, nc_snp_scan_set_sampling, k_scan<.., false, true>) against
tests/neighbor_ref.py, from the scan up to the trainer.  Golden worlds only (<= 135 kb).
Run on a real MI355X: python -m pytest tests -m gpu"""
import os
import tempfile

import numpy as np
import pytest

from tests import genotype_ref as G
from tests import neighbor_ref as R
from tests.util import assert_tuple_matches_gold, load_world

pytestmark = pytest.mark.gpu

KW = dict(mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])
ENV = ("NC_GENOTYPE_SITES", "NC_GENOTYPE_ONLY", "NC_NEIGHBOR_SITES", "NC_NEIGHBOR_ONLY")


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _dct(world, dct, exclude, **kw):
    return dict(dct, sam_path=world, fasta_path=None, exclude_bed=exclude if exclude else None, **kw)


_ont = {}


def ont_columns():
    """the `ont` world's columns over the whole contig, computed once: (world, nbr, N, E, En, Ealt, EN)"""
    if not _ont:
        world = load_world("ont")
        region = dict(chrom=world.chrom, start=1, end=world.length, ploidy="diploid")
        rc, nbr, N, E, En, Ealt = G.scans(world, KW, region, None)
        _ont["v"] = (world, nbr, N, E, En, Ealt, R.eligible_neighbors(world, KW, region, None))
    return _ont["v"]


@pytest.mark.parametrize("only", [False, True], ids=["add", "only"])
@pytest.mark.parametrize("case", G.GPU_CASES)
def test_tuple_with_a_neighbor_list_matches_the_rule(eng, case, only):
    """get_snp_testing_candidates with dct['neighbor_sites']: every field exact, as the goldens are compared"""
    from nanocaller_amd.generate_SNP_pileups import get_snp_testing_candidates
    world, dct, region, exclude = G.load_case(case)
    exp = R.expected_for(case, only)
    out = get_snp_testing_candidates(_dct(world, dct, exclude, neighbor_sites={world.chrom: G.site_list(case)}, neighbor_only=only), region)
    assert len(exp[0]) > 20
    assert_tuple_matches_gold(out, G.as_gold(exp))


def _edge_list(dpk, world, tile_size):
    """the list of test_genotype_gpu.test_positions_on_every_edge_of_the_bitmap: every edge of a lane's 16-bit load, of a 32-bit word, of a tile,
    of the contig; positions the device must drop; duplicates, unsorted"""
    t0, T, nt = dpk.tile_pos0, dpk.tile_size, dpk.n_tiles
    assert nt > 2
    g = []
    for t in sorted({0, 1, nt // 2, nt - 2, nt - 1}):
        for w in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, T // 2 - 1, T // 2, T - 33, T - 32, T - 17, T - 16, T - 15, T - 2, T - 1):
            g.append(t * T + w)
    p = np.array(g, np.int64) + t0
    ignored = np.array([0, -1, -5, t0 - 1, t0 - 32, -(1 << 30), np.iinfo(np.int32).min, t0 + nt * T, t0 + nt * T + 1, t0 + nt * T + 31, world.length + 1,
                        world.length + 100_000, np.iinfo(np.int32).max], np.int64)
    s = np.concatenate([p, ignored, [1, world.length, 2, world.length - 1], p[::3], ignored[::2]])
    np.random.Generator(np.random.PCG64(tile_size)).shuffle(s)
    return s


@pytest.mark.parametrize("tile_size", [1024, 2048, 4096])
def test_neighbor_positions_on_every_edge_of_the_bitmap(eng, tile_size):
    """the edge list as the neighbour list, a device tensor (nothing on the host filters it), all three instantiations of the new form: the
    neighbours are nbr' in both modes, the candidate arrays the plain scan's"""
    import torch
    from nanocaller_amd.pack import pack_world
    world, nbr, N, E, En, Ealt, EN = ont_columns()
    dpk = eng.upload(pack_world(world, tile_size=tile_size))
    s = _edge_list(dpk, world, tile_size)
    d_nbr = torch.from_numpy(s.astype(np.int32)).cuda()
    LE = np.intersect1d(s, EN)
    assert len(LE) > 60 and len(np.setdiff1d(LE, nbr)) > 40
    k = np.searchsorted(E, N)
    for only in (False, True):
        sites = eng.snp_scan(dpk, [(1, world.length)], nbr_sites=d_nbr, nbr_only=only, **KW)
        assert np.array_equal(eng.fetch_nbr_sites(sites.n_nbr), R.expected_neighbors(nbr, EN, s, only))
        assert np.array_equal(sites.pos, N) and np.array_equal(sites.dp, En[k]) and np.array_equal(sites.alt, Ealt[k])


def test_a_neighbor_list_and_a_candidate_list_in_one_scan(eng):
    """different positions in the two lists: neighbours and candidates each equal their own yardstick, neither list leaks into the other's output"""
    from nanocaller_amd.pack import pack_world
    world, nbr, N, E, En, Ealt, EN = ont_columns()
    dpk = eng.upload(pack_world(world))
    quiet = np.setdiff1d(E, np.union1d(N, nbr))                      # eligible, neither candidate nor neighbour on their own
    nl, cl = quiet[3::40], quiet[7::40]
    assert len(nl) > 1000 and len(cl) > 1000 and not np.intersect1d(nl, cl).size
    for nbr_only in (False, True):
        for sites_only in (False, True):
            sites = eng.snp_scan(dpk, [(1, world.length)], nbr_sites=nl, nbr_only=nbr_only, sites=cl, sites_only=sites_only, **KW)
            exp_c = cl if sites_only else np.union1d(N, cl)
            k = np.searchsorted(E, exp_c)
            assert np.array_equal(sites.pos, exp_c) and np.array_equal(sites.dp, En[k]) and np.array_equal(sites.alt, Ealt[k])
            assert np.array_equal(eng.fetch_nbr_sites(sites.n_nbr), R.expected_neighbors(nbr, EN, nl, nbr_only))


KEEPS = {"every_bin": [0.02, 0.05, 0.3, 0.5, 0.7, 0.9], "bin_1": [0.0, 0.04, 0.0, 0.0, 0.0, 0.0]}
_sampled_scans = {}


@pytest.mark.parametrize("tile_size", [1024, 2048, 4096])
def test_sampling_equals_the_numpy_restatement_at_every_tile_size(eng, tile_size):
    """sample=(seed, keep) on `ont`, two seeds, a table with every bin set and one with bin 1 alone: positions, dp and alt exact, and the same at
    every tile size (the decision depends on the position alone).  min_allele_freq = 0.3 leaves columns of every bin under the candidate test."""
    from nanocaller_amd.pack import pack_world
    world, nbr, N, E, En, Ealt, EN = ont_columns()
    dpk = eng.upload(pack_world(world, tile_size=tile_size))
    kw = dict(KW, min_allele_freq=0.3)
    for seed in (1, 0xC0FFEE11):
        for name, keep in KEEPS.items():
            exp = R.expected_sampled_scan(E, En, Ealt, 0.3, seed, keep)
            plain = int((Ealt / En >= 0.3).sum())
            assert len(exp[0]) > plain + 500
            sites = eng.snp_scan(dpk, [(1, world.length)], sample=(seed, keep), **kw)
            got = (sites.pos.copy(), sites.dp.copy(), sites.alt.copy())
            assert all(np.array_equal(a, b) for a, b in zip(got, exp)), (seed, name)
            first = _sampled_scans.setdefault((seed, name), got)
            assert all(np.array_equal(a, b) for a, b in zip(got, first))
            assert np.array_equal(eng.fetch_nbr_sites(sites.n_nbr), nbr)
    # with a list of positions to genotype in add mode: the union
    lst = np.setdiff1d(E, N)[5::50]
    exp = R.expected_sampled_scan(E, En, Ealt, 0.15, 9, KEEPS["every_bin"], sites=lst)
    only_sampled = R.expected_sampled_scan(E, En, Ealt, 0.15, 9, KEEPS["every_bin"])[0]
    assert len(np.setdiff1d(lst, only_sampled)) > 500 and len(np.setdiff1d(only_sampled, np.union1d(N, lst))) > 500
    sites = eng.snp_scan(dpk, [(1, world.length)], sample=(9, KEEPS["every_bin"]), sites=lst, **KW)
    assert np.array_equal(sites.pos, exp[0]) and np.array_equal(sites.dp, exp[1]) and np.array_equal(sites.alt, exp[2])


def test_no_list_and_no_table_is_carried_into_the_next_scan(eng):
    """a plain scan right after a scan with a neighbour list and a sampling table gives the plain result"""
    from nanocaller_amd.pack import pack_world
    world, nbr, N, E, En, Ealt, EN = ont_columns()
    dpk = eng.upload(pack_world(world))
    k = np.searchsorted(E, N)
    for only in (False, True):
        busy = eng.snp_scan(dpk, [(1, world.length)], nbr_sites=E[::9], nbr_only=only, sample=(3, [0.1] * 6), **KW)
        assert busy.n_sites > len(N) + 1000 and busy.n_nbr != len(nbr)
        plain = eng.snp_scan(dpk, [(1, world.length)], **KW)
        assert np.array_equal(plain.pos, N) and np.array_equal(plain.dp, En[k]) and np.array_equal(plain.alt, Ealt[k])
        assert np.array_equal(eng.fetch_nbr_sites(plain.n_nbr), nbr)
    with pytest.raises(ValueError):
        eng.snp_scan(dpk, [(1, world.length)], sample=(1, [0.1] * 5 + [1.0]), **KW)


def test_only_mode_with_no_position_for_the_contig(eng):
    """zero neighbours come back, and with min_nbr_sites = 1 the empty tuple: in only mode min_nbr_sites counts the listed neighbours in reach,
    not the site's own column"""
    from nanocaller_amd.generate_SNP_pileups import get_snp_testing_candidates
    from nanocaller_amd.pack import pack_world
    world, nbr, N, E, En, Ealt, EN = ont_columns()
    dpk = eng.upload(pack_world(world))
    for lst in ([], None, [0, -4, world.length + 7]):
        sites = eng.snp_scan(dpk, [(1, world.length)], nbr_sites=lst, nbr_only=True, **KW)
        assert sites.n_nbr == 0 and np.array_equal(sites.pos, N)
    world, dct, region, exclude = G.load_case("ont_dip")
    assert dct["min_nbr_sites"] == 1 and R.expected(world, dct, region, exclude, [], True) == G.EMPTY
    for lst in ({world.chrom: []}, {"another_contig": [region["start"] + 5]}):
        assert get_snp_testing_candidates(_dct(world, dct, exclude, neighbor_sites=lst, neighbor_only=True), region) == G.EMPTY
    # one listed site: the sites it reaches keep their tensor, the others have none (the yardstick asks the oracle for two columns)
    one = [int(G.site_classes(world, dct, region, exclude)["natural"][0])]
    exp = R.expected(world, dct, region, exclude, one, True)
    out = get_snp_testing_candidates(_dct(world, dct, exclude, neighbor_sites={world.chrom: one}, neighbor_only=True), region)
    assert 20 < len(exp[0])
    assert_tuple_matches_gold(out, G.as_gold(exp))
    # the same lists in add mode change nothing
    plain = get_snp_testing_candidates(_dct(world, dct, exclude), region)
    out = get_snp_testing_candidates(_dct(world, dct, exclude, neighbor_sites={world.chrom: []}), region)
    assert len(plain[0]) > 100 and len(exp[0]) < len(plain[0])
    assert_tuple_matches_gold(out, G.as_gold(plain))
    # the caller's route drops the same sites
    from nanocaller_amd import snpCaller
    params = dict(_dct(world, dct, exclude), snp_model="ONT-HG002", disable_coverage_normalization=False, neighbor_only=True)
    assert snpCaller.call_chunks(dict(params, neighbor_sites={world.chrom: []}), [region])["n"] == 0
    r = snpCaller.call_chunks(dict(params, neighbor_sites={world.chrom: one}), [region])
    assert r["n"] == len(exp[0]) and np.array_equal(r["pos"], exp[0])


# ------------------------------------------------------------------ training
PARAMS = dict(fasta_path=None, mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6], seq="ont", supplementary=False,
              exclude_bed=None, disable_coverage_normalization=False)
_train = {}


def train_world():
    """the world of tests/test_snp_train_gpu.py and its first-pass examples, computed once"""
    if not _train:
        from nanocaller_amd import train
        from nanocaller_amd.synth import make_world
        world = make_world(seed=7, length=50_000, depth=20, read_len_scale=0.4)
        params = dict(PARAMS, sam_path=world)
        _train["v"] = (world, params, train.world_truth(world), train.snp_training_examples(params, neg_ratio=2.0, seed=0)[world.chrom])
    return _train["v"]


def test_truth_neighbors_appends_second_examples(eng):
    """the first pass unchanged, then every kept site with the truth's heterozygous sites as its only neighbours: tensors equal the oracle's
    featuriser on that neighbour list"""
    import torch
    from nanocaller_amd import train
    from oracle import oracle
    world, params, truth, first = train_world()
    x, ref, lab, pos, depth = train.snp_training_examples(params, neg_ratio=2.0, seed=0, truth_neighbors=True)[world.chrom]
    n1 = first[0].shape[0]
    assert train.snp_training_examples.plan[world.chrom]["n_first"] == n1 > 200
    assert torch.equal(x[:n1], first[0]) and torch.equal(ref[:n1], first[1]) and np.array_equal(lab[:n1], first[2]) and np.array_equal(pos[:n1], first[3])
    assert depth == first[4]
    region = dict(chrom=world.chrom, start=1, end=world.length, ploidy="diploid")
    het = np.array(sorted(p for p, t in truth.items() if t[0] == 1), np.int64)
    EN = R.eligible_neighbors(world, params, region, None)
    rc = oracle.ref_codes_with_exclusions(world)
    nbr2 = np.intersect1d(het, EN).astype(np.int32)
    assert len(nbr2) > 20
    p2, r2, m2, _, _, _ = oracle.snp_featurize(world, rc, nbr2, first[3].astype(np.int32), "ont", 160, 2)     # (min_nbr_sites = 1 neighbour + the site)
    n2 = len(p2)
    assert 100 < n2 <= n1 and x.shape[0] == n1 + n2
    assert np.array_equal(pos[n1:], p2) and np.array_equal(ref[n1:].cpu().numpy(), r2) and np.array_equal(x[n1:].cpu().numpy(), m2)
    at = np.searchsorted(first[3], p2)
    assert np.array_equal(lab[n1:], first[2][at])
    assert (x[n1:] != x[:n1][torch.from_numpy(at).to(x.device)]).flatten(1).any(1).sum().item() > 20       # (other neighbours: other tensors)


def test_background_samples_columns_under_the_threshold(eng):
    """the extra positions are a subset of the restated sample, none is a truth position, the three caps hold, the labels are reference calls;
    the other examples are the plain run's"""
    import torch
    from nanocaller_amd import train
    world, params, truth, first = train_world()
    region = dict(chrom=world.chrom, start=1, end=world.length, ploidy="diploid")
    rc, nbr, N, E, En, Ealt = G.scans(world, params, region, None)
    truth_pos = np.array(sorted(truth), np.int64)
    for background in (True, {0: 40, 2: 3}):
        x, ref, lab, pos, depth = train.snp_training_examples(params, neg_ratio=2.0, seed=0, background=background)[world.chrom]
        plan = train.snp_training_examples.plan[world.chrom]
        seed, keep = plan["sample"]
        extra = ~np.isin(pos, first[3])
        T = int(np.isin(first[3], truth_pos).sum())
        caps = [T, T // 3, T // 3] if background is True else [40, 0, 3]
        assert plan["caps"] == caps and plan["n_truth"] == T > 30
        # the other examples: the plain run's
        sel = torch.from_numpy(~extra).to(x.device)
        assert np.array_equal(pos[~extra], first[3]) and np.array_equal(lab[~extra], first[2]) and torch.equal(x[sel], first[0])
        # the restated sample
        cand = (Ealt / En >= 0.15) | np.isin(E, truth_pos)
        samp = E[R.sampled(E, En, Ealt, cand, seed, keep)]
        assert extra.sum() > 0 and np.isin(pos[extra], samp).all() and not np.isin(pos[extra], truth_pos).any()
        k = np.searchsorted(E, pos[extra])
        grp = np.minimum(2, R.bins(En[k], Ealt[k]))
        got = np.bincount(grp, minlength=3).tolist()
        avail = np.bincount(np.minimum(2, R.bins(En, Ealt)[np.isin(E, samp)]), minlength=3).tolist()
        print("background %r: T %d, caps %s, sampled by the scan %s, kept %s" % (background, T, caps, avail, got))
        assert all(got[g] == min(caps[g], avail[g]) for g in range(3))
        assert np.all(Ealt[k] / En[k] < 0.15)
        rcode = ref.cpu().numpy()[extra]
        want = np.zeros((int(extra.sum()), 5), np.uint8)
        want[np.arange(len(rcode)), rcode] = 1
        assert np.array_equal(lab[extra], want)                      # (0, ref, ref): the reference-call label
        assert np.all(np.diff(pos) > 0)


def test_train_snp_model_with_both_keys_writes_a_loadable_model(eng):
    from nanocaller_amd import train
    from nanocaller_amd.weights import Weights
    world, params, truth, first = train_world()
    with tempfile.TemporaryDirectory() as tmp:
        hist = train.train_snp_model(dict(params, out_dir=os.path.join(tmp, "m"), epochs=1, batch=128, seed=2, truth_neighbors=True, background=True))
        plan = train.snp_training_examples.plan[world.chrom]
        assert len(hist) == 1 and np.isfinite(hist[0]["train_cost"]) and plan["n_first"] > first[0].shape[0]
        w = Weights(hist[0]["path"])
        assert w.kind == 0 and 10 < w.train_coverage < 30 and np.isfinite(w.flat).all()

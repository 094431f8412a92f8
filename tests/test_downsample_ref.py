"""The uniform sample above maxcov without a GPU: nanocaller_amd.downsample against the independent restatement of tests/downsample_ref.py, the
rule's own properties (distinct keys, uniformity under a stated bound), the proof that the worlds of tests/test_downsample_gpu.py hold enough sites
at which the sample is NOT the first maxcov reads, and the parameter checks."""
import numpy as np
import pytest

import downsample_ref as D
from nanocaller_amd import downsample as M


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_mixers_agree():
    rng = np.random.default_rng(1)
    p = rng.integers(-2**31, 2**31, 2000)
    for seed in (0, 812, 0xffffffff, 0x68E31DA4):
        a, b = M.mix32(p, seed), D.mix32_vec(p, seed)
        assert np.array_equal(a.astype(np.uint64), b)
        assert [int(v) for v in a[:50]] == [D.mix32(int(q), seed) for q in p[:50]]


def _draws():
    rng = np.random.default_rng(2)
    fixed = [(160, 160), (161, 160), (5, 1), (2, 1), (300, 255), (256, 255), (1025, 1024), (5000, 1024), (100_000, 160), (100_000, 1024), (7, 255), (0, 4)]
    out = [(int(rng.integers(0, 2**32)), int(rng.integers(1, 2**31 - 1)), int(rng.integers(0, 3)), n, k) for n, k in fixed]
    for _ in range(60):
        k = int(rng.integers(1, 300))
        out.append((int(rng.integers(0, 2**32)), int(rng.integers(1, 2**31 - 1)), int(rng.integers(0, 3)), k + int(rng.integers(-5, 400)) if k > 5 else k + 3, k))
    return out


def test_sample_indices_equal_the_restatement():
    for seed, pos, s, n, k in _draws():
        got = M.sample_indices(seed, pos, s, n, k)
        exp = D.sample(seed, pos, s, n, k)
        assert got.dtype == np.int64 and np.array_equal(got, exp), (seed, pos, s, n, k)
        assert got.size == min(n, k) and np.all(np.diff(got) > 0)
        if n > k:                                                    # the k smallest keys, by the scalar mixer
            base = D.mix32(pos, seed ^ D.SETC[s])
            thr = sorted(D.mix32(j, base) for j in range(n))[k - 1] if n <= 5000 else None
            if thr is not None:
                assert [j for j in range(n) if D.mix32(j, base) <= thr] == got.tolist()
    with pytest.raises(ValueError):
        M.sample_indices(1, 1, 3, 10, 4)
    with pytest.raises(ValueError):
        M.sample_indices(1, 1, 0, 10, 0)


@pytest.mark.parametrize("base", [0, 812, 0x9E3779B1, 0xffffffff, D.mix32(12345, 812)])
def test_keys_of_a_million_ordinals_are_distinct(base):
    k = D.mix32_vec(np.arange(1 << 20, dtype=np.int64), base)
    assert np.unique(k).size == 1 << 20


@pytest.mark.parametrize("n,k,npos", [(161, 160, 20_000), (200, 160, 20_000), (1000, 160, 20_000), (5000, 160, 20_000), (300, 255, 20_000), (40, 16, 50_000)])
def test_uniform_within_five_sigma(n, k, npos):
    """Inclusion count of every ordinal over npos consecutive positions: binomial(npos, k / n), so |z| <= 5 fails by chance about 6e-7 per ordinal;
    the mean selected ordinal of a uniform k-subset has variance (n + 1)(n - k) / (12 k) per draw."""
    cnt = np.zeros(n, np.int64)
    tot = 0.0
    for pos in range(1_000_000, 1_000_000 + npos):
        s = D.sample(812, pos, 0, n, k)
        cnt[s] += 1
        tot += s.mean()
    p = k / n
    z = (cnt - npos * p) / np.sqrt(npos * p * (1 - p))
    se = np.sqrt((n + 1) * (n - k) / (12.0 * k) / npos)
    mean = tot / npos
    print("n %d k %d: max |z| %.2f, chi2/n %.2f, mean ordinal %.2f (%.1f), se %.3f" % (n, k, np.abs(z).max(), float((z * z).sum()) / n, mean, (n - 1) / 2, se))
    assert np.abs(z).max() <= 5.0
    assert abs(mean - (n - 1) / 2) <= 5 * se


def test_sets_and_neighbouring_positions_draw_independently():
    """n = 1000, k = 160: two independent samples share k^2 / n = 25.6 entries on average (hypergeometric, sd 4.3)"""
    a = [np.intersect1d(D.sample(812, p, 0, 1000, 160), D.sample(812, p + 1, 0, 1000, 160)).size for p in range(5000, 5400)]
    b = [np.intersect1d(D.sample(812, p, 1, 1000, 160), D.sample(812, p, 2, 1000, 160)).size for p in range(5000, 5400)]
    c = [np.intersect1d(D.sample(812, p, 0, 1000, 160), D.sample(813, p, 0, 1000, 160)).size for p in range(5000, 5400)]
    for x in (a, b, c):
        assert abs(np.mean(x) - 25.6) < 5 * 4.3 / np.sqrt(400)


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' inputs are sharp
@pytest.mark.parametrize("maxcov", D.STAIR_MAXCOVS_PAIRS + D.STAIR_MAXCOVS_WALK)
def test_staircase_offers_sharp_sites(maxcov):
    w = D.staircase_world()
    depth = np.array([D.pileup(w, int(v)).size for v in D.stair_sites()])
    assert np.array_equal(depth, np.arange(1, D.STAIR_R + 1))            # the depth passes through every value
    seed = D.stair_seed(maxcov)
    sharp = D.sharp_sites(w, D.stair_sites(), seed, maxcov)
    print("maxcov %d: seed %d, %d sharp sites of %d deeper than maxcov" % (maxcov, seed, len(sharp), D.STAIR_R - maxcov))
    assert len(sharp) >= 20 and D.stair_col(maxcov + 1) in sharp
    assert not any(D.sharp(seed, D.stair_col(d), 0, d, maxcov) for d in (maxcov - 1, maxcov) if d >= 1)
    # reads deleted at the centre inside the sample and outside it, at sharp sites
    io = [D.deleted_in_and_out(w, v, seed, maxcov) for v in sharp]
    assert any(i > 0 for i, _ in io) and any(o > 0 for _, o in io)


def test_mixed_world_offers_sharp_sites_over_several_steps_and_at_tile_edges():
    w = D.mixed_world()
    sites, edges = D.mixed_sites(w)
    sharp = D.sharp_sites(w, sites, D.SEED, D.MIXED_MAXCOV)
    assert len(sharp) >= 20 and all(e in sharp for e in edges) and len(edges) >= 2
    keep = (w.read_flag & D.KEEP_MASK) == 0
    assert (~keep).sum() >= 10
    for v in sharp:
        cov = D.pileup(w, v)
        chosen = cov[D.sample(D.SEED, v, 0, cov.size, D.MIXED_MAXCOV)]
        # ranks among the kept reads (the tile's entries hold at least those up to the last covering one): the sample spans more than two 64-entry
        # steps, and reads that do not cover v lie between sampled ones
        rank = np.cumsum(keep) - 1
        assert rank[chosen[-1]] - rank[chosen[0]] > 128
        assert np.setdiff1d(np.arange(chosen[0], chosen[-1]), cov).size > 10


@pytest.mark.parametrize("name", ["ont", "deep"])
def test_golden_worlds_offer_sharp_sites_at_maxcov_8(name):
    w, sites = D.golden_sites(name)
    sharp = D.sharp_sites(w, sites, D.SEED, 8)
    print("%s: %d sites, %d sharp" % (name, len(sites), len(sharp)))
    assert len(sharp) >= 20


# ---------------------------------------------------------------------------------------------------------------- parameters
def test_params_and_environment(monkeypatch):
    monkeypatch.delenv("NC_DOWNSAMPLE", raising=False)
    monkeypatch.delenv("NC_DOWNSAMPLE_SEED", raising=False)
    assert M.resolve({}) == ("first", 812) and M.resolve(None) == ("first", 812)
    assert M.resolve(dict(downsample="uniform")) == ("uniform", 812)
    assert M.resolve(dict(downsample="uniform", downsample_seed=5)) == ("uniform", 5)
    for bad in ("random", "Uniform", 1, True, ""):
        with pytest.raises(ValueError):
            M.resolve(dict(downsample=bad))
    for bad in ("812", 1.5, True):
        with pytest.raises(ValueError):
            M.resolve(dict(downsample="uniform", downsample_seed=bad))
    monkeypatch.setenv("NC_DOWNSAMPLE", "uniform")
    monkeypatch.setenv("NC_DOWNSAMPLE_SEED", "77")
    assert M.resolve({}) == ("uniform", 77)
    assert M.resolve(dict(downsample="first")) == ("first", 77)          # the keys win where they are present
    assert M.resolve(dict(downsample_seed=3)) == ("uniform", 3)
    monkeypatch.setenv("NC_DOWNSAMPLE", "sometimes")
    with pytest.raises(ValueError):
        M.resolve({})
    monkeypatch.delenv("NC_DOWNSAMPLE")
    assert M.for_pack({}, None, "c") is None and M.for_pack(dict(downsample="uniform"), None, "c") == ("uniform", 77)
    with pytest.raises(ValueError, match="share read names"):
        M.for_pack(dict(downsample="uniform"), (object(), object()), "c")
    assert M.for_pack(dict(downsample="first"), (object(), object()), "c") is None


def test_routes_without_a_sample_raise(tmp_path):
    """the host-assembled and per-chunk indel routes, the Python rules and an external aligner cut at the first maxcov reads: with 'uniform' they
    raise before any work; without the key they are what they were"""
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd import indelCaller
    dct = dict(downsample="uniform", impute_indel_phase=False)
    chunks = [dict(chrom="c", start=1, end=100, sam_path="x.bam")]
    with pytest.raises(ValueError, match="uniform"):
        gip.plan_routes(dct, chunks, False, route="host")
    with pytest.raises(ValueError, match="uniform"):
        gip.plan_routes(dct, [dict(chunks[0], sam_path=object())], False)                    # not a BAM path: the host-assembled route
    with pytest.raises(ValueError, match="uniform"):
        gip.get_indel_testing_candidates(dct, chunks[0])
    from nanocaller_amd.generate_indel_pileups_haploid import get_indel_testing_candidates_haploid
    with pytest.raises(ValueError, match="uniform"):
        get_indel_testing_candidates_haploid(dct, chunks[0])
    assert gip.plan_routes(dct, chunks, False) == [("device", [0], dct)]
    assert gip.plan_routes(dict(impute_indel_phase=False), chunks, False, route="host")[0][0] == "host"
    params = dict(dct, intermediate_indel_files_dir=str(tmp_path), prefix="p", indel_model="ONT-HG002")
    for kw in (dict(rules="python"), dict(aligner=lambda names, seqs, ref: None)):
        with pytest.raises(ValueError, match="uniform"):
            indelCaller.indel_run(params, {}, None, None, [], **kw)
    with pytest.raises(ValueError, match="downsample"):
        indelCaller.indel_run(dict(params, downsample="sometimes"), {}, None, None, [])


# ---------------------------------------------------------------------------------------------------------------- the indel tests' anchors are sharp
@pytest.mark.parametrize("maxcov", D.INDEL_MAXCOVS)
def test_indel_world_offers_sharp_anchors_of_every_kind(maxcov):
    cl = D.indel_classes("dip", maxcov)
    per_set = {s: sum(1 for _, c in cl if c[s] == "sharp") for s in (0, 1, 2)}
    kinds = {k: 0 for k in ("hp1", "hp2", "all_only", "all_three")}
    for _, c in cl:
        d1, d2, da = c[1] != "whole", c[2] != "whole", c[0] != "whole"
        assert da or not (d1 or d2)                                  # the `all` set holds both haplotype sets
        kinds["all_three"] += d1 and d2
        kinds["hp1"] += d1 and not d2
        kinds["hp2"] += d2 and not d1
        kinds["all_only"] += da and not d1 and not d2
    sizes = [ids.size for an, _ in cl for _, ids in D.indel_sets("dip", an)]
    print("maxcov %d: %d kept anchors, sharp per set %r, kinds %r" % (maxcov, len(cl), per_set, kinds))
    assert all(v >= 10 for v in per_set.values())
    if maxcov == 8:
        assert all(v >= 1 for v in kinds.values())
        assert maxcov in sizes and maxcov + 1 in sizes                # n = maxcov and n = maxcov + 1
    else:
        assert kinds["all_three"] >= 10
    hp = D.indel_classes("hap", maxcov)
    assert sum(1 for _, c in hp if c[0] == "sharp") >= 10


def test_deep_indel_world_offers_samples_that_cross_a_step():
    cl = D.indel_classes("deep", 8)
    assert sum(1 for _, c in cl if all(v == "sharp" for v in c.values())) >= 10
    assert sum(1 for an, _ in cl if D.indel_spans_a_step("deep", an, 8)) >= 5

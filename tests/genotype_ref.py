"""The yardstick of known-sites calling ("Genotyping a given list of sites"), built from the CPU oracle alone.

The rule: generate_SNP_pileups.py:183 of the reference reads `v_pos>=start and v_pos<=end and dct['min_allele_freq']<=alt_freq`; with a list
S the last term becomes `(min_allele_freq <= alt_freq or v_pos in S)` (add mode) or `v_pos in S` (only mode).  Everything before that line
(depth >= mincov, an unmasked AGTC reference base outside the excluded intervals) and after it (neighbours, tensors, depth) is unchanged, so the
expected tuple is the oracle's featuriser run on an explicit candidate list:

    E = oracle.snp_scan(..., min_allele_freq=0.0)        every eligible column of the chunk (alt_freq >= 0 always holds), with its counts
    N = oracle.snp_scan(..., dct['min_allele_freq'])     the natural candidates, and the neighbour list (independent of min_allele_freq)
    cpos = N u (S n E), or S n E in only mode

tests/test_genotype_ref.py checks this construction on the CPU; tests/test_genotype_gpu.py compares the HIP path with it.
"""
import numpy as np

from oracle import oracle
from tests.util import load_snp_case

EMPTY = ([], [], [], [], [], 0, [], [])

# the golden cases the GPU tests run (add and only mode each); the last one is ont_dip with mincov raised to the median depth of its region, so that
# the lists also hold positions that fail the depth test
GPU_CASES = ["ont_dip", "ont_dip_start", "ont_dip_end", "deep_ont", "hifi_pacbio_hap", "ont_exclude", "ont_mates", "ont_dip@mincov"]

CLASSES = ("zero_alt", "below_af", "natural", "below_mincov", "masked_ref", "excluded", "outside")


def load_case(case):
    """load_snp_case + the `@mincov` variant -> (world, dct, region, exclude)"""
    name, _, var = case.partition("@")
    world, dct, region, exclude, _ = load_snp_case(name)
    if var == "mincov":
        rc = oracle.ref_codes_with_exclusions(world, exclude)
        n = oracle.snp_scan(world, rc, region["start"], region["end"], region["ploidy"], dct["mincov"], 0.0, dct["threshold"], dct["supplementary"])[2]
        dct = dict(dct, mincov=int(np.median(n)))
    return world, dct, region, exclude


def scans(world, dct, region, exclude):
    """-> (rc, nbr, N, E, En, Ealt)"""
    rc = oracle.ref_codes_with_exclusions(world, exclude)
    a = (world, rc, region["start"], region["end"], region["ploidy"], dct["mincov"])
    _, E, En, Ealt = oracle.snp_scan(*a, 0.0, dct["threshold"], dct.get("supplementary", False))
    nbr, N, _, _ = oracle.snp_scan(*a, dct["min_allele_freq"], dct["threshold"], dct.get("supplementary", False))
    return rc, nbr, N, E, En, Ealt


def expected(world, dct, region, exclude, sites, only):
    """the reference's 8-tuple (pos, ref_onehot, mat, dp, freq, depth, fwd_dp, rev_dp) with the list `sites`"""
    rc, nbr, N, E, En, Ealt = scans(world, dct, region, exclude)
    S = np.unique(np.asarray(sites, np.int64)) if len(sites) else np.zeros(0, np.int64)
    SE = np.intersect1d(S, E)
    cpos = (SE if only else np.union1d(N, SE)).astype(np.int32)
    if cpos.size == 0:
        return EMPTY
    pos, ref, mat, fwd, rev, dep = oracle.snp_featurize(world, rc, nbr, cpos, dct["seq"], dct["maxcov"], dct["min_nbr_sites"], dct.get("supplementary", False))
    if pos.size == 0:
        return EMPTY
    sel = np.searchsorted(E, pos)
    assert np.array_equal(E[sel], pos)
    n, alt = En[sel].astype(np.int64), Ealt[sel]
    return (pos.astype(np.int64), np.eye(4, dtype=np.int32)[ref], mat, n, alt.astype(np.float64) / n.astype(np.float64),
            float(np.mean(dep.astype(np.float64))), fwd.astype(np.float64), rev.astype(np.float64))


def site_classes(world, dct, region, exclude):
    """{class: positions} of a case: what a listed position can be"""
    from nanocaller_amd.synth import world_ref_codes
    rc, nbr, N, E, En, Ealt = scans(world, dct, region, exclude)
    rc0 = world_ref_codes(world)
    lo, hi = max(1, region["start"]), min(region["end"], world.length)
    inside = np.arange(lo, hi + 1)
    not_e = np.setdiff1d(inside, E)
    freq = Ealt.astype(np.float64) / En.astype(np.float64)
    return dict(zero_alt=E[Ealt == 0], below_af=E[(Ealt > 0) & (freq < dct["min_allele_freq"])], natural=N,
                below_mincov=not_e[rc[not_e - 1] < 4], masked_ref=not_e[rc0[not_e - 1] >= 4],
                excluded=not_e[(rc0[not_e - 1] < 4) & (rc[not_e - 1] >= 4)],
                outside=np.array([p for p in (lo - 1, lo - 7, lo - 40_000, hi + 1, hi + 9, hi + 40_000, hi + 60_000) if p >= 1 and not lo <= p <= hi], np.int64))


_lists = {}


def site_list(case, per_class=24):
    """the list the tests use for `case`: up to per_class positions of every class, spread over the region with its first and last members,
    shuffled, a tenth of them twice (int64 array; deterministic)"""
    if case not in _lists:
        world, dct, region, exclude = load_case(case)
        parts = []
        for name, p in site_classes(world, dct, region, exclude).items():
            if len(p):
                parts.append(np.asarray(p, np.int64)[np.unique(np.linspace(0, len(p) - 1, min(per_class, len(p))).astype(np.int64))])
        s = np.concatenate(parts)
        rng = np.random.Generator(np.random.PCG64(len(case) + int(s.sum() % 1000)))
        s = np.concatenate([s, s[::10]])
        rng.shuffle(s)
        _lists[case] = s
    return _lists[case]


_expected = {}


def expected_for(case, only):
    """expected() of `case` with site_list(case), computed once (callers must not modify it)"""
    if (case, only) not in _expected:
        world, dct, region, exclude = load_case(case)
        _expected[case, only] = expected(world, dct, region, exclude, site_list(case), only)
    return _expected[case, only]


def as_gold(t):
    """an 8-tuple in the dict form assert_tuple_matches_gold compares against"""
    pos, ref, mat, dp, freq, depth, fwd, rev = t
    return dict(pos=np.asarray(pos), ref=np.asarray(ref), mat=np.asarray(mat, np.float32), dp=np.asarray(dp), freq=np.asarray(freq), depth=float(depth),
                fwd_dp=np.asarray(fwd), rev_dp=np.asarray(rev))

"""The yardstick of listed neighbour sites and background sampling, built from the CPU oracle alone.

Neighbours.  generate_SNP_pileups.py:173 / :177 of the reference make a column a neighbour site by its allele frequency; with a list L the test
reads `frequency rule or v_pos in L` (add mode) or `v_pos in L` (only mode).  Everything before it stays (an unmasked AGTC reference base outside
the excluded intervals, depth >= mincov, inside the scan window), so with

    EN  = oracle.snp_scan(..., "haploid", mincov, 2.0, [0.0, 1.0])[0]     every column of the scan window that passes those tests
    nbr = oracle.snp_scan(..., dct['threshold'])[0]                       the frequency rule's neighbours

the expected list is nbr u (L n EN), or L n EN in only mode, and the expected tuple is the oracle's featuriser run on it.  The candidates are
untouched: a listed neighbour is no candidate because of it.  In only mode min_nbr_sites counts the listed neighbours in reach, not the site's own
column as :244 does: the oracle's featuriser, which restates :244, is asked for min_nbr_sites + 1 columns.  With no position listed for the
contig the tuple is therefore empty at min_nbr_sites = 1.

Sampling.  A column that passes the same tests and fails the candidate test is a candidate all the same when mix(p, seed) < thr[b],
b = min(5, (20 * alt) // n), thr = floor(keep * 2^32): restated here in numpy over the columns (E, En, Ealt) of genotype_ref.scans.

tests/test_neighbor_ref.py checks these constructions on the CPU; tests/test_neighbor_gpu.py compares the HIP path with them.
"""
import numpy as np

from oracle import oracle
from tests import genotype_ref as G

EMPTY = G.EMPTY


def eligible_neighbors(world, dct, region, exclude):
    """EN: every column of the scan window that passes the tests in front of the neighbour rule (the haploid rule with t0 = 0 takes them all)"""
    rc = oracle.ref_codes_with_exclusions(world, exclude)
    return oracle.snp_scan(world, rc, region["start"], region["end"], "haploid", dct["mincov"], 2.0, [0.0, 1.0], dct.get("supplementary", False))[0]


def expected_neighbors(nbr, EN, listed, only, intersect=True):
    """nbr u (L n EN), or L n EN in only mode (intersect=False: the deliberate mistake of taking L as it is)"""
    L = np.unique(np.asarray(listed, np.int64)) if len(listed) else np.zeros(0, np.int64)
    LE = np.intersect1d(L, EN) if intersect else L[(L >= 1) & (L <= np.iinfo(np.int32).max)]
    return (LE if only else np.union1d(nbr, LE)).astype(np.int32)


def expected(world, dct, region, exclude, listed, only, *, sites=None, sites_only=False, intersect=True, as_candidates=False):
    """the reference's 8-tuple with the neighbour list `listed` (and, optionally, a list of positions to genotype).  intersect=False and
    as_candidates=True are the deliberate mistakes tests/test_neighbor_ref.py proves the yardstick sharp against."""
    rc, nbr, N, E, En, Ealt = G.scans(world, dct, region, exclude)
    EN = eligible_neighbors(world, dct, region, exclude)
    nbr2 = expected_neighbors(nbr, EN, listed, only, intersect)
    S = np.unique(np.asarray(sites, np.int64)) if sites is not None and len(sites) else np.zeros(0, np.int64)
    if as_candidates:
        S = np.union1d(S, np.asarray(listed, np.int64))
    SE = np.intersect1d(S, E)
    cpos = (SE if sites_only else np.union1d(N, SE)).astype(np.int32)
    if cpos.size == 0:
        return EMPTY
    min_cols = dct["min_nbr_sites"] + (1 if only else 0)               # (:244 counts the site's own column; only mode counts neighbours)
    pos, ref, mat, fwd, rev, dep = oracle.snp_featurize(world, rc, nbr2, cpos, dct["seq"], dct["maxcov"], min_cols, dct.get("supplementary", False))
    if pos.size == 0:
        return EMPTY
    sel = np.searchsorted(E, pos)
    assert np.array_equal(E[sel], pos)
    n, alt = En[sel].astype(np.int64), Ealt[sel]
    return (pos.astype(np.int64), np.eye(4, dtype=np.int32)[ref], mat, n, alt.astype(np.float64) / n.astype(np.float64),
            float(np.mean(dep.astype(np.float64))), fwd.astype(np.float64), rev.astype(np.float64))


_expected = {}


def expected_for(case, only):
    """expected() of `case` with genotype_ref.site_list(case) as the neighbour list, computed once (callers must not modify it)"""
    if (case, only) not in _expected:
        world, dct, region, exclude = G.load_case(case)
        _expected[case, only] = expected(world, dct, region, exclude, G.site_list(case), only)
    return _expected[case, only]


# ------------------------------------------------------------------ sampling
def mix(p, seed):
    """the 32-bit mixer over an array of 1-based positions (uint32 arithmetic, wrapping)"""
    with np.errstate(over="ignore"):
        x = (np.asarray(p).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32) * np.uint32(0x9E3779B1) ^ np.uint32(seed & 0xFFFFFFFF)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    return x


def mix_int(p, seed):
    """the same for one position, in Python integers"""
    M = 0xFFFFFFFF
    x = ((p & M) * 0x9E3779B1 & M) ^ (seed & M)
    x ^= x >> 16
    x = x * 0x85EBCA6B & M
    x ^= x >> 13
    x = x * 0xC2B2AE35 & M
    x ^= x >> 16
    return x


def bins(n, alt):
    """b = min(5, (20 * alt) // n)"""
    return np.minimum(5, (20 * np.asarray(alt, np.int64)) // np.asarray(n, np.int64))


def thresholds(keep):
    """probabilities in [0, 1) -> floor(keep * 2^32), exact in Python integers (a double times a power of two is exact)"""
    return np.array([int(float(k) * 4294967296.0) for k in keep], np.uint64)


def sampled(E, En, Ealt, is_candidate, seed, keep):
    """mask over the eligible columns E: the columns background sampling adds (is_candidate: mask of those that pass the candidate test)"""
    thr = thresholds(keep)[bins(En, Ealt)]
    return ~np.asarray(is_candidate, bool) & (mix(E, seed).astype(np.uint64) < thr)


def expected_sampled_scan(E, En, Ealt, min_allele_freq, seed, keep, sites=None):
    """(pos, dp, alt) of a scan with sample=(seed, keep) and, optionally, a list of positions to genotype in add mode"""
    cand = Ealt.astype(np.float64) / En.astype(np.float64) >= min_allele_freq
    if sites is not None:
        cand |= np.isin(E, np.asarray(sites, np.int64))
    k = cand | sampled(E, En, Ealt, cand, seed, keep)
    return E[k], En[k], Ealt[k]

"""CPU-only: the yardstick of listed neighbour sites and background sampling (tests/neighbor_ref.py) is sharp, and the parser of a
neighbour-sites VCF (genotype_sites.neighbor_sites_for) takes the records the reference's training generator takes."""
import gzip

import numpy as np
import pytest

from oracle import oracle
from tests import genotype_ref as G
from tests import neighbor_ref as R
from tests.util import load_world

CASES = ["ont_dip", "ont_exclude", "ont_dip@mincov"]


def _same(a, b):
    if len(a[0]) != len(b[0]):
        return False
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES)
def test_an_empty_list_gives_the_plain_oracle_tuple(case):
    world, dct, region, exclude = G.load_case(case)
    plain = oracle.get_snp_testing_candidates(world, dct, region, exclude)
    assert len(plain[0]) > 20
    assert _same(R.expected(world, dct, region, exclude, [], False), plain)
    assert _same(R.expected(world, dct, region, exclude, np.zeros(0, np.int64), False), plain)


@pytest.mark.parametrize("case", CASES)
def test_a_list_changes_the_tensors_of_many_sites(case):
    """24 positions of every class as neighbours, add mode: same sites, more than 20 of them with another tensor"""
    world, dct, region, exclude = G.load_case(case)
    plain = oracle.get_snp_testing_candidates(world, dct, region, exclude)
    exp = R.expected_for(case, False)
    assert np.array_equal(exp[0], plain[0]) and np.array_equal(exp[3], plain[3])              # a listed neighbour is no candidate because of it
    changed = np.any(np.asarray(exp[2]) != np.asarray(plain[2]), axis=(1, 2, 3))
    print("%s: %d of %d sites change their tensor" % (case, int(changed.sum()), len(changed)))
    assert changed.sum() > 20


def test_each_deliberate_mistake_changes_the_expected_tuple():
    """the list not intersected with EN (the excluded, masked_ref and below_mincov classes become neighbours), only mode computed as add mode,
    listed neighbours made candidates too: each differs from the yardstick on at least one of the three cases"""
    hit = dict(not_intersected=0, only_as_add=0, as_candidates=0)
    for case in CASES:
        world, dct, region, exclude = G.load_case(case)
        lst = G.site_list(case)
        add, only = R.expected_for(case, False), R.expected_for(case, True)
        hit["not_intersected"] += not _same(R.expected(world, dct, region, exclude, lst, False, intersect=False), add)
        hit["only_as_add"] += not _same(add, only)
        hit["as_candidates"] += not _same(R.expected(world, dct, region, exclude, lst, False, as_candidates=True), add)
    print(hit)
    assert all(v >= 1 for v in hit.values()), hit


def test_numpy_mix_equals_the_integer_restatement():
    rng = np.random.Generator(np.random.PCG64(3))
    p = np.concatenate([np.arange(1, 5001), rng.integers(1, np.iinfo(np.int32).max, 4998), [np.iinfo(np.int32).max, 1 << 30]])
    assert p.size == 10_000
    for seed in (0, 1, 0x9E3779B1, 0xFFFFFFFF):
        assert R.mix(p, seed).tolist() == [R.mix_int(int(v), seed) for v in p]
    assert R.mix_int(1, 0) == R.mix(np.array([1]), 0)[0] and len(set(R.mix(p, 7).tolist())) > 9_990


def test_sampling_keeps_the_binomial_share_of_every_large_bin():
    """`ont` at mincov 4: 134,597 eligible columns, 81,285 / 44,916 / 5,834 / 1,371 / 450 / 741 per bin; keep = 0.01 in every bin"""
    world = load_world("ont")
    dct = dict(mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])
    region = dict(chrom=world.chrom, start=1, end=world.length, ploidy="diploid")
    rc, nbr, N, E, En, Ealt = G.scans(world, dct, region, None)
    assert np.array_equal(R.eligible_neighbors(world, dct, region, None), E)
    b = R.bins(En, Ealt)
    pop = np.bincount(b, minlength=6)
    assert pop.tolist() == [81_285, 44_916, 5_834, 1_371, 450, 741]
    # the integer bins are the reference's float comparisons 0.05 <= alt_freq < 0.10 and the rest
    f = Ealt.astype(np.float64) / En.astype(np.float64)
    assert np.array_equal(b, sum((f >= t).astype(np.int64) for t in (0.05, 0.10, 0.15, 0.20, 0.25)))
    for seed in (1, 2024):
        k = R.sampled(E, En, Ealt, np.zeros(E.size, bool), seed, [0.01] * 6)
        got = np.bincount(b[k], minlength=6)
        for g in range(3):
            mean, sd = 0.01 * pop[g], np.sqrt(pop[g] * 0.01 * 0.99)
            print("seed %d bin %d: kept %d, expected %.1f +- %.1f" % (seed, g, got[g], mean, sd))
            assert abs(got[g] - mean) < 5 * sd
    assert not R.sampled(E, En, Ealt, np.zeros(E.size, bool), 1, [0.0] * 6).any()
    only1 = R.sampled(E, En, Ealt, np.zeros(E.size, bool), 1, [0, 0.5, 0, 0, 0, 0])
    assert only1.sum() > 20_000 and np.all(b[only1] == 1)


HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
RECORDS = [                                           # (line after CHROM, taken)
    ("100\t.\tA\tG\t.\t.\t.\tGT\t0/1", True),
    ("110\t.\tA\tG\t.\t.\t.\tGT:DP\t1|0:30", True),
    ("120\t.\tA\tG\t.\t.\t.\tGT\t1/1", False),        # homozygous
    ("130\t.\tA\tG\t.\t.\t.\tGT\t0/0", False),
    ("140\t.\tC\tG,T\t.\t.\t.\tGT\t1/2", True),       # multi-allelic, two different single bases
    ("150\t.\tC\tG,T\t.\t.\t.\tGT\t2|2", False),
    ("160\t.\tC\tG,TA\t.\t.\t.\tGT\t1/2", False),     # one chosen allele is no single base
    ("165\t.\tC\tG,TA\t.\t.\t.\tGT\t0/1", True),      # ... the chosen ones are
    ("170\t.\tAC\tA\t.\t.\t.\tGT\t0/1", False),       # deletion
    ("180\t.\tA\tAC\t.\t.\t.\tGT\t0/1", False),       # insertion
    ("190\t.\tN\tG\t.\t.\t.\tGT\t0/1", False),        # REF not one of AGTC
    ("200\t.\tT\tG\t.\t.\t.\tGT\t./.", False),
    ("210\t.\tT\tG\t.\t.\t.\tGT\t0/3", False),        # allele index past the ALT list
    ("220\t.\tt\tg\t.\t.\t.\tDP:GT\t9:0|1", True),
    ("100\t.\tA\tG\t.\t.\t.\tGT\t0/1", True),         # a duplicate
]


def _vcf(tmp_path, name, with_samples=True, compress=None):
    lines = [HEADER + ("\tFORMAT\tS1" if with_samples else "")]
    for rec, _ in RECORDS:
        f = rec.split("\t")
        lines.append("chrT\t" + ("\t".join(f) if with_samples else "\t".join(f[:7])))
    lines.append("chrU\t5\t.\tA\tG\t.\t.\t." + ("\tGT\t0/1" if with_samples else ""))
    text = "\n".join(lines) + "\n"
    path = str(tmp_path / name)
    if compress == "gzip":
        with gzip.open(path, "wt") as f:
            f.write(text)
    elif compress == "bgzf":
        from nanocaller_amd import vcfio
        vcfio.bgzf_write(path, text.encode())
    else:
        with open(path, "w") as f:
            f.write(text)
    return path


def test_the_vcf_parser_takes_heterozygous_single_base_records(tmp_path, monkeypatch):
    """fails on the parent commit: genotype_sites has no neighbor_sites_for"""
    from nanocaller_amd.genotype_sites import neighbor_sites_for
    monkeypatch.delenv("NC_NEIGHBOR_SITES", raising=False)
    monkeypatch.delenv("NC_NEIGHBOR_ONLY", raising=False)
    want = sorted({int(r.split("\t")[0]) for r, ok in RECORDS if ok})
    assert want == [100, 110, 140, 165, 220]
    for name, comp in (("a.vcf", None), ("b.vcf.gz", "gzip"), ("c.vcf.gz", "bgzf")):
        path = _vcf(tmp_path, name, compress=comp)
        pos, only = neighbor_sites_for(dict(neighbor_sites=path), "chrT")
        assert pos.dtype == np.int32 and pos.tolist() == want and only is False
        pos, only = neighbor_sites_for(dict(neighbor_sites=path, neighbor_only=1), "chrU")
        assert pos.tolist() == [5] and only is True
        pos, only = neighbor_sites_for(dict(neighbor_sites=path, neighbor_only=True), "chrNone")               # an unknown contig: an empty list
        assert pos.size == 0 and only is True
    # no sample columns: every record with a single-base REF and one single-base ALT
    bare = _vcf(tmp_path, "d.vcf", with_samples=False)
    assert neighbor_sites_for(dict(neighbor_sites=bare), "chrT")[0].tolist() == [100, 110, 120, 130, 200, 210, 220]
    # the dict form, the environment, and no list at all
    pos, only = neighbor_sites_for(dict(neighbor_sites={"chrT": [7, 3, 3, 0, -2, 1 << 40]}), "chrT")
    assert pos.tolist() == [3, 7] and only is False
    assert neighbor_sites_for(dict(neighbor_sites={"chrT": [7]}), "chrU")[0].size == 0
    assert neighbor_sites_for({}, "chrT") == (None, False)
    monkeypatch.setenv("NC_NEIGHBOR_SITES", _vcf(tmp_path, "e.vcf"))
    monkeypatch.setenv("NC_NEIGHBOR_ONLY", "1")
    pos, only = neighbor_sites_for({}, "chrT")
    assert pos.tolist() == want and only is True
    assert neighbor_sites_for(dict(neighbor_sites=None), "chrT") == (None, False)                              # the key wins over the environment

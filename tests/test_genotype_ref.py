"""CPU-only: the yardstick of known-sites calling (tests/genotype_ref.py) is sound before the HIP path is compared with it
(tests/test_genotype_gpu.py), and the host half of the feature (the sites VCF, the counts) does what DESIGN.md says."""
import numpy as np
import pytest

from tests import genotype_ref as G
from tests.util import SNP_CASES, assert_tuple_matches_gold, load_snp_case


@pytest.mark.parametrize("case", SNP_CASES)
def test_empty_list_reproduces_the_reference_golden(case):
    """no list, add mode: cpos = N, dp / freq looked up in the scan with min_allele_freq = 0 -- the reference's own tuple, exact"""
    world, dct, region, exclude, gold = load_snp_case(case)
    assert_tuple_matches_gold(G.expected(world, dct, region, exclude, [], False), gold)
    assert G.expected(world, dct, region, exclude, [], True) == G.EMPTY               # only mode, nothing listed


@pytest.mark.parametrize("case", [c for c in G.GPU_CASES if "@" not in c])
def test_added_sites_leave_the_natural_sites_rows_bit_identical(case):
    """the listed non-candidates are extra rows; the rows of the natural candidates (tensor, reference base, dp, freq, strand depths) are the golden's
    bit for bit -- only the chunk's mean depth moves, as the reference averages over the chunk's sites"""
    gold = load_snp_case(case)[4]
    pos, ref, mat, dp, freq, depth, fwd, rev = G.expected_for(case, False)
    assert len(pos) > len(gold["pos"]) and np.all(np.diff(pos) > 0)
    sel = np.searchsorted(pos, gold["pos"])
    assert np.array_equal(pos[sel], gold["pos"])
    assert_tuple_matches_gold((pos[sel], ref[sel], mat[sel], dp[sel], freq[sel], gold["depth"], fwd[sel], rev[sel]), gold)
    extra = np.setdiff1d(np.arange(len(pos)), sel)
    assert np.all(freq[extra] < 0.15) and np.any(freq[extra] == 0.0)
    # only mode: exactly the listed eligible positions, the same rows
    opos, oref, omat, odp, ofreq, odepth, ofwd, orev = G.expected_for(case, True)
    s = np.unique(G.site_list(case))
    assert np.array_equal(opos, pos[np.isin(pos, s)]) and 0 < len(opos) < len(pos)
    k = np.searchsorted(pos, opos)
    assert np.array_equal(omat, mat[k]) and np.array_equal(odp, dp[k]) and np.array_equal(ofreq, freq[k]) and np.array_equal(ofwd, fwd[k])


def test_site_lists_hold_every_class_of_position():
    """an input cannot silently degrade: over the cases the GPU tests run, the lists hold positions with zero alternative reads, below
    min_allele_freq, natural candidates, below mincov, on a masked / non-AGTC reference base, inside an excluded interval and outside the
    region; every single list holds the first three and the last"""
    seen = {c: 0 for c in G.CLASSES}
    for case in G.GPU_CASES:
        world, dct, region, exclude = G.load_case(case)
        s = np.unique(G.site_list(case))
        assert len(s) < len(G.site_list(case)), "the list should hold duplicates"
        assert np.any(np.diff(G.site_list(case)) < 0), "the list should be unsorted"
        cl = G.site_classes(world, dct, region, exclude)
        n = {c: int(np.isin(s, cl[c]).sum()) for c in G.CLASSES}
        for c in ("zero_alt", "below_af", "natural", "outside"):
            assert n[c] > 0, (case, c)
        for c in G.CLASSES:
            seen[c] += n[c]
    assert all(v > 0 for v in seen.values()), seen


def test_sites_vcf_parsing_and_env_fallback(tmp_path, monkeypatch):
    """a one-base REF contributes its POS whatever its ALT; indel lines and short lines are skipped and counted; the file is parsed once per
    path; plain, gzipped and bgzipped files read the same; dct keys win over the environment"""
    import gzip
    from nanocaller_amd import genotype_sites as gs
    from nanocaller_amd import vcfio
    text = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
            "chr20\t500\t.\tA\tG\t.\t.\t.\nchr20\t100\t.\tC\t.\t.\t.\t.\nchr20\t500\t.\tA\tT\t.\t.\t.\nchr20\t700\t.\tAT\tA\t.\t.\t.\n"
            "chr21\t9\t.\tG\tGTT,C\t.\t.\t.\nchr21\t3\t.\tg\t<DEL>\t.\t.\t.\nbroken line\n")
    plain, gz, bgz = (str(tmp_path / n) for n in ("s.vcf", "s.gz.vcf.gz", "s.vcf.gz"))
    open(plain, "w").write(text)
    gzip.open(gz, "wt").write(text)
    vcfio.bgzf_write(bgz, text.encode())
    for p in (plain, gz, bgz):
        by, skipped = gs.parse_sites_vcf(p)
        assert sorted(by) == ["chr20", "chr21"] and by["chr20"].tolist() == [100, 500] and by["chr21"].tolist() == [3, 9] and skipped == 2
        assert by["chr20"].dtype == np.int32
    assert gs.load_sites_vcf(plain) is gs.load_sites_vcf(plain)
    monkeypatch.delenv("NC_GENOTYPE_SITES", raising=False)
    monkeypatch.delenv("NC_GENOTYPE_ONLY", raising=False)
    assert gs.sites_for({}, "chr20") == (None, False)
    assert gs.sites_for({"genotype_sites": None, "genotype_only": True}, "chr20") == (None, False)
    a, only = gs.sites_for({"genotype_sites": plain}, "chr20")
    assert a.tolist() == [100, 500] and only is False
    a, only = gs.sites_for({"genotype_sites": {"chr20": [7, 3, 7, 0, -4, 1 << 40]}, "genotype_only": 1}, "chr20")
    assert a.tolist() == [3, 7] and only is True
    a, only = gs.sites_for({"genotype_sites": {"chr20": [7]}}, "chrX")
    assert a.size == 0 and only is False
    monkeypatch.setenv("NC_GENOTYPE_SITES", bgz)
    monkeypatch.setenv("NC_GENOTYPE_ONLY", "1")
    a, only = gs.sites_for({}, "chr21")
    assert a.tolist() == [3, 9] and only is True
    assert gs.sites_for({"genotype_sites": None}, "chr21") == (None, False)           # the key, present, wins over the environment
    a, only = gs.sites_for({"genotype_only": False}, "chr21")
    assert a.tolist() == [3, 9] and only is False


def test_count_listed():
    from nanocaller_amd.genotype_sites import count_listed
    s = np.array([5, 10, 20, 30, 31, 99], np.int32)
    assert count_listed(None, [(1, 100)], [5]) == (0, 0)
    assert count_listed(s, [(10, 20), (20, 30)], [10, 20, 20, 44]) == (3, 2)          # a shared chunk end counts once
    assert count_listed(s, [(40, 90)], [5]) == (0, 0)

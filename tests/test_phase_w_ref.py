"""CPU: the weighted phasing model's restatement (tests/phase_w_ref.py) against a weighted brute-force MEC search, against the unit-cost
restatements (phase_ref, phase_gt_ref) where every weight is 1 and no read is refused, on a hand instance whose weighted and unit optima differ,
its quality lookup on hand-written CIGARs, and what the instances of the GPU comparison cover."""
import numpy as np

from phase_gt_ref import exhaustive_cost, phase_gt
from phase_ref import brute_force_mec, haplotag, phase, random_instance
from phase_w_ref import (brute_force_wmec, continuing, gpu_instances, hand_instance, haplotag_w, mec_cost_w, phase_w, qual_lookup,
                         random_weighted_instance, select_reads_w, unit_weights)


def _small(rng):
    n_sites, n_reads = int(rng.integers(2, 9)), int(rng.integers(1, 11))
    reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=0.2)
    weights, ok = random_weighted_instance(rng, reads)
    return np.arange(1, n_sites + 1, dtype=np.int32) * 10, reads, weights, ok, n_sites


def test_block_costs_equal_a_weighted_brute_force():
    rng = np.random.default_rng(11)
    for _ in range(40):
        pos, reads, weights, ok, n_sites = _small(rng)
        res = phase_w(pos, reads, weights, ok)
        assert not res["accepted"][ok == 0].any() and (res["side"][ok == 0] == -1).all()
        total = sum(b[3] for b in res["blocks"])
        assert total == brute_force_wmec(reads, weights, res["accepted"], n_sites)
        assert total == mec_cost_w(reads, weights, res)                  # the sides and haplotypes realise the cost


def test_genotype_aware_costs_equal_a_weighted_brute_force():
    rng = np.random.default_rng(12)
    for _ in range(30):
        pos, reads, weights, ok, n_sites = _small(rng)
        gt = rng.choice([0, 0, 1, 2], n_sites)
        G = int(rng.choice([1, 30, 100]))
        res = phase_w(pos, reads, weights, ok, site_gt=gt, G=G)
        inside = res["site_block"] >= 0                                  # (a site outside the blocks keeps its call and costs nothing)
        want = brute_force_wmec(reads, weights, res["accepted"], n_sites, np.where(inside, gt, 0), G)
        # outside the blocks no accepted read has an allele: a het call there costs 0 in the search as well
        assert sum(b[3] for b in res["blocks"]) == want
        assert np.array_equal(res["site_gt"][~inside], gt[~inside])


def test_unit_weights_without_a_floor_are_the_plain_restatements():
    rng = np.random.default_rng(13)
    for k in range(40):
        n_sites, n_reads = int(rng.integers(2, 30)), int(rng.integers(1, 40))
        reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=0.15, max_len=int(rng.integers(2, n_sites + 1)))
        pos = np.arange(1, n_sites + 1, dtype=np.int32) * 7
        max_cov = int(rng.choice([15, 6, 2]))
        groups = rng.integers(0, max(1, n_reads // 2), n_reads)
        u = unit_weights(reads)
        plain, got = phase(pos, reads, max_cov=max_cov), phase_w(pos, reads, u, max_cov=max_cov)
        for key in plain:
            assert np.array_equal(plain[key], got[key]) if key != "blocks" else plain[key] == got[key], key
        assert all(np.array_equal(a, b) for a, b in zip(haplotag(reads, groups, plain), haplotag_w(reads, u, groups, got)))
        gt, G = rng.choice([0, 0, 2], n_sites), int(rng.choice([1, 2, 3]))
        plain, got = phase_gt(pos, reads, gt, G=G, max_cov=max_cov), phase_w(pos, reads, u, site_gt=gt, G=G, max_cov=max_cov)
        for key in plain:
            assert np.array_equal(plain[key], got[key]) if key != "blocks" else plain[key] == got[key], key
        assert all(np.array_equal(a, b) for a, b in zip(haplotag(reads, groups, plain), haplotag_w(reads, u, groups, got)))
        if n_reads <= 10 and n_sites <= 8:
            assert sum(b[3] for b in got["blocks"]) == exhaustive_cost(reads, got["accepted"], n_sites, np.where(got["site_block"] >= 0, gt, 0), G)
            assert sum(b[3] for b in phase_w(pos, reads, u)["blocks"]) == brute_force_mec(reads, select_reads_w(reads, n_sites), n_sites)


def test_hand_instance_two_q40_reads_outvote_three_q5_reads():
    pos, reads, weights = hand_instance()
    unit, wtd = phase_w(pos, reads, unit_weights(reads)), phase_w(pos, reads, weights)
    assert unit["blocks"] == [(0, 2, 100, 2)] and wtd["blocks"] == [(0, 2, 100, 15)]
    assert np.array_equal(unit["side"], wtd["side"]) and len(set(unit["side"][:5])) == 1 and unit["side"][5] != unit["side"][0]
    # the allele the first haplotype (reads 0-4, allele 0 at site 0) carries at site 1
    first = lambda res: int(res["site_h"][1]) ^ int(res["site_h"][0])  # noqa: E731
    assert first(unit) == 1 and first(wtd) == 0
    assert brute_force_wmec(reads, weights, wtd["accepted"], 3) == 15 and brute_force_wmec(reads, unit_weights(reads), unit["accepted"], 3) == 2
    # a name made of reads 0 and 2 alone: tagged with the first haplotype by weight (40 + 40 + 40 - 5 ... > 0)
    hp, _ = haplotag_w(reads, weights, np.arange(8), wtd)
    assert (hp[:5] == hp[0]).all() and (hp[5:] == 3 - hp[0]).all()


def test_haplotag_sign_follows_the_weights():
    """one read, two phased sites it disagrees / agrees with: unit scores cancel (untagged), weights decide"""
    pos = np.array([10, 20], np.int32)
    reads = [[(0, 0), (1, 0)], [(0, 0), (1, 0)], [(0, 1), (1, 1)], [(0, 1), (1, 1)], [(0, 0), (1, 1)]]
    weights = [[30, 30]] * 4 + [[40, 3]]
    ok = np.array([1, 1, 1, 1, 0], np.uint8)                             # the mixed read is refused by the floor, and still tagged
    res = phase_w(pos, reads, weights, ok)
    assert res["side"][4] == -1 and res["blocks"][0][3] == 0
    hp, ps = haplotag_w(reads, weights, np.arange(5), res)
    assert hp[4] == hp[0] and ps[4] == 10
    hp1, _ = haplotag_w(reads, unit_weights(reads), np.arange(5), res)
    assert hp1[4] == 0


def test_quality_lookup_on_hand_written_cigars():
    q = list(range(10, 30))                                              # 20 query bases, qualities 10 .. 29
    # 3S 5M 2I 4M 3D 6M, first reference base at 100: M runs cover 100-104 (q 3-7), 105-108 (q 10-13), D 109-111, M 112-117 (q 14-19)
    cig = [("H", 7), ("S", 3), ("M", 5), ("I", 2), ("M", 4), ("D", 3), ("M", 6), ("H", 2)]
    sites = [99, 100, 104, 105, 108, 109, 111, 112, 117, 118]
    assert qual_lookup(100, cig, q, sites, default_weight=30) == [30, 13, 17, 20, 23, 23, 23, 24, 29, 30]
    assert qual_lookup(100, cig, q, sites, default_weight=30, w_max=20) == [30, 13, 17, 20, 20, 20, 20, 20, 20, 30]
    # a deletion right at the start: no query base before it
    assert qual_lookup(50, [("D", 2), ("M", 3)], [40, 41, 42], [50, 51, 52, 54]) == [30, 30, 40, 42]
    # behind a soft clip the last query base is the clip's last
    assert qual_lookup(50, [("S", 2), ("N", 2), ("M", 1)], [1, 2, 3], [50, 51, 52]) == [2, 2, 3]
    # absent qualities, and a record without sequence
    assert qual_lookup(100, cig, [0xff] * 20, sites, default_weight=7) == [7] * 10
    assert qual_lookup(100, cig, [], sites, default_weight=7) == [7] * 10
    # = and X are matches; P consumes nothing
    assert qual_lookup(5, [("=", 2), ("P", 4), ("X", 1), ("M", 1)], [9, 8, 7, 6], [5, 6, 7, 8]) == [9, 8, 7, 6]


def test_gpu_instances_cover_the_model():
    inst = gpu_instances()
    assert len(inst) == 51
    differ = zero = floor_only = full = small = two = 0
    for t in inst:
        res = phase_w(t["pos"], t["reads"], t["weights"], t["read_ok"], max_cov=t["max_cov"])
        unit = phase_w(t["pos"], t["reads"], unit_weights(t["reads"]), t["read_ok"], max_cov=t["max_cov"])
        assert np.array_equal(res["accepted"], unit["accepted"])         # (selection does not look at the weights)
        differ += int(not np.array_equal(res["site_h"], unit["site_h"]) or not np.array_equal(res["side"], unit["side"]))
        zero += sum(w == 0 for r in np.flatnonzero(res["accepted"]) for w in t["weights"][r])
        free = select_reads_w(t["reads"], t["n_sites"], None, t["max_cov"])
        floor_only += int((free & (t["read_ok"] == 0)).sum())
        cont = continuing(t["reads"], res)
        full += sum(n == 15 for n in cont)
        small += sum(n < 10 for n in cont)
        two += sum(l == f + 1 for f, l, _, _ in res["blocks"])
    assert differ >= 10 and zero >= 10 and floor_only >= 10 and full >= 2 and small >= 10 and two >= 1

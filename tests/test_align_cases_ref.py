"""The tie-heavy aligner cases of tests/align_cases.py on the CPU: the host C++ (nc_star_msa, nc_nw_cigar, nc_allele_prediction) against the
independent Python restatements and against what the reference's own allele_prediction returned for them, and the condition that keeps the
device tests of the same cases from being vacuous -- the cases do contain the ties they are there for."""
import collections
import json
import os

import numpy as np

from nanocaller_amd import _lib
from nanocaller_amd import generate_indel_pileups as gip
from oracle import oracle

import align_cases as ac
from util import GOLD

_memo = {}


def star_refs():
    """{call name: [(rows, reference row)] per set} by the pure-Python star alignment: computed once, shared, never changed"""
    if "star" not in _memo:
        _memo["star"] = {name: [oracle.star_msa_ref(rd, w, *ac.STAR) for rd, w in zip(c.sets, c.refs)] for name, c in ac.star_calls().items()}
    return _memo["star"]


def allele_gold():
    if "gold" not in _memo:
        _memo["gold"] = json.load(open(os.path.join(GOLD, "allele_prediction_ties.json")))["calls"]
    return _memo["gold"]


def test_the_generator_is_deterministic_and_covers_every_layout():
    assert tuple(ac.STAR) == tuple(_lib.STAR_SCORING)
    calls = ac.star_calls()
    assert list(calls) == [c + s for c in ac.CLASSES for s in ("", "_mix")]
    for name, c in calls.items():
        lo, hi = ac.BOUNDS[c.cls]
        lens = set(len(w) for w in c.refs)
        assert lo <= max(lens) <= hi and max(lens) == ac.CLASSES[c.cls][-1], name       # one layout class per call, chosen by its longest window
        if name.endswith("_mix"):
            assert set(range(1, 11)) <= lens
        else:
            assert lens == set(ac.CLASSES[c.cls]) and set(c.family) == set(ac.FAMILIES)
            sizes = set(len(rd) for rd in c.sets)
            assert {0, 1, 3, 5} <= sizes
            k = c.sets.index([])
            assert c.sets[k - 1] and c.sets[k + 1]                                      # an empty set between non-empty ones
        assert all(1 <= len(q) <= 1000 for rd in c.sets for q in rd)
        n_al = sum(len(rd) for rd in c.sets)
        assert n_al % 4, name                                                          # a last wave with dead 16-lane groups
    assert max(len(q) for rd in calls["cpl4"].sets for q in rd) == 1000
    assert any("N" in q for rd in calls["cpl17"].sets for q in rd)
    al = ac.allele_calls()
    assert list(al) == ["cpl4", "cpl8", "cpl11", "cpl17", "fb_empty", "fb_long", "fb_wide"]
    assert 200 < sum(len(v[0]) for v in al.values()) < 600
    assert max(len(a) for a in al["cpl17"][0]) == 1000 and max(len(r) for r in al["cpl17"][1]) == 272
    assert "" in al["fb_empty"][0] and max(len(a) for a in al["fb_long"][0]) > 1000 and max(len(r) for r in al["fb_wide"][1]) > 272
    # the same again in a fresh interpreter state: nothing depends on hash salting or call order
    ac._star = ac._allele = None
    again = ac.star_calls()
    assert all(again[k].sets == calls[k].sets and again[k].refs == calls[k].refs for k in calls) and ac.allele_calls() == al


def test_host_star_aligner_equals_the_restatement_on_every_case():
    n = 0
    for name, c in ac.star_calls().items():
        for s, (rd, w) in enumerate(zip(c.sets, c.refs)):
            rows, rr = gip.star_aligner(["r%d" % k for k in range(len(rd))], rd, w)
            erows, err = star_refs()[name][s]
            assert rr == err and rows == erows, (name, s, c.family[s])
            assert rr.replace("-", "") == w and all(r.replace("-", "") == q for r, q in zip(rows, rd))
            n += len(rd)
    assert n > 500


def test_host_nw_cigar_equals_the_restatement_on_every_pair():
    n = 0
    for name, (alts, refs, mrs) in ac.allele_calls().items():
        for a, r in zip(alts, refs):
            if len(a) * len(r) > 30_000:
                continue                      # (the longer pairs: the golden below was recorded with this very comparison made on every pair)
            got = gip.nw_cigar(a, r)
            assert got == oracle.nw_cigar_ref(a, r), (name, a, r)
            n += 1
    assert n > 150
    # the star scoring and the scorings whose gap opening equals its extension, on the short classes
    for sc in (ac.STAR, (9, 9, 20, -10), (0, 0, 100, -100)):
        for name in ("cpl4", "cpl4_mix"):
            c = ac.star_calls()[name]
            for rd, w in zip(c.sets, c.refs):
                for q in rd[:3]:
                    if len(q) <= 80:
                        assert gip.nw_cigar(q, w, *sc) == oracle.nw_cigar_ref(q, w, *sc), (sc, q, w)


def test_the_cases_contain_the_ties_they_are_there_for():
    """every pair of the homopolymer, tandem and run_in_flank families, and 90 % of the two_letter and disjoint pairs, has a cell on its optimal
    path that only the tie rule decides; every kind of tie occurs.  (Printed, not asserted: the share among uniform random AGTC pairs, as the
    device tests before these drew them.)"""
    share = collections.defaultdict(lambda: [0, 0])
    kinds = collections.Counter()
    for name, c in ac.star_calls().items():
        for rd, w, f in zip(c.sets, c.refs, c.family):
            for q in rd:
                t = ac.tie_cells_of_family(f, q, w)
                kinds.update({k: v for k, v in t.items() if v})
                share[f][0] += sum(t.values()) > 0
                share[f][1] += 1
                if f in ("homopolymer", "tandem", "run_in_flank"):
                    assert sum(t.values()) > 0, (name, f, q, w)
    for f in ("two_letter", "disjoint"):
        assert share[f][0] >= 0.9 * share[f][1] and share[f][1] > 50, (f, share[f])
    for name, (alts, refs, mrs) in ac.allele_calls().items():
        for a, r in zip(alts, refs):
            if a and len(a) * len(r) <= 120_000:
                kinds.update({k: v for k, v in ac.tie_cells(a, r, ac.NW, free_tail=False).items() if v})
    assert all(kinds[k] > 0 for k in ac.TIE_KINDS), dict(kinds)
    print("pairs with a tie on the optimal path:", {f: "%d / %d" % tuple(v) for f, v in share.items()}, "tie cells by kind:", dict(kinds))
    # the generator of test_device_star_alignment_equals_host_star_alignment, for comparison
    from test_indel_pass2 import _mutate
    rng = np.random.Generator(np.random.PCG64(909))
    n_tie = n_all = 0
    for s in range(30):
        n_ref = int(rng.integers(30, 170))
        ref = "".join("AGTC"[i] for i in rng.integers(0, 4, size=n_ref))
        for r in range(3):
            indels = [(int(rng.integers(2, n_ref - 8)), int(rng.choice([-9, -3, -1, 1, 2, 5, 12]))) for _ in range(int(rng.integers(0, 3)))]
            indels = [(p, ln) for k, (p, ln) in enumerate(indels) if all(abs(p - p2) > 14 for p2, _ in indels[:k])]
            q = _mutate(rng, ref, int(rng.integers(0, 6)), indels)
            t = ac.tie_cells(q, ref, ac.STAR, True)
            n_tie += sum(t.values()) > 0
            n_all += 1
    print("uniform random AGTC pairs with a tie on the optimal path: %d / %d" % (n_tie, n_all))


def test_tie_cells_on_hand_cases():
    t = ac.tie_cells("AAAA", "AAAAAA", ac.NW, free_tail=False)                  # a 2-base gap in a run: the diagonal equals E wherever the gap could go
    assert t["diag_e"] > 0 and t["h_f"] == 0 and t["end"] == 0
    assert sum(ac.tie_cells("AAAA", "AAAAAA", ac.STAR, free_tail=True).values()) == 0      # free tail: nothing to place
    assert ac.tie_cells("TTTT", "AAAA", ac.STAR, free_tail=True)["end"] == 1    # the far end of the last row scores what the far end of the last column does
    assert ac.tie_cells("ACGT", "ACGT", ac.STAR, True) == collections.Counter()
    t = ac.tie_cells("AAGAA", "AAAA", (5, 5, 20, -10), free_tail=False)
    assert t["f_open_ext"] == 0 and t["diag_e"] + t["h_f"] >= 0
    assert ac.tie_cells("AAGGAA", "AAAA", (5, 5, 20, -10), free_tail=False)["f_open_ext"] > 0      # opening == extension inside the 2-base gap
    # the path it walks is the restatement's, on some of the cases and under three scorings
    for sc in (ac.STAR, ac.NW, (7, 7, 20, -10)):
        for name in ("cpl4", "cpl4_mix"):
            c = ac.star_calls()[name]
            for rd, w in zip(c.sets, c.refs):
                for q in rd[:2]:
                    for ft, fn in ((True, oracle.nw_cigar_free_tail_ref), (False, oracle.nw_cigar_ref)):
                        if len(q) > 80:
                            continue
                        path = []
                        ac.tie_cells(q, w, sc, ft, path_out=path)
                        want = [op for op, cnt in fn(q, w, *sc) for _ in range(cnt)]
                        assert path[::-1] == want, (sc, ft, q, w)


def test_host_allele_prediction_equals_the_reference_on_the_tie_pairs():
    """tests/golden/allele_prediction_ties.json: the reference's unchanged allele_prediction over the oracle aligner on the pairs of
    align_cases.allele_calls() (oracle/tools/make_goldens.py allele_ties)"""
    gold = allele_gold()
    calls = ac.allele_calls()
    assert list(gold) == list(calls)
    n = n_indel = 0
    for name, (alts, refs, mrs) in calls.items():
        rows = gold[name]
        assert [r[:3] for r in rows] == [[a, r, m] for a, r, m in zip(alts, refs, mrs)], name          # the golden is of these very inputs
        keep = [k for k, r in enumerate(rows) if not (isinstance(r[3], str) and r[3].startswith("!"))]
        assert len(keep) == len(rows)                                                                  # the reference raised on none of them
        want = [(rows[k][3], rows[k][4]) for k in keep]
        assert gip.allele_prediction_batch(alts, refs, mrs) == want, name
        assert [gip.allele_prediction(a, r, m) for a, r, m in zip(alts[:20], refs[:20], mrs[:20])] == want[:20]
        n += len(rows)
        n_indel += sum(1 for w in want if w[0] is not None and len(w[0]) != len(w[1]))
    assert n > 250 and n_indel > 100

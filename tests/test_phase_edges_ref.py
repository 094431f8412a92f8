"""CPU: the instances of tests/phase_edges.py reach the edges they are built for, by the restatements alone -- the range family spreads by exactly
65,535 / 65,536 in its forms, its closed-form solve is the restatements' where those are affordable, the transition family holds every
(continuing, leaving) pair on interleaved slots in more than 256 blocks, and the long-operation records' expected weights (phase_w_ref.qual_lookup,
which walks operations) equal a base-by-base expansion of the CIGAR."""
import time

import numpy as np
import pytest

import phase_edges as E
from phase_gt_ref import phase_gt
from phase_ref import haplotag, phase
from phase_w_ref import haplotag_w, phase_w, qual_lookup


def _same(ref, want, keys):
    for k in keys:
        assert np.array_equal(ref[k], want[k]), k
    assert [tuple(int(v) for v in b) for b in ref["blocks"]] == want["blocks"]


@pytest.fixture(scope="module")
def members():
    return E.range_members()


def test_range_members_spread_by_the_edge_and_one_beyond(members):
    assert 704 * 93 + 63 == E.EDGE and E.W_COLUMNS == 705
    for name, (t, forms, want) in members.items():
        t0 = time.time()
        got = E.relative_spread(t["reads"], t["n_sites"], t["weights"], t["read_ok"], t["gt"], t["G"], forms=forms)
        print("%s: %d sites, spread %s, %.2f s" % (name, t["n_sites"], got, time.time() - t0))
        assert got == {f: want for f in forms}, name
        assert want == (E.EDGE + 1 if name.endswith("over") else E.EDGE)
        assert (t["gt"] == 0).all() and t["G"] == E.G_MAX and t["read_ok"].all()
    # the genotype-aware forms' homozygous outcomes do not cap the split state: with a small price the same reads spread far less
    t = members["weighted-edge"][0]
    assert E.relative_spread(t["reads"], t["n_sites"], t["weights"], t["read_ok"], t["gt"], 30, forms=("GW",))["GW"] < E.EDGE // 2


def test_two_reads_closed_form_is_the_restatements_solve(members):
    """weighted: the member at the edge itself; unit costs: the 4,000-column member of the family (the restatements need ~20 s for 65,535)"""
    t = members["weighted-edge"][0]
    want, hp, ps = E.two_reads_closed_form(t)
    keys = ("accepted", "side", "site_block", "site_h", "site_phased", "site_ps")
    for gt in (None, t["gt"]):
        ref = phase_w(t["pos"], t["reads"], t["weights"], t["read_ok"], site_gt=gt, G=t["G"])
        _same(ref, want, keys + (("site_gt",) if gt is not None else ()))
        got = haplotag_w(t["reads"], t["weights"], t["groups"], ref)
        assert np.array_equal(got[0], hp) and np.array_equal(got[1], ps)
    assert want["blocks"] == [(0, 704, int(t["pos"][0]), 0)]
    u = E.two_reads(4000)
    want, hp, ps = E.two_reads_closed_form(u)
    for ref, extra in ((phase(u["pos"], u["reads"]), ()), (phase_gt(u["pos"], u["reads"], u["gt"], G=u["G"]), ("site_gt",))):
        _same(ref, want, keys + extra)
        got = haplotag(u["reads"], u["groups"], ref)
        assert np.array_equal(got[0], hp) and np.array_equal(got[1], ps)
    assert E.relative_spread(u["reads"], 4000, None, None, u["gt"], u["G"], forms=("ff", "Gf")) == {"ff": 4000, "Gf": 4000}


def test_fifteen_reads_reach_the_edge_in_a_state_of_both_table_halves(members):
    t = members["fifteen-edge"][0]
    for gt in (None, t["gt"]):
        d = E.spread_walk(t["reads"], t["n_sites"], t["weights"], t["read_ok"], gt, t["G"])
        ref = phase_w(t["pos"], t["reads"], t["weights"], t["read_ok"], site_gt=gt, G=t["G"])          # the expectation: no brute force over 2^15
        assert d["spread"] == E.EDGE and d["site"] == t["n_sites"] - 1                 # reached in the last column only
        assert d["state"] & 0xFF and d["state"] >> 8                                   # slots 0-7 and slots 8-14
        assert d["totals"] == [b[3] for b in ref["blocks"]]                            # the helper's recurrence is the restatement's
        acc, blocks = E.block_columns(t["reads"], t["n_sites"], t["weights"], t["read_ok"])
        assert acc.all() and len(blocks) == 1 and all(c[0] == 0x7FFF for c in blocks[0][1])
        assert ref["side"].any() and ref["site_h"].any() and not ref["site_h"].all() and ref["blocks"][0][3] > 0
        # the optimum is unique up to the exchange of the two sides: every other state of the last column costs more
        assert d["minima"] == [2]


@pytest.fixture(scope="module")
def transitions():
    return E.transition_instance()


def test_transition_family_holds_every_pair_on_interleaved_slots(transitions):
    t, specs = transitions
    acc, blocks = E.block_columns(t["reads"], t["n_sites"], t["weights"], t["read_ok"])
    assert acc.all() and len(blocks) == len(specs) > 256                 # none dropped by max_cov; more blocks than compute units
    seen, broken = set(), 0
    for (f, cols), (nk, nl, ne) in zip(blocks, specs):
        assert len(cols) == 4 and f % 5 == 0
        K, Lm = cols[2][1], cols[1][0] & ~cols[2][1]
        assert (bin(K).count("1"), bin(Lm).count("1")) == (nk, nl) and bin(cols[2][0]).count("1") == nk + ne
        assert cols[1][1] == cols[1][0] == cols[0][0] and cols[3][1] == cols[3][0]     # columns 1 and 3: everything continues
        seen.add((nk, nl))
        broken += not E.is_run(K) and not E.is_run(Lm)
    assert seen == set(E.transition_pairs()) and len(seen) == 120
    assert {(nk, nl) for nk in (9, 10, 11) for nl in (0, 1, 4)} <= seen
    assert 3 * broken >= len(blocks), broken
    g = t["groups"]
    block_of = np.array([rd[0][0] // 5 for rd in t["reads"]])
    two = [np.unique(block_of[g == k]).size for k in range(int(g.max()) + 1)]
    assert max(two) == 2 and sum(n == 2 for n in two) > 50               # names with reads in two blocks
    assert t["read_ok"].all() and set(t["gt"].tolist()) == {0, 2}


def test_transition_family_solves_in_the_restatements(transitions):
    t, _ = transitions
    t0 = time.time()
    ref = phase_w(t["pos"], t["reads"], t["weights"], t["read_ok"], site_gt=t["gt"], G=t["G"])
    t1 = time.time()
    d = E.spread_walk(t["reads"], t["n_sites"], t["weights"], t["read_ok"], t["gt"], t["G"])
    print("transition family: %d blocks, %d reads, phase_w %.2f s, spread_walk %.2f s, spread %d" % (len(ref["blocks"]), len(t["reads"]), t1 - t0,
                                                                                                      time.time() - t1, d["spread"]))
    assert d["totals"] == [b[3] for b in ref["blocks"]] and d["spread"] < E.EDGE
    assert ref["accepted"].all() and ref["site_phased"].sum() > 800 and (ref["site_gt"] != t["gt"]).sum() > 20
    plain = phase(t["pos"], t["reads"])
    assert E.spread_walk(t["reads"], t["n_sites"])["totals"] == [b[3] for b in plain["blocks"]]


# ------------------------------------------------------------------------------------------- records with long operations
def _by_base(r, sites, default_weight, w_max):
    """the lookup with the CIGAR expanded base by base: the query index of every reference base of the alignment"""
    s1, chunks, q = r["pos0"] + 1, [], 0
    for op, n in E.real_cigar(r):
        if op in "M=X":
            chunks.append(np.arange(q, q + n))
        elif op in "DN":
            chunks.append(np.full(n, q - 1))
        if op in "MIS=X":
            q += n
    qi = np.concatenate(chunks)
    out = []
    for sp in sites:
        k = sp - s1
        ok = 0 <= k < qi.size and 0 <= qi[k] < len(r["qual"]) and r["qual"][qi[k]] != 0xff
        out.append(min(r["qual"][qi[k]], w_max) if ok else default_weight)
    return out


def test_long_operation_records_reach_the_high_halves():
    recs = E.long_op_records()
    pos, reads = E.long_op_csr(recs)
    cig = E.long_op_cigars()
    assert len(recs) == 8 and (np.diff(pos) > 0).all() and pos[-1] < 2 ** 31 - 1
    assert cig["m70000"][0][1] >> 16 == 1
    pairs = [n for _, n in cig["pairs"]]
    assert len(pairs) == 192 and sum(pairs[:58]) < 65536 < sum(pairs[:60]) < sum(pairs[:64])     # the reference prefix crosses inside the chunk
    assert sum(pairs[0:58:2]) < 65536 < sum(pairs[0:60:2])                                      # the query prefix too (the M operations)
    assert cig["bigdel"][1] == ("D", 200_000_000) and len(cig["many700"]) == 151 and E.ref_span(cig["many700"]) > 3 * 65536
    for r, rd in zip(recs, reads):
        own = [int(pos[s]) for s, _ in rd]                                # its own sites and its twin's, 7 bases to one side
        a, b = r["pos0"] + 1, r["pos0"] + 1 + E.ref_span(E.real_cigar(r))
        assert {a - 1, a, b - 1, b, b + 1} <= E.long_op_sites(r) <= set(own) and min(own) < a
        inside = [p for p in own if a <= p < b]
        assert {(p - a) % 65536 for p in inside} >= {65535, 0, 1} and len(rd) >= 8
        if "CG" in r["tags"]:
            assert r["cigar"] == [("S", len(r["seq"])), ("N", b - a)] and len(r["tags"]["CG"]) == len(E.real_cigar(r))
        for dw, wm in ((30, 93), (7, 50)):
            want = qual_lookup(a, E.real_cigar(r), list(r["qual"]), own, dw, wm)
            if not r["name"].startswith("bigdel"):
                assert want == _by_base(r, own, dw, wm), r["name"]
            else:                                                        # every site of the deletion takes the 20th query base
                assert all(w == min(r["qual"][19], wm) for p, w in zip(own, want) if a + 20 <= p < b - 20)
                assert want[own.index(b - 1)] == min(r["qual"][39], wm) and sum(a + 20 <= p < b - 20 for p in own) >= 20
            assert all(w == dw for p, w in zip(own, want) if p < a or p >= b) and want[0] == dw and want[-1] == dw

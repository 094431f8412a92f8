"""CPU: the restatement of the realignment allele rule (tests/phase_realign_ref.py) on hand-built reads whose answer is known by
construction, the worlds the GPU tests use (the two rules must differ on them), and the switch that selects the rule."""
import numpy as np
import pytest

from phase_realign_ref import (QMAX, compare_rules, entries, het_site_alleles, levenshtein, make_realign_world, query_window, realign_allele,
                               ref_codes)

C = {"A": 0, "G": 1, "T": 2, "C": 3, "N": 4}
#      1        10        20        30        40        50        60
REF = "TCAGGCTAACGTCATGGACTTGCAGTCGATCCGTAAAAATCGGATGCACTGACCTAGGTCAT"
P = 30                                                                    # REF[29] = 'C'; alleles C / T
A0, A1 = C["C"], C["T"]


def _read(start, end, allele=None, p=P):
    """codes of a read that follows REF over [start, end) and carries `allele` at p"""
    c = [C[b] for b in REF[start - 1:end - 1]]
    if allele is not None:
        c[p - start] = allele
    return c


def _call(codes, events=(), start=5, end=58, p=P, a0=A0, a1=A1, ref=REF):
    return realign_allele(ref_codes(ref), p, a0, a1, start, end, codes, list(events))


def _column(codes, start=5, p=P, a0=A0, a1=A1):
    c = codes[p - start]
    return 0 if c == a0 else (1 if c == a1 else None)


def test_levenshtein_textbook_values():
    assert levenshtein("kitten", "sitting") == 3 and levenshtein("", "abc") == 3 and levenshtein("abc", "abc") == 0
    assert levenshtein("flaw", "lawn") == 2 and levenshtein("a", "") == 1


def test_clean_reads_take_their_allele():
    assert _call(_read(5, 58, A0)) == 0 and _call(_read(5, 58, A1)) == 1


def test_deletion_error_left_of_the_site_with_the_gap_placed_right():
    """the read lacks the base on column p - 1; the alignment keeps matching and opens the gap on column p + 2: columns p - 1 .. p + 1 hold the
    bases of p .. p + 2.  The column shows REF's base of p + 1 ('C', the first allele by chance); the read carries the second."""
    c = _read(5, 58, A1)
    c[P - 1 - 5:P + 2 - 5] = c[P - 5:P + 3 - 5]
    c[P + 2 - 5] = 4
    ev = [(P + 1, -1, [])]
    assert _column(c) == 0                                              # wrong
    assert query_window(c, 5, ev, P - 10, P + 10) == _read(5, 58, A1)[P - 10 - 5:P - 1 - 5] + _read(5, 58, A1)[P - 5:P + 11 - 5]
    assert _call(c, ev) == 1


def test_deletion_error_right_of_the_site_with_the_gap_placed_left():
    """the read lacks the base on column p + 1; the gap stands on column p - 2 and columns p - 1 .. p + 1 hold the bases of p - 2 .. p"""
    c = _read(5, 58, A1)
    c[P - 1 - 5:P + 2 - 5] = c[P - 2 - 5:P + 1 - 5]
    c[P - 2 - 5] = 4
    ev = [(P - 3, -1, [])]
    assert _column(c) is None                                           # column p shows 'G', the base of p - 1: neither allele
    assert _call(c, ev) == 1


def test_insertion_error_in_a_homopolymer_that_spans_the_site():
    """REF 35 .. 39 = AAAAA, site 37 with alleles A / G, and one base too many in the run, left-aligned in front of it as aligners do.
    A read that carries A shows six A's: one insertion from the A haplotype, two edits from the G haplotype -> allele 0.
    A read that carries G (A A G A A A) has its run's columns read A G A A A: column 37 shows A, the wrong allele.  The realignment cannot
    tell either: dropping the G gives the A haplotype, dropping an A the G haplotype, one edit each -> no entry (it abstains where the column
    rule votes for the wrong haplotype)."""
    p = 37
    assert REF[34:39] == "AAAAA"
    ev = [(34, 1, [C["A"]])]
    assert _call(_read(5, 58), ev, p=p, a0=C["A"], a1=C["G"]) == 0
    c = _read(5, 58)
    c[35 - 5:40 - 5] = [C[b] for b in "AGAAA"]
    assert _column(c, p=p, a0=C["A"], a1=C["G"]) == 0                   # wrong
    assert _call(c, ev, p=p, a0=C["A"], a1=C["G"]) is None
    assert levenshtein([C[b] for b in "AAGAAA"], [C[b] for b in "AAGAA"]) == 1 and levenshtein([C[b] for b in "AAGAAA"], [C[b] for b in "AAAAA"]) == 1


def test_read_that_ends_inside_the_window_has_no_entry():
    assert _call(_read(5, P + 10, A1), end=P + 10) is None              # last column P + 9
    assert _call(_read(5, P + 11, A1), end=P + 11) == 1
    assert _call(_read(P - 9, 58, A1), start=P - 9) is None
    assert _call(_read(P - 10, 58, A1), start=P - 10) == 1


def test_equal_distances_give_no_entry():
    assert _call(_read(5, 58, C["A"])) is None                          # a third base on the site's column
    c = _read(5, 58, A1)
    c[P - 5] = 4
    assert _call(c, [(P - 1, -1, [])]) is None                          # the site's own base deleted


def test_site_with_two_alternative_alleles():
    assert _call(_read(5, 58, C["T"]), a0=C["A"], a1=C["T"]) == 1 and _call(_read(5, 58, C["A"]), a0=C["A"], a1=C["T"]) == 0
    assert _call(_read(5, 58, C["C"]), a0=C["A"], a1=C["T"]) is None    # the REF base: as far from either


def test_site_three_bases_from_the_contig_end():
    L = len(REF)
    p = L - 3
    a0, a1 = C[REF[p - 1]], (C[REF[p - 1]] + 1) % 4
    assert _call(_read(20, L + 1, a1, p=p), start=20, end=L + 1, p=p, a0=a0, a1=a1) == 1       # the window is cut at L: 14 columns
    assert _call(_read(20, L, a1, p=p), start=20, end=L, p=p, a0=a0, a1=a1) is None            # the read stops one column short of it
    a0, a1 = C[REF[2]], (C[REF[2]] + 2) % 4
    assert _call(_read(1, 40, a1, p=3), start=1, end=40, p=3, a0=a0, a1=a1) == 1


def test_n_in_the_window_gives_no_entry_and_lower_case_does_not():
    ref = REF[:P + 6] + "N" + REF[P + 7:]
    assert _call(_read(5, 58, A1), ref=ref) is None
    ref = REF[:P - 8] + REF[P - 8:P + 8].lower() + REF[P + 8:]
    assert _call(_read(5, 58, A1), ref=ref) == 1


def test_query_window_longer_than_64_bases_gives_no_entry():
    c = _read(5, 58, A1)
    assert _call(c, [(P - 4, QMAX - 21, [0] * (QMAX - 21))]) == 1       # 21 + 43 = 64 bases
    assert _call(c, [(P - 4, QMAX - 20, [0] * (QMAX - 20))]) is None    # 65
    assert _call(c, [(P + 10, 60, [0] * 60)]) == 1                      # behind the window's last column: not part of it
    assert _call(c, [(P - 11, 60, [0] * 60)]) == 1                      # in front of its first column: not part of it


def test_worlds_of_the_gpu_tests_separate_the_two_rules():
    """on the planted worlds the rules differ in at least 1 % of the pairs, in both directions"""
    from nanocaller_amd.phase import kept_reads
    w = make_realign_world(11, length=60_000)
    kept = kept_reads(w, False)[0]
    pos, al = het_site_alleles(w, kept)
    col, rea = entries(w, kept, pos, al, "column"), entries(w, kept, pos, al, "realign")
    truth = []
    for r in kept.tolist():
        truth.append({int(np.searchsorted(pos, p)): (0 if c == al[np.searchsorted(pos, p), 0] else 1 if c == al[np.searchsorted(pos, p), 1] else None)
                      for p, c in w.meta["truth_allele"][r].items() if p in set(pos.tolist())})
    st = compare_rules(col, rea, truth)
    print(st)
    assert st["differ"] >= 0.01 * st["pairs"] and st["gained"] > 0 and st["corrected"] > 0


@pytest.mark.parametrize("key,env,want", [(None, None, False), (None, "1", True), (None, "0", False), (True, None, True), (False, "1", False),
                                          (1, "0", True), (0, "1", False)])
def test_phase_realign_selected(monkeypatch, key, env, want):
    from nanocaller_amd.phase import phase_realign_selected
    if env is None:
        monkeypatch.delenv("NC_PHASE_REALIGN", raising=False)
    else:
        monkeypatch.setenv("NC_PHASE_REALIGN", env)
    params = {} if key is None else {"phase_realign": key}
    assert phase_realign_selected(params) is want

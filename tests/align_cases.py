"""Tie-heavy inputs for every statement of the Gotoh aligner (CPU only, fixed seeds, no GPU code): homopolymers, tandem repeats, runs in a
random flank, two-letter sequences, read / window pairs that share nothing, and the shape edges, at the window lengths that sit on both sides of
every lane layout of the device kernels (nc_msa.hip: 4 / 8 / 11 / 17 columns per lane up to 64 / 128 / 176 / 272 reference bases, one lane per
read above).  A call holds windows of ONE layout class, so the kernel template under test is the one that runs.

  star_calls()    {name: StarCall}  read sets against their windows, for the star alignment (free tail, STAR scoring)
  allele_calls()  {name: (consensus list, window list, max_range list)}  for allele_prediction (global alignment, parasail's 9 / 1 / 20 / -10)
  tie_cells()     where on the optimal path the winning move only won by the tie rule

Under the free tail a pure run against a pure run has nothing to decide (the diagonal to the shorter string's end is the only optimum): the
homopolymer family's ties are those of its GLOBAL alignment, which has to place the gap -- see tie_cells_of_family."""
import collections

import numpy as np

STAR = (25, 1, 20, -10)            # _lib.STAR_SCORING
NW = (9, 1, 20, -10)               # parasail.nw_trace(alt, ref, 9, 1, matrix 20 / -10)

CLASSES = collections.OrderedDict([("cpl4", (1, 2, 3, 4, 5, 63, 64)), ("cpl8", (65, 127, 128)), ("cpl11", (129, 161, 175, 176)),
                                   ("cpl17", (177, 261, 271, 272)), ("lane", (273, 300))])
BOUNDS = {"cpl4": (1, 64), "cpl8": (65, 128), "cpl11": (129, 176), "cpl17": (177, 272), "lane": (273, 1000)}      # longest window of a call -> route
READS_PER_SET = {"cpl4": 12, "cpl8": 6, "cpl11": 3, "cpl17": 2, "lane": 2}       # the pure-Python restatement pays per cell: fewer reads on long windows
FAMILIES = ("homopolymer", "tandem", "run_in_flank", "two_letter", "disjoint", "shapes")
TIE_KINDS = ("e_open_ext", "f_open_ext", "diag_e", "h_f", "end")

StarCall = collections.namedtuple("StarCall", "cls sets refs family")


def _rng(*key):
    return np.random.Generator(np.random.PCG64([abs(hash_(k)) for k in key]))


def hash_(k):
    return k if isinstance(k, int) else sum((i + 1) * ord(c) for i, c in enumerate(k))       # not hash(): that one is salted per process


def _rand(rng, n, alphabet="AGTC"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def _mutate(rng, s, n_sub, indels, alphabet="AGTC"):
    """n_sub substitutions by another letter of `alphabet`, then indels [(position, +inserted / -deleted length)]"""
    q = list(s)
    for p in rng.choice(len(q), size=min(n_sub, len(q)), replace=False):
        q[p] = alphabet[(alphabet.index(q[p]) + int(rng.integers(1, len(alphabet)))) % len(alphabet)]
    for pos, ln in sorted(indels, reverse=True):
        if ln > 0:
            q[pos:pos] = list(_rand(rng, ln, alphabet))
        else:
            del q[pos:pos - ln]
    return "".join(q) or alphabet[0]


def _not(c, rng=None):
    return "AGTC"[("AGTC".index(c) + 1 + (int(rng.integers(0, 3)) if rng is not None else 0)) % 4]


# ------------------------------------------------------------------------------------------------------------------------ the families
def homopolymer(n, k, rng):
    x = "AGTC"[n % 4]
    ms = [m for m in range(n - 12, n + 13) if m >= 1 and m != n]
    pick = sorted(set(int(m) for m in rng.choice(ms, size=min(k - 1, len(ms)), replace=False)))
    reads = [x * m for m in pick]
    m = pick[0] if n < 3 else n + (-2 if n > 4 else 2)                      # the foreign base sits in a read that also needs a gap
    p = int(rng.integers(0, m))
    reads.append(x * p + _not(x) + x * (m - p - 1))
    return x * n, reads


def tandem(n, k, rng):
    """two repeat blocks of different units, a spacer between them and a random tail that anchors the end.  A whole unit lost or gained has as
    many places as the block has units; a partial unit or a phase shift has one place only (and would merge with a whole-unit indel of its
    own block into one net event), so a read with one of those in the first block carries a whole-unit indel in the second"""
    ua, ub = (2, 3, 5)[n % 3], (3, 5, 2)[n % 3]
    unit_a = "".join(rng.permutation(list("AGTC"))[:min(ua, 4)]) + ("" if ua < 5 else "AGTC"[int(rng.integers(0, 4))])
    unit_b = "".join(rng.permutation(list("AGTC"))[:min(ub, 4)]) + ("" if ub < 5 else "AGTC"[int(rng.integers(0, 4))])
    na = (n - 18) // 2
    nb = n - 18 - na
    A, B = (unit_a * (na // ua + 2))[:na], (unit_b * (nb // ub + 2))[:nb]
    sp, tail = _rand(rng, 6), _rand(rng, 12)
    if sp[0] == unit_a[na % ua]:
        sp = _not(sp[0]) + sp[1:]
    if tail[0] == unit_b[nb % ub]:
        tail = _not(tail[0]) + tail[1:]
    reads = []
    for r in range(k):
        kind = r % 6
        at = int(rng.integers(0, max(1, na // ua - 3))) * ua                # the same indel planted at another unit of the repeat
        bt = int(rng.integers(0, max(1, nb // ub - 1))) * ub
        b_lost, b_gained = B[:bt] + B[bt + ub:], B[:bt] + unit_b + B[bt:]
        if kind == 0:
            q = A[:at] + A[at + ua:] + sp + B                              # one whole unit lost
        elif kind == 1:
            q = A[:at] + unit_a + A[at:] + sp + B                          # one whole unit gained
        elif kind == 2:
            q = A[:at + 1] + A[at + ua:] + sp + b_lost                     # a partial unit lost (ua - 1 bases)
        elif kind == 3:
            q = A[:at] + unit_a[:ua - 1] + A[at:] + sp + b_gained          # a partial unit gained
        elif kind == 4:
            q = A[1:] + unit_a[na % ua] + sp + b_lost                      # the repeat phase-shifted (ACACAC against CACACA)
        else:
            c = int(rng.integers(2, 4))
            q = (A[:at] + A[at + c * ua:] if r % 12 == 5 else A[:at] + unit_a * c + A[at:]) + sp + B       # several units at once
        reads.append(q + tail)
    return A + sp + B + tail, reads


def run_in_flank(n, k, rng):
    r = int(rng.integers(6, min(30, n - 24) + 1))
    x = "AGTC"[int(rng.integers(0, 4))]
    right = n - r - int(rng.integers(3, n - r - 12))
    left = n - r - right
    fl, fr = _rand(rng, left), _rand(rng, right)
    fl = fl[:-1] + _not(x, rng)
    fr = _not(x, rng) + fr[1:]
    reads = []
    for _ in range(k):
        d = int(rng.integers(1, 10)) * (1 if rng.random() < 0.5 else -1)
        d = max(d, 1 - r)
        q = fl + x * (r + d) + fr
        reads.append(_mutate(rng, q, int(rng.integers(0, 2)) if left > 6 else 0, []) if rng.random() < 0.3 and left > 6 else q)
        if reads[-1][left - 1:left + r + d + 1] != q[left - 1:left + r + d + 1]:      # a substitution must not touch the run or its borders
            reads[-1] = q
    return fl + x * r + fr, reads


def two_letter(n, k, rng):
    win = _rand(rng, n, "AG")
    reads = []
    for _ in range(k):
        # the indels sit in the first two thirds: what follows anchors them, so the alignment has to place each gap
        indels = [(int(rng.integers(1, 2 * n // 3)), int(rng.choice([-9, -3, -2, -1, 1, 2, 4, 11]))) for _ in range(int(rng.integers(2, 4)))]
        q = _mutate(rng, win, int(rng.integers(0, 3)), indels, "AG")
        reads.append(q[:int(rng.integers(max(5, len(q) - 5), len(q) + 1))])
    return win, reads


def disjoint(n, k, rng):
    """nothing matches: the best path is one gap along an edge, and the free tail ends at the far end of the last row or of the last column,
    whichever string is shorter -- a read as long as the window scores the same at both (the last row wins)"""
    lens = [n if rng.random() < 0.94 else max(1, n + int(rng.integers(-12, 13))) for _ in range(k)]
    return _rand(rng, n, "AG"), [_rand(rng, m, "TC") for m in lens]


def tiny(n, k, rng):
    """windows of 1 - 5 bases (shorter than one lane's columns, or than two lanes'): every family shrinks to this"""
    win = _rand(rng, n, "AG" if n % 2 else "AGTC")
    reads = [_rand(rng, int(rng.integers(1, n + 13)), "AG") for _ in range(k - 3)]
    return win, reads + [win, win[0] * (n + 2), _rand(rng, n + 3, "TC")]


def shapes(n, rng):
    """-> [(window, reads)]: sets of 1, 3 and 5 reads with an empty set between them"""
    win = _rand(rng, n)
    longer = [win + _rand(rng, int(t)) for t in (1, int(rng.integers(2, 40)), 40)]
    with_n = [_mutate(rng, win, 2, [(n // 2, -2)])[:n - 1] for _ in range(5)]
    for r, q in enumerate(with_n[:4]):
        p = sorted(int(t) for t in rng.choice(len(q), size=r + 1, replace=False))
        with_n[r] = "".join("N" if i in p else c for i, c in enumerate(q))
    return [(win, [win]), (win, []), (win, [win[n // 3:n // 3 + 1], win[:5], _rand(rng, 5)]), (_rand(rng, n), []), (win, with_n),
            (win, longer)]


_FAMILY_FN = {"homopolymer": homopolymer, "tandem": tandem, "run_in_flank": run_in_flank, "two_letter": two_letter, "disjoint": disjoint}


def _family_sets(cls):
    sets, refs, fam = [], [], []
    for n in CLASSES[cls]:
        if n <= 5:
            w, rd = tiny(n, READS_PER_SET[cls], _rng("tiny", n))
            sets.append(rd); refs.append(w); fam.append("shapes")
            continue
        for f in FAMILIES[:5]:
            k = READS_PER_SET[cls]
            if cls in ("cpl11", "cpl17", "lane") and n != BOUNDS[cls][0] and n != BOUNDS[cls][1]:
                k = 1                                                       # away from the route bounds of the long classes: one read
            w, rd = _FAMILY_FN[f](n, k, _rng(f, n))
            assert len(w) == n, (f, n, len(w))
            sets.append(rd); refs.append(w); fam.append(f)
    n = CLASSES[cls][-1] if cls != "lane" else CLASSES[cls][0]
    for w, rd in shapes(n, _rng("shapes", n)):
        sets.append(rd); refs.append(w); fam.append("shapes")
    if cls == "cpl4":                                                       # the longest read the device takes, against a short window
        rng = _rng("long read")
        w = _rand(rng, 64, "AG")
        sets.append([w[:40] + _rand(rng, 1000 - 64, "AG") + w[40:]]); refs.append(w); fam.append("shapes")
    return sets, refs, fam


def _mix_sets(cls):
    """the class maximum together with windows of 1 - 10 bases: a small jn_lane, mostly idle lanes inside a wide layout"""
    rng = _rng("mix", cls)
    nmax = CLASSES[cls][-1]
    sets, refs, fam = [], [], []
    w, rd = run_in_flank(nmax, 2, rng)
    sets.append(rd); refs.append(w); fam.append("run_in_flank")
    for n in range(1, 11):
        w = _rand(rng, n, "AG")
        sets.append([_rand(rng, int(rng.integers(1, n + 6)), "AG") for _ in range(1 + n % 3)] + [w]); refs.append(w); fam.append("shapes")
    w, rd = homopolymer(nmax, 3, rng)
    sets.append(rd); refs.append(w); fam.append("homopolymer")
    return sets, refs, fam


_star = None


def star_calls():
    """{name: StarCall(cls, sets, refs, family per set)}: "<cls>" holds every family at the class's window lengths, "<cls>_mix" the class
    maximum beside windows of 1 - 10 bases"""
    global _star
    if _star is None:
        _star = collections.OrderedDict()
        for cls in CLASSES:
            for name, (sets, refs, fam) in ((cls, _family_sets(cls)), (cls + "_mix", _mix_sets(cls))):
                if sum(len(rd) for rd in sets) % 4 == 0:                    # four alignments per wave: the last wave keeps a dead 16-lane group
                    sets.append([refs[0][:-1]]); refs.append(refs[0]); fam.append("shapes")
                _star[name] = StarCall(cls, sets, refs, fam)
    return _star


_allele = None


def allele_calls():
    """{name: (consensus strings, windows, max_range)}: per device layout class the first reads of every star set as consensus sequences
    (global alignment: a read that stops early costs a terminal gap), plus the calls the device refuses (host fallback): an empty string, a
    consensus over 1,000 bases, a window over 272"""
    global _allele
    if _allele is None:
        _allele = collections.OrderedDict()
        for name, call in star_calls().items():
            if name.endswith("_mix"):
                continue
            alts, refs, mrs = [], [], []
            for s, (reads, w) in enumerate(zip(call.sets, call.refs)):
                for r, q in enumerate(reads[:4 if call.cls in ("cpl4", "cpl8") else 2]):
                    if len(q) > 400:
                        continue
                    alts.append(q); refs.append(w); mrs.append((10, 40, 20)[(s + r) % 3])
            _allele[name] = (alts, refs, mrs)
        rng = _rng("allele long")
        w = _rand(rng, 272, "AG")
        a, r, m = _allele["cpl17"]
        a.append(w[:100] + _rand(rng, 1000 - 272, "AG") + w[100:]); r.append(w); m.append(40)      # a consensus of exactly 1,000 bases
        a, r, m = _allele["cpl4"]
        _allele["fb_empty"] = (a[:6] + [""], r[:6] + ["AAAA"], m[:6] + [10])
        _allele["fb_long"] = (a[:3] + ["AG" * 501], r[:3] + ["AG" * 30], m[:3] + [10])
        a, r, m = _allele.pop("lane")
        _allele["fb_wide"] = (a, r, m)
    return _allele


# ------------------------------------------------------------------------------------------------------------------------ where the ties are
def tie_cells(s1, s2, scoring=STAR, free_tail=True, path_out=None):
    """Plain DP of the Gotoh recurrences, then the optimal path by the documented rules (extension before opening, diagonal before E, the
    better of those before F; free tail: corner, then last row outward from the corner, then last column).  -> Counter over TIE_KINDS of the
    path cells where the winner only equalled another candidate: opening == extension in E / in F, diagonal == E, max(diagonal, E) == F, and
    (free tail) the best end-point score found in more than one cell.  The matrices are filled a row at a time (numpy), the walk is plain
    Python; path_out, when given, receives the alignment's operations from its end back (7 / 8 diagonal, 2 E, 1 F)."""
    open_, extend, match, mismatch = scoring
    assert open_ >= extend >= 0                   # (the row form of E below: a gap never opens from a cell that a gap already reached)
    n1, n2 = len(s1), len(s2)
    out = collections.Counter()
    if n1 == 0 or n2 == 0:
        return out
    NEG = -10 ** 9
    b2 = np.frombuffer(s2.encode(), np.uint8)
    jx = np.arange(n2 + 1, dtype=np.int64) * extend
    H = np.zeros((n1 + 1, n2 + 1), np.int64)
    E = np.full((n1 + 1, n2 + 1), NEG, np.int64)
    F = np.full((n1 + 1, n2 + 1), NEG, np.int64)
    H[0, 1:] = E[0, 1:] = -open_ - jx[:n2]
    for i in range(1, n1 + 1):
        H[i, 0] = F[i, 0] = -open_ - (i - 1) * extend
        F[i, 1:] = np.maximum(H[i - 1, 1:] - open_, F[i - 1, 1:] - extend)
        d = H[i - 1, :-1] + np.where(b2 == ord(s1[i - 1]), match, mismatch)
        g = np.maximum(d, F[i, 1:])                # H without E; E[i][j] = max over k < j of max(g, H[i][0])[k] - open - (j - 1 - k) * extend
        src = np.concatenate(([H[i, 0]], g[:-1])) + jx[:n2]
        E[i, 1:] = np.maximum.accumulate(src) - open_ - jx[:n2]
        H[i, 1:] = np.maximum(g, E[i, 1:])
    H, E, F = H.tolist(), E.tolist(), F.tolist()
    i, j = n1, n2
    if free_tail:
        ends = [(H[n1][jj], n1, jj) for jj in range(n2, -1, -1)] + [(H[ii][n2], ii, n2) for ii in range(n1 - 1, -1, -1)]
        best = max(v for v, _, _ in ends)
        _, i, j = next(t for t in ends if t[0] == best)                     # the first in the documented order
        out["end"] += sum(1 for v, _, _ in ends if v == best) > 1
        if path_out is not None:
            path_out.extend([1] * (n1 - i) + [2] * (n2 - j))               # the unaligned tail: the rest of the window, then the rest of the read
    state = 0
    while i > 0 and j > 0:
        if state == 0:
            d = H[i - 1][j - 1] + (match if s1[i - 1] == s2[j - 1] else mismatch)
            e, f = E[i][j], F[i][j]
            out["diag_e"] += d == e and d >= f
            out["h_f"] += f == max(d, e)
            if f > max(d, e):
                state = 2
            elif e > d:
                state = 1
            else:
                if path_out is not None:
                    path_out.append(7 if s1[i - 1] == s2[j - 1] else 8)
                i, j = i - 1, j - 1
                continue
        if path_out is not None:
            path_out.append(3 - state)
        if state == 1:
            eo, ee = H[i][j - 1] - open_, E[i][j - 1] - extend
            out["e_open_ext"] += eo == ee
            j -= 1
            if ee < eo:
                state = 0
        else:
            fo, fe = H[i - 1][j] - open_, F[i - 1][j] - extend
            out["f_open_ext"] += fo == fe
            i -= 1
            if fe < fo:
                state = 0
    if path_out is not None:
        path_out.extend([2] * j + [1] * i)
    return out


def tie_cells_of_family(family, s1, s2):
    """the ties of one star pair as its family means them: free tail with the star scoring, but the homopolymer family by its global alignment
    (the allele_prediction form): a pure run against a pure run has a single optimal free-tail path and nothing to decide"""
    if family == "homopolymer":
        return tie_cells(s1, s2, NW, free_tail=False)
    return tie_cells(s1, s2, STAR, free_tail=True)


# ------------------------------------------------------------------------------------------------------------------------ a small world of repeats
def tie_world(seed=5, n_features=40, depth=16):
    """A contig stitched from the families above -- homopolymer runs, tandem repeats of 2-, 3- and 5-base units, two-letter stretches, random
    spacers between them -- with a het or hom indel of 1 - 12 bases planted in every run and repeat, and reads (explicit CIGARs, HP / PS tags on
    most) that carry it with the gap at DIFFERENT units of the repeat, as real aligners leave it.  A few reads hold a stretch whose CIGAR
    says aligned while its bases are the reference's 12 - 17 further on (the optimal path runs along their band's edge: a re-run), a long private deletion (a band too wide
    for 64 diagonals) or a middle-sized private indel (64 diagonals).  -> (reference, records for bamio.write_bam, features)"""
    rng = _rng("tie world", seed)
    parts, feats, pos = [_rand(rng, 260)], [], 260
    for f in range(n_features):
        kind = ("homopolymer", "tandem", "two_letter", "tandem")[f % 4]
        before = parts[-1][-1]
        if kind == "homopolymer":
            unit, cnt = _not(before, rng), int(rng.integers(8, 31))
        elif kind == "tandem":
            u = (2, 3, 5)[(f // 2) % 3]
            unit = _not(before, rng) + "".join(rng.permutation(list("AGTC"))[:u - 1])
            if len(set(unit)) == 1:
                unit = unit[:-1] + _not(unit[0])
            cnt = int(rng.integers(5, 40 // u + 1))
        else:
            unit, cnt = None, 60
        body = unit * cnt if unit else _rand(rng, cnt, "AG")
        if unit:
            d_units = int(rng.integers(1, max(2, min(12 // len(unit), cnt - 2) + 1))) * (1 if rng.random() < 0.5 else -1)
            delta = d_units * len(unit)
        else:
            delta = int(rng.integers(1, 7)) * (1 if rng.random() < 0.5 else -1)
        feats.append(dict(kind=kind, start=pos, unit=unit, cnt=cnt, delta=delta, hom=f % 3 == 0, ins=_rand(rng, abs(delta), "AG")))
        parts.append(body)
        pos += len(body)
        sp = _rand(rng, int(rng.integers(170, 231)))
        if unit and sp[0] == unit[0]:
            sp = _not(unit[0]) + sp[1:]
        parts.append(sp)
        pos += len(sp)
    ref = "".join(parts)
    L = len(ref)
    recs = []
    n_reads = int(depth * L / 1800)
    for r in range(n_reads):
        a = int(rng.integers(0, L - 700)) if r >= 4 else 0
        b = min(L, a + int(rng.integers(1200, 2500)))
        for ft in feats:                                                    # a read does not start or end inside a feature
            lo, hi = ft["start"] - 3, ft["start"] + len(ft["unit"] or "") * ft["cnt"] + (0 if ft["unit"] else 60) + 3
            if lo <= a < hi:
                a = hi + 2
            if lo < b <= hi:
                b = lo - 2
        if b - a < 300:
            continue
        truth = 1 + int(rng.integers(0, 2))
        special = ("none", "junk", "none", "none", "none", "junk", "none", "wide", "none", "mid_del", "none", "mid_ins")[r % 12]
        cigar, seq, p = [], [], a
        def emit(op, n, s=""):
            if n > 0:
                if cigar and cigar[-1][0] == op:
                    cigar[-1] = (op, cigar[-1][1] + n)
                else:
                    cigar.append((op, n))
                seq.append(s)
        done_special = False
        for ft in feats:
            flen = len(ft["unit"]) * ft["cnt"] if ft["unit"] else 60
            if ft["start"] < a or ft["start"] + flen > b:
                continue
            emit("M", ft["start"] - p, ref[p:ft["start"]])
            p = ft["start"]
            carries = ft["hom"] or truth == 1
            d, u = ft["delta"], len(ft["unit"] or "A")
            if not carries:
                emit("M", flen, ref[p:p + flen])
            elif ft["unit"]:
                if d > 0:                                                   # whole units gained before unit k of the repeat
                    k = int(rng.integers(0, ft["cnt"] + 1))
                    emit("M", k * u, ref[p:p + k * u]); emit("I", d, ft["unit"] * (d // u)); emit("M", flen - k * u, ref[p + k * u:p + flen])
                else:                                                       # whole units lost, from unit k on
                    k = int(rng.integers(0, ft["cnt"] + d // u + 1))
                    emit("M", k * u, ref[p:p + k * u]); emit("D", -d); emit("M", flen - k * u + d, ref[p + k * u - d:p + flen])
            else:
                k = 30
                if d > 0:
                    emit("M", k, ref[p:p + k]); emit("I", d, ft["ins"]); emit("M", flen - k, ref[p + k:p + flen])
                else:
                    emit("M", k, ref[p:p + k]); emit("D", -d); emit("M", flen - k + d, ref[p + k - d:p + flen])
            p += flen
            if special != "none" and not done_special and p + 150 < b and rng.random() < 0.5:
                done_special = True
                g = int(rng.integers(8, 40))
                emit("M", g, ref[p:p + g]); p += g
                if special == "junk":
                    n, sh = int(rng.integers(30, 51)), int(rng.integers(12, 18))      # the CIGAR says aligned, the bases are the reference's 12 - 17
                    emit("M", n, ref[p + sh:p + sh + n]); p += n                     # further on: the optimal path runs along the band's edge
                elif special == "wide":
                    emit("D", 58); p += 58
                elif special == "mid_del":
                    emit("D", 24); p += 24
                else:
                    emit("I", 22, _rand(rng, 22))
        emit("M", b - p, ref[p:b])
        tags = {"HP": truth, "PS": 1000} if rng.random() < 0.85 else {}
        recs.append(dict(name="t%03d" % r, flag=16 if r % 2 else 0, pos0=a, cigar=cigar, seq="".join(seq), tags=tags))
    recs.sort(key=lambda x: x["pos0"])
    return ref, recs, feats

"""Instances that drive the device phaser (csrc/nc_happhase.hip, nc_hpquals.hip) to the ends of its input space, built in plain Python and numpy:

  range family        two reads (and one member with fifteen) whose partition costs spread by exactly 65,535 -- the largest value k_hp_dp's uint16
                      relative costs hold -- and twins that spread by 65,536, which the solve must refuse with NC_ERR_CAPACITY
  transition family   one instance of four-column blocks, one block per pair (continuing reads nk, leaving reads nl) and more blocks than the device
                      has compute units, the slots of continuing and leaving reads interleaved
  long operations     BAM records whose CIGAR operations are longer than 65,535 bases, or add up to more inside and across k_hp_quals' 64-operation
                      chunks, with sites on the operations' ends and around the multiples of 65,536

Every builder returns what Engine.snp_phase(csr=...) and the restatements (phase_ref, phase_gt_ref, phase_w_ref) take.  `relative_spread` stands
beside the restatements: the same column recurrence on absolute costs (int64: a column adds at most 15 * 93 + 1024, so nothing here comes near
2^63), reporting the quantity the kernel keeps in 16 bits.  The four forms carry k_hp_dp<GT, W>'s letters: ff plain, fW weighted, Gf
genotype-aware, GW both."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from phase_ref import NSLOT, _subsets
from phase_w_ref import W_MAX, _costs, random_weighted_instance, select_reads_w

FORMS = ("ff", "fW", "Gf", "GW")
EDGE = 0xFFFF                    # the largest relative cost a uint16 holds
G_MAX = 1024                     # nc_snp_phase_solve_gt's largest price


# ------------------------------------------------------------------------------------------- columns and the spread of their costs
def block_columns(reads, n_sites, weights=None, read_ok=None, max_cov=15):
    """read selection, blocks and slots as DESIGN.md "Read-based phasing" states them (a read entering at a column takes the lowest free slot, in
    read-index order) -> (accepted, blocks): per block (first site, [(act, keep, m0, m1, wvec) per column]); wvec = the 15 slots' weights at the
    column (1 for an allele where `weights` is None)"""
    acc = select_reads_w(reads, n_sites, read_ok, max_cov)
    rr = np.flatnonzero(acc).tolist()
    joined, covered = np.zeros(n_sites, bool), np.zeros(n_sites, bool)
    starts, ends = {}, {}
    for r in rr:
        a, b = reads[r][0][0], reads[r][-1][0]
        joined[a:b] = True
        covered[a:b + 1] = True
        starts.setdefault(a, []).append(r)
        ends.setdefault(b, []).append(r)
    cols = [None] * n_sites
    slot, firsts, i = {}, [], 0
    while i < n_sites:
        if not covered[i]:
            i += 1
            continue
        f = i
        free, act = set(range(NSLOT)), 0
        while True:
            if i > f:
                for r in ends.get(i - 1, []):
                    free.add(slot[r])
                    act &= ~(1 << slot[r])
            enter = 0
            for r in starts.get(i, []):
                slot[r] = min(free)
                free.remove(slot[r])
                enter |= 1 << slot[r]
            act |= enter
            cols[i] = [act, act & ~enter, 0, 0, [0] * NSLOT]
            if i == n_sites - 1 or not joined[i]:
                break
            i += 1
        firsts.append((f, i))
        i += 1
    for r in rr:
        for k, (s, a) in enumerate(reads[r]):
            cols[s][3 if a else 2] |= 1 << slot[r]
            cols[s][4][slot[r]] = 1 if weights is None else int(weights[r][k])
    return acc, [(f, [(c[0], c[1], c[2], c[3], tuple(c[4])) for c in cols[f:l + 1]]) for f, l in firsts]


_subs = lru_cache(maxsize=4096)(_subsets)


@lru_cache(maxsize=4096)
def _column_cost(act, m0, m1, wvec, gt, G):
    """the column's cost for every subset of `act`, ascending (gt None: the plain rule)"""
    c0, c1 = _costs(_subs(act), m0, m1, wvec)
    cost = np.minimum(c0, c1)
    if gt is not None:
        hom_a = sum(wvec[s] for s in range(NSLOT) if m1 >> s & 1) + (0 if gt == 1 else G)
        hom_b = sum(wvec[s] for s in range(NSLOT) if m0 >> s & 1) + (0 if gt == 2 else G)
        cost = np.minimum(cost + (0 if gt == 0 else G), min(hom_a, hom_b))
    cost.setflags(write=False)
    return cost


def spread_walk(reads, n_sites, weights=None, read_ok=None, site_gt=None, G=30, max_cov=15):
    """one form's recurrence D(j, B) = min over the leaving slots of D(j - 1, .) + cost(j, B) on absolute costs
    -> dict: spread (the maximum over the columns of max_B D - min_B D over the column's active states), site and state (where the maximum is
    reached first, the state the largest of the column), totals (min_B D of every block's last column: the block costs),
    minima (how many states of that column reach it)"""
    _, blocks = block_columns(reads, n_sites, weights, read_ok, max_cov)
    D, P = np.zeros(1 << NSLOT, np.int64), np.zeros(1 << NSLOT, np.int64)
    best, totals, minima = dict(spread=0, site=-1, state=0), [], []
    for f, cols in blocks:
        prev, v = 0, None
        for k, (act, K, m0, m1, wvec) in enumerate(cols):
            B = _subs(act)
            v = _column_cost(act, m0, m1, wvec, None if site_gt is None else int(site_gt[f + k]), G)
            if k:
                bk, xl = _subs(K), _subs(prev & ~K)
                P[bk] = D[bk[:, None] | xl[None, :]].min(axis=1)
                v = P[B & K] + v
            D[B] = v
            sp = int(v.max() - v.min())
            if sp > best["spread"]:
                best = dict(spread=sp, site=f + k, state=int(B[np.argmax(v)]))
            prev = act
        totals.append(int(v.min()))
        minima.append(int((v == v.min()).sum()))
    best.update(totals=totals, minima=minima)
    return best


def form_arguments(form, weights, read_ok, site_gt):
    """what a form reads of an instance: the plain forms no weight and no read_ok, the forms without genotypes no called class"""
    w = form[1] == "W"
    return (weights if w else None), (read_ok if w else None), (site_gt if form[0] == "G" else None)


def relative_spread(reads, n_sites, weights=None, read_ok=None, site_gt=None, G=30, max_cov=15, forms=FORMS):
    """-> {form: the maximum over the columns of max_B D(j, B) - min_B D(j, B)}: what k_hp_dp holds as uint16"""
    out = {}
    for form in forms:
        w, ok, gt = form_arguments(form, weights, read_ok, site_gt)
        out[form] = spread_walk(reads, n_sites, w, ok, gt, G, max_cov)["spread"]
    return out


# ------------------------------------------------------------------------------------------- the range family
def _instance(reads, weights, n_sites, gt=None, G=G_MAX, groups=None, pos=None):
    pos = 10 * np.arange(1, n_sites + 1, dtype=np.int32) if pos is None else pos
    return dict(reads=reads, weights=weights, read_ok=np.ones(len(reads), np.uint8), n_sites=n_sites, max_cov=15, pos=pos,
                groups=np.arange(len(reads), dtype=np.int32) if groups is None else groups, gt=np.zeros(n_sites, np.uint8) if gt is None else gt, G=G)


def two_reads(n, weight=1, last=None):
    """two reads with allele 0 at every one of n sites, every weight `weight` and the last column's `last`: the state that separates them costs
    the smaller of the two weights per column, the states that keep them together nothing -- the spread is the sum of the columns' weights.
    Called class 0 everywhere and the largest price, so neither homozygous outcome (2 w + G) caps the split state's cost"""
    w = [weight] * (n - 1) + [weight if last is None else last]
    return _instance([[(s, 0) for s in range(n)] for _ in range(2)], [list(w), list(w)], n)


def two_reads_closed_form(inst):
    """the solve of a two_reads instance in every form: one block of cost 0, every site phased with h 0 (and outcome het), both reads on side 0
    (the smallest of the two minimising states), PS the first position; both names tagged HP 1"""
    n, ps = inst["n_sites"], int(inst["pos"][0])
    res = dict(accepted=np.ones(2, bool), side=np.zeros(2, np.int8), site_block=np.zeros(n, np.int32), site_h=np.zeros(n, np.uint8),
               site_gt=np.zeros(n, np.uint8), site_phased=np.ones(n, bool), site_ps=np.full(n, ps, np.int32), blocks=[(0, n - 1, ps, 0)])
    return res, np.ones(2, np.uint8), np.full(2, ps, np.int32)


W_COLUMNS, W_LAST = 705, 63      # 704 * 93 + 63 = 65,535
U_COLUMNS = EDGE                 # one unit per column: n columns spread by n


def range_members():
    """-> {name: (instance, the forms it is for, its spread)}: each member at the edge and its twin one beyond"""
    out = {}
    for over in (0, 1):
        tag = "over" if over else "edge"
        out["weighted-" + tag] = (two_reads(W_COLUMNS, W_MAX, W_LAST + over), ("fW", "GW"), EDGE + over)
        out["unit-" + tag] = (two_reads(U_COLUMNS + over), ("ff", "Gf"), EDGE + over)
        out["fifteen-" + tag] = (fifteen_reads(over), ("fW", "GW"), EDGE + over)
    return out


F_COLUMNS = 102
# the last column's weights of fifteen_reads, found by a search on spread_walk (tests/test_phase_edges_ref.py asserts the spreads they give)
F_LAST = (91, 88, 88, 88, 88, 88, 88, 88, 88, 90, 88, 88, 88, 88, 88)
F_LAST_OVER = (9, 1)             # (read, its last weight's increment) of the twin


def fifteen_reads(over=0, last=None):
    """fifteen reads over every one of 102 sites, eight from one haplotype and seven from the other of a seeded truth, a few alleles flipped so
    that the optimum is no all-zero state; every weight 93 but the last column's (F_LAST: tuned so that the spread is exactly 65,535; the twin's
    one beyond).  All 15 slots are active in every column, so the state that reaches the edge reads both halves of the weighted form's tables"""
    rng = np.random.default_rng(1515)
    n = F_COLUMNS
    truth = rng.integers(0, 2, n)
    flips = {(int(rng.integers(0, NSLOT)), int(rng.integers(1, n - 1))) for _ in range(9)}
    reads = [[(s, int(truth[s]) ^ (r & 1) ^ int((r, s) in flips)) for s in range(n)] for r in range(NSLOT)]
    last = list(F_LAST if last is None else last)
    if over:
        last[F_LAST_OVER[0]] += F_LAST_OVER[1]
    weights = [[W_MAX] * (n - 1) + [last[r]] for r in range(NSLOT)]
    gt = np.zeros(n, np.uint8)
    return _instance(reads, weights, n, gt=gt, pos=np.sort(rng.choice(np.arange(1, 10 * n), n, replace=False)).astype(np.int32))


# ------------------------------------------------------------------------------------------- the transition family
def transition_pairs():
    return [(nk, nl) for nk in range(1, NSLOT + 1) for nl in range(0, NSLOT + 1 - nk)]


def transition_instance(seed=1510):
    """blocks of four columns with an uncovered site between them: nk reads over columns 0-3, nl over columns 0-1, ne over columns 2-3 -- every
    pair (nk, nl) with ne = 15 - nk and with ne = 0, and nk in {9, 10, 11} with nl in {0, 1, 4} once more with the leaving reads first.  The
    continuing and leaving reads alternate in read-index order, so they take interleaved slots: at column 2 the continuing mask K and the leaving
    mask are no runs of bits.  Alleles from a two-haplotype truth with 10 % errors and 20 % missing entries (a read's first and last entry stay,
    so its span is as built); weights, called classes, a price and name groups as phase_w_ref.gpu_instances draws them, every read allowed; some
    names own two reads in different blocks.  -> (instance, specs): specs[b] = (nk, nl, ne) of block b"""
    rng = np.random.default_rng(seed)
    specs = [(nk, nl, ne, 0) for nk, nl in transition_pairs() for ne in (NSLOT - nk, 0)]
    specs += [(nk, nl, ne, 1) for nk in (9, 10, 11) for nl in (0, 1, 4) for ne in (NSLOT - nk, 0)]
    n_sites = 5 * len(specs)
    truth = rng.integers(0, 2, n_sites)
    reads, block_of = [], []
    for b, (nk, nl, ne, leaving_first) in enumerate(specs):
        kinds, k, l = [], nk, nl
        while k or l:                                                    # alternate while both kinds last
            for kind in ("lk" if leaving_first else "kl"):
                if kind == "k" and k:
                    kinds.append((0, 3))
                    k -= 1
                elif kind == "l" and l:
                    kinds.append((0, 1))
                    l -= 1
        for a, e in kinds + [(2, 3)] * ne:
            h, rd = int(rng.integers(0, 2)), []
            for s in range(5 * b + a, 5 * b + e + 1):
                if a + 5 * b < s < e + 5 * b and rng.random() < 0.2:
                    continue
                rd.append((s, int(truth[s]) ^ h ^ int(rng.random() < 0.1)))
            reads.append(rd)
            block_of.append(b)
    weights, _ = random_weighted_instance(rng, reads)
    groups = np.arange(len(reads))
    block_of = np.array(block_of)
    paired = set()
    for r in range(0, len(reads), 11):                                   # a name with a second alignment seven blocks on (no name gets a third)
        later = np.flatnonzero(block_of == block_of[r] + 7)
        if later.size and not {r, int(later[r % later.size])} & paired:
            groups[later[r % later.size]] = groups[r]
            paired |= {r, int(later[r % later.size])}
    groups = np.unique(groups, return_inverse=True)[1].astype(np.int32)
    pos = np.sort(rng.choice(np.arange(1, 10 * n_sites + 1), n_sites, replace=False)).astype(np.int32)
    inst = _instance(reads, weights, n_sites, gt=rng.choice([0, 0, 2], n_sites).astype(np.uint8), G=30, groups=groups, pos=pos)
    return inst, [s[:3] for s in specs]


def is_run(mask):
    """whether the set bits of mask are one contiguous run (the empty mask counts as one)"""
    if not mask:
        return True
    m = mask >> ((mask & -mask).bit_length() - 1)
    return m & (m + 1) == 0


# ------------------------------------------------------------------------------------------- records with long CIGAR operations
_OPS = "MIDNSHP=X"
HIGH = 200_000_000


def real_cigar(r):
    """a record's CIGAR: the CG tag's behind the placeholder <l_seq>S<n>N, else its own"""
    return [(_OPS[v & 15], v >> 4) for v in r["tags"]["CG"]] if "CG" in r.get("tags", {}) else r["cigar"]


def ref_span(cigar):
    return sum(n for op, n in cigar if op in "MDN=X")


def long_op_cigars():
    """-> {name: cigar}"""
    many = []                                                            # the 151 operations of the hand-made records' `many`, each 700 times as long
    for k in range(50):
        many += [("M", 700 * (3 + k % 4)), ("I" if k % 2 else "D", 700 * (1 + k % 3)), ("=", 1400)]
    many.append(("X", 2800))
    return {"m70000": [("M", 70000)],                                    # one lane with a non-zero high half
            # three chunks of 32 pairs: a chunk's low halves add up to 70,432 (they pass 65,536 at its 30th pair), and the second and third
            # chunk start from rp and qp above 65,536.  (1100M 1D pairs add up to 35,232 a chunk, which never crosses.)
            "pairs": [("M", 2200), ("D", 1)] * 96,
            "bigdel": [("M", 20), ("D", HIGH), ("M", 20)],                # large high halves, 64-bit a / b inside int32 positions
            "many700": many}


def long_op_records(seed=65536):
    """each CIGAR once as the record's own and once behind the placeholder with the CG tag; random qualities 0..93 and MAPQs on both sides of 20.
    `bigdel` starts at position 100, the others beyond 200,000,000 -> record dicts for bamio_w.record_stream"""
    rng = np.random.default_rng(seed)
    recs, pos0 = [], {"bigdel": 99}
    nxt = HIGH + 1000
    for name, cig in long_op_cigars().items():
        if name not in pos0:
            pos0[name] = nxt
            nxt += ref_span(cig) + 3 * 65536 + 17
    for name, cig in long_op_cigars().items():
        for twin in (0, 1):
            L = sum(n for op, n in cig if op in "MIS=X")
            r = dict(name=name + ("-cg" if twin else ""), flag=0, pos0=pos0[name] + 7 * twin, seq="".join(np.array(list("ACGT"))[rng.integers(0, 4, L)]),
                     mapq=int(rng.choice([60, 60, 20, 19, 3])), qual=bytes(rng.integers(0, 94, L, dtype=np.uint8)), tags={}, cigar=cig)
            if twin:
                r["tags"] = {"XA": "text", "CG": [(n << 4) | _OPS.index(op) for op, n in cig]}
                r["cigar"] = [("S", L), ("N", ref_span(cig))]
            recs.append(r)
    return recs


def long_op_sites(r, cap=4):
    """the 1-based positions of a record's sites: the first and last reference base of every reference-consuming operation, the bases m - 1, m,
    m + 1 around every offset m from the alignment's start that is a multiple of 65,536 (of an operation with more than 2 * cap of them the
    first and last `cap`: inside one operation the kernel's arithmetic is the same for every multiple, and inside a deletion every site takes the
    same query base), the base before the alignment and the two behind it"""
    s1, o, out = r["pos0"] + 1, 0, set()
    for op, n in real_cigar(r):
        if op not in "MDN=X":
            continue
        out |= {s1 + o, s1 + o + n - 1}
        mult = list(range((o // 65536 + 1) * 65536, o + n, 65536))
        if len(mult) > 2 * cap:
            mult = mult[:cap] + mult[-cap:]
        for m in mult:
            out |= {s1 + x for x in (m - 1, m, m + 1) if o <= x < o + n}
        o += n
    return out | {s1 - 1, s1 + o, s1 + o + 1}


def long_op_csr(recs, seed=7):
    """-> (site positions, reads): a record's read holds its own sites and its twin's (long_op_sites; the twin starts 7 bases on, so these fall
    beside the operations' ends), with seeded alleles -- the two disagree at about half of their sites, so a solve's costs are sums of weights"""
    rng = np.random.default_rng(seed)
    own = [long_op_sites(r) for r in recs]
    pos = np.array(sorted(set().union(*own)), np.int32)
    index = {int(p): s for s, p in enumerate(pos)}
    reads = [[(s, int(rng.integers(0, 2))) for s in sorted(index[p] for p in own[k] | own[k ^ 1])] for k in range(len(recs))]
    return pos, reads

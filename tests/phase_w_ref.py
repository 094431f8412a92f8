"""Pure-numpy restatement of the phaser's weighted model (DESIGN.md "Read-based phasing", step 6c), written from the model's statement and
independently of csrc/nc_happhase.hip: every entry (read, site, allele) carries a weight 0..93 -- the price of flipping it --, a read with
read_ok 0 is never accepted, a name's haplotag score adds +-weight.  The subset enumeration is phase_ref's; selection, blocks, slots, the DP
with its tie-breaks, the outcomes of the genotype-aware form, the haplotagger and the quality lookup on a BAM record's CIGAR are restated here.

An instance is phase_ref's (`reads`: per read a sorted list of (site, allele 0/1)) plus `weights`: per read the list of its entries' weights,
and `read_ok` (None: every read allowed).  `site_gt` / `G` as in phase_gt_ref (None: the plain column rule).

Column rule, W(mask) = the summed weights of the slots in mask:
    c0(B) = W(m1 & ~B) + W(m0 & B)      c1(B) = W(m0 & ~B) + W(m1 & B)      cost(B) = min(c0, c1), site_h = 0 iff c0 <= c1
    genotype-aware: het = min(c0, c1) (+G), homA = W(m1) (+G), homB = W(m0) (+G), ties as in phase_gt_ref."""
from __future__ import annotations

import numpy as np

from phase_ref import NSLOT, _subsets

W_MAX = 93


def select_reads_w(reads, n_sites, read_ok=None, max_cov=15):
    """entry count, then first site, then index; a read with read_ok 0 is never accepted"""
    cand = [r for r in range(len(reads)) if len(reads[r]) >= 2 and (read_ok is None or read_ok[r])]
    cand.sort(key=lambda r: (-len(reads[r]), reads[r][0][0], r))
    depth = [0] * n_sites
    acc = np.zeros(len(reads), bool)
    for r in cand:
        a, b = reads[r][0][0], reads[r][-1][0]
        if all(depth[s] < max_cov for s in range(a, b + 1)):
            for s in range(a, b + 1):
                depth[s] += 1
            acc[r] = True
    return acc


def _wsum(B, wvec, mask):
    """W(B & mask) for every B of the array"""
    out = np.zeros(B.shape, np.int64)
    for s in range(NSLOT):
        if mask >> s & 1:
            out += ((B >> s) & 1) * int(wvec[s])
    return out


def _costs(B, m0, m1, wvec):
    full = (1 << NSLOT) - 1
    c0 = _wsum(~B & full, wvec, m1) + _wsum(B, wvec, m0)
    c1 = _wsum(~B & full, wvec, m0) + _wsum(B, wvec, m1)
    return c0, c1


def _outcome(c0, c1, wa, wb, gt, G):
    """(costs of het / homA / homB, the winner): the smallest (cost, pref), pref 0 for the called class, else 1 het, 2 homA, 3 homB"""
    cost = [min(int(c0), int(c1)) + (0 if gt == 0 else G), wa + (0 if gt == 1 else G), wb + (0 if gt == 2 else G)]
    return cost, min(range(3), key=lambda o: (cost[o], 0 if o == gt else o + 1))


def phase_w(site_pos, reads, weights, read_ok=None, site_gt=None, G=30, max_cov=15):
    """-> dict: accepted, side, site_block, site_h, site_phased, site_ps, blocks [(first, last, ps, cost)], and with site_gt the outcomes"""
    n_sites = len(site_pos)
    gt_in = None if site_gt is None else np.asarray(site_gt, np.int64)
    acc = select_reads_w(reads, n_sites, read_ok, max_cov)
    span = {r: (reads[r][0][0], reads[r][-1][0]) for r in np.flatnonzero(acc).tolist()}
    joined, covered, has = np.zeros(max(n_sites - 1, 0), bool), np.zeros(n_sites, bool), np.zeros(n_sites, bool)
    for r, (a, b) in span.items():
        joined[a:b] = True
        covered[a:b + 1] = True
        for s, _ in reads[r]:
            has[s] = True
    site_block = np.full(n_sites, -1, np.int32)
    site_h = np.zeros(n_sites, np.uint8)
    phased = np.zeros(n_sites, bool)
    site_ps = np.zeros(n_sites, np.int32)
    out_gt = None if gt_in is None else gt_in.astype(np.uint8).copy()
    side = np.full(len(reads), -1, np.int8)
    bounds, i = [], 0
    while i < n_sites:
        if not covered[i]:
            i += 1
            continue
        j = i
        while j < n_sites - 1 and joined[j]:
            j += 1
        bounds.append((i, j))
        i = j + 1
    blocks = []
    for bi, (f, l) in enumerate(bounds):
        site_block[f:l + 1] = bi
        mine = sorted(r for r, (a, b) in span.items() if f <= a and b <= l)
        slot, free, active, cols = {}, set(range(NSLOT)), [], []
        for c in range(f, l + 1):
            for r in [r for r in active if span[r][1] == c - 1]:
                free.add(slot[r])
                active.remove(r)
            enter = 0
            for r in (r for r in mine if span[r][0] == c):
                slot[r] = min(free)
                free.remove(slot[r])
                enter |= 1 << slot[r]
                active.append(r)
            act = m0 = m1 = 0
            wvec = [0] * NSLOT
            for r in active:
                act |= 1 << slot[r]
                for (s, a), w in zip(reads[r], weights[r]):
                    if s == c:
                        wvec[slot[r]] = int(w)
                        if a == 0:
                            m0 |= 1 << slot[r]
                        else:
                            m1 |= 1 << slot[r]
            cols.append((act, act & ~enter, m0, m1, wvec, 0 if gt_in is None else int(gt_in[c])))
        D, back = None, []
        for k, (act, K, m0, m1, wvec, gt) in enumerate(cols):
            B = _subsets(act)
            c0, c1 = _costs(B, m0, m1, wvec)
            cost = np.minimum(c0, c1)
            if gt_in is not None:
                wa = sum(wvec[s] for s in range(NSLOT) if m1 >> s & 1) + (0 if gt == 1 else G)
                wb = sum(wvec[s] for s in range(NSLOT) if m0 >> s & 1) + (0 if gt == 2 else G)
                cost = np.minimum(cost + (0 if gt == 0 else G), min(wa, wb))
            Dn = np.full(1 << NSLOT, -1, np.int64)
            if k == 0:
                Dn[B] = cost
                back.append(None)
            else:
                leaving = cols[k - 1][0] & ~K
                bk, xl = _subsets(K), _subsets(leaving)
                M = D[bk[:, None] | xl[None, :]]
                arg = np.argmin(M, axis=1)                          # the first minimum: the smallest leaving-slot bits
                P = np.zeros(1 << NSLOT, np.int64)
                P[bk] = M[np.arange(bk.size), arg]
                bt = np.zeros(1 << NSLOT, np.int64)
                bt[bk] = xl[arg]
                back.append(bt)
                Dn[B] = P[B & K] + cost
            D = Dn
        B = _subsets(cols[-1][0])
        best = int(B[np.argmin(D[B])])                              # the smallest minimising B of the last column
        total = int(D[best])
        chosen = [0] * len(cols)
        for k in range(len(cols) - 1, -1, -1):
            chosen[k] = best
            if k:
                best = (best & cols[k][1]) | int(back[k][best & cols[k][1]])
        for k, (act, K, m0, m1, wvec, gt) in enumerate(cols):
            c = f + k
            c0, c1 = _costs(np.array([chosen[k]]), m0, m1, wvec)
            site_h[c] = 0 if c0[0] <= c1[0] else 1
            phased[c] = has[c]
            if gt_in is not None:
                wa = sum(wvec[s] for s in range(NSLOT) if m1 >> s & 1)
                wb = sum(wvec[s] for s in range(NSLOT) if m0 >> s & 1)
                out_gt[c] = _outcome(c0[0], c1[0], wa, wb, gt, G)[1]
                phased[c] = has[c] and out_gt[c] == 0
        ph = [c for c in range(f, l + 1) if phased[c]]
        ps = int(site_pos[ph[0]]) if ph else 0
        site_ps[ph] = ps
        for r in mine:
            side[r] = (chosen[span[r][0] - f] >> slot[r]) & 1
        blocks.append((f, l, ps, total))
    res = dict(accepted=acc, side=side, site_block=site_block, site_h=site_h, site_phased=phased, site_ps=site_ps, blocks=blocks)
    if gt_in is not None:
        res["site_gt"] = out_gt
    return res


def haplotag_w(reads, weights, groups, res):
    """-> (hp uint8, ps int32) per name group: the block by the count of phased sites, then PS; HP by the sign of the summed +-weights"""
    n_groups = int(max(groups) + 1) if len(groups) else 0
    tot = [dict() for _ in range(n_groups)]
    for r, g in enumerate(groups):
        for (s, a), w in zip(reads[r], weights[r]):
            if not res["site_phased"][s]:
                continue
            t = tot[g].setdefault(int(res["site_block"][s]), [0, 0])
            t[0] += 1
            t[1] += int(w) if a == res["site_h"][s] else -int(w)
    hp, ps = np.zeros(n_groups, np.uint8), np.zeros(n_groups, np.int32)
    for g in range(n_groups):
        if tot[g]:
            b = min(tot[g], key=lambda b: (-tot[g][b][0], res["blocks"][b][2]))
            if tot[g][b][1]:
                hp[g] = 1 if tot[g][b][1] > 0 else 2
                ps[g] = res["blocks"][b][2]
    return hp, ps


def brute_force_wmec(reads, weights, accepted, n_sites, site_gt=None, G=30):
    """the minimum over every bipartition of the accepted reads of the summed per-site cost (weighted; with site_gt the cheapest outcome)"""
    rr = np.flatnonzero(accepted).tolist()
    al = np.full((len(rr), n_sites), -1, np.int64)
    wt = np.zeros((len(rr), n_sites), np.int64)
    for i, r in enumerate(rr):
        for (s, a), w in zip(reads[r], weights[r]):
            al[i, s], wt[i, s] = a, w
    best = None
    for part in range(1 << len(rr)):
        side = np.array([(part >> i) & 1 for i in range(len(rr))], np.int64).reshape(-1, 1)
        c0 = (wt * (((al == 1) & (side == 0)) | ((al == 0) & (side == 1)))).sum(0)
        c1 = (wt * (((al == 0) & (side == 0)) | ((al == 1) & (side == 1)))).sum(0)
        cost = np.minimum(c0, c1)
        if site_gt is not None:
            gt = np.asarray(site_gt)
            wa, wb = (wt * (al == 1)).sum(0) + np.where(gt == 1, 0, G), (wt * (al == 0)).sum(0) + np.where(gt == 2, 0, G)
            cost = np.minimum(cost + np.where(gt == 0, 0, G), np.minimum(wa, wb))
        v = int(cost.sum())
        best = v if best is None else min(best, v)
    return 0 if best is None else best


def mec_cost_w(reads, weights, res):
    """the weighted disagreements of the accepted reads with their part's haplotype under a result of the plain rule"""
    n = 0
    for r, rd in enumerate(reads):
        if res["side"][r] >= 0:
            n += sum(int(w) for (s, a), w in zip(rd, weights[r]) if a != (int(res["site_h"][s]) ^ int(res["side"][r])))
    return n


def hand_instance():
    """two Q40 reads against three Q5 reads at one site.  Reads 0-4 come from one haplotype (allele 0 at sites 0 and 2), reads 5-7 from the other
    (allele 1 there, no allele at site 1).  At site 1 reads 0-1 show allele 0 at Q40, reads 2-4 allele 1 at Q5.  Unit costs: flipping the two is
    cheaper (2 < 3), the first haplotype carries allele 1 at site 1; weighted: flipping the three costs 15 < 80, it carries allele 0.
    -> (site_pos, reads, weights)"""
    reads = [[(0, 0), (1, int(r >= 2)), (2, 0)] for r in range(5)] + [[(0, 1), (2, 1)] for _ in range(3)]
    weights = [[40, 40 if r < 2 else 5, 40] for r in range(5)] + [[40, 40] for _ in range(3)]
    return np.array([100, 200, 300], np.int32), reads, weights


def random_weighted_instance(rng, reads):
    """weights and read_ok for an instance of phase_ref.random_instance: qualities drawn from 0..93 (a share of them low, some zero), about a
    sixth of the reads below the floor -> (weights, read_ok uint8)"""
    weights = []
    for rd in reads:
        w = rng.integers(0, W_MAX + 1, len(rd))
        low = rng.random(len(rd)) < 0.3
        w[low] = rng.integers(0, 8, int(low.sum()))
        weights.append([int(v) for v in w])
    return weights, (rng.random(len(reads)) >= 1 / 6).astype(np.uint8)


def unit_weights(reads):
    return [[1] * len(rd) for rd in reads]


def flat_weights(weights):
    return np.array([w for rd in weights for w in rd], np.uint8)


# ------------------------------------------------------------------------------------------- the quality lookup on a BAM record
_CONSUMES_REF, _CONSUMES_QUERY = "MDN=X", "MIS=X"


def qual_lookup(pos1, cigar, qual, site_positions, default_weight=30, w_max=W_MAX):
    """pos1: the 1-based position of the alignment's first reference base; cigar: [(op letter, length)]; qual: the record's quality bytes (a
    list / bytes of l_seq values, 0xff = absent; empty when the record stores no sequence) -> per site position its weight: min(quality of the
    aligned query base, w_max) under M / = / X, the last query base's before the operation under D / N, default_weight where there is no such
    base, no quality, or the alignment does not reach the site.  H and P consume nothing; S and I consume query."""
    out = []
    for sp in site_positions:
        rp, qp, w = pos1, 0, default_weight
        for op, n in cigar:
            if op in _CONSUMES_REF and rp <= sp < rp + n:
                q = qp + (sp - rp) if op in "M=X" else qp - 1
                if 0 <= q < len(qual) and qual[q] != 0xff:
                    w = min(int(qual[q]), w_max)
                break
            if op in _CONSUMES_REF:
                rp += n
            if op in _CONSUMES_QUERY:
                qp += n
        out.append(w)
    return out


# ------------------------------------------------------------------------------------------- the instances of the GPU comparison
def gpu_instances(seed=9393):
    """the shapes of tests/test_phase_gt_gpu.py: 48 random instances of 2-40 sites and 1-60 reads, two with more than 15 reads over every site,
    the two-column block beside a block whose middle column has no accepted allele -- each with weights from 0..93, read_ok, called classes,
    a price, name groups and positions -> list of dicts"""
    from phase_ref import random_instance
    rng = np.random.default_rng(seed)
    raw = []
    for k in range(48):
        n_sites = int(rng.integers(2, 41))
        n_reads = int(rng.integers(1, 61 if k % 3 == 0 else 14))
        reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=float(rng.choice([0.0, 0.05, 0.2])), max_len=int(rng.integers(2, n_sites + 1)))
        raw.append((reads, n_sites, int(rng.choice([15, 15, 6, 2]))))
    for n_reads, n_sites in ((20, 6), (33, 11)):
        truth = rng.integers(0, 2, n_sites)
        raw.append(([[(s, int(truth[s]) ^ (r & 1) ^ int(rng.random() < 0.15)) for s in range(n_sites)] for r in range(n_reads)], n_sites, 15))
    raw.append(([[(0, 0), (1, 1)], [(3, 0), (5, 0)], [(3, 1), (5, 1)], [(4, 1)]], 6, 15))
    out = []
    for k, (reads, n_sites, max_cov) in enumerate(raw):
        n_reads = len(reads)
        weights, read_ok = random_weighted_instance(rng, reads)
        if k == len(raw) - 1:
            read_ok[:] = 1                                               # (the two-column block stays)
        groups = np.unique(rng.integers(0, max(1, n_reads - n_reads // 4), n_reads), return_inverse=True)[1].astype(np.int32)
        pos = np.sort(rng.choice(np.arange(1, 10 * n_sites + 1), n_sites, replace=False)).astype(np.int32)
        out.append(dict(reads=reads, weights=weights, read_ok=read_ok, n_sites=n_sites, max_cov=max_cov, groups=groups, pos=pos,
                        gt=rng.choice([0, 0, 2], n_sites).astype(np.uint8), G=int(rng.choice([1, 30, 30, 120]))))
    return out


def continuing(reads, res):
    """per block the largest number of accepted spans that cover two adjacent columns (the continuing set's size)"""
    acc = np.flatnonzero(res["accepted"])
    return [max(sum(1 for r in acc if reads[r][0][0] < c <= reads[r][-1][0]) for c in range(f + 1, l + 1)) for f, l, _, _ in res["blocks"]]

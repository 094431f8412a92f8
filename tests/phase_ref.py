"""Pure-numpy restatement of the read-based SNP phaser and haplotagger (DESIGN.md "Read-based phasing"), steps 2-8, written
from the algorithm's statement and independently of csrc/nc_happhase.hip.  The tests compare the library's results with it bit
for bit and check it against a brute-force minimum-error-correction search on small instances.

An instance: `n_sites` sites in position order (`site_pos`), and per read its alleles as a sorted list of (site, allele 0/1)
(`reads`).  `groups`: one name-group id per read (alignments that share a read name), for the haplotags."""
from __future__ import annotations

import numpy as np

NSLOT = 15


def _subsets(mask):
    """every submask of `mask`, ascending"""
    bits = [b for b in range(NSLOT) if mask >> b & 1]
    t = np.arange(1 << len(bits), dtype=np.int64)
    out = np.zeros(t.size, np.int64)
    for i, b in enumerate(bits):
        out |= ((t >> i) & 1) << b
    return out


_POPC = np.array([bin(v).count("1") for v in range(1 << NSLOT)], np.int64)


def _popc(a):
    return _POPC[np.asarray(a, np.int64) & ((1 << NSLOT) - 1)]


def _col_costs(B, m0, m1):
    c0 = _popc(m1 & ~B) + _popc(m0 & B)
    c1 = _popc(m0 & ~B) + _popc(m1 & B)
    return c0, c1


def select_reads(reads, n_sites, max_cov=15):
    """step 3 -> bool accepted per read (informative reads only can be accepted)"""
    info = [r for r in range(len(reads)) if len(reads[r]) >= 2]
    order = sorted(info, key=lambda r: (-len(reads[r]), reads[r][0][0], r))
    cov = np.zeros(n_sites, np.int64)
    acc = np.zeros(len(reads), bool)
    for r in order:
        a, b = reads[r][0][0], reads[r][-1][0]
        if cov[a:b + 1].max() < max_cov:
            cov[a:b + 1] += 1
            acc[r] = True
    return acc


def phase(site_pos, reads, max_cov=15):
    """steps 3-7 -> dict: accepted, side (int8 per read, -1 not accepted), site_block (int32, -1 outside blocks), site_h (uint8),
    site_phased (bool), site_ps (int32, 0 unphased), blocks [(first site, last site, ps, cost)]"""
    n_sites = len(site_pos)
    acc = select_reads(reads, n_sites, max_cov)
    span = {r: (reads[r][0][0], reads[r][-1][0]) for r in np.flatnonzero(acc).tolist()}
    # step 4: blocks
    link = np.zeros(max(n_sites - 1, 0), bool)              # link[i]: sites i and i+1 share a block
    covered = np.zeros(n_sites, bool)
    for a, b in span.values():
        link[a:b] = True
        covered[a:b + 1] = True
    site_block = np.full(n_sites, -1, np.int32)
    site_h = np.zeros(n_sites, np.uint8)
    phased = np.zeros(n_sites, bool)
    site_ps = np.zeros(n_sites, np.int32)
    side = np.full(len(reads), -1, np.int8)
    alle = {}
    for r in span:
        for s, a in reads[r]:
            alle[(r, s)] = a
            phased[s] = True
    blocks = []
    i = 0
    while i < n_sites:
        if not covered[i]:
            i += 1
            continue
        j = i
        while j < n_sites - 1 and link[j]:
            j += 1
        blocks.append((i, j))
        i = j + 1
    out_blocks = []
    for bi, (f, l) in enumerate(blocks):
        site_block[f:l + 1] = bi
        rb = sorted(r for r, (a, b) in span.items() if f <= a and b <= l)
        starts = {}
        for r in rb:
            starts.setdefault(span[r][0], []).append(r)
        slot_of, free, ends, active = {}, list(range(NSLOT)), {}, set()
        cols = []
        for c in range(f, l + 1):
            for r in ends.pop(c - 1, []):                       # spans that ended at the previous column free their slots
                free.append(slot_of[r])
                active.discard(r)
            free.sort()
            enter = 0
            for r in starts.get(c, []):                         # read-index order, lowest free slot first
                slot_of[r] = free.pop(0)
                enter |= 1 << slot_of[r]
                ends.setdefault(span[r][1], []).append(r)
                active.add(r)
            act, m0, m1 = 0, 0, 0
            for r in active:
                act |= 1 << slot_of[r]
                v = alle.get((r, c))
                if v == 0:
                    m0 |= 1 << slot_of[r]
                elif v == 1:
                    m1 |= 1 << slot_of[r]
            cols.append((act, act & ~enter, m0, m1))
        # step 6: the DP over the partition masks
        D = np.full(1 << NSLOT, -1, np.int64)
        bts = []
        for k, (act, K, m0, m1) in enumerate(cols):
            B = _subsets(act)
            c0, c1 = _col_costs(B, m0, m1)
            cost = np.minimum(c0, c1)
            if k == 0:
                D[B] = cost
                bts.append(None)
                continue
            Lv = cols[k - 1][0] & ~K
            bk = _subsets(K)
            xl = _subsets(Lv)
            M = D[bk[:, None] | xl[None, :]]
            arg = np.argmin(M, axis=1)                          # first minimum: the smallest leaving-slot bits
            P = np.zeros(1 << NSLOT, np.int64)
            P[bk] = M[np.arange(bk.size), arg]
            bt = np.zeros(1 << NSLOT, np.int64)
            bt[bk] = xl[arg]
            bts.append(bt)
            Dn = np.full(1 << NSLOT, -1, np.int64)
            Dn[B] = P[B & K] + cost
            D = Dn
        B = _subsets(cols[-1][0])
        best = int(B[np.argmin(D[B])])
        total = int(D[best])
        colB = [0] * len(cols)
        for k in range(len(cols) - 1, -1, -1):
            colB[k] = best
            if k:
                K = cols[k][1]
                best = (best & K) | int(bts[k][best & K])
        ps = 0
        for k, (act, K, m0, m1) in enumerate(cols):
            c = f + k
            c0, c1 = _col_costs(np.array([colB[k]]), m0, m1)
            site_h[c] = 0 if c0[0] <= c1[0] else 1
            if phased[c] and ps == 0:
                ps = int(site_pos[c])
        for k in range(len(cols)):
            if phased[f + k]:
                site_ps[f + k] = ps
        for r in rb:
            side[r] = (colB[span[r][0] - f] >> slot_of[r]) & 1
        out_blocks.append((f, l, ps, total))
    return dict(accepted=acc, side=side, site_block=site_block, site_h=site_h, site_phased=phased, site_ps=site_ps, blocks=out_blocks)


def haplotag(reads, groups, res):
    """step 8 -> (hp uint8, ps int32) per name group"""
    n_groups = int(max(groups) + 1) if len(groups) else 0
    tot = [dict() for _ in range(n_groups)]                     # block -> [n phased sites, score]
    for r, g in enumerate(groups):
        for s, a in reads[r]:
            if not res["site_phased"][s]:
                continue
            b = int(res["site_block"][s])
            t = tot[g].setdefault(b, [0, 0])
            t[0] += 1
            t[1] += 1 if a == res["site_h"][s] else -1
    hp = np.zeros(n_groups, np.uint8)
    ps = np.zeros(n_groups, np.int32)
    for g in range(n_groups):
        if not tot[g]:
            continue
        b = min(tot[g], key=lambda b: (-tot[g][b][0], res["blocks"][b][2]))
        sc = tot[g][b][1]
        if sc:
            hp[g] = 1 if sc > 0 else 2
            ps[g] = res["blocks"][b][2]
    return hp, ps


def mec_cost(reads, site_h, side, sites=None):
    """the number of allele disagreements of accepted reads with their part's haplotype (part 0 carries allele site_h)"""
    n = 0
    for r, rd in enumerate(reads):
        if side[r] < 0:
            continue
        for s, a in rd:
            if sites is None or s in sites:
                n += int(a != (site_h[s] ^ side[r]))
    return n


def brute_force_mec(reads, accepted, n_sites):
    """the minimum over every bipartition of the accepted reads of the per-site best haplotype cost"""
    rr = np.flatnonzero(accepted).tolist()
    if not rr:
        return 0
    mat = np.full((len(rr), n_sites), -1, np.int64)
    for i, r in enumerate(rr):
        for s, a in reads[r]:
            mat[i, s] = a
    best = None
    for part in range(1 << len(rr)):
        side = np.array([(part >> i) & 1 for i in range(len(rr))])[:, None]
        c0 = ((mat == 1) & (side == 0)).sum(0) + ((mat == 0) & (side == 1)).sum(0)
        c1 = ((mat == 0) & (side == 0)).sum(0) + ((mat == 1) & (side == 1)).sum(0)
        v = int(np.minimum(c0, c1).sum())
        best = v if best is None else min(best, v)
    return best


def random_instance(rng, n_reads, n_sites, p_err=0.1, max_len=None):
    """reads over a random two-haplotype truth with allele errors and missing alleles"""
    truth = rng.integers(0, 2, n_sites)
    reads, origin = [], []
    max_len = max_len or n_sites
    for _ in range(n_reads):
        a = int(rng.integers(0, n_sites))
        b = min(n_sites - 1, a + int(rng.integers(0, max_len)))
        h = int(rng.integers(0, 2))
        rd = []
        for s in range(a, b + 1):
            if rng.random() < 0.2:
                continue
            al = int(truth[s] ^ h)
            if rng.random() < p_err:
                al ^= 1
            rd.append((s, al))
        reads.append(rd)
        origin.append(h)
    return reads, truth, origin

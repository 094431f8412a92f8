"""Pure-numpy restatement of the phaser's genotype-aware solve (DESIGN.md "Read-based phasing", step 6b: the sites' genotypes are not
trusted), written from the rule's statement and independently of csrc/nc_happhase.hip.  Read selection, the subset enumeration and the
haplotagger are the plain phaser's (tests/phase_ref.py, unchanged); blocks, slots, the DP with its tie-breaks and the outcomes are restated
here.  The tests compare the library with it bit for bit and check it against an exhaustive search on small instances.

An instance is phase_ref's (`reads`: per read a sorted list of (site, allele 0/1)) plus `site_gt`, the called class of every site:
0 = het, 1 = homozygous for the first allele, 2 = homozygous for the second; G >= 1 is the price of leaving the called class.

Column rule, for the active slots' partition B, allele masks m0 / m1:
    het(B) = min(e0, e1) + (gt == 0 ? 0 : G)          e0 = popc(m1 & ~B) + popc(m0 & B), e1 = popc(m0 & ~B) + popc(m1 & B)
    homA   = popc(m1)    + (gt == 1 ? 0 : G)          every read should show the first allele
    homB   = popc(m0)    + (gt == 2 ? 0 : G)
    cost(B) = min(het(B), homA, homB)
Outcome of a column under the traced-back B: the smallest (cost, pref), pref 0 for the called class, else 1 het, 2 homA, 3 homB."""
from __future__ import annotations

import numpy as np

from phase_ref import NSLOT, _col_costs, _popc, _subsets, select_reads


def column_outcomes(c0, c1, m0, m1, gt, G):
    """the three outcomes' costs (het, homA, homB) of one column under one partition -> (cost [3], winner 0 / 1 / 2)"""
    cost = [min(int(c0), int(c1)) + (0 if gt == 0 else G), int(_popc(m1)) + (0 if gt == 1 else G), int(_popc(m0)) + (0 if gt == 2 else G)]
    win = min(range(3), key=lambda o: (cost[o], 0 if o == gt else o + 1))
    return cost, win


def phase_gt(site_pos, reads, site_gt, G=1, max_cov=15):
    """-> dict as phase_ref.phase's, plus site_gt (the outcome per site; outside the blocks the call) -- site_phased needs an accepted allele
    and the outcome het; site_h is set for every column of a block"""
    n_sites = len(site_pos)
    site_gt = np.asarray(site_gt, np.int64)
    acc = select_reads(reads, n_sites, max_cov)
    span = {r: (reads[r][0][0], reads[r][-1][0]) for r in np.flatnonzero(acc).tolist()}
    joined = np.zeros(max(n_sites - 1, 0), bool)
    covered = np.zeros(n_sites, bool)
    has_allele = np.zeros(n_sites, bool)
    for r, (a, b) in span.items():
        joined[a:b] = True
        covered[a:b + 1] = True
        for s, _ in reads[r]:
            has_allele[s] = True
    site_block = np.full(n_sites, -1, np.int32)
    site_h = np.zeros(n_sites, np.uint8)
    out_gt = site_gt.astype(np.uint8).copy()
    phased = np.zeros(n_sites, bool)
    site_ps = np.zeros(n_sites, np.int32)
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
        # slots: a span that ended at the previous column frees its slot; spans starting here take the lowest free slots in read order
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
            for r in active:
                act |= 1 << slot[r]
                for s, a in reads[r]:
                    if s == c:
                        if a == 0:
                            m0 |= 1 << slot[r]
                        else:
                            m1 |= 1 << slot[r]
            cols.append((act, act & ~enter, m0, m1, int(site_gt[c])))
        D, back = None, []
        for k, (act, K, m0, m1, gt) in enumerate(cols):
            B = _subsets(act)
            c0, c1 = _col_costs(B, m0, m1)
            het = np.minimum(c0, c1) + (0 if gt == 0 else G)
            hom_a = int(_popc(m1)) + (0 if gt == 1 else G)
            hom_b = int(_popc(m0)) + (0 if gt == 2 else G)
            cost = np.minimum(het, min(hom_a, hom_b))
            if k == 0:
                Dn = np.full(1 << NSLOT, -1, np.int64)
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
                Dn = np.full(1 << NSLOT, -1, np.int64)
                Dn[B] = P[B & K] + cost
            D = Dn
        B = _subsets(cols[-1][0])
        best = int(B[np.argmin(D[B])])                              # the smallest minimising B of the last column
        total = int(D[best])
        chosen = [0] * len(cols)
        for k in range(len(cols) - 1, -1, -1):
            chosen[k] = best
            if k:
                K = cols[k][1]
                best = (best & K) | int(back[k][best & K])
        for k, (act, K, m0, m1, gt) in enumerate(cols):
            c = f + k
            c0, c1 = _col_costs(np.array([chosen[k]]), m0, m1)
            site_h[c] = 0 if c0[0] <= c1[0] else 1
            out_gt[c] = column_outcomes(c0[0], c1[0], m0, m1, gt, G)[1]
            phased[c] = has_allele[c] and out_gt[c] == 0
        ph = [c for c in range(f, l + 1) if phased[c]]
        ps = int(site_pos[ph[0]]) if ph else 0
        site_ps[ph] = ps
        for r in mine:
            side[r] = (chosen[span[r][0] - f] >> slot[r]) & 1
        blocks.append((f, l, ps, total))
    return dict(accepted=acc, side=side, site_block=site_block, site_h=site_h, site_gt=out_gt, site_phased=phased, site_ps=site_ps, blocks=blocks)


def exhaustive_cost(reads, accepted, n_sites, site_gt, G):
    """the minimum, over every bipartition of the accepted reads and every outcome (het with either orientation, homozygous first, homozygous
    second) of every site, of the allele errors plus G per site whose outcome leaves its called class.  The sites' terms are independent given
    the bipartition, so the minimum over the outcomes is taken site by site."""
    rr = np.flatnonzero(accepted).tolist()
    mat = np.full((len(rr), n_sites), -1, np.int64)
    for i, r in enumerate(rr):
        for s, a in reads[r]:
            mat[i, s] = a
    gt = np.asarray(site_gt)
    n0, n1 = (mat == 0).sum(0), (mat == 1).sum(0)
    hom_a = n1 + np.where(gt == 1, 0, G)
    hom_b = n0 + np.where(gt == 2, 0, G)
    best = None
    for part in range(1 << len(rr)):
        side = np.array([(part >> i) & 1 for i in range(len(rr))], np.int64).reshape(-1, 1)
        e0 = ((mat == 1) & (side == 0)).sum(0) + ((mat == 0) & (side == 1)).sum(0)
        e1 = ((mat == 0) & (side == 0)).sum(0) + ((mat == 1) & (side == 1)).sum(0)
        het = np.minimum(e0, e1) + np.where(gt == 0, 0, G)
        v = int(np.minimum(het, np.minimum(hom_a, hom_b)).sum())
        best = v if best is None else min(best, v)
    return best


def hand_instance():
    """8 reads on two clean haplotypes over 5 sites (reads 0-3 carry the first allele everywhere, reads 4-7 the second), except:
    site 2 is called 1/1 although its alleles split exactly by haplotype; site 3 is called 0/1 although only read 7 shows the second allele.
    -> (site_pos, reads, site_gt)"""
    reads = []
    for r in range(8):
        hap = r // 4
        reads.append([(s, hap if s != 3 else int(r == 7)) for s in range(5)])
    return np.array([100, 200, 300, 400, 500], np.int32), reads, np.array([0, 0, 2, 0, 0], np.uint8)


LETTER = "AGTC"


def world_calls(world, kept, third_every=0):
    """the SNP records a perfect caller would write for a World of phase_realign_ref.make_realign_world: 0/1 at its het sites (REF and the
    other base the kept reads truly carry; every `third_every`-th one as 1/2 with a third base) and 1/1 at its homozygous sites (ALT = the kept
    reads' most frequent base there) -> records in position order"""
    from phase_realign_ref import het_site_alleles, ref_codes
    refc = ref_codes(world.ref)
    pos, al = het_site_alleles(world, kept)
    out = {}
    for k, (p, (a0, a1)) in enumerate(zip(pos.tolist(), al.tolist())):
        if third_every and k % third_every == 3:
            third = [b for b in range(4) if b not in (a0, a1)][k & 1]
            out[p] = "%s\t%d\t.\t%s\t%s,%s\t30.00\tPASS\t.\tGT:GQ\t1/2:30\n" % (world.chrom, p, LETTER[a0], LETTER[a1], LETTER[third])
        else:
            out[p] = "%s\t%d\t.\t%s\t%s\t30.00\tPASS\t.\tGT:GQ\t0/1:30\n" % (world.chrom, p, LETTER[a0], LETTER[a1])
    kept = np.asarray(kept)
    rs, re_ = np.asarray(world.read_start)[kept].astype(np.int64), np.asarray(world.read_end)[kept].astype(np.int64)
    for p in np.asarray(world.hom_sites).tolist():
        rc = int(refc[p - 1])
        over = kept[(rs <= p) & (p < re_)]
        c = world.codes[np.asarray(world.read_off)[over] + (p - np.asarray(world.read_start)[over])]
        cnt = np.bincount(c[c < 4], minlength=4)
        if rc > 3 or p in out or cnt.sum() == 0 or int(np.argmax(cnt)) == rc:
            continue
        out[p] = "%s\t%d\t.\t%s\t%s\t30.00\tPASS\t.\tGT:GQ\t1/1:30\n" % (world.chrom, p, LETTER[rc], LETTER[int(np.argmax(cnt))])
    return [out[p] for p in sorted(out)]


def hom_ref_columns(world, taken, step, rng):
    """about one position per `step` where both haplotypes carry the reference base (no het or homozygous site within 30 columns, none of
    `taken`, REF an upper-case base) -> (positions, alt_of for edit_calls)"""
    from phase_realign_ref import ref_codes
    refc = ref_codes(world.ref)
    near = np.zeros(world.length + 62, bool)
    for p in list(np.asarray(world.het_sites).tolist()) + list(np.asarray(world.hom_sites).tolist()) + [int(t) for t in taken]:
        near[p:p + 61] = True                                          # (index p + 30 is position p)
    out = []
    for lo in range(200, world.length - 200, step):
        p = lo + int(rng.integers(0, step // 2))
        if not near[p + 30] and world.ref[p - 1] in LETTER:
            out.append(p)
    return out, lambda p: (world.ref[p - 1], LETTER[(int(refc[p - 1]) + 1 + p % 3) % 4])


def edit_calls(records, true_het_pos, hom_ref_pos, rng, share_hom=0.1, alt_of=None):
    """the SNP records as a caller with genotype errors would have written them: a share of the true het 0/1 records rewritten to 1/1, and a
    false 0/1 record added at every position of `hom_ref_pos` (REF from alt_of(pos)[0], ALT alt_of(pos)[1]).
    -> (records in position order, positions rewritten to 1/1, positions of the added records)"""
    out, to_hom = [], []
    het = set(int(p) for p in true_het_pos)
    for ln in records:
        f = ln.rstrip("\n").split("\t")
        smp = f[9].split(":")
        if int(f[1]) in het and smp[0] == "0/1" and "," not in f[4] and rng.random() < share_hom:
            f[9] = ":".join(["1/1"] + smp[1:])
            to_hom.append(int(f[1]))
            ln = "\t".join(f) + "\n"
        out.append(ln)
    have = {int(ln.split("\t")[1]) for ln in out}
    chrom = out[0].split("\t")[0]
    added = []
    for p in hom_ref_pos:
        if int(p) in have:
            continue
        ref, alt = alt_of(int(p))
        out.append("%s\t%d\t.\t%s\t%s\t30.000\tPASS\t.\tGT:GQ\t0/1:30\n" % (chrom, int(p), ref, alt))
        added.append(int(p))
    out.sort(key=lambda ln: int(ln.split("\t")[1]))
    return out, to_hom, added

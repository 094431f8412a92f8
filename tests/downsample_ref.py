"""The uniform sample above maxcov (params['downsample'] = 'uniform'), restated for the tests: the rule in plain numpy (independent of
nanocaller_amd.downsample, which it is compared with), the small worlds the GPU tests run, and their yardsticks.

The rule.  mix32(p, s): x = (p * 0x9E3779B1 mod 2^32) ^ s; x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16.
For the pileup at the 1-based column v, set id s (0: SNP pileup / `all`, 1: HP 1, 2: HP 2), n entries in file order and k = maxcov:
base = mix32(v, seed ^ SETC[s]), key(j) = mix32(j, base); n <= k keeps everything, otherwise the k entries of the smallest keys, in pileup order.

The SNP yardstick.  For a site v whose pileup of n reads is deeper than maxcov, the tensor of the sampled form equals the oracle's on a sub-world
made of the reads that do not cover v plus the sampled covering reads, featurised with maxcov >= n and with the full world's neighbour list."""
import copy

import numpy as np

M32 = 0xffffffff
SETC = (0x00000000, 0x68E31DA4, 0xB5297A4D)
SEED = 812
KEEP_MASK = 0xF04                      # flags the SNP and indel steps drop without `supplementary` (unmapped, secondary, QC fail, duplicate, supplementary)


def mix32(p, seed):
    """on Python ints: no overflow to think about"""
    x = ((int(p) & M32) * 0x9E3779B1 & M32) ^ (int(seed) & M32)
    x ^= x >> 16
    x = x * 0x85EBCA6B & M32
    x ^= x >> 13
    x = x * 0xC2B2AE35 & M32
    x ^= x >> 16
    return x


def mix32_vec(p, seed):
    """the same on an int64 array (products taken in uint64 and masked: 32 x 32 bits never overflow 64)"""
    x = ((np.asarray(p, np.int64) & M32).astype(np.uint64) * np.uint64(0x9E3779B1) & np.uint64(M32)) ^ np.uint64(int(seed) & M32)
    x ^= x >> np.uint64(16)
    x = x * np.uint64(0x85EBCA6B) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = x * np.uint64(0xC2B2AE35) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def keys(seed, pos, set_id, n):
    return mix32_vec(np.arange(n, dtype=np.int64), mix32(pos, (seed ^ SETC[set_id]) & M32))


def sample(seed, pos, set_id, n, k):
    """ordinals of the sampled entries, ascending (a full stable sort: no partition tricks shared with the module under test)"""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.argsort(keys(seed, pos, set_id, n), kind="stable")[:k]).astype(np.int64)


def sharp(seed, pos, set_id, n, k):
    """the uniform sample of this pileup is not its first k entries"""
    return n > k and not np.array_equal(sample(seed, pos, set_id, n, k), np.arange(k))


# ---------------------------------------------------------------------------------------------------------------- worlds
def _world(ref_codes, starts, ends, rng, het_every, sub=0.04, dele=0.04, flags=None):
    """reads [start, end) over a reference given as codes: every het_every-th column is heterozygous (a read carries the alternative base by the parity
    of its index draw), plus substitutions and deletions (code 4) at the given rates; reads in start order"""
    from nanocaller_amd.synth import World
    order = np.argsort(starts, kind="stable")
    starts, ends = np.asarray(starts, np.int32)[order], np.asarray(ends, np.int32)[order]
    L = ref_codes.size
    het = np.zeros(L + 2, bool)
    het[het_every::het_every] = True
    parts = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        c = ref_codes[s - 1:e - 1].copy()
        if rng.random() < 0.5:
            h = het[s:e]
            c[h] = (c[h] + 1) & 3
        u = rng.random(c.size)
        c[u < sub] = rng.integers(0, 4, int((u < sub).sum()), dtype=np.uint8)
        c[(u >= sub) & (u < sub + dele)] = 4
        c[0] = ref_codes[s - 1]                                          # (a read neither starts nor ends deleted)
        c[-1] = ref_codes[e - 2]
        parts.append(c)
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=off[1:])
    R = len(parts)
    fl = np.where(rng.random(R) < 0.5, 16, 0).astype(np.int32) if flags is None else np.asarray(flags, np.int32)[order]
    return World(chrom="chrS", ref="".join("AGTC"[c] for c in ref_codes), read_start=starts, read_end=ends, read_flag=fl, read_off=off,
                 codes=np.concatenate(parts).astype(np.uint8), names=["s%05d" % i for i in range(R)])


STAIR_LO, STAIR_R = 100, 340           # the first read starts at column STAIR_LO, one read per column, STAIR_R reads
_cache = {}


def staircase_world():
    """One read starts per column of [STAIR_LO, STAIR_LO + STAIR_R) and all end behind the stretch: the pileup at column STAIR_LO + i is the first
    i + 1 reads, so the depth passes through every value 1 .. STAIR_R"""
    if "stair" not in _cache:
        rng = np.random.Generator(np.random.PCG64(20))
        L = STAIR_LO + STAIR_R + 900
        ref = rng.integers(0, 4, L, dtype=np.uint8)
        starts = STAIR_LO + np.arange(STAIR_R)
        ends = STAIR_LO + STAIR_R + 300 + rng.integers(0, 500, STAIR_R)
        _cache["stair"] = _world(ref, starts, ends, rng, het_every=23)
    return _cache["stair"]


def stair_col(depth):
    return STAIR_LO + depth - 1


MIXED_MAXCOV = 100


def mixed_world():
    """600 reads over 6 kb with starts all over and lengths from 300 to 4000: at a column of its middle the covering reads (250 and more) are
    spread over several 64-entry steps of the tile's entries, with reads that ended before the column between them; the columns around the tile
    edges (2048 and 4096 columns into the pack's grid, whichever the pack chose) are deep as well"""
    if "mixed" not in _cache:
        rng = np.random.Generator(np.random.PCG64(21))
        L = 6600
        ref = rng.integers(0, 4, L, dtype=np.uint8)
        starts = rng.integers(50, 5200, 600)
        ends = np.minimum(starts + rng.integers(300, 4000, 600), L - 20)
        # a few reads the steps drop: they take no place in the pileup and so none among the ordinals
        flags = np.where(rng.random(600) < 0.5, 16, 0) | np.where(rng.random(600) < 0.05, 0x100, 0)
        _cache["mixed"] = _world(ref, starts, ends, rng, het_every=41, flags=flags)
    return _cache["mixed"]


def pileup(world, v):
    """indices of the kept reads that cover v, in file order"""
    keep = (world.read_flag & KEEP_MASK) == 0
    return np.flatnonzero(keep & (world.read_start <= v) & (v < world.read_end))


def sub_world(world, reads):
    """the world with only `reads` (ascending indices)"""
    reads = np.asarray(reads, np.int64)
    w = copy.copy(world)
    w.read_start, w.read_end, w.read_flag = world.read_start[reads], world.read_end[reads], world.read_flag[reads]
    w.names = [world.names[r] for r in reads]
    off = np.asarray(world.read_off, np.int64)
    lens = off[reads + 1] - off[reads]
    w.read_off = np.zeros(reads.size + 1, np.int64)
    np.cumsum(lens, out=w.read_off[1:])
    w.codes = world.codes[np.arange(int(w.read_off[-1]), dtype=np.int64) + np.repeat(off[reads] - w.read_off[:-1], lens)]
    w.meta = {}
    w.hap = None
    return w


def sampled_world(world, v, seed, maxcov, set_id=0):
    """(sub-world of the reads that do not cover v plus the sampled covering ones, n = the pileup's depth, the sampled reads)"""
    cov = pileup(world, v)
    chosen = cov[sample(seed, v, set_id, cov.size, maxcov)]
    drop = np.setdiff1d(cov, chosen)
    return sub_world(world, np.setdiff1d(np.arange(world.n_reads), drop)), int(cov.size), chosen


def snp_yardstick(world, rc, nbr, v, seed, maxcov, seq="ont"):
    """-> (tensor float32 [5, 41, 5], fwd_dp [4], rev_dp [4], site_depth) of the site v under the uniform sample"""
    from oracle import oracle
    sub, n, _ = sampled_world(world, v, seed, maxcov)
    big = max(n, maxcov) + 1
    pos, _, mat, _, _, dep = oracle.snp_featurize(sub, rc, nbr, np.array([v], np.int32), seq, big, 1)
    assert pos.size == 1 and int(dep[0]) == min(n, maxcov)
    _, _, _, fwd, rev, _ = oracle.snp_featurize(world, rc, nbr, np.array([v], np.int32), seq, big, 1)
    return mat[0], fwd[0], rev[0], min(n, maxcov)


def world_nbr(world, mincov=1):
    """(reference codes, the world's neighbour sites) by the oracle's scan"""
    from oracle import oracle
    rc = oracle.ref_codes_with_exclusions(world)
    nbr, _, _, _ = oracle.snp_scan(world, rc, 1, world.length - 1, "diploid", mincov, 0.15, [0.3, 0.7])
    return rc, nbr


def sharp_seed(world, v, maxcov, set_id=0):
    """the first seed from 812 on under which the site's sample is not its first maxcov reads (812 itself at most sites)"""
    n = pileup(world, v).size
    for seed in range(SEED, SEED + 64):
        if sharp(seed, v, set_id, n, maxcov):
            return seed
    raise AssertionError("no seed makes the site at %d sharp" % v)


STAIR_MAXCOVS_PAIRS = (1, 63, 64, 65, 160, 255)      # through k_featurize_pairs (int16 tensors, maxcov <= 255)
STAIR_MAXCOVS_WALK = (256, 300)                      # through k_featurize


def stair_seed(maxcov):
    """the seed of the staircase runs at this maxcov: the one that makes the site of depth maxcov + 1 sharp"""
    return sharp_seed(staircase_world(), stair_col(maxcov + 1), maxcov)


def stair_sites():
    return np.arange(STAIR_LO, STAIR_LO + STAIR_R, dtype=np.int64)


def sharp_sites(world, sites, seed, maxcov):
    return [int(v) for v in sites if sharp(seed, int(v), 0, pileup(world, int(v)).size, maxcov)]


def deleted_in_and_out(world, v, seed, maxcov):
    """(reads deleted at v inside the sample, outside it)"""
    cov = pileup(world, v)
    centre = np.array([world.codes[world.read_off[r] + v - int(world.read_start[r])] for r in cov])
    inside = np.zeros(cov.size, bool)
    inside[sample(seed, v, 0, cov.size, maxcov)] = True
    return int(((centre == 4) & inside).sum()), int(((centre == 4) & ~inside).sum())


def tile_grid(world):
    """(tile_pos0, tile_size) of the pack the device tests upload for this world"""
    from nanocaller_amd.wire import build_wire_from_world
    wp = build_wire_from_world(world)
    return int(wp.tile_pos0), int(wp.tile_size)


def mixed_sites(world):
    """(the columns the mixed world's tests list, those of them that are the last column of a tile or the first of the next)"""
    p0, ts = tile_grid(world)
    edges = [c for t in range(1, 8) for c in (p0 + t * ts - 1, p0 + t * ts) if 1500 <= c <= 4500]
    return np.array(sorted(set(range(2600, 2640)) | set(edges)), np.int64), edges


GOLDEN_REGION = dict(ont=(20_000, 26_000), deep=(20_000, 23_000))


def golden_sites(name):
    """(the golden world, its candidate sites deeper than 8 reads in a short region, by the oracle's scan)"""
    from oracle import oracle
    from util import load_world
    w = load_world(name)
    rc = oracle.ref_codes_with_exclusions(w)
    lo, hi = GOLDEN_REGION[name]
    _, cpos, _, _ = oracle.snp_scan(w, rc, lo, hi, "diploid", 4, 0.15, [0.4, 0.6])
    return w, np.array([int(v) for v in cpos if pileup(w, int(v)).size > 8], np.int64)


# ---------------------------------------------------------------------------------------------------------------- indel worlds and yardstick
# "listed": the world of the listed-sites tests (indel_genotype_ref.listed_world: 30 kb at depth 26, haplotagged, with an unphased block over
# 20,000 .. 24,000 where most reads lose their HP tag).  "deep": the same kind at 12 kb and depth 90, where a pileup alone is longer than a 64-entry
# step of its tile.  The anchors are forced with a list of columns that alone decides (genotype_indel_only), 115 columns apart.
INDEL_BASE = dict(mincov=4, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6)
INDEL_CASES = dict(dip=dict(world="listed", chunks=[(1_000, 6_000), (6_000, 11_000), (19_000, 24_500)], haploid=False),
                   hap=dict(world="listed", chunks=[(1_000, 6_000)], haploid=True),
                   deep=dict(world="deep", chunks=[(2_000, 6_000)], haploid=False))
INDEL_MAXCOVS = (4, 8)
INDEL_WINDOW_AFTER = 160


def indel_world(wname):
    if ("indel_world", wname) not in _cache:
        import bamio
        import indel_genotype_ref as R
        _cache[("indel_world", wname)] = R.listed_world() if wname == "listed" else bamio.make_pass2_world(seed=12, length=12_000, depth=90)
    return _cache[("indel_world", wname)]


def indel_listed(case):
    cols = np.concatenate([np.arange(a + 100, b - 100, 115) for a, b in case["chunks"]])
    return cols.astype(np.int64), np.zeros(cols.size, np.uint8)


def indel_host(wname):
    """the kept records of the world in file order, with their first and last column, haplotype and phase set"""
    if ("indel_host", wname) not in _cache:
        import bamio
        w = indel_world(wname)
        all_recs = bamio.world_to_records(w, None)
        recs = [rc for rc in all_recs if not rc["flag"] & KEEP_MASK]
        beg = np.array([rc["pos0"] + 1 for rc in recs])
        end = beg + np.array([sum(n for op, n in rc["cigar"] if op in "MDN=X") for rc in recs])
        _cache[("indel_host", wname)] = dict(w=w, all_recs=all_recs, recs=recs, beg=beg, end=end, hap=np.array([rc["tags"].get("HP", 0) for rc in recs]),
                                             ps=np.array([rc["tags"].get("PS", 0) for rc in recs]))
    return _cache[("indel_host", wname)]


def indel_anchors(name):
    """[(chunk, anchor, type)] that the listed columns of the case force, by the yardstick's pass 1 (indel_genotype_ref.scan_listed)"""
    if ("anchors", name) not in _cache:
        import indel_genotype_ref as R
        case = INDEL_CASES[name]
        w = indel_world(case["world"])
        S = R.as_dict(*indel_listed(case))
        out = []
        for ci, (a, b) in enumerate(case["chunks"]):
            v, _, _ = R.scan_listed(w, a, b, exclude=[], haploid=case["haploid"], impute=False, sites=S, only=True, **INDEL_BASE)
            out += [(ci, an, v[an]) for an in R.pass2_range(v, a, b, INDEL_BASE["win_size"])]
        _cache[("anchors", name)] = out
    return _cache[("anchors", name)]


def indel_sets(name, an):
    """[(set id, record indices in file order)] of the anchor's pileup: haploid [(0, all)]; diploid [(1, HP 1), (2, HP 2), (0, all)] in the tensor's order"""
    h = indel_host(INDEL_CASES[name]["world"])
    ids = np.flatnonzero((h["beg"] <= an) & (h["end"] > an))
    if INDEL_CASES[name]["haploid"]:
        return [(0, ids)]
    return [(1, ids[h["hap"][ids] == 1]), (2, ids[h["hap"][ids] == 2]), (0, ids)]


def indel_kept(name, an, mincov=4):
    """the set-size tests of :48 / :345 on min(n, maxcov): with maxcov >= mincov they do not depend on maxcov; and the window test of :325-327"""
    w = indel_world(INDEL_CASES[name]["world"])
    if any(c not in "AGTC" for c in w.ref[an - 1:min(w.length, an + INDEL_WINDOW_AFTER)]):
        return False
    n = [ids.size for _, ids in indel_sets(name, an)]
    return n[0] >= mincov if len(n) == 1 else (n[0] >= 2 and n[1] >= 2 and n[2] >= mincov)


def indel_set_task(name, an, set_id, ids, seed, maxcov):
    """oracle_pool's task for one read set under the uniform sample: the records of the set's sample as one haploid site"""
    import oracle_pool
    h = indel_host(INDEL_CASES[name]["world"])
    chosen = ids[sample(seed, an, set_id, ids.size, maxcov)]
    return oracle_pool.site_task(an, [h["recs"][i] for i in chosen], np.zeros(chosen.size, int), np.zeros(chosen.size, int), h["w"].ref,
                                 INDEL_WINDOW_AFTER, 1, 1 << 20, haploid=True, band=True)


def indel_first_hp1_ps(name, an):
    h = indel_host(INDEL_CASES[name]["world"])
    ids = indel_sets(name, an)[0][1]
    return int(h["ps"][ids[0]]) if ids.size else 0


def indel_classes(name, maxcov, seed=SEED):
    """per kept anchor of the case: (anchor, {set id: 'sharp' | 'deep' (sampled, but the sample is the first maxcov) | 'whole'})"""
    out = []
    for _, an, _ in indel_anchors(name):
        if indel_kept(name, an):
            out.append((an, {s: ("sharp" if sharp(seed, an, s, ids.size, maxcov) else "deep" if ids.size > maxcov else "whole")
                             for s, ids in indel_sets(name, an)}))
    return out


def indel_spans_a_step(name, an, maxcov, seed=SEED):
    """the `all` sample of the anchor takes ordinals 64 or more apart: entries of different 64-entry steps wherever the pileup starts in its tile"""
    ids = indel_sets(name, an)[-1][1]
    ch = sample(seed, an, 0, ids.size, maxcov)
    return ch.size > 1 and int(ch[-1] - ch[0]) >= 64

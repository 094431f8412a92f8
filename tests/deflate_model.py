"""The device DEFLATE writer (k_deflate, csrc/nc_bamwrite.hip) restated in plain Python / numpy: the writer's specification (DESIGN.md
section 13).  The kernel is deterministic -- candidates are read before a batch's heads are updated, its integer atomics do not depend on
their order, frequency ties are broken by symbol index -- so `deflate_model(member)` predicts its payload byte for byte, and returns next to
it what a test needs to prove that a crafted input reached the edge it was built for.  No GPU, no torch.

  LZ77      hash of p = (le32(p) * 2654435761 mod 2^32) >> 20, only for p + 4 <= len; positions are taken in batches of 1,024; the candidate of
            p is the latest position of an EARLIER batch in p's bucket, and only at a distance <= 32,768.
  parse     segment k = positions [32k, 32k + 32): greedy from 32k on, a match where the candidate agrees on >= 4 bytes (at most
            min(258, len - p)), a literal otherwise, until the position passes the segment's end.
  join      segment k's entry = the largest end of the segments before it.  A token that ends at or before the entry is dropped, one that
            starts at or behind it is kept, the one that straddles it keeps its tail: a match of the same distance when >= 3 bytes are
            left, literals otherwise.
  codes     frequencies (+ 1 end of block; an alphabet with fewer than two used symbols gets a second); symbols ranked by (frequency,
            index); minimum-redundancy lengths (ties: a leaf before an internal node), limited to 15 bits (7 for the code-length code) by
            moving counts up until Kraft's sum is one; the longest codes to the lowest ranks; canonical codes (RFC 1951 3.2.2).
  block     one dynamic block (BFINAL), code lengths run-length coded with zlib's symbols (zeros in chunks <= 138, others <= 6); a
            stored block when the dynamic one would have >= len + 5 bytes; `03 00` for an empty member."""
import heapq

import numpy as np

BGZF_MAX = 0xff00
BATCH, SEG, HALF = 1024, 32, 32768
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# RFC 1951 3.2.5: (base, extra bits) of the length codes 257.. and of the distance codes
LEN_TAB = [(3 + i, 0) for i in range(8)]
for _e in range(1, 6):
    for _i in range(4):
        LEN_TAB.append((LEN_TAB[-1][0] + (1 << LEN_TAB[-1][1]), _e))
LEN_TAB.append((258, 0))
DIST_TAB = [(1 + i, 0) for i in range(4)]
for _e in range(1, 14):
    for _i in range(2):
        DIST_TAB.append((DIST_TAB[-1][0] + (1 << DIST_TAB[-1][1]), _e))
LEN_CODE = np.zeros(259, np.int64)
for _c, (_b, _e) in enumerate(LEN_TAB):
    LEN_CODE[_b:min(259, _b + (1 << _e))] = _c
LEN_CODE[258] = 28
DIST_BASES = np.array([b for b, _ in DIST_TAB], np.int64)


def dist_code(d):
    return int(np.searchsorted(DIST_BASES, d, side="right")) - 1


def candidates(a):
    """distance of every position's candidate (0: none)"""
    n = a.size
    cand = np.zeros(n, np.int64)
    if n < 4:
        return cand, np.zeros(0, np.uint32)
    b = a.astype(np.uint64)
    v = b[:n - 3] | b[1:n - 2] << np.uint64(8) | b[2:n - 1] << np.uint64(16) | b[3:] << np.uint64(24)
    hv = (((v * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
    heads = np.full(4096, -1, np.int64)
    for bat in range(0, n - 3, BATCH):
        ps = np.arange(bat, min(bat + BATCH, n - 3))
        c = heads[hv[ps]]
        d = ps - c
        cand[ps] = np.where((c >= 0) & (d <= MAX_DIST), d, 0)
        np.maximum.at(heads, hv[ps], ps)
    return cand, v.astype(np.uint32)


def parse(a, cand, v):
    """every segment's greedy parse: ([tokens of segment k], end of segment k, matches that the member's end cut short); a token is a byte
    or (length, distance)"""
    n = a.size
    segs, ends, clipped = [], [], 0
    lit = a.tolist()
    cd = cand.tolist()
    for s in range(0, n, SEG):
        e = min(s + SEG, n)
        p, toks = s, []
        while p < e:
            d = cd[p]
            ln = 0
            if d and v[p] == v[p - d]:
                m = min(MAX_MATCH, n - p)
                ne = np.flatnonzero(a[p:p + m] != a[p - d:p - d + m])
                ln = int(ne[0]) if ne.size else m
            if ln >= MIN_MATCH:
                toks.append((ln, d))
                clipped += ln == n - p < MAX_MATCH
                p += ln
            else:
                toks.append(lit[p])
                p += 1
        segs.append(toks)
        ends.append(p)
    return segs, ends, clipped


def join(a, segs, ends):
    """-> tokens [(position, token)], cuts that stayed matches, cuts that became literals"""
    out, cut_match, cut_lit, entry = [], 0, 0, 0
    for k, toks in enumerate(segs):
        p = k * SEG
        for t in toks:
            te = p + (t[0] if isinstance(t, tuple) else 1)
            if te > entry:
                if p >= entry:
                    out.append((p, t))
                elif te - entry >= 3:
                    out.append((entry, (te - entry, t[1])))
                    cut_match += 1
                else:
                    out.extend((q, int(a[q])) for q in range(entry, te))
                    cut_lit += 1
            p = te
        entry = max(entry, ends[k])
    return out, cut_match, cut_lit


def ranked(freq):
    """used symbols by ascending (frequency, index)"""
    return sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))


def unlimited_depths(weights):
    """leaf depths of the Huffman tree over `weights` (ascending), by a heap: of equal weights a leaf goes before an internal node, an
    earlier node before a later one.  -> depth of every leaf"""
    n = len(weights)
    if n == 1:
        return [1]
    heap = [(w, i) for i, w in enumerate(weights)]
    heapq.heapify(heap)
    parent = {}
    nxt = n
    while len(heap) > 1:
        w0, i0 = heapq.heappop(heap)
        w1, i1 = heapq.heappop(heap)
        parent[i0] = parent[i1] = nxt
        heapq.heappush(heap, (w0 + w1, nxt))
        nxt += 1
    depth = {nxt - 1: 0}
    for i in range(nxt - 2, -1, -1):
        depth[i] = depth[parent[i]] + 1
    return [depth[i] for i in range(n)]


def min_redundancy_counts(weights):
    """codes per length of a minimum-redundancy code over `weights` (ascending): two queues, the leaves and the internal nodes in the order
    they were made; the lighter front is taken, the leaf on a tie.  -> {length: count}"""
    n = len(weights)
    made, par = [], []                                 # internal nodes: weight, parent (index into made)
    leaf_par = [0] * n
    li = ii = 0
    for _ in range(n - 1):
        w = 0
        me = len(made)
        for _pick in range(2):
            if li < n and (ii >= me or weights[li] <= made[ii]):
                w += weights[li]
                leaf_par[li] = me
                li += 1
            else:
                w += made[ii]
                par[ii] = me
                ii += 1
        made.append(w)
        par.append(-1)
    depth = [0] * len(made)
    for i in range(len(made) - 2, -1, -1):
        depth[i] = depth[par[i]] + 1
    counts = {}
    for i in range(n):
        d = depth[leaf_par[i]] + 1
        counts[d] = counts.get(d, 0) + 1
    return counts


def limit_counts(counts, maxbits):
    """codes per length with no length above maxbits: the longer ones are counted at maxbits, then, while Kraft's sum is too large, one code
    leaves maxbits and the deepest shorter length gives one code up for two of the next length"""
    num = [0] * (maxbits + 1)
    for ln, c in counts.items():
        num[min(ln, maxbits)] += c
    total = sum(num[ln] << (maxbits - ln) for ln in range(1, maxbits + 1))
    while total != 1 << maxbits:
        num[maxbits] -= 1
        for ln in range(maxbits - 1, 0, -1):
            if num[ln]:
                num[ln] -= 1
                num[ln + 1] += 2
                break
        total -= 1
    return num


def code_lengths(freq, maxbits):
    """-> (limited length of every symbol, depth of the unlimited tree)"""
    order = ranked(freq)
    lens = [0] * len(freq)
    if not order:
        return lens, 0
    if len(order) == 1:
        lens[order[0]] = 1
        return lens, 1
    w = [int(freq[s]) for s in order]
    counts = min_redundancy_counts(w)
    deep = unlimited_depths(w)
    hist = {}
    for d in deep:
        hist[d] = hist.get(d, 0) + 1
    assert hist == counts, (hist, counts)              # the two constructions agree on the unlimited code
    num = limit_counts(counts, maxbits)
    i = 0
    for ln in range(maxbits, 0, -1):
        for _ in range(num[ln]):
            lens[order[i]] = ln
            i += 1
    return lens, max(deep)


def canonical(lens):
    """RFC 1951 3.2.2 -> code of every symbol (most significant bit first)"""
    mx = max(lens) if lens else 0
    cnt = [0] * (mx + 2)
    for ln in lens:
        if ln:
            cnt[ln] += 1
    nxt, code = [0] * (mx + 2), 0
    for ln in range(1, mx + 1):
        code = (code + cnt[ln - 1]) << 1
        nxt[ln] = code
    out = []
    for ln in lens:
        out.append(nxt[ln] if ln else 0)
        if ln:
            nxt[ln] += 1
    return out


def run_length_ops(lens):
    """zlib's code-length symbols: [(symbol, repeat count or 0)]"""
    ops, i = [], 0
    while i < len(lens):
        cur, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == cur:
            run += 1
        i += run
        if cur == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r))
                run -= r
            if run >= 3:
                ops.append((17, run))
                run = 0
        else:
            ops.append((cur, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
        ops.extend([(cur, 0)] * run)
    return ops


def _rev(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


def pack_bits(vals, nbits):
    """fields of <= 16 bits, each least significant bit first, one behind the other -> (bytes, number of bits)"""
    vals = np.asarray(vals, np.uint64)
    nbits = np.asarray(nbits, np.int64)
    off = np.concatenate([[0], np.cumsum(nbits)])
    total = int(off[-1])
    out = np.zeros((total + 7) // 8 + 3, np.uint8)
    sh = vals << (off[:-1] & 7).astype(np.uint64)
    at = off[:-1] >> 3
    for k in range(3):
        np.bitwise_or.at(out, at + k, ((sh >> np.uint64(8 * k)) & np.uint64(0xff)).astype(np.uint8))
    return out[:(total + 7) // 8].tobytes(), total


def deflate_model(member):
    """-> (payload, info) of one member (bytes, at most 0xff00)"""
    member = bytes(member)
    n = len(member)
    if n > BGZF_MAX:
        raise ValueError("a member has at most 0xff00 bytes")
    if n == 0:
        return b"\x03\x00", dict(tokens=[], stored=False, empty=True)
    a = np.frombuffer(member, np.uint8)
    cand, v = candidates(a)
    segs, ends, clipped = parse(a, cand, v)
    tokens, cut_match, cut_lit = join(a, segs, ends)

    fll, fd = [0] * 286, [0] * 30
    for _, t in tokens:
        if isinstance(t, tuple):
            fll[257 + int(LEN_CODE[t[0]])] += 1
            fd[dist_code(t[1])] += 1
        else:
            fll[t] += 1
    fll[256] = 1
    if sum(1 for f in fll if f) < 2:
        fll[0] = 1
    used = sum(1 for f in fd if f)
    if used < 2:
        if not fd[0]:
            fd[0] = 1
        else:
            fd[1] = 1
    if used == 0:
        fd[1] = 1
    lll, deep_ll = code_lengths(fll, 15)
    ld, deep_d = code_lengths(fd, 15)
    hlit, hdist = 286, 30
    while hlit > 257 and not lll[hlit - 1]:
        hlit -= 1
    while hdist > 1 and not ld[hdist - 1]:
        hdist -= 1
    ops = run_length_ops(lll[:hlit] + ld[:hdist])
    fc = [0] * 19
    for s, _ in ops:
        fc[s] += 1
    if sum(1 for f in fc if f) < 2:
        if not fc[0]:
            fc[0] = 1
        else:
            fc[1] = 1
    lc, deep_c = code_lengths(fc, 7)
    hclen = 19
    while hclen > 4 and not lc[CL_ORDER[hclen - 1]]:
        hclen -= 1
    cll, cd, cc = canonical(lll), canonical(ld), canonical(lc)
    rll = [_rev(c, ln) for c, ln in zip(cll, lll)]
    rd = [_rev(c, ln) for c, ln in zip(cd, ld)]
    rc = [_rev(c, ln) for c, ln in zip(cc, lc)]

    vals, nb = [1 | 2 << 1, hlit - 257, hdist - 1, hclen - 4], [3, 5, 5, 4]
    for s in CL_ORDER[:hclen]:
        vals.append(lc[s])
        nb.append(3)
    for s, r in ops:
        vals.append(rc[s])
        nb.append(lc[s])
        if s >= 16:
            vals.append(r - (3, 3, 11)[s - 16])
            nb.append((2, 3, 7)[s - 16])
    for _, t in tokens:
        if isinstance(t, tuple):
            c = int(LEN_CODE[t[0]])
            vals.append(rll[257 + c])
            nb.append(lll[257 + c])
            if LEN_TAB[c][1]:
                vals.append(t[0] - LEN_TAB[c][0])
                nb.append(LEN_TAB[c][1])
            c = dist_code(t[1])
            vals.append(rd[c])
            nb.append(ld[c])
            if DIST_TAB[c][1]:
                vals.append(t[1] - DIST_TAB[c][0])
                nb.append(DIST_TAB[c][1])
        else:
            vals.append(rll[t])
            nb.append(lll[t])
    vals.append(rll[256])
    nb.append(lll[256])
    dyn, _ = pack_bits(vals, nb)
    stored = len(dyn) >= n + 5
    payload = bytes([1, n & 0xff, n >> 8, ~n & 0xff, (~n >> 8) & 0xff]) + member if stored else dyn
    matches = [(p, t) for p, t in tokens if isinstance(t, tuple)]
    info = dict(tokens=tokens, cut_match=cut_match, cut_lit=cut_lit, end_clipped=clipped, n_match=len(matches),
                max_len=max((t[0] for _, t in matches), default=0), max_dist=max((t[1] for _, t in matches), default=0),
                depth_ll=deep_ll, depth_d=deep_d, depth_cl=deep_c, lens_ll=lll, lens_d=ld, lens_cl=lc, hlit=hlit, hdist=hdist, hclen=hclen,
                ops={(s, r) for s, r in ops if s >= 16}, cl_hist={s: f for s, f in enumerate(fc) if f},
                stored=stored, dyn_bytes=len(dyn), empty=False)
    return payload, info

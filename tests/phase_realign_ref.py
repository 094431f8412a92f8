"""Numpy / plain-Python restatement of the phaser's allele detection by local realignment (DESIGN.md "Read-based phasing", the allele
detectors; csrc/nc_happhase.hip k_hr_*), independent of the kernel: windows built column by column, a textbook dynamic-programming
Levenshtein distance, no bit vectors.  Also the column rule (k_hp_gather) for comparison, and the worlds the tests run both on: reads whose
indel errors sit next to het SNPs with the gap placed a few columns away from the error, as long-read aligners leave them.

The rule, for a kept read r and a site at 1-based position p with alleles (a0, a1), overhang W = 10:
  1. reference window: columns lo = max(1, p - W) .. hi = min(L, p + W); H0 / H1 = its bases with the one at p replaced by a0 / a1
  2. query window: the read's bases on those columns in order, each followed by the bases the read inserts behind that column when the
     column is not the window's last; columns the read deletes are left out (a read's N stays: it matches no base)
  3. an entry only when rd_start <= lo and hi < rd_end (rd_end exclusive) and no window base is outside ACGT (either letter case)
  4. d0, d1 = Levenshtein(query, H0 / H1); allele 0 when d0 < d1, 1 when d1 < d0, none when equal; none when the query is longer than 64
"""
import numpy as np

W = 10
QMAX = 64
_ASCII2CODE = np.full(256, 4, np.uint8)
for _k, _b in enumerate("AGTC"):
    _ASCII2CODE[ord(_b)] = _ASCII2CODE[ord(_b.lower())] = _k


def ref_codes(ref: str) -> np.ndarray:
    """A0 G1 T2 C3 whatever the case, 4 otherwise; position p at index p - 1"""
    return _ASCII2CODE[np.frombuffer(ref.encode("ascii"), np.uint8)]


def levenshtein(a, b) -> int:
    """unit-cost global edit distance, the full matrix row by row"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        prev = cur
    return prev[len(b)]


def query_window(codes, rs, events, lo, hi):
    """codes: the read's code per column from rs on; events: [(pos, len, inserted codes)] with the marker on the column BEFORE the inserted /
    deleted bases -> the read's bases over columns lo .. hi"""
    deleted = set()
    ins = {}
    for pos, ln, bases in events:
        if ln < 0:
            deleted.update(range(pos + 1, pos + 1 - ln))
        elif ln > 0:
            ins.setdefault(pos, []).extend(int(c) for c in bases)
    q = []
    for x in range(lo, hi + 1):
        if x not in deleted:
            q.append(int(codes[x - rs]))
        if x < hi:
            q.extend(ins.get(x, []))
    return q


def realign_allele(refc, p, a0, a1, rs, re_, codes, events):
    """-> 0, 1 or None for one (read, site) pair; refc = ref_codes(contig)"""
    L = len(refc)
    lo, hi = max(1, p - W), min(L, p + W)
    if not (rs <= lo and hi < re_):
        return None
    win = [int(c) for c in refc[lo - 1:hi]]
    if any(c > 3 for c in win) or a0 > 3 or a1 > 3:
        return None
    q = query_window(codes, rs, events, lo, hi)
    if len(q) > QMAX:
        return None
    h0, h1 = list(win), list(win)
    h0[p - lo], h1[p - lo] = int(a0), int(a1)
    d0, d1 = levenshtein(q, h0), levenshtein(q, h1)
    return 0 if d0 < d1 else (1 if d1 < d0 else None)


def world_events(world, r):
    """read r's events of a World decorated with meta['events'] (+ meta['ev_ins'], ASCII letters) as query_window takes them"""
    ev_off, ev_pos, ev_len = world.meta["events"]
    ins_off, ins_bases = world.meta.get("ev_ins", (None, None))
    out = []
    for k in range(int(ev_off[r]), int(ev_off[r + 1])):
        b = _ASCII2CODE[np.asarray(ins_bases[ins_off[k]:ins_off[k + 1]], np.uint8)] if ins_off is not None and ev_len[k] > 0 else []
        out.append((int(ev_pos[k]), int(ev_len[k]), b))
    return out


def entries(world, kept, pos, alleles, rule):
    """per kept read (World indices `kept`, pack order) its [(site index, allele)] by `rule` = 'realign' or 'column'; candidates are the sites
    inside [read_start, read_end)"""
    refc = ref_codes(world.ref)
    pos = np.asarray(pos, np.int64)
    out = []
    for r in np.asarray(kept).tolist():
        rs, re_ = int(world.read_start[r]), int(world.read_end[r])
        codes = world.read_codes(r)
        ev = world_events(world, r) if rule == "realign" else None
        a, b = np.searchsorted(pos, rs), np.searchsorted(pos, re_)
        rd = []
        for s in range(a, b):
            p, a0, a1 = int(pos[s]), int(alleles[s][0]), int(alleles[s][1])
            if rule == "realign":
                al = realign_allele(refc, p, a0, a1, rs, re_, codes, ev)
            else:
                c = int(codes[p - rs])
                al = 0 if c == a0 else (1 if c == a1 else None)
            if al is not None:
                rd.append((s, al))
        out.append(rd)
    return out


def compare_rules(col, rea, truth=None):
    """counts over the (read, site) pairs where either rule has an entry: pairs, differing pairs, entries only the realignment has, entries
    only the column has, alleles that differ; with truth (per read {site: allele}): wrong column alleles the realignment corrects"""
    n = diff = gained = lost = flipped = corrected = 0
    for r, (c, a) in enumerate(zip(col, rea)):
        dc, da = dict(c), dict(a)
        for s in set(dc) | set(da):
            n += 1
            x, y = dc.get(s), da.get(s)
            if x == y:
                continue
            diff += 1
            gained += x is None
            lost += y is None
            if x is not None and y is not None:
                flipped += 1
                if truth is not None and truth[r].get(s) == y:
                    corrected += 1
    return dict(pairs=n, differ=diff, gained=gained, lost=lost, flipped=flipped, corrected=corrected)


# ------------------------------------------------------------------------------------------------------------------ worlds
def make_realign_world(seed, length=200_000, depth=30.0, read_len_scale=0.4, het_rate=1 / 400.0, noise_rate=0.004, plant_frac=0.1):
    """make_world + add_indels made consistent with its codes (as bamio.make_bam_world does), inserted bases given, and on `plant_frac` of
    the (read, het site) pairs an indel error NEXT to the site whose gap the alignment places 1 - 3 columns further on, so that the bases
    between the error and the gap sit one column off:
      kind 0  the read lacks the base left of the site, the gap stands right of it     (the site's column shows the right neighbour)
      kind 1  the read lacks the base right of the site, the gap stands left of it     (the site's column shows the left neighbour)
      kind 2  the read has an extra base left of the site, the insertion stands right  (the site's column shows the extra base)
      kind 3  a 50-base insertion three columns left of the site                       (query window over 64 bases: no entry)
    -> World; meta['truth_allele'][r] = {het position: the base the read carried there before planting}, meta['planted'] = [(r, p, kind)]"""
    import bamio
    from nanocaller_amd.synth import add_indels, apply_impute_inputs, make_world
    w = add_indels(make_world(seed=seed, length=length, depth=depth, read_len_scale=read_len_scale, het_rate=het_rate, odd_flag_frac=0.03),
                   seed=seed, het_rate=1 / 3000.0, noise_rate=noise_rate)
    rng = np.random.default_rng(seed + 9001)
    ev_off, ev_pos, ev_len = w.meta["events"]
    codes = w.codes.copy()
    per_read = []
    for r in range(w.n_reads):                                           # events consistent with the codes: no overlap, none at the ends
        s, e = int(w.read_start[r]), int(w.read_end[r])
        busy, ev = s, []
        for k in range(ev_off[r], ev_off[r + 1]):
            p, ln = int(ev_pos[k]), int(ev_len[k])
            need = -ln if ln < 0 else 0
            if p < busy or p + need + 2 >= e or p <= s:
                continue
            if ln < 0:
                codes[w.read_off[r] + (p + 1 - s):w.read_off[r] + (p + 1 - s) + need] = 4
            ev.append((p, ln, None))
            busy = p + need + 1
        per_read.append(ev)
    w.codes = codes
    flat = [x for ev in per_read for x in ev]
    off = np.zeros(w.n_reads + 1, np.int32)
    off[1:] = np.cumsum([len(ev) for ev in per_read])
    w.meta["events"] = (off, np.array([x[0] for x in flat], np.int32), np.array([x[1] for x in flat], np.int32))
    bamio.clean_noise_deletions(w)
    codes = w.codes
    het = np.asarray(w.het_sites, np.int64)
    letters = "AGTC"
    truth, planted, new_events = [], [], []
    for r in range(w.n_reads):
        s, e = int(w.read_start[r]), int(w.read_end[r])
        o = int(w.read_off[r])
        ev = [(p, ln, "".join("ACGT"[(p + i) % 4] for i in range(ln)) if ln > 0 else "") for p, ln, _ in per_read[r]]
        a, b = np.searchsorted(het, s), np.searchsorted(het, e)
        truth.append({int(p): int(codes[o + int(p) - s]) for p in het[a:b]})
        touched = np.zeros(e - s, bool)
        for p, ln, _ in ev:
            touched[max(0, p - s - 2):p - s + max(1, -ln) + 3] = True
        for p in het[a:b].tolist():
            if rng.random() >= plant_frac or p - 16 < s or p + 16 >= e:
                continue
            span = slice(p - 16 - s, p + 17 - s)
            if touched[span].any() or (codes[o + span.start:o + span.stop] > 3).any():
                continue
            old = codes[o + span.start:o + span.stop].copy()
            at = lambda x: int(old[x - (p - 16)])                        # noqa: E731  (the read's base on column x before planting)
            kind = int(rng.choice([0, 1, 2, 3], p=[0.35, 0.3, 0.3, 0.05]))
            k = int(rng.integers(1, 4))
            if kind == 0:
                for j in range(k + 1):
                    codes[o + p - 1 + j - s] = at(p + j)
                codes[o + p + k - s] = 4
                ev.append((p + k - 1, -1, ""))
            elif kind == 1:
                for j in range(k + 1):
                    codes[o + p - k + 1 + j - s] = at(p - k + j)
                codes[o + p - k - s] = 4
                ev.append((p - k - 1, -1, ""))
            elif kind == 2:
                codes[o + p - s] = int(rng.integers(0, 4))
                for j in range(k):
                    codes[o + p + 1 + j - s] = at(p + j)
                ev.append((p + k, 1, letters[at(p + k)]))
            else:
                ev.append((p - 3, 50, "".join("ACGT"[i] for i in rng.integers(0, 4, 50))))
            touched[span] = True
            planted.append((r, int(p), kind))
        new_events.append(sorted(ev))
    flat = [x for ev in new_events for x in ev]
    off = np.zeros(w.n_reads + 1, np.int32)
    off[1:] = np.cumsum([len(ev) for ev in new_events])
    w.meta["events"] = (off, np.array([x[0] for x in flat], np.int32), np.array([x[1] for x in flat], np.int32))
    ins_len = np.array([len(x[2]) for x in flat], np.int64)
    ins_off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum(ins_len, out=ins_off[1:])
    apply_impute_inputs(w, np.zeros(w.n_reads, np.uint8), ins_off, np.frombuffer("".join(x[2] for x in flat).encode(), np.uint8))
    w.meta["truth_allele"] = truth
    w.meta["planted"] = planted
    return w


def het_site_alleles(world, kept):
    """the world's het sites as phasing sites: (pos int32, alleles uint8 [n, 2] = REF base, the most frequent other base among the kept
    reads' true bases); sites whose REF is not a base, or without a second base, are left out"""
    refc = ref_codes(world.ref)
    cnt = {}
    for r in np.asarray(kept).tolist():
        for p, c in world.meta["truth_allele"][r].items():
            if c < 4:
                cnt.setdefault(p, np.zeros(4, np.int64))[c] += 1
    pos, al = [], []
    for p in sorted(cnt):
        rc = int(refc[p - 1])
        if rc > 3:
            continue
        v = cnt[p].copy()
        v[rc] = -1
        if v.max() <= 0:
            continue
        pos.append(p)
        al.append((rc, int(np.argmax(v))))
    return np.array(pos, np.int32), np.array(al, np.uint8).reshape(-1, 2)

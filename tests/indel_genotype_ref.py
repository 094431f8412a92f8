"""The yardstick of known-sites calling for indels: pass 1 of get_indel_testing_candidates[_haploid] WITH a list of columns,
restated column by column in pure Python the way oracle.indel_scan_impute restates pass 1 (oracle/ holds the reference's restatements and does
not change; this one is a rule of the project, so it lives with the tests).

The rule.  S = the listed columns of the contig, each of the small or the long class.  generate_indel_pileups.py:249-304 becomes

    if v_pos <= prev: continue
    if len_seq_0 >= mincov and len_seq_1 >= mincov:
        if   <long-window rule>:   prev = v_pos + window_size; variants[max(1, v_pos - window_size)] = 0
        elif <small-window rule>:  prev = v_pos + 10;          variants[max(1, v_pos - 10)] = 1
        elif v_pos in S:           the same two lines by S[v_pos]'s class                               # new
    elif impute_indel_phase and len_seq_tot >= 2 * mincov:
        if del_t <= del_freq_tot or ins_t <= ins_freq_tot or v_pos in S:                                # `or v_pos in S` is new
            ... the read grouping, unchanged ...

(haploid: the same `elif` under `len_seq_tot >= mincov`).  Only mode: the two window rules and the imputed frequency test read False.  The source
column of an anchor is the listed column that wrote or overwrote it through the new `elif`; a later natural column that overwrites the anchor's
type leaves the source, as extra_variants stays.  A listed column that only opened the imputed branch is not a source: that branch writes its
anchor and read sets as it always did.

by_name: alignments that share a read name count once per column and haplotype set, as the reference's name-keyed sets do (:218-235).
"""
import collections

import numpy as np

from oracle import oracle

CLASSES = ("natural_long", "natural_small", "below_thresholds", "no_event", "hap_below_mincov", "no_reads", "excluded", "n_in_window",
           "in_natural_skip", "in_listed_skip", "col_le_10", "chunk_first", "chunk_last", "shared_end", "outside", "off_contig", "both_classes")


_world = []


def listed_world():
    """The world of the GPU tests: test_indel_pipeline's kind (bamio.make_pass2_world) at 30 kb with an unphased block over 20,000 .. 24,000, a run of
    N in the reference at 1,500 .. 1,502, and no kept read over 7,000 .. 7,010 (every alignment there is flagged a duplicate: the pileup has no
    column there and thin ones around it).  Made once; callers must not modify it."""
    if not _world:
        import bamio
        w = bamio.make_pass2_world(seed=11, length=30_000, depth=26, blocks=[(20_000, 24_000)])
        w.ref = w.ref[:1_499] + "NNN" + w.ref[1_502:]
        gone = (np.asarray(w.read_start) <= 7_010) & (np.asarray(w.read_end) > 7_000)
        w.read_flag = np.where(gone, np.asarray(w.read_flag) | 0x400, np.asarray(w.read_flag)).astype(np.asarray(w.read_flag).dtype)
        _world.append(w)
    return _world[0]


_BASE = dict(mincov=4, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6, window_after=160)
# the cases of the GPU tests: chunks of 2,000 columns, two of them sharing an end; the first starts at column 1 (anchors clipped to 1), the third
# lies around the stretch without reads; the imputed case straddles the start of the unphased block
CASES = dict(
    dip=dict(_BASE, name="dip", chunks=[(1, 2_000), (2_000, 4_000), (6_000, 8_000)], exclude=[(2_500, 2_520)]),
    hap=dict(_BASE, name="hap", chunks=[(1, 2_000), (2_000, 4_000), (6_000, 8_000)], exclude=[(2_500, 2_520)], haploid=True, mincov=12),
    imp=dict(_BASE, name="imp", chunks=[(19_000, 21_000), (21_000, 23_000)], exclude=[], impute=True, mincov=3, ins_t=0.3, del_t=0.3))


def scan_listed(world, start, end, *, mincov, win_size, small_win_size, ins_t, del_t, exclude=None, supplementary=False, haploid=False,
                impute=False, sites=None, only=False, by_name=False, trace=None):
    """-> (variants {anchor: type}, src {anchor: listed column}, extra {anchor: (read indices 0, read indices 1)}).
    sites: {column: is_long}.  trace (a dict, filled): column -> what the walk saw there: 'excluded', 'no_reads', 'skipped' (v <= prev),
    'long', 'small' (a window rule fired), 'imputed', 'forced', 'depth' (a depth test failed), 'none'."""
    sites = sites or {}
    rs, re_, ro, codes, strand, keep = oracle._reads(world, supplementary)
    ev_off, ev_pos, ev_len = world.meta["events"]
    hap = np.asarray(world.meta["hap"])
    raw = None
    if impute:
        ins_off, ins_bases = world.meta["ev_ins"]
        raw = np.asarray(ins_bases, np.uint8).tobytes().decode("ascii")
    excl = np.zeros(world.length + 2, bool)
    for (a, b) in exclude or []:
        excl[max(0, a):max(0, b)] = True                              # IntervalTree.overlaps(pos): a <= pos < b
    lo, hi = max(1, start), min(end, world.length)
    order = np.nonzero(keep)[0]
    order = order[(rs[order] <= hi) & (re_[order] > lo)]
    ors, ore = rs[order], re_[order]
    ev_at = {}
    for r in order.tolist():
        for k in range(int(ev_off[r]), int(ev_off[r + 1])):
            ev_at[(r, int(ev_pos[k]))] = k
    if by_name:
        names = world.names
        mask = {}
        for r in range(len(names)):                                   # a name is in a hap set when any of its records carries that HP (:181-188)
            mask[names[r]] = mask.get(names[r], 0) | (1 if hap[r] == 1 else 2 if hap[r] == 2 else 0)
        key = lambda r: names[r]                                      # noqa: E731
        in0 = lambda r: bool(mask[names[r]] & 1)                      # noqa: E731
        in1 = lambda r: bool(mask[names[r]] & 2)                      # noqa: E731
    else:
        key = lambda r: r                                             # noqa: E731
        in0 = lambda r: hap[r] == 1                                   # noqa: E731
        in1 = lambda r: hap[r] == 2                                   # noqa: E731
    classes = [("del", False), ("ins", False), ("del", True), ("ins", True)]
    dq = {(c, h): collections.deque([set()] * (small_win_size if c >= 2 else win_size), small_win_size if c >= 2 else win_size)
          for c in range(4) for h in (0, 1)}
    variants, src, extra = {}, {}, {}
    prev = 0
    note = (lambda v, what: trace.__setitem__(v, what)) if trace is not None else (lambda v, what: None)
    for v in range(lo, hi + 1):
        reads = order[(ors <= v) & (ore > v)].tolist()
        if not reads:
            note(v, "no_reads")
            continue
        if excl[v]:
            note(v, "excluded")
            continue
        if haploid:
            r0, r1 = reads, []
        else:
            r0, r1 = [r for r in reads if in0(r)], [r for r in reads if in1(r)]
        for c, (kind, small) in enumerate(classes):
            for h, rh in ((0, r0), (1, r1)):
                members = set()
                for r in rh:
                    k = ev_at.get((r, v))
                    if k is None:
                        continue
                    ln = int(ev_len[k])
                    if (ln > 0) != (kind == "ins"):
                        continue
                    n = abs(ln)
                    if (n <= 10) if small else (2 < n <= 50):
                        members.add(key(r))
                dq[(c, h)].append(members)
        if v <= prev:
            note(v, "skipped")
            continue
        tot = len(reads)
        n0 = tot if haploid else len({key(r) for r in r0})
        n1 = 0 if haploid else len({key(r) for r in r1})
        if (n0 >= mincov) if haploid else (n0 >= mincov and n1 >= mincov):
            hs = ((0, n0),) if haploid else ((0, n0), (1, n1))
            f = {(c, h): (len(set.union(*dq[(c, h)])) / n if n > 0 else 0) for c in range(4) for h, n in hs}
            if haploid:
                long_rule = f[(0, 0)] >= del_t or f[(1, 0)] >= ins_t
                small_rule = f[(2, 0)] >= del_t or f[(3, 0)] >= ins_t or f[(2, 0)] + f[(3, 0)] >= 0.9
            else:
                long_rule = max(f[(0, 0)], f[(0, 1)]) >= del_t or max(f[(1, 0)], f[(1, 1)]) >= ins_t
                small_rule = (max(f[(2, 0)], f[(2, 1)]) >= del_t or max(f[(3, 0)], f[(3, 1)]) >= ins_t or f[(2, 0)] + f[(3, 0)] >= 0.9 or
                              f[(2, 1)] + f[(3, 1)] >= 0.9)
            if only:
                long_rule = small_rule = False
            if long_rule:
                prev = v + win_size
                variants[max(1, v - win_size)] = 0
                note(v, "long")
            elif small_rule:
                prev = v + 10
                variants[max(1, v - 10)] = 1
                note(v, "small")
            elif v in sites:
                if sites[v]:
                    prev, an, t = v + win_size, max(1, v - win_size), 0
                else:
                    prev, an, t = v + 10, max(1, v - 10), 1
                variants[an] = t
                src[an] = v
                note(v, "forced")
            else:
                note(v, "none")
        elif impute and not haploid and tot >= 2 * mincov:
            strs = []
            for r in reads:
                s = "AGTC*"[int(codes[ro[r] + (v - rs[r])])]
                k = ev_at.get((r, v))
                if k is not None:
                    ln = int(ev_len[k])
                    s += ("+%d%s" % (ln, raw[ins_off[k]:ins_off[k + 1]].upper())) if ln > 0 else ("-%d%s" % (-ln, "N" * -ln))
                strs.append(s)
            two = "".join(s[:2] for s in strs)
            del_f = (two.count("-") + two.count("*")) / tot
            ins_f = two.count("+") / tot
            note(v, "none")
            if (not only and (del_t <= del_f or ins_t <= ins_f)) or v in sites:
                groups = {}
                for s, r in zip(strs, reads):
                    groups.setdefault(s, []).append(r)
                counts = sorted(((g, len(m)) for g, m in groups.items()), key=lambda x: x[1], reverse=True)
                if counts[0][1] <= 0.8 * tot:
                    a = set(groups[counts[0][0]])
                    b = (set(groups[counts[1][0]]) if len(counts) > 1 and counts[1][1] >= mincov else set(reads) - a)
                else:
                    m = groups[counts[0][0]]
                    a, b = m[:counts[0][1] // 2], m[counts[0][1] // 2:]
                if len(a) >= mincov and len(b) >= mincov:
                    prev = v + 10
                    variants[max(1, v - 10)] = 1
                    extra[max(1, v - 10)] = (sorted(a), sorted(b))
                    note(v, "imputed")
        else:
            note(v, "depth")
    return variants, src, extra


def pass2_range(variants, start, end, win_size):
    """the anchors pass 2 visits (:306): max(0, start - 10 - win_size) < anchor <= end, ascending"""
    return sorted(a for a in variants if max(0, start - 10 - win_size) < a <= end)


def n_in_window(world, anchor, window_after):
    """:325-327: the reference window [anchor, min(chrom_length, anchor + window_after + 1)) holds a base that is not upper-case AGTC"""
    ref = world.ref[anchor - 1:min(world.length, anchor + window_after)]
    return any(c not in "AGTC" for c in ref)


def site_classes(world, case):
    """{class: columns, or (column, is_long) pairs for both_classes} of `case` (a dict: chunks [(start, end)], the scan's parameters, haploid,
    impute, exclude, window_after): what a listed column can be.  Classes are told from the PLAIN walk's trace (no list)."""
    kw = {k: case[k] for k in ("mincov", "win_size", "small_win_size", "ins_t", "del_t")}
    out = {c: [] for c in CLASSES}
    chunks = case["chunks"]
    win, wa = case["win_size"], case.get("window_after", 160)
    for ci, (a, b) in enumerate(chunks):
        tr = {}
        scan_listed(world, a, b, exclude=case.get("exclude"), haploid=case.get("haploid", False), impute=case.get("impute", False),
                    supplementary=case.get("supplementary", False), by_name=case.get("by_name", False), trace=tr, **kw)
        lo, hi = max(1, a), min(b, world.length)
        cols = range(lo, hi + 1)
        out["natural_long"] += [v for v in cols if tr.get(v) == "long"]
        out["natural_small"] += [v for v in cols if tr.get(v) == "small"]
        out["hap_below_mincov"] += [v for v in cols if tr.get(v) == "depth"]
        out["no_reads"] += [v for v in cols if tr.get(v) == "no_reads"]
        out["excluded"] += [v for v in cols if tr.get(v) == "excluded"]
        out["in_natural_skip"] += [v for v in cols if tr.get(v) == "skipped"]
        ev_near = _event_columns(world, lo - win, hi)
        none = [v for v in cols if tr.get(v) == "none"]
        out["below_thresholds"] += [v for v in none if ev_near[v - (lo - win):v - (lo - win) + win + 1].any()]
        quiet = [v for v in none if not ev_near[v - (lo - win):v - (lo - win) + win + 1].any()]
        out["no_event"] += quiet
        out["n_in_window"] += [v for v in none if v > 10 and n_in_window(world, v - 10, wa)]
        out["col_le_10"] += [v for v in none if v <= 10]
        out["chunk_first"] += [lo]
        out["chunk_last"] += [hi]
        if ci + 1 < len(chunks) and chunks[ci + 1][0] == b:
            out["shared_end"] += [b]
        # two listed columns 5 apart where nothing natural fires: the second lies in the first one's skip range
        pairs = [v for v in quiet if v + 5 in set(quiet)]
        out["in_listed_skip"] += [p for v in pairs[:1] + pairs[-1:] for p in (v, v + 5)]
        out["both_classes"] += quiet[len(quiet) // 3:len(quiet) // 3 + 1]
    los, his = min(a for a, _ in chunks), max(b for _, b in chunks)
    inside = lambda p: any(max(1, a) <= p <= b for a, b in chunks)      # noqa: E731
    out["outside"] = [p for p in (los - 1, los - 7, his + 1, his + 9, his + 4000) if 1 <= p <= world.length and not inside(p)]
    out["off_contig"] = [0, -3, world.length + 9]
    return {k: sorted(set(v)) for k, v in out.items()}


def _event_columns(world, lo, hi):
    """bool per column lo .. hi + 1: some kept read carries an event on it"""
    ev_off, ev_pos, ev_len = world.meta["events"]
    m = np.zeros(hi - lo + 2, bool)
    p = np.asarray(ev_pos)
    p = p[(p >= lo) & (p <= hi)]
    m[p - lo] = True
    return m


_lists = {}


def site_list(world, case, per_class=8):
    """the list the tests use for `case` -> (positions int64, is_long uint8): up to per_class columns of every class, their first and last members
    included, shuffled, a tenth listed twice; every third column is of the long class, the both_classes columns are listed once per class.
    Deterministic; computed once per case name."""
    name = case["name"]
    if name not in _lists:
        pos, lng = [], []
        for cname, p in site_classes(world, case).items():
            if not len(p):
                continue
            p = np.asarray(p, np.int64)[np.unique(np.linspace(0, len(p) - 1, min(per_class, len(p))).astype(np.int64))]
            for i, v in enumerate(p.tolist()):
                if cname == "both_classes":
                    pos += [v, v]
                    lng += [0, 1]
                else:
                    pos.append(v)
                    lng.append(1 if (v % 3 == 0 and cname != "in_listed_skip") else 0)
        pos, lng = np.asarray(pos, np.int64), np.asarray(lng, np.uint8)
        rng = np.random.Generator(np.random.PCG64(len(name) + int(pos.sum() % 1000)))
        pos, lng = np.concatenate([pos, pos[::10]]), np.concatenate([lng, lng[::10]])
        perm = rng.permutation(pos.size)
        _lists[name] = (pos[perm], lng[perm])
    return _lists[name]


def as_dict(pos, is_long):
    """{column: is_long} of a list: a column listed with both classes is long"""
    d = {}
    for p, g in zip(np.asarray(pos).tolist(), np.asarray(is_long).tolist()):
        d[p] = bool(d.get(p, False) or g)
    return d


def depth_verdicts(world, cols, *, mincov, haploid=False, by_name=False, exclude=None, supplementary=False):
    """{column: a listed column passes pass 1's depth test there} -- the walk over the one-column chunk [v, v] in only mode with S = {v}: reads
    present, not excluded, both haplotype depths (haploid: all reads) >= mincov.  What k_listed decides per column before any `prev` skip."""
    out = {}
    for v in cols:
        got, _, _ = scan_listed(world, v, v, mincov=mincov, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6, exclude=exclude,
                                supplementary=supplementary, haploid=haploid, sites={int(v): False}, only=True, by_name=by_name)
        out[int(v)] = bool(got)
    return out


MATES_MINCOV = 7              # the mates world of tests/test_indel_mates.py: where by-name and per-alignment depths part at the shared names


def mates_columns(world, lo, hi, step=3):
    """columns of [lo, hi] where two kept alignments of one read name overlap (every `step`-th), ascending"""
    by = {}
    for r, nm in enumerate(world.names):
        by.setdefault(nm, []).append(r)
    cols = set()
    for rs_ in by.values():
        for i, a in enumerate(rs_):
            for b in rs_[i + 1:]:
                s, e = max(int(world.read_start[a]), int(world.read_start[b]), lo), min(int(world.read_end[a]), int(world.read_end[b]), hi + 1)
                cols.update(range(s, e, step))
    return sorted(cols)


def world_of_device_workload(host):
    """a World of the reads a tests/util.IndelReadsHost holds (a synthetic workload generated in HBM): what scan_listed walks"""
    from nanocaller_amd.synth import World
    s, e = np.asarray(host.s, np.int32), np.asarray(host.e, np.int32)
    off = np.zeros(len(s) + 1, np.int64)
    np.cumsum(e - s, out=off[1:])
    codes = np.concatenate([host.codes[int(host.slot[r]) + (int(s[r]) & 15):int(host.slot[r]) + (int(s[r]) & 15) + int(e[r] - s[r])] for r in range(len(s))])
    w = World(chrom="synth", ref=host.ref.upper(), read_start=s, read_end=e, read_flag=np.zeros(len(s), np.int32), read_off=off, codes=codes,
              names=["r%07d" % i for i in range(len(s))])
    w.meta.update(events=(host.ev_off, host.ev_pos, host.ev_len), hap=np.asarray(host.hap))
    return w

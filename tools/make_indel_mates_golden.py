#!/usr/bin/env python3
"""tests/golden/indel_ont_mates.npz: the reference's own get_indel_testing_candidates / _haploid on a world whose kept alignments
share read names (split reads under dct['supplementary'] = True), and on the same world with every name made unique.

Needs the reference checkout the oracle tools use (oracle/tools/make_goldens.py, imported here for its stub modules and aligner
stand-ins, unchanged); what is written is DATA: the world's arrays and the tuples the reference returned.

The world (seed, ~30 kb at 30x, default ONT thresholds, three chunks) plants, each at a true heterozygous deletion or -- (c) -- at a
pair of planted insertions:
  a  an overlapping pair that both carry the deletion
  b  an overlapping pair where only the later record carries it (the earlier one untagged)
  c  two records of one name that do not overlap, within win_size columns, each with an insertion; the haplotype's depth there is
     cut to five reads, so that two owners pass ins_t and one does not
  d  a supplementary record without HP whose primary has HP
  e  a name with two records at an anchor whose windows differ
  f  a name whose records carry HP 1 and HP 2
`plants` in the file lists (case, first column, last column) of every plant; fixture_condition() counts, per case a .. f, the sites that
differ between the by-name and the per-alignment answers (the test asks for one of every case a .. e).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
OUT = os.path.join(REPO, "tests", "golden", "indel_ont_mates.npz")
REFERENCE_SRC = "/root/reference/nanocaller_src"                      # where oracle/tools/make_goldens.py pins the reference's package
SEED = 7
LENGTH, DEPTH = 30_000, 30
CHUNKS = [(1, 10_000), (10_001, 20_000), (20_001, 29_500)]
DCT = dict(seq="ont", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6, supplementary=True, exclude_bed=None,
           impute_indel_phase=False)


def build_world(seed=SEED):
    """-> (world with shared names, list of (case, lo, hi))"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import bamio
    w = bamio.make_pass2_world(seed=seed, length=LENGTH, depth=DEPTH)
    rs, re_ = w.read_start.astype(np.int64), w.read_end.astype(np.int64)
    flag = w.read_flag.copy()
    hap = np.asarray(w.meta["hap"], np.uint8).copy()
    ev_off, ev_pos, ev_len = (np.asarray(a).copy() for a in w.meta["events"])
    ins_off, ins_bases = (np.asarray(a).copy() for a in w.meta["ev_ins"])
    R = w.n_reads
    names = ["r%07d" % i for i in range(R)]
    plain = [r for r in range(R) if int(flag[r]) in (0, 16)]
    used, plants = set(), []

    def has(r, p, ln):
        k = np.flatnonzero(ev_pos[ev_off[r]:ev_off[r + 1]] == p)
        return k.size and ev_len[ev_off[r] + k[0]] == ln

    # true heterozygous deletions: (column, length) carried by at least eight reads of one haplotype, ascending
    cnt = {}
    for r in plain:
        for k in range(ev_off[r], ev_off[r + 1]):
            if -50 <= ev_len[k] < -2 and hap[r]:
                cnt.setdefault((int(ev_pos[k]), int(ev_len[k]), int(hap[r])), []).append(r)
    sites = sorted(k for k, v in cnt.items() if len(v) >= 8 and 500 < k[0] < LENGTH - 1_500)
    taken = []
    clean = lambda lo, hi: all(c in "AGTC" for c in w.ref[lo - 1:hi])   # noqa: E731  (a window with another letter is skipped by pass 2, :325-328)

    def free_site(pred):
        for s in sites:
            if any(abs(s[0] - t) < 400 for t in taken) or not clean(s[0] - 60, s[0] + 230):
                continue
            got = pred(s)
            if got:
                taken.append(s[0])
                return s, got
        raise RuntimeError("no site for a plant: change the seed")

    def share(r1, r2):
        names[r2] = names[r1]
        flag[r2] = 0x800 | (int(flag[r2]) & 16)
        used.update((r1, r2))

    def carriers(s):
        return [r for r in cnt[s] if r not in used]

    def covering(s, h=None):                                         # reads over the site's window that do not carry the deletion
        return [r for r in plain if r not in used and rs[r] < s[0] - 60 and re_[r] > s[0] + 200 and not has(r, s[0], s[1]) and (h is None or hap[r] == h)]

    # a: both carry it
    s, (r1, r2) = free_site(lambda s: tuple(carriers(s)[:2]) if len(carriers(s)) >= 2 else None)
    share(r1, r2)
    plants.append(("a", s[0] - 45, s[0] + 5))
    # b: only the later record carries it; the earlier one loses its tag
    def pick_b(s):
        for r2 in carriers(s):
            c = [r for r in covering(s, 3 - s[2]) if r < r2]
            if c:
                return c[-1], r2
    s, (r1, r2) = free_site(pick_b)
    hap[r1] = 0
    share(r1, r2)
    plants.append(("b", s[0] - 45, s[0] + 5))
    # d: the later (supplementary) record carries it too but has no HP
    s, (r1, r2) = free_site(lambda s: tuple(carriers(s)[:2]) if len(carriers(s)) >= 2 else None)
    hap[r2] = 0
    share(r1, r2)
    plants.append(("d", s[0] - 45, s[0] + 5))
    # e: two records at the anchor whose windows differ (a carrier and a non-carrier of the same tag)
    def pick_e(s):
        for r1 in carriers(s):
            c = [r for r in covering(s, 3 - s[2]) if r > r1]
            if c:
                return r1, c[0]
    s, (r1, r2) = free_site(pick_e)
    hap[r2] = hap[r1]
    share(r1, r2)
    plants.append(("e", s[0] - 45, s[0] + 5))
    # f: HP 1 and HP 2 under one name
    s, (r1, r2) = free_site(pick_e)
    share(r1, r2)
    plants.append(("f", s[0] - 45, s[0] + 5))
    # c: two records that do not overlap, the second starting within 20 columns of the first's end; an insertion of five bases in each
    new_ev = {}
    for r1 in plain:
        if r1 in used or not hap[r1] or any(abs(re_[r1] - t) < 600 for t in taken) or not (1_000 < re_[r1] < LENGTH - 2_000):
            continue
        nxt = [r for r in plain if r not in used and r != r1 and hap[r] == hap[r1] and 0 < rs[r] - re_[r1] <= 20 and re_[r] - rs[r] > 300]
        if not nxt:
            continue
        r2 = nxt[0]
        p1, p2 = int(re_[r1]) - 8, int(rs[r2]) + 3
        busy = lambda r, p: any(abs(int(q) - p) < 60 for q in ev_pos[ev_off[r]:ev_off[r + 1]])   # noqa: E731
        if busy(r1, p1) or busy(r2, p2) or not clean(p1 - 60, p2 + 230):
            continue
        span = [r for r in range(R) if not (int(flag[r]) & 0x704) and r not in (r1, r2) and hap[r] == hap[r1] and re_[r] > p1 - 60 and rs[r] < p2 + 60]
        whole = [r for r in span if r in plain and r not in used and rs[r] < p1 - 60 and re_[r] > p2 + 60 and not any(p1 - 60 <= q <= p2 + 60 for q in ev_pos[ev_off[r]:ev_off[r + 1]])]
        if len(whole) < 4:
            continue
        for r in span:
            if r not in whole[:4]:
                hap[r] = 0
        new_ev[r1], new_ev[r2] = p1, p2
        share(r1, r2)
        plants.append(("c", p1 - 45, p2 + 45))
        break
    else:
        raise RuntimeError("no pair for plant c: change the seed")
    # rebuild the events with the two insertions
    n_off, n_pos, n_len, n_ioff, n_ib = [0], [], [], [0], []
    for r in range(R):
        evs = [(int(ev_pos[k]), int(ev_len[k]), bytes(ins_bases[ins_off[k]:ins_off[k + 1]])) for k in range(ev_off[r], ev_off[r + 1])]
        if r in new_ev:
            evs = sorted(evs + [(new_ev[r], 5, b"GATCA")])
        for p, ln, b in evs:
            n_pos.append(p)
            n_len.append(ln)
            n_ib.append(b)
            n_ioff.append(n_ioff[-1] + len(b))
        n_off.append(len(n_pos))
    w.read_flag = flag
    w.names = names
    w.meta["events"] = (np.array(n_off, np.int32), np.array(n_pos, np.int32), np.array(n_len, np.int32))
    from nanocaller_amd.synth import apply_impute_inputs
    w = apply_impute_inputs(w, hap, np.array(n_ioff, np.int64), np.frombuffer(b"".join(n_ib), np.uint8))
    return w, plants


def run_reference(w, tag):
    """the reference's two functions on every chunk -> {key: array} for the npz"""
    import make_goldens as mg                                        # noqa: F401  (oracle/tools: path set-up, stub modules, aligner stand-ins)
    import pysam
    import bamio
    from nanocaller_src import generate_indel_pileups as ref_indel
    from nanocaller_src import generate_indel_pileups_haploid as ref_hap
    mg._install_aligner_stubs(ref_indel, check_every=10 ** 9)
    ref_hap.Popen = ref_indel.Popen
    pysam.register_records("bam_" + tag, w.chrom, w.length, w.ref, bamio.world_to_records(w, None))
    pysam.register_records("fa_" + tag, w.chrom, w.length, w.ref, [])
    dct = dict(DCT, fasta_path="fa_" + tag)
    rec = {}
    for ci, (a, b) in enumerate(CHUNKS):
        chunk = dict(chrom=w.chrom, start=a, end=b, sam_path="bam_" + tag)
        pos, x0, x1, x2, alleles, phase = ref_indel.get_indel_testing_candidates(dct, chunk)
        hpos, hx, halleles = ref_hap.get_indel_testing_candidates_haploid(dct, chunk)
        pre = "%s_c%d_" % (tag, ci)
        rec[pre + "pos"] = np.asarray(pos, np.int64)
        for i, x in enumerate((x0, x1, x2)):
            rec[pre + "x%d" % i] = np.asarray(x, np.float64).reshape(-1, 5, 128, 2).astype(np.float32)
        rec[pre + "alleles"] = np.array(json.dumps(alleles))
        rec[pre + "phase"] = np.array(json.dumps(phase))
        rec[pre + "hpos"] = np.asarray(hpos, np.int64)
        rec[pre + "hx"] = np.asarray(hx, np.float64).reshape(-1, 5, 128, 2).astype(np.float32)
        rec[pre + "halleles"] = np.array(json.dumps(halleles))
        print("%s chunk %d [%d, %d]: %d diploid, %d haploid sites" % (tag, ci, a, b, len(pos), len(hpos)))
    return rec


def sites_of(z, tag, haploid=False):
    """{position: (tensors, alleles, phase)} over all chunks of one answer in the golden (a position of two chunks keeps the later)"""
    out = {}
    for ci in range(len(json.loads(str(z["chunks"])))):
        pre = "%s_c%d_" % (tag, ci)
        pos = z[pre + ("hpos" if haploid else "pos")].tolist()
        al = json.loads(str(z[pre + ("halleles" if haploid else "alleles")]))
        ph = [None] * len(pos) if haploid else json.loads(str(z[pre + "phase"]))
        xs = [z[pre + "hx"]] if haploid else [z[pre + "x%d" % i] for i in range(3)]
        for k, p in enumerate(pos):
            out[(ci, p)] = (tuple(x[k].tobytes() for x in xs), json.dumps(al[k]), ph[k])
    return out


def fixture_condition(z):
    """-> {case: number of diploid sites inside a plant of the case that differ between the by-name and the per-alignment answers}"""
    a, b = sites_of(z, "name"), sites_of(z, "uniq")
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    out = {}
    for case, lo, hi in json.loads(str(z["plants"])):
        out[case] = out.get(case, 0) + sum(1 for (_, p) in diff if lo <= p <= hi)
    return out


def generate(path=OUT, seed=SEED):
    sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
    sys.path.insert(0, REPO)
    import copy
    w, plants = build_world(seed)
    import bamio
    rec = bamio.world_arrays(w, "w_")
    rec["w_name_id"] = np.array([int(n[1:]) for n in w.names], np.int32)
    rec["plants"] = np.array(json.dumps(plants))
    rec["chunks"] = np.array(json.dumps(CHUNKS))
    rec["dct"] = np.array(json.dumps(DCT))
    rec.update(run_reference(w, "name"))
    u = copy.copy(w)
    u.names = ["r%07d" % i for i in range(w.n_reads)]
    rec.update(run_reference(u, "uniq"))
    np.savez_compressed(path, **rec)
    z = np.load(path)
    print("plants:", plants)
    print("differing sites per case:", fixture_condition(z))
    return path


if __name__ == "__main__":
    if not os.path.isdir(REFERENCE_SRC):
        sys.exit("the reference is absent: no %s" % REFERENCE_SRC)
    generate(*(sys.argv[1:2] or [OUT]))

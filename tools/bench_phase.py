"""Wall time of the read-based phaser on a chr20-sized synthetic ONT contig (64.4 Mb, 30x, generated in HBM by nc_synth_indel_*):
allele gather, read selection + blocks + slots (host), the MEC DP, haplotagging.  The het sites are the generator's own (its truth,
recomputed from the same seed); every read is its own name.  --realign: the alleles by local realignment (nc_snp_phase_realign) instead of
the column gather.  --distrust N: the genotype-aware DP (nc_snp_phase_solve_gt) against the plain one on the same het-only site list, and on the
list with the homozygous SNP sites added as 1/1 calls.  --weighted N: the weighted DP (nc_snp_phase_set_weights: ONT-like qualities drawn per
entry, capped at --w-max, every read allowed) against the plain one on the same entries, interleaved; then whether the contig still solves inside
the DP's 16-bit relative range when EVERY entry weighs --w-max, and if not the largest uniform weight that does.  Prints one JSON line.
Usage: python tools/bench_phase.py [--length L] [--reps N] [--realign | --compare N | --distrust N | --weighted N] [--w-max W] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nanocaller_amd.engine import get_engine  # noqa: E402
from nanocaller_amd.synth_device import make_indel_device_workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=812)
    ap.add_argument("--realign", action="store_true")
    ap.add_argument("--compare", type=int, default=0, help="N interleaved runs of the column gather and of the realignment, medians and their ratio")
    ap.add_argument("--distrust", type=int, default=0, help="N interleaved runs of the plain solve, the genotype-aware solve on the same het-only sites, "
                    "and the genotype-aware solve with the homozygous sites added: medians, and the DP's ratio to the plain form")
    ap.add_argument("--distrust-cost", type=int, default=1)
    ap.add_argument("--weighted", type=int, default=0, help="N interleaved runs of the plain solve and of the weighted solve on the same entries: medians, "
                    "the DP's ratio to the plain form, and the capacity check at --w-max")
    ap.add_argument("--w-max", type=int, default=93)
    ap.add_argument("--out", default=None, help="with --distrust / --weighted: also write the JSON to this file")
    a = ap.parse_args()
    eng = get_engine(0)
    eng.use_torch_stream()
    L = a.length
    pack, reads_c, info = make_indel_device_workload(eng, L, depth=a.depth, seed=a.seed)
    # the generator's haplotype bases (make_indel_device_workload's defaults): het SNP sites and their two alleles
    ref = torch.zeros(L + 1, dtype=torch.uint8, device=eng.device)
    hapb = torch.zeros(2 * (L + 1), dtype=torch.uint8, device=eng.device)
    hapi = torch.zeros(2 * (L + 1), dtype=torch.int8, device=eng.device)
    P = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    assert eng.L.nc_synth_indel_truth(eng.ctx, L, a.seed, 1 / 1000.0, 1 / 2000.0, 1 / 5000.0, 1 / 15000.0, 50, P(ref), P(hapb), P(hapi)) == 0
    hb = hapb.view(2, L + 1).cpu().numpy()
    r = ref.cpu().numpy()
    het = np.flatnonzero((hb[0] != hb[1]) & (r < 4))
    het = het[het >= 1].astype(np.int32)
    alt = np.where(hb[0][het] != r[het], hb[0][het], hb[1][het])
    alleles = np.stack([r[het], alt], 1).astype(np.uint8)
    R = info["n_reads"]
    reads = (pack.codes, pack.reads["rd_start"], pack.reads["rd_end"], pack.reads["slot_off"])
    group = np.arange(R, dtype=np.int32)
    kw = dict(reads=reads)
    if a.realign:                                                       # reference codes with position p at index p - 1
        kw = dict(realign=(pack.codes, reads_c, info["n_events"], info["n_ins_bases"], ref[1:].contiguous()))
    if a.distrust:
        # the same gather, three solves: plain / genotype-aware on the het sites (every class 0), genotype-aware with the truth's homozygous SNP
        # sites added as 1/1 calls (alleles REF, ALT; class 2).  The plain form is the yardstick.
        hom = np.flatnonzero((hb[0] == hb[1]) & (hb[0] != r) & (r < 4) & (hb[0] < 4))
        hom = hom[hom >= 1].astype(np.int32)
        both = np.concatenate([het, hom])
        o = np.argsort(both, kind="stable")
        pos2 = both[o]
        al2 = np.concatenate([alleles, np.stack([r[hom], hb[0][hom]], 1).astype(np.uint8)])[o]
        gt2 = np.concatenate([np.zeros(het.size, np.uint8), np.full(hom.size, 2, np.uint8)])[o]
        forms = dict(plain=(het, alleles, {}), distrust=(het, alleles, dict(site_gt=np.zeros(het.size, np.uint8), distrust_cost=a.distrust_cost)),
                     distrust_with_hom=(pos2, al2, dict(site_gt=gt2, distrust_cost=a.distrust_cost)))
        eng.snp_phase(het, alleles, group, R, reads=reads)
        walls, stages, last = {k: [] for k in forms}, {k: [] for k in forms}, {}
        for _ in range(a.distrust):
            for k, (p_, al_, kw_) in forms.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                last[k] = eng.snp_phase(p_, al_, group, R, reads=reads, **kw_)
                walls[k].append(time.perf_counter() - t)
                stages[k].append(last[k]["ms"])
        med = lambda v: float(np.median(v))                              # noqa: E731
        dp = {k: med([m["dp"] for m in stages[k]]) for k in forms}
        out = dict(metric="phase_chr20_sized_distrust_dp_over_plain", value=round(dp["distrust"] / dp["plain"], 4),
                   with_hom_dp_over_plain=round(dp["distrust_with_hom"] / dp["plain"], 4), length=L, depth=a.depth, reads=R, het_sites=int(het.size),
                   hom_sites=int(hom.size), distrust_cost=a.distrust_cost, runs=a.distrust)
        for k in forms:
            res = last[k]
            out[k] = dict(wall_s=round(med(walls[k]), 4), walls_s=[round(x, 4) for x in walls[k]], sites=int(forms[k][0].size),
                          entries=int(res["entry_site"].size), phased_sites=int(res["site_phased"].sum()), blocks=int(res["block_first"].size),
                          mec_cost=int(res["block_cost"].sum()), tagged_reads=int((res["group_hp"] > 0).sum()),
                          stage_ms={s_: round(med([m[s_] for m in stages[k]]), 3) for s_ in stages[k][0]})
            if "site_gt" in res:
                out[k]["outcomes_left_call"] = int((res["site_gt"] != forms[k][2]["site_gt"]).sum())
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.weighted:
        from nanocaller_amd import _lib
        first = eng.snp_phase(het, alleles, group, R, reads=reads)       # (warm; and the number of entries the weights are drawn for)
        ne = int(first["entry_site"].size)
        rng = np.random.default_rng(a.seed)
        # ONT-like base qualities: a gamma body around Q20 with a tail, a seventh of the bases low (Q1-7)
        q = np.clip(rng.gamma(5.0, 4.0, ne), 1, 93)
        low = rng.random(ne) < 1 / 7
        q[low] = rng.integers(1, 8, int(low.sum()))
        q = np.minimum(q.astype(np.uint8), a.w_max).astype(np.uint8)
        forms = dict(plain={}, weighted=dict(weights=(q, None)))
        walls, stages, last = {k: [] for k in forms}, {k: [] for k in forms}, {}
        for _ in range(a.weighted):
            for k, kw_ in forms.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                last[k] = eng.snp_phase(het, alleles, group, R, reads=reads, **kw_)
                walls[k].append(time.perf_counter() - t)
                stages[k].append(last[k]["ms"])
        med = lambda v: float(np.median(v))                              # noqa: E731
        dp = {k: [m["dp"] for m in stages[k]] for k in forms}
        out = dict(metric="phase_chr20_sized_weighted_dp_over_plain", value=round(med(dp["weighted"]) / med(dp["plain"]), 4), length=L, depth=a.depth, reads=R,
                   het_sites=int(het.size), entries=ne, w_max=a.w_max, runs=a.weighted, mean_weight=round(float(q.mean()), 2),
                   plain_dp_ms=[round(x, 2) for x in dp["plain"]], weighted_dp_ms=[round(x, 2) for x in dp["weighted"]])
        for k in forms:
            res = last[k]
            out[k] = dict(wall_s=round(med(walls[k]), 4), walls_s=[round(x, 4) for x in walls[k]], phased_sites=int(res["site_phased"].sum()),
                          blocks=int(res["block_first"].size), mec_cost=int(res["block_cost"].sum()), tagged_reads=int((res["group_hp"] > 0).sum()),
                          stage_ms={s_: round(med([m[s_] for m in stages[k]]), 3) for s_ in stages[k][0]})
        out["sites_whose_h_differs"] = int((last["plain"]["site_h"] != last["weighted"]["site_h"]).sum())
        # capacity: the worst case of a cap is every entry AT the cap (the relative costs scale with it)
        solved = {}
        for v in [a.w_max] + [x for x in (80, 64, 48, 40, 32, 24, 16, 8) if x < a.w_max]:
            try:
                eng.snp_phase(het, alleles, group, R, reads=reads, weights=(np.full(ne, v, np.uint8), None))
                solved[v] = True
                break
            except _lib.NanoCallerHipError as e:
                if "(%d)" % _lib.NC_ERR_CAPACITY not in str(e):
                    raise
                solved[v] = False
        out["uniform_weight_solves"] = {str(k): v for k, v in solved.items()}
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if a.compare:
        # both allele detectors on the same contig, interleaved, median of `compare` runs each (the column gather is the yardstick)
        kws = dict(column=dict(reads=reads), realign=dict(realign=(pack.codes, reads_c, info["n_events"], info["n_ins_bases"], ref[1:].contiguous())))
        eng.snp_phase(het, alleles, group, R, **kws["column"])
        walls, stages, last = {k: [] for k in kws}, {k: [] for k in kws}, {}
        for _ in range(a.compare):
            for k, kw in kws.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                last[k] = eng.snp_phase(het, alleles, group, R, **kw)
                walls[k].append(time.perf_counter() - t)
                stages[k].append(last[k]["ms"])
        med = lambda v: float(np.median(v))                              # noqa: E731
        out = dict(metric="phase_chr20_sized_realign_over_column", value=round(med(walls["realign"]) / med(walls["column"]), 4), length=L, depth=a.depth,
                   reads=R, het_sites=int(het.size), runs=a.compare,
                   pairs=int((np.searchsorted(het, info["read_end"]) - np.searchsorted(het, info["read_start"])).sum()))
        for k in kws:
            out[k] = dict(wall_s=round(med(walls[k]), 4), walls_s=[round(x, 4) for x in walls[k]], entries=int(last[k]["entry_site"].size),
                          phased_sites=int(last[k]["site_phased"].sum()), tagged_reads=int((last[k]["group_hp"] > 0).sum()),
                          stage_ms={s_: round(med([m[s_] for m in stages[k]]), 3) for s_ in stages[k][0]})
        print(json.dumps(out))
        return
    runs = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = eng.snp_phase(het, alleles, group, R, **kw)
        runs.append((time.perf_counter() - t, res["ms"]))
    wall, ms = min(runs[1:], key=lambda x: x[0])
    out = dict(metric="phase_chr20_sized_s", value=round(wall, 4), realign=bool(a.realign), length=L, depth=a.depth, reads=R, het_sites=int(het.size),
               phased_sites=int(res["site_phased"].sum()), blocks=int(res["block_first"].size), entries=int(res["entry_site"].size),
               tagged_reads=int((res["group_hp"] > 0).sum()), stage_ms={k: round(v, 2) for k, v in ms.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

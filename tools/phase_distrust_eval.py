"""The device phaser with and without distrusted genotypes on calls with planted genotype errors (the 2 Mb ONT-like 30x world of
tools/phase_realign_eval.py; the calls are its true ones, tests/phase_gt_ref.py world_calls): a stated share of the true het 0/1 records is
rewritten to 1/1, and a false 0/1 record is added about every `--false-het-step` bases where both haplotypes carry the reference base.  Reports
how many of either kind the distrust mode brings back (rewritten het -> het and phased; false het -> 0/0), how many untouched calls it changes,
and, for the plain mode and the distrust mode on the same records, the switch errors between adjacent phased true het sites, the share of reads
tagged and of those tagged on the right haplotype, and phase_contig's wall time (median of interleaved runs).  Prints one JSON line.
Usage: python tools/phase_distrust_eval.py [--length L] [--seed S] [--share-hom F] [--false-het-step N] [--cost G] [--runs N] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bamio  # noqa: E402
from phase_gt_ref import edit_calls, hom_ref_columns, world_calls  # noqa: E402
from phase_realign_eval import figures  # noqa: E402
from phase_realign_ref import make_realign_world  # noqa: E402

CODE = {"A": 0, "G": 1, "T": 2, "C": 3}


def phasing_figures(w, kept, res):
    """phase_realign_eval's figures over the result's sites that are true het sites with both alleles among the reads' true bases (the added and
    the homozygous sites have no planted haplotypes to compare with)"""
    het = set(np.asarray(w.het_sites).tolist())
    keep = np.array([int(p) in het for p in res.sites["pos"].tolist()])
    remap = np.cumsum(keep) - 1
    off, site, allele = res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]
    ek = keep[site]
    rid = np.repeat(np.arange(kept.size), np.diff(off))
    off2 = np.zeros(kept.size + 1, np.int64)
    np.cumsum(np.bincount(rid[ek], minlength=kept.size), out=off2[1:])
    al = np.array([[CODE[x] for x in (ln.split("\t")[3], ln.split("\t")[4].split(",")[0])] if "," not in ln.split("\t")[4] else
                   [CODE[x] for x in ln.split("\t")[4].split(",")] for ln in (res.records[i] for i in res.sites["record"][keep].tolist())], np.uint8)

    class Sub:
        sites = dict(phased=res.sites["phased"][keep], h=res.sites["h"][keep], block=res.sites["block"][keep])
        reads = dict(res.reads, entry_off=off2, entry_site=remap[site[ek]], entry_allele=allele[ek])
        blocks = res.blocks
    return figures(w, kept, res.sites["pos"][keep], al.reshape(-1, 2), Sub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--share-hom", type=float, default=0.1, help="share of the true het 0/1 records rewritten to 1/1")
    ap.add_argument("--false-het-step", type=int, default=5_000, help="a false 0/1 record about every this many bases")
    ap.add_argument("--cost", type=int, default=1, help="distrust_cost")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nanocaller_amd.phase import kept_reads, phase_contig
    w = make_realign_world(a.seed, length=a.length, depth=30.0, read_len_scale=1.0, het_rate=1 / 1000.0)
    d = tempfile.mkdtemp(prefix="distrust_eval")
    bam, fa = os.path.join(d, "w.bam"), os.path.join(d, "w.fa")
    bamio.write_bam(bam, w.chrom, w.length, [dict(r, tags={}) for r in bamio.world_to_records(w, None)], level=1)
    bamio.write_fasta(fa, w.chrom, w.ref)
    kept = kept_reads(w, False)[0]
    rng = np.random.default_rng(a.seed)
    calls = world_calls(w, kept)
    cols, alt_of = hom_ref_columns(w, [], a.false_het_step, rng)
    vcf, to_hom, added = edit_calls(calls, w.het_sites, cols, rng, share_hom=a.share_hom, alt_of=alt_of)
    gt_of = lambda ln: ln.split("\t")[9].split(":")[0]                     # noqa: E731
    out = dict(metric="phase_distrust_eval", length=a.length, seed=a.seed, distrust_cost=a.cost, runs=a.runs, records=len(vcf),
               true_calls=dict(het=sum(gt_of(ln) != "1/1" for ln in calls), hom=sum(gt_of(ln) == "1/1" for ln in calls)),
               het_rewritten_to_hom=len(to_hom), false_het_added=len(added))
    modes = dict(plain={}, distrust=dict(distrust=True, distrust_cost=a.cost))
    res, walls = {}, {k: [] for k in modes}
    for k, kw in modes.items():
        res[k] = phase_contig(bam, fa, w.chrom, vcf, 10, False, **kw)
        out[k] = {f: v for f, v in phasing_figures(w, kept, res[k]).items() if f not in ("entries", "alleles_right")}
        out[k]["mec_cost"] = int(sum(b[3] for b in res[k].blocks))
    for _ in range(a.runs):
        for k, kw in modes.items():
            t = time.perf_counter()
            r = phase_contig(bam, fa, w.chrom, vcf, 10, False, **kw)
            walls[k].append(time.perf_counter() - t)
            out[k]["stage_ms"] = {s: round(float(v), 3) for s, v in r.ms.items()}
    for k in modes:
        out[k]["phase_contig_s"] = round(float(np.median(walls[k])), 4)
    rd = res["distrust"]
    by_pos = {int(ln.split("\t")[1]): ln for ln in rd.records}
    was = {int(ln.split("\t")[1]): gt_of(ln) for ln in vcf}
    touched = set(to_hom) | set(added)
    out["distrust"].update(
        rewritten_het_back_to_phased_het=sum("|" in gt_of(by_pos[p]) for p in to_hom),
        false_het_out_as_hom_ref=sum(gt_of(by_pos[p]) == "0/0" for p in added),
        untouched_calls=len(vcf) - len(touched),
        untouched_calls_changed=sum(1 for p, ln in by_pos.items() if p not in touched and gt_of(ln).replace("|", "/") not in (was[p], was[p][::-1])),
        records_dropped_as_hom_ref=sum(gt_of(ln) == "0/0" for ln in rd.records))
    out["value"] = round(out["distrust"]["phase_contig_s"] / out["plain"]["phase_contig_s"], 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""The phaser's two allele detectors side by side on one world with indel errors next to its het SNPs (tests/phase_realign_ref.py
make_realign_world: 2 Mb, ONT-like, 30x, a tenth of the (read, site) pairs with a misplaced gap beside the site), against the planted truth:
share of (read, site) alleles that are right, share of het sites phased, switch errors between adjacent phased sites, share of reads tagged and
of those tagged on the right haplotype; and the wall time of phase_contig with either rule, median of interleaved runs.  The sites are the
planted het SNPs (REF / ALT records), so the figures are the phaser's alone.  Prints one JSON line.
Usage: python tools/phase_realign_eval.py [--length L] [--seed S] [--runs N] [--out FILE]"""
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
from phase_realign_ref import het_site_alleles, make_realign_world  # noqa: E402


def figures(w, kept, pos, al, res):
    hap = np.asarray(w.hap)[kept]
    at = {int(p): k for k, p in enumerate(pos.tolist())}
    votes = np.zeros((pos.size, 2, 2), np.int64)                           # site, haplotype of origin, allele the read truly carried
    for i, r in enumerate(kept.tolist()):
        for p, c in w.meta["truth_allele"][r].items():
            k = at.get(p)
            if k is not None and c in (al[k, 0], al[k, 1]):
                votes[k, hap[i], 0 if c == al[k, 0] else 1] += 1
    t0 = (votes[:, 0, 1] > votes[:, 0, 0]).astype(np.uint8)                 # the allele haplotype 0 carries
    off, site, allele = res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]
    rid = np.repeat(np.arange(kept.size), np.diff(off))
    right = allele == (t0[site] ^ hap[rid])
    phased = res.sites["phased"]
    orient = res.sites["h"] ^ t0
    idx = np.flatnonzero(phased)
    same = res.sites["block"][idx[1:]] == res.sites["block"][idx[:-1]]
    switches = int(((orient[idx[1:]] != orient[idx[:-1]]) & same).sum())
    blk_or = {}
    for b in np.unique(res.sites["block"][idx]).tolist():
        o = orient[idx][res.sites["block"][idx] == b]
        blk_or[int(res.blocks[b][2])] = int(o.sum() * 2 > o.size)
    hp, ps = res.reads["hp"], res.reads["ps"]
    tagged = hp > 0
    exp = np.array([1 + (int(o) ^ blk_or.get(int(p), 0)) for o, p in zip(hap, ps)])
    return dict(entries=int(site.size), alleles_right=round(float(right.mean()), 5), sites=int(pos.size), sites_phased=round(float(phased.mean()), 5),
                adjacent_pairs=int(same.sum()), switch_errors=switches, reads=int(kept.size), reads_tagged=round(float(tagged.mean()), 5),
                tagged_right=round(float((hp[tagged] == exp[tagged]).mean()), 5), blocks=len(res.blocks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nanocaller_amd.phase import kept_reads, name_hash, phase_contig
    w = make_realign_world(a.seed, length=a.length, depth=30.0, read_len_scale=1.0, het_rate=1 / 1000.0)
    d = tempfile.mkdtemp(prefix="realign_eval")
    bam, fa = os.path.join(d, "w.bam"), os.path.join(d, "w.fa")
    bamio.write_bam(bam, w.chrom, w.length, [dict(r, tags={}) for r in bamio.world_to_records(w, None)], level=1)
    bamio.write_fasta(fa, w.chrom, w.ref)
    kept = kept_reads(w, False)[0]
    pos, al = het_site_alleles(w, kept)
    vcf = ["%s\t%d\t.\t%s\t%s\t30.00\tPASS\t.\tGT:GQ\t0/1:30\n" % (w.chrom, p, "AGTC"[x], "AGTC"[y]) for p, (x, y) in zip(pos.tolist(), al.tolist())]
    out = dict(metric="phase_realign_eval", length=a.length, seed=a.seed, planted_pairs=len(w.meta["planted"]), runs=a.runs)
    walls = dict(column=[], realign=[])
    res = {}
    for k in ("column", "realign"):                                        # warm: the decode and the packs of both routes stay cached
        res[k] = phase_contig(bam, fa, w.chrom, vcf, 10, False, realign=k == "realign")
        assert np.array_equal(res[k].reads["hash"], name_hash([w.names[r] for r in kept.tolist()]))
        out[k] = figures(w, kept, pos, al, res[k])
    for _ in range(a.runs):
        for k in walls:
            t = time.perf_counter()
            r = phase_contig(bam, fa, w.chrom, vcf, 10, False, realign=k == "realign")
            walls[k].append(time.perf_counter() - t)
            out[k]["stage_ms"] = {s: round(float(v), 3) for s, v in r.ms.items()}
    for k in walls:
        out[k]["phase_contig_s"] = round(float(np.median(walls[k])), 4)
    out["value"] = round(out["realign"]["phase_contig_s"] / out["column"]["phase_contig_s"], 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""The phaser's unit-cost model and its weighted model (phase_contig(weighted=True): base qualities as flip costs, a MAPQ floor) side by side on
one world with two planted effects, against the planted truth.  The world is tools/phase_realign_eval.py's (2 Mb, ONT-like, 30x, het SNPs about
every kb); its records get base qualities -- a share `--low-share` of the bases low (Q2-8), the rest Q15-40 -- and
  * substitution errors concentrated on the low-quality bases: a low-quality aligned base is replaced with probability `--low-error`, any other
    with `--high-error`;
  * a share `--paralog-share` of the reads with MAPQ 0-19 (every other read MAPQ 60) that carries a paralog's alleles: at every het site one
    fixed random allele of the two, the same for all such reads, whatever haplotype the read was drawn from.
Both modes run on the same records: share of (read, site) alleles that are right, switch errors between adjacent phased sites, share of reads
tagged and of the tagged reads on the right haplotype (reads that are not paralog reads), and phase_contig's wall time, median of interleaved runs.
Prints one JSON line.
Usage: python tools/phase_weighted_eval.py [--length L] [--seed S] [--runs N] [--low-share F] [--low-error F] [--high-error F] [--paralog-share F] [--out FILE]"""
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
import bamio_w  # noqa: E402
from phase_realign_ref import het_site_alleles, make_realign_world  # noqa: E402


def plant(w, recs, pos, al, rng, low_share, low_error, high_error, paralog_share):
    """qualities, substitution errors and paralog reads written into the records -> (is_paralog bool per record, errors planted)"""
    letters = np.frombuffer(b"AGTC", np.uint8)
    para_allele = rng.integers(0, 2, pos.size)                           # the paralog's allele at every het site
    is_para = rng.random(len(recs)) < paralog_share
    n_err = 0
    for k, r in enumerate(recs):
        seq = np.frombuffer(r["seq"].encode("ascii"), np.uint8).copy()
        L = seq.size
        low = rng.random(L) < low_share
        qual = np.where(low, rng.integers(2, 9, L), rng.integers(15, 41, L)).astype(np.uint8)
        aligned = np.zeros(L, bool)
        rp, qp = r["pos0"] + 1, 0
        for op, n in r["cigar"]:
            if op in "M=X":
                aligned[qp:qp + n] = True
                if is_para[k]:                                           # the paralog's alleles at the het sites of this run
                    a, b = np.searchsorted(pos, rp), np.searchsorted(pos, rp + n)
                    for s in range(a, b):
                        seq[qp + int(pos[s]) - rp] = letters[al[s, para_allele[s]]]
            if op in "MDN=X":
                rp += n
            if op in "MIS=X":
                qp += n
        hit = aligned & (rng.random(L) < np.where(low, low_error, high_error))
        code = np.searchsorted(np.sort(letters), seq[hit])               # any other base of the four
        other = np.sort(letters)[(code + rng.integers(1, 4, int(hit.sum()))) % 4]
        seq[hit] = np.where(np.isin(seq[hit], letters), other, seq[hit])
        n_err += int(hit.sum())
        r["seq"], r["qual"], r["tags"] = seq.tobytes().decode("ascii"), qual.tobytes(), {}
        r["mapq"] = int(rng.integers(0, 20)) if is_para[k] else 60
    return is_para, n_err


def figures(w, kept, pos, al, res, is_para):
    hap = np.asarray(w.hap)[kept]
    para = is_para[kept]
    at = {int(p): k for k, p in enumerate(pos.tolist())}
    votes = np.zeros((pos.size, 2, 2), np.int64)                          # site, haplotype of origin, allele the read truly carried
    for i, r in enumerate(kept.tolist()):
        for p, c in w.meta["truth_allele"][r].items():
            k = at.get(p)
            if k is not None and c in (al[k, 0], al[k, 1]):
                votes[k, hap[i], 0 if c == al[k, 0] else 1] += 1
    t0 = (votes[:, 0, 1] > votes[:, 0, 0]).astype(np.uint8)                # the allele haplotype 0 carries
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
    tagged = (hp > 0) & ~para
    exp = np.array([1 + (int(o) ^ blk_or.get(int(p), 0)) for o, p in zip(hap, ps)])
    out = dict(entries=int(site.size), alleles_right=round(float(right.mean()), 5), sites=int(pos.size), sites_phased=round(float(phased.mean()), 5),
               adjacent_pairs=int(same.sum()), switch_errors=switches, reads=int((~para).sum()), reads_tagged=round(float(tagged.sum() / (~para).sum()), 5),
               tagged_right=round(float((hp[tagged] == exp[tagged]).mean()), 5), paralog_reads=int(para.sum()), paralog_reads_accepted=int((res.reads["side"][para] >= 0).sum()),
               blocks=len(res.blocks), mec_cost=int(sum(b[3] for b in res.blocks)))
    if "entry_weight" in res.reads:
        ew = res.reads["entry_weight"].astype(np.int64)
        out.update(weight_share_on_wrong_alleles=round(float(ew[~right].sum() / max(1, ew.sum())), 5), wrong_alleles_share=round(float((~right).mean()), 5))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--low-share", type=float, default=0.15)
    ap.add_argument("--low-error", type=float, default=0.4)
    ap.add_argument("--high-error", type=float, default=0.005)
    ap.add_argument("--paralog-share", type=float, default=0.08)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nanocaller_amd.phase import kept_reads, phase_contig
    w = make_realign_world(a.seed, length=a.length, depth=30.0, read_len_scale=1.0, het_rate=1 / 1000.0)
    kept = kept_reads(w, False)[0]
    pos, al = het_site_alleles(w, kept)
    rng = np.random.default_rng(a.seed)
    recs = bamio.world_to_records(w, None)
    is_para, n_err = plant(w, recs, pos, al, rng, a.low_share, a.low_error, a.high_error, a.paralog_share)
    d = tempfile.mkdtemp(prefix="weighted_eval")
    bam, fa = os.path.join(d, "w.bam"), os.path.join(d, "w.fa")
    bamio_w.write_bam(bam, w.chrom, w.length, recs, level=1)
    bamio.write_fasta(fa, w.chrom, w.ref)
    vcf = ["%s\t%d\t.\t%s\t%s\t30.00\tPASS\t.\tGT:GQ\t0/1:30\n" % (w.chrom, p, "AGTC"[x], "AGTC"[y]) for p, (x, y) in zip(pos.tolist(), al.tolist())]
    out = dict(metric="phase_weighted_eval", length=a.length, seed=a.seed, runs=a.runs, low_share=a.low_share, low_error=a.low_error,
               high_error=a.high_error, paralog_share=a.paralog_share, substitutions_planted=n_err, mapq_min=20, default_weight=30, w_max=93)
    modes = dict(plain={}, weighted=dict(weighted=True))
    walls = {k: [] for k in modes}
    for k, kw in modes.items():                                            # warm: the decode and the packs stay cached
        out[k] = figures(w, kept, pos, al, phase_contig(bam, fa, w.chrom, vcf, 10, False, **kw), is_para)
    for _ in range(a.runs):
        for k, kw in modes.items():
            t = time.perf_counter()
            r = phase_contig(bam, fa, w.chrom, vcf, 10, False, **kw)
            walls[k].append(time.perf_counter() - t)
            out[k]["stage_ms"] = {s: round(float(v), 3) for s, v in r.ms.items()}
    for k in walls:
        out[k]["phase_contig_s"] = round(float(np.median(walls[k])), 4)
    out["value"] = round(out["plain"]["switch_errors"] / max(1, out["weighted"]["switch_errors"]), 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

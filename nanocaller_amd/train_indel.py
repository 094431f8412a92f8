"""Training and fine-tuning of the diploid indel model on the GPU.

Replaces the reference's misc/training/model_run_indels.py, model_architect_indel.py and generate_indel_pileups.py (TensorFlow 1, pysam, 46 KB
of text per example): labelled sites come from the device indel pipeline (its `x` is the network's input as it is), the forward / backward
pass and TensorFlow-form Adam are the HIP kernels of csrc/nc_train_indel.hip.  torch is plumbing only: device memory, the dropout mask's
random generator, casts.

    tr = IndelTrainer(init="ONT-HG002", lr=1e-4)          # or init=None: Xavier-uniform from the seed
    x, labels, pos, depth = indel_training_examples(params, truth_vcf, confident_bed)[chrom]
    tr.step(x, labels); tr.evaluate(x, labels); tr.save("model-1.ncw", depth)
    python -m nanocaller_amd.train_indel -bam x.bam -ref x.fa -vcf truth.vcf.gz -bed confident.bed -chrom chr20:1-1000000 -o out_dir

The result is used as indel_model='/path/model-N.ncw'.
"""
from __future__ import annotations

import numpy as np

from . import train_common
from .genotype_sites import LONG_INDEL
from .train import _read_text, in_bed, parse_bed
from .train_common import IndelFamilyTrainer, add_train_args, class_recall, indel_params, initial_blob, run_epochs, subsample_negatives, weighted_coverage
from .weights import KIND_INDEL, get_indel_model

LOSS_KEYS = ("cost", "CE")
N_CLASSES = 4
# genotype -> class, generate_indel_pileups.py:9 of misc/training
GT_MAP = {(0, 0): 0, (1, 1): 1, (0, 1): 2, (1, 0): 2, (1, 2): 3, (2, 1): 3}
CLASS_UNKNOWN = 255           # an indel record whose genotype GT_MAP does not hold: every site that sees it is ambiguous
WINDOW = 128                  # columns of a site's tensor behind its anchor
LABEL_REACH = 40              # the reference's farthest labelled offset (generate_indel_pileups.py:137-141 of misc/training)
CHUNK = 100_000               # bases per chunk of the device pipeline (its limit is 130 kb)
DROP_KEYS = ("outside_bed", "ambiguous", "negatives_subsampled")


def xavier_init(seed=0):
    """train_common.xavier_init for the diploid indel model"""
    return train_common.xavier_init(KIND_INDEL, seed)


def blob_tensors(flat):
    """train_common.blob_tensors for the diploid indel model"""
    return train_common.blob_tensors(flat, KIND_INDEL)


# ------------------------------------------------------------------ labels (pure host code)
def parse_indel_records(text, chrom, classify):
    """VCF text -> (pos int64 ascending, class uint8, is_long uint8) of the indel records of `chrom`: a record counts when some ALT length
    differs from REF's and is long when the difference exceeds 10 (genotype_sites.parse_indel_sites_vcf's test); its class is
    classify(the first sample's GT as a list of digit strings), CLASS_UNKNOWN where that gives None or the GT is not all digits.  SNP lines
    and other contigs are skipped."""
    rows = []
    for ln in text.splitlines():
        if not ln or ln[0] == "#":
            continue
        f = ln.split("\t")
        if len(f) < 5 or f[0] != chrom or not f[1].isdigit():
            continue
        d = [abs(len(a) - len(f[3])) for a in f[4].split(",")]
        if not any(d):
            continue
        cls = None
        if len(f) >= 10 and "GT" in f[8].split(":"):
            g = f[9].split(":")[f[8].split(":").index("GT")].replace("|", "/").split("/")
            if all(v.isdigit() for v in g):
                cls = classify(g)
        rows.append((int(f[1]), CLASS_UNKNOWN if cls is None else cls, max(d) > LONG_INDEL))
    rows.sort()
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.uint8), np.array([r[2] for r in rows], np.uint8))


def parse_truth_indels(text, chrom):
    """parse_indel_records with the diploid classes: a two-copy genotype through GT_MAP, CLASS_UNKNOWN for any other genotype"""
    return parse_indel_records(text, chrom, lambda g: GT_MAP.get((int(g[0]), int(g[1]))) if len(g) == 2 else None)


def world_truth(world):
    """the planted truth of a synth.World decorated by add_indels -> (pos, class, is_long): every planted site is heterozygous, class 2"""
    if "indel_sites" not in world.meta:
        raise ValueError("world_truth: the world carries no planted indel sites (synth.add_indels records them)")
    pos, length = world.meta["indel_sites"]
    order = np.argsort(pos, kind="stable")
    pos, length = np.asarray(pos, np.int64)[order], np.asarray(length, np.int64)[order]
    return pos, np.full(pos.size, 2, np.uint8), (np.abs(length) > LONG_INDEL).astype(np.uint8)


def label_sites(pos, truth_pos, truth_class, intervals=None, neg_ratio=2.0, seed=0):
    """The labelling rule.  pos: the sites' anchors (1-based); truth_pos (ascending) / truth_class: the truth indel records; intervals:
    parse_bed's (None: everywhere).  A site outside the intervals is dropped.  Of the records with pos <= POS < pos + 128: none -> class 0;
    all of one class and at least one of them within [pos, pos + 40] -> that class; anything else -> dropped as ambiguous.  Class-0 sites
    are then subsampled to neg_ratio x the count of the others with a seeded generator (None, or no other site: all kept).
    -> (indices into pos, ascending; labels uint8; dropped: dict of counts by reason, DROP_KEYS)"""
    pos = np.asarray(pos, np.int64)
    truth_pos, truth_class = np.asarray(truth_pos, np.int64), np.asarray(truth_class, np.uint8)
    inside = in_bed(intervals, pos) if intervals is not None else np.ones(pos.shape, bool)
    lo, hi = np.searchsorted(truth_pos, pos, "left"), np.searchsorted(truth_pos, pos + WINDOW, "left")
    near = np.searchsorted(truth_pos, pos + LABEL_REACH, "right")
    labels = np.zeros(pos.size, np.uint8)
    ok = inside.copy()
    for i in np.nonzero(inside & (hi > lo))[0]:
        c = truth_class[lo[i]:hi[i]]
        if (c == c[0]).all() and c[0] != CLASS_UNKNOWN and near[i] > lo[i]:
            labels[i] = c[0]
        else:
            ok[i] = False
    dropped = dict(outside_bed=int((~inside).sum()), ambiguous=int((inside & ~ok).sum()), negatives_subsampled=0)
    neg, lab = np.nonzero(ok & (labels == 0))[0], np.nonzero(ok & (labels != 0))[0]
    neg, dropped["negatives_subsampled"] = subsample_negatives(neg, lab.size, neg_ratio, seed)
    idx = np.sort(np.concatenate([lab, neg]))
    return idx, labels[idx], dropped


def indel_examples(who, params, truth_vcf, confident_bed, neg_ratio, seed, device, parse, label, haploid, listed):
    """What indel_training_examples and train_haploid.haploid_indel_training_examples do, -> (their result, the dropped counts per contig).
    who: the caller's name for the error texts; parse(vcf text, chrom) -> the truth records; label: the labelling rule (label_sites'
    arguments and result); haploid: the pipeline's form; listed(classes) -> the mask of the truth records that are handed to the pipeline."""
    import torch

    from .generate_indel_pileups import indel_sites_for_chunks, plan_routes
    from .synth import World
    src = params["sam_path"]
    if not isinstance(src, str):
        raise ValueError("%s: the device indel pipeline reads a BAM file; sam_path is %s (a synth.World gives the truth as params['truth'], its reads "
                         "come from a BAM written from it)" % (who, type(src).__name__))
    vcf_text = _read_text(truth_vcf) if truth_vcf is not None else None
    bed_text = _read_text(confident_bed) if confident_bed is not None else None
    out, dropped = {}, {}
    for k, (chrom, start, end) in enumerate(params["chrom_list"]):
        if vcf_text is not None:
            truth = parse(vcf_text, chrom)
        elif isinstance(params.get("truth"), World):
            truth = world_truth(params["truth"]) if params["truth"].chrom == chrom else None
        elif isinstance(params.get("truth"), dict):
            truth = params["truth"].get(chrom)
        else:
            raise ValueError("%s: a truth VCF, or params['truth'] = a synth.World or {chrom: (pos, class, is_long)}" % who)
        if truth is None:
            truth = (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        intervals = parse_bed(bed_text, chrom) if bed_text is not None else None
        keep = listed(np.asarray(truth[1]))
        dct = dict(params, genotype_indel_sites={chrom: (np.asarray(truth[0])[keep], np.asarray(truth[2])[keep])}, genotype_indel_only=False,
                   impute_indel_phase=False)
        dct.setdefault("supplementary", False)
        dct.setdefault("exclude_bed", None)
        chunks = [dict(chrom=chrom, start=a, end=min(a + CHUNK - 1, end), sam_path=src) for a in range(start, end + 1, CHUNK)]
        if [kind for kind, _, _ in plan_routes(dct, chunks, haploid, device=device)] != ["device"]:
            raise ValueError("%s: %s:%d-%d does not take the device indel pipeline" % (who, chrom, start, end))
        r, _, _ = indel_sites_for_chunks(dct, chunks, device, haploid)
        if r["n"] == 0:
            continue
        pos = r["pos"].astype(np.int64)
        idx, labels, dropped[chrom] = label(pos, truth[0], truth[1], intervals, neg_ratio, seed + k)
        if idx.size == 0:
            continue
        x = r["x"][torch.from_numpy(idx).to(r["x"].device)].contiguous()
        out[chrom] = (x, labels, pos[idx], _mean_depth(dct, chunks, device, start, end))
    return out, dropped


def indel_training_examples(params, truth_vcf=None, confident_bed=None, neg_ratio=2.0, seed=0, device=0):
    """Labelled sites per contig: {chrom: (x float32 [n][15][128][2] device tensor, labels uint8 [n] numpy, pos int64 [n] numpy, mean depth)};
    the counts of dropped sites by reason (DROP_KEYS) per contig are in indel_training_examples.dropped afterwards.

    params: the indel step's dict (sam_path: a haplotagged BAM -- HP / PS tags or <contig>.haplotags.npz --, fasta_path, mincov, maxcov,
    win_size, small_win_size, ins_t, del_t, seq, ...), plus 'chrom_list' = [(chrom, start, end)].  The truth is truth_vcf, or with
    truth_vcf=None params['truth']: a synth.World decorated by add_indels whose reads the BAM holds (its planted sites, all class 2) or
    {chrom: (pos, class, is_long)}.  The truth records are handed to the device pipeline as genotype_indel_sites in add mode, so the sites are
    the scan's own candidates + the anchors the truth columns make.  Only the device pipeline runs: chunks that would take the host-assembled
    route raise ValueError.  Deviation from the reference's generator: negatives are candidates that hold no truth record, not columns sampled
    by event frequency, because only candidates ever reach the model."""
    out, indel_training_examples.dropped = indel_examples("indel_training_examples", params, truth_vcf, confident_bed, neg_ratio, seed, device,
                                                          parse_truth_indels, label_sites, False, lambda cls: np.ones(cls.size, bool))
    return out


def _mean_depth(dct, chunks, device, start, end):
    """mean depth of the kept reads over [start, end] (the pack the pipeline has just used is cached)"""
    from .indel_device import indel_pack_for
    _, dp, _, _, _, _ = indel_pack_for(dct, chunks, device, by_name=True)
    n = int(dp.reads["n_reads"])
    a, b = dp.reads["rd_start"][:n].long().clamp(min=start), dp.reads["rd_end"][:n].long().clamp(max=end + 1)
    return float((b - a).clamp(min=0).sum().item()) / float(end - start + 1)


# ------------------------------------------------------------------ the trainer
class IndelTrainer(IndelFamilyTrainer):
    """One trainer per engine context.  init: a built-in indel model name, an .ncw path, a canonical blob (numpy), or None = Xavier-uniform
    from `seed`.  slice_sites: sites per workspace slice (765 KB each); 0 = min(max_batch, 1024)."""

    PREFIX, KIND, X_SHAPE, PROBS_TAIL = "nc_indel_train", KIND_INDEL, (15, 128, 2), (N_CLASSES,)
    LABEL_TEXT = "one class in 0..3 per site"

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-5, keep=0.5, seed=0, max_batch=1024, slice_sites=0, kind=KIND_INDEL,
                 beta1=0.9, beta2=0.999, eps=1e-8):
        if kind != KIND_INDEL:
            raise ValueError("IndelTrainer: only the diploid indel model (kind %d) is trained, not kind %d" % (KIND_INDEL, kind))
        flat = initial_blob("IndelTrainer", init, KIND_INDEL, seed, get_indel_model)
        self._open(device, flat, lr, gamma, keep, seed, max_batch, (beta1, beta2, eps), int(slice_sites))

    def _labels(self, labels, n):
        """(the device call does not look at this model's labels: a class above 3 is refused here)"""
        labels = super()._labels(labels, n)
        if labels is not None and int(labels.max()) >= N_CLASSES:
            raise ValueError("IndelTrainer: %s" % self.LABEL_TEXT)
        return labels

    def evaluate(self, x, labels):
        """keep = 1: cost, CE, the overall accuracy as model_run_indels.py:126-137 counts it (argmax of the four probabilities against the
        label), the recall per class ('recall': four floats, NaN for a class the batch does not hold) and 'probs', the device tensor"""
        import torch
        losses, _ = self.loss_grad(x, labels, None, 1.0, want_grad=False)
        probs = self.forward(x)
        lab = torch.as_tensor(labels).to(self.device).long()
        hit = probs.argmax(1) == lab
        out = dict(losses)
        out.update(acc=float(hit.float().mean().item()), recall=class_recall(hit, lab, N_CLASSES), probs=probs)
        return out


def _pooled_recall(ev, labs):
    """val_recall: the batches' recalls pooled by class over the whole validation set"""
    hits = np.array([[0.0 if np.isnan(r) else r * float((lab == c).sum()) for c, r in enumerate(e["recall"])] for lab, e in zip(labs, ev)]).sum(0)
    cnt = np.array([sum(float((lab == c).sum()) for lab in labs) for c in range(N_CLASSES)])
    return dict(val_recall=[float(h / c) if c else float("nan") for h, c in zip(hits, cnt)])


def train_indel_model(params):
    """Epochs over the contigs of params['chrom_list'] with a validation split; writes <out_dir>/model-<epoch>.ncw.
    params: indel_training_examples' keys + truth_vcf, confident_bed, out_dir, and optionally epochs (10), batch (256), lr (1e-3), gamma (1e-5),
    keep (0.5), seed, init (model to fine-tune), val_frac (0.1), neg_ratio (2).  -> list of per-epoch dicts (train cost, validation cost / CE /
    accuracy / recalls, path)"""
    seed = int(params.get("seed", 0))
    ex = indel_training_examples(params, params.get("truth_vcf"), params.get("confident_bed"), params.get("neg_ratio", 2.0), seed, params.get("device", 0))
    return train_on_indel_examples("train_indel_model", IndelTrainer, ex, params, _pooled_recall)


def train_on_indel_examples(who, trainer, ex, params, val_extra=None):
    """the epochs of train_indel_model / train_haploid.train_haploid_indel_model over the examples `ex` of a *_indel_training_examples"""
    import torch
    if not ex:
        raise ValueError("%s: no labelled site" % who)
    batch = int(params.get("batch", 256))
    x = torch.cat([v[0] for v in ex.values()])
    lab = torch.from_numpy(np.concatenate([v[1] for v in ex.values()])).to(x.device)
    tr = trainer(params.get("device", 0), params.get("init"), params.get("lr", 1e-3), params.get("gamma", 1e-5), params.get("keep", 0.5),
                 int(params.get("seed", 0)), max_batch=max(batch, 1))
    return run_epochs(tr, (x,), lab, params, batch, weighted_coverage([v[0].shape[0] for v in ex.values()], [v[3] for v in ex.values()]),
                      ("cost", "CE", "acc"), val_extra)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nanocaller_amd.train_indel", description="train or fine-tune the diploid indel model on the GPU")
    add_train_args(ap, False, "indel model name or .ncw file to fine-tune (default: Xavier-uniform)", "haplotagged BAM (HP / PS tags)")
    a = ap.parse_args(argv)
    train_indel_model(indel_params(a))


if __name__ == "__main__":
    main()

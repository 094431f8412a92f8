"""Training and fine-tuning of the haploid SNP and indel models on the GPU.

The reference ships one haploid SNP model and one haploid indel model (CHM13) and no script that made them; every haploid contig (chrX / chrY
of a male sample, chrM, --haploid_genome) is called with them.  Here they are trained like the diploid ones (train.py, train_indel.py):
labelled sites come from the device scan + featuriser, or the device indel pipeline, on haploid chunks; the forward / backward pass and
TensorFlow-form Adam are the HIP kernels of csrc/nc_train_hap.hip and csrc/nc_train_hap_indel.hip.  torch is plumbing only: device memory,
the dropout mask's random generator, casts.

    tr = HaploidSnpTrainer(init="haploid", lr=1e-4)       # or an .ncw of kind KIND_SNP_HAP, or None: Xavier-uniform from the seed
    x, ref_code, labels, pos, depth = haploid_snp_training_examples(params, truth_vcf, confident_bed)[chrom]
    tr.step(x, ref_code, labels); tr.evaluate(x, ref_code, labels); tr.save("model-1.ncw", depth)
    python -m nanocaller_amd.train_haploid snp -bam x.bam -ref x.fa -vcf truth.vcf.gz -bed confident.bed -chrom chrX:1-1000000 -o out_dir

    tr = HaploidIndelTrainer(init="haploid", lr=1e-4)
    x, labels, pos, depth = haploid_indel_training_examples(params, truth_vcf, confident_bed)[chrom]
    tr.step(x, labels); tr.evaluate(x, labels); tr.save("model-1.ncw", depth)
    python -m nanocaller_amd.train_haploid indel -bam x.bam -ref x.fa -vcf truth.vcf.gz -bed confident.bed -chrom chrX:1-1000000 -o out_dir

The results are used as params['haploid_snp_model'] / params['haploid_indel_model'] = '/path/model-N.ncw' (or NC_HAPLOID_SNP_MODEL /
NC_HAPLOID_INDEL_MODEL).
"""
from __future__ import annotations

import numpy as np

from . import train_common
from .train import BASE_CODE, _read_text, in_bed, parse_bed, world_truth
from .train_common import (IndelFamilyTrainer, SnpFamilyTrainer, add_train_args, class_recall, indel_params, initial_blob, run_epochs, snp_params,
                           subsample_negatives, weighted_coverage)
from .train_indel import CLASS_UNKNOWN, LABEL_REACH, WINDOW, indel_examples, parse_indel_records, train_on_indel_examples
from .weights import KIND_INDEL_HAP, KIND_SNP_HAP, get_indel_model, get_SNP_model

LOSS_KEYS = ("cost", "CE")
AMBIGUOUS = -1                # a truth record that does not say which single base a haploid sample has
DROP_KEYS = ("outside_bed", "ambiguous", "negatives_subsampled")


def xavier_init(kind=KIND_SNP_HAP, seed=0):
    """train_common.xavier_init, by default for the haploid SNP model"""
    return train_common.xavier_init(kind, seed)


def blob_tensors(flat, kind=KIND_SNP_HAP):
    """train_common.blob_tensors, by default for the haploid SNP model"""
    return train_common.blob_tensors(flat, kind)


# ------------------------------------------------------------------ labels (pure host code)
def parse_haploid_truth_vcf(text, chrom):
    """VCF text -> {pos: base code A0 G1 T2 C3, or AMBIGUOUS}.  A record whose first sample's genotype names one ALT allele on every copy
    ('1', '1/1', '1|1') with single-base REF and ALT gives that ALT base; every other record of the contig (a heterozygous or reference
    genotype, an indel or multi-base allele, no GT) is AMBIGUOUS: the site is dropped, not labelled with its reference base."""
    out = {}
    for ln in text.splitlines():
        if not ln or ln[0] == "#":
            continue
        f = ln.split("\t")
        if len(f) < 5 or f[0] != chrom or not f[1].isdigit():
            continue
        code = AMBIGUOUS
        alts = f[4].split(",")
        if len(f) >= 10 and "GT" in f[8].split(":") and len(f[3]) == 1:
            g = f[9].split(":")[f[8].split(":").index("GT")].replace("|", "/").split("/")
            if 1 <= len(g) <= 2 and all(v.isdigit() for v in g) and len(set(g)) == 1 and 1 <= int(g[0]) <= len(alts):
                code = BASE_CODE.get(alts[int(g[0]) - 1].upper(), AMBIGUOUS)
        pos = int(f[1])
        out[pos] = code if pos not in out else AMBIGUOUS               # two records at one position: ambiguous
    return out


def haploid_world_truth(world):
    """the planted truth of a synth.World read as a haploid sample: homozygous sites carry their base, heterozygous ones are AMBIGUOUS"""
    return {p: (a if gt == 0 and a == b else AMBIGUOUS) for p, (gt, a, b) in world_truth(world).items()}


def label_haploid_sites(pos, ref_code, truth, intervals=None, neg_ratio=2.0, seed=0):
    """The labelling rule.  pos (1-based), ref_code (A0 G1 T2 C3) of the featurised sites; truth = parse_haploid_truth_vcf's map; intervals =
    parse_bed's (None: everywhere).  Sites outside the intervals are dropped; a truth site takes its ALT base, an AMBIGUOUS one is dropped;
    every other site takes its reference base, and those are subsampled to neg_ratio x the count of labelled truth sites with a seeded
    generator (all kept when there is none or neg_ratio is None).
    -> (indices into pos, ascending; labels uint8 [k]; dropped: dict of counts by reason, DROP_KEYS)"""
    pos = np.asarray(pos, np.int64)
    ref_code = np.asarray(ref_code, np.int64)
    inside = in_bed(intervals, pos) if intervals is not None else np.ones(pos.shape, bool)
    code = np.fromiter((truth.get(int(p), -2) for p in pos), np.int64, pos.size)          # -2: no truth record
    amb = inside & (code == AMBIGUOUS)
    is_truth = inside & (code >= 0)
    neg = np.nonzero(inside & (code == -2))[0]
    dropped = dict(outside_bed=int((~inside).sum()), ambiguous=int(amb.sum()), negatives_subsampled=0)
    neg, dropped["negatives_subsampled"] = subsample_negatives(neg, int(is_truth.sum()), neg_ratio, seed)
    idx = np.sort(np.concatenate([np.nonzero(is_truth)[0], neg]))
    labels = np.where(is_truth[idx], code[idx], ref_code[idx]).astype(np.uint8)
    return idx, labels, dropped


def haploid_snp_training_examples(params, truth_vcf=None, confident_bed=None, neg_ratio=2.0, seed=0, device=0):
    """Labelled sites per contig: {chrom: (x float32 [n][5][41][5] device tensor, ref_code int32 [n] device tensor, labels uint8 [n] numpy,
    pos int64 [n] numpy, mean depth)}; the counts of dropped sites by reason (DROP_KEYS) per contig are in
    haploid_snp_training_examples.dropped afterwards.

    params: the SNP step's dict plus 'chrom_list' = [(chrom, start, end)], as train.snp_training_examples takes it; the contig's chunks are
    scanned as haploid.  sam_path may be a synth.World: truth_vcf=None then takes its planted truth (haploid_world_truth), confident_bed=None
    means everywhere.  Sites = the haploid scan's candidates + the truth positions, the latter handed over as a genotype_sites list."""
    import torch

    from .generate_SNP_pileups import get_snp_testing_candidates
    from .synth import World
    src = params["sam_path"]
    out, dropped = {}, {}
    regions = params.get("chrom_list")
    if regions is None and isinstance(src, World):
        regions = [(src.chrom, 1, src.length)]
    vcf_text = _read_text(truth_vcf) if truth_vcf is not None else None
    bed_text = _read_text(confident_bed) if confident_bed is not None else None
    for k, (chrom, start, end) in enumerate(regions):
        if vcf_text is not None:
            truth = parse_haploid_truth_vcf(vcf_text, chrom)
        elif isinstance(src, World):
            truth = haploid_world_truth(src)
        else:
            raise ValueError("haploid_snp_training_examples: a truth VCF is needed unless sam_path is a synth.World")
        intervals = parse_bed(bed_text, chrom) if bed_text is not None else None
        dct = dict(params)
        dct["genotype_sites"] = {chrom: np.fromiter(truth.keys(), np.int64, len(truth))}
        dct["genotype_only"] = False
        pos, ref1h, mat, _, _, depth, _, _ = get_snp_testing_candidates(dct, dict(chrom=chrom, start=start, end=end, ploidy="haploid"), device)
        if len(pos) == 0:
            continue
        ref_code = np.argmax(ref1h, 1).astype(np.int32)
        idx, labels, dropped[chrom] = label_haploid_sites(pos, ref_code, truth, intervals, neg_ratio, seed + k)
        if idx.size == 0:
            continue
        dev = torch.device("cuda", device)
        out[chrom] = (torch.from_numpy(np.ascontiguousarray(mat[idx], np.float32)).to(dev), torch.from_numpy(ref_code[idx]).to(dev), labels,
                      np.asarray(pos)[idx], float(depth))
    haploid_snp_training_examples.dropped = dropped
    return out


# ------------------------------------------------------------------ the trainer
class HaploidSnpTrainer(SnpFamilyTrainer):
    """One trainer per engine context.  init: 'haploid' (the shipped CHM13 model), an .ncw path of kind KIND_SNP_HAP, a canonical blob
    (numpy), or None = Xavier-uniform from `seed`."""

    PREFIX, KIND, LABEL_TEXT = "nc_hap_train", KIND_SNP_HAP, "one base A0 G1 T2 C3 per site"

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-3, keep=0.5, seed=0, max_batch=4096, beta1=0.9, beta2=0.999, eps=1e-8):
        flat = initial_blob("HaploidSnpTrainer", init, self.KIND, seed, lambda name: get_SNP_model(name)[0])
        self._open(device, flat, lr, gamma, keep, seed, max_batch, (beta1, beta2, eps))

    def evaluate(self, x, ref_code, labels, scale=None):
        """keep = 1: cost, CE, 'acc' (argmax of the four probabilities against the label), 'recall' per base A, G, T, C (NaN for a base the
        batch does not hold) and 'probs', the device tensor"""
        import torch
        losses, _ = self.loss_grad(x, ref_code, labels, None, 1.0, scale, want_grad=False)
        probs = self.forward(x, ref_code, scale)
        lab = torch.as_tensor(labels).to(self.device).long()
        hit = probs.argmax(1) == lab
        out = dict(losses)
        out.update(acc=float(hit.float().mean().item()), recall=class_recall(hit, lab, 4), probs=probs)
        return out


def train_haploid_snp_model(params):
    """Epochs over the contigs of params['chrom_list'] with a validation split; writes <out_dir>/model-<epoch>.ncw, each carrying
    train_coverage = the mean depth of its training sites.  params: the SNP step's keys + truth_vcf, confident_bed, out_dir, and optionally
    epochs (10), batch (1024), lr (1e-3), gamma (1e-3), keep (0.5), seed, init ('haploid' or a file to fine-tune), val_frac (0.1), neg_ratio (2).
    -> list of per-epoch dicts (train cost, validation cost / CE / accuracy, path)"""
    import torch
    seed = int(params.get("seed", 0))
    batch = int(params.get("batch", 1024))
    ex = haploid_snp_training_examples(params, params.get("truth_vcf"), params.get("confident_bed"), params.get("neg_ratio", 2.0), seed,
                                       params.get("device", 0))
    if not ex:
        raise ValueError("train_haploid_snp_model: no labelled site")
    x = torch.cat([v[0] for v in ex.values()])
    ref = torch.cat([v[1] for v in ex.values()])
    lab = torch.from_numpy(np.concatenate([v[2] for v in ex.values()])).to(x.device)
    tr = HaploidSnpTrainer(params.get("device", 0), params.get("init"), params.get("lr", 1e-3), params.get("gamma", 1e-3), params.get("keep", 0.5), seed,
                           max_batch=max(batch, 1))
    return run_epochs(tr, (x, ref), lab, params, batch, weighted_coverage([v[0].shape[0] for v in ex.values()], [v[4] for v in ex.values()]),
                      ("cost", "CE", "acc"))


# ------------------------------------------------------------------ the haploid indel model
def parse_haploid_truth_indels(text, chrom):
    """VCF text -> (pos int64 ascending, class uint8, is_long uint8) of the indel records of `chrom`, as train_indel.parse_truth_indels reads
    them (a record counts when some ALT length differs from REF's, long when the difference exceeds 10), with the two classes of a haploid
    sample: 1 when the first sample's genotype, written for one copy or two ('1', '1/1', '0|1', ...), names an ALT allele, 0 when it names
    only the reference, CLASS_UNKNOWN for anything else."""
    return parse_indel_records(text, chrom, lambda g: (1 if any(int(v) for v in g) else 0) if len(g) <= 2 else None)


def label_haploid_indel_sites(pos, truth_pos, truth_class, intervals=None, neg_ratio=2.0, seed=0):
    """The labelling rule of train_indel.label_sites with two classes.  pos: the sites' anchors (1-based); truth_pos (ascending) /
    truth_class: parse_haploid_truth_indels' records (train_indel.world_truth's serve as well); a record of class 0 (a 0/0 genotype) says that there is no indel and is no record
    here.  A site outside the intervals is dropped.  Of the records with pos <= POS < pos + 128: none -> 0; at least one within
    [pos, pos + 40] -> 1; only beyond 40 -> dropped; a record without a usable genotype anywhere in the window -> dropped.  Class-0 sites are
    then subsampled to neg_ratio x the count of class-1 sites with a seeded generator (None, or no class-1 site: all kept).
    -> (indices into pos, ascending; labels uint8; dropped: dict of counts by reason, INDEL_DROP_KEYS)"""
    pos = np.asarray(pos, np.int64)
    truth_pos, truth_class = np.asarray(truth_pos, np.int64), np.asarray(truth_class, np.uint8)
    unknown = np.sort(truth_pos[truth_class == CLASS_UNKNOWN])
    tp = truth_pos[(truth_class != 0) & (truth_class != CLASS_UNKNOWN)]
    inside = in_bed(intervals, pos) if intervals is not None else np.ones(pos.shape, bool)
    in_window = np.searchsorted(tp, pos + WINDOW, "left") > np.searchsorted(tp, pos, "left")
    in_reach = np.searchsorted(tp, pos + LABEL_REACH, "right") > np.searchsorted(tp, pos, "left")
    has_unknown = np.searchsorted(unknown, pos + WINDOW, "left") > np.searchsorted(unknown, pos, "left")
    beyond = inside & in_window & ~in_reach & ~has_unknown
    ok = inside & ~beyond & ~has_unknown
    labels = (in_reach & ok).astype(np.uint8)
    dropped = dict(outside_bed=int((~inside).sum()), beyond_reach=int(beyond.sum()), no_genotype=int((inside & has_unknown).sum()), negatives_subsampled=0)
    neg, lab = np.nonzero(ok & (labels == 0))[0], np.nonzero(ok & (labels == 1))[0]
    neg, dropped["negatives_subsampled"] = subsample_negatives(neg, lab.size, neg_ratio, seed)
    idx = np.sort(np.concatenate([lab, neg]))
    return idx, labels[idx], dropped


INDEL_DROP_KEYS = ("outside_bed", "beyond_reach", "no_genotype", "negatives_subsampled")


def haploid_indel_training_examples(params, truth_vcf=None, confident_bed=None, neg_ratio=2.0, seed=0, device=0):
    """Labelled sites per contig: {chrom: (x float32 [n][5][128][2] device tensor, labels uint8 [n] numpy (1 = indel), pos int64 [n] numpy, mean
    depth)}; the counts of dropped sites by reason (INDEL_DROP_KEYS) per contig are in haploid_indel_training_examples.dropped afterwards.

    params: the indel step's dict as train_indel.indel_training_examples takes it (sam_path: a BAM; no HP tags are needed, the haploid
    pipeline reads all reads as one group), plus 'chrom_list'.  The truth is truth_vcf, or with truth_vcf=None params['truth']: a synth.World
    decorated by add_indels whose reads the BAM holds, or {chrom: (pos, class, is_long)}.  The truth records go to the device pipeline in its
    haploid form as genotype_indel_sites in add mode.  Only the device pipeline runs: chunks that would take the host-assembled route raise."""
    out, haploid_indel_training_examples.dropped = indel_examples("haploid_indel_training_examples", params, truth_vcf, confident_bed, neg_ratio, seed,
                                                                  device, parse_haploid_truth_indels, label_haploid_indel_sites, True,
                                                                  lambda cls: cls != 0)            # (a 0/0 record is no site to add)
    return out


class HaploidIndelTrainer(IndelFamilyTrainer):
    """One trainer per engine context.  init: 'haploid' (the shipped CHM13 model), an .ncw path of kind KIND_INDEL_HAP, a canonical blob
    (numpy), or None = Xavier-uniform from `seed`.  slice_sites: sites per workspace slice (228 KB each); 0 = min(max_batch, 1024)."""

    PREFIX, KIND, X_SHAPE, LABEL_TEXT = "nc_hap_indel_train", KIND_INDEL_HAP, (5, 128, 2), "one label (0 or 1) per site"

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-5, keep=0.5, seed=0, max_batch=1024, slice_sites=0, beta1=0.9, beta2=0.999, eps=1e-8):
        flat = initial_blob("HaploidIndelTrainer", init, self.KIND, seed, get_indel_model)
        self._open(device, flat, lr, gamma, keep, seed, max_batch, (beta1, beta2, eps), int(slice_sites))

    def evaluate(self, x, labels):
        """keep = 1: cost, CE, 'acc' (the call at >= 0.5, indelCaller.py:175, against the label), 'recall' of class 0 and class 1 (NaN for a
        class the batch does not hold) and 'probs', the device tensor"""
        import torch
        losses, _ = self.loss_grad(x, labels, None, 1.0, want_grad=False)
        probs = self.forward(x)
        lab = torch.as_tensor(labels).to(self.device).long()
        hit = (probs >= 0.5).long() == lab
        out = dict(losses)
        out.update(acc=float(hit.float().mean().item()), recall=class_recall(hit, lab, 2), probs=probs)
        return out


def train_haploid_indel_model(params):
    """Epochs over the contigs of params['chrom_list'] with a validation split; writes <out_dir>/model-<epoch>.ncw.  params:
    haploid_indel_training_examples' keys + truth_vcf, confident_bed, out_dir, and optionally epochs (10), batch (256), lr (1e-3), gamma
    (1e-5), keep (0.5), seed, init, val_frac (0.1), neg_ratio (2).  -> list of per-epoch dicts (train cost, validation cost / CE / accuracy, path)"""
    ex = haploid_indel_training_examples(params, params.get("truth_vcf"), params.get("confident_bed"), params.get("neg_ratio", 2.0),
                                         int(params.get("seed", 0)), params.get("device", 0))
    return train_on_indel_examples("train_haploid_indel_model", HaploidIndelTrainer, ex, params)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nanocaller_amd.train_haploid", description="train or fine-tune a haploid model on the GPU")
    sub = ap.add_subparsers(dest="model", required=True)
    sp = sub.add_parser("snp", help="the haploid SNP model")
    add_train_args(sp, True, "'haploid' or an .ncw file to fine-tune (default: Xavier-uniform)")
    ip = sub.add_parser("indel", help="the haploid indel model")
    add_train_args(ip, False, "'haploid' or an .ncw file to fine-tune (default: Xavier-uniform)")
    a = ap.parse_args(argv)
    if a.model == "indel":
        train_haploid_indel_model(indel_params(a))
    else:
        train_haploid_snp_model(snp_params(a))


if __name__ == "__main__":
    main()

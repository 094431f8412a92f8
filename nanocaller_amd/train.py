"""Training and fine-tuning of the diploid SNP model on the GPU.

Replaces the reference's misc/training/model_run.py, model_architect.py and generate_SNP_pileups.py (TensorFlow 1, pysam, text pileups):
labelled sites come from the device scan + featuriser, the forward / backward pass and TensorFlow-form Adam are the HIP kernels of
csrc/nc_train.hip.  torch is plumbing only: device memory, the dropout mask's random generator, casts.

    tr = SnpTrainer(init="ONT-HG002", lr=1e-4)            # or init=None: Xavier-uniform from the seed
    x, ref_code, labels, pos = snp_training_examples(params, truth_vcf, confident_bed)[chrom]
    tr.step(x, ref_code, labels); tr.evaluate(x, ref_code, labels); tr.save("model-1.ncw", train_coverage)
    python -m nanocaller_amd.train -bam x.bam -ref x.fa -vcf truth.vcf.gz -bed confident.bed -o out_dir

The result is used as snp_model='/path/model-N.ncw'.  Opt-in, the two further halves of the reference's generator:
truth_neighbors (-truth_neighbors) adds every site a second time with the truth's heterozygous sites as its neighbours, background
(-background) samples columns under the candidate threshold as further reference-call examples.
"""
from __future__ import annotations

import gzip

import numpy as np

from . import train_common
from .train_common import SnpFamilyTrainer, add_train_args, initial_blob, run_epochs, snp_params, subsample_negatives, weighted_coverage
from .weights import KIND_SNP, get_SNP_model, write_ncw  # noqa: F401  (write_ncw: imported from here by its users)

LOSS_KEYS = ("cost", "GT", "A", "G", "T", "C")
BASE_CODE = {"A": 0, "G": 1, "T": 2, "C": 3}
# genotype -> GT class (1 = heterozygous), generate_SNP_pileups.py:179 of misc/training
GT_MAP = {(0, 0): 0, (1, 1): 0, (2, 2): 0, (1, 2): 1, (2, 1): 1, (0, 1): 1, (1, 0): 1, (0, 2): 1, (2, 0): 1}


def xavier_init(seed=0):
    """train_common.xavier_init for the diploid SNP model"""
    return train_common.xavier_init(KIND_SNP, seed)


def blob_tensors(flat):
    """train_common.blob_tensors for the diploid SNP model"""
    return train_common.blob_tensors(flat, KIND_SNP)


# ------------------------------------------------------------------ labels (pure host code)
def parse_truth_vcf(text, chrom):
    """VCF text -> {pos: (GT class, allele code, allele code)}: the first sample's GT through GT_MAP, both alleles among A, G, T, C
    (generate_SNP_pileups.py:179-185 of misc/training); everything else (indels, other genotypes, other contigs) is skipped"""
    out = {}
    for ln in text.splitlines():
        if not ln or ln[0] == "#":
            continue
        f = ln.split("\t")
        if len(f) < 10 or f[0] != chrom or not f[1].isdigit():
            continue
        fmt = f[8].split(":")
        if "GT" not in fmt:
            continue
        g = f[9].split(":")[fmt.index("GT")].replace("|", "/").split("/")
        if len(g) != 2 or not all(v.isdigit() for v in g):
            continue
        gt = (int(g[0]), int(g[1]))
        alleles = [f[3]] + f[4].split(",")
        if gt not in GT_MAP or max(gt) >= len(alleles):
            continue
        a, b = alleles[gt[0]].upper(), alleles[gt[1]].upper()
        if a in BASE_CODE and b in BASE_CODE:
            out[int(f[1])] = (GT_MAP[gt], BASE_CODE[a], BASE_CODE[b])
    return out


def parse_bed(text, chrom):
    """BED text -> sorted [(start0, end0)] half-open 0-based intervals of `chrom`"""
    iv = []
    for ln in text.splitlines():
        f = ln.split()
        if len(f) >= 3 and f[0] == chrom and f[1].isdigit() and f[2].isdigit():
            iv.append((int(f[1]), int(f[2])))
    return sorted(iv)


def in_bed(intervals, pos):
    """pos: 1-based positions -> bool mask: 0-based start <= pos - 1 < end of some interval"""
    pos = np.asarray(pos, np.int64)
    if not intervals:
        return np.zeros(pos.shape, bool)
    iv = np.asarray(intervals, np.int64)
    # overlapping intervals: the running maximum of the ends decides
    ends = np.maximum.accumulate(iv[:, 1])
    k = np.searchsorted(iv[:, 0], pos - 1, "right") - 1
    return (k >= 0) & (pos - 1 < ends[np.maximum(k, 0)])


def label_sites(pos, ref_code, truth, intervals, neg_ratio=2.0, seed=0):
    """The labelling rule.  pos (1-based), ref_code (A0 G1 T2 C3) of the featurised sites; truth = parse_truth_vcf's map; intervals =
    parse_bed's (None: everywhere).  Sites outside the intervals are dropped; a truth site is labelled by its genotype, every other site
    (0, ref, ref) (:321); the others are subsampled to neg_ratio x the truth count with a seeded generator (all kept when there is no
    truth site or neg_ratio is None).  -> (indices into pos, ascending; labels uint8 [k][5] = A, G, T, C in the site's alleles, GT class)"""
    pos = np.asarray(pos, np.int64)
    ref_code = np.asarray(ref_code, np.int64)
    keep = in_bed(intervals, pos) if intervals is not None else np.ones(pos.shape, bool)
    is_truth = np.fromiter((int(p) in truth for p in pos), bool, pos.size) & keep
    neg, _ = subsample_negatives(np.nonzero(keep & ~is_truth)[0], int(is_truth.sum()), neg_ratio, seed)
    idx = np.sort(np.concatenate([np.nonzero(is_truth)[0], neg]))
    labels = np.zeros((idx.size, 5), np.uint8)
    for j, i in enumerate(idx):
        gt, a, b = truth[int(pos[i])] if is_truth[i] else (0, int(ref_code[i]), int(ref_code[i]))
        labels[j, a] = labels[j, b] = 1
        labels[j, 4] = gt
    return idx, labels


def world_truth(world):
    """the planted truth of a synth.World -> {pos: (GT class, allele, allele)}: het sites carry ref and alt, hom sites alt twice"""
    from .synth import CODE_DEL, _ref_codes_from_string
    refc = _ref_codes_from_string(world.ref.upper())
    starts = world.read_start.astype(np.int64)
    out = {}

    def hap_base(p, h):
        # the base of haplotype h at p: the plurality among the reads of that haplotype
        cnt = np.zeros(5, np.int64)
        for r in np.nonzero((starts <= p) & (world.read_end > p) & (world.hap == h))[0]:
            cnt[world.codes[world.read_off[r] + p - starts[r]]] += 1
        cnt[CODE_DEL] = 0
        return int(np.argmax(cnt)) if cnt.sum() else int(refc[p - 1])

    for p in world.het_sites:
        a, b = hap_base(int(p), 0), hap_base(int(p), 1)
        if a < 4 and b < 4 and a != b:
            out[int(p)] = (1, a, b)
    for p in world.hom_sites:
        a = hap_base(int(p), 0)
        if a < 4:
            out[int(p)] = (0, a, a)
    return out


def _read_text(path):
    with open(path, "rb") as f:
        raw = f.read()
    return (gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw).decode()


BACKGROUND_GROUPS = 3         # the sampled columns' bins: alt_freq in [0, 5 %), [5 %, 10 %), [10 %, min_allele_freq)
_KEEP_MAX = 1.0 - 2.0 ** -20  # the largest keep probability handed to the scan (its thresholds take [0, 1))


def background_group(n, alt):
    """the bin of a sampled column from its depth and its largest alternative count: min(2, (20 * alt) // n)"""
    return np.minimum(2, (20 * np.asarray(alt, np.int64)) // np.asarray(n, np.int64))


def background_caps(background, n_truth):
    """caps of the three bins: T, T // 3, T // 3 of generate_SNP_pileups.py:260 (misc/training) with T truth sites, or the {bin: cap} given"""
    caps = [n_truth, n_truth // 3, n_truth // 3]
    if isinstance(background, dict):
        unknown = set(background) - set(range(BACKGROUND_GROUPS))
        if unknown:
            raise ValueError("background: bins are 0, 1, 2, got %s" % sorted(unknown))
        caps = [int(background.get(g, 0)) for g in range(BACKGROUND_GROUPS)]
    return caps


def _background_keep(eng, dpk, dct, start, end, caps, seed):
    """the six keep probabilities of the scan (engine.snp_scan, sample=): per bin about twice its cap expected.  The bins' populations are
    estimated by a scan that samples every bin alike and takes no candidate otherwise (about 2^16 columns come back)."""
    q = min(0.5, 65536.0 / max(1, end - start + 1))
    probe = eng.snp_scan(dpk, [(start, end)], mincov=dct["mincov"], min_allele_freq=dct["min_allele_freq"], threshold=dct["threshold"], sites_only=True,
                         sample=(seed ^ 0x5bd1e995, [q] * 6))
    under = probe.alt.astype(np.float64) / np.maximum(probe.dp, 1) < dct["min_allele_freq"]
    count = np.bincount(background_group(np.maximum(probe.dp[under], 1), probe.alt[under]), minlength=BACKGROUND_GROUPS)
    keep3 = [0.0 if caps[g] <= 0 else min(_KEEP_MAX, 2.0 * caps[g] * q / max(1, int(count[g]))) for g in range(BACKGROUND_GROUPS)]
    return keep3[:2] + [keep3[2]] * 4                                # (columns at min_allele_freq and above are candidates, never sampled)


def snp_training_examples(params, truth_vcf=None, confident_bed=None, neg_ratio=2.0, seed=0, device=0, truth_neighbors=False, background=None):
    """Labelled sites per contig: {chrom: (x int16-valued float32 [n][5][41][5] device tensor, ref_code int32 [n] device tensor,
    labels uint8 [n][5] numpy, pos int64 [n] numpy, mean depth)}.

    params: the SNP step's dict (sam_path, fasta_path, mincov, maxcov, min_allele_freq, min_nbr_sites, threshold, seq, ...), plus
    'chrom_list' = [(chrom, start, end)].  sam_path may be a synth.World or a key registered with register_alignments; with a World,
    truth_vcf=None takes its planted truth and confident_bed=None means everywhere.  Sites = the ordinary scan candidates + the truth
    positions, the latter handed over as a genotype_sites list.

    background (True, or {bin: cap} with bins 0, 1, 2): columns under the candidate threshold are sampled too, in the bins alt_freq in
    [0, 5 %), [5 %, 10 %) and [10 %, min_allele_freq) (generate_SNP_pileups.py:223-260 of misc/training): the scan keeps a column when a hash
    of its position and the seed falls under the bin's probability (engine.snp_scan, sample=), chosen for about twice the bin's cap; of
    those inside the confident regions (none is a truth position) a seeded uniform subset of at most T, T // 3, T // 3 is kept, T the
    truth sites kept, labelled (0, ref, ref) like any other non-truth site.  They are not counted against neg_ratio.  Deviation: the
    reference's np.take(pos_list, np.random.permutation(size)) keeps the first `size` positions, not a random subset.

    truth_neighbors: every kept site a second time (:273), its neighbours the truth's heterozygous single-base sites alone
    (nc_snp_scan_set_nbr_sites in only mode) instead of the columns the frequency rule picks; these examples follow the first ones with the
    same labels, so pos holds a position twice.  A site with fewer than min_nbr_sites such neighbours in reach has no second example (in only
    mode the site's own column is not counted, engine.snp_featurize).

    The mean depth is that of the first pass's sites, sampled ones included.  snp_training_examples.plan[chrom] afterwards: n_first (examples
    of the first pass), n_truth (T), and with background its sample = (seed, keep) and caps."""
    import torch

    from .engine import get_engine
    from .generate_SNP_pileups import device_pack_for, get_snp_testing_candidates
    from .synth import World
    src = params["sam_path"]
    out, plan = {}, {}
    regions = params.get("chrom_list")
    if regions is None and isinstance(src, World):
        regions = [(src.chrom, 1, src.length)]
    vcf_text = _read_text(truth_vcf) if truth_vcf is not None else None
    bed_text = _read_text(confident_bed) if confident_bed is not None else None
    for k, (chrom, start, end) in enumerate(regions):
        if vcf_text is not None:
            truth = parse_truth_vcf(vcf_text, chrom)
        elif isinstance(src, World):
            truth = world_truth(src)
        else:
            raise ValueError("snp_training_examples: a truth VCF is needed unless sam_path is a synth.World")
        intervals = parse_bed(bed_text, chrom) if bed_text is not None else None
        region = dict(chrom=chrom, start=start, end=end, ploidy="diploid")
        truth_pos = np.fromiter(truth.keys(), np.int64, len(truth))
        dct = dict(params)
        dct["genotype_sites"] = {chrom: truth_pos}
        dct["genotype_only"] = False
        dct["neighbor_sites"] = None                                 # (the first pass takes the inference rule's neighbours, whatever the environment says)
        info = {}
        if background:
            inside = truth_pos[(truth_pos >= start) & (truth_pos <= end)]
            caps = background_caps(background, int(in_bed(intervals, inside).sum()) if intervals is not None else int(inside.size))
            eng = get_engine(device)
            eng.use_torch_stream()
            sample = ((seed + k) & 0xFFFFFFFF, _background_keep(eng, device_pack_for(dct, chrom, device), dct, start, end, caps, seed + k))
            dct["background_sample"] = sample
            info.update(sample=sample)
        pos, ref1h, mat, n_all, freq, depth, _, _ = get_snp_testing_candidates(dct, region, device)
        if len(pos) == 0:
            continue
        pos, n_all = np.asarray(pos), np.asarray(n_all, np.int64)
        ref_code = np.argmax(ref1h, 1).astype(np.int32)
        # a sampled column: under the candidate threshold and no truth position (it failed the candidate test)
        sampled = (np.asarray(freq) < dct["min_allele_freq"]) & ~np.isin(pos, truth_pos) if background else np.zeros(pos.size, bool)
        own = np.nonzero(~sampled)[0]
        idx, labels = label_sites(pos[own], ref_code[own], truth, intervals, neg_ratio, seed + k)
        idx = own[idx]
        n_truth = int(np.isin(pos[idx], truth_pos).sum())
        if background:
            caps = background_caps(background, n_truth)
            bg = np.nonzero(sampled)[0]
            bi, bl = label_sites(pos[bg], ref_code[bg], {}, intervals, None)
            bg = bg[bi]
            grp = background_group(n_all[bg], np.rint(np.asarray(freq)[bg] * n_all[bg]))            # (freq = alt / n: the count back, exactly)
            rng = np.random.default_rng([seed + k, 1])
            take = np.zeros(bg.size, bool)
            for g in range(BACKGROUND_GROUPS):
                m = np.nonzero(grp == g)[0]
                take[m if m.size <= caps[g] else rng.permutation(m)[:caps[g]]] = True
            idx, labels = np.concatenate([idx, bg[take]]), np.concatenate([labels, bl[take]])
            order = np.argsort(idx, kind="stable")
            idx, labels = idx[order], labels[order]
            info.update(caps=caps)
        x_all, ref_all, pos_all = mat[idx], ref_code[idx], pos[idx]
        info.update(n_first=int(idx.size), n_truth=n_truth)
        if truth_neighbors and idx.size:
            het = np.array(sorted(p for p, t in truth.items() if t[0] == 1), np.int64)
            d2 = dict(params)
            d2.update(genotype_sites={chrom: pos_all}, genotype_only=True, neighbor_sites={chrom: het}, neighbor_only=True)
            pos2, ref2, mat2 = get_snp_testing_candidates(d2, region, device)[:3]
            if len(pos2):
                at = np.searchsorted(pos_all, pos2)                  # (pos_all ascends; every position of the second pass is one of it)
                assert np.array_equal(pos_all[at], pos2)
                x_all = np.concatenate([x_all, mat2])
                ref_all = np.concatenate([ref_all, np.argmax(ref2, 1).astype(np.int32)])
                labels = np.concatenate([labels, labels[at]])
                pos_all = np.concatenate([pos_all, np.asarray(pos2)])
        dev = torch.device("cuda", device)
        out[chrom] = (torch.from_numpy(np.ascontiguousarray(x_all, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(ref_all)).to(dev), labels,
                      pos_all, float(depth))
        plan[chrom] = info
    snp_training_examples.plan = plan
    return out


# ------------------------------------------------------------------ the trainer
class SnpTrainer(SnpFamilyTrainer):
    """One trainer per engine context.  init: a model name, an .ncw path, a canonical blob (numpy), or None = Xavier-uniform from `seed`."""

    PREFIX, KIND, LOSS_KEYS, OUT_WIDTHS = "nc_train", KIND_SNP, LOSS_KEYS, (4, 2)
    LABEL_WIDTH, LABEL_TEXT = 5, "labels are [n][5]: A, G, T, C in the site's alleles, GT class"

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-3, keep=0.5, seed=0, max_batch=4096, kind=KIND_SNP,
                 beta1=0.9, beta2=0.999, eps=1e-8):
        if kind != KIND_SNP:
            raise ValueError("SnpTrainer: only the diploid SNP model (kind %d) is trained, not kind %d" % (KIND_SNP, kind))
        flat = initial_blob("SnpTrainer", init, KIND_SNP, seed, lambda name: get_SNP_model(name)[0])
        self._open(device, flat, lr, gamma, keep, seed, max_batch, (beta1, beta2, eps))

    def evaluate(self, x, ref_code, labels, scale=None):
        """keep = 1: the losses and the six accuracies of model_run.py:164-175 (GT, the four allele heads, all five right at once);
        also 'probs' / 'gt', the device tensors they were taken from"""
        import torch
        losses, _ = self.loss_grad(x, ref_code, labels, None, 1.0, scale, want_grad=False)
        probs, gt = self.forward(x, ref_code, scale)
        lab = torch.as_tensor(labels).to(self.device)
        hit = torch.cat([(probs > 0.5) == (lab[:, :4] > 0), ((gt[:, 1] > gt[:, 0]) == (lab[:, 4] > 0)).unsqueeze(1)], 1)
        acc = hit.float().mean(0).cpu().numpy()
        out = dict(losses)
        out.update(acc_A=float(acc[0]), acc_G=float(acc[1]), acc_T=float(acc[2]), acc_C=float(acc[3]), acc_GT=float(acc[4]),
                   acc_all=float(hit.all(1).float().mean().item()), probs=probs, gt=gt)
        return out


def train_snp_model(params):
    """Epochs over the contigs of params['chrom_list'] with a validation split; writes <out_dir>/model-<epoch>.ncw.
    params: the SNP step's keys + truth_vcf, confident_bed, out_dir, and optionally epochs (10), batch (1024), lr (1e-3), gamma, keep, seed,
    init (model to fine-tune), val_frac (0.1), neg_ratio (2), truth_neighbors and background (snp_training_examples).  The file's train_coverage
    is the mean depth of the training sites, sampled background columns included.  -> list of per-epoch dicts (train cost, validation losses / accuracies, path)"""
    import torch
    seed = int(params.get("seed", 0))
    batch = int(params.get("batch", 1024))
    ex = snp_training_examples(params, params.get("truth_vcf"), params.get("confident_bed"), params.get("neg_ratio", 2.0), seed,
                               params.get("device", 0), truth_neighbors=bool(params.get("truth_neighbors")), background=params.get("background"))
    if not ex:
        raise ValueError("train_snp_model: no labelled site")
    x = torch.cat([v[0] for v in ex.values()])
    ref = torch.cat([v[1] for v in ex.values()])
    lab = torch.from_numpy(np.concatenate([v[2] for v in ex.values()])).to(x.device)
    tr = SnpTrainer(params.get("device", 0), params.get("init"), params.get("lr", 1e-3), params.get("gamma", 1e-3), params.get("keep", 0.5), seed,
                    max_batch=max(batch, 1))
    return run_epochs(tr, (x, ref), lab, params, batch, weighted_coverage([v[0].shape[0] for v in ex.values()], [v[4] for v in ex.values()]),
                      LOSS_KEYS + ("acc_A", "acc_G", "acc_T", "acc_C", "acc_GT", "acc_all"))


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nanocaller_amd.train", description="train or fine-tune the diploid SNP model on the GPU")
    add_train_args(ap, True, "model name or .ncw file to fine-tune (default: Xavier-uniform)")
    ap.add_argument("-truth_neighbors", action="store_true", help="every site a second time with the truth's heterozygous sites as its neighbours")
    ap.add_argument("-background", action="store_true", help="sample columns under the candidate threshold as further reference-call examples")
    a = ap.parse_args(argv)
    train_snp_model(dict(snp_params(a), truth_neighbors=a.truth_neighbors, background=a.background))


if __name__ == "__main__":
    main()

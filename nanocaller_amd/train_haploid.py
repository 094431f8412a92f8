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

import ctypes as C
import os

import numpy as np

from . import _lib
from .train import BASE_CODE, _read_text, in_bed, parse_bed, world_truth
from .weights import KIND_INDEL_HAP, KIND_SNP_HAP, LAYER_SPECS, Weights, get_indel_model, get_SNP_model, n_params, write_ncw

LOSS_KEYS = ("cost", "CE")
AMBIGUOUS = -1                # a truth record that does not say which single base a haploid sample has
DROP_KEYS = ("outside_bed", "ambiguous", "negatives_subsampled")


def xavier_init(kind=KIND_SNP_HAP, seed=0):
    """canonical float32 blob: Xavier-uniform kernels (limit sqrt(6 / (fan_in + fan_out)), TensorFlow's initializer), zero biases"""
    rng = np.random.default_rng(seed)
    parts = []
    for _, shp in LAYER_SPECS[kind]:
        rf = int(np.prod(shp[:-2]))
        lim = np.sqrt(6.0 / (rf * shp[-2] + rf * shp[-1]))
        parts.append(rng.uniform(-lim, lim, int(np.prod(shp))).astype(np.float32))
        parts.append(np.zeros(shp[-1], np.float32))
    return np.concatenate(parts)


def blob_tensors(flat, kind=KIND_SNP_HAP):
    """canonical blob -> [(name, array)] as weights.write_ncw takes them"""
    out, off = [], 0
    for name, shp in LAYER_SPECS[kind]:
        nk = int(np.prod(shp))
        out.append((name + ".k", np.asarray(flat[off:off + nk], np.float32).reshape(shp)))
        out.append((name + ".b", np.asarray(flat[off + nk:off + nk + shp[-1]], np.float32)))
        off += nk + shp[-1]
    return out


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
    n_truth = int(is_truth.sum())
    if neg_ratio is not None and n_truth > 0 and neg.size > int(neg_ratio * n_truth):
        kept = np.sort(np.random.default_rng(seed).permutation(neg)[:int(neg_ratio * n_truth)])
        dropped["negatives_subsampled"] = int(neg.size - kept.size)
        neg = kept
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
def _initial_blob(who, init, kind, seed, resolve):
    """init -> canonical blob: a model name / .ncw path through `resolve` (a file of another kind raises ValueError, before the device is
    touched), a blob, or None = Xavier-uniform from `seed`"""
    if isinstance(init, str):
        path = resolve(init)
        if path is None:
            raise ValueError("%s: %r is neither 'haploid' nor an .ncw file" % (who, init))
        w = Weights(path)
        if w.kind != kind:
            raise ValueError("%s: %s holds a model of kind %d, this trainer trains kind %d" % (who, path, w.kind, kind))
        return w.flat
    if init is None:
        return xavier_init(kind, seed)
    flat = np.ascontiguousarray(init, np.float32)
    if flat.size != n_params(kind):
        raise ValueError("%s: a blob of %d floats, the model has %d" % (who, flat.size, n_params(kind)))
    return flat


class HaploidSnpTrainer:
    """One trainer per engine context.  init: 'haploid' (the shipped CHM13 model), an .ncw path of kind KIND_SNP_HAP, a canonical blob
    (numpy), or None = Xavier-uniform from `seed`."""

    KIND = KIND_SNP_HAP

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-3, keep=0.5, seed=0, max_batch=4096, beta1=0.9, beta2=0.999, eps=1e-8):
        flat = _initial_blob("HaploidSnpTrainer", init, self.KIND, seed, lambda name: get_SNP_model(name)[0])
        import torch

        from .engine import get_engine
        self.eng = get_engine(device)
        self.eng.use_torch_stream()
        self.L, self.device = self.eng.L, self.eng.device
        self.lr, self.gamma, self.keep, self.max_batch = float(lr), float(gamma), float(keep), int(max_batch)
        self.adam = (float(beta1), float(beta2), float(eps))
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        h = C.c_void_p()
        self.eng._check(self.L.nc_hap_train_create(self.eng.ctx, int(self.KIND), self.max_batch, C.byref(h)), "nc_hap_train_create")
        self.h = h
        self.set_weights(flat)

    def close(self):
        if getattr(self, "h", None) and getattr(self.eng, "ctx", None):
            self.L.nc_hap_train_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc, what):
        self.eng._check(rc, what)

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        self._c(self.L.nc_hap_train_set_weights(self.h, _lib.npp(flat), flat.size), "nc_hap_train_set_weights")

    def get_weights(self):
        flat = np.zeros(n_params(self.KIND), np.float32)
        self._c(self.L.nc_hap_train_get_weights(self.h, _lib.npp(flat), flat.size), "nc_hap_train_get_weights")
        return flat

    def _inputs(self, x, ref_code, labels=None, scale=None, mask=None):
        import torch
        dev = self.device
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()          # (an int16 tensor is cast here)
        n = int(x.shape[0])
        if tuple(x.shape[1:]) != (5, 41, 5):
            raise ValueError("HaploidSnpTrainer: tensors of shape %s, the model takes [n][5][41][5]" % (tuple(x.shape),))
        if not 1 <= n <= self.max_batch:
            raise ValueError("HaploidSnpTrainer: %d sites, max_batch is %d" % (n, self.max_batch))
        ref_code = torch.as_tensor(ref_code).to(device=dev, dtype=torch.int32).contiguous()
        if ref_code.numel() != n:
            raise ValueError("HaploidSnpTrainer: one reference code per site")
        if labels is not None:
            labels = torch.as_tensor(labels).to(device=dev, dtype=torch.uint8).contiguous()
            if labels.numel() != n:
                raise ValueError("HaploidSnpTrainer: one base A0 G1 T2 C3 per site")
        if scale is not None:
            scale = torch.as_tensor(scale).to(device=dev, dtype=torch.float64).contiguous()
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8).contiguous()
            if mask.numel() != n * 48:
                raise ValueError("HaploidSnpTrainer: the dropout mask is [n][48]")
        return n, x, ref_code, labels, scale, mask

    def draw_mask(self, n):
        """uint8 [n][48], 1 = kept with probability `keep`, from the trainer's seeded device generator"""
        import torch
        return (torch.rand((n, 48), generator=self.gen, device=self.device) < self.keep).to(torch.uint8)

    def forward(self, x, ref_code, scale=None, mask=None, keep=1.0):
        """-> probs [n][4] device tensor (A, G, T, C) of the training forward"""
        import torch
        n, x, ref_code, _, scale, mask = self._inputs(x, ref_code, None, scale, mask)
        probs = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        self._c(self.L.nc_hap_train_forward(self.h, n, p(x), p(ref_code), p(scale), p(mask), float(keep), p(probs)), "nc_hap_train_forward")
        return probs

    def loss_grad(self, x, ref_code, labels, mask=None, keep=1.0, scale=None, want_grad=True):
        """-> (dict cost, CE; gradient blob device tensor or None); adam_step steps with this gradient.  A label above 3 is refused by the
        device call (the labels may be a device tensor: they are not fetched to look)."""
        import torch
        n, x, ref_code, labels, scale, mask = self._inputs(x, ref_code, labels, scale, mask)
        grad = torch.empty(n_params(self.KIND), dtype=torch.float32, device=self.device) if want_grad else None
        l2 = np.zeros(2, np.float32)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        self._c(self.L.nc_hap_train_loss_grad(self.h, n, p(x), p(ref_code), p(scale), p(mask), float(keep), p(labels), self.gamma, _lib.npp(l2), p(grad)),
                "nc_hap_train_loss_grad")
        return dict(zip(LOSS_KEYS, (float(v) for v in l2))), grad

    def adam_step(self, lr=None):
        b1, b2, eps = self.adam
        self._c(self.L.nc_hap_train_adam(self.h, self.lr if lr is None else float(lr), b1, b2, eps), "nc_hap_train_adam")

    def step(self, x, ref_code, labels, mask=None, scale=None):
        """one Adam step on the batch -> dict(cost, CE) before the step; mask: the dropout mask to use instead of a drawn one"""
        if mask is None and self.keep < 1.0:
            mask = self.draw_mask(int(x.shape[0]))
        losses, _ = self.loss_grad(x, ref_code, labels, mask, self.keep, scale, want_grad=False)
        self.adam_step()
        return losses

    def evaluate(self, x, ref_code, labels, scale=None):
        """keep = 1: cost, CE, 'acc' (argmax of the four probabilities against the label), 'recall' per base A, G, T, C (NaN for a base the
        batch does not hold) and 'probs', the device tensor"""
        import torch
        losses, _ = self.loss_grad(x, ref_code, labels, None, 1.0, scale, want_grad=False)
        probs = self.forward(x, ref_code, scale)
        lab = torch.as_tensor(labels).to(self.device).long()
        hit = probs.argmax(1) == lab
        recall = [float(hit[lab == c].float().mean().item()) if bool((lab == c).any()) else float("nan") for c in range(4)]
        out = dict(losses)
        out.update(acc=float(hit.float().mean().item()), recall=recall, probs=probs)
        return out

    def info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._c(self.L.nc_hap_train_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "nc_hap_train_info")
        return dict(slice_sites=int(a.value), workspace_bytes=int(b.value), steps=int(c.value))

    def stage_ms(self, on=True):
        """per-stage HIP-event times of the last loss_grad (ms; of its last slice) when timing was on; switches timing on / off for the next ones"""
        ms = np.zeros(7, np.float32)
        self._c(self.L.nc_hap_train_stage_ms(self.h, 1 if on else 0, _lib.npp(ms)), "nc_hap_train_stage_ms")
        return dict(zip(("forward_trunk", "heads", "fc1_grad", "conv3_grad", "conv2_grad", "conv1_grad", "params"), (float(v) for v in ms)))

    def save(self, path, train_coverage):
        write_ncw(path, self.KIND, float(train_coverage), blob_tensors(self.get_weights(), self.KIND))
        return path


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
    n_each = np.array([v[0].shape[0] for v in ex.values()], np.float64)
    coverage = float((np.array([v[4] for v in ex.values()]) * n_each).sum() / n_each.sum())    # mean depth of the training sites
    n = int(x.shape[0])
    perm = np.random.default_rng(seed).permutation(n)
    n_val = min(max(1, int(n * float(params.get("val_frac", 0.1)))), n - 1) if n > 1 else 0
    val, trn = torch.from_numpy(perm[:n_val]).to(x.device), perm[n_val:]
    tr = HaploidSnpTrainer(params.get("device", 0), params.get("init"), params.get("lr", 1e-3), params.get("gamma", 1e-3), params.get("keep", 0.5), seed,
                           max_batch=max(batch, 1))
    os.makedirs(params["out_dir"], exist_ok=True)
    rng, hist = np.random.default_rng(seed + 1), []
    for epoch in range(1, int(params.get("epochs", 10)) + 1):
        order, costs = rng.permutation(trn), []
        for o in range(0, order.size, batch):
            sel = torch.from_numpy(order[o:o + batch]).to(x.device)
            costs.append(tr.step(x[sel], ref[sel], lab[sel])["cost"])
        rec = dict(epoch=epoch, train_cost=float(np.mean(costs)))
        if n_val:
            ev = [tr.evaluate(x[val[o:o + batch]], ref[val[o:o + batch]], lab[val[o:o + batch]]) for o in range(0, n_val, batch)]
            wts = [min(batch, n_val - o) for o in range(0, n_val, batch)]
            rec.update({"val_" + k: float(np.average([e[k] for e in ev], weights=wts)) for k in ("cost", "CE", "acc")})
        rec["path"] = tr.save(os.path.join(params["out_dir"], "model-%d.ncw" % epoch), coverage)
        print("epoch %d: %s" % (epoch, ", ".join("%s %.4g" % (k, v) for k, v in rec.items() if k not in ("epoch", "path"))), flush=True)
        hist.append(rec)
    tr.close()
    return hist


# ------------------------------------------------------------------ the haploid indel model
def parse_haploid_truth_indels(text, chrom):
    """VCF text -> (pos int64 ascending, class uint8, is_long uint8) of the indel records of `chrom`, as train_indel.parse_truth_indels reads
    them (a record counts when some ALT length differs from REF's, long when the difference exceeds 10), with the two classes of a haploid
    sample: 1 when the first sample's genotype, written for one copy or two ('1', '1/1', '0|1', ...), names an ALT allele, 0 when it names
    only the reference, CLASS_UNKNOWN for anything else."""
    from .genotype_sites import LONG_INDEL
    from .train_indel import CLASS_UNKNOWN
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
        cls = CLASS_UNKNOWN
        if len(f) >= 10 and "GT" in f[8].split(":"):
            g = f[9].split(":")[f[8].split(":").index("GT")].replace("|", "/").split("/")
            if 1 <= len(g) <= 2 and all(v.isdigit() for v in g):
                cls = 1 if any(int(v) for v in g) else 0
        rows.append((int(f[1]), cls, max(d) > LONG_INDEL))
    rows.sort()
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.uint8), np.array([r[2] for r in rows], np.uint8))


def label_haploid_indel_sites(pos, truth_pos, truth_class, intervals=None, neg_ratio=2.0, seed=0):
    """The labelling rule of train_indel.label_sites with two classes.  pos: the sites' anchors (1-based); truth_pos (ascending) /
    truth_class: parse_haploid_truth_indels' records (train_indel.world_truth's serve as well); a record of class 0 (a 0/0 genotype) says that there is no indel and is no record
    here.  A site outside the intervals is dropped.  Of the records with pos <= POS < pos + 128: none -> 0; at least one within
    [pos, pos + 40] -> 1; only beyond 40 -> dropped; a record without a usable genotype anywhere in the window -> dropped.  Class-0 sites are
    then subsampled to neg_ratio x the count of class-1 sites with a seeded generator (None, or no class-1 site: all kept).
    -> (indices into pos, ascending; labels uint8; dropped: dict of counts by reason, INDEL_DROP_KEYS)"""
    from .train_indel import CLASS_UNKNOWN, LABEL_REACH, WINDOW
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
    if neg_ratio is not None and lab.size > 0 and neg.size > int(neg_ratio * lab.size):
        kept = np.sort(np.random.default_rng(seed).permutation(neg)[:int(neg_ratio * lab.size)])
        dropped["negatives_subsampled"] = int(neg.size - kept.size)
        neg = kept
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
    import torch

    from .generate_indel_pileups import indel_sites_for_chunks, plan_routes
    from .synth import World
    from .train_indel import CHUNK, _mean_depth
    from .train_indel import world_truth as indel_world_truth
    src = params["sam_path"]
    if not isinstance(src, str):
        raise ValueError("haploid_indel_training_examples: the device indel pipeline reads a BAM file; sam_path is %s" % type(src).__name__)
    vcf_text = _read_text(truth_vcf) if truth_vcf is not None else None
    bed_text = _read_text(confident_bed) if confident_bed is not None else None
    out, dropped = {}, {}
    for k, (chrom, start, end) in enumerate(params["chrom_list"]):
        if vcf_text is not None:
            truth = parse_haploid_truth_indels(vcf_text, chrom)
        elif isinstance(params.get("truth"), World):
            truth = indel_world_truth(params["truth"]) if params["truth"].chrom == chrom else None
        elif isinstance(params.get("truth"), dict):
            truth = params["truth"].get(chrom)
        else:
            raise ValueError("haploid_indel_training_examples: a truth VCF, or params['truth'] = a synth.World or {chrom: (pos, class, is_long)}")
        if truth is None:
            truth = (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        intervals = parse_bed(bed_text, chrom) if bed_text is not None else None
        listed = np.asarray(truth[1]) != 0                              # (a 0/0 record is no site to add)
        dct = dict(params, genotype_indel_sites={chrom: (np.asarray(truth[0])[listed], np.asarray(truth[2])[listed])}, genotype_indel_only=False,
                   impute_indel_phase=False)
        dct.setdefault("supplementary", False)
        dct.setdefault("exclude_bed", None)
        chunks = [dict(chrom=chrom, start=a, end=min(a + CHUNK - 1, end), sam_path=src) for a in range(start, end + 1, CHUNK)]
        if [kind for kind, _, _ in plan_routes(dct, chunks, True, device=device)] != ["device"]:
            raise ValueError("haploid_indel_training_examples: %s:%d-%d does not take the device indel pipeline" % (chrom, start, end))
        r, _, _ = indel_sites_for_chunks(dct, chunks, device, True)
        if r["n"] == 0:
            continue
        pos = r["pos"].astype(np.int64)
        idx, labels, dropped[chrom] = label_haploid_indel_sites(pos, truth[0], truth[1], intervals, neg_ratio, seed + k)
        if idx.size == 0:
            continue
        x = r["x"][torch.from_numpy(idx).to(r["x"].device)].contiguous()
        out[chrom] = (x, labels, pos[idx], _mean_depth(dct, chunks, device, start, end))
    haploid_indel_training_examples.dropped = dropped
    return out


class HaploidIndelTrainer:
    """One trainer per engine context.  init: 'haploid' (the shipped CHM13 model), an .ncw path of kind KIND_INDEL_HAP, a canonical blob
    (numpy), or None = Xavier-uniform from `seed`.  slice_sites: sites per workspace slice (228 KB each); 0 = min(max_batch, 1024)."""

    KIND = KIND_INDEL_HAP

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-5, keep=0.5, seed=0, max_batch=1024, slice_sites=0, beta1=0.9, beta2=0.999, eps=1e-8):
        flat = _initial_blob("HaploidIndelTrainer", init, self.KIND, seed, get_indel_model)
        import torch

        from .engine import get_engine
        self.eng = get_engine(device)
        self.eng.use_torch_stream()
        self.L, self.device = self.eng.L, self.eng.device
        self.lr, self.gamma, self.keep, self.max_batch = float(lr), float(gamma), float(keep), int(max_batch)
        self.adam = (float(beta1), float(beta2), float(eps))
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        h = C.c_void_p()
        self.eng._check(self.L.nc_hap_indel_train_create(self.eng.ctx, int(self.KIND), self.max_batch, int(slice_sites), C.byref(h)), "nc_hap_indel_train_create")
        self.h = h
        self.set_weights(flat)

    def close(self):
        if getattr(self, "h", None) and getattr(self.eng, "ctx", None):
            self.L.nc_hap_indel_train_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc, what):
        self.eng._check(rc, what)

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        self._c(self.L.nc_hap_indel_train_set_weights(self.h, _lib.npp(flat), flat.size), "nc_hap_indel_train_set_weights")

    def get_weights(self):
        flat = np.zeros(n_params(self.KIND), np.float32)
        self._c(self.L.nc_hap_indel_train_get_weights(self.h, _lib.npp(flat), flat.size), "nc_hap_indel_train_get_weights")
        return flat

    def _inputs(self, x, labels=None, mask=None):
        import torch
        dev = self.device
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
        n = int(x.shape[0])
        if tuple(x.shape[1:]) != (5, 128, 2):
            raise ValueError("HaploidIndelTrainer: tensors of shape %s, the haploid indel model takes [n][5][128][2]" % (tuple(x.shape),))
        if not 1 <= n <= self.max_batch:
            raise ValueError("HaploidIndelTrainer: %d sites, max_batch is %d" % (n, self.max_batch))
        if labels is not None:
            labels = torch.as_tensor(labels).to(device=dev, dtype=torch.uint8).contiguous()
            if labels.numel() != n:
                raise ValueError("HaploidIndelTrainer: one label (0 or 1) per site")
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8).contiguous()
            if mask.numel() != n * 32:
                raise ValueError("HaploidIndelTrainer: the dropout mask is [n][32]")
        return n, x, labels, mask

    def draw_mask(self, n):
        """uint8 [n][32], 1 = kept with probability `keep`, from the trainer's seeded device generator"""
        import torch
        return (torch.rand((n, 32), generator=self.gen, device=self.device) < self.keep).to(torch.uint8)

    def forward(self, x, mask=None, keep=1.0):
        """-> probs [n] device tensor of the training forward: the probability that the site holds an indel"""
        import torch
        n, x, _, mask = self._inputs(x, None, mask)
        probs = torch.empty(n, dtype=torch.float32, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        self._c(self.L.nc_hap_indel_train_forward(self.h, n, p(x), p(mask), float(keep), p(probs)), "nc_hap_indel_train_forward")
        return probs

    def loss_grad(self, x, labels, mask=None, keep=1.0, want_grad=True):
        """-> (dict cost, CE; gradient blob device tensor or None); adam_step steps with this gradient.  A label above 1 is refused by the
        device call (the labels may be a device tensor: they are not fetched to look)."""
        import torch
        n, x, labels, mask = self._inputs(x, labels, mask)
        grad = torch.empty(n_params(self.KIND), dtype=torch.float32, device=self.device) if want_grad else None
        l2 = np.zeros(2, np.float32)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        self._c(self.L.nc_hap_indel_train_loss_grad(self.h, n, p(x), p(mask), float(keep), p(labels), self.gamma, _lib.npp(l2), p(grad)),
                "nc_hap_indel_train_loss_grad")
        return dict(zip(LOSS_KEYS, (float(v) for v in l2))), grad

    def adam_step(self, lr=None):
        b1, b2, eps = self.adam
        self._c(self.L.nc_hap_indel_train_adam(self.h, self.lr if lr is None else float(lr), b1, b2, eps), "nc_hap_indel_train_adam")

    def step(self, x, labels, mask=None):
        """one Adam step on the batch -> dict(cost, CE) before the step; mask: the dropout mask to use instead of a drawn one"""
        if mask is None and self.keep < 1.0:
            mask = self.draw_mask(int(x.shape[0]))
        losses, _ = self.loss_grad(x, labels, mask, self.keep, want_grad=False)
        self.adam_step()
        return losses

    def evaluate(self, x, labels):
        """keep = 1: cost, CE, 'acc' (the call at >= 0.5, indelCaller.py:175, against the label), 'recall' of class 0 and class 1 (NaN for a
        class the batch does not hold) and 'probs', the device tensor"""
        import torch
        losses, _ = self.loss_grad(x, labels, None, 1.0, want_grad=False)
        probs = self.forward(x)
        lab = torch.as_tensor(labels).to(self.device).long()
        hit = (probs >= 0.5).long() == lab
        recall = [float(hit[lab == c].float().mean().item()) if bool((lab == c).any()) else float("nan") for c in range(2)]
        out = dict(losses)
        out.update(acc=float(hit.float().mean().item()), recall=recall, probs=probs)
        return out

    def info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._c(self.L.nc_hap_indel_train_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "nc_hap_indel_train_info")
        return dict(slice_sites=int(a.value), workspace_bytes=int(b.value), steps=int(c.value))

    def stage_ms(self, on=True):
        """per-stage HIP-event times of the last loss_grad (ms; of its last slice) when timing was on; switches timing on / off for the next ones"""
        ms = np.zeros(7, np.float32)
        self._c(self.L.nc_hap_indel_train_stage_ms(self.h, 1 if on else 0, _lib.npp(ms)), "nc_hap_indel_train_stage_ms")
        return dict(zip(("forward_trunk", "heads", "fc1_grad", "conv3_grad", "conv2_grad", "conv1_grad", "params"), (float(v) for v in ms)))

    def save(self, path, train_coverage):
        write_ncw(path, self.KIND, float(train_coverage), blob_tensors(self.get_weights(), self.KIND))
        return path


def train_haploid_indel_model(params):
    """Epochs over the contigs of params['chrom_list'] with a validation split; writes <out_dir>/model-<epoch>.ncw.  params:
    haploid_indel_training_examples' keys + truth_vcf, confident_bed, out_dir, and optionally epochs (10), batch (256), lr (1e-3), gamma
    (1e-5), keep (0.5), seed, init, val_frac (0.1), neg_ratio (2).  -> list of per-epoch dicts (train cost, validation cost / CE / accuracy, path)"""
    import torch
    seed = int(params.get("seed", 0))
    batch = int(params.get("batch", 256))
    ex = haploid_indel_training_examples(params, params.get("truth_vcf"), params.get("confident_bed"), params.get("neg_ratio", 2.0), seed,
                                         params.get("device", 0))
    if not ex:
        raise ValueError("train_haploid_indel_model: no labelled site")
    x = torch.cat([v[0] for v in ex.values()])
    lab = torch.from_numpy(np.concatenate([v[1] for v in ex.values()])).to(x.device)
    n_each = np.array([v[0].shape[0] for v in ex.values()], np.float64)
    coverage = float((np.array([v[3] for v in ex.values()]) * n_each).sum() / n_each.sum())
    n = int(x.shape[0])
    perm = np.random.default_rng(seed).permutation(n)
    n_val = min(max(1, int(n * float(params.get("val_frac", 0.1)))), n - 1) if n > 1 else 0
    val, trn = torch.from_numpy(perm[:n_val]).to(x.device), perm[n_val:]
    tr = HaploidIndelTrainer(params.get("device", 0), params.get("init"), params.get("lr", 1e-3), params.get("gamma", 1e-5), params.get("keep", 0.5), seed,
                             max_batch=max(batch, 1))
    os.makedirs(params["out_dir"], exist_ok=True)
    rng, hist = np.random.default_rng(seed + 1), []
    for epoch in range(1, int(params.get("epochs", 10)) + 1):
        order, costs = rng.permutation(trn), []
        for o in range(0, order.size, batch):
            sel = torch.from_numpy(order[o:o + batch]).to(x.device)
            costs.append(tr.step(x[sel], lab[sel])["cost"])
        rec = dict(epoch=epoch, train_cost=float(np.mean(costs)))
        if n_val:
            ev = [tr.evaluate(x[val[o:o + batch]], lab[val[o:o + batch]]) for o in range(0, n_val, batch)]
            wts = [min(batch, n_val - o) for o in range(0, n_val, batch)]
            rec.update({"val_" + k: float(np.average([e[k] for e in ev], weights=wts)) for k in ("cost", "CE", "acc")})
        rec["path"] = tr.save(os.path.join(params["out_dir"], "model-%d.ncw" % epoch), coverage)
        print("epoch %d: %s" % (epoch, ", ".join("%s %.4g" % (k, v) for k, v in rec.items() if k not in ("epoch", "path"))), flush=True)
        hist.append(rec)
    tr.close()
    return hist


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nanocaller_amd.train_haploid", description="train or fine-tune a haploid model on the GPU")
    sub = ap.add_subparsers(dest="model", required=True)
    sp = sub.add_parser("snp", help="the haploid SNP model")
    sp.add_argument("-bam", required=True)
    sp.add_argument("-ref", required=True)
    sp.add_argument("-vcf", required=True, help="truth VCF (plain or gzipped)")
    sp.add_argument("-bed", required=True, help="confident regions")
    sp.add_argument("-o", "--out_dir", required=True)
    sp.add_argument("-chrom", nargs="+", required=True, help="contigs as NAME:START-END")
    sp.add_argument("-seq", default="ont")
    sp.add_argument("-init", default=None, help="'haploid' or an .ncw file to fine-tune (default: Xavier-uniform)")
    sp.add_argument("-epochs", type=int, default=10)
    sp.add_argument("-batch", type=int, default=1024)
    sp.add_argument("-lr", type=float, default=1e-3)
    sp.add_argument("-gamma", type=float, default=1e-3)
    sp.add_argument("-keep", type=float, default=0.5)
    sp.add_argument("-seed", type=int, default=0)
    sp.add_argument("-mincov", type=int, default=4)
    sp.add_argument("-maxcov", type=int, default=160)
    sp.add_argument("-min_allele_freq", type=float, default=0.15)
    ip = sub.add_parser("indel", help="the haploid indel model")
    ip.add_argument("-bam", required=True)
    ip.add_argument("-ref", required=True)
    ip.add_argument("-vcf", required=True, help="truth VCF (plain or gzipped)")
    ip.add_argument("-bed", required=True, help="confident regions")
    ip.add_argument("-o", "--out_dir", required=True)
    ip.add_argument("-chrom", nargs="+", required=True, help="contigs as NAME:START-END")
    ip.add_argument("-seq", default="ont")
    ip.add_argument("-init", default=None, help="'haploid' or an .ncw file to fine-tune (default: Xavier-uniform)")
    ip.add_argument("-epochs", type=int, default=10)
    ip.add_argument("-batch", type=int, default=256)
    ip.add_argument("-lr", type=float, default=1e-3)
    ip.add_argument("-seed", type=int, default=0)
    a = ap.parse_args(argv)
    regions = []
    for c in a.chrom:
        name, span = c.rsplit(":", 1)
        s, e = span.split("-")
        regions.append((name, int(s), int(e)))
    if a.model == "indel":
        ins_t, del_t = (0.4, 0.6) if a.seq != "pacbio" else (0.4, 0.4)
        train_haploid_indel_model(dict(sam_path=a.bam, fasta_path=a.ref, truth_vcf=a.vcf, confident_bed=a.bed, out_dir=a.out_dir, chrom_list=regions,
                                       seq=a.seq, mincov=4, maxcov=160, win_size=40, small_win_size=4, ins_t=ins_t, del_t=del_t, supplementary=False,
                                       exclude_bed=None, init=a.init, epochs=a.epochs, batch=a.batch, lr=a.lr, seed=a.seed))
        return
    thr = {"ont": [0.4, 0.6], "ul_ont": [0.4, 0.6], "ul_ont_extreme": [0.4, 0.6], "pacbio": [0.3, 0.7]}.get(a.seq, [0.4, 0.6])
    params = dict(sam_path=a.bam, fasta_path=a.ref, truth_vcf=a.vcf, confident_bed=a.bed, out_dir=a.out_dir, chrom_list=regions, seq=a.seq,
                  mincov=a.mincov, maxcov=a.maxcov, min_allele_freq=a.min_allele_freq, min_nbr_sites=1, threshold=thr, supplementary=False,
                  exclude_bed=None, init=a.init, epochs=a.epochs, batch=a.batch, lr=a.lr, gamma=a.gamma, keep=a.keep, seed=a.seed)
    train_haploid_snp_model(params)


if __name__ == "__main__":
    main()

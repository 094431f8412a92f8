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

import ctypes as C
import os

import numpy as np

from . import _lib
from .genotype_sites import LONG_INDEL
from .train import _read_text, in_bed, parse_bed
from .weights import KIND_INDEL, KIND_INDEL_HAP, LAYER_SPECS, Weights, get_indel_model, n_params, write_ncw

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
    """canonical float32 blob: Xavier-uniform kernels (limit sqrt(6 / (fan_in + fan_out)), TensorFlow's initializer), zero biases"""
    rng = np.random.default_rng(seed)
    parts = []
    for _, shp in LAYER_SPECS[KIND_INDEL]:
        rf = int(np.prod(shp[:-2]))
        lim = np.sqrt(6.0 / (rf * shp[-2] + rf * shp[-1]))
        parts.append(rng.uniform(-lim, lim, int(np.prod(shp))).astype(np.float32))
        parts.append(np.zeros(shp[-1], np.float32))
    return np.concatenate(parts)


def blob_tensors(flat):
    """canonical blob -> [(name, array)] as weights.write_ncw takes them"""
    out, off = [], 0
    for name, shp in LAYER_SPECS[KIND_INDEL]:
        nk = int(np.prod(shp))
        out.append((name + ".k", np.asarray(flat[off:off + nk], np.float32).reshape(shp)))
        out.append((name + ".b", np.asarray(flat[off + nk:off + nk + shp[-1]], np.float32)))
        off += nk + shp[-1]
    return out


# ------------------------------------------------------------------ labels (pure host code)
def parse_truth_indels(text, chrom):
    """VCF text -> (pos int64 ascending, class uint8, is_long uint8) of the indel records of `chrom`: a record counts when some ALT length
    differs from REF's and is long when the difference exceeds 10 (genotype_sites.parse_indel_sites_vcf's test); its class is the first
    sample's GT through GT_MAP, CLASS_UNKNOWN for any other genotype.  SNP lines and other contigs are skipped."""
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
            if len(g) == 2 and all(v.isdigit() for v in g):
                cls = GT_MAP.get((int(g[0]), int(g[1])), CLASS_UNKNOWN)
        rows.append((int(f[1]), cls, max(d) > LONG_INDEL))
    rows.sort()
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.uint8), np.array([r[2] for r in rows], np.uint8))


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
    if neg_ratio is not None and lab.size > 0 and neg.size > int(neg_ratio * lab.size):
        kept = np.sort(np.random.default_rng(seed).permutation(neg)[:int(neg_ratio * lab.size)])
        dropped["negatives_subsampled"] = int(neg.size - kept.size)
        neg = kept
    idx = np.sort(np.concatenate([lab, neg]))
    return idx, labels[idx], dropped


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
    import torch

    from .generate_indel_pileups import indel_sites_for_chunks, plan_routes
    from .synth import World
    src = params["sam_path"]
    if not isinstance(src, str):
        raise ValueError("indel_training_examples: the device indel pipeline reads a BAM file; sam_path is %s (a synth.World gives the truth as "
                         "params['truth'], its reads come from a BAM written from it)" % type(src).__name__)
    vcf_text = _read_text(truth_vcf) if truth_vcf is not None else None
    bed_text = _read_text(confident_bed) if confident_bed is not None else None
    out, dropped = {}, {}
    for k, (chrom, start, end) in enumerate(params["chrom_list"]):
        if vcf_text is not None:
            truth = parse_truth_indels(vcf_text, chrom)
        elif isinstance(params.get("truth"), World):
            truth = world_truth(params["truth"]) if params["truth"].chrom == chrom else None
        elif isinstance(params.get("truth"), dict):
            truth = params["truth"].get(chrom)
        else:
            raise ValueError("indel_training_examples: a truth VCF, or params['truth'] = a synth.World or {chrom: (pos, class, is_long)}")
        if truth is None:
            truth = (np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        intervals = parse_bed(bed_text, chrom) if bed_text is not None else None
        dct = dict(params, genotype_indel_sites={chrom: (truth[0], truth[2])}, genotype_indel_only=False, impute_indel_phase=False)
        dct.setdefault("supplementary", False)
        dct.setdefault("exclude_bed", None)
        chunks = [dict(chrom=chrom, start=a, end=min(a + CHUNK - 1, end), sam_path=src) for a in range(start, end + 1, CHUNK)]
        if [kind for kind, _, _ in plan_routes(dct, chunks, False, device=device)] != ["device"]:
            raise ValueError("indel_training_examples: %s:%d-%d does not take the device indel pipeline" % (chrom, start, end))
        r, _, _ = indel_sites_for_chunks(dct, chunks, device, False)
        if r["n"] == 0:
            continue
        pos = r["pos"].astype(np.int64)
        idx, labels, dropped[chrom] = label_sites(pos, truth[0], truth[1], intervals, neg_ratio, seed + k)
        if idx.size == 0:
            continue
        x = r["x"][torch.from_numpy(idx).to(r["x"].device)].contiguous()
        out[chrom] = (x, labels, pos[idx], _mean_depth(dct, chunks, device, start, end))
    indel_training_examples.dropped = dropped
    return out


def _mean_depth(dct, chunks, device, start, end):
    """mean depth of the kept reads over [start, end] (the pack the pipeline has just used is cached)"""
    from .indel_device import indel_pack_for
    _, dp, _, _, _, _ = indel_pack_for(dct, chunks, device, by_name=True)
    n = int(dp.reads["n_reads"])
    a, b = dp.reads["rd_start"][:n].long().clamp(min=start), dp.reads["rd_end"][:n].long().clamp(max=end + 1)
    return float((b - a).clamp(min=0).sum().item()) / float(end - start + 1)


# ------------------------------------------------------------------ the trainer
class IndelTrainer:
    """One trainer per engine context.  init: a built-in indel model name, an .ncw path, a canonical blob (numpy), or None = Xavier-uniform
    from `seed`.  slice_sites: sites per workspace slice (765 KB each); 0 = min(max_batch, 1024)."""

    def __init__(self, device=0, init=None, lr=1e-3, gamma=1e-5, keep=0.5, seed=0, max_batch=1024, slice_sites=0, kind=KIND_INDEL,
                 beta1=0.9, beta2=0.999, eps=1e-8):
        if kind != KIND_INDEL:
            raise ValueError("IndelTrainer: only the diploid indel model (kind %d) is trained, not kind %d" % (KIND_INDEL, kind))
        if isinstance(init, str):
            path = get_indel_model(init)
            if path is None:
                raise ValueError("IndelTrainer: %r is neither an indel model name nor an .ncw file" % init)
            w = Weights(path)
            if w.kind != KIND_INDEL:
                raise ValueError("IndelTrainer: %s holds a model of kind %d, only the diploid indel model is trained%s"
                                 % (path, w.kind, " (the haploid indel model is not)" if w.kind == KIND_INDEL_HAP else ""))
            flat = w.flat
        elif init is None:
            flat = xavier_init(seed)
        else:
            flat = np.ascontiguousarray(init, np.float32)
            if flat.size != n_params(KIND_INDEL):
                raise ValueError("IndelTrainer: a blob of %d floats, the diploid indel model has %d" % (flat.size, n_params(KIND_INDEL)))
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
        self.eng._check(self.L.nc_indel_train_create(self.eng.ctx, int(kind), self.max_batch, int(slice_sites), C.byref(h)), "nc_indel_train_create")
        self.h = h
        self.set_weights(flat)

    def close(self):
        if getattr(self, "h", None) and getattr(self.eng, "ctx", None):
            self.L.nc_indel_train_free(self.h)
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
        self._c(self.L.nc_indel_train_set_weights(self.h, _lib.npp(flat), flat.size), "nc_indel_train_set_weights")

    def get_weights(self):
        flat = np.zeros(n_params(KIND_INDEL), np.float32)
        self._c(self.L.nc_indel_train_get_weights(self.h, _lib.npp(flat), flat.size), "nc_indel_train_get_weights")
        return flat

    def _inputs(self, x, labels=None, mask=None):
        import torch
        dev = self.device
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
        n = int(x.shape[0])
        if tuple(x.shape[1:]) != (15, 128, 2):
            raise ValueError("IndelTrainer: tensors of shape %s, the diploid indel model takes [n][15][128][2]" % (tuple(x.shape),))
        if not 1 <= n <= self.max_batch:
            raise ValueError("IndelTrainer: %d sites, max_batch is %d" % (n, self.max_batch))
        if labels is not None:
            labels = torch.as_tensor(labels).to(device=dev, dtype=torch.uint8).contiguous()
            if labels.numel() != n or int(labels.max()) >= N_CLASSES:
                raise ValueError("IndelTrainer: one class in 0..3 per site")
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8).contiguous()
            if mask.numel() != n * 32:
                raise ValueError("IndelTrainer: the dropout mask is [n][32]")
        return n, x, labels, mask

    def draw_mask(self, n):
        """uint8 [n][32], 1 = kept with probability `keep`, from the trainer's seeded device generator"""
        import torch
        return (torch.rand((n, 32), generator=self.gen, device=self.device) < self.keep).to(torch.uint8)

    def forward(self, x, mask=None, keep=1.0):
        """-> probs [n][4] device tensor of the training forward"""
        import torch
        n, x, _, mask = self._inputs(x, None, mask)
        probs = torch.empty((n, N_CLASSES), dtype=torch.float32, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        self._c(self.L.nc_indel_train_forward(self.h, n, p(x), p(mask), float(keep), p(probs)), "nc_indel_train_forward")
        return probs

    def loss_grad(self, x, labels, mask=None, keep=1.0, want_grad=True):
        """-> (dict cost, CE; gradient blob device tensor or None); adam_step steps with this gradient"""
        import torch
        n, x, labels, mask = self._inputs(x, labels, mask)
        grad = torch.empty(n_params(KIND_INDEL), dtype=torch.float32, device=self.device) if want_grad else None
        l2 = np.zeros(2, np.float32)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        self._c(self.L.nc_indel_train_loss_grad(self.h, n, p(x), p(mask), float(keep), p(labels), self.gamma, _lib.npp(l2), p(grad)),
                "nc_indel_train_loss_grad")
        return dict(zip(LOSS_KEYS, (float(v) for v in l2))), grad

    def adam_step(self, lr=None):
        b1, b2, eps = self.adam
        self._c(self.L.nc_indel_train_adam(self.h, self.lr if lr is None else float(lr), b1, b2, eps), "nc_indel_train_adam")

    def step(self, x, labels, mask=None):
        """one Adam step on the batch -> dict(cost, CE) before the step; mask: the dropout mask to use instead of a drawn one"""
        if mask is None and self.keep < 1.0:
            mask = self.draw_mask(int(x.shape[0]))
        losses, _ = self.loss_grad(x, labels, mask, self.keep, want_grad=False)
        self.adam_step()
        return losses

    def evaluate(self, x, labels):
        """keep = 1: cost, CE, the overall accuracy as model_run_indels.py:126-137 counts it (argmax of the four probabilities against the
        label), the recall per class ('recall': four floats, NaN for a class the batch does not hold) and 'probs', the device tensor"""
        import torch
        losses, _ = self.loss_grad(x, labels, None, 1.0, want_grad=False)
        probs = self.forward(x)
        lab = torch.as_tensor(labels).to(self.device).long()
        hit = probs.argmax(1) == lab
        recall = [float(hit[lab == c].float().mean().item()) if bool((lab == c).any()) else float("nan") for c in range(N_CLASSES)]
        out = dict(losses)
        out.update(acc=float(hit.float().mean().item()), recall=recall, probs=probs)
        return out

    def info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._c(self.L.nc_indel_train_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "nc_indel_train_info")
        return dict(slice_sites=int(a.value), workspace_bytes=int(b.value), steps=int(c.value))

    def stage_ms(self, on=True):
        """per-stage HIP-event times of the last loss_grad (ms; of its last slice) when timing was on; switches timing on / off for the next ones"""
        ms = np.zeros(7, np.float32)
        self._c(self.L.nc_indel_train_stage_ms(self.h, 1 if on else 0, _lib.npp(ms)), "nc_indel_train_stage_ms")
        return dict(zip(("forward_trunk", "heads", "fc1_grad", "conv3_grad", "conv2_grad", "conv1_grad", "params"), (float(v) for v in ms)))

    def save(self, path, train_coverage):
        write_ncw(path, KIND_INDEL, float(train_coverage), blob_tensors(self.get_weights()))
        return path


def train_indel_model(params):
    """Epochs over the contigs of params['chrom_list'] with a validation split; writes <out_dir>/model-<epoch>.ncw.
    params: indel_training_examples' keys + truth_vcf, confident_bed, out_dir, and optionally epochs (10), batch (256), lr (1e-3), gamma (1e-5),
    keep (0.5), seed, init (model to fine-tune), val_frac (0.1), neg_ratio (2).  -> list of per-epoch dicts (train cost, validation cost / CE /
    accuracy / recalls, path)"""
    import torch
    seed = int(params.get("seed", 0))
    batch = int(params.get("batch", 256))
    ex = indel_training_examples(params, params.get("truth_vcf"), params.get("confident_bed"), params.get("neg_ratio", 2.0), seed, params.get("device", 0))
    if not ex:
        raise ValueError("train_indel_model: no labelled site")
    x = torch.cat([v[0] for v in ex.values()])
    lab = torch.from_numpy(np.concatenate([v[1] for v in ex.values()])).to(x.device)
    n_each = np.array([v[0].shape[0] for v in ex.values()], np.float64)
    coverage = float((np.array([v[3] for v in ex.values()]) * n_each).sum() / n_each.sum())
    n = int(x.shape[0])
    perm = np.random.default_rng(seed).permutation(n)
    n_val = min(max(1, int(n * float(params.get("val_frac", 0.1)))), n - 1) if n > 1 else 0
    val, trn = torch.from_numpy(perm[:n_val]).to(x.device), perm[n_val:]
    tr = IndelTrainer(params.get("device", 0), params.get("init"), params.get("lr", 1e-3), params.get("gamma", 1e-5), params.get("keep", 0.5), seed,
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
            hits = np.array([[0.0 if np.isnan(r) else r * float((lab[val[o:o + batch]] == c).sum()) for c, r in enumerate(e["recall"])]
                             for o, e in zip(range(0, n_val, batch), ev)]).sum(0)
            cnt = np.array([float((lab[val] == c).sum()) for c in range(N_CLASSES)])
            rec["val_recall"] = [float(h / c) if c else float("nan") for h, c in zip(hits, cnt)]
        rec["path"] = tr.save(os.path.join(params["out_dir"], "model-%d.ncw" % epoch), coverage)
        print("epoch %d: %s" % (epoch, ", ".join("%s %s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in rec.items()
                                                 if k not in ("epoch", "path"))), flush=True)
        hist.append(rec)
    tr.close()
    return hist


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m nanocaller_amd.train_indel", description="train or fine-tune the diploid indel model on the GPU")
    ap.add_argument("-bam", required=True, help="haplotagged BAM (HP / PS tags)")
    ap.add_argument("-ref", required=True)
    ap.add_argument("-vcf", required=True, help="truth VCF (plain or gzipped)")
    ap.add_argument("-bed", required=True, help="confident regions")
    ap.add_argument("-o", "--out_dir", required=True)
    ap.add_argument("-chrom", nargs="+", required=True, help="contigs as NAME:START-END")
    ap.add_argument("-seq", default="ont")
    ap.add_argument("-init", default=None, help="indel model name or .ncw file to fine-tune (default: Xavier-uniform)")
    ap.add_argument("-epochs", type=int, default=10)
    ap.add_argument("-batch", type=int, default=256)
    ap.add_argument("-lr", type=float, default=1e-3)
    ap.add_argument("-seed", type=int, default=0)
    a = ap.parse_args(argv)
    regions = []
    for c in a.chrom:
        name, span = c.rsplit(":", 1)
        s, e = span.split("-")
        regions.append((name, int(s), int(e)))
    ins_t, del_t = (0.4, 0.6) if a.seq != "pacbio" else (0.4, 0.4)
    params = dict(sam_path=a.bam, fasta_path=a.ref, truth_vcf=a.vcf, confident_bed=a.bed, out_dir=a.out_dir, chrom_list=regions, seq=a.seq,
                  mincov=4, maxcov=160, win_size=40, small_win_size=4, ins_t=ins_t, del_t=del_t, supplementary=False, exclude_bed=None,
                  init=a.init, epochs=a.epochs, batch=a.batch, lr=a.lr, seed=a.seed)
    train_indel_model(params)


if __name__ == "__main__":
    main()

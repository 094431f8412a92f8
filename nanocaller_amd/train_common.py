"""What the four trainers share (train.py, train_indel.py, train_haploid.py; DESIGN.md sections 17 - 19): the blob helpers, the base trainer
over the nc_*train_* entry points with its two call shapes (the SNP family takes x, ref_code, scale; the indel family x), the epoch loop,
the seeded subsampling of the negatives and the pieces of the three command lines.  A model's own module keeps its labels, its examples,
its metrics (evaluate) and its defaults.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .weights import LAYER_SPECS, Weights, n_params, write_ncw

ENTRY_POINTS = ("create", "free", "set_weights", "get_weights", "forward", "loss_grad", "adam", "info", "stage_ms")      # of every family
STAGES = ("forward_trunk", "heads", "fc1_grad", "conv3_grad", "conv2_grad", "conv1_grad", "params")


# ------------------------------------------------------------------ blobs
def xavier_init(kind, seed=0):
    """canonical float32 blob: Xavier-uniform kernels (limit sqrt(6 / (fan_in + fan_out)), TensorFlow's initializer), zero biases"""
    rng = np.random.default_rng(seed)
    parts = []
    for _, shp in LAYER_SPECS[kind]:
        rf = int(np.prod(shp[:-2]))
        lim = np.sqrt(6.0 / (rf * shp[-2] + rf * shp[-1]))
        parts.append(rng.uniform(-lim, lim, int(np.prod(shp))).astype(np.float32))
        parts.append(np.zeros(shp[-1], np.float32))
    return np.concatenate(parts)


def blob_tensors(flat, kind):
    """canonical blob -> [(name, array)] as weights.write_ncw takes them"""
    out, off = [], 0
    for name, shp in LAYER_SPECS[kind]:
        nk = int(np.prod(shp))
        out.append((name + ".k", np.asarray(flat[off:off + nk], np.float32).reshape(shp)))
        out.append((name + ".b", np.asarray(flat[off + nk:off + nk + shp[-1]], np.float32)))
        off += nk + shp[-1]
    return out


def initial_blob(who, init, kind, seed, resolve):
    """init -> canonical blob: a model name / .ncw path through `resolve` (a file of another kind raises ValueError, before the device is
    touched), a blob, or None = Xavier-uniform from `seed`"""
    if isinstance(init, str):
        path = resolve(init)
        if path is None:
            raise ValueError("%s: %r is neither a model name nor an .ncw file" % (who, init))
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


def subsample_negatives(neg, n_pos, neg_ratio, seed):
    """neg: ascending indices of the negatives.  More than neg_ratio x n_pos of them: a seeded uniform subset of that size, ascending (all
    kept when neg_ratio is None or n_pos is 0).  -> (the kept indices, how many were dropped)"""
    if neg_ratio is None or n_pos <= 0 or neg.size <= int(neg_ratio * n_pos):
        return neg, 0
    kept = np.sort(np.random.default_rng(seed).permutation(neg)[:int(neg_ratio * n_pos)])
    return kept, int(neg.size - kept.size)


# ------------------------------------------------------------------ the trainers
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Trainer:
    """One trainer per engine context over the entry points PREFIX_create .. PREFIX_stage_ms.  A model's class sets PREFIX, KIND, X_SHAPE
    (a site's tensor), MASK_WIDTH (fc1's units), LABEL_WIDTH / LABEL_TEXT (labels per site and what they are), LOSS_KEYS, and has its own
    constructor (defaults, how `init` is resolved) and evaluate."""

    PREFIX = KIND = X_SHAPE = MASK_WIDTH = LABEL_TEXT = None
    LABEL_WIDTH = 1
    LOSS_KEYS = ("cost", "CE")

    def _open(self, device, flat, lr, gamma, keep, seed, max_batch, adam, *create_args):
        """flat: the initial blob (initial_blob has checked it); create_args: what PREFIX_create takes between max_batch and the handle"""
        import torch

        from .engine import get_engine
        self.eng = get_engine(device)
        self.eng.use_torch_stream()
        self.L, self.device = self.eng.L, self.eng.device
        self.lr, self.gamma, self.keep, self.max_batch = float(lr), float(gamma), float(keep), int(max_batch)
        self.adam = tuple(float(v) for v in adam)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        self._fns = {fn: (getattr(self.L, self.PREFIX + "_" + fn), self.PREFIX + "_" + fn) for fn in ENTRY_POINTS}
        h = C.c_void_p()
        self.eng._check(self._fns["create"][0](self.eng.ctx, int(self.KIND), self.max_batch, *create_args, C.byref(h)), self.PREFIX + "_create")
        self.h = h
        self.set_weights(flat)

    def _call(self, fn, *args):
        f, name = self._fns[fn]
        self.eng._check(f(self.h, *args), name)

    def close(self):
        if getattr(self, "h", None) and getattr(self.eng, "ctx", None):
            self._fns["free"][0](self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def get_n_params(cls):
        return n_params(cls.KIND)

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        self._call("set_weights", _lib.npp(flat), flat.size)

    def get_weights(self):
        flat = np.zeros(n_params(self.KIND), np.float32)
        self._call("get_weights", _lib.npp(flat), flat.size)
        return flat

    # the arguments of a call as contiguous device tensors of the entry points' types; a wrong shape raises ValueError here, since the
    # kernels read n sites of each
    def _sites(self, x):
        import torch
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).contiguous()          # (an int16 tensor is cast here)
        if tuple(x.shape[1:]) != self.X_SHAPE or x.dim() == 0:
            raise ValueError("%s: tensors of shape %s, the model takes [n]%s" % (type(self).__name__, tuple(x.shape), "".join("[%d]" % d for d in self.X_SHAPE)))
        n = int(x.shape[0])
        if not 1 <= n <= self.max_batch:
            raise ValueError("%s: %d sites, max_batch is %d" % (type(self).__name__, n, self.max_batch))
        return n, x

    def _labels(self, labels, n):
        import torch
        if labels is None:
            return None
        labels = torch.as_tensor(labels).to(device=self.device, dtype=torch.uint8).contiguous()
        if labels.numel() != n * self.LABEL_WIDTH:
            raise ValueError("%s: %s" % (type(self).__name__, self.LABEL_TEXT))
        return labels

    def _mask(self, mask, n):
        import torch
        if mask is None:
            return None
        mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
        if mask.numel() != n * self.MASK_WIDTH:
            raise ValueError("%s: the dropout mask is [n][%d]" % (type(self).__name__, self.MASK_WIDTH))
        return mask

    def draw_mask(self, n):
        """uint8 [n][MASK_WIDTH], 1 = kept with probability `keep`, from the trainer's seeded device generator"""
        import torch
        return (torch.rand((n, self.MASK_WIDTH), generator=self.gen, device=self.device) < self.keep).to(torch.uint8)

    def _loss_grad(self, n, site_args, labels, want_grad):
        """site_args: the call's arguments between n and the labels (the caller holds their tensors)"""
        import torch
        grad = torch.empty(n_params(self.KIND), dtype=torch.float32, device=self.device) if want_grad else None
        losses = np.zeros(len(self.LOSS_KEYS), np.float32)
        self._call("loss_grad", n, *site_args, _p(labels), self.gamma, _lib.npp(losses), _p(grad))
        return dict(zip(self.LOSS_KEYS, (float(v) for v in losses))), grad

    def adam_step(self, lr=None):
        b1, b2, eps = self.adam
        self._call("adam", self.lr if lr is None else float(lr), b1, b2, eps)

    def _step_mask(self, x, mask):
        """the dropout mask of a step: the one given, else one drawn for x's sites (none at keep = 1)"""
        return self.draw_mask(int(x.shape[0])) if mask is None and self.keep < 1.0 else mask

    def info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._call("info", C.byref(a), C.byref(b), C.byref(c))
        return dict(slice_sites=int(a.value), workspace_bytes=int(b.value), steps=int(c.value))

    def stage_ms(self, on=True):
        """per-stage HIP-event times of the last loss_grad (ms; of its last slice) when timing was on; switches timing on / off for the next ones"""
        ms = np.zeros(len(STAGES), np.float32)
        self._call("stage_ms", 1 if on else 0, _lib.npp(ms))
        return dict(zip(STAGES, (float(v) for v in ms)))

    def save(self, path, train_coverage):
        write_ncw(path, self.KIND, float(train_coverage), blob_tensors(self.get_weights(), self.KIND))
        return path


class SnpFamilyTrainer(Trainer):
    """the call shape of the two SNP models: x [n][5][41][5], ref_code [n] (A0 G1 T2 C3) and optionally the coverage scale [n]"""

    X_SHAPE, MASK_WIDTH = (5, 41, 5), 48
    OUT_WIDTHS = (4,)             # the forward's outputs: probs [n][4] (the diploid model also gt [n][2])

    def _inputs(self, x, ref_code, labels=None, scale=None, mask=None):
        import torch
        n, x = self._sites(x)
        ref_code = torch.as_tensor(ref_code).to(device=self.device, dtype=torch.int32).contiguous()
        if ref_code.numel() != n:
            raise ValueError("%s: one reference code per site" % type(self).__name__)
        if scale is not None:
            scale = torch.as_tensor(scale).to(device=self.device, dtype=torch.float64).contiguous()
        return n, x, ref_code, self._labels(labels, n), scale, self._mask(mask, n)

    def forward(self, x, ref_code, scale=None, mask=None, keep=1.0):
        """-> the device tensors of the training forward: probs [n][4]; the diploid model (probs, gt [n][2])"""
        import torch
        n, x, ref_code, _, scale, mask = self._inputs(x, ref_code, None, scale, mask)
        out = [torch.empty((n, w), dtype=torch.float32, device=self.device) for w in self.OUT_WIDTHS]
        self._call("forward", n, _p(x), _p(ref_code), _p(scale), _p(mask), float(keep), *(_p(t) for t in out))
        return out[0] if len(out) == 1 else tuple(out)

    def loss_grad(self, x, ref_code, labels, mask=None, keep=1.0, scale=None, want_grad=True):
        """-> (dict of LOSS_KEYS, gradient blob device tensor or None); adam_step steps with this gradient.  The haploid model's device call
        refuses a label above 3 (the labels may be a device tensor: they are not fetched to look)."""
        n, x, ref_code, labels, scale, mask = self._inputs(x, ref_code, labels, scale, mask)
        return self._loss_grad(n, (_p(x), _p(ref_code), _p(scale), _p(mask), float(keep)), labels, want_grad)

    def step(self, x, ref_code, labels, mask=None, scale=None):
        """one Adam step on the batch -> dict of LOSS_KEYS before the step; mask: the dropout mask to use instead of a drawn one"""
        losses, _ = self.loss_grad(x, ref_code, labels, self._step_mask(x, mask), self.keep, scale, want_grad=False)
        self.adam_step()
        return losses


class IndelFamilyTrainer(Trainer):
    """the call shape of the two indel models: x [n][rows][128][2] alone"""

    MASK_WIDTH = 32
    PROBS_TAIL = ()               # the forward's output is [n] + PROBS_TAIL

    def _inputs(self, x, labels=None, mask=None):
        n, x = self._sites(x)
        return n, x, self._labels(labels, n), self._mask(mask, n)

    def forward(self, x, mask=None, keep=1.0):
        """-> probs, the device tensor of the training forward: [n][4] class probabilities, the haploid model [n] = P(indel)"""
        import torch
        n, x, _, mask = self._inputs(x, None, mask)
        probs = torch.empty((n,) + self.PROBS_TAIL, dtype=torch.float32, device=self.device)
        self._call("forward", n, _p(x), _p(mask), float(keep), _p(probs))
        return probs

    def loss_grad(self, x, labels, mask=None, keep=1.0, want_grad=True):
        """-> (dict cost, CE; gradient blob device tensor or None); adam_step steps with this gradient.  The haploid model's device call
        refuses a label above 1 (the labels may be a device tensor: they are not fetched to look)."""
        n, x, labels, mask = self._inputs(x, labels, mask)
        return self._loss_grad(n, (_p(x), _p(mask), float(keep)), labels, want_grad)

    def step(self, x, labels, mask=None):
        """one Adam step on the batch -> dict(cost, CE) before the step; mask: the dropout mask to use instead of a drawn one"""
        losses, _ = self.loss_grad(x, labels, self._step_mask(x, mask), self.keep, want_grad=False)
        self.adam_step()
        return losses


def class_recall(hit, lab, n_classes):
    """the share of `hit` among the sites of each class (NaN for a class the batch does not hold)"""
    return [float(hit[lab == c].float().mean().item()) if bool((lab == c).any()) else float("nan") for c in range(n_classes)]


# ------------------------------------------------------------------ the epoch loop
def weighted_coverage(n_each, depths):
    """mean depth of the training sites over the contigs"""
    n_each = np.asarray(n_each, np.float64)
    return float((np.asarray(depths) * n_each).sum() / n_each.sum())


def run_epochs(tr, inputs, lab, params, batch, coverage, val_keys, val_extra=None):
    """Epochs of tr.step over a seeded train / validation split of the sites; writes <out_dir>/model-<epoch>.ncw with `coverage` and closes
    the trainer.  inputs: the device tensors tr.step takes before the labels, (x, ref_code) or (x,); lab: the labels, a device tensor.
    params: out_dir, and optionally seed (0), epochs (10), val_frac (0.1).  The split is default_rng(seed).permutation(n), the epochs' orders
    come from default_rng(seed + 1).  val_keys: the keys of tr.evaluate averaged over the validation batches as val_<key>;
    val_extra(evaluations, the batches' labels) -> further entries of the record.  -> list of per-epoch dicts (train cost, validation, path)"""
    import torch
    seed = int(params.get("seed", 0))
    dev = inputs[0].device
    n = int(inputs[0].shape[0])
    perm = np.random.default_rng(seed).permutation(n)
    n_val = min(max(1, int(n * float(params.get("val_frac", 0.1)))), n - 1) if n > 1 else 0
    val, trn = torch.from_numpy(perm[:n_val]).to(dev), perm[n_val:]
    os.makedirs(params["out_dir"], exist_ok=True)
    rng, hist = np.random.default_rng(seed + 1), []
    for epoch in range(1, int(params.get("epochs", 10)) + 1):
        order, costs = rng.permutation(trn), []
        for o in range(0, order.size, batch):
            sel = torch.from_numpy(order[o:o + batch]).to(dev)
            costs.append(tr.step(*(t[sel] for t in inputs), lab[sel])["cost"])
        rec = dict(epoch=epoch, train_cost=float(np.mean(costs)))
        if n_val:
            sels = [val[o:o + batch] for o in range(0, n_val, batch)]
            ev = [tr.evaluate(*(t[s] for t in inputs), lab[s]) for s in sels]
            rec.update({"val_" + k: float(np.average([e[k] for e in ev], weights=[int(s.numel()) for s in sels])) for k in val_keys})
            if val_extra is not None:
                rec.update(val_extra(ev, [lab[s] for s in sels]))
        rec["path"] = tr.save(os.path.join(params["out_dir"], "model-%d.ncw" % epoch), coverage)
        print("epoch %d: %s" % (epoch, ", ".join("%s %s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in rec.items()
                                                 if k not in ("epoch", "path"))), flush=True)
        hist.append(rec)
    tr.close()
    return hist


# ------------------------------------------------------------------ the command lines
def parse_regions(chroms):
    """['NAME:START-END', ...] -> [(name, start, end)]"""
    regions = []
    for c in chroms:
        name, span = c.rsplit(":", 1)
        s, e = span.split("-")
        regions.append((name, int(s), int(e)))
    return regions


def add_train_args(ap, snp, init_help, bam_help=None):
    """the arguments of a training command line; snp: the SNP models' (batch 1024, gamma, keep and the scan's thresholds), else the indel models'"""
    ap.add_argument("-bam", required=True, help=bam_help)
    ap.add_argument("-ref", required=True)
    ap.add_argument("-vcf", required=True, help="truth VCF (plain or gzipped)")
    ap.add_argument("-bed", required=True, help="confident regions")
    ap.add_argument("-o", "--out_dir", required=True)
    ap.add_argument("-chrom", nargs="+", required=True, help="contigs as NAME:START-END")
    ap.add_argument("-seq", default="ont")
    ap.add_argument("-init", default=None, help=init_help)
    ap.add_argument("-epochs", type=int, default=10)
    ap.add_argument("-batch", type=int, default=1024 if snp else 256)
    ap.add_argument("-lr", type=float, default=1e-3)
    if snp:
        ap.add_argument("-gamma", type=float, default=1e-3)
        ap.add_argument("-keep", type=float, default=0.5)
    ap.add_argument("-seed", type=int, default=0)
    if snp:
        ap.add_argument("-mincov", type=int, default=4)
        ap.add_argument("-maxcov", type=int, default=160)
        ap.add_argument("-min_allele_freq", type=float, default=0.15)


SNP_THRESHOLD = {"ont": [0.4, 0.6], "ul_ont": [0.4, 0.6], "ul_ont_extreme": [0.4, 0.6], "pacbio": [0.3, 0.7]}      # by -seq; others as ont
INDEL_THRESHOLDS = {"pacbio": (0.4, 0.4)}                                                                        # (ins_t, del_t) by -seq; others (0.4, 0.6)


def _file_params(a):
    return dict(sam_path=a.bam, fasta_path=a.ref, truth_vcf=a.vcf, confident_bed=a.bed, out_dir=a.out_dir, chrom_list=parse_regions(a.chrom), seq=a.seq,
                supplementary=False, exclude_bed=None, init=a.init, epochs=a.epochs, batch=a.batch, lr=a.lr, seed=a.seed)


def snp_params(a):
    """the parsed arguments of a SNP training command line -> the params of train_snp_model / train_haploid_snp_model"""
    return dict(_file_params(a), mincov=a.mincov, maxcov=a.maxcov, min_allele_freq=a.min_allele_freq, min_nbr_sites=1,
                threshold=SNP_THRESHOLD.get(a.seq, [0.4, 0.6]), gamma=a.gamma, keep=a.keep)


def indel_params(a):
    """the parsed arguments of an indel training command line -> the params of train_indel_model / train_haploid_indel_model"""
    ins_t, del_t = INDEL_THRESHOLDS.get(a.seq, (0.4, 0.6))
    return dict(_file_params(a), mincov=4, maxcov=160, win_size=40, small_win_size=4, ins_t=ins_t, del_t=del_t)

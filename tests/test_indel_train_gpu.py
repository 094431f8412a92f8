"""The indel trainer on the device (csrc/nc_train_indel.hip, nanocaller_amd/train_indel.py) against the float64 restatement of
tests/indel_train_ref.py.

Inputs (indel_train_ref.make_inputs): tensors that look like the pipeline's, all four classes, a seeded 0/1 mask.  Weight sets: the shipped
ONT-HG002 indel model and Xavier-uniform from seed 3.  Batch sizes 1, 3, 17, 64, 130: one site, a partial 16-site MFMA tile and one slab of the
small parameters, a slab boundary, four slabs and a quarter of 16 sites per wave in fc1's weight gradient, a quarter that is no multiple of the
tile (36, 36, 36, 22) with a partial last slab.  Every comparison is per parameter tensor, never global, and its bound is 10 x the
float32-against-float64 error of the restatement itself on the same inputs (the figures stand next to the constants in indel_train_ref.py).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import indel_train_ref as R  # noqa: E402
from nanocaller_amd import _lib, train_indel  # noqa: E402
from nanocaller_amd.weights import KIND_INDEL, KIND_INDEL_HAP, SNP_MODEL_FILES, WEIGHT_DIR, Weights  # noqa: E402

pytestmark = pytest.mark.gpu
KEEP = 0.5
SIZES = (1, 3, 17, 64, 130)
WNAMES = ["ONT-HG002", "xavier3"]


@functools.lru_cache(None)
def weights(wname):
    return R.weight_set(wname)


@functools.lru_cache(None)
def reference(wname, n):
    """-> (inputs, float64 losses, float64 gradient); computed once and shared"""
    x, lab, mask = R.make_inputs(n)
    l2, g = R.loss_grad(weights(wname), x, lab, mask, KEEP)
    return (x, lab, mask), l2, g


@functools.lru_cache(None)
def trainer(wname, max_batch=130, slice_sites=0):
    return train_indel.IndelTrainer(0, weights(wname), lr=R.TRAJ_LR, gamma=R.GAMMA, keep=KEEP, seed=0, max_batch=max_batch, slice_sites=slice_sites)


def precheck(wname, n):
    """no dead tensor, no output saturated on every site: otherwise an error there would not show"""
    (x, lab, mask), _, g = reference(wname, n)
    for name, off, size, _ in R.segments():
        assert np.linalg.norm(g[off:off + size]) > 0, name
    p = R.forward(R.split(weights(wname)), x, mask, KEEP)["probs"].numpy()
    if n >= 3:
        assert (np.minimum(p, 1 - p) > 1e-6).any(0).all(), "an output is saturated on all sites"


def compare(wname, case, l2, grad, want_l2, want_g, what):
    bound = R.grad_bound(wname, case)
    e = R.rel_errors(grad, want_g)
    le = np.abs(np.asarray(l2, np.float64) - want_l2) / np.abs(want_l2)
    worst = max(e, key=e.get)
    print("%s %s %s: largest per-tensor error %.2e (%s), losses %.2e, bound %.1e" % (what, wname, case, e[worst], worst, le.max(), bound))
    assert le.max() <= bound, dict(zip(R.LOSS_KEYS, le))
    assert e[worst] <= bound, {k: v for k, v in e.items() if v > bound}


def device_loss_grad(tr, inputs, keep=KEEP):
    x, lab, mask = inputs
    losses, grad = tr.loss_grad(x, lab, mask, keep)
    return np.array([losses[k] for k in R.LOSS_KEYS]), grad


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("wname", WNAMES)
def test_gradient(wname, n):
    precheck(wname, n)
    inputs, want_l2, want_g = reference(wname, n)
    l2, grad = device_loss_grad(trainer(wname), inputs)
    compare(wname, n, l2, grad.cpu().numpy(), want_l2, want_g, "gradient")


@pytest.mark.parametrize("wname", WNAMES)
def test_gradient_over_three_slices(wname):
    """130 sites in slices of 64: three slices, the last of two sites; the slices' gradients are accumulated"""
    inputs, want_l2, want_g = reference(wname, 130)
    tr = trainer(wname, 130, 64)
    assert tr.info()["slice_sites"] == 64 and trainer(wname).info()["slice_sites"] == 130
    assert tr.info()["workspace_bytes"] < trainer(wname).info()["workspace_bytes"]
    l2, grad = device_loss_grad(tr, inputs)
    compare(wname, 130, l2, grad.cpu().numpy(), want_l2, want_g, "gradient, three slices")


_TMP = []


def _tmp():
    import tempfile
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory())
    return _TMP[0].name


@pytest.mark.parametrize("wname", WNAMES)
def test_forward(wname):
    from nanocaller_amd.engine import get_engine
    from oracle import oracle
    n = 130
    x, _, mask = R.make_inputs(n)
    tr = trainer(wname)
    probs = tr.forward(x)
    ep = oracle.indel_forward(weights(wname), x, precision="f64")
    err = float(np.abs(probs.cpu().numpy() - ep).max())
    print("training forward against the oracle (%s): %.2e" % (wname, err))
    assert err < 1e-4
    # with a mask: the restatement, which test_indel_train_ref.py pins to the oracle without one
    pm = tr.forward(x, mask, KEEP)
    em = R.forward(R.split(weights(wname)), x, mask, KEEP)["probs"].numpy()
    err = float(np.abs(pm.cpu().numpy() - em).max())
    print("training forward with a mask against the restatement (%s): %.2e" % (wname, err))
    assert err < 1e-4 and float((pm - probs).abs().max()) > 1e-3
    assert torch.equal(tr.forward(x, mask, 1.0), probs)                 # keep = 1 means no mask
    # against the inference path in exact-fp32 mode: two float32 evaluations of the same function
    eng = get_engine(0)
    path = tr.save(os.path.join(_tmp(), "w_%s.ncw" % wname), 30.0)
    w = Weights(path)
    assert w.kind == KIND_INDEL and np.array_equal(w.flat, weights(wname))
    eng.load_weights(_lib.MODEL_INDEL, w)
    dx = torch.from_numpy(x).to(eng.device)
    with eng._snp_state(exact_fp32=True):
        p2 = eng.indel_forward(_lib.MODEL_INDEL, dx)
    err = float((probs - p2).abs().max())
    print("training forward against Engine.indel_forward, exact fp32 (%s): %.2e" % (wname, err))
    assert err <= R.grad_bound(wname, 130)


def test_determinism():
    inputs, _, _ = reference("ONT-HG002", 130)
    tr = trainer("ONT-HG002")
    _, g1 = device_loss_grad(tr, inputs)
    _, g2 = device_loss_grad(tr, inputs)
    assert torch.equal(g1, g2)
    tr2 = train_indel.IndelTrainer(0, weights("ONT-HG002"), gamma=R.GAMMA, max_batch=130)
    _, g3 = device_loss_grad(tr2, inputs)
    assert torch.equal(g1, g3)
    tr2.close()
    # a larger max_batch changes the workspace, not the sums
    tr3 = train_indel.IndelTrainer(0, weights("ONT-HG002"), gamma=R.GAMMA, max_batch=200)
    _, g4 = device_loss_grad(tr3, inputs)
    assert torch.equal(g1, g4)
    tr3.close()
    # one slice of 64 sites, asked for or by default
    in64, _, _ = reference("ONT-HG002", 64)
    _, ga = device_loss_grad(trainer("ONT-HG002", 130, 64), in64)
    _, gb = device_loss_grad(tr, in64)
    assert torch.equal(ga, gb)


def test_padding_contributes_nothing():
    """17 sites in a 64-site workspace that a 64-site batch of NaN tensors has filled with NaN (activations, gradients, slabs) give the
    bits of 17 sites in a workspace of their own"""
    inputs, _, _ = reference("xavier3", 17)
    x64, lab64, mask64 = R.make_inputs(64)
    big = train_indel.IndelTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=64)
    l_nan, g_nan = device_loss_grad(big, (np.full_like(x64, np.nan), lab64, mask64))
    assert np.isnan(l_nan).any() and bool(torch.isnan(g_nan).any())
    _, g_big = device_loss_grad(big, inputs)
    small = train_indel.IndelTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=17)
    _, g_small = device_loss_grad(small, inputs)
    assert not bool(torch.isnan(g_big).any())
    assert torch.equal(g_big, g_small)
    big.close()
    small.close()


@pytest.mark.parametrize("wname", WNAMES)
def test_trajectory(wname):
    """five Adam steps at n = 64 with fixed masks"""
    x, lab, _ = R.make_inputs(64)
    masks = [R.make_inputs(64, seed=50 + t)[2] for t in range(5)]
    want_l, want_w = R.trajectory(weights(wname), x, lab, masks, KEEP, R.TRAJ_LR)
    bound = R.traj_bound(wname)
    tr = train_indel.IndelTrainer(0, weights(wname), lr=R.TRAJ_LR, gamma=R.GAMMA, keep=KEEP, max_batch=64)
    for t, mask in enumerate(masks):
        got = tr.step(x, lab, mask=mask)
        le = np.abs(np.array([got[k] for k in R.LOSS_KEYS]) - want_l[t]) / np.abs(want_l[t])
        print("step %d: losses %.2e" % (t + 1, le.max()))
        assert le.max() <= bound, (t, dict(zip(R.LOSS_KEYS, le)))
    assert tr.info()["steps"] == 5
    w0 = np.asarray(weights(wname), np.float64)
    e = R.rel_errors(tr.get_weights().astype(np.float64) - w0, want_w - w0)
    worst = max(e, key=e.get)
    print("trajectory %s: largest per-tensor error of delta w %.2e (%s), bound %.1e" % (wname, e[worst], worst, bound))
    assert e[worst] <= bound, {k: v for k, v in e.items() if v > bound}
    tr.close()


def test_refusals():
    from nanocaller_amd.engine import get_engine
    eng = get_engine(0)
    for kind in (_lib.MODEL_SNP, _lib.MODEL_SNP_HAP, _lib.MODEL_INDEL_HAP):
        h = C.c_void_p()
        assert eng.L.nc_indel_train_create(eng.ctx, kind, 64, 0, C.byref(h)) == _lib.NC_ERR_UNSUPPORTED and not h.value
        assert b"diploid indel" in eng.L.nc_last_error(eng.ctx)
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, None, kind=KIND_INDEL_HAP)
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, "haploid")
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, os.path.join(WEIGHT_DIR, SNP_MODEL_FILES["ONT-HG002"]))
    tr = train_indel.IndelTrainer(0, weights("xavier3"), max_batch=1)
    with pytest.raises(_lib.NanoCallerHipError):                       # no gradient to step with
        tr.adam_step()
    x, lab, _ = R.make_inputs(3)
    with pytest.raises(ValueError):                                    # more sites than max_batch
        tr.loss_grad(x, lab)
    with pytest.raises(ValueError):                                    # a class outside 0..3
        tr.loss_grad(x[:1], np.array([4], np.uint8))
    tr.close()


# ------------------------------------------------------------------ end to end
WORLD = dict(seed=5, length=40_000, depth=20)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """the world as a BAM + FASTA (the device pipeline reads files), its planted truth as a VCF, and a BED"""
    import bamio
    d = tmp_path_factory.mktemp("indel_train")
    w = bamio.make_bam_world(**WORLD)
    bam, fa, vcf, bed = str(d / "w.bam"), str(d / "w.fa"), str(d / "truth.vcf"), str(d / "conf.bed")
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, np.random.default_rng(WORLD["seed"])))
    bamio.write_fasta(fa, w.chrom, w.ref)
    pos, length = w.meta["indel_sites"]
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for p, ln in zip(pos.tolist(), length.tolist()):
        base = w.ref[p - 1].upper()
        ref, alt = (base, base + "A" * ln) if ln > 0 else ((base + w.ref[p:p - ln].upper()).ljust(1 - ln, "A"), base)
        lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t0|1" % (w.chrom, p, ref, alt))
    lines.insert(5, "%s\t%d\t.\tA\tG\t.\tPASS\t.\tGT\t0/1" % (w.chrom, 77))                   # a SNP line: not a record of the rule
    open(vcf, "w").write("\n".join(lines) + "\n")
    open(bed, "w").write("%s\t0\t15000\n%s\t20000\t40000\n" % (w.chrom, w.chrom))
    params = dict(sam_path=bam, fasta_path=fa, seq="ont", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6,
                  supplementary=False, exclude_bed=None, chrom_list=[(w.chrom, 1, w.length)])
    return dict(w=w, bam=bam, fa=fa, vcf=vcf, bed=bed, params=params)


def _rule(pos, tp, tc):
    """the labelling rule, site by site -> class, or None for an ambiguous site"""
    out = []
    for p in pos:
        c = [int(k) for q, k in zip(tp, tc) if p <= q < p + 128]
        near = any(p <= q <= p + 40 for q in tp)
        out.append(0 if not c else (c[0] if len(set(c)) == 1 and near else None))
    return out


def test_end_to_end_on_a_synthetic_world(env):
    """a world of 40,000 bases (bamio.make_bam_world: add_indels with het_rate 1 / 400): the smallest multiple of 10,000 at which the labelling
    rule keeps at least 100 sites with classes 0 and 2 both present (found with the oracle's indel_scan on the CPU, neg_ratio 2:
    30,000 -> 87 sites, 40,000 -> 108, four of them class 0)"""
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.engine import get_engine
    w = env["w"]
    ex = train_indel.indel_training_examples(dict(env["params"], truth=w), neg_ratio=2.0, seed=0)
    x, lab, pos, depth = ex[w.chrom]
    dropped = train_indel.indel_training_examples.dropped[w.chrom]
    n = int(x.shape[0])
    print("end to end: %d sites, classes %s, dropped %s, depth %.1f" % (n, np.bincount(lab, minlength=4).tolist(), dropped, depth))
    assert n >= 100 and n == lab.shape[0] == pos.shape[0] and tuple(x.shape[1:]) == (15, 128, 2) and x.dtype == torch.float32
    assert (lab == 0).any() and (lab == 2).any() and set(lab.tolist()) <= {0, 2} and set(dropped) == set(train_indel.DROP_KEYS)
    assert 10 < depth < 30 and np.all(np.diff(pos) >= 0)
    tp, tc, _ = train_indel.world_truth(w)
    assert _rule(pos.tolist(), tp.tolist(), tc.tolist()) == lab.tolist()
    with pytest.raises(ValueError):                                    # the device pipeline reads files: a World is not an input of its own
        train_indel.indel_training_examples(dict(env["params"], sam_path=w, truth=w))
    tr = train_indel.IndelTrainer(0, None, lr=1e-3, seed=1, max_batch=n)
    before = tr.evaluate(x, lab)["cost"]
    for _ in range(30):
        tr.step(x, lab)
    ev = tr.evaluate(x, lab)
    print("cost %.4f -> %.4f after 30 steps, accuracy %.2f, recall %s" % (before, ev["cost"], ev["acc"], ev["recall"]))
    assert ev["cost"] < before and 0 <= ev["acc"] <= 1 and np.isnan(ev["recall"][1]) and not np.isnan(ev["recall"][2])
    path = tr.save(os.path.join(_tmp(), "model-30.ncw"), depth)
    wt = Weights(path)
    assert wt.kind == KIND_INDEL and abs(wt.train_coverage - depth) < 1e-3 and np.array_equal(wt.flat, tr.get_weights())
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_INDEL, wt)
    p2 = eng.indel_forward(_lib.MODEL_INDEL, x)
    assert float((p2 - ev["probs"]).abs().max()) < 1e-4
    # the indel caller's own path with indel_model=<the file>: the model resolved as indel_run resolves it, the pipeline, the CNN, the rules
    from nanocaller_amd.weights import get_indel_model
    eng.load_weights(_lib.MODEL_INDEL, Weights(get_indel_model(path)))
    counts = {}
    chunks = [dict(chrom=w.chrom, start=1, end=w.length, sam_path=env["bam"])]
    dct = {k: v for k, v in env["params"].items() if k != "chrom_list"}
    texts = gip.indel_chunks_vcf_text(dict(dct, impute_indel_phase=False), chunks, 0, False, _lib.MODEL_INDEL, counts)
    assert counts["probs"].shape[1] == 4 and counts["probs"].shape[0] > 50 and np.isfinite(counts["probs"]).all() and len(texts) == 1
    tr.close()


def test_train_indel_model_from_files(env):
    """the file route (truth VCF + confident BED) gives the planted-truth route's examples inside the intervals, and train_indel_model writes
    one loadable model per epoch"""
    w = env["w"]
    tp, tc, tl = train_indel.world_truth(w)
    fp, fc, fl = train_indel.parse_truth_indels(open(env["vcf"]).read(), w.chrom)
    assert np.array_equal(tp, fp) and np.array_equal(tc, fc) and np.array_equal(tl, fl)
    whole = train_indel.indel_training_examples(dict(env["params"], truth=w), neg_ratio=None)[w.chrom]
    files = train_indel.indel_training_examples(env["params"], env["vcf"], env["bed"], neg_ratio=None)[w.chrom]
    assert train_indel.indel_training_examples.dropped[w.chrom]["outside_bed"] > 0
    inside = (whole[2] <= 15000) | (whole[2] > 20000)
    assert 0 < inside.sum() < inside.size
    assert np.array_equal(files[2], whole[2][inside]) and np.array_equal(files[1], whole[1][inside])
    assert torch.equal(files[0], whole[0][torch.from_numpy(inside).to(whole[0].device)])
    out = os.path.join(_tmp(), "models")
    hist = train_indel.train_indel_model(dict(env["params"], truth_vcf=env["vcf"], confident_bed=env["bed"], out_dir=out, epochs=3, batch=32, seed=2))
    assert [os.path.basename(h["path"]) for h in hist] == ["model-1.ncw", "model-2.ncw", "model-3.ncw"] and hist[2]["train_cost"] < hist[0]["train_cost"]
    for h in hist:
        wt = Weights(h["path"])
        assert wt.kind == KIND_INDEL and 10 < wt.train_coverage < 30 and np.isfinite(wt.flat).all()
    assert 0 <= hist[2]["val_acc"] <= 1 and len(hist[2]["val_recall"]) == 4

"""The haploid SNP and indel trainers on the device (csrc/nc_train_hap.hip, csrc/nc_train_hap_indel.hip, nanocaller_amd/train_haploid.py) against
the float64 restatements of tests/hap_train_ref.py and tests/hap_indel_train_ref.py (the indel half is at the end of this file).

Inputs (hap_train_ref.make_inputs): integer tensors in -1..1, all four reference bases, all four bases among the labels, a seeded 0/1 mask; no
case is saturated (tests/test_hap_train_ref.py proves it on the CPU).  Weight sets: the shipped CHM13 model and Xavier-uniform from seed 3.
Batch sizes 1, 3, 17, 64, 300, 4160: one site, a partial 16-site MFMA tile, a tile boundary, a full slab of four tiles, several workgroups'
slabs, more than one workspace slice.  Every comparison is per parameter tensor, never global, and its bound is 10 x the
float32-against-float64 error of the restatement itself on the same inputs (the figures stand next to the constants in hap_train_ref.py).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hap_train_ref as R  # noqa: E402
from nanocaller_amd import _lib, train, train_haploid  # noqa: E402
from nanocaller_amd.weights import KIND_SNP_HAP, Weights, get_SNP_model, write_ncw  # noqa: E402

pytestmark = pytest.mark.gpu
KEEP = R.KEEP


@functools.lru_cache(None)
def weights(wname):
    return R.weights(wname)


@functools.lru_cache(None)
def reference(wname, n, scaled=False):
    """-> (inputs, scale, float64 losses, float64 gradient); computed once and shared"""
    x, ref, lab, mask = R.make_inputs(n)
    scale = np.linspace(0.5, 2.0, n) if scaled else None
    l2, g = R.loss_grad(weights(wname), x, ref, lab, mask, KEEP, scale=scale)
    return (x, ref, lab, mask), scale, l2, g


@functools.lru_cache(None)
def trainer(wname, max_batch=300):
    return train_haploid.HaploidSnpTrainer(0, weights(wname), lr=R.TRAJ_LR, gamma=R.GAMMA, keep=KEEP, seed=0, max_batch=max_batch)


def compare(wname, case, l2, grad, want_l2, want_g, what):
    bound = R.grad_bound(wname, case)
    e = R.rel_errors(grad, want_g)
    le = np.abs(np.asarray(l2, np.float64) - want_l2) / np.abs(want_l2)
    worst = max(e, key=e.get)
    print("%s %s %s: largest per-tensor error %.2e (%s), losses %.2e, bound %.1e" % (what, wname, case, e[worst], worst, le.max(), bound))
    assert le.max() <= bound, dict(zip(R.LOSS_KEYS, le))
    assert e[worst] <= bound, {k: v for k, v in e.items() if v > bound}


def device_loss_grad(tr, inputs, scale=None, keep=KEEP):
    x, ref, lab, mask = inputs
    losses, grad = tr.loss_grad(x, ref, lab, mask, keep, scale)
    return np.array([losses[k] for k in R.LOSS_KEYS]), grad


@pytest.mark.parametrize("n", R.SIZES[:-1])
@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_gradient(wname, n):
    inputs, _, want_l2, want_g = reference(wname, n)
    for name, off, size, _ in R.segments():                            # no dead tensor: an error there would not show
        assert np.linalg.norm(want_g[off:off + size]) > 0, name
    l2, grad = device_loss_grad(trainer(wname), inputs)
    compare(wname, n, l2, grad.cpu().numpy(), want_l2, want_g, "gradient")


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_gradient_with_coverage_scale(wname):
    inputs, scale, want_l2, want_g = reference(wname, 17, True)
    l2, grad = device_loss_grad(trainer(wname), inputs, scale)
    compare(wname, "17s", l2, grad.cpu().numpy(), want_l2, want_g, "gradient, scaled input")


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_gradient_over_two_slices(wname):
    """4160 sites = one workspace slice of 4096 and a second of one slab: the slices' gradients are accumulated"""
    inputs, _, want_l2, want_g = reference(wname, 4160)
    tr = train_haploid.HaploidSnpTrainer(0, weights(wname), gamma=R.GAMMA, max_batch=4160)
    assert tr.info()["slice_sites"] == 4096
    l2, grad = device_loss_grad(tr, inputs)
    compare(wname, 4160, l2, grad.cpu().numpy(), want_l2, want_g, "gradient, two slices")
    tr.close()


_TMP = []


def _tmp():
    import tempfile
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory())
    return _TMP[0].name


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_forward(wname):
    from nanocaller_amd.engine import get_engine
    n = 300
    x, ref, _, mask = R.make_inputs(n)
    scale = np.linspace(0.5, 2.0, n)
    tr = trainer(wname)
    for sc, m, keep in ((None, None, 1.0), (scale, None, 1.0), (None, mask, KEEP)):
        probs = tr.forward(x, ref, sc, m, keep).cpu().numpy()
        want = R.forward(R.split(weights(wname)), x, ref, sc, m, keep)["probs"].numpy()
        err = float(np.abs(probs - want).max())
        print("training forward against the float64 reference (%s, scale %s, mask %s): %.2e" % (wname, sc is not None, m is not None, err))
        assert err <= R.forward_bound(wname) and abs(float(probs.sum(1).max()) - 1) < 1e-6
    # against the inference path in exact-fp32 mode: two float32 evaluations of the same function
    eng = get_engine(0)
    path = os.path.join(_tmp(), "w_%s.ncw" % wname)
    write_ncw(path, KIND_SNP_HAP, 30.0, train_haploid.blob_tensors(weights(wname)))
    eng.load_weights(_lib.MODEL_SNP_HAP, Weights(path))
    dx, dref, dsc = torch.from_numpy(x).to(eng.device), torch.from_numpy(ref).to(eng.device), torch.from_numpy(scale).to(eng.device)
    with eng._snp_state(exact_fp32=True):
        p2, _ = eng.snp_forward(_lib.MODEL_SNP_HAP, dx, dref, dsc)
    err = float((tr.forward(x, ref, scale) - p2).abs().max())
    print("training forward against Engine.snp_forward, exact fp32 (%s): %.2e, bound %.1e" % (wname, err, R.forward_bound(wname)))
    assert err <= R.forward_bound(wname)


def test_determinism():
    inputs, _, _, _ = reference("haploid", 300)
    tr = trainer("haploid")
    _, g1 = device_loss_grad(tr, inputs)
    _, g2 = device_loss_grad(tr, inputs)
    assert torch.equal(g1, g2)
    tr2 = train_haploid.HaploidSnpTrainer(0, weights("haploid"), gamma=R.GAMMA, max_batch=1000)     # another max_batch: the same bits
    _, g3 = device_loss_grad(tr2, inputs)
    assert torch.equal(g1, g3)
    tr2.close()


def test_padding_contributes_nothing():
    """17 sites in a 64-site workspace that a 64-site batch of NaN tensors has filled with NaN (activations, gradients, slabs) give the
    bits of 17 sites in a workspace of their own"""
    inputs, _, _, _ = reference("xavier3", 17)
    x64, ref64, lab64, mask64 = R.make_inputs(64)
    big = train_haploid.HaploidSnpTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=64)
    l_nan, g_nan = device_loss_grad(big, (np.full_like(x64, np.nan), ref64, lab64, mask64))
    assert np.isnan(l_nan).any() and bool(torch.isnan(g_nan).any())
    _, g_big = device_loss_grad(big, inputs)
    small = train_haploid.HaploidSnpTrainer(0, weights("xavier3"), gamma=R.GAMMA, max_batch=17)
    _, g_small = device_loss_grad(small, inputs)
    assert not bool(torch.isnan(g_big).any())
    assert torch.equal(g_big, g_small)
    big.close()
    small.close()


@pytest.mark.parametrize("wname", R.WEIGHT_SETS)
def test_trajectory(wname):
    """five Adam steps at n = 64 with fixed masks"""
    x, ref, lab, _ = R.make_inputs(64)
    masks = [R.make_inputs(64, seed=50 + t)[3] for t in range(5)]
    want_l, want_w = R.trajectory(weights(wname), x, ref, lab, masks, KEEP, R.TRAJ_LR)
    tr = train_haploid.HaploidSnpTrainer(0, weights(wname), lr=R.TRAJ_LR, gamma=R.GAMMA, keep=KEEP, max_batch=64)
    bound = R.traj_bound(wname)
    for t, mask in enumerate(masks):
        got = tr.step(x, ref, lab, mask=mask)
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
    for kind in (_lib.MODEL_SNP, _lib.MODEL_INDEL, _lib.MODEL_INDEL_HAP):
        h = C.c_void_p()
        assert eng.L.nc_hap_train_create(eng.ctx, kind, 64, C.byref(h)) == _lib.NC_ERR_UNSUPPORTED and not h.value
        assert b"haploid SNP" in eng.L.nc_last_error(eng.ctx)
    # the untouched diploid trainer goes on refusing the haploid kind
    h = C.c_void_p()
    assert eng.L.nc_train_create(eng.ctx, _lib.MODEL_SNP_HAP, 64, C.byref(h)) == _lib.NC_ERR_UNSUPPORTED and not h.value
    with pytest.raises(ValueError):
        train.SnpTrainer(0, "haploid")
    x, ref, lab, _ = R.make_inputs(3)
    tr = train_haploid.HaploidSnpTrainer(0, weights("xavier3"), max_batch=2)
    with pytest.raises(_lib.NanoCallerHipError):                       # no gradient to step with
        tr.adam_step()
    p = lambda a: C.c_void_p(a.data_ptr())                             # noqa: E731
    dx, dref, dlab = (torch.from_numpy(a).to(tr.device) for a in (x, ref, lab))
    probs = torch.empty((3, 4), device=tr.device)
    assert tr.L.nc_hap_train_forward(tr.h, 3, p(dx), p(dref), None, None, 1.0, p(probs)) == _lib.NC_ERR_ARG           # n > max_batch
    assert tr.L.nc_hap_train_loss_grad(tr.h, 3, p(dx), p(dref), None, None, 1.0, p(dlab), 0.0, None, None) == _lib.NC_ERR_ARG
    assert tr.L.nc_hap_train_loss_grad(tr.h, 0, p(dx), p(dref), None, None, 1.0, p(dlab), 0.0, None, None) == _lib.NC_ERR_ARG
    assert tr.L.nc_hap_train_loss_grad(tr.h, 2, p(dx), p(dref), None, None, 1.5, p(dlab), 0.0, None, None) == _lib.NC_ERR_ARG   # keep
    with pytest.raises(ValueError):
        tr.loss_grad(x, ref, lab)
    bad = np.array([1, 4], np.uint8)                                   # a label outside A0 G1 T2 C3
    with pytest.raises(_lib.NanoCallerHipError):
        tr.loss_grad(x[:2], ref[:2], bad)
    with pytest.raises(_lib.NanoCallerHipError):                       # and it left no gradient behind
        tr.adam_step()
    losses, _ = tr.loss_grad(x[:2], ref[:2], lab[:2])                  # the trainer is usable afterwards
    assert np.isfinite(losses["cost"])
    tr.adam_step()
    assert tr.info()["steps"] == 1
    tr.close()


def _haploid_world():
    """30,000 bases with a homozygous SNP every 300 and no heterozygous one: a haploid sample read at depth 20"""
    from nanocaller_amd.synth import make_world
    return make_world(seed=7, length=30_000, depth=20, read_len_scale=0.4, het_rate=0.0, hom_rate=1 / 300.0)


PARAMS = dict(fasta_path=None, mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6], seq="ont", supplementary=False,
              exclude_bed=None, disable_coverage_normalization=False)


def test_end_to_end_on_a_synthetic_haploid_world(monkeypatch):
    from nanocaller_amd import snpCaller
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.generate_SNP_pileups import get_snp_testing_candidates
    monkeypatch.delenv("NC_HAPLOID_SNP_MODEL", raising=False)
    world = _haploid_world()
    params = dict(PARAMS, sam_path=world)
    ex = train_haploid.haploid_snp_training_examples(params, neg_ratio=2.0, seed=0)
    x, ref, lab, pos, depth = ex[world.chrom]
    dropped = train_haploid.haploid_snp_training_examples.dropped[world.chrom]
    n = int(x.shape[0])
    print("end to end: %d sites, labels %s, dropped %s, depth %.1f" % (n, np.bincount(lab, minlength=4).tolist(), dropped, depth))
    assert n >= 100 and n == lab.shape[0] == pos.shape[0] and set(lab.tolist()) == {0, 1, 2, 3} and set(dropped) == set(train_haploid.DROP_KEYS)
    truth = train_haploid.haploid_world_truth(world)
    refc = ref.cpu().numpy()
    assert all(lab[i] == (truth[int(p)] if int(p) in truth else refc[i]) for i, p in enumerate(pos))
    assert (lab != refc).sum() >= 50                                   # the planted sites are there, labelled with their ALT base
    tr = train_haploid.HaploidSnpTrainer(0, None, lr=1e-3, seed=1, max_batch=n)
    before = tr.evaluate(x, ref, lab)["cost"]
    for _ in range(30):
        tr.step(x, ref, lab)
    ev = tr.evaluate(x, ref, lab)
    print("cost %.4f -> %.4f after 30 steps, accuracy %.2f, recall %s" % (before, ev["cost"], ev["acc"], ev["recall"]))
    assert ev["cost"] < before and 0 <= ev["acc"] <= 1 and len(ev["recall"]) == 4
    path = tr.save(os.path.join(_tmp(), "hap-model-30.ncw"), depth)
    w = Weights(path)
    assert w.kind == KIND_SNP_HAP and abs(w.train_coverage - depth) < 1e-3 and np.array_equal(w.flat, tr.get_weights())
    tr.close()
    # the caller with and without the key, against nc_snp_forward on the weights each run must have used
    chunk = dict(chrom=world.chrom, start=1, end=world.length, ploidy="haploid")
    cpos, ref1h, mat, _, _, cdepth, _, _ = get_snp_testing_candidates(params, chunk)
    eng = get_engine(0)
    dx = torch.from_numpy(np.ascontiguousarray(mat)).to(eng.device).to(torch.int16)
    dref = torch.from_numpy(np.argmax(ref1h, 1).astype(np.int32)).to(eng.device)

    def expected(wts, train_cov):
        eng.load_weights(_lib.MODEL_SNP_HAP, wts)
        scale = torch.full((len(cpos),), train_cov / cdepth, dtype=torch.float64, device=eng.device)
        return eng.snp_forward_guarded(_lib.MODEL_SNP_HAP, dx, dref, scale)[0].cpu().numpy()

    want_new, want_old = expected(w, w.train_coverage), expected(Weights(get_SNP_model("haploid")[0]), 30)
    r_key = snpCaller.call_chunks(dict(params, haploid_snp_model=path), [chunk])
    r_none = snpCaller.call_chunks(params, [chunk])
    r_name = snpCaller.call_chunks(dict(params, haploid_snp_model="haploid"), [chunk])
    assert np.array_equal(r_key["pos"], cpos) and np.array_equal(r_none["pos"], cpos) and r_key["n"] == len(cpos) > 100
    d_new, d_old = float(np.abs(r_key["probs"] - want_new).max()), float(np.abs(r_none["probs"] - want_old).max())
    print("caller against nc_snp_forward: with the key %.2e, without %.2e; the two models differ by %.2e" % (d_new, d_old, float(np.abs(want_new - want_old).max())))
    assert d_new == 0.0 and d_old == 0.0 and np.array_equal(r_none["probs"], r_name["probs"])
    assert float(np.abs(want_new - want_old).max()) > 0.1              # the key changes what is called

    def vcf(r):
        return bytes(snpCaller.snp_vcf_text(world.chrom, r["pos"], r["ref"], r["probs"], r["dp"], r["freq"], haploid=True))

    # the records as they are written: byte for byte the same without the key, with 'haploid', and from the shipped weights' own forward
    assert vcf(r_none) == vcf(r_name) == vcf(dict(r_none, probs=want_old)) and len(vcf(r_none)) > 1000
    assert vcf(r_key) == vcf(dict(r_key, probs=want_new)) and vcf(r_key) != vcf(r_none)
    monkeypatch.setenv("NC_HAPLOID_SNP_MODEL", path)                   # the environment stands in for the key
    assert np.array_equal(snpCaller.call_chunks(params, [chunk])["probs"], r_key["probs"])
    with pytest.raises(FileNotFoundError):
        snpCaller.call_chunks(dict(params, haploid_snp_model=os.path.join(_tmp(), "missing.ncw")), [chunk])
    with pytest.raises(ValueError):
        snpCaller.call_chunks(dict(params, haploid_snp_model=get_SNP_model("ONT-HG002")[0]), [chunk])


def test_train_haploid_snp_model_from_files():
    """the file route (truth VCF + confident BED) gives the planted-truth route's examples inside the intervals, and train_haploid_snp_model
    writes one loadable model per epoch that carries the training sites' mean depth"""
    world = _haploid_world()
    params = dict(PARAMS, sam_path=world)
    truth = train_haploid.haploid_world_truth(world)
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for p in sorted(truth):
        r = world.ref[p - 1].upper()
        if truth[p] >= 0 and r in "AGTC":
            lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t1" % (world.chrom, p, r, "AGTC"[truth[p]]))
    vcf, bed = os.path.join(_tmp(), "hap_truth.vcf"), os.path.join(_tmp(), "hap_conf.bed")
    open(vcf, "w").write("\n".join(lines) + "\n")
    open(bed, "w").write("%s\t0\t18000\n%s\t21000\t30000\n" % (world.chrom, world.chrom))
    in_file = train_haploid.parse_haploid_truth_vcf(open(vcf).read(), world.chrom)
    assert in_file == {p: c for p, c in truth.items() if p in in_file} and len(in_file) >= len(truth) - 2
    whole = train_haploid.haploid_snp_training_examples(params, neg_ratio=None)[world.chrom]
    files = train_haploid.haploid_snp_training_examples(dict(params, chrom_list=[(world.chrom, 1, world.length)]), vcf, bed, neg_ratio=None)[world.chrom]
    assert train_haploid.haploid_snp_training_examples.dropped[world.chrom]["outside_bed"] > 0
    # (a planted site whose reference base is N has no line in the file: it is left out of the comparison)
    inside = ((whole[3] <= 18000) | (whole[3] > 21000)) & ~np.isin(whole[3], [p for p in truth if p not in in_file])
    keep = ~np.isin(files[3], [p for p in truth if p not in in_file])
    assert 0 < inside.sum() < inside.size
    assert np.array_equal(files[3][keep], whole[3][inside]) and np.array_equal(files[2][keep], whole[2][inside])
    out = os.path.join(_tmp(), "hap_models")
    hist = train_haploid.train_haploid_snp_model(dict(params, truth_vcf=vcf, confident_bed=bed, chrom_list=[(world.chrom, 1, world.length)], out_dir=out,
                                                      epochs=3, batch=64, seed=2))
    assert [os.path.basename(h["path"]) for h in hist] == ["model-1.ncw", "model-2.ncw", "model-3.ncw"] and hist[2]["train_cost"] < hist[0]["train_cost"]
    w = Weights(hist[2]["path"])
    assert w.kind == KIND_SNP_HAP and 10 < w.train_coverage < 30 and np.isfinite(w.flat).all() and 0 <= hist[2]["val_acc"] <= 1


# ------------------------------------------------------------------ the haploid indel model
# Inputs (hap_indel_train_ref.make_inputs): pipeline-like tensors [5][128][2], both labels, a seeded mask; no case saturated (proved on the CPU).
# Batch sizes 1, 3, 17, 64, 130: one site, a partial slab, a slab boundary, four slabs and a full quarter per wave of k_fc1_wgrad, a tail; 130
# also in three slices of 64.
I = R.indel
KIND_INDEL_HAP = 3


@functools.lru_cache(None)
def indel_weights(wname):
    return I.weights(wname)


@functools.lru_cache(None)
def indel_reference(wname, n):
    x, lab, mask = I.make_inputs(n)
    l2, g = I.loss_grad(indel_weights(wname), x, lab, mask, I.KEEP)
    return (x, lab, mask), l2, g


@functools.lru_cache(None)
def indel_trainer(wname, max_batch=130, slice_sites=0):
    return train_haploid.HaploidIndelTrainer(0, indel_weights(wname), lr=I.TRAJ_LR, gamma=I.GAMMA, keep=I.KEEP, seed=0, max_batch=max_batch,
                                             slice_sites=slice_sites)


def indel_compare(wname, n, l2, grad, want_l2, want_g, what):
    bound = I.grad_bound(wname, n)
    e = I.rel_errors(grad, want_g)
    le = np.abs(np.asarray(l2, np.float64) - want_l2) / np.abs(want_l2)
    worst = max(e, key=e.get)
    print("indel %s %s %s: largest per-tensor error %.2e (%s), losses %.2e, bound %.1e" % (what, wname, n, e[worst], worst, le.max(), bound))
    assert le.max() <= bound, dict(zip(I.LOSS_KEYS, le))
    assert e[worst] <= bound, {k: v for k, v in e.items() if v > bound}


def indel_loss_grad(tr, inputs, keep=I.KEEP):
    x, lab, mask = inputs
    losses, grad = tr.loss_grad(x, lab, mask, keep)
    return np.array([losses[k] for k in I.LOSS_KEYS]), grad


@pytest.mark.parametrize("n", I.SIZES)
@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_gradient(wname, n):
    inputs, want_l2, want_g = indel_reference(wname, n)
    for name, off, size, _ in I.segments():
        assert np.linalg.norm(want_g[off:off + size]) > 0, name
    l2, grad = indel_loss_grad(indel_trainer(wname), inputs)
    indel_compare(wname, n, l2, grad.cpu().numpy(), want_l2, want_g, "gradient")


@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_gradient_over_three_slices(wname):
    """130 sites in slices of 64: three slices, the last of two sites; the slices' gradients are accumulated"""
    inputs, want_l2, want_g = indel_reference(wname, 130)
    tr = indel_trainer(wname, 130, 64)
    assert tr.info()["slice_sites"] == 64
    l2, grad = indel_loss_grad(tr, inputs)
    indel_compare(wname, 130, l2, grad.cpu().numpy(), want_l2, want_g, "gradient, three slices")


@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_forward(wname):
    from nanocaller_amd.engine import get_engine
    n = 130
    x, _, mask = I.make_inputs(n)
    tr = indel_trainer(wname)
    probs = tr.forward(x)
    bound = I.forward_bound(wname)
    for m, keep in ((None, 1.0), (mask, I.KEEP)):
        got = tr.forward(x, m, keep).cpu().numpy()
        want = I.forward(I.split(indel_weights(wname)), x, m, keep)["probs"].detach().numpy()
        err = float(np.abs(got - want).max())
        print("indel training forward against the float64 reference (%s, mask %s): %.2e, bound %.1e" % (wname, m is not None, err, bound))
        assert got.shape == (n,) and err <= bound
    assert torch.equal(tr.forward(x, mask, 1.0), probs)                 # keep = 1 means no mask
    # against the inference path in exact-fp32 mode: two float32 evaluations of the same function
    eng = get_engine(0)
    path = tr.save(os.path.join(_tmp(), "wi_%s.ncw" % wname), 30.0)
    w = Weights(path)
    assert w.kind == KIND_INDEL_HAP and np.array_equal(w.flat, indel_weights(wname))
    eng.load_weights(_lib.MODEL_INDEL_HAP, w)
    with eng._snp_state(exact_fp32=True):
        p2 = eng.indel_forward(_lib.MODEL_INDEL_HAP, torch.from_numpy(x).to(eng.device)).reshape(-1)
    err = float((probs - p2).abs().max())
    print("indel training forward against Engine.indel_forward, exact fp32 (%s): %.2e" % (wname, err))
    assert err <= bound


def test_indel_determinism_and_padding():
    inputs, _, _ = indel_reference("haploid", 130)
    tr = indel_trainer("haploid")
    _, g1 = indel_loss_grad(tr, inputs)
    _, g2 = indel_loss_grad(tr, inputs)
    assert torch.equal(g1, g2)
    tr2 = train_haploid.HaploidIndelTrainer(0, indel_weights("haploid"), gamma=I.GAMMA, max_batch=500)      # another max_batch: the same bits
    _, g3 = indel_loss_grad(tr2, inputs)
    assert torch.equal(g1, g3)
    tr2.close()
    # 17 sites in a 64-site workspace that a batch of NaN tensors has filled with NaN give the bits of 17 sites in a workspace of their own
    small_in, _, _ = indel_reference("xavier3", 17)
    x64, lab64, mask64 = I.make_inputs(64)
    big = train_haploid.HaploidIndelTrainer(0, indel_weights("xavier3"), gamma=I.GAMMA, max_batch=64)
    l_nan, g_nan = indel_loss_grad(big, (np.full_like(x64, np.nan), lab64, mask64))
    assert np.isnan(l_nan).any() and bool(torch.isnan(g_nan).any())
    _, g_big = indel_loss_grad(big, small_in)
    small = train_haploid.HaploidIndelTrainer(0, indel_weights("xavier3"), gamma=I.GAMMA, max_batch=17)
    _, g_small = indel_loss_grad(small, small_in)
    assert not bool(torch.isnan(g_big).any()) and torch.equal(g_big, g_small)
    big.close()
    small.close()


@pytest.mark.parametrize("wname", I.WEIGHT_SETS)
def test_indel_trajectory(wname):
    """five Adam steps at n = 64 with fixed masks"""
    x, lab, _ = I.make_inputs(64)
    masks = [I.make_inputs(64, seed=50 + t)[2] for t in range(5)]
    want_l, want_w = I.trajectory(indel_weights(wname), x, lab, masks, I.KEEP, I.TRAJ_LR)
    tr = train_haploid.HaploidIndelTrainer(0, indel_weights(wname), lr=I.TRAJ_LR, gamma=I.GAMMA, keep=I.KEEP, max_batch=64)
    bound = I.traj_bound(wname)
    for t, mask in enumerate(masks):
        got = tr.step(x, lab, mask=mask)
        le = np.abs(np.array([got[k] for k in I.LOSS_KEYS]) - want_l[t]) / np.abs(want_l[t])
        assert le.max() <= bound, (t, dict(zip(I.LOSS_KEYS, le)))
    assert tr.info()["steps"] == 5
    w0 = np.asarray(indel_weights(wname), np.float64)
    e = I.rel_errors(tr.get_weights().astype(np.float64) - w0, want_w - w0)
    worst = max(e, key=e.get)
    print("indel trajectory %s: largest per-tensor error of delta w %.2e (%s), bound %.1e" % (wname, e[worst], worst, bound))
    assert e[worst] <= bound, {k: v for k, v in e.items() if v > bound}
    tr.close()


def test_indel_refusals():
    from nanocaller_amd import train_indel
    from nanocaller_amd.engine import get_engine
    eng = get_engine(0)
    for kind in (_lib.MODEL_SNP, _lib.MODEL_SNP_HAP, _lib.MODEL_INDEL):
        h = C.c_void_p()
        assert eng.L.nc_hap_indel_train_create(eng.ctx, kind, 64, 0, C.byref(h)) == _lib.NC_ERR_UNSUPPORTED and not h.value
        assert b"haploid indel" in eng.L.nc_last_error(eng.ctx)
    h = C.c_void_p()                                                   # the untouched diploid trainer goes on refusing the haploid kind
    assert eng.L.nc_indel_train_create(eng.ctx, _lib.MODEL_INDEL_HAP, 64, 0, C.byref(h)) == _lib.NC_ERR_UNSUPPORTED and not h.value
    with pytest.raises(ValueError):
        train_indel.IndelTrainer(0, "haploid")
    x, lab, _ = I.make_inputs(3)
    tr = train_haploid.HaploidIndelTrainer(0, indel_weights("xavier3"), max_batch=2)
    with pytest.raises(_lib.NanoCallerHipError):                       # no gradient to step with
        tr.adam_step()
    p = lambda a: C.c_void_p(a.data_ptr())                             # noqa: E731
    dx, dlab = torch.from_numpy(x).to(tr.device), torch.from_numpy(lab).to(tr.device)
    probs = torch.empty(3, device=tr.device)
    assert tr.L.nc_hap_indel_train_forward(tr.h, 3, p(dx), None, 1.0, p(probs)) == _lib.NC_ERR_ARG                    # n > max_batch
    assert tr.L.nc_hap_indel_train_loss_grad(tr.h, 3, p(dx), None, 1.0, p(dlab), 0.0, None, None) == _lib.NC_ERR_ARG
    assert tr.L.nc_hap_indel_train_loss_grad(tr.h, 2, p(dx), None, 0.0, p(dlab), 0.0, None, None) == _lib.NC_ERR_ARG  # keep
    with pytest.raises(ValueError):
        tr.loss_grad(x, lab)
    with pytest.raises(_lib.NanoCallerHipError):                       # a label outside 0, 1
        tr.loss_grad(x[:2], np.array([1, 2], np.uint8))
    with pytest.raises(_lib.NanoCallerHipError):                       # and it left no gradient behind
        tr.adam_step()
    losses, _ = tr.loss_grad(x[:2], lab[:2])
    assert np.isfinite(losses["cost"])
    tr.adam_step()
    assert tr.info()["steps"] == 1
    tr.close()


WORLD = dict(seed=5, length=40_000, depth=20)


@pytest.fixture(scope="module")
def indel_env(tmp_path_factory):
    """a world with planted indels as a BAM + FASTA (the device pipeline reads files), its planted truth as a VCF with haploid genotypes, a BED"""
    import bamio
    d = tmp_path_factory.mktemp("hap_indel_train")
    w = bamio.make_bam_world(**WORLD)
    bam, fa, vcf, bed = str(d / "w.bam"), str(d / "w.fa"), str(d / "truth.vcf"), str(d / "conf.bed")
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, np.random.default_rng(WORLD["seed"])))
    bamio.write_fasta(fa, w.chrom, w.ref)
    pos, length = w.meta["indel_sites"]
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for q, ln in zip(pos.tolist(), length.tolist()):
        base = w.ref[q - 1].upper()
        ref, alt = (base, base + "A" * ln) if ln > 0 else ((base + w.ref[q:q - ln].upper()).ljust(1 - ln, "A"), base)
        lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t1" % (w.chrom, q, ref, alt))
    open(vcf, "w").write("\n".join(lines) + "\n")
    open(bed, "w").write("%s\t0\t15000\n%s\t20000\t40000\n" % (w.chrom, w.chrom))
    # ins_t / del_t are lowered from the caller's 0.4 / 0.6: at those the haploid scan of this world finds planted sites only (44 candidates,
    # none of class 0); at 0.1 / 0.15 sequencing noise adds candidates of class 0 and 26 sites whose only record lies beyond column 40
    # (counted on the CPU with oracle.indel_scan(haploid=True): 241 candidates, 91 of class 0, 124 of class 1)
    params = dict(sam_path=bam, fasta_path=fa, seq="ont", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.1, del_t=0.15,
                  supplementary=False, exclude_bed=None, chrom_list=[(w.chrom, 1, w.length)])
    return dict(w=w, bam=bam, vcf=vcf, bed=bed, params=params)


def test_indel_end_to_end_on_a_synthetic_world(indel_env, monkeypatch):
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd import train_indel
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.weights import get_haploid_indel_model, get_indel_model
    monkeypatch.delenv("NC_HAPLOID_INDEL_MODEL", raising=False)
    w = indel_env["w"]
    ex = train_haploid.haploid_indel_training_examples(dict(indel_env["params"], truth=w), neg_ratio=2.0, seed=0)
    x, lab, pos, depth = ex[w.chrom]
    dropped = train_haploid.haploid_indel_training_examples.dropped[w.chrom]
    n = int(x.shape[0])
    print("indel end to end: %d sites, labels %s, dropped %s, depth %.1f" % (n, np.bincount(lab, minlength=2).tolist(), dropped, depth))
    assert n >= 50 and n == lab.shape[0] == pos.shape[0] and tuple(x.shape[1:]) == (5, 128, 2) and x.dtype == torch.float32
    assert (lab == 0).sum() >= 20 and (lab == 1).sum() >= 20 and dropped["beyond_reach"] > 0 and set(dropped) == set(train_haploid.INDEL_DROP_KEYS) and np.all(np.diff(pos) >= 0)
    tp = train_indel.world_truth(w)[0]
    want = [1 if any(q <= t <= q + 40 for t in tp) else 0 for q in pos.tolist()]                 # the rule, site by site
    assert lab.tolist() == want and not any(all(not (q <= t <= q + 40) for t in tp) and any(q <= t < q + 128 for t in tp) for q in pos.tolist())
    # the file route gives the planted-truth route's examples inside the intervals
    files = train_haploid.haploid_indel_training_examples(indel_env["params"], indel_env["vcf"], indel_env["bed"], neg_ratio=None)[w.chrom]
    whole = train_haploid.haploid_indel_training_examples(dict(indel_env["params"], truth=w), neg_ratio=None)[w.chrom]
    inside = (whole[2] <= 15000) | (whole[2] > 20000)
    assert 0 < inside.sum() < inside.size and np.array_equal(files[2], whole[2][inside]) and np.array_equal(files[1], whole[1][inside])
    tr = train_haploid.HaploidIndelTrainer(0, None, lr=1e-3, seed=1, max_batch=n)
    before = tr.evaluate(x, lab)["cost"]
    for _ in range(30):
        tr.step(x, lab)
    ev = tr.evaluate(x, lab)
    print("indel cost %.4f -> %.4f after 30 steps, accuracy %.2f, recall %s" % (before, ev["cost"], ev["acc"], ev["recall"]))
    assert ev["cost"] < before and 0 <= ev["acc"] <= 1 and len(ev["recall"]) == 2
    path = tr.save(os.path.join(_tmp(), "hap-indel-model-30.ncw"), depth)
    wt = Weights(path)
    assert wt.kind == KIND_INDEL_HAP and np.array_equal(wt.flat, tr.get_weights())
    tr.close()
    # the indel caller's path on the haploid contig: the model resolved as indel_run resolves it, the pipeline, the CNN, the native rules
    eng = get_engine(0)
    chunks = [dict(chrom=w.chrom, start=1, end=w.length, sam_path=indel_env["bam"])]
    dct = dict({k: v for k, v in indel_env["params"].items() if k != "chrom_list"}, impute_indel_phase=False)
    r, _, _ = gip.indel_sites_for_chunks(dct, chunks, 0, True)

    def call(params):
        wts = Weights(get_haploid_indel_model(params))
        eng.load_weights(_lib.MODEL_INDEL_HAP, wts)
        counts = {}
        texts = gip.indel_chunks_vcf_text(dict(dct, **params), chunks, 0, True, _lib.MODEL_INDEL_HAP, counts)
        want = eng.indel_forward(_lib.MODEL_INDEL_HAP, r["x"]).cpu().numpy()
        return texts, counts["probs"], want

    t_key, p_key, want_key = call(dict(haploid_indel_model=path))
    t_none, p_none, want_none = call({})
    t_name, p_name, _ = call(dict(haploid_indel_model="haploid"))
    assert get_haploid_indel_model({}) == get_indel_model("haploid")                            # what the caller had hard-wired
    print("indel caller: %d sites, %d / %d bytes of records with the key / without" % (p_key.shape[0], len(t_key[0]), len(t_none[0])))
    assert p_key.shape[0] == r["n"] > 50 and np.array_equal(p_key.reshape(-1), want_key.reshape(-1)) and np.array_equal(p_none.reshape(-1), want_none.reshape(-1))
    assert t_none == t_name and np.array_equal(p_none, p_name) and float(np.abs(p_key - p_none).max()) > 0.1
    with pytest.raises(FileNotFoundError):
        get_haploid_indel_model(dict(haploid_indel_model=os.path.join(_tmp(), "missing.ncw")))
    hist = train_haploid.train_haploid_indel_model(dict(indel_env["params"], truth_vcf=indel_env["vcf"], confident_bed=indel_env["bed"],
                                                        out_dir=os.path.join(_tmp(), "hap_indel_models"), epochs=2, batch=32, seed=2))
    assert [os.path.basename(h["path"]) for h in hist] == ["model-1.ncw", "model-2.ncw"] and Weights(hist[1]["path"]).kind == KIND_INDEL_HAP

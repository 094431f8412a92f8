#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own code in the build container.

Container-only (needs /root/reference; never runs on the GPU box).  The reference featurisers are
imported with the stub modules of oracle/tools/refstub and driven on seeded
synthetic worlds; what is committed is DATA: the world arrays (inputs) and the reference's outputs.

  world_<w>.npz            inputs (reference string, read-major codes, flags)
  snp_<case>.npz           8-tuple of get_snp_testing_candidates (generate_SNP_pileups.py:279)
  cnd_pos.npz              get_cnd_pos on random sorted arrays, all five modes
  caller_vcf.npz           VCF lines written by snpCaller.caller (snpCaller.py:113-198) on canned
                           probabilities (TensorFlow stubbed; the models are replaced by canned outputs)
  indel_msa.npz            msa() tensors (generate_indel_pileups.py:12-73) on canned MUSCLE output
  indel_scan*.npz          `variants` of pass 1 (:197-276, haploid :185-241) captured from the reference's frame
  indel_impute.npz         `variants` + `extra_variants` of pass 1 with impute_indel_phase (:278-304)
  allele_prediction_ties.json   allele_prediction (:77-127) on the tie-heavy pairs of tests/align_cases.py (`allele_ties` writes it alone)
"""
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [os.path.join(HERE, "refstub"), "/root/reference", REPO]

import types  # noqa: E402

# `nanocaller_src` must be the REFERENCE's package here.  This repository has a regular package of the same name (the drop-in
# alias of nanocaller_amd), which would shadow the reference's namespace package whatever the path order: pin the name to the
# reference directory before anything imports it.
_ref_pkg = types.ModuleType("nanocaller_src")
_ref_pkg.__path__ = ["/root/reference/nanocaller_src"]
sys.modules["nanocaller_src"] = _ref_pkg

import numpy as np  # noqa: E402
import pysam  # noqa: E402  (stub)

from nanocaller_amd.synth import make_world  # noqa: E402
from nanocaller_src import generate_SNP_pileups as ref_snp  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")


def save_world(name, w):
    np.savez_compressed(os.path.join(OUT, "world_%s.npz" % name), chrom=np.array(w.chrom),
                        ref=np.frombuffer(w.ref.encode(), dtype=np.uint8), read_start=w.read_start,
                        read_end=w.read_end, read_flag=w.read_flag, read_off=w.read_off, codes=w.codes)


def run_snp(case, world_name, w, seq, ploidy, start, end, threshold=(0.4, 0.6), mincov=4, maxcov=160,
            min_allele_freq=0.15, min_nbr_sites=1, supplementary=False, exclude=None, extra=None):
    pysam.register("bam", w)
    pysam.register("fa", w)
    if exclude:
        pysam.register("bed", exclude)
    dct = dict(exclude_bed="bed" if exclude else None, sam_path="bam", fasta_path="fa",
               threshold=list(threshold), supplementary=supplementary, mincov=mincov, maxcov=maxcov,
               min_allele_freq=min_allele_freq, min_nbr_sites=min_nbr_sites, seq=seq)
    reg = dict(chrom=w.chrom, start=start, end=end, ploidy=ploidy)
    pos, ref, mat, dp, freq, depth, fwd, rev = ref_snp.get_snp_testing_candidates(dct, reg)
    n = len(pos)
    print("%-22s world=%s seq=%s %s [%d,%d] -> %d sites depth=%s" % (case, world_name, seq, ploidy, start, end, n, depth))
    mat = np.asarray(mat, np.float32).reshape(n, 5, 41, 5)
    assert np.array_equal(mat, mat.astype(np.int16).astype(np.float32))
    np.savez_compressed(
        os.path.join(OUT, "snp_%s.npz" % case), world=np.array(world_name), seq=np.array(seq),
        ploidy=np.array(ploidy), start=start, end=end, threshold=np.array(threshold, np.float64), mincov=mincov,
        maxcov=maxcov, min_allele_freq=np.float64(min_allele_freq), min_nbr_sites=min_nbr_sites,
        supplementary=supplementary,
        exclude=np.array([(a, b) for (_, a, b) in (exclude or [])], np.int64).reshape(-1, 2),
        pos=np.asarray(pos, np.int64), ref=np.asarray(ref, np.int32).reshape(n, 4), mat=mat.astype(np.int16),
        dp=np.asarray(dp, np.int64), freq=np.asarray(freq, np.float64), depth=np.float64(depth),
        fwd_dp=np.asarray(fwd, np.float64).reshape(n, 4), rev_dp=np.asarray(rev, np.float64).reshape(n, 4), **(extra or {}))
    return np.asarray(pos, np.int64)


def mates_world(w, start, end, seed):
    """`w` with some alignments RENAMED to share another alignment's read name and flagged supplementary (0x800, strand bit redrawn): what a split
    read looks like to the pileup (generate_SNP_pileups.py:141-143,175,185 key strand, bases and neighbour lookups by NAME).  Every group's
    primary overlaps [start, end] (the reference raises KeyError for a name without a primary in its fetch window).  Kinds, in turn: a later
    overlapping alignment, an earlier overlapping one, one nearby without overlap, two partners.  -> (world, name id per alignment)"""
    import copy
    rng = np.random.Generator(np.random.PCG64(seed))
    R = w.n_reads
    name_id = np.arange(R, dtype=np.int32)
    flag = w.read_flag.copy()
    plain = [r for r in range(R) if int(flag[r]) in (0, 16)]
    prim = [r for r in plain if w.read_start[r] <= end and w.read_end[r] > start]
    rng.shuffle(prim)
    used, kinds, made = set(), 0, []
    for r1 in prim:
        if r1 in used:
            continue
        ov = [r for r in plain if r != r1 and r not in used and w.read_start[r] < w.read_end[r1] and w.read_start[r1] < w.read_end[r]]
        near = [r for r in plain if r != r1 and r not in used and r not in ov
                and min(abs(int(w.read_start[r]) - int(w.read_end[r1])), abs(int(w.read_start[r1]) - int(w.read_end[r]))) < 15_000]
        kind = kinds % 4
        pick = {0: [r for r in ov if r > r1][:1], 1: [r for r in ov if r < r1][-1:], 2: near[:1], 3: ([r for r in ov if r > r1][:1] + near[:1])}[kind]
        if not pick or (kind == 3 and len(pick) < 2):
            continue
        kinds += 1
        used.add(r1)
        for r2 in pick:
            used.add(r2)
            name_id[r2] = name_id[r1]
            flag[r2] = 0x800 | (16 if rng.random() < 0.5 else 0)
        made.append((r1, pick))
        if len(made) >= 14:
            break
    w2 = copy.copy(w)
    w2.read_flag = flag
    w2.names = ["r%07d" % i for i in name_id]
    print("mates_world: %d names shared by %d alignments" % (len(made), len(made) + sum(len(p) for _, p in made)))
    return w2, name_id


def make_snp_goldens():
    w_ont = make_world(seed=812, length=135_000, depth=18, tech="ont", read_len_scale=0.8)
    # decorate some pileup strings with indel suffixes and explicit 'N' letters (only x[0] is read, :162)
    rng = np.random.Generator(np.random.PCG64(5))
    deco = {}
    for _ in range(4000):
        i = int(rng.integers(0, w_ont.n_reads))
        p0 = int(rng.integers(w_ont.read_start[i] - 1, w_ont.read_end[i] - 1))
        deco[(i, p0)] = ["+2GG", "-1N", "+1a", "-3NNN"][int(rng.integers(0, 4))]
    w_ont.meta["deco"] = deco
    save_world("ont", w_ont)
    w_hifi = make_world(seed=813, length=90_000, depth=24, tech="hifi", read_len_scale=0.6, het_rate=1 / 400.0,
                        sys_err_rate=0.02)
    save_world("hifi", w_hifi)
    w_deep = make_world(seed=814, length=24_000, depth=120, tech="ont", read_len_scale=0.25)
    save_world("deep", w_deep)

    run_snp("ont_dip", "ont", w_ont, "ont", "diploid", 52_000, 80_000)
    run_snp("ont_dip_start", "ont", w_ont, "ont", "diploid", 1, 20_000)
    run_snp("ont_dip_end", "ont", w_ont, "ont", "diploid", 110_000, 135_000)
    run_snp("ont_hap", "ont", w_ont, "ont", "haploid", 60_000, 75_000)
    run_snp("short_ont", "ont", w_ont, "short_ont", "diploid", 55_000, 75_000)
    run_snp("ul_ont", "ont", w_ont, "ul_ont", "diploid", 55_000, 75_000)
    run_snp("ul_ont_extreme", "ont", w_ont, "ul_ont_extreme", "diploid", 60_000, 70_000)
    run_snp("ont_exclude", "ont", w_ont, "ont", "diploid", 52_000, 70_000,
            exclude=[("chr20", 55_000, 58_000), ("chr20", 30_000, 41_000), ("chrX", 1, 100)])
    run_snp("ont_suppl_params", "ont", w_ont, "ont", "diploid", 60_000, 72_000, threshold=(0.3, 0.7), mincov=8,
            min_allele_freq=0.2, supplementary=True, min_nbr_sites=3)
    run_snp("ont_empty", "ont", w_ont, "ont", "diploid", 60_000, 60_400, min_allele_freq=0.999, mincov=500)
    # alignments that share read names (split reads under dct['supplementary']): the world "ont" with the names / flags stored in the case file
    w_m, name_id = mates_world(w_ont, 60_000, 72_000, seed=77)
    plain = run_snp("ont_mates_off", "ont", w_ont, "ont", "diploid", 60_000, 72_000, supplementary=True, mincov=4)
    got = run_snp("ont_mates", "ont", w_m, "ont", "diploid", 60_000, 72_000, supplementary=True, mincov=4,
                  extra=dict(name_id=name_id, read_flag=w_m.read_flag))
    os.remove(os.path.join(OUT, "snp_ont_mates_off.npz"))                # (only its sites: the renamed world must not be the plain one in disguise)
    z0, z1 = plain, got
    print("   sites: %d with shared names, %d with unique names" % (len(z1), len(z0)))
    run_snp("hifi_pacbio_dip", "hifi", w_hifi, "pacbio", "diploid", 30_000, 60_000, threshold=(0.3, 0.7))
    run_snp("hifi_pacbio_hap", "hifi", w_hifi, "pacbio", "haploid", 30_000, 60_000)
    run_snp("deep_ont", "deep", w_deep, "ont", "diploid", 6_000, 18_000)


def make_cnd_pos_goldens():
    rng = np.random.Generator(np.random.PCG64(99))
    rec = {}
    k = 0
    for seq in ("ont", "short_ont", "ul_ont", "ul_ont_extreme", "pacbio"):
        for dens in (0.0002, 0.001, 0.01):
            span = 700_000
            sites = np.nonzero(rng.random(span) < dens)[0] + 1_000_000
            for v in (1_000_010, 1_350_000, 1_350_001, 1_699_990, int(sites[len(sites) // 2])):
                l, r = ref_snp.get_cnd_pos(v, sites, seq)
                rec["c%d_seq" % k] = np.array(seq)
                rec["c%d_v" % k] = v
                rec["c%d_sites" % k] = sites.astype(np.int32)
                rec["c%d_l" % k] = np.array(l, np.int64)
                rec["c%d_r" % k] = np.array(r, np.int64)
                k += 1
    rec["n"] = k
    np.savez_compressed(os.path.join(OUT, "cnd_pos.npz"), **rec)
    print("cnd_pos cases:", k)


def make_caller_goldens():
    """Run the reference's caller() (snpCaller.py:57-203) with TensorFlow stubbed and the model classes
    replaced by canned-probability tables; capture the VCF lines it writes."""
    import queue

    from nanocaller_src import snpCaller as ref_caller

    rng = np.random.Generator(np.random.PCG64(7))
    n = 400
    # canned per-site head probabilities, f32, away from the 1-p < 1e-4 region where numpy-1 vs numpy-2
    # casting changes the QUAL text; saturated cases are hand-enumerated in tests instead.
    probs = rng.random((n, 4)).astype(np.float32) * np.float32(0.9998) + np.float32(1e-4)
    probs[::7] = np.round(probs[::7])                       # many 0/1-ish values -> ties kept apart below
    probs = np.clip(probs, 1e-4, 1 - 1e-4).astype(np.float32)
    # make ties impossible (E15): perturb so all four values differ per site
    for j in range(n):
        while len(set(probs[j].tolist())) < 4:
            probs[j] = np.clip(probs[j] + (rng.random(4).astype(np.float32) - np.float32(0.5)) * np.float32(2e-3),
                               2e-4, 1 - 2e-4).astype(np.float32)
    ref = rng.integers(0, 4, size=n)
    pos = np.sort(rng.choice(np.arange(1000, 90000), size=n, replace=False))
    dp = rng.integers(8, 80, size=n)
    freq = rng.random(n)
    fwd = rng.integers(0, 30, size=(n, 4)).astype(np.float64)
    rev = rng.integers(0, 30, size=(n, 4)).astype(np.float64)
    hap_probs = rng.dirichlet(np.ones(4) * 0.3, size=n).astype(np.float32)
    hap_probs = np.clip(hap_probs, 1e-4, 1 - 1e-4).astype(np.float32)

    state = {"i": 0}

    class FakeT:
        def __init__(self, a):
            self.a = a

        def numpy(self):
            return self.a

        def __getitem__(self, k):
            return self.a[k]

    class FakeSNP:
        def load_weights(self, p):
            return self

        def expect_partial(self):
            return self

        def __call__(self, inputs):
            b = len(inputs[0])
            i = state["i"]
            pr = probs[i:i + b]
            state["i"] += b
            outs = [np.stack([1 - pr[:, k], pr[:, k]], axis=1).astype(np.float32) for k in range(4)]
            return outs + [np.tile(np.array([[0.5, 0.5]], np.float32), (b, 1))]

    class FakeHap:
        def load_weights(self, p):
            return self

        def __call__(self, inputs):
            if len(inputs[0]) == 1 and not np.any(inputs[0]):
                return None
            b = len(inputs[0])
            i = state["i"]
            state["i"] += b
            return FakeT(hap_probs[i:i + b])

    out = {}
    for ploidy in ("diploid", "haploid"):
        state["i"] = 0
        ref_caller.SNP_model = FakeSNP
        ref_caller.haploid_SNP_model = FakeHap
        ref_caller.get_SNP_model = lambda name: ("x", 48.0)
        onehot = np.eye(4, dtype=np.int32)[ref]
        mat = np.zeros((n, 5, 41, 5), np.float32)
        ref_caller.get_snp_testing_candidates = lambda params, chunk: (pos, onehot, mat, dp, freq, 30.0, fwd, rev)

        class P:
            _identity = (1,)

        ref_caller.current_process = lambda: P
        tmpdir = "/tmp/nc_gold_vcf"
        os.makedirs(tmpdir, exist_ok=True)
        params = dict(intermediate_snp_files_dir=tmpdir, prefix="g", snp_model="ONT-HG002",
                      disable_coverage_normalization=False)
        q = queue.Queue()
        q.put(dict(chrom="chr20", start=1, end=100000, ploidy=ploidy))
        cq = queue.Queue()
        files = []
        ref_caller.caller(params, q, cq, files)
        lines = open(files[0]).read()
        out["vcf_" + ploidy] = np.array(lines)
        print("caller", ploidy, lines.count("\n"), "lines")
    np.savez_compressed(os.path.join(OUT, "caller_vcf.npz"), probs=probs, hap_probs=hap_probs, ref=ref, pos=pos,
                        dp=dp, freq=freq, fwd=fwd, rev=rev, **out)


def make_msa_goldens():
    from nanocaller_src import generate_indel_pileups as ref_indel

    rng = np.random.Generator(np.random.PCG64(11))
    rec = {}
    k = 0
    for ncols, nrows in ((90, 7), (128, 20), (161, 33), (200, 12), (170, 2)):
        ref_row = rng.integers(0, 4, size=ncols)
        gap = rng.random(ncols) < 0.1
        ref_row[gap] = 4
        rows = np.tile(ref_row, (nrows, 1))
        e = rng.random(rows.shape)
        rows[e < 0.1] = rng.integers(0, 5, size=int((e < 0.1).sum()))
        # every column needs at least one non-gap symbol overall in real MUSCLE output; not required here
        sym = "AGTC-"
        names = ["rd%03d" % i for i in range(nrows)]
        fasta = "".join(">%s_SEQ\n%s\n" % (nm, "".join(sym[c] for c in row)) for nm, row in zip(names, rows))
        fasta += ">ref_SEQ\n%s\n" % "".join(sym[c] for c in ref_row)

        class FakePopen:
            def __init__(self, *a, **kw):
                pass

            def communicate(self, input=None):
                return (fasta.encode(), b"")

        ref_indel.Popen = FakePopen
        seq_list = {nm: "ACGT" for nm in names}
        flag, _, mat, cns, ref_seq = ref_indel.msa(seq_list, "ACGT", 100, 2, 160)
        assert flag == 1
        rec["m%d_rows" % k] = rows.astype(np.uint8)
        rec["m%d_ref" % k] = ref_row.astype(np.uint8)
        rec["m%d_mat" % k] = np.asarray(mat, np.float64)
        rec["m%d_cns" % k] = np.array(cns)
        rec["m%d_refseq" % k] = np.array(ref_seq)
        k += 1
    rec["n"] = k
    np.savez_compressed(os.path.join(OUT, "indel_msa.npz"), **rec)
    print("msa cases:", k)


def make_indel_caller_goldens():
    """Run the reference's indel_run() (indelCaller.py:41-189) with TensorFlow stubbed, canned probabilities and
    canned candidate tuples; capture the VCF lines."""
    import queue

    from nanocaller_src import indelCaller as ref_ic

    rng = np.random.Generator(np.random.PCG64(21))
    n = 330                                   # > 3 batches of 100: `prev` carries across batches
    bases = "ACGT"

    def rs(k):
        return "".join(bases[i] for i in rng.integers(0, 4, size=k))

    def allele():
        u = rng.random()
        if u < 0.35:
            return (None, None)
        ref = rs(int(rng.integers(1, 8)))
        alt = ref[0] + rs(int(rng.integers(0, 6))) if rng.random() < 0.5 else ref[:max(1, len(ref) - int(rng.integers(0, 4)))]
        return (ref, alt)

    pos = np.sort(rng.choice(np.arange(100, 4000), size=n, replace=False)).tolist()
    probs = rng.dirichlet(np.ones(4) * 0.4, size=n).astype(np.float32)
    probs[::9] = np.float32([0.97, 0.01, 0.01, 0.01])                 # hom-ref > 0.95: skipped
    alleles = []
    for j in range(n):
        a0, a1, at = allele(), allele(), allele()
        if j % 11 == 0 and a0[0]:
            a1 = a0                                                   # identical haplotype alleles -> 1/1
        alleles.append([a0, a1, at])
    phase = [None if rng.random() < 0.4 else int(rng.integers(1000, 99999)) for _ in range(n)]
    x = np.zeros((n, 5, 128, 2))
    hap_probs = rng.random((n, 1)).astype(np.float32)
    hap_alleles = [a[2] for a in alleles]
    state = {"i": 0}

    class FakeModel:
        def load_weights(self, p):
            return self

        def expect_partial(self):
            return self

        def build(self, input_shape=None):
            return None

    class FakeDip(FakeModel):
        def __call__(self, xb):
            b = len(xb)
            i = state["i"]
            state["i"] += b
            return probs[i:i + b]

    class FakeHap(FakeModel):
        def __call__(self, xb):
            b = len(xb)
            i = state["i"]
            state["i"] += b
            return hap_probs[i:i + b]

    class P:
        _identity = (1,)

    ref_ic.Indel_model = FakeDip
    ref_ic.haploid_Indel_model = FakeHap
    ref_ic.get_indel_model = lambda name: "x"
    ref_ic.current_process = lambda: P
    ref_ic.get_indel_testing_candidates = lambda params, chunk: (pos, x, x, x, alleles, phase)
    ref_ic.get_indel_testing_candidates_haploid = lambda params, chunk: (pos, x, hap_alleles)
    out = {}
    tmpdir = "/tmp/nc_gold_indel"
    os.makedirs(tmpdir, exist_ok=True)
    for ploidy in ("diploid", "haploid"):
        state["i"] = 0
        q = queue.Queue()
        q.put(("indel", dict(chrom="chr20", start=1, end=5000, ploidy=ploidy)))
        files = []
        ref_ic.indel_run(dict(intermediate_indel_files_dir=tmpdir, prefix="g" + ploidy, indel_model="ONT-HG002"), {}, q,
                         queue.Queue(), files)
        txt = open(files[0]).read()
        out["vcf_" + ploidy] = np.array(txt)
        print("indel_run", ploidy, txt.count("\n"), "lines")
    import json
    np.savez_compressed(os.path.join(OUT, "indel_caller_vcf.npz"), pos=np.array(pos), probs=probs, hap_probs=hap_probs,
                        alleles=np.array(json.dumps(alleles)), phase=np.array(json.dumps(phase)), **out)


def make_indel_scan_goldens():
    """Pass 1 of get_indel_testing_candidates (generate_indel_pileups.py:197-304): the `variants` dict, captured from
    the reference's own frame when it opens its second pileup (stub pysam, CAPTURE_INDEL)."""
    from nanocaller_amd.synth import add_indels
    from nanocaller_src import generate_indel_pileups as ref_indel

    w = add_indels(make_world(seed=815, length=60_000, depth=28, tech="ont", read_len_scale=0.5, odd_flag_frac=0.03))
    ev_off, ev_pos, ev_len = w.meta["events"]
    np.savez_compressed(os.path.join(OUT, "world_indel.npz"), chrom=np.array(w.chrom),
                        ref=np.frombuffer(w.ref.encode(), dtype=np.uint8), read_start=w.read_start, read_end=w.read_end,
                        read_flag=w.read_flag, read_off=w.read_off, codes=w.codes, ev_off=ev_off, ev_pos=ev_pos,
                        ev_len=ev_len, hap=w.meta["hap"], ps=w.meta["ps"])
    pysam.register("bam", w)
    pysam.register("fa", w)
    pysam.register("bed", [("chr20", 30_000, 30_400)])
    rec = {}
    k = 0
    for (start, end, kw) in [(5_000, 55_000, {}), (1, 20_000, {}), (20_000, 59_990, dict(mincov=8)),
                             (10_000, 40_000, dict(ins_t=0.3, del_t=0.3, win_size=20, small_win_size=2)),
                             (25_000, 35_000, dict(exclude_bed="bed")), (40_000, 41_000, dict(mincov=200))]:
        dct = dict(seq="ont", fasta_path="fa", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6,
                   exclude_bed=None, supplementary=False, impute_indel_phase=False)
        dct.update(kw)
        pysam.CAPTURE_INDEL = True
        pysam.CAPTURED.clear()
        out = ref_indel.get_indel_testing_candidates(dct, dict(chrom=w.chrom, start=start, end=end, sam_path="bam"))
        pysam.CAPTURE_INDEL = False
        assert len(out[0]) == 0
        v = pysam.CAPTURED["variants"]
        keys = sorted(v)
        rec["s%d_start" % k], rec["s%d_end" % k] = start, end
        for name in ("mincov", "win_size", "small_win_size"):
            rec["s%d_%s" % (k, name)] = dct[name]
        rec["s%d_ins_t" % k], rec["s%d_del_t" % k] = np.float64(dct["ins_t"]), np.float64(dct["del_t"])
        rec["s%d_excl" % k] = np.array([[30_000, 30_400]] if dct["exclude_bed"] else [], np.int64).reshape(-1, 2)
        rec["s%d_pos" % k] = np.array(keys, np.int64)
        rec["s%d_type" % k] = np.array([v[p] for p in keys], np.int64)
        print("indel scan [%d,%d] %s -> %d variants (%d type 0)" % (start, end, kw, len(keys), sum(1 for p in keys if v[p] == 0)))
        k += 1
    rec["n"] = k
    np.savez_compressed(os.path.join(OUT, "indel_scan.npz"), **rec)
    # haploid pass 1 (generate_indel_pileups_haploid.py:185-241): one read set, no HP split
    from nanocaller_src import generate_indel_pileups_haploid as ref_hap
    rec, k = {}, 0
    for (start, end, kw) in [(5_000, 55_000, {}), (1, 20_000, dict(mincov=12)),
                             (10_000, 40_000, dict(ins_t=0.3, del_t=0.3, win_size=20, small_win_size=2)),
                             (25_000, 35_000, dict(exclude_bed="bed")), (40_000, 41_000, dict(mincov=200))]:
        dct = dict(seq="ont", fasta_path="fa", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6,
                   exclude_bed=None, supplementary=False, impute_indel_phase=False)
        dct.update(kw)
        pysam.CAPTURE_INDEL = True
        pysam.CAPTURED.clear()
        out = ref_hap.get_indel_testing_candidates_haploid(dct, dict(chrom=w.chrom, start=start, end=end, sam_path="bam"))
        pysam.CAPTURE_INDEL = False
        assert len(out[0]) == 0
        v = pysam.CAPTURED["variants"]
        keys = sorted(v)
        rec["s%d_start" % k], rec["s%d_end" % k] = start, end
        for name in ("mincov", "win_size", "small_win_size"):
            rec["s%d_%s" % (k, name)] = dct[name]
        rec["s%d_ins_t" % k], rec["s%d_del_t" % k] = np.float64(dct["ins_t"]), np.float64(dct["del_t"])
        rec["s%d_excl" % k] = np.array([[30_000, 30_400]] if dct["exclude_bed"] else [], np.int64).reshape(-1, 2)
        rec["s%d_pos" % k] = np.array(keys, np.int64)
        rec["s%d_type" % k] = np.array([v[p] for p in keys], np.int64)
        print("haploid indel scan [%d,%d] %s -> %d variants (%d type 0)" % (start, end, kw, len(keys), sum(1 for p in keys if v[p] == 0)))
        k += 1
    rec["n"] = k
    np.savez_compressed(os.path.join(OUT, "indel_scan_hap.npz"), **rec)


def make_indel_impute_goldens():
    """Pass 1 with dct['impute_indel_phase'] (generate_indel_pileups.py:278-304): `variants` and `extra_variants` captured
    from the reference's frame, on the indel world with unphased stretches and per-read inserted bases."""
    from nanocaller_amd.synth import add_indels, unphase_blocks
    from nanocaller_src import generate_indel_pileups as ref_indel

    w = add_indels(make_world(seed=815, length=60_000, depth=28, tech="ont", read_len_scale=0.5, odd_flag_frac=0.03))
    w = unphase_blocks(w, [(8_000, 16_000), (33_000, 39_000), (50_000, 52_000)], seed=815)
    idx = {n: i for i, n in enumerate(w.names)}
    pysam.register("bam_imp", w)
    pysam.register("fa_imp", w)
    pysam.register("bed_imp", [("chr20", 35_000, 36_000)])
    rec = dict(hap=w.meta["hap"], ins_off=w.meta["ev_ins"][0], ins_bases=w.meta["ev_ins"][1])
    k = 0
    for (start, end, kw) in [(1, 30_000, dict(del_t=0.4)), (5_000, 59_000, dict(del_t=0.4)), (30_000, 45_000, {}),
                             (7_000, 40_000, dict(ins_t=0.3, del_t=0.3, mincov=6, win_size=10, small_win_size=2)),
                             (30_000, 45_000, dict(del_t=0.4, exclude_bed="bed_imp")), (8_000, 16_000, dict(del_t=0.4, mincov=2)),
                             (8_000, 16_000, dict(del_t=0.2, ins_t=0.2, mincov=10)), (49_000, 53_000, dict(del_t=0.05, ins_t=0.05))]:
        dct = dict(seq="ont", fasta_path="fa_imp", win_size=40, small_win_size=4, mincov=4, maxcov=160, ins_t=0.4, del_t=0.6,
                   exclude_bed=None, supplementary=False, impute_indel_phase=True)
        dct.update(kw)
        pysam.CAPTURE_INDEL = True
        pysam.CAPTURED.clear()
        out = ref_indel.get_indel_testing_candidates(dct, dict(chrom=w.chrom, start=start, end=end, sam_path="bam_imp"))
        pysam.CAPTURE_INDEL = False
        assert len(out[0]) == 0
        v, ex = pysam.CAPTURED["variants"], pysam.CAPTURED["extra_variants"]
        keys, xkeys = sorted(v), sorted(ex)
        rec["s%d_start" % k], rec["s%d_end" % k] = start, end
        for name in ("mincov", "win_size", "small_win_size"):
            rec["s%d_%s" % (k, name)] = dct[name]
        rec["s%d_ins_t" % k], rec["s%d_del_t" % k] = np.float64(dct["ins_t"]), np.float64(dct["del_t"])
        rec["s%d_excl" % k] = np.array([[35_000, 36_000]] if dct["exclude_bed"] else [], np.int64).reshape(-1, 2)
        rec["s%d_pos" % k] = np.array(keys, np.int64)
        rec["s%d_type" % k] = np.array([v[p] for p in keys], np.int64)
        rec["s%d_xpos" % k] = np.array(xkeys, np.int64)
        for j, p in enumerate(xkeys):                             # the two read collections as sorted read indices
            for side in (0, 1):
                rec["s%d_x%d_%d" % (k, j, side)] = np.array(sorted(idx[n] for n in ex[p][side]), np.int32)
        n_split = sum(1 for p in xkeys if isinstance(ex[p][0], list))
        print("impute scan [%d,%d] %s -> %d variants, %d imputed (%d by halving the top group)" % (start, end, kw, len(keys), len(xkeys), n_split))
        k += 1
    rec["n"] = k
    np.savez_compressed(os.path.join(OUT, "indel_impute.npz"), **rec)


def make_chunk_goldens():
    """get_chunks (utils.py:67-83) on a few region lists; utils.py imports pysam at module top (stub)."""
    import json

    from nanocaller_src import utils as ref_utils
    cases = []
    for regions, cpu, kw in [
        ([("chr22", 20000000, 21000000, "diploid")], 2, {}),
        ([("chr22", 20000000, 21000000, "diploid")], 16, {}),
        ([("chr20", 1, 64444167, "diploid")], 16, {}),
        ([("chr1", 1, 248956422, "diploid"), ("chrX", 1, 156040895, "haploid"), ("chrM", 1, 16569, "haploid")], 8, {}),
        ([("chr1", 1, 1234567, "diploid")], 3, dict(max_chunk_size=100000)),
        ([("c", 5, 5, "diploid"), ("d", 10, 10010, "haploid")], 4, {}),
    ]:
        out = ref_utils.get_chunks(regions, cpu, **kw)
        cases.append(dict(regions=[list(r) for r in regions], cpu=cpu, kw=kw, chunks=out))
    with open(os.path.join(OUT, "chunks.json"), "w") as f:
        json.dump(cases, f)
    print("chunk cases:", len(cases), "total chunks", sum(len(c["chunks"]) for c in cases))


# ----------------------------------------------------------------------------- pass 2 of the indel featuriser (a11-a13)
def _install_aligner_stubs(ref_mod, check_every=1):
    """MUSCLE and parasail are absent.  The reference's msa() and allele_prediction() are run UNCHANGED with
    * `Popen` replaced by an object that answers the FASTA the reference writes with the star alignment of the same reads
      (nc_star_msa, the aligner the product uses when `muscle` is not on PATH), in the FASTA format the reference parses;
    * `parasail.nw_trace` answered by the Gotoh aligner behind nc_nw_cigar.
    EVERY call (check_every = 1; it was every 25th until round 5) is answered by the pure-Python restatements in oracle/ (star_msa_ref,
    nw_cigar_ref) -- the goldens are "reference code + oracle aligner", no product code in their making -- and the product's host aligners
    (gip.star_aligner, gip.nw_cigar) are asserted to give the same answer on every one of those calls."""
    import parasail

    from nanocaller_amd import generate_indel_pileups as gip
    from oracle import oracle

    cnt = {"msa": 0, "nw": 0}

    class FakePopen:
        def __init__(self, argv, **kw):
            assert argv[0] == "muscle", argv

        def communicate(self, input=None):
            recs = input.decode("utf-8")[1:].split(">")
            names, seqs, ref = [], [], None
            for rec in recs:
                nm, sq = rec.split("\n", 1)
                sq = sq.replace("\n", "")
                assert nm.endswith("_SEQ")
                if nm == "ref_SEQ":
                    ref = sq
                else:
                    names.append(nm[:-4])
                    seqs.append(sq)
            if not seqs:
                return (b">ref_SEQ\n" + ref.encode() + b"\n", b"")
            from nanocaller_amd import _lib
            cnt["msa"] += 1
            if check_every == 1 or cnt["msa"] % check_every == 1:
                rows, ref_row = oracle.star_msa_ref(seqs, ref, *_lib.STAR_SCORING)
                assert (rows, ref_row) == tuple(gip.star_aligner(names, seqs, ref)), "product star aligner differs from the oracle's"
            else:
                rows, ref_row = gip.star_aligner(names, seqs, ref)
            out = "".join(">%s_SEQ\n%s\n" % (n, r) for n, r in zip(names, rows)) + ">ref_SEQ\n%s\n" % ref_row
            return (out.encode(), b"")

    def backend(s1, s2, open_, extend, match, mismatch):
        cnt["nw"] += 1
        if check_every == 1 or cnt["nw"] % check_every == 1:
            ops = oracle.nw_cigar_ref(s1, s2, open_, extend, match, mismatch)
            assert ops == gip.nw_cigar(s1, s2, open_, extend, match, mismatch), "product Gotoh aligner differs from the oracle's"
        else:
            ops = gip.nw_cigar(s1, s2, open_, extend, match, mismatch)
        return ops

    ref_mod.Popen = FakePopen
    parasail.BACKEND = backend
    return cnt


def make_pass2_goldens():
    """The reference's FULL get_indel_testing_candidates 6-tuple / haploid 3-tuple (generate_indel_pileups.py:129-371,
    generate_indel_pileups_haploid.py:128-277) on record-based worlds served by the stub pysam (pileups[*].alignment.
    query_sequence, query_position_or_next), plus every (alt, ref_seq, max_range) -> (REF, ALT) the reference's own
    allele_prediction (:77-127) returned on the way and on a set of seeded mutated pairs."""
    import json

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import bamio
    from nanocaller_src import generate_indel_pileups as ref_indel
    from nanocaller_src import generate_indel_pileups_haploid as ref_hap

    calls = []

    def wrap(mod):
        orig = mod.allele_prediction

        def spy(alt, ref_seq, max_range):
            out = orig(alt, ref_seq, max_range)
            calls.append([alt, ref_seq, int(max_range), out[0], out[1]])
            return out
        mod.allele_prediction = spy
        return orig
    ref_ap = wrap(ref_indel)
    wrap(ref_hap)
    _install_aligner_stubs(ref_indel)
    ref_hap.Popen = ref_indel.Popen

    worlds = {"a": bamio.make_pass2_world(seed=11, length=24_000, depth=16),
              "b": bamio.make_pass2_world(seed=31, length=20_000, depth=18, blocks=[(4_000, 15_000)])}
    rec = {}
    for wn, w in worlds.items():
        rec.update(bamio.world_arrays(w, "w%s_" % wn))
        pysam.register_records("bam_" + wn, w.chrom, w.length, w.ref, bamio.world_to_records(w, None))
        pysam.register_records("fa_" + wn, w.chrom, w.length, w.ref, [])
    base = dict(seq="ont", win_size=40, small_win_size=4, mincov=2, maxcov=160, ins_t=0.4, del_t=0.6, supplementary=False,
                exclude_bed=None, impute_indel_phase=False)
    cases = [("a", "diploid", 2_000, 22_000, {}), ("a", "haploid", 2_000, 22_000, {}),
             ("a", "diploid", 1, 9_000, dict(seq="pacbio", mincov=3)), ("a", "haploid", 15_000, 24_000, dict(seq="pacbio", mincov=4)),
             ("a", "diploid", 5_000, 16_000, dict(supplementary=True, win_size=20, small_win_size=2, ins_t=0.3, del_t=0.4)),
             ("b", "diploid", 1_000, 19_000, dict(impute_indel_phase=True, del_t=0.4)),
             ("b", "diploid", 1_000, 19_000, dict(impute_indel_phase=False, del_t=0.4)),
             ("a", "diploid", 12_000, 12_300, dict(mincov=40))]
    for k, (wn, ploidy, start, end, kw) in enumerate(cases):
        w = worlds[wn]
        dct = dict(base, fasta_path="fa_" + wn)
        dct.update(kw)
        chunk = dict(chrom=w.chrom, start=start, end=end, sam_path="bam_" + wn)
        if ploidy == "diploid":
            pos, x0, x1, x2, alleles, phase = ref_indel.get_indel_testing_candidates(dct, chunk)
            xs = [np.asarray(x0), np.asarray(x1), np.asarray(x2)]
        else:
            pos, x, alleles = ref_hap.get_indel_testing_candidates_haploid(dct, chunk)
            xs, phase = [np.asarray(x)], None
        rec["c%d_world" % k], rec["c%d_ploidy" % k] = np.array(wn), np.array(ploidy)
        rec["c%d_start" % k], rec["c%d_end" % k] = start, end
        rec["c%d_dct" % k] = np.array(json.dumps({kk: vv for kk, vv in dct.items() if kk != "fasta_path"}))
        rec["c%d_pos" % k] = np.asarray(pos, np.int64)
        for i, x in enumerate(xs):
            if len(pos):
                assert x.dtype == np.float64 and x.shape == (len(pos), 5, 128, 2)
                assert np.array_equal(x.astype(np.float32).astype(np.float64), x)        # f32-rounded values (:59)
                rec["c%d_x%d" % (k, i)] = x.astype(np.float32)
        rec["c%d_alleles" % k] = np.array(json.dumps(alleles))
        rec["c%d_phase" % k] = np.array(json.dumps(phase))
        print("pass2 case %d world=%s %s [%d,%d] %s -> %d sites" % (k, wn, ploidy, start, end, kw, len(pos)))
    rec["n"] = len(cases)
    np.savez_compressed(os.path.join(OUT, "indel_pass2.npz"), **rec)
    # ---- the reference's allele_prediction on seeded pairs (in addition to the calls it made above)
    n_pipeline = len(calls)
    rng = np.random.Generator(np.random.PCG64(43))
    letters = "AGTC"

    def rand_seq(n):
        return "".join(letters[i] for i in rng.integers(0, 4, size=n))
    for trial in range(260):
        ref = rand_seq(int(rng.integers(30, 262)))
        s = list(ref)
        for _ in range(int(rng.integers(0, 5))):
            i = int(rng.integers(0, len(s)))
            s[i] = letters[(letters.index(s[i]) + int(rng.integers(1, 4))) % 4]
        for _ in range(int(rng.integers(0, 3))):
            i = int(rng.integers(0, len(s)))
            ln = int(rng.choice([-30, -7, -3, -1, 1, 2, 5, 20]))
            if ln > 0:
                s[i:i] = list(rand_seq(ln))
            else:
                del s[i:i - ln]
        alt = "".join(s) or "A"
        if trial % 9 == 0:
            alt = alt[:int(rng.integers(1, len(alt) + 1))]                 # consensus shorter than the window
        mr = int(rng.choice([10, 40, 20]))
        try:
            out = ref_ap(alt, ref, mr)
            calls.append([alt, ref, mr, out[0], out[1]])
        except Exception as e:                                              # the latent tuple-mutation bug (E12) raises
            calls.append([alt, ref, mr, "!" + type(e).__name__, None])
    with open(os.path.join(OUT, "allele_prediction.json"), "w") as f:
        json.dump(dict(n_pipeline=n_pipeline, calls=calls), f)
    print("allele_prediction cases: %d from the pipeline + %d seeded (%d (None, None), %d raised)" % (
        n_pipeline, len(calls) - n_pipeline, sum(1 for c in calls if c[3] is None), sum(1 for c in calls if isinstance(c[3], str) and c[3].startswith("!"))))
    _allele_ties_block(ref_ap)


def _allele_ties_block(ref_ap):
    """The reference's allele_prediction on the tie-heavy (consensus, window, max_range) pairs of tests/align_cases.py (homopolymers, tandem
    repeats, runs in a flank, two-letter and disjoint sequences, the shape edges, per lane layout of the device aligner) -> its own file,
    tests/golden/allele_prediction_ties.json: {call name: [[alt, ref_seq, max_range, REF, ALT]]}, an exception as "!" + its type name."""
    import json

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import align_cases
    out, n, n_none, n_raised = {}, 0, 0, 0
    for name, (alts, refs, mrs) in align_cases.allele_calls().items():
        rows = []
        for alt, ref, mr in zip(alts, refs, mrs):
            try:
                r = ref_ap(alt, ref, mr)
                rows.append([alt, ref, int(mr), r[0], r[1]])
                n_none += r[0] is None
            except Exception as e:
                rows.append([alt, ref, int(mr), "!" + type(e).__name__, None])
                n_raised += 1
        out[name] = rows
        n += len(rows)
    with open(os.path.join(OUT, "allele_prediction_ties.json"), "w") as f:
        json.dump(dict(calls=out), f)
    print("allele_prediction tie cases: %d in %d calls (%d (None, None), %d raised)" % (n, len(out), n_none, n_raised))


def make_allele_ties_golden():
    """_allele_ties_block alone (make_pass2_goldens runs it too): the reference's unchanged allele_prediction over the oracle aligner,
    without rewriting indel_pass2.npz / allele_prediction.json"""
    from nanocaller_src import generate_indel_pileups as ref_indel
    _install_aligner_stubs(ref_indel)
    _allele_ties_block(ref_indel.allele_prediction)


# ----------------------------------------------------------------------------- CNNs through the reference's own call()
REFSRC = "/root/reference/nanocaller_src"


def make_cnn_goldens():
    """Probabilities returned by the reference's own model classes (model_architect.py:36-64, model_architect_SNP_haploid.py:
    33-53, model_architect_indel.py:28-48, model_architect_indels_haploid.py:29-48) with the reference's REAL checkpoints,
    executed on the numpy Keras layers of oracle/tools/refstub/tensorflow (float64 arithmetic on float32 inputs / weights).
    Inputs are the committed reference-made tensors (snp_*.npz, indel_pass2.npz), fed as snpCaller.py:90-111,167-183 and
    indelCaller.py:83-85,171 feed them."""
    import tensorflow as tf

    sys.path.insert(0, HERE)
    from convert_weights import INDEL_MODELS, SNP_MODELS
    from nanocaller_src.model_architect import SNP_model
    from nanocaller_src.model_architect_indel import Indel_model
    from nanocaller_src.model_architect_indels_haploid import haploid_Indel_model
    from nanocaller_src.model_architect_SNP_haploid import haploid_SNP_model

    assert tf.COMPUTE_DTYPE is np.float64 and not tf.RETURN_F32

    def coverage_of(prefix):
        return float(open(os.path.join(REFSRC, prefix + ".coverage")).readline().strip())

    def snp_inputs(case, n, train_cov, mode):
        z = np.load(os.path.join(OUT, "snp_%s.npz" % case))
        n = min(n, len(z["pos"]))
        x = z["mat"][:n].astype(np.float32)
        ref = z["ref"][:n]
        if mode == 0:      # snpCaller.py:96 under numpy < 2 (environment.yml:10): f32 array * f64 scalar multiplies in f32 (E7)
            x[:, 1:, :, :4] = x[:, 1:, :, :4] * np.float32(train_cov / float(z["depth"]))
        else:              # snpCaller.py:94: f32 array * f64 array -> f64 product, rounded into the f32 array
            x[:, 1:, :, :4] = (x[:, 1:, :, :4].astype(np.float64) * (train_cov / z["dp"][:n, None, None, None])).astype(np.float32)
        return n, x, ref.astype(np.float16)

    rec, k = {}, 0
    models = {}
    todo = [("ONT-HG002", "ont_dip", 400, 0), ("ONT-HG002", "deep_ont", 160, 0), ("ONT-HG002", "ont_dip_start", 120, 1),
            ("ONT-HG002", "ul_ont", 120, 0), ("CCS-HG002", "hifi_pacbio_dip", 400, 0), ("CLR-HG002", "short_ont", 120, 0)]
    todo += [(m, "ont_dip", 48, 0) for m in SNP_MODELS if m not in ("ONT-HG002",)]
    for name, case, n, mode in todo:
        prefix = SNP_MODELS[name]
        if name not in models:
            models[name] = SNP_model()
            models[name].load_weights(os.path.join(REFSRC, prefix)).expect_partial()
        cov = coverage_of(prefix)
        n, x, r16 = snp_inputs(case, n, cov, mode)
        out = models[name]([x, r16[:, 0][:, np.newaxis], r16[:, 1][:, np.newaxis], r16[:, 2][:, np.newaxis], r16[:, 3][:, np.newaxis]])
        out = np.stack([np.asarray(o) for o in out], axis=1)                      # (n, 5 heads A G T C GT, 2)
        assert out.shape == (n, 5, 2) and out.dtype == np.float64
        rec.update({"c%d_model" % k: np.array(name), "c%d_case" % k: np.array(case), "c%d_n" % k: n, "c%d_mode" % k: mode,
                    "c%d_cov" % k: np.float64(cov), "c%d_out" % k: out})
        k += 1
    rec["n"] = k
    hap = haploid_SNP_model()
    hap([np.zeros(5 * 41 * 5).reshape(1, 5, 41, 5), np.zeros(4).reshape(1, 4)])          # snpCaller.py:76-77
    hap.load_weights(os.path.join(REFSRC, "release_data/haploid_models/SNPs/CHM13/model.24-0.9985.h5"))
    h = 0
    for case, n, mode in (("ont_hap", 400, 0), ("hifi_pacbio_hap", 400, 0), ("ont_hap", 100, 1)):
        n, x, r16 = snp_inputs(case, n, 30, mode)                                 # hap_train_coverage (snpCaller.py:73)
        out = np.asarray(hap([x, r16]).numpy())
        assert out.shape == (n, 4)
        rec.update({"h%d_case" % h: np.array(case), "h%d_n" % h: n, "h%d_mode" % h: mode, "h%d_out" % h: out})
        h += 1
    rec["nh"] = h
    np.savez_compressed(os.path.join(OUT, "cnn_snp.npz"), **rec)
    print("cnn_snp: %d diploid cases (%d models), %d haploid cases" % (k, len(models), h))

    # ---- indel models on the reference-made pass-2 tensors
    zp = np.load(os.path.join(OUT, "indel_pass2.npz"))
    rec, k = {}, 0
    rng = np.random.Generator(np.random.PCG64(77))
    dense = np.round(rng.random((24, 15, 128, 2)) * 2 - 1, 3)                     # dense inputs: every tap of every filter is hit
    dense[..., 1] = (rng.random((24, 15, 128)) < 0.25)
    rec["dense"] = dense.astype(np.float32)
    todo = [(m, 0) for m in INDEL_MODELS] + [("ONT-HG002", 4), ("CCS-HG002", 2), ("ONT-HG002", 5), ("ONT-HG002", -1)]
    models = {}
    for name, c in todo:
        if name not in models:
            models[name] = Indel_model()
            models[name].load_weights(os.path.join(REFSRC, INDEL_MODELS[name])).expect_partial()
        if c >= 0:
            x = np.hstack([zp["c%d_x%d" % (c, i)].astype(np.float64) for i in range(3)])   # indelCaller.py:83
        else:
            x = dense.astype(np.float32).astype(np.float64)
        out = np.asarray(models[name](x))
        assert out.shape == (len(x), 4)
        rec.update({"c%d_model" % k: np.array(name), "c%d_src" % k: c, "c%d_out" % k: out})
        k += 1
    rec["n"] = k
    hm = haploid_Indel_model()
    hm.build(input_shape=(1, 5, 128, 2))                                          # indelCaller.py:56-57
    hm.load_weights(os.path.join(REFSRC, "release_data/haploid_models/indels/CHM13/model.19-0.9811.h5"))
    h = 0
    for c in (1, 3, -1):
        x = zp["c%d_x0" % c].astype(np.float64) if c >= 0 else dense[:, :5].astype(np.float32).astype(np.float64)
        out = np.asarray(hm(x))
        assert out.shape == (len(x), 1)
        rec.update({"h%d_src" % h: c, "h%d_out" % h: out})
        h += 1
    rec["nh"] = h
    np.savez_compressed(os.path.join(OUT, "cnn_indel.npz"), **rec)
    print("cnn_indel: %d diploid cases (%d models), %d haploid cases" % (k, len(models), h))


def make_e2e_goldens():
    """The reference's worker loops END TO END in the build container: snpCaller.caller (snpCaller.py:57-203) and
    indelCaller.indel_run (indelCaller.py:41-189) unchanged, featurisers on the stub pysam, models = the reference's classes
    on the numpy Keras layers with the real checkpoints (outputs rounded to float32 as TensorFlow returns them).  The VCF
    text they write is the golden.  Caveat: this container has numpy 2, the reference pins numpy < 2 -- the
    coverage scale is multiplied in float64 here and in float32 there (a last-place difference of the inputs)."""
    import queue

    import tensorflow as tf

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import bamio
    from nanocaller_src import indelCaller as ref_ic
    from nanocaller_src import snpCaller as ref_caller
    from nanocaller_src import generate_indel_pileups as ref_indel
    from nanocaller_src import generate_indel_pileups_haploid as ref_hap

    class P:
        _identity = (1,)

    tf.RETURN_F32 = True
    out = {}
    try:
        # ---- SNPs: the committed worlds (world_ont.npz / world_hifi.npz are exactly these)
        w_ont = make_world(seed=812, length=135_000, depth=18, tech="ont", read_len_scale=0.8)
        w_hifi = make_world(seed=813, length=90_000, depth=24, tech="hifi", read_len_scale=0.6, het_rate=1 / 400.0, sys_err_rate=0.02)
        ref_caller.current_process = lambda: P
        tmpdir = "/tmp/nc_gold_e2e"
        os.makedirs(tmpdir, exist_ok=True)
        runs = [("snp_ont", w_ont, "ONT-HG002", "ont", [0.4, 0.6], False,
                 [("diploid", 52_000, 66_000), ("diploid", 66_000, 80_000), ("haploid", 60_000, 75_000)]),
                ("snp_ont_nonorm", w_ont, "ONT-HG002", "ont", [0.4, 0.6], True, [("diploid", 100_000, 112_000)]),
                ("snp_hifi", w_hifi, "CCS-HG002", "pacbio", [0.3, 0.7], False, [("diploid", 30_000, 60_000), ("haploid", 30_000, 45_000)])]
        for tag, w, model, seq, thr, nonorm, chunks in runs:
            pysam.register("bam", w)
            pysam.register("fa", w)
            params = dict(intermediate_snp_files_dir=tmpdir, prefix=tag, snp_model=model, disable_coverage_normalization=nonorm,
                          exclude_bed=None, sam_path="bam", fasta_path="fa", threshold=thr, supplementary=False, mincov=4,
                          maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, seq=seq)
            q = queue.Queue()
            for ploidy, a, b in chunks:
                q.put(dict(chrom=w.chrom, start=a, end=b, ploidy=ploidy))
            files = []
            ref_caller.caller(params, q, queue.Queue(), files)
            txt = open(files[0]).read()
            out[tag + "_vcf"] = np.array(txt)
            out[tag + "_chunks"] = np.array(json_dumps(chunks))
            out[tag + "_params"] = np.array(json_dumps({kk: vv for kk, vv in params.items() if kk not in ("intermediate_snp_files_dir", "sam_path", "fasta_path")}))
            print("e2e %s: %d VCF lines (%d PASS)" % (tag, txt.count("\n"), txt.count("\tPASS\t")))
        # ---- indels: the pass-2 worlds
        _install_aligner_stubs(ref_indel)
        ref_hap.Popen = ref_indel.Popen
        ref_ic.current_process = lambda: P
        z = np.load(os.path.join(OUT, "indel_pass2.npz"))
        for tag, wn, model, kw, chunks in [
                ("indel_a", "a", "ONT-HG002", {}, [("diploid", 2_000, 12_000), ("diploid", 12_000, 22_000), ("haploid", 2_000, 22_000)]),
                ("indel_b", "b", "CCS-HG002", dict(impute_indel_phase=True, del_t=0.4), [("diploid", 1_000, 19_000)])]:
            w = bamio.world_from_arrays(z, "w%s_" % wn)
            pysam.register_records("bam_e2e", w.chrom, w.length, w.ref, bamio.world_to_records(w, None))
            pysam.register_records("fa_e2e", w.chrom, w.length, w.ref, [])
            params = dict(intermediate_indel_files_dir=tmpdir, prefix=tag, indel_model=model, seq="ont", win_size=40, small_win_size=4,
                          mincov=2, maxcov=160, ins_t=0.4, del_t=0.6, supplementary=False, exclude_bed=None, impute_indel_phase=False,
                          fasta_path="fa_e2e")
            params.update(kw)
            q = queue.Queue()
            for ploidy, a, b in chunks:
                q.put(("indel", dict(chrom=w.chrom, start=a, end=b, ploidy=ploidy, sam_path="bam_e2e")))
            files = []
            ref_ic.indel_run(params, {}, q, queue.Queue(), files)
            txt = open(files[0]).read()
            out[tag + "_vcf"] = np.array(txt)
            out[tag + "_world"] = np.array(wn)
            out[tag + "_chunks"] = np.array(json_dumps(chunks))
            out[tag + "_params"] = np.array(json_dumps({kk: vv for kk, vv in params.items() if kk not in ("intermediate_indel_files_dir", "fasta_path")}))
            print("e2e %s: %d VCF lines" % (tag, txt.count("\n")))
    finally:
        tf.RETURN_F32 = False
    np.savez_compressed(os.path.join(OUT, "e2e_vcf.npz"), **out)


def json_dumps(o):
    import json
    return json.dumps(o)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    # order matters: "e2e" runs the reference's real loops and must come before "caller" / "indel_caller" replace the model classes
    what = sys.argv[1:] or ["snp", "cnd", "msa", "chunks", "indel_scan", "indel_impute", "pass2", "cnn", "e2e", "caller", "indel_caller"]
    if "snp" in what:
        make_snp_goldens()
    if "cnd" in what:
        make_cnd_pos_goldens()
    if "msa" in what:
        make_msa_goldens()
    if "chunks" in what:
        make_chunk_goldens()
    if "indel_scan" in what:
        make_indel_scan_goldens()
    if "indel_impute" in what:
        make_indel_impute_goldens()
    if "pass2" in what:
        make_pass2_goldens()
    elif "allele_ties" in what:
        make_allele_ties_golden()
    if "cnn" in what:
        make_cnn_goldens()
    if "e2e" in what:
        make_e2e_goldens()
    if "caller" in what:                      # these two replace the reference's model classes by canned tables: last
        make_caller_goldens()
    if "indel_caller" in what:
        make_indel_caller_goldens()

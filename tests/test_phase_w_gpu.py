"""GPU: the phaser's weighted model (csrc/nc_happhase.hip k_hp_dp<*, true>, k_hp_tag<true>, k_hp_quals; nc_snp_phase_set_weights,
nc_snp_phase_weights_from_bam; phase_contig(weighted=True)) against the numpy restatement (tests/phase_w_ref.py) bit for bit -- sides, h, phased,
PS, block costs, outcomes, HP / PS --, against the plain solves where every weight is 1, the qualities and MAPQs read from a small BAM's
record stream against the Python lookup on both allele rules, and through phase_run."""
import gzip
import os

import numpy as np
import pytest

import bamio
from phase_w_ref import continuing, flat_weights, gpu_instances, hand_instance, haplotag_w, phase_w, unit_weights
from test_phase_gpu import _csr, _indels, _reads_of, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _assert_equal(got, reads, weights, ok, pos, groups, max_cov=15, gt=None, G=30):
    ref = phase_w(pos, reads, weights, ok, site_gt=gt, G=G, max_cov=max_cov)
    hp, ps = haplotag_w(reads, weights, groups, ref)
    for k in ("side", "site_block", "site_h", "site_phased", "site_ps") + (("site_gt",) if gt is not None else ()):
        assert np.array_equal(got[k], ref[k]), k
    assert [tuple(int(v) for v in b) for b in zip(got["block_first"], got["block_last"], got["block_ps"], got["block_cost"])] == \
        [tuple(int(v) for v in b) for b in ref["blocks"]]
    assert np.array_equal(got["group_hp"], hp) and np.array_equal(got["group_ps"], ps)
    return ref


@pytest.fixture(scope="module")
def instances():
    return gpu_instances()


@pytest.mark.parametrize("with_gt", [False, True])
def test_kernel_equals_restatement_on_random_weighted_instances(eng, instances, with_gt):  # noqa: F811
    full = small = two = 0
    for t in instances:
        kw = dict(site_gt=t["gt"], distrust_cost=t["G"]) if with_gt else {}
        got = eng.snp_phase(t["pos"], None, t["groups"], int(t["groups"].max()) + 1, max_cov=t["max_cov"], csr=_csr(t["reads"]),
                            weights=(flat_weights(t["weights"]), t["read_ok"]), **kw)
        ref = _assert_equal(got, t["reads"], t["weights"], t["read_ok"], t["pos"], t["groups"], t["max_cov"], t["gt"] if with_gt else None, t["G"])
        assert np.array_equal(got["entry_weight"], flat_weights(t["weights"])) and np.array_equal(got["read_ok"], t["read_ok"])
        assert not got["read_mapq"].any()
        cont = continuing(t["reads"], ref)
        full += sum(n == 15 for n in cont)
        small += sum(n < 10 for n in cont)
        two += sum(l == f + 1 for f, l, _, _ in ref["blocks"])
    # 15 continuing slots (the one-subset-per-thread branch), fewer than 10 (the shared-subset branch), a two-column block
    assert full >= 2 and small >= 10 and two >= 1


def test_hand_instance(eng):  # noqa: F811
    pos, reads, weights = hand_instance()
    groups = np.arange(8, dtype=np.int32)
    got = eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), weights=(flat_weights(weights), None))
    _assert_equal(got, reads, weights, None, pos, groups)
    plain = eng.snp_phase(pos, None, groups, 8, csr=_csr(reads))
    assert got["block_cost"].tolist() == [15] and plain["block_cost"].tolist() == [2]
    assert (got["site_h"][1] ^ got["site_h"][0]) == 0 and (plain["site_h"][1] ^ plain["site_h"][0]) == 1


def test_unit_weights_without_a_floor_are_the_plain_solves(eng, instances):  # noqa: F811
    for t in instances[::3] + instances[-3:]:
        reads, groups = t["reads"], t["groups"]
        ng = int(groups.max()) + 1
        for kw in ({}, dict(site_gt=t["gt"], distrust_cost=2)):
            plain = eng.snp_phase(t["pos"], None, groups, ng, max_cov=t["max_cov"], csr=_csr(reads), **kw)
            for w in ((flat_weights(unit_weights(reads)), np.ones(len(reads), np.uint8)), (None, None)):
                got = eng.snp_phase(t["pos"], None, groups, ng, max_cov=t["max_cov"], csr=_csr(reads), weights=w, **kw)
                assert set(got) == set(plain) | {"entry_weight", "read_mapq", "read_ok"}
                for k in plain:
                    if k != "ms":
                        assert np.array_equal(plain[k], got[k]), k


def test_bad_arguments_are_refused(eng):  # noqa: F811
    from nanocaller_amd import _lib
    pos, reads, weights = hand_instance()
    groups = np.arange(8, dtype=np.int32)
    w = flat_weights(weights)
    bad_w = w.copy()
    bad_w[3] = 94
    for ws in ((bad_w, None), (None, np.full(8, 2, np.uint8))):
        with pytest.raises(_lib.NanoCallerHipError):
            eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), weights=ws)
    for ws in ((w[:-1], None), (None, np.ones(7, np.uint8))):
        with pytest.raises(ValueError):
            eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), weights=ws)
    import torch
    raw = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    rec = torch.zeros(8, dtype=torch.int64, device=eng.device)
    for q in ((raw, rec, -1, 30, 93), (raw, rec, 256, 30, 93), (raw, rec, 20, 94, 93), (raw, rec, 20, 30, 94), (raw, rec, 20, -1, 93)):
        with pytest.raises(_lib.NanoCallerHipError):
            eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), bam_quals=q)
    with pytest.raises(ValueError):
        eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), bam_quals=(raw, rec[:5], 20, 30, 93))
    with pytest.raises(ValueError):
        eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), weights=(w, None), bam_quals=(raw, rec, 20, 30, 93))


# ------------------------------------------------------------------------------------------- k_hp_quals on hand-made records
def _real_cigar(r):
    ops = "MIDNSHP=X"
    return [(ops[v & 15], v >> 4) for v in r["tags"]["CG"]] if "CG" in r.get("tags", {}) else r["cigar"]


def _expected_weights(recs, reads, pos, default_weight=30, w_max=93):
    from phase_w_ref import qual_lookup
    out = []
    for r, rd in zip(recs, reads):
        q = list(r["qual"]) if r.get("qual") is not None else [0xff] * len(r["seq"])
        out += qual_lookup(r["pos0"] + 1, _real_cigar(r), q, [int(pos[s]) for s, _ in rd], default_weight, w_max)
    return np.array(out, np.uint8)


def _hand_records():
    import bamio_w
    rng = np.random.default_rng(5)
    ops = "MIDNSHP=X"

    def rec(name, pos0, cigar, mapq, qual="random", **kw):
        L = sum(n for op, n in cigar if op in "MIS=X")
        q = bytes(rng.integers(0, 94, L, dtype=np.uint8)) if qual == "random" else qual
        return dict(name=name, flag=0, pos0=pos0, cigar=cigar, seq="".join("ACGT"[i] for i in rng.integers(0, 4, L)), mapq=mapq, qual=q, tags={}, **kw)
    many = []                                                            # 151 operations: the walk crosses two chunk borders
    for k in range(50):
        many += [("M", 3 + k % 4), ("I" if k % 2 else "D", 1 + k % 3), ("=", 2)]
    many.append(("X", 4))
    recs = [rec("clips", 99, [("H", 7), ("S", 3), ("M", 5), ("I", 2), ("M", 4), ("D", 3), ("M", 6), ("S", 2), ("H", 2)], 60),
            rec("delfirst", 120, [("D", 2), ("M", 10), ("N", 5), ("P", 3), ("X", 4)], 19),
            rec("noqual", 130, [("M", 20), ("I", 1), ("M", 20)], 20, qual=None),
            dict(name="noseq", flag=0, pos0=140, cigar=[("M", 30), ("D", 4), ("M", 20)], seq="", mapq=0, tags={}),
            rec("many", 150, many, 255),
            rec("hot", 200, [("M", 40)], 21, qual=bytes([200] * 20 + [93] * 20))]
    long_ = rec("longcig", 260, many, 3)
    long_["tags"] = {"XA": "some text", "CG": [(n << 4) | ops.index(op) for op, n in many], "HP": 1}
    long_["cigar"] = [("S", len(long_["seq"])), ("N", bamio_w.ref_span(many))]
    recs.append(long_)
    return recs


def _hand_csr(recs, step=3):
    import bamio_w
    last = max(r["pos0"] + bamio_w.ref_span(_real_cigar(r)) for r in recs)
    pos = np.arange(90, last + 12, step, dtype=np.int32)
    reads = []
    for k, r in enumerate(recs):                                         # every site of the span, and (read 0) two outside it
        a, b = r["pos0"] + 1, r["pos0"] + 1 + bamio_w.ref_span(_real_cigar(r))
        reads.append([(s, (s + k) & 1) for s in range(pos.size) if a <= pos[s] < b or (k == 0 and s in (0, pos.size - 1))])
    return pos, reads


@pytest.mark.parametrize("w_max,default_weight,mapq_min", [(93, 30, 20), (50, 7, 0)])
def test_qualities_of_hand_made_records(eng, w_max, default_weight, mapq_min):  # noqa: F811
    import bamio_w
    import torch
    recs = _hand_records()
    pos, reads = _hand_csr(recs)
    raw, off = bamio_w.record_stream(recs)
    groups = np.arange(len(recs), dtype=np.int32)
    got = eng.snp_phase(pos, None, groups, len(recs), csr=_csr(reads),
                        bam_quals=(torch.from_numpy(raw).to(eng.device), torch.from_numpy(off).to(eng.device), mapq_min, default_weight, w_max))
    want = _expected_weights(recs, reads, pos, default_weight, w_max)
    assert np.array_equal(got["entry_weight"], want)
    mapq = np.array([r["mapq"] for r in recs], np.uint8)
    assert np.array_equal(got["read_mapq"], mapq) and np.array_equal(got["read_ok"], (mapq >= mapq_min).astype(np.uint8))
    # the lookup's cases are all there: a site in a deletion, before the first query base, under the cap, without a quality
    assert (want == default_weight).sum() > 20 and (want == w_max).any() and len(set(want.tolist())) > 30
    weights, k = [], 0
    for rd in reads:
        weights.append(want[k:k + len(rd)].tolist())
        k += len(rd)
    _assert_equal(got, reads, weights, got["read_ok"], pos, groups)


def test_a_record_that_overruns_its_block_size_returns_a_status(eng):  # noqa: F811
    import bamio_w
    import torch
    from nanocaller_amd import _lib
    recs = _hand_records()[:3]
    pos, reads = _hand_csr(recs)
    groups = np.arange(len(recs), dtype=np.int32)
    chunks = [bamio_w.record_bytes(r) for r in recs]
    chunks[1] = bamio_w.record_bytes(recs[1], l_seq=4000)                # l_seq claims more bases and qualities than block_size holds
    off = np.array([0, len(chunks[0]), len(chunks[0]) + len(chunks[1])], np.int64)
    raw = torch.from_numpy(np.frombuffer(b"".join(chunks), np.uint8).copy()).to(eng.device)
    with pytest.raises(_lib.NanoCallerHipError, match="status 4"):
        eng.snp_phase(pos, None, groups, len(recs), csr=_csr(reads), bam_quals=(raw, torch.from_numpy(off).to(eng.device), 20, 30, 93))
    # a record offset whose block would leave the stream
    off[2] = raw.numel() - 20
    with pytest.raises(_lib.NanoCallerHipError, match="status 1"):
        eng.snp_phase(pos, None, groups, len(recs), csr=_csr(reads), bam_quals=(raw[:int(off[1])], torch.from_numpy(off).to(eng.device), 20, 30, 93))


# ------------------------------------------------------------------------------------------- a small BAM
@pytest.fixture(scope="module")
def wbam(tmp_path_factory):
    """a 30 kb, depth-12 world with indel errors beside its het SNPs and soft clips at both ends, written as a BAM with random base qualities
    (every seventh record without), MAPQ spread around 20 and one record whose CIGAR stands in the CG tag; its true SNP calls"""
    import bamio_w
    from nanocaller_amd.phase import het_sites, kept_reads
    from phase_gt_ref import world_calls
    from phase_realign_ref import make_realign_world
    w = make_realign_world(93, length=30_000, depth=12.0)
    d = str(tmp_path_factory.mktemp("weighted"))
    rng = np.random.default_rng(93)
    recs = bamio.world_to_records(w, None)
    ops = "MIDNSHP=X"
    for k, r in enumerate(recs):
        r["tags"] = {}
        r["mapq"] = int(rng.choice([0, 3, 12, 19, 20, 21, 30, 60, 60, 60, 60, 60]))
        r["qual"] = None if k % 7 == 3 else bytes(rng.integers(0, 94, len(r["seq"]), dtype=np.uint8))
    k = next(k for k, r in enumerate(recs) if len(r["cigar"]) > 8 and r["flag"] == 0 and r["mapq"] >= 20 and r["qual"] is not None)
    recs[k]["tags"] = {"CG": [(n << 4) | ops.index(op) for op, n in recs[k]["cigar"]]}
    recs[k]["cigar"] = [("S", len(recs[k]["seq"])), ("N", bamio_w.ref_span(_real_cigar(recs[k])))]
    bam, fa = os.path.join(d, "w.bam"), os.path.join(d, "r.fa")
    bamio_w.write_bam(bam, w.chrom, w.length, recs)
    bamio.write_fasta(fa, w.chrom, w.ref)
    kept = kept_reads(w, False)[0]
    vcf = world_calls(w, kept, third_every=7)
    idx, pos, al, kind = het_sites(vcf, 10)
    return dict(w=w, d=d, bam=bam, fa=fa, recs=recs, kept=kept, vcf=vcf, pos=pos, al=al, longcig=k, rule={})


@pytest.mark.parametrize("realign", [False, True])
def test_small_bam_weights_and_phasing_equal_restatement(wbam, monkeypatch, realign):
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import phase_contig
    from phase_realign_ref import entries
    e = wbam
    monkeypatch.setenv("NC_DEVICE_INGEST", "1")
    release_contig()
    res = phase_contig(e["bam"], e["fa"], e["w"].chrom, e["vcf"], 10, False, realign=realign, weighted=True)
    rule = "realign" if realign else "column"
    if rule not in e["rule"]:
        e["rule"][rule] = entries(e["w"], e["kept"], e["pos"], e["al"], rule)
    reads = e["rule"][rule]
    assert _reads_of(res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]) == reads
    recs = [e["recs"][k] for k in e["kept"].tolist()]
    want = _expected_weights(recs, reads, e["pos"])
    assert np.array_equal(res.reads["entry_weight"], want)
    mapq = np.array([r["mapq"] for r in recs], np.uint8)
    assert np.array_equal(res.reads["mapq"], mapq) and np.array_equal(res.reads["ok"], (mapq >= 20).astype(np.uint8))
    kk = e["kept"].tolist().index(e["longcig"])
    assert len(reads[kk]) >= 2 and 0 < (mapq < 20).sum() < mapq.size and (want == 30).sum() > 10 and len(set(want.tolist())) > 60
    weights, k = [], 0
    for rd in reads:
        weights.append(want[k:k + len(rd)].tolist())
        k += len(rd)
    pos = e["pos"]
    n_groups = int(res.reads["group"].max()) + 1
    g = dict(side=res.reads["side"], site_block=res.sites["block"], site_phased=res.sites["phased"], site_h=res.sites["h"], site_ps=res.sites["ps"],
             block_first=np.searchsorted(pos, [b[0] for b in res.blocks]), block_last=np.searchsorted(pos, [b[1] for b in res.blocks]),
             block_ps=[b[2] for b in res.blocks], block_cost=[b[3] for b in res.blocks],
             group_hp=np.zeros(n_groups, np.uint8), group_ps=np.zeros(n_groups, np.int32))
    g["group_hp"][res.reads["group"]] = res.reads["hp"]
    g["group_ps"][res.reads["group"]] = res.reads["ps"]
    ref = _assert_equal(g, reads, weights, res.reads["ok"], pos, res.reads["group"])
    refused = res.reads["ok"] == 0
    assert (res.reads["side"][refused] == -1).all() and (res.reads["hp"][refused] > 0).sum() > 0     # left out of the MEC, still tagged
    assert ref["site_phased"].sum() > 20
    e.setdefault("res", {})[rule] = res


def test_phase_run_with_phase_weighted(wbam, monkeypatch):
    """mode 'all', phaser='device': with params['phase_weighted'] (and 'phase_mapq') the phased VCF and the haplotag table are
    phase_contig(weighted=True)'s; with the key absent phase_contig never receives `weighted` and the output is weighted=False's"""
    from nanocaller_amd import indelCaller, phase, snpCaller, vcfio
    from nanocaller_amd.generate_SNP_pileups import release_contig
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    for v in ("NC_PHASE_WEIGHTED", "NC_PHASE_DISTRUST", "NC_PHASE_REALIGN", "NC_PHASED_BAM"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("NC_DEVICE_INGEST", "1")
    e = wbam
    w, d = e["w"], e["d"]
    snp_vcf = os.path.join(d, "true.snps.vcf.gz")
    vcfio.write_sorted_vcf(snp_vcf, snpCaller.VCF_HEADER.format(contigs="##contig=<ID=%s>\n" % w.chrom, sample="SAMPLE"), e["vcf"], [w.chrom])
    calls = []
    real = phase.phase_contig

    def spy(*a, **kw):
        calls.append(dict(kw))
        return real(*a, **kw)
    monkeypatch.setattr(phase, "phase_contig", spy)
    f_off, _ = _indels(e["bam"], e["fa"], w.chrom, w.length, os.path.join(d, "off"), "all", snp_vcf, phaser="device")
    assert len(calls) == 1 and not {"weighted", "mapq_min", "default_weight"} & set(calls[0])
    f_on, _ = _indels(e["bam"], e["fa"], w.chrom, w.length, os.path.join(d, "on"), "all", snp_vcf, phaser="device", phase_weighted=True, phase_mapq=25)
    assert len(calls) == 2 and calls[1].get("weighted") is True and calls[1].get("mapq_min") == 25
    release_contig()
    want_on = real(e["bam"], e["fa"], w.chrom, e["vcf"], 10, False, weighted=True, mapq_min=25)
    want_off = real(e["bam"], e["fa"], w.chrom, e["vcf"], 10, False)
    read = lambda p: [ln for ln in gzip.open(p, "rt") if not ln.startswith("#")]   # noqa: E731
    assert sorted(read(f_on["snps"])) == sorted(want_on.records) and sorted(read(f_off["snps"])) == sorted(want_off.records)
    assert want_on.records != want_off.records
    for out, want in (("on", want_on), ("off", want_off)):
        t = np.load(os.path.join(d, out, "intermediate_phase_files", "%s.haplotags.npz" % w.chrom))
        assert all(np.array_equal(t[k], want.haplotags[k]) for k in ("hash", "hp", "ps")) and t["hash"].size > 20
    assert os.path.exists(f_on["indels"])
    # the environment switch, read only without the key
    monkeypatch.setenv("NC_PHASE_WEIGHTED", "1")
    assert phase.phase_weighted_selected({}) and not phase.phase_weighted_selected(dict(phase_weighted=False))


def test_weighted_mode_refuses_the_host_route(wbam, monkeypatch):
    from nanocaller_amd import _lib
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import phase_contig
    e = wbam
    release_contig()
    monkeypatch.setenv("NC_DEVICE_INGEST", "0")
    for realign in (False, True):
        with pytest.raises(_lib.NanoCallerHipError, match="device ingest"):
            phase_contig(e["bam"], e["fa"], e["w"].chrom, e["vcf"], 10, False, realign=realign, weighted=True)
    monkeypatch.setenv("NC_DEVICE_INGEST", "1")
    with pytest.raises(_lib.NanoCallerHipError, match="device ingest"):
        phase_contig(e["w"], None, e["w"].chrom, e["vcf"], 10, False, weighted=True)
    release_contig()

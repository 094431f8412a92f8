"""GPU: the phaser's genotype-aware solve (csrc/nc_happhase.hip k_hp_dp<true>, nc_snp_phase_solve_gt; phase_contig(distrust=True)) against the
numpy restatement (tests/phase_gt_ref.py) bit for bit -- outcomes, h, phased, PS, sides, block costs, HP / PS --, against the plain solve where no
call can be left, on a small BAM on both decode routes and both allele rules, and through phase_run."""
import gzip
import os

import numpy as np
import pytest

import bamio
from phase_gt_ref import edit_calls, hand_instance, hom_ref_columns, phase_gt, world_calls
from phase_realign_ref import entries, make_realign_world
from phase_ref import haplotag, random_instance
from test_phase_gpu import _csr, _indels, _reads_of, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _assert_equal(got, reads, pos, groups, gt, G, max_cov=15):
    ref = phase_gt(pos, reads, gt, G=G, max_cov=max_cov)
    hp, ps = haplotag(reads, groups, ref)
    for k in ("side", "site_block", "site_gt", "site_phased", "site_ps"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["site_h"], ref["site_h"])                  # every column of a block, phased or not
    assert [tuple(int(v) for v in b) for b in zip(got["block_first"], got["block_last"], got["block_ps"], got["block_cost"])] == \
        [tuple(int(v) for v in b) for b in ref["blocks"]]
    assert np.array_equal(got["group_hp"], hp) and np.array_equal(got["group_ps"], ps)
    return ref


def _continuing(reads, ref):
    """per block the largest number of accepted spans that cover two adjacent columns (the continuing set's size)"""
    out = []
    for f, l, _, _ in ref["blocks"]:
        n = [sum(1 for r in np.flatnonzero(ref["accepted"]) if reads[r][0][0] < c <= reads[r][-1][0]) for c in range(f + 1, l + 1)]
        out.append(max(n))
    return out


def _instances():
    rng = np.random.default_rng(4242)
    out = []
    for k in range(48):
        n_sites = int(rng.integers(2, 41))
        n_reads = int(rng.integers(1, 61 if k % 3 == 0 else 14))
        reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=float(rng.choice([0.0, 0.05, 0.2])), max_len=int(rng.integers(2, n_sites + 1)))
        out.append((reads, n_sites, int(rng.choice([15, 15, 6, 2]))))
    # more than 15 reads over every site: every continuing set holds 15 slots
    for n_reads, n_sites in ((20, 6), (33, 11)):
        truth = rng.integers(0, 2, n_sites)
        out.append(([[(s, int(truth[s]) ^ (r & 1) ^ int(rng.random() < 0.15)) for s in range(n_sites)] for r in range(n_reads)], n_sites, 15))
    # the smallest block there is, beside a block whose middle column has no accepted allele.  (A block of ONE column cannot be built: a block is
    # the union of accepted spans, and a span runs from a read's first to its last site, two sites at least -- so two columns it is.)
    out.append(([[(0, 0), (1, 1)], [(3, 0), (5, 0)], [(3, 1), (5, 1)], [(4, 1)]], 6, 15))
    return out, rng


def test_kernel_equals_restatement_on_random_allele_matrices(eng):  # noqa: F811
    inst, rng = _instances()
    full = small = two = bare = left = 0
    for reads, n_sites, max_cov in inst:
        n_reads = len(reads)
        gt = rng.choice([0, 0, 2], n_sites).astype(np.uint8)
        G = int(rng.choice([1, 2, 3]))
        groups = np.unique(rng.integers(0, max(1, n_reads - n_reads // 4), n_reads), return_inverse=True)[1].astype(np.int32)
        pos = np.sort(rng.choice(np.arange(1, 10 * n_sites + 1), n_sites, replace=False)).astype(np.int32)
        got = eng.snp_phase(pos, None, groups, int(groups.max()) + 1, max_cov=max_cov, csr=_csr(reads), site_gt=gt, distrust_cost=G)
        ref = _assert_equal(got, reads, pos, groups, gt, G, max_cov)
        cont = _continuing(reads, ref)
        full += sum(n == 15 for n in cont)
        small += sum(n < 10 for n in cont)
        two += sum(l == f + 1 for f, l, _, _ in ref["blocks"])
        with_allele = {s for r in np.flatnonzero(ref["accepted"]) for s, _ in reads[r]}
        bare += sum(1 for s in range(n_sites) if ref["site_block"][s] >= 0 and s not in with_allele)
        left += int((ref["site_gt"] != gt).sum())
    # 15 continuing slots (the one-subset-per-thread branch), fewer than 10 (the shared-subset branch), a two-column block, a column without
    # an accepted allele, calls that were left
    assert full >= 2 and small >= 10 and two >= 1 and bare >= 1 and left >= 20


def test_hand_instance(eng):  # noqa: F811
    pos, reads, gt = hand_instance()
    groups = np.arange(8, dtype=np.int32)
    got = eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), site_gt=gt, distrust_cost=1)
    _assert_equal(got, reads, pos, groups, gt, 1)
    assert got["site_gt"].tolist() == [0, 0, 0, 1, 0] and got["block_cost"].tolist() == [3]
    assert got["site_phased"].tolist() == [True, True, True, False, True] and got["block_ps"].tolist() == [100]
    assert (got["group_hp"][:4] == got["group_hp"][0]).all() and (got["group_hp"][4:] == 3 - got["group_hp"][0]).all() and got["group_hp"][0] in (1, 2)
    # the defaults: G = 1
    assert np.array_equal(eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), site_gt=gt)["site_gt"], got["site_gt"])


def test_no_call_can_be_left_is_the_plain_solve(eng):  # noqa: F811
    """every site called het and G = 16: a column's het cost is 7 at most (15 reads), so no homozygous outcome can win, and every array is the
    plain nc_snp_phase_solve's on the same CSR"""
    inst, rng = _instances()
    for reads, n_sites, max_cov in inst[::3] + inst[-3:]:
        groups = np.arange(len(reads), dtype=np.int32)
        pos = (np.arange(n_sites, dtype=np.int32) + 1) * 7
        plain = eng.snp_phase(pos, None, groups, groups.size, max_cov=max_cov, csr=_csr(reads))
        got = eng.snp_phase(pos, None, groups, groups.size, max_cov=max_cov, csr=_csr(reads), site_gt=np.zeros(n_sites, np.uint8), distrust_cost=16)
        assert "site_gt" not in plain and not got["site_gt"].any()
        for k in plain:
            if k != "ms":
                assert np.array_equal(plain[k], got[k]), k


def test_bad_arguments_are_refused(eng):  # noqa: F811
    from nanocaller_amd import _lib
    pos, reads, gt = hand_instance()
    groups = np.arange(8, dtype=np.int32)
    for kw in (dict(site_gt=gt, distrust_cost=0), dict(site_gt=gt, distrust_cost=5000), dict(site_gt=np.full(5, 3, np.uint8))):
        with pytest.raises(_lib.NanoCallerHipError):
            eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), **kw)
    with pytest.raises(ValueError):
        eng.snp_phase(pos, None, groups, 8, csr=_csr(reads), site_gt=gt[:3])


# ------------------------------------------------------------------------------------------- a small BAM
@pytest.fixture(scope="module")
def edited(tmp_path_factory):
    """a 100 kb world with indel errors beside its het SNPs, written as a BAM; its true calls (0/1, some 1/2, 1/1) with a fifth of the het 0/1
    rewritten to 1/1 and a false 0/1 about every 2.5 kb where both haplotypes carry the reference base"""
    from nanocaller_amd.phase import distrust_sites, kept_reads
    w = make_realign_world(31, length=100_000)
    d = str(tmp_path_factory.mktemp("distrust"))
    recs = bamio.world_to_records(w, None)
    bam, fa = os.path.join(d, "untagged.bam"), os.path.join(d, "r.fa")
    bamio.write_bam(bam, w.chrom, w.length, [dict(r, tags={}) for r in recs], write_csi=True)
    bamio.write_fasta(fa, w.chrom, w.ref)
    kept = kept_reads(w, False)[0]
    rng = np.random.default_rng(31)
    calls = world_calls(w, kept, third_every=7)
    cols, alt_of = hom_ref_columns(w, [], 2_500, rng)
    vcf, to_hom, added = edit_calls(calls, w.het_sites, cols, rng, share_hom=0.2, alt_of=alt_of)
    idx, pos, al, kind, gt = distrust_sites(vcf, 10)
    assert len(to_hom) >= 10 and len(added) >= 20 and "1/2" in kind and (gt == 2).sum() > len(to_hom)
    return dict(w=w, d=d, bam=bam, fa=fa, kept=kept, vcf=vcf, to_hom=to_hom, added=added, idx=idx, pos=pos, al=al, kind=kind, gt=gt, rule={})


@pytest.mark.parametrize("realign", [False, True])
@pytest.mark.parametrize("ingest", ["0", "1"])
def test_small_bam_equals_restatement(edited, monkeypatch, ingest, realign):
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import distrust_record, phase_contig
    e = edited
    monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
    release_contig()
    res = phase_contig(e["bam"], e["fa"], e["w"].chrom, e["vcf"], 10, False, realign=realign, distrust=True)
    if realign:
        assert bool(gip._DEV_INGEST) == (ingest == "1")
    rule = "realign" if realign else "column"
    if rule not in e["rule"]:
        e["rule"][rule] = entries(e["w"], e["kept"], e["pos"], e["al"], rule)
    reads = e["rule"][rule]
    assert _reads_of(res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]) == reads
    pos = e["pos"]
    assert np.array_equal(res.sites["pos"], pos) and np.array_equal(res.sites["gt_in"], e["gt"]) and np.array_equal(res.sites["record"], e["idx"])
    n_groups = int(res.reads["group"].max()) + 1
    g = dict(side=res.reads["side"], site_block=res.sites["block"], site_phased=res.sites["phased"], site_h=res.sites["h"], site_ps=res.sites["ps"],
             site_gt=res.sites["gt_out"], block_first=np.searchsorted(pos, [b[0] for b in res.blocks]),
             block_last=np.searchsorted(pos, [b[1] for b in res.blocks]), block_ps=[b[2] for b in res.blocks], block_cost=[b[3] for b in res.blocks],
             group_hp=np.zeros(n_groups, np.uint8), group_ps=np.zeros(n_groups, np.int32))
    g["group_hp"][res.reads["group"]] = res.reads["hp"]
    g["group_ps"][res.reads["group"]] = res.reads["ps"]
    ref = _assert_equal(g, reads, pos, res.reads["group"], e["gt"], 1)
    # the records: the restatement's outcomes written by the rows of the record rule
    want = list(e["vcf"])
    for k, i in enumerate(e["idx"].tolist()):
        want[i] = distrust_record(e["vcf"][i], e["kind"][k], int(ref["site_gt"][k]), int(ref["site_h"][k]), bool(ref["site_phased"][k]), int(ref["site_ps"][k]))
    assert res.records == want
    at = {int(p): k for k, p in enumerate(pos.tolist())}
    back = sum(ref["site_gt"][at[p]] == 0 and ref["site_phased"][at[p]] for p in e["to_hom"])
    gone = sum(ref["site_gt"][at[p]] == 1 for p in e["added"])
    print("%s, ingest %s: %d of %d rewritten het calls back to het, %d of %d false het calls out as 0/0" % (rule, ingest, back, len(e["to_hom"]), gone, len(e["added"])))
    assert back > 0 and gone > 0


def test_phase_run_with_distrust(edited, monkeypatch):
    """mode 'all', phaser='device': with params['phase_distrust'] the phased VCF is phase_contig(distrust=True)'s records without the 0/0 ones,
    the haplotag table is that call's and the indel pass runs from it; with the key absent phase_contig never receives `distrust`"""
    from nanocaller_amd import indelCaller, phase, snpCaller, vcfio
    from nanocaller_amd.generate_SNP_pileups import release_contig
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    for v in ("NC_PHASE_DISTRUST", "NC_PHASE_REALIGN", "NC_PHASED_BAM"):
        monkeypatch.delenv(v, raising=False)
    e = edited
    w, d = e["w"], e["d"]
    snp_vcf = os.path.join(d, "edited.snps.vcf.gz")
    vcfio.write_sorted_vcf(snp_vcf, snpCaller.VCF_HEADER.format(contigs="##contig=<ID=%s>\n" % w.chrom, sample="SAMPLE"), e["vcf"], [w.chrom])
    calls = []
    real = phase.phase_contig

    def spy(*a, **kw):
        calls.append(dict(kw))
        return real(*a, **kw)
    monkeypatch.setattr(phase, "phase_contig", spy)
    f_off, _ = _indels(e["bam"], e["fa"], w.chrom, w.length, os.path.join(d, "off"), "all", snp_vcf, phaser="device")
    assert len(calls) == 1 and "distrust" not in calls[0] and "distrust_cost" not in calls[0]
    f_on, ind = _indels(e["bam"], e["fa"], w.chrom, w.length, os.path.join(d, "on"), "all", snp_vcf, phaser="device", phase_distrust=True)
    assert len(calls) == 2 and calls[1].get("distrust") is True
    release_contig()
    want = real(e["bam"], e["fa"], w.chrom, e["vcf"], 10, False, distrust=True)
    gt_of = lambda ln: ln.split("\t")[9].split(":")[0]                     # noqa: E731
    dropped = [ln for ln in want.records if gt_of(ln) == "0/0"]
    out = [ln for ln in gzip.open(f_on["snps"], "rt") if not ln.startswith("#")]
    assert len(dropped) > 0 and sorted(out) == sorted(ln for ln in want.records if gt_of(ln) != "0/0")
    plain = [ln for ln in gzip.open(f_off["snps"], "rt") if not ln.startswith("#")]
    assert len(plain) == len(e["vcf"]) and len(out) == len(e["vcf"]) - len(dropped)
    t = np.load(os.path.join(d, "on", "intermediate_phase_files", "%s.haplotags.npz" % w.chrom))
    assert all(np.array_equal(t[k], want.haplotags[k]) for k in ("hash", "hp", "ps")) and t["hash"].size > 100
    assert os.path.exists(f_on["indels"])

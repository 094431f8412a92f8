"""CPU: the restatement of the phaser's genotype-aware solve (tests/phase_gt_ref.py) against an exhaustive search and a hand-provable
instance, and the host helpers of the distrust mode: the site list, the records' GT rewriting, the 0/0 drop of phase_run."""
import numpy as np
import pytest

from phase_gt_ref import exhaustive_cost, hand_instance, phase_gt
from phase_ref import phase, random_instance


@pytest.mark.parametrize("G", [1, 2, 3])
def test_restatement_reaches_the_exhaustive_minimum(G):
    rng = np.random.default_rng(500 + G)
    changed = n_hom_in = 0
    for k in range(300):
        n_sites = int(rng.integers(1, 7))
        n_reads = int(rng.integers(1, 11)) if k % 2 else int(rng.integers(7, 11))      # (every other instance deep and full length: calls get left)
        reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=float(rng.choice([0.0, 0.15, 0.35])),
                                      max_len=int(rng.integers(1, n_sites + 1)) if k % 2 else n_sites)
        gt = rng.choice([0, 0, 2, 1], n_sites).astype(np.uint8)
        if k % 3 == 0:                                                   # a site every read agrees on, called het: a false het call
            s = int(rng.integers(0, n_sites))
            reads = [[(t, 0 if t == s else a) for t, a in rd] for rd in reads]
            gt[s] = 0
        pos = np.arange(1, n_sites + 1) * 100
        res = phase_gt(pos, reads, gt, G=G)
        assert sum(b[3] for b in res["blocks"]) == exhaustive_cost(reads, res["accepted"], n_sites, gt, G)
        # the recorded outcomes and orientations pay exactly the block costs
        paid = 0
        for s in range(n_sites):
            if res["site_block"][s] < 0:
                assert res["site_gt"][s] == gt[s] and not res["site_phased"][s]
                continue
            al = [(a, res["side"][r]) for r, rd in enumerate(reads) if res["side"][r] >= 0 for t, a in rd if t == s]
            o = int(res["site_gt"][s])
            err = sum(a != (int(res["site_h"][s]) ^ sd) for a, sd in al) if o == 0 else sum(a != o - 1 for a, _ in al)
            paid += err + (0 if o == gt[s] else G)
        assert paid == sum(b[3] for b in res["blocks"])
        changed += int((res["site_gt"] != gt).sum())
        n_hom_in += int((gt != 0).sum())
    assert changed >= 3 and n_hom_in > 50                               # (the instances do leave their calls: 83 / 24 / 5 sites)


def test_every_site_het_and_a_prohibitive_price_is_the_plain_phaser():
    rng = np.random.default_rng(9)
    for _ in range(40):
        n_sites = int(rng.integers(2, 12))
        reads, _, _ = random_instance(rng, int(rng.integers(2, 14)), n_sites, p_err=0.2, max_len=n_sites)
        pos = np.arange(1, n_sites + 1) * 10
        a, b = phase(pos, reads), phase_gt(pos, reads, np.zeros(n_sites, np.uint8), G=16)
        for k in ("accepted", "side", "site_block", "site_phased", "site_ps"):
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["site_h"], b["site_h"]) and a["blocks"] == b["blocks"] and not b["site_gt"].any()


def test_hand_instance():
    """site 2 (called 1/1, alleles split by haplotype): het costs 0 + G, homB 4, homA 4 + G -> het for G < 4.  Site 3 (called 0/1, 7 reads on the
    first allele, read 7 on the second): het costs 3 (reads 4-6 against their haplotype), homA 1 + G -> homA for G = 1."""
    pos, reads, gt = hand_instance()
    res = phase_gt(pos, reads, gt, G=1)
    assert res["accepted"].all() and res["blocks"] == [(0, 4, 100, 1 + 2)]
    assert res["site_gt"].tolist() == [0, 0, 0, 1, 0]
    assert res["site_phased"].tolist() == [True, True, True, False, True]
    assert res["site_ps"].tolist() == [100, 100, 100, 0, 100]
    assert len(set(res["side"][:4].tolist())) == 1 and len(set(res["side"][4:].tolist())) == 1 and res["side"][0] != res["side"][4]
    assert res["site_h"][[0, 1, 2, 4]].tolist() == [int(res["side"][0])] * 4
    assert exhaustive_cost(reads, res["accepted"], 5, gt, 1) == 3


# ------------------------------------------------------------------------------------------- host helpers
RECS = ["c\t100\t.\tA\tG\t30.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t0/1:30:0.5\n",
        "c\t150\t.\tC\tT\t5.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/1:30:0.5\n",            # below phase_qual_score
        "c\t200\t.\tT\tA,C\t40.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/2:30:0.5\n",
        "c\t300\t.\tG\tC\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/1:30:0.9\n",             # homozygous: taken, alleles REF, ALT
        "c\t350\t.\tG\tC,T\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/1:30:0.9\n",           # two ALTs on a 1/1: not taken
        "c\t400\t.\tAT\tA\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/1:30:0.5\n",            # not a SNP
        "c\t500\t.\tA\tT\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t0/0:30:0.5\n"]             # never a site


def test_distrust_sites():
    from nanocaller_amd.phase import distrust_sites, het_sites
    idx, pos, al, kind, gt = distrust_sites(RECS, 10)
    assert idx.tolist() == [0, 2, 3] and pos.tolist() == [100, 200, 300] and al.tolist() == [[0, 1], [0, 3], [1, 3]]
    assert kind == ["0/1", "1/2", "1/1"] and gt.tolist() == [0, 0, 2] and gt.dtype == np.uint8
    assert het_sites(RECS, 10)[0].tolist() == [0, 2]                      # unchanged
    assert distrust_sites(RECS, 60)[0].size == 0


def _gt(line):
    return line.split("\t")[9].split(":")[0]


def test_distrust_record_rows():
    from nanocaller_amd.phase import distrust_record
    r01, r12, r11 = RECS[0], RECS[2], RECS[3]
    tail = lambda ln: ln.split("\t")[:8]                                  # noqa: E731
    # outcome het, phased
    assert distrust_record(r01, "0/1", 0, 0, True, 100) == "c\t100\t.\tA\tG\t30.000\tPASS\tPR=1;FQ=0\tGT:DP:VF:PS\t0|1:30:0.5:100\n"
    assert _gt(distrust_record(r01, "0/1", 0, 1, True, 100)) == "1|0"
    assert distrust_record(r12, "1/2", 0, 0, True, 100).split("\t")[9] == "1|2:30:0.5:100\n"
    assert _gt(distrust_record(r12, "1/2", 0, 1, True, 100)) == "2|1"
    assert distrust_record(r11, "1/1", 0, 0, True, 100) == "c\t300\t.\tG\tC\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF:PS\t0|1:30:0.9:100\n"
    assert distrust_record(r11, "1/1", 0, 1, True, 100).split("\t")[8:] == ["GT:DP:VF:PS", "1|0:30:0.9:100\n"]
    # outcome het without an accepted allele, or the called class kept: the record as it was
    assert distrust_record(r01, "0/1", 0, 0, False, 0) == r01 and distrust_record(r12, "1/2", 0, 1, False, 0) == r12
    assert distrust_record(r11, "1/1", 2, 0, False, 0) == r11
    # homozygous outcomes: only the GT subfield changes, no PS
    for rec, kind, o, want in ((r01, "0/1", 2, "1/1"), (r01, "0/1", 1, "0/0"), (r12, "1/2", 1, "1/1"), (r12, "1/2", 2, "2/2"), (r11, "1/1", 1, "0/0")):
        got = distrust_record(rec, kind, o, 1, False, 0)
        assert _gt(got) == want and tail(got) == tail(rec) and got.split("\t")[8] == "GT:DP:VF" and got.split("\t")[9].split(":")[1:] == rec.split("\t")[9].split(":")[1:]


def test_phase_run_drops_hom_ref_records():
    from nanocaller_amd.indelCaller import without_hom_ref
    from nanocaller_amd.phase import distrust_record, phase_distrust_selected
    recs = [distrust_record(RECS[0], "0/1", 1, 0, False, 0), RECS[2], distrust_record(RECS[3], "1/1", 1, 0, False, 0), RECS[3],
            distrust_record(RECS[0], "0/1", 0, 1, True, 100)]
    assert without_hom_ref(recs) == [recs[1], recs[3], recs[4]]
    assert phase_distrust_selected({"phase_distrust": 1}) and not phase_distrust_selected({"phase_distrust": 0})


def test_distrust_switch(monkeypatch):
    from nanocaller_amd.phase import phase_distrust_selected
    monkeypatch.delenv("NC_PHASE_DISTRUST", raising=False)
    assert not phase_distrust_selected({})
    monkeypatch.setenv("NC_PHASE_DISTRUST", "1")
    assert phase_distrust_selected({}) and not phase_distrust_selected({"phase_distrust": False})


def _fake_phase_contig(seen):
    def fake(sam_path, fasta_path, chrom, snp_records, phase_qual_score, supplementary=False, device=0, **kw):
        from nanocaller_amd.phase import PhaseResult, distrust_record, distrust_sites
        seen.append(dict(kw))
        recs = list(snp_records)
        idx = distrust_sites(snp_records, phase_qual_score)[0].tolist()
        if kw.get("distrust"):
            for i in idx[:3]:
                recs[i] = distrust_record(recs[i], "0/1", 1, 0, False, 0)  # three calls come out 0/0
        tags = dict(hash=np.zeros(0, np.uint64), hp=np.zeros(0, np.uint8), ps=np.zeros(0, np.int32))
        return PhaseResult(records=recs, blocks=[], haplotags=tags)
    return fake


@pytest.mark.parametrize("on", [False, True])
def test_phase_run_passes_the_switch_and_drops_hom_ref(tmp_path, monkeypatch, on):
    """phase_run with the device phaser stubbed: `distrust` reaches phase_contig only with params['phase_distrust'], and then the phased VCF
    lacks exactly the records that came out 0/0"""
    import gzip
    import queue

    from nanocaller_amd import indelCaller, phase, snpCaller, vcfio
    monkeypatch.delenv("NC_PHASE_DISTRUST", raising=False)
    monkeypatch.delenv("NC_PHASE_REALIGN", raising=False)
    monkeypatch.delenv("NC_PHASED_BAM", raising=False)
    seen = []
    monkeypatch.setattr(phase, "phase_contig", _fake_phase_contig(seen))
    d = str(tmp_path)
    snp_vcf = d + "/s.vcf.gz"
    hdr = snpCaller.VCF_HEADER.format(contigs="##contig=<ID=chr1>\n", sample="S")
    lines = ["chr1\t%d\t.\tA\tG\t30.000\tPASS\tPR=0.1;FQ=0.5\tGT:DP:VF\t0/1:30:0.5\n" % p for p in range(500, 5000, 500)]
    vcfio.write_sorted_vcf(snp_vcf, hdr, lines, ["chr1"])
    params = dict(intermediate_phase_files_dir=d, snp_vcf=snp_vcf, sam_path="in.bam", fasta_path="x.fa", phase_qual_score=10, mode="snps", phaser="device")
    if on:
        params["phase_distrust"] = True
    files = []
    indelCaller.phase_run(dict(name="chr1", ploidy="diploid", start=1, end=6000), params, {}, queue.Queue(), queue.Queue(), files)
    assert seen == [dict(distrust=True)] if on else seen == [{}]
    got = [ln for ln in gzip.open(d + "/chr1.snps.phased.vcf.gz", "rt") if not ln.startswith("#")]
    assert got == (lines[3:] if on else lines)

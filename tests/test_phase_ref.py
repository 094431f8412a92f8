"""CPU: the restatement of the read-based phaser (tests/phase_ref.py) against a brute-force MEC search, the phased-VCF text of
phase_run, and the plumbing of the device phaser through phase_run / call_manager (phaser monkeypatched: no GPU)."""
import os

import numpy as np
import pytest

from phase_ref import brute_force_mec, haplotag, mec_cost, phase, random_instance


def _cases():
    rng = np.random.default_rng(2026)
    out = []
    for k in range(220):
        n_reads = int(rng.integers(1, 13))
        n_sites = int(rng.integers(1, 14))
        reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=float(rng.choice([0.0, 0.1, 0.3])), max_len=int(rng.integers(1, n_sites + 1)))
        out.append((reads, n_sites))
    # slot reuse in one column: a read ends at column 2, the next starts at 3 while a third spans both
    out.append(([[(0, 0), (2, 1)], [(3, 0), (5, 1)], [(0, 1), (5, 0)], [(1, 1), (4, 1)]], 6))
    # single-site coverage only between blocks, a column without informative reads inside a block
    out.append(([[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(3, 0)], [(4, 0), (7, 1)], [(4, 1), (7, 0)]], 9))
    return out


@pytest.mark.parametrize("max_cov", [15, 3])
def test_restatement_reaches_brute_force_mec(max_cov):
    n_reuse = n_single = n_gap = 0
    for reads, n_sites in _cases():
        pos = np.arange(1, n_sites + 1) * 100
        res = phase(pos, reads, max_cov=max_cov)
        acc = res["accepted"]
        assert brute_force_mec(reads, acc, n_sites) == sum(b[3] for b in res["blocks"])
        assert mec_cost(reads, res["site_h"], res["side"]) == sum(b[3] for b in res["blocks"])
        for f, l, ps, _ in res["blocks"]:
            ph = [s for s in range(f, l + 1) if res["site_phased"][s]]
            assert ps == pos[ph[0]]
            n_gap += len(ph) < l - f + 1
        n_single += sum(1 for r in reads if len(r) == 1)
        spans = [(r[0][0], r[-1][0]) for r, a in zip(reads, acc) if a]
        n_reuse += any(b1 + 1 == a2 for (_, b1) in spans for (a2, _) in spans)
        if max_cov == 3:
            cov = np.zeros(n_sites, int)
            for a, b in spans:
                cov[a:b + 1] += 1
            assert cov.max(initial=0) <= 3
    assert n_reuse > 10 and n_single > 10 and n_gap > 0


def test_haplotags_follow_scores():
    reads = [[(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (2, 1)], [(0, 0), (1, 0)], [(1, 1)], [(0, 1), (2, 0)], [(5, 0)]]
    pos = np.array([10, 20, 30, 40, 50, 60])
    res = phase(pos, reads)
    assert res["site_phased"][:3].all() and not res["site_phased"][3:].any()
    # groups: read 4's two alleles disagree with each other -> untagged; read 3 and read 2 share a name
    hp, ps = haplotag(reads, [0, 1, 2, 2, 3, 4], res)
    h1 = 1 if res["site_h"][0] == 0 else 2
    assert hp[0] == h1 and hp[1] == 3 - h1 and hp[2] == h1 and hp[3] == 0 and hp[4] == 0
    assert ps[0] == ps[1] == ps[2] == 10 and ps[3] == 0


# ------------------------------------------------------------------------------------------- phased VCF text, phase_run plumbing
def test_phased_vcf_text():
    from nanocaller_amd.indelCaller import _with_phase_format
    from nanocaller_amd.phase import het_sites, phased_record
    recs = ["c\t100\t.\tA\tG\t30.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t0/1:30:0.5\n",
            "c\t150\t.\tC\tT\t5.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t0/1:30:0.5\n",          # below phase_qual_score
            "c\t200\t.\tT\tA,C\t40.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/2:30:0.5\n",
            "c\t300\t.\tG\tC\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t1/1:30:0.9\n",           # homozygous
            "c\t400\t.\tAT\tA\t50.000\tPASS\tPR=1;FQ=0\tGT:DP:VF\t0/1:30:0.5\n"]          # not a SNP
    idx, pos, al, kind = het_sites(recs, 10)
    assert idx.tolist() == [0, 2] and pos.tolist() == [100, 200] and al.tolist() == [[0, 1], [0, 3]] and kind == ["0/1", "1/2"]
    assert phased_record(recs[0], 0, 100) == "c\t100\t.\tA\tG\t30.000\tPASS\tPR=1;FQ=0\tGT:DP:VF:PS\t0|1:30:0.5:100\n"
    assert phased_record(recs[0], 1, 100) == "c\t100\t.\tA\tG\t30.000\tPASS\tPR=1;FQ=0\tGT:DP:VF:PS\t1|0:30:0.5:100\n"
    assert phased_record(recs[2], 0, 100).split("\t")[9] == "1|2:30:0.5:100\n"
    assert phased_record(recs[2], 1, 100).split("\t")[9] == "2|1:30:0.5:100\n"
    hdr = "##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    h2 = _with_phase_format(hdr)
    assert h2.split("\n")[-3].startswith("##FORMAT=<ID=PS,") and _with_phase_format(h2) == h2


def test_name_hash_is_the_bam_records_fnv1a():
    from nanocaller_amd.phase import name_hash

    def fnv(b):
        h = 1469598103934665603
        for c in b + b"\0":
            h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
        return h
    names = ["r0000001", "read/2", "x", "a" * 80]
    assert name_hash(names).tolist() == [fnv(n.encode()) for n in names]


def test_phaser_switch():
    from nanocaller_amd.phase import device_phaser_selected
    env = os.environ.pop("NC_PHASER", None)
    try:
        assert not device_phaser_selected({}) and device_phaser_selected({"phaser": "device"})
        os.environ["NC_PHASER"] = "device"
        assert device_phaser_selected({}) and not device_phaser_selected({"phaser": "whatshap"})
    finally:
        os.environ.pop("NC_PHASER", None)
        if env is not None:
            os.environ["NC_PHASER"] = env


def _fake_phase_contig(sam_path, fasta_path, chrom, snp_records, phase_qual_score, supplementary=False, max_cov=15, device=0):
    from nanocaller_amd.phase import PhaseResult, het_sites, phased_record
    idx, pos, _, _ = het_sites(snp_records, phase_qual_score)
    recs = list(snp_records)
    for k, i in enumerate(idx.tolist()[:10]):
        recs[i] = phased_record(recs[i], k & 1, int(pos[0]))
    tags = dict(hash=np.array([7, 9], np.uint64), hp=np.array([1, 2], np.uint8), ps=np.array([int(pos[0])] * 2, np.int32))
    return PhaseResult(records=recs, blocks=[(int(pos[0]), int(pos[9]), int(pos[0]), 0)], haplotags=tags)


def _plumbing_params(tmpdir, **kw):
    from nanocaller_amd import snpCaller, vcfio
    from nanocaller_amd.utils import get_chunks
    regions = [("chr1", 1, 40_000, "diploid"), ("chrX", 1, 5_000, "haploid")]          # (two ranks: rank 1 gets part of chr1)
    snp_vcf = os.path.join(tmpdir, "s.snps.vcf.gz")
    if not os.path.exists(snp_vcf):
        hdr = snpCaller.VCF_HEADER.format(contigs="##contig=<ID=chr1>\n##contig=<ID=chrX>\n", sample="SAMPLE")
        lines = ["%s\t%d\t.\tA\tG\t%.3f\tPASS\tPR=0.1;FQ=0.5\tGT:DP:VF\t0/1:30:0.5\n" % (c, p, 20 + p % 7) for c in ("chr1", "chrX")
                 for p in range(500, 19_000, 700)]
        vcfio.write_sorted_vcf(snp_vcf, hdr, lines, ["chr1", "chrX"])
    return dict(chunks_list=get_chunks(regions, 2, max_chunk_size=2_500), mode="all", snp_vcf=snp_vcf, regions_list=regions, sam_path="in.bam",
                fasta_path="x.fa", vcf_path=tmpdir, prefix="t", sample="S", phase_qual_score=10, suppress_progress=True, verbose=False,
                enable_whatshap=False, cpu=2, **kw)


def _plumbing_run(tmpdir, rank, **kw):
    from nanocaller_amd import indelCaller, phase
    seen = []

    def fake_indel_run(params, indel_dict, job_Q, counter_Q, files, device=0, worker_id=1, aligner=None):
        path = os.path.join(params["intermediate_indel_files_dir"], "%s.%d.indel.vcf" % (params["prefix"], worker_id))
        files.append(path)
        open(path, "a").close()
        while not job_Q.empty():
            kind, chunk = job_Q.get()
            seen.append((chunk["chrom"], chunk["start"], chunk["sam_path"], chunk.get("haplotags")))
            counter_Q.put(1)
    indelCaller.indel_run = fake_indel_run
    indelCaller._whatshap_available = lambda: False
    phase.phase_contig = _fake_phase_contig
    out = indelCaller.call_manager(_plumbing_params(tmpdir, **kw))
    with open(os.path.join(tmpdir, "plog.%d" % rank), "w") as f:
        f.write(repr((out, seen)))
    return out, seen


def _plumbing_worker(rank, world, port, tmpdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.is_available = lambda: True
    torch.cuda.device_count = lambda: 8
    _plumbing_run(tmpdir, rank, phaser="device")
    dist.destroy_process_group()


def test_device_phaser_haplotags_reach_every_ranks_chunks(tmp_path):
    """call_manager(mode='all') with phaser='device' over a gloo world of 2 (phaser stubbed): rank 0 phases, every rank's diploid chunks
    carry chunk['haplotags'] = <contig>.haplotags.npz beside the input BAM, the phased SNP file has GT '|' + PS and declares PS"""
    import gzip
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_plumbing_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    logs = [eval(open(os.path.join(str(tmp_path), "plog.%d" % r)).read()) for r in range(2)]
    tags = os.path.join(str(tmp_path), "intermediate_phase_files", "chr1.haplotags.npz")
    assert os.path.exists(tags)
    for out, seen in logs:
        assert seen and all(sp == "in.bam" for (_, _, sp, _) in seen)
        assert all(t == (tags if c == "chr1" else None) for (c, _, _, t) in seen)
    assert {c for lg in logs for (c, _, _, _) in lg[1]} == {"chr1", "chrX"}
    assert any(c == "chr1" for (c, _, _, _) in logs[1][1])
    snps = [ln for ln in gzip.open(logs[0][0]["snps"], "rt")]
    assert any(ln.startswith("##FORMAT=<ID=PS,") for ln in snps)
    ph = [ln for ln in snps if not ln.startswith("#") and "|" in ln.split("\t")[9]]
    assert len(ph) == 10 and all(ln.split("\t")[8].endswith(":PS") for ln in ph)
    from nanocaller_amd.phase import load_haplotags
    h, hp, ps = load_haplotags(tags)
    assert h.tolist() == [7, 9] and hp.tolist() == [1, 2]


def test_switch_unset_leaves_chunks_untagged(tmp_path, monkeypatch):
    monkeypatch.delenv("NC_PHASER", raising=False)
    from nanocaller_amd import indelCaller, phase
    for name in ("indel_run", "_whatshap_available"):
        monkeypatch.setattr(indelCaller, name, getattr(indelCaller, name))      # restored after the test
    monkeypatch.setattr(phase, "phase_contig", phase.phase_contig)
    out, seen = _plumbing_run(str(tmp_path), 0)
    assert seen and all(t is None for (_, _, _, t) in seen)
    assert not any(f.endswith(".haplotags.npz") for f in os.listdir(os.path.join(str(tmp_path), "intermediate_phase_files")))
    import gzip
    assert not any("|" in ln for ln in gzip.open(out["snps"], "rt") if not ln.startswith("#"))

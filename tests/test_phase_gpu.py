"""GPU: the read-based phaser and haplotagger (csrc/nc_happhase.hip, nanocaller_amd/phase.py) against the numpy restatement
(tests/phase_ref.py) bit for bit, against the truth of synthetic worlds, and the indel pass on haplotags instead of BAM tags."""
import gzip
import os

import numpy as np
import pytest

import bamio
from phase_ref import haplotag, phase, random_instance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


def _csr(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    site = np.array([s for r in reads for s, _ in r], np.int32)
    al = np.array([a for r in reads for _, a in r], np.uint8)
    return off, site, al


def _reads_of(off, site, al):
    return [list(zip(site[off[r]:off[r + 1]].tolist(), al[off[r]:off[r + 1]].tolist())) for r in range(len(off) - 1)]


def _assert_equal_to_restatement(got, reads, pos, groups, max_cov):
    ref = phase(pos, reads, max_cov=max_cov)
    hp, ps = haplotag(reads, groups, ref)
    assert np.array_equal(got["side"], ref["side"])
    assert np.array_equal(got["site_block"], ref["site_block"])
    assert np.array_equal(got["site_phased"], ref["site_phased"])
    assert np.array_equal(got["site_h"][ref["site_phased"]], ref["site_h"][ref["site_phased"]])
    assert np.array_equal(got["site_ps"], ref["site_ps"])
    assert [tuple(int(v) for v in b) for b in zip(got["block_first"], got["block_last"], got["block_ps"], got["block_cost"])] == \
        [tuple(int(v) for v in b) for b in ref["blocks"]]
    assert np.array_equal(got["group_hp"], hp) and np.array_equal(got["group_ps"], ps)
    return ref


def test_kernel_equals_restatement_on_random_allele_matrices(eng):
    rng = np.random.default_rng(77)
    full = 0
    for k in range(60):
        n_sites = int(rng.integers(2, 40))
        n_reads = int(rng.integers(1, 60 if k % 3 == 0 else 14))
        reads, _, _ = random_instance(rng, n_reads, n_sites, p_err=float(rng.choice([0.0, 0.05, 0.2])), max_len=int(rng.integers(2, n_sites + 1)))
        max_cov = int(rng.choice([15, 15, 6, 2]))
        groups = rng.integers(0, max(1, n_reads - n_reads // 4), n_reads)          # some names shared by several alignments
        groups = np.unique(groups, return_inverse=True)[1].astype(np.int32)
        pos = np.sort(rng.choice(np.arange(1, 10 * n_sites + 1), n_sites, replace=False)).astype(np.int32)
        got = eng.snp_phase(pos, None, groups, int(groups.max()) + 1, max_cov=max_cov, csr=_csr(reads))
        ref = _assert_equal_to_restatement(got, reads, pos, groups, max_cov)
        acc = np.flatnonzero(ref["accepted"])
        cov = np.zeros(n_sites, int)
        for r in acc:
            cov[reads[r][0][0]:reads[r][-1][0] + 1] += 1
        full += max_cov == 15 and cov.max(initial=0) == 15
    assert full >= 3                                                     # columns with all 15 slots active


@pytest.fixture(scope="module")
def contig(eng, tmp_path_factory):
    """a 2 Mb ONT-like 30x world with its reads' HP tags absent, SNPs called by snpCaller, then phased"""
    from nanocaller_amd import snpCaller
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import phase_contig
    from nanocaller_amd.synth import make_world
    from nanocaller_amd.utils import get_chunks
    release_contig()
    w = make_world(seed=2026, length=2_000_000, depth=30.0)
    d = str(tmp_path_factory.mktemp("phase2mb"))
    regions = [(w.chrom, 1, w.length, "diploid")]
    sp = dict(chunks_list=get_chunks(regions, 4), regions_list=regions, sam_path=w, fasta_path=None, mincov=4, maxcov=160, min_allele_freq=0.15,
              min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=4, vcf_path=d, prefix="t", sample="SAMPLE", seq="ont",
              supplementary=False, exclude_bed=None, suppress_progress=True, disable_coverage_normalization=False)
    vcf = snpCaller.call_manager(sp)
    recs = [ln for ln in gzip.open(vcf, "rt") if not ln.startswith("#")]
    res = phase_contig(w, None, w.chrom, recs, 10, False)
    return w, recs, res


def test_contig_gather_and_phase_equal_restatement(contig):
    from nanocaller_amd.phase import kept_reads
    w, recs, res = contig
    pos, rec = res.sites["pos"], res.sites["record"]
    kept = res.reads["index"]
    assert np.array_equal(kept, kept_reads(w, False)[0])
    # the gather: every kept read's code at every site, first / second allele
    al = []
    for i in rec.tolist():
        f = recs[i].split("\t")
        pair = (f[3], f[4]) if f[9].split(":")[0] == "0/1" else tuple(f[4].split(","))
        al.append(["AGTC".index(pair[0]), "AGTC".index(pair[1])])
    al = np.array(al, np.int64).reshape(-1, 2)
    reads = []
    for r in kept.tolist():
        s0, s1 = int(w.read_start[r]), int(w.read_end[r])
        a, b = np.searchsorted(pos, s0), np.searchsorted(pos, s1)
        c = w.read_codes(r)[pos[a:b] - s0]
        rd = [(a + k, 0 if c[k] == al[a + k, 0] else 1) for k in range(b - a) if c[k] in (al[a + k, 0], al[a + k, 1])]
        reads.append(rd)
    off, site, allele = res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]
    assert _reads_of(off, site, allele) == reads
    got = dict(side=res.reads["side"], site_block=res.sites["block"], site_phased=res.sites["phased"], site_h=res.sites["h"], site_ps=res.sites["ps"],
               block_first=np.searchsorted(pos, [b[0] for b in res.blocks]), block_last=np.searchsorted(pos, [b[1] for b in res.blocks]),
               block_ps=[b[2] for b in res.blocks], block_cost=[b[3] for b in res.blocks],
               group_hp=np.zeros(res.reads["group"].max() + 1, np.uint8), group_ps=np.zeros(res.reads["group"].max() + 1, np.int32))
    got["group_hp"][res.reads["group"]] = res.reads["hp"]
    got["group_ps"][res.reads["group"]] = res.reads["ps"]
    _assert_equal_to_restatement(got, reads, pos, res.reads["group"], 15)
    assert len(res.blocks) >= 1 and res.sites["phased"].sum() > 1000


def test_contig_against_truth(contig):
    w, recs, res = contig
    pos = res.sites["pos"]
    true_het = set(np.asarray(w.het_sites).tolist())
    phased = res.sites["phased"]
    frac_phased = len(true_het & set(pos[phased].tolist())) / len(true_het)
    # the allele hap 0 carries at each site: the majority of the alleles of the reads that come from hap 0
    kept = res.reads["index"]
    origin = np.asarray(w.hap)[kept]
    off, site, allele = res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]
    rid = np.repeat(np.arange(kept.size), np.diff(off))
    votes = np.zeros((pos.size, 2), np.int64)
    np.add.at(votes, (site[origin[rid] == 0], allele[origin[rid] == 0]), 1)
    t0 = (votes[:, 1] > votes[:, 0]).astype(np.uint8)
    orient = res.sites["h"] ^ t0                                          # 0: HP 1 is hap 0 at this site
    ok = phased & np.isin(pos, list(true_het))
    idx = np.flatnonzero(ok)
    same_block = res.sites["block"][idx[1:]] == res.sites["block"][idx[:-1]]
    switches = (orient[idx[1:]] != orient[idx[:-1]]) & same_block
    switch_rate = switches.sum() / max(1, same_block.sum())
    # tagged reads after block orientation (the majority orientation of the block's sites)
    blk_or = {}
    for b in np.unique(res.sites["block"][idx]).tolist():
        o = orient[idx][res.sites["block"][idx] == b]
        blk_or[int(res.blocks[b][2])] = int(o.sum() * 2 > o.size)
    hp, ps = res.reads["hp"], res.reads["ps"]
    tagged = hp > 0
    exp = np.array([1 + (int(o) ^ blk_or.get(int(p), 0)) for o, p in zip(origin, ps)])
    acc = (hp[tagged] == exp[tagged]).mean()
    frac_tagged = tagged.mean()
    print("truth: phased %.4f of %d het sites, switch rate %.5f over %d pairs, tagged %.4f of %d reads, tagged correct %.4f, blocks %d, %s" % (
        frac_phased, len(true_het), switch_rate, same_block.sum(), frac_tagged, kept.size, acc, len(res.blocks), res.ms))
    assert frac_phased >= 0.85
    assert switch_rate <= 0.02
    assert acc >= 0.97 and frac_tagged >= 0.8


def _assert_nothing_phased(got, n_reads, n_sites, n_groups):
    assert got["entry_off"].size == n_reads + 1 and got["entry_site"].size == got["entry_allele"].size == got["entry_off"][-1]
    assert got["side"].tolist() == [-1] * n_reads and got["site_block"].tolist() == [-1] * n_sites
    for k in ("site_h", "site_phased", "site_ps"):
        assert got[k].size == n_sites and not got[k].any(), k
    for k in ("group_hp", "group_ps"):
        assert got[k].size == n_groups and not got[k].any(), k
    assert all(got[k].size == 0 for k in ("block_first", "block_last", "block_ps", "block_cost"))


def test_degenerate_inputs_come_out_empty(eng, contig):
    """the handle set-up and the counts-to-entries tail that the allele sources share (csrc/nc_happhase.h) at their zero counts: no reads and no
    sites, reads without sites, reads that all have fewer than two entries (no block forms, the DP is not launched), and a resident pack's reads
    against an empty site list -> arrays of the documented lengths, nothing phased or tagged, and the restatement's result"""
    for reads, n_sites in (([], 0), ([[], [], []], 0), ([[(0, 1)], [], [(2, 0)]], 3)):
        pos = 7 * np.arange(1, n_sites + 1, dtype=np.int32)
        groups = np.arange(len(reads), dtype=np.int32)
        got = eng.snp_phase(pos, None, groups, len(reads), csr=_csr(reads))
        _assert_nothing_phased(got, len(reads), n_sites, len(reads))
        assert got["entry_off"][-1] == sum(len(r) for r in reads)
        _assert_equal_to_restatement(got, reads, pos, groups, 15)
    import torch
    from nanocaller_amd.generate_SNP_pileups import device_pack
    from nanocaller_amd.phase import kept_reads
    w = contig[0]
    dp = device_pack(w, None, w.chrom, False, None, 0, by_name=True)[0]   # the resident pack, and its kept reads as phase_contig passes them
    kept, rs, re_, slot = kept_reads(w, False)
    n_reads = kept.size
    assert n_reads > 1000 and int(slot[-1]) <= dp.codes.numel()
    groups = np.arange(n_reads, dtype=np.int32)
    got = eng.snp_phase(np.zeros(0, np.int32), np.zeros((0, 2), np.uint8), groups, n_reads,
                        reads=(dp.codes,) + tuple(torch.from_numpy(a).to(eng.device) for a in (rs, re_, slot)))
    _assert_nothing_phased(got, n_reads, 0, n_reads)
    _assert_equal_to_restatement(got, [[]] * n_reads, np.zeros(0, np.int32), groups, 15)


# ------------------------------------------------------------------------------------------- the indel pass on haplotags
@pytest.fixture(scope="module")
def pass2_files(tmp_path_factory):
    """one pass-2 world written three times: with its truth HP / PS, without any HP / PS, and (later) with the phaser's"""
    d = str(tmp_path_factory.mktemp("p2phase"))
    w = bamio.make_pass2_world(seed=41, length=150_000, depth=28)
    recs = bamio.world_to_records(w, None)
    tagged, untagged, fa = os.path.join(d, "tagged.bam"), os.path.join(d, "untagged.bam"), os.path.join(d, "r.fa")
    bamio.write_bam(tagged, w.chrom, w.length, recs)
    bamio.write_bam(untagged, w.chrom, w.length, [dict(r, tags={}) for r in recs])
    bamio.write_fasta(fa, w.chrom, w.ref)
    return w, recs, tagged, untagged, fa, d


def _snp_vcf(bam, fa, chrom, length, out):
    from nanocaller_amd import snpCaller
    from nanocaller_amd.utils import get_chunks
    regions = [(chrom, 1, length, "diploid")]
    sp = dict(chunks_list=get_chunks(regions, 2), regions_list=regions, sam_path=bam, fasta_path=fa, mincov=4, maxcov=160, min_allele_freq=0.15,
              min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=2, vcf_path=out, prefix="s", sample="SAMPLE", seq="ont",
              supplementary=False, exclude_bed=None, suppress_progress=True, disable_coverage_normalization=False)
    return snpCaller.call_manager(sp)


def _indels(bam, fa, chrom, length, out, mode, snp_vcf=None, **kw):
    from nanocaller_amd import indelCaller
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.utils import get_chunks
    release_contig()
    os.makedirs(out, exist_ok=True)
    regions = [(chrom, 1, length, "diploid")]
    ip = dict(chunks_list=get_chunks(regions, 2, max_chunk_size=50_000), mode=mode, snp_vcf=snp_vcf, regions_list=regions, sam_path=bam, fasta_path=fa,
              mincov=4, maxcov=160, indel_model="ONT-HG002", cpu=2, vcf_path=out, prefix="t", sample="SAMPLE", seq="ont", del_t=0.6, ins_t=0.4,
              impute_indel_phase=False, supplementary=False, exclude_bed=None, win_size=40, small_win_size=4, enable_whatshap=False,
              suppress_progress=True, phase_qual_score=10, verbose=False, **kw)
    files = indelCaller.call_manager(ip)
    return files, [ln for ln in gzip.open(files["indels"], "rt") if not ln.startswith("#")]


def test_indel_calls_from_an_untagged_bam(pass2_files, monkeypatch):
    """mode 'all' on a BAM without HP / PS: with phaser='device' the indel pass gets diploid calls (the pass-through gives none)"""
    from nanocaller_amd import indelCaller
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    w, recs, tagged, untagged, fa, d = pass2_files
    snp_vcf = _snp_vcf(untagged, fa, w.chrom, w.length, os.path.join(d, "snp_u"))
    _, truth = _indels(tagged, fa, w.chrom, w.length, os.path.join(d, "i_truth"), "indels")
    _, plain = _indels(untagged, fa, w.chrom, w.length, os.path.join(d, "i_plain"), "all", snp_vcf)
    files, got = _indels(untagged, fa, w.chrom, w.length, os.path.join(d, "i_dev"), "all", snp_vcf, phaser="device")
    key = lambda ln: tuple(ln.split("\t")[:5])                             # noqa: E731
    rec = len({key(ln) for ln in got} & {key(ln) for ln in truth}) / max(1, len(truth))
    print("indel calls: truth-tagged %d, untagged pass-through %d, untagged + device phaser %d, recall %.4f" % (len(truth), len(plain), len(got), rec))
    assert len(truth) > 20 and len(plain) == 0 and len(got) > 20
    # measured 0.344 (134 of 302 calls): the world's reads are ~1.5 kb with one het SNP per kb, so a read often carries fewer than two
    # het alleles -- it joins no block and stays untagged, and the truth-tagged BAM has every read in a haplotype set
    assert rec >= 0.3
    snps = [ln for ln in gzip.open(files["snps"], "rt") if not ln.startswith("#")]
    assert sum("|" in ln.split("\t")[9].split(":")[0] for ln in snps) > 50
    tags = os.path.join(d, "i_dev", "intermediate_phase_files", "%s.haplotags.npz" % w.chrom)
    assert os.path.exists(tags)


@pytest.mark.parametrize("ingest", ["0", "1"])
def test_haplotags_equal_the_same_tags_in_the_bam(pass2_files, monkeypatch, ingest):
    """indel VCF from (untagged BAM + the phaser's haplotags) == indel VCF from a BAM whose records carry exactly those HP / PS, byte for byte,
    on the host decode route and on the device ingest route"""
    from nanocaller_amd import indelCaller
    from nanocaller_amd.phase import tags_for_names
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
    w, recs, tagged, untagged, fa, d = pass2_files
    snp_vcf = _snp_vcf(untagged, fa, w.chrom, w.length, os.path.join(d, "snp_p" + ingest))
    files, got = _indels(untagged, fa, w.chrom, w.length, os.path.join(d, "j_dev" + ingest), "all", snp_vcf, phaser="device")
    tags = os.path.join(d, "j_dev" + ingest, "intermediate_phase_files", "%s.haplotags.npz" % w.chrom)
    hp, ps = tags_for_names([r["name"] for r in recs], tags)
    assert (hp > 0).mean() > 0.2                                        # (measured 0.31: ~1.5 kb reads, see above)
    re_bam = os.path.join(d, "retagged%s.bam" % ingest)
    bamio.write_bam(re_bam, w.chrom, w.length, [dict(r, tags={"HP": int(h), "PS": int(p)} if h else {}) for r, h, p in zip(recs, hp, ps)])
    _, exp = _indels(re_bam, fa, w.chrom, w.length, os.path.join(d, "j_re" + ingest), "indels")
    assert len(exp) > 20 and got == exp

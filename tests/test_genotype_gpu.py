"""Known-sites calling on the GPU (nc_snp_scan_set_sites, k_scan<.., true>, k_site_bits) against tests/genotype_ref.py: the candidate test
`min_allele_freq <= alt_freq or v_pos in S` (or `v_pos in S` alone) and nothing else changed.  Golden worlds only (<= 135 kb).
Run on a real MI355X: python -m pytest tests -m gpu"""
import gzip
import os

import numpy as np
import pytest

from tests import genotype_ref as G
from tests.util import assert_tuple_matches_gold, load_world

pytestmark = pytest.mark.gpu

BASE = dict(threshold=[0.4, 0.6], mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, seq="ont", supplementary=False, exclude_bed=None)


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("NC_GENOTYPE_SITES", raising=False)
    monkeypatch.delenv("NC_GENOTYPE_ONLY", raising=False)


def _dct(world, dct, exclude, **kw):
    return dict(dct, sam_path=world, fasta_path=None, exclude_bed=exclude if exclude else None, **kw)


@pytest.mark.parametrize("only", [False, True], ids=["add", "only"])
@pytest.mark.parametrize("case", G.GPU_CASES)
def test_tuple_with_a_list_matches_the_reference_rule(eng, case, only):
    """get_snp_testing_candidates with dct['genotype_sites']: every field exact, as the goldens are compared"""
    from nanocaller_amd.generate_SNP_pileups import get_snp_testing_candidates
    world, dct, region, exclude = G.load_case(case)
    exp = G.expected_for(case, only)
    out = get_snp_testing_candidates(_dct(world, dct, exclude, genotype_sites={world.chrom: G.site_list(case)}, genotype_only=only), region)
    assert len(exp[0]) > 20
    assert_tuple_matches_gold(out, G.as_gold(exp))


@pytest.mark.parametrize("tile_size", [1024, 2048, 4096])
def test_positions_on_every_edge_of_the_bitmap(eng, tile_size):
    """one list built from the pack's grid (g = p - tile_pos0): the first and last bit of a lane's 16-bit load, of a 32-bit word of the atomic OR,
    of a tile; the first and last column of the contig; position 0, negative positions and positions past the grid, which the device must drop
    (the list goes in as a device tensor: nothing on the host filters it); duplicates, unsorted.  All three instantiations of k_scan<.., true>."""
    import torch
    from nanocaller_amd.pack import pack_world
    from oracle import oracle
    world = load_world("ont")
    dpk = eng.upload(pack_world(world, tile_size=tile_size))
    t0, T, nt = dpk.tile_pos0, dpk.tile_size, dpk.n_tiles
    assert nt > 2
    g = []
    for t in sorted({0, 1, nt // 2, nt - 2, nt - 1}):
        for w in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, T // 2 - 1, T // 2, T - 33, T - 32, T - 17, T - 16, T - 15, T - 2, T - 1):
            g.append(t * T + w)
    p = np.array(g, np.int64) + t0
    ignored = np.array([0, -1, -5, t0 - 1, t0 - 32, -(1 << 30), np.iinfo(np.int32).min, t0 + nt * T, t0 + nt * T + 1, t0 + nt * T + 31, world.length + 1,
                        world.length + 100_000, np.iinfo(np.int32).max], np.int64)
    s = np.concatenate([p, ignored, [1, world.length, 2, world.length - 1], p[::3], ignored[::2]])
    np.random.Generator(np.random.PCG64(tile_size)).shuffle(s)
    d_sites = torch.from_numpy(s.astype(np.int32)).cuda()
    rc = oracle.ref_codes_with_exclusions(world)
    a = (world, rc, 1, world.length, "diploid", 4)
    _, E, En, Ealt = oracle.snp_scan(*a, 0.0, [0.4, 0.6])
    nbr, N, _, _ = oracle.snp_scan(*a, 0.15, [0.4, 0.6])
    SE = np.intersect1d(s, E)
    assert len(SE) > 60 and len(np.setdiff1d(SE, N)) > 40
    for only in (False, True):
        exp = SE if only else np.union1d(N, SE)
        sites = eng.snp_scan(dpk, [(1, world.length)], mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6], sites=d_sites, sites_only=only)
        k = np.searchsorted(E, exp)
        assert np.array_equal(sites.pos, exp) and np.array_equal(sites.dp, En[k]) and np.array_equal(sites.alt, Ealt[k])
        assert np.array_equal(eng.fetch_nbr_sites(sites.n_nbr), nbr)              # a listed position is no neighbour unless it passes on its own


def test_only_mode_with_an_empty_intersection_returns_the_empty_tuple(eng):
    from nanocaller_amd.generate_SNP_pileups import get_snp_testing_candidates
    world, dct, region, exclude = G.load_case("ont_exclude")
    cl = G.site_classes(world, dct, region, exclude)
    dead = np.concatenate([cl["excluded"][:50], cl["outside"], [0, -3]])
    assert len(cl["excluded"]) > 10
    for lst in ({world.chrom: dead}, {world.chrom: []}, {"another_contig": cl["natural"]}):
        d = _dct(world, dct, exclude, genotype_sites=lst, genotype_only=True)
        assert get_snp_testing_candidates(d, region) == G.EMPTY
    # the same lists in add mode change nothing
    plain = get_snp_testing_candidates(_dct(world, dct, exclude), region)
    out = get_snp_testing_candidates(_dct(world, dct, exclude, genotype_sites={world.chrom: dead}), region)
    assert len(plain[0]) > 100
    assert_tuple_matches_gold(out, G.as_gold(plain))


def test_no_list_is_carried_into_the_next_scan(eng):
    """a plain scan right after a listed one (either mode) gives the plain result"""
    from nanocaller_amd.pack import pack_world
    from oracle import oracle
    world = load_world("ont")
    dpk = eng.upload(pack_world(world))
    rc = oracle.ref_codes_with_exclusions(world)
    kw = dict(mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6])
    _, N, Nn, Nalt = oracle.snp_scan(world, rc, 50_000, 70_000, "diploid", 4, 0.15, [0.4, 0.6])
    s = np.arange(55_000, 56_000)
    for only in (False, True):
        listed = eng.snp_scan(dpk, [(50_000, 70_000)], sites=s, sites_only=only, **kw)
        assert listed.n_sites != len(N)
        plain = eng.snp_scan(dpk, [(50_000, 70_000)], **kw)
        assert np.array_equal(plain.pos, N) and np.array_equal(plain.dp, Nn) and np.array_equal(plain.alt, Nalt)


def test_a_pack_that_holds_a_span_of_the_contig(eng):
    """a rank that owns part of a contig packs only its span: listed positions outside the pack's grid are dropped by the device"""
    from nanocaller_amd.generate_SNP_pileups import device_pack
    from oracle import oracle
    world = load_world("ont")
    dpk = device_pack(world, None, world.chrom, span=(60_000, 80_000))[0]
    assert dpk.tile_pos0 > 1 or dpk.tile_pos0 + dpk.n_tiles * dpk.tile_size <= world.length      # (not the whole contig)
    rc = oracle.ref_codes_with_exclusions(world)
    _, E, En, Ealt = oracle.snp_scan(world, rc, 64_000, 76_000, "diploid", 4, 0.0, [0.4, 0.6])
    s = np.arange(1, world.length + 1, 7)
    sites = eng.snp_scan(dpk, [(64_000, 76_000)], mincov=4, min_allele_freq=0.15, threshold=[0.4, 0.6], sites=s, sites_only=True)
    k = np.isin(E, s)
    assert k.sum() > 1000 and np.array_equal(sites.pos, E[k]) and np.array_equal(sites.dp, En[k]) and np.array_equal(sites.alt, Ealt[k])


def _two_chunks(world, lo, hi):
    """two chunks of [lo, hi] that share an end position with zero alternative reads + a list with that position in it"""
    region = dict(chrom=world.chrom, start=lo, end=hi, ploidy="diploid")
    cl = G.site_classes(world, BASE, region, None)
    shared = int(cl["zero_alt"][len(cl["zero_alt"]) // 2])
    s = np.concatenate([c[np.unique(np.linspace(0, len(c) - 1, 30).astype(int))] for c in (cl["zero_alt"], cl["below_af"], cl["natural"])] + [[shared, lo - 3, hi + 3]])
    chunks = [dict(chrom=world.chrom, start=lo, end=shared, ploidy="diploid"), dict(chrom=world.chrom, start=shared, end=hi, ploidy="diploid")]
    return chunks, shared, s


@pytest.mark.parametrize("only", [False, True], ids=["add", "only"])
def test_call_chunks_with_a_list_and_a_listed_shared_chunk_end(eng, only):
    """two chunks share an end position that is listed (and no candidate on its own): it is emitted once in each chunk (quirk E3).  pos, chunk, ref,
    dp, alt, strand depths and the chunks' mean depths exact; probabilities within the standing 1e-4 of the oracle CNN on the expected tensors
    and scale; the counts of listed / emitted positions"""
    from nanocaller_amd import snpCaller
    from nanocaller_amd.weights import Weights, get_SNP_model
    from oracle import oracle
    world = load_world("ont")
    chunks, shared, s = _two_chunks(world, 40_000, 64_000)
    params = dict(BASE, sam_path=world, fasta_path=None, snp_model="ONT-HG002", disable_coverage_normalization=False,
                  genotype_sites={world.chrom: s}, genotype_only=only)
    r = snpCaller.call_chunks(params, chunks)
    path, cov = get_SNP_model("ONT-HG002")
    w = Weights(path)
    off = 0
    for ci, c in enumerate(chunks):
        pos, ref, mat, dp, freq, depth, fwd, rev = G.expected(world, BASE, c, None, s, only)
        n = len(pos)
        sl = slice(off, off + n)
        assert n > 30 and shared in pos
        assert np.array_equal(r["pos"][sl], pos) and np.all(r["chunk"][sl] == ci)
        rcode = np.argmax(ref, 1).astype(np.int32)
        assert np.array_equal(r["ref"][sl], rcode) and np.array_equal(r["dp"][sl], dp)
        assert np.array_equal(r["alt"][sl].astype(np.float64) / r["dp"][sl], freq) and np.array_equal(r["freq"][sl], freq)
        assert np.array_equal(r["fwd_dp"][sl], fwd) and np.array_equal(r["rev_dp"][sl], rev)
        assert r["chunk_depth"][ci] == depth
        ep, _ = oracle.snp_forward(w.flat, mat, rcode, np.full(n, cov / depth), precision="f64")
        err = float(np.abs(r["probs"][sl] - ep).max())
        print("chunk %d: %d sites, max |probs - oracle| = %.3g" % (ci, n, err))
        assert err < 1e-4
        off += n
    assert off == r["n"] and int((r["pos"] == shared).sum()) == 2
    inside = np.unique(s[(s >= 40_000) & (s <= 64_000)])
    assert r["genotype_listed"] == len(inside) and r["genotype_emitted"] == len(inside)      # (every listed position inside is eligible here)
    plain = snpCaller.call_chunks(dict(params, genotype_sites=None), chunks)
    assert plain["genotype_listed"] == 0 and shared not in plain["pos"] and (plain["n"] < r["n"] or only)


def _records(vdir):
    return [ln for ln in gzip.open(os.path.join(str(vdir), "t.unfiltered.snps.vcf.gz"), "rt") if not ln.startswith("#")]


def _manager_params(world_or_bam, fasta, regions, vdir, **kw):
    from nanocaller_amd.utils import get_chunks
    return dict(BASE, chunks_list=get_chunks(regions, cpu=3), regions_list=regions, sam_path=world_or_bam, fasta_path=fasta, snp_model="ONT-HG002", cpu=1,
                vcf_path=str(vdir), prefix="t", sample="S", suppress_progress=True, disable_coverage_normalization=False, **kw)


def test_end_to_end_forced_records_equal_the_plain_records_of_a_run_on_every_column(eng, tmp_path, capsys):
    """snpCaller.caller (through call_manager) with per-site coverage scaling, which makes a record independent of the other sites: a list in only
    mode against a plain run with min_allele_freq = 0 -- the forced run's VCF records are, byte for byte, the plain run's records at the same
    positions; listed positions without a pileup have no record and are reported"""
    from nanocaller_amd import snpCaller
    world = load_world("ont")
    regions = [(world.chrom, 60_000, 84_000, "diploid")]
    region = dict(chrom=world.chrom, start=60_000, end=84_000, ploidy="diploid")
    cl = G.site_classes(world, BASE, region, None)
    s = np.concatenate([c[np.unique(np.linspace(0, len(c) - 1, 150).astype(int))] for c in (cl["zero_alt"], cl["below_af"], cl["natural"])] + [cl["outside"]])
    out = {}
    for tag, kw in (("forced", dict(genotype_sites={world.chrom: s}, genotype_only=True)), ("plain", dict(min_allele_freq=0.0))):
        vdir = tmp_path / tag
        vdir.mkdir()
        p = _manager_params(world, None, regions, vdir, **kw)
        p.update(disable_coverage_normalization=True, suppress_progress=(tag == "plain"))
        snpCaller.call_manager(p)
        out[tag] = _records(vdir)
    msg = capsys.readouterr().out
    by_pos = {}
    for ln in out["plain"]:
        by_pos.setdefault(int(ln.split("\t")[1]), []).append(ln)
    inside = np.unique(s[(s >= 60_000) & (s <= 84_000)])
    assert len(out["plain"]) > 20_000 and len(inside) > 300
    assert sorted({int(ln.split("\t")[1]) for ln in out["forced"]}) == inside.tolist()
    exp = [ln for p in inside.tolist() for ln in by_pos[p]]
    assert out["forced"] == exp
    assert sum("\tREF\t" in ln or "\tLOW\t" in ln for ln in out["forced"]) > 100 and all(ln.split("\t")[9].startswith("./.") for ln in out["forced"] if "\tREF\t" in ln)
    assert "%s: 0 listed sites got no record" % world.chrom in msg


def test_host_decode_route_and_device_ingest_give_the_same_calls(eng, tmp_path, monkeypatch):
    """a small BAM, the same list: NC_DEVICE_INGEST=0 (host decode, wire form) and the device ingest write identical records, and identical to the
    run on the in-memory world; the listed positions are there"""
    from nanocaller_amd import snpCaller
    from tests import bamio
    world = bamio.make_bam_world(seed=9, length=40_000, depth=22)
    rng = np.random.Generator(np.random.PCG64(2))
    bam, fa = str(tmp_path / "s.bam"), str(tmp_path / "r.fa")
    bamio.write_bam(bam, world.chrom, world.length, bamio.world_to_records(world, rng))
    bamio.write_fasta(fa, world.chrom, world.ref)
    regions = [(world.chrom, 2_000, 38_000, "diploid")]
    region = dict(chrom=world.chrom, start=2_000, end=38_000, ploidy="diploid")
    cl = G.site_classes(world, BASE, region, None)
    s = np.concatenate([c[np.unique(np.linspace(0, len(c) - 1, 60).astype(int))] for c in (cl["zero_alt"], cl["below_af"], cl["natural"])] + [cl["outside"], cl["masked_ref"][:20]])
    forced = np.unique(np.concatenate([cl["zero_alt"], cl["below_af"]])[np.isin(np.concatenate([cl["zero_alt"], cl["below_af"]]), s)])
    assert len(forced) > 60
    outs = {}
    for tag, sam, ingest in (("host", bam, "0"), ("device", bam, "1"), ("world", world, "1")):
        monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
        vdir = tmp_path / tag
        vdir.mkdir()
        snpCaller.call_manager(_manager_params(sam, fa, regions, vdir, genotype_sites={world.chrom: s}))
        outs[tag] = _records(vdir)
    assert outs["host"] == outs["device"] == outs["world"]
    got = {int(ln.split("\t")[1]) for ln in outs["host"]}
    assert set(forced.tolist()) <= got and len(outs["host"]) > len(forced) + 50


def test_a_sites_vcf_plain_or_bgzipped_gives_the_calls_of_the_dict_form(eng, tmp_path, monkeypatch):
    """the list from a VCF (one-base REF lines; an indel line and a second contig in it), as params['genotype_sites'] and through NC_GENOTYPE_SITES"""
    from nanocaller_amd import snpCaller, vcfio
    world = load_world("ont")
    chunks, shared, s = _two_chunks(world, 70_000, 90_000)
    lines = ["%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (world.chrom, p, world.ref[p - 1].upper() if p <= world.length else "A", "ACGT"[i % 4]) for i, p in enumerate(s.tolist()) if p >= 1]
    lines.insert(5, "%s\t%d\t.\tACG\tA\t.\t.\t.\n" % (world.chrom, 75_001))              # an indel line: skipped (75,001 is listed by no other line)
    lines += ["chrOther\t%d\t.\tA\tC\t.\t.\t.\n" % p for p in (71_000, 71_001)]
    assert 75_001 not in s
    text = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join(lines)
    plain, bgz = str(tmp_path / "sites.vcf"), str(tmp_path / "sites.vcf.gz")
    open(plain, "w").write(text)
    vcfio.bgzf_write(bgz, text.encode())
    params = dict(BASE, sam_path=world, fasta_path=None, snp_model="ONT-HG002", disable_coverage_normalization=False)
    ref = snpCaller.call_chunks(dict(params, genotype_sites={world.chrom: s}), chunks)
    assert ref["n"] > 100 and int((ref["pos"] == shared).sum()) == 2 and 75_001 not in ref["pos"]
    runs = [snpCaller.call_chunks(dict(params, genotype_sites=p), chunks) for p in (plain, bgz)]
    monkeypatch.setenv("NC_GENOTYPE_SITES", bgz)
    runs.append(snpCaller.call_chunks(params, chunks))
    for r in runs:
        assert r["n"] == ref["n"] and r["genotype_listed"] == ref["genotype_listed"] and r["genotype_emitted"] == ref["genotype_emitted"]
        for key in ("pos", "chunk", "ref", "probs", "gt", "dp", "alt", "fwd_dp", "rev_dp", "freq", "chunk_depth"):
            assert np.array_equal(r[key], ref[key]), key

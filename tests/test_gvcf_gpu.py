"""The gVCF's reference-confidence blocks on the GPU (csrc/nc_refconf.hip through Engine.refconf_columns / refconf_blocks / refconf_text, and
snpCaller.call_manager with params['gvcf']) against tests/gvcf_ref.py.  Golden worlds and crafted arrays only.
Run on a real MI355X: python -m pytest tests -m gpu"""
import gzip
import os

import numpy as np
import pytest

from nanocaller_amd import gvcf
from tests import gvcf_ref as R
from tests.util import load_world

pytestmark = pytest.mark.gpu

T = 4096                                                              # Engine.REFCONF_TILE: columns per workgroup of the blocks kernels
KW = dict(error=0.1, bands=R.BANDS)
# words whose columns fall into the no-call band and the five default bands: n reads, all reference -> GQ 2, 25, 51, 76, 99
NOCALL, B0, B1, B2, B3, B4 = 0, 1, 10, 20, 30, 40
MASK = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    e = get_engine(0)
    assert e.REFCONF_TILE == T
    return e


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("NC_GVCF", raising=False)


def _dev(w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w, np.uint32).view(np.int32)).cuda()


def _check(eng, w, pos0, chunks, cuts=None, haploid=False, bands=R.BANDS):
    """device blocks of the word array == the yardstick's; -> the blocks"""
    exp = R.blocks_of_words(w, pos0, chunks, cuts, R.CONSTS, bands, haploid)
    got = eng.refconf_blocks(_dev(w), pos0, chunks, np.asarray(cuts, np.int32) if cuts else None, error=0.1, bands=bands, haploid=haploid)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert np.array_equal(got, exp)
    return got


# ------------------------------------------------------------------ columns
@pytest.mark.parametrize("tile_size", [1024, 2048, 4096])
@pytest.mark.parametrize("name", ["ont", "deep"])
def test_words_equal_the_yardstick(eng, name, tile_size):
    from nanocaller_amd.pack import pack_world
    world = load_world(name)
    col = R.columns(world, key=name)
    dpk = eng.upload(pack_world(world, tile_size=tile_size))
    words, ref_code, pos0 = eng.refconf_columns(dpk)
    got = words.cpu().numpy().view(np.uint32)
    assert got.size == dpk.n_tiles * tile_size and pos0 == dpk.tile_pos0
    assert np.array_equal(got, R.words(col, pos0, got.size))
    assert np.array_equal(ref_code.cpu().numpy(), dpk.ref_code.cpu().numpy()[:got.size])


def _deep_world():
    """three tiles of 1024 columns; 600 reads over one stretch (the byte-lane counters are widened twice and hold a remainder), a column nobody covers
    between covered ones, reads that end on and one past a 16-column slot edge, a masked reference base under the reads"""
    from nanocaller_amd.synth import World
    rng = np.random.Generator(np.random.PCG64(11))
    L = 3000
    ref = rng.integers(0, 4, L)
    spans = [(500 + int(rng.integers(0, 40)), 700 + int(rng.integers(0, 40))) for _ in range(600)]
    spans += [(1000, 1024), (1001, 1025), (1008, 1040), (1100, 1150), (1151, 1200), (2040, 2060), (2047, 2049)]
    spans.sort()
    codes, off = [], [0]
    for s, e in spans:
        c = ref[s - 1:e - 1].copy()
        noise = rng.random(e - s)
        c = np.where(noise < 0.12, rng.integers(0, 4, e - s), c)
        c = np.where(noise > 0.95, 4, c)
        codes.append(c.astype(np.uint8))
        off.append(off[-1] + e - s)
    letters = np.frombuffer(b"AGTC", np.uint8)[ref].copy()
    letters[[599, 640]] = ord("N")
    n = len(spans)
    return World(chrom="c", ref=letters.tobytes().decode(), read_start=np.array([s for s, _ in spans], np.int32), read_end=np.array([e for _, e in spans], np.int32),
                 read_flag=np.zeros(n, np.int32), read_off=np.array(off, np.int64), codes=np.concatenate(codes), names=["q%d" % i for i in range(n)])


@pytest.mark.parametrize("tile_size", [1024, 2048, 4096])
def test_words_past_the_widening_of_the_counters(eng, tile_size):
    from nanocaller_amd.pack import pack_world
    world = _deep_world()
    col = R.columns(world)
    assert col["n"].max() >= 560 and col["n"][1149] == 0 and col["n"][1148] > 0 and col["n"][1150] > 0 and col["rc"][599] >= 4
    assert col["n"][1021:1025].tolist() == [3, 3, 2, 1] and (col["ref"] > 510).any() and col["n"].max() == 600 and (col["alt"] > 60).any()
    dpk = eng.upload(pack_world(world, tile_size=tile_size))
    if tile_size == 1024:
        assert dpk.n_tiles == 3
    words, _, pos0 = eng.refconf_columns(dpk)
    got = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, R.words(col, pos0, got.size))


# ------------------------------------------------------------------ blocks on crafted words
def test_one_band_over_five_tiles_is_one_block(eng):
    w = np.full(5 * T, B3, np.uint32)
    got = _check(eng, w, 1600, [(1600, 1600 + 5 * T - 1)])
    assert got.tolist() == [[1600, 1600 + 5 * T - 1, 30, 76, 30, 0]]
    # ... and a stretch nobody covers, as long: one no-call block
    got = _check(eng, np.zeros(5 * T, np.uint32), 0, [(1, 10 * T)])
    assert got.tolist() == [[1, 5 * T - 1, 0, 0, 0, 0]]


def test_a_band_that_alternates_on_every_column_gives_one_block_per_column(eng):
    w = np.where(np.arange(3 * T) % 2 == 0, B1, B3).astype(np.uint32)
    got = _check(eng, w, 0, [(0, 3 * T)])
    assert len(got) == 3 * T and np.array_equal(got[:, 0], got[:, 1])
    # no-call columns and called columns with GQ 0 are two bands (n = 1, alt = 0 has GQ 2; n = 2, alt = 1: S00 = S11 > S01 is a no-call)
    w = np.where(np.arange(2 * T) % 2 == 0, 1, 2 | (1 << 16)).astype(np.uint32)
    assert len(_check(eng, w, 0, [(0, 2 * T)])) == 2 * T


@pytest.mark.parametrize("shift", [0, 1, 15])
def test_borders_on_every_lane_wave_and_tile_edge(eng, shift):
    """the band changes where (column + shift) is a multiple of 16: on every edge of a lane, of a wave and of a tile, one column in front of them, one
    behind them"""
    g = np.arange(3 * T + 1024)
    w = np.array([B1, B2, B4, NOCALL], np.uint32)[((g + shift) // 16) % 4]
    got = _check(eng, w, 160, [(0, 10 * T)])
    assert len(got) >= g.size // 16
    # runs of random lengths from 1 to a few tiles, random counts: every position of a border relative to the three edges
    rng = np.random.Generator(np.random.PCG64(shift))
    runs = np.concatenate([rng.integers(1, 40, 300), rng.integers(1000, 9000, 6), rng.integers(1, 3, 300), [T, T, 1024, 16, 16]])
    rng.shuffle(runs)
    val = rng.choice(np.array([NOCALL, B0, B1, B2, B3, B4, MASK, 7 | (2 << 16), 30 | (9 << 16), 65535, 65535 | (30000 << 16)], np.uint32), runs.size)
    w = np.repeat(val, runs)
    w = w[:(w.size // 16) * 16].copy()
    jitter = rng.random(w.size) < 0.3
    # depths differ inside a band: min n and the leftmost minimum GQ are not trivial
    w[jitter & (w != MASK) & ((w & 0xFFFF) < 60000)] += 1
    _check(eng, w, 16 * shift, [(1, w.size + 99)])
    _check(eng, w, 16 * shift, [(1, w.size + 99)], haploid=True)
    _check(eng, w, 16 * shift, [(1, w.size + 99)], bands=[0, 3, 26, 27, 52, 98, 99])


def test_a_masked_tile_inside_a_run(eng):
    w = np.full(4 * T, B2, np.uint32)
    w[T:2 * T] = MASK
    got = _check(eng, w, 0, [(0, 4 * T)])
    assert got[:, :2].tolist() == [[0, T - 1], [2 * T, 4 * T - 1]]


def test_cuts_on_tile_edges_and_adjacent_cuts(eng):
    w = np.full(3 * T, B2, np.uint32)
    cuts = [(T, T), (2 * T - 1, 2 * T - 1), (2 * T, 2 * T), (100, 100), (101, 101), (102, 102), (3 * T - 1, 3 * T - 1), (0, 0), (500, 520), (510, 530),
            (-40, -3), (3 * T, 3 * T + 50)]
    got = _check(eng, w, 0, [(0, 3 * T)], cuts)
    assert got[:, :2].tolist() == [[1, 99], [103, 499], [531, T - 1], [T + 1, 2 * T - 2], [2 * T + 1, 3 * T - 2]]
    # a grid that starts elsewhere: the same cuts in positions
    _check(eng, w, 4800, [(0, 4 * T)], [(a + 4800, b + 4800) for a, b in cuts])


def test_chunks_mid_lane_gaps_abutting_and_overlapping(eng):
    rng = np.random.Generator(np.random.PCG64(3))
    w = rng.choice(np.array([B1, B1, B1, B3, NOCALL], np.uint32), 3 * T)
    assert _check(eng, w, 0, [(5, 9)])[[0, -1], [0, 1]].tolist() == [5, 9]                   # starts and ends mid-lane
    got = _check(eng, w, 0, [(21, 1000), (T + 7, 2 * T + 3)])                                # two chunks with a gap
    assert got[0, 0] == 21 and got[-1, 1] == 2 * T + 3 and not np.any((got[:, 0] <= 1001) & (got[:, 1] >= 1001))
    a = _check(eng, w, 0, [(21, 1000), (1001, 5000)])                                        # abutting
    b = _check(eng, w, 0, [(21, 1000), (1000, 5000)])                                        # sharing their end point
    c = _check(eng, w, 0, [(900, 5000), (21, 1000), (30, 40)])                               # overlapping, unsorted
    d = _check(eng, w, 0, [(21, 5000)])
    assert np.array_equal(a, d) and np.array_equal(b, d) and np.array_equal(c, d)


def test_the_leftmost_minimum_wins_a_tie(eng):
    """two columns of one block with the same, smallest GQ and different counts, tiles apart, in both orders"""
    c = R.CONSTS
    cand = [(n, a) for n in range(1, 60) for a in range(0, 8) if a <= n and not gvcf.scores(n, a, c)[0] and gvcf.scores(n, a, c)[1] == 20]
    assert len(cand) >= 2 and cand[0] == (8, 0)
    x, y = (cand[0][0] | (cand[0][1] << 16)), (cand[1][0] | (cand[1][1] << 16))
    for first, second in ((x, y), (y, x)):
        w = np.full(3 * T, B1, np.uint32)
        w[100], w[2 * T + 77] = first, second
        got = _check(eng, w, 0, [(0, 3 * T)])
        assert len(got) == 1 and got[0, 3] == 20 and (got[0, 4] | (got[0, 5] << 16)) == first


def test_one_tile_and_nothing_open(eng):
    w = np.array([B1] * 7 + [B3] * 9 + [NOCALL] * 16, np.uint32)
    assert len(_check(eng, w, 0, [(0, 100)])) == 3
    assert len(_check(eng, np.full(1024, B2, np.uint32), 16, [(0, 5000)])) == 1
    for ww, chunks, cuts in ((np.full(2 * T, MASK, np.uint32), [(0, 3 * T)], None), (np.full(2 * T, B2, np.uint32), [(3 * T, 4 * T)], None),
                             (np.full(2 * T, B2, np.uint32), [], None), (np.full(64, B2, np.uint32), [(0, 63)], [(-5, 900)])):
        assert _check(eng, ww, 0, chunks, cuts).shape == (0, 6)


def test_two_runs_are_bit_identical(eng):
    world = load_world("ont")
    col = R.columns(world, key="ont")
    w = R.words(col, 0, 33 * T)
    d = _dev(w)
    runs = [eng.refconf_blocks(d, 0, [(1, world.length)], None, **KW) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]) and runs[0].tobytes() == runs[1].tobytes()
    exp = R.world_blocks(col, [(1, world.length)])
    assert len(exp) > 60_000 and np.array_equal(runs[0], exp)
    dev = eng.refconf_blocks(d, 0, [(1, world.length)], None, device_out=True, **KW)
    assert np.array_equal(dev.cpu().numpy(), exp)


# ------------------------------------------------------------------ text
@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_text_equals_the_python_formatter(eng, haploid):
    """1- to 9-digit positions (a 10-digit END), depths 0, 9, 10, 8000 and 65535, capped PLs, calls and no-calls"""
    import torch
    counts = [(0, 0), (9, 0), (10, 0), (10, 5), (8000, 0), (8000, 4000), (65535, 0), (65535, 65535), (65535, 20000), (3000, 0), (1, 0), (2, 1), (37, 2)]
    for digits in range(1, 10):
        start = int("123456789"[:digits])
        pos0 = max(0, (start - 40) // 16 * 16)
        ref = np.random.Generator(np.random.PCG64(digits)).integers(0, 4, 4096).astype(np.uint8)
        blk, s = [], start
        for k, (n, a) in enumerate(counts):
            e = s + [0, 8, 99, 1000][k % 4]
            min_dp = [0, 9, 10, 8000, 65535][k % 5] if n else 0
            blk.append((s, e, min(min_dp, n), gvcf.scores(n, a, R.CONSTS, haploid)[1], n, a))
            s = e + 2
        blk.append((s, 2_000_000_000, 10, 25, 10, 0))
        blk = np.asarray(blk, np.int32)
        assert blk[-2, 0] - pos0 < 4096
        text, off = eng.refconf_text(blk, torch.from_numpy(ref).cuda(), pos0, "chr20_x", error=0.1, haploid=haploid)
        exp = R.lines("chr20_x", blk, lambda p: "AGTC"[ref[p - pos0]], R.CONSTS, haploid)
        assert text.tobytes().decode() == "".join(exp)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(x) for x in exp])]))
    text, off = eng.refconf_text(np.zeros((0, 6), np.int32), torch.from_numpy(ref).cuda(), 0, "c", error=0.1, haploid=haploid)
    assert text.size == 0 and off.tolist() == [0]


def test_text_of_many_blocks(eng):
    """more lines than one workgroup scans: the blocks of `deep` and of `ont`, every line offset"""
    from nanocaller_amd.pack import pack_world
    for name in ("deep", "ont"):
        world = load_world(name)
        dpk = eng.upload(pack_world(world))
        words, ref_code, pos0 = eng.refconf_columns(dpk)
        blk = eng.refconf_blocks(words, dpk, [(1, world.length)], None, **KW)
        assert np.array_equal(blk, R.world_blocks(R.columns(world, key=name), [(1, world.length)]))
        text, off = eng.refconf_text(blk, ref_code, pos0, world.chrom, error=0.1)
        exp = R.lines(world.chrom, blk, lambda p: world.ref[p - 1].upper())
        assert text.tobytes().decode() == "".join(exp) and off[-1] == text.size and np.array_equal(np.diff(off), [len(x) for x in exp])


# ------------------------------------------------------------------ end to end
BASE = dict(threshold=[0.4, 0.6], mincov=4, maxcov=160, min_allele_freq=0.15, min_nbr_sites=1, seq="ont", supplementary=False, exclude_bed=None)


def _manager_params(world, regions, vdir, **kw):
    from nanocaller_amd.utils import get_chunks
    return dict(BASE, chunks_list=get_chunks(regions, cpu=3), regions_list=regions, sam_path=world, fasta_path=None, snp_model="ONT-HG002", cpu=1,
                vcf_path=str(vdir), prefix="t", sample="S", suppress_progress=True, disable_coverage_normalization=False, **kw)


def test_call_manager_writes_the_gvcf_and_leaves_the_vcfs_alone(eng, tmp_path):
    from nanocaller_amd import snpCaller, vcfio
    from tests.test_vcfio import _parse_csi, _read_range, _reg2bins
    world = load_world("deep")
    col = R.columns(world, key="deep")
    regions = [(world.chrom, 1_000, 23_000, "diploid")]
    files = {}
    for tag, kw in (("plain", {}), ("gvcf", dict(gvcf=True))):
        vdir = tmp_path / tag
        vdir.mkdir()
        p = _manager_params(world, regions, vdir, **kw)
        snpCaller.call_manager(p)
        files[tag] = {f: open(os.path.join(str(vdir), f), "rb").read() for f in sorted(os.listdir(str(vdir))) if not os.path.isdir(os.path.join(str(vdir), f))}
    chunks = [(c["start"], c["end"]) for c in p["chunks_list"]]
    assert len(chunks) > 1
    assert sorted(files["plain"]) == ["t.snps.vcf.gz", "t.snps.vcf.gz.csi", "t.unfiltered.snps.vcf.gz", "t.unfiltered.snps.vcf.gz.csi"]
    assert sorted(files["gvcf"]) == sorted(list(files["plain"]) + ["t.snps.g.vcf.gz", "t.snps.g.vcf.gz.csi"])
    for f in files["plain"]:
        assert files["gvcf"][f] == files["plain"][f], f
    gpath = os.path.join(str(tmp_path / "gvcf"), "t.snps.g.vcf.gz")
    hdr, recs = vcfio.read_vcf_gz(gpath)
    assert "".join(hdr) == gvcf.header([world.chrom], "S")
    _, var = vcfio.read_vcf_gz(os.path.join(str(tmp_path / "gvcf"), "t.unfiltered.snps.vcf.gz"))
    is_block = np.array(["\t<*>\t" in ln for ln in recs])
    assert [ln for ln, b in zip(recs, is_block) if not b] == var and len(var) > 20
    vpos = [int(ln.split("\t")[1]) for ln in var]
    exp = R.world_blocks(col, chunks, [(q, q) for q in vpos])
    exp_lines = R.lines(world.chrom, exp, lambda q: world.ref[q - 1].upper())
    assert [ln for ln, b in zip(recs, is_block) if b] == exp_lines and len(exp) > 300
    pos = [int(ln.split("\t")[1]) for ln in recs]
    assert pos == sorted(pos)
    # every open column is covered exactly once: by a block or by a record's position
    cover = np.zeros(world.length + 2, np.int64)
    for ln in exp_lines:
        s, e = R.parse_block(ln)[:2]
        cover[s:e + 1] += 1
    cover[np.unique(vpos)] += 1
    assert np.array_equal(cover[1:world.length + 1], R.open_mask(world.length, 1, chunks, None, col["rc"] < 4).astype(np.int64))
    # the index follows END: a position in the middle of the longest block finds it
    k = int(np.argmax(exp[:, 1] - exp[:, 0]))
    mid = int(exp[k, 0] + exp[k, 1]) // 2
    raw = open(gpath, "rb").read()
    idx = _parse_csi(gzip.decompress(open(gpath + ".csi", "rb").read()))
    bins, found = idx["refs"][0], []
    for x in _reg2bins(mid - 1, mid, 14, 5):
        for cb, ce in bins.get(x, (0, []))[1]:
            for rec in _read_range(raw, cb, ce).decode().splitlines(keepends=True):
                if "\t<*>\t" in rec:
                    s, e = R.parse_block(rec)[:2]
                    if s <= mid <= e:
                        found.append(rec)
    assert set(found) == {exp_lines[k]}


def test_the_ingest_pipeline_of_a_bam_gives_the_worlds_blocks(eng, tmp_path, monkeypatch):
    """a small BAM through caller()'s ingest pipeline, host decode and device ingest (their packs share buffers between groups): the same gVCF
    records, and the blocks the yardstick makes from the in-memory world"""
    from nanocaller_amd import snpCaller, vcfio
    from tests import bamio
    world = bamio.make_bam_world(seed=9, length=40_000, depth=22)
    rng = np.random.Generator(np.random.PCG64(2))
    bam, fa = str(tmp_path / "s.bam"), str(tmp_path / "r.fa")
    bamio.write_bam(bam, world.chrom, world.length, bamio.world_to_records(world, rng))
    bamio.write_fasta(fa, world.chrom, world.ref)
    regions = [(world.chrom, 2_000, 38_000, "diploid")]
    outs = {}
    for tag, ingest in (("host", "0"), ("device", "1")):
        monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
        vdir = tmp_path / tag
        vdir.mkdir()
        p = dict(_manager_params(bam, regions, vdir, gvcf=True, gvcf_gq_bands=[0, 30, 70]), fasta_path=fa)
        snpCaller.call_manager(p)
        outs[tag] = vcfio.read_vcf_gz(os.path.join(str(vdir), "t.snps.g.vcf.gz"))[1]
    assert outs["host"] == outs["device"]
    chunks = [(c["start"], c["end"]) for c in p["chunks_list"]]
    vpos = [int(ln.split("\t")[1]) for ln in outs["host"] if "\t<*>\t" not in ln]
    exp = R.world_blocks(R.columns(world), chunks, [(q, q) for q in vpos], bands=[0, 30, 70])
    assert len(vpos) > 20 and len(exp) > 300
    assert [ln for ln in outs["host"] if "\t<*>\t" in ln] == R.lines(world.chrom, exp, lambda q: world.ref[q - 1].upper())

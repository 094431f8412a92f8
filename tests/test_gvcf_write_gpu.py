"""The gVCF's device writer on the GPU (csrc/nc_vcfwrite.hip through Engine.lines_merge / lines_index,
vcf_write.write_piece, gvcf.group_pieces / merge_pieces and snpCaller.call_manager with params['gvcf_writer'] = 'device').  The yardsticks
are code of the tree: gvcf.splice for the order of the lines, zlib for the members, vcfio.csi_bytes -- the per-record index writer -- on the
file's own virtual offsets, and the host writer's file.  Crafted arrays and golden worlds only.
Run on a real MI355X: python -m pytest tests -m gpu"""
import gzip
import io
import os

import numpy as np
import pytest

from nanocaller_amd import gvcf, vcfio
from nanocaller_amd.bgzf import BGZF_BLOCK
from tests import gvcf_write_ref as W

pytestmark = pytest.mark.gpu
W14 = 1 << 14


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("NC_GVCF", raising=False)
    monkeypatch.delenv("NC_GVCF_WRITER", raising=False)


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


# ------------------------------------------------------------------ merge
def _text_lines(rng, lens):
    """lines of the given lengths (the newline included): lower-case letters, so a 1-byte line is a bare newline"""
    return [bytes(rng.integers(97, 123, int(n) - 1).astype(np.uint8)) + b"\n" for n in lens]


def _lists(rng, na, nb, a_lens=None, b_lens=None):
    """A: na lines on distinct ascending keys; B: nb lines whose keys hold runs of several lines in one gap of A, duplicates, keys equal to a key
    of A, keys in front of A's first and behind A's last"""
    a_key = np.sort(rng.choice(np.arange(100, 100 + 40 * max(na, 1)), na, replace=False)).astype(np.int64)
    lo, hi = (int(a_key[0]), int(a_key[-1])) if na else (100, 200)
    b_key = rng.integers(lo, hi + 1, nb).astype(np.int64)
    if nb >= 12 and na >= 4:
        b_key[:3] = [lo - 7, lo - 7, lo - 1]                          # in front of A's first, two of them on one key
        b_key[3:5] = [hi + 1, hi + 9]                                 # behind A's last
        b_key[5:8] = a_key[[1, na // 2, na - 1]]                      # on a key of A
        gap = int(np.argmax(np.diff(a_key)))                          # several lines in one gap, two of them on one key
        b_key[8:12] = np.minimum(a_key[gap] + np.array([1, 1, 2, 3]), a_key[gap + 1])
    b_key.sort()
    a_lines = _text_lines(rng, rng.integers(1, 201, na) if a_lens is None else a_lens)
    b_lines = _text_lines(rng, rng.integers(1, 201, nb) if b_lens is None else b_lens)
    a_end = a_key + rng.integers(1, 50, na)
    b_end = b_key + rng.integers(1, 5, nb)
    return (a_lines, a_key, a_end), (b_lines, b_key, b_end)


def _as_list(lines, key, end):
    """-> Engine.lines_merge's tuple of device tensors (None: no lines)"""
    if not lines:
        return None
    text = np.frombuffer(b"".join(lines), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)
    return _dev(text), _dev(off), _dev(key), _dev(key), _dev(end)


def _check_merge(eng, A, B):
    import torch
    (a_lines, a_key, a_end), (b_lines, b_key, b_end) = A, B
    na, nb = len(a_lines), len(b_lines)
    # the yardstick: gvcf.splice of A's text with B's lines (B's lines end with their only newline)
    a_off = np.concatenate([[0], np.cumsum([len(x) for x in a_lines])]).astype(np.int64)
    want = b"".join(bytes(x) for x in gvcf.splice(np.frombuffer(b"".join(a_lines), np.uint8), a_off, a_key, b"".join(b_lines), b_key))
    # ... whose order is: B's line j in front of A's line searchsorted(a_key, b_key[j], 'left'), stable
    order = np.lexsort((np.concatenate([np.ones(na), np.zeros(nb)]), np.concatenate([a_key, b_key])))
    src = np.concatenate([np.arange(na), na + np.arange(nb)])[order]
    lines = (a_lines + b_lines)
    assert b"".join(lines[k] for k in src) == want
    runs = [eng.lines_merge(_as_list(a_lines, a_key, a_end), _as_list(b_lines, b_key, b_end)) for _ in range(2)]
    text, off, beg, end, got_src = runs[0]
    assert text.cpu().numpy().tobytes() == want
    assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(lines[k]) for k in src])]))
    assert np.array_equal(beg.cpu().numpy(), np.concatenate([a_key, b_key])[src]) and np.array_equal(end.cpu().numpy(), np.concatenate([a_end, b_end])[src])
    assert np.array_equal(got_src.cpu().numpy(), src)
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
    return src


def test_merge_equals_splice(eng):
    rng = np.random.Generator(np.random.PCG64(1))
    A, B = _lists(rng, 3000, 200)
    assert len(set(B[1].tolist())) < 200 and np.intersect1d(A[1], B[1]).size >= 3 and B[1][0] < A[1][0] and B[1][-1] > A[1][-1]
    assert {1, 200} <= {len(x) for x in A[0]} and sum(len(x) for x in A[0] + B[0]) > 16 * 16384
    src = _check_merge(eng, A, B)
    assert np.max(np.diff(np.flatnonzero(src < 3000))) >= 4              # a run of several of B's lines between two of A's


@pytest.mark.parametrize("na,nb", [(3000, 0), (0, 200), (0, 0), (1, 0), (0, 1)])
def test_merge_with_an_empty_list(eng, na, nb):
    rng = np.random.Generator(np.random.PCG64(2))
    _check_merge(eng, *_lists(rng, na, nb))


@pytest.mark.parametrize("total", [15, 16, 17, 4097])
def test_merge_of_small_totals(eng, total):
    """texts that end one byte short of, on, and one byte behind a 16-byte store; 4,097 bytes: one byte behind a multiple of 16, lines that cross
    the 16-byte pieces at every phase"""
    rng = np.random.Generator(np.random.PCG64(total))
    if total < 100:
        a_lens, b_lens = [total - 9], [3, 6]
    else:
        a_lens = [7] * 300 + [total - 2100 - 1100]
        b_lens = [11] * 100
    A, B = _lists(rng, len(a_lens), len(b_lens), a_lens, b_lens)
    assert sum(a_lens) + sum(b_lens) == total
    _check_merge(eng, A, B)


def test_merge_refuses_keys_that_descend(eng):
    rng = np.random.Generator(np.random.PCG64(3))
    A, B = _lists(rng, 50, 20)
    B[1][5], B[1][6] = B[1][6] + 1, B[1][5]
    with pytest.raises(ValueError, match="keys descend"):
        eng.lines_merge(_as_list(*A), _as_list(*B))


# ------------------------------------------------------------------ members
def _member_text(rng, kind):
    """lines (letters from a small alphabet, so the members deflate) and their bounds for the three shapes of a piece's text"""
    if kind == "3.2 members":
        # a line that ends exactly on byte 65,280, one that straddles 2 x 65,280, 0.2 members behind the third border
        lens, left = [], BGZF_BLOCK
        while left > 400:
            lens.append(int(rng.integers(30, 200)))
            left -= lens[-1]
        lens.append(left)
        at = BGZF_BLOCK
        while at < 2 * BGZF_BLOCK - 150:
            lens.append(int(rng.integers(30, 140)))
            at += lens[-1]
        assert at < 2 * BGZF_BLOCK
        lens.append(2 * BGZF_BLOCK - at + 17)
        total = int(3.2 * BGZF_BLOCK)
    elif kind == "last member of 1 byte":
        lens, total = [], 3 * BGZF_BLOCK + 1
    else:
        lens, total = [], 2 * BGZF_BLOCK
    left = total - sum(lens)
    while left > 400:
        lens.append(int(rng.integers(30, 200)))
        left -= lens[-1]
    lens.append(left)
    lines = [bytes(rng.choice(np.frombuffer(b"ACGT\t0123:,./", np.uint8), n - 1)) + b"\n" for n in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    beg = 1000 + np.arange(len(lens), dtype=np.int64) * 37
    return lines, off, beg, beg + 37


@pytest.mark.parametrize("kind", ["3.2 members", "last member of 1 byte", "exactly two members"])
def test_piece_members_and_offsets(eng, kind):
    from nanocaller_amd import vcf_write
    rng = np.random.Generator(np.random.PCG64(5))
    lines, off, beg, end = _member_text(rng, kind)
    text = b"".join(lines)
    if kind == "3.2 members":
        assert BGZF_BLOCK in off and 2 * BGZF_BLOCK not in off and 3 * BGZF_BLOCK not in off and len(text) == int(3.2 * BGZF_BLOCK)
    pad = 48                                                             # the piece lies inside a longer text, as a group's pieces do
    d_text = _dev(np.frombuffer(b"x" * pad + text + b"yy", np.uint8))
    args = (d_text, _dev(off + pad), _dev(beg), _dev(end))
    f = io.BytesIO()
    s = vcf_write.write_piece(eng, f, *args)
    raw = f.getvalue()
    got, foff, uoff = W.inflate_members(raw)                             # (zlib; every member's CRC-32 and ISIZE)
    assert got == text and s["bytes"] == len(raw) and s["lines"] == len(lines) and s["text_bytes"] == len(text)
    assert s["members"] == foff.size - 1 == -(-len(text) // BGZF_BLOCK) and np.array_equal(np.diff(uoff)[:-1], np.full(s["members"] - 1, BGZF_BLOCK))
    if kind == "last member of 1 byte":
        assert uoff[-1] - uoff[-2] == 1
    exp = W.lines_index(beg, end, off, foff)
    for k in ("run_bin", "run_vbeg", "run_vend", "win_min"):
        assert np.array_equal(s[k], exp[k]), k
    assert s["w0"] == exp["w0"] and int(s["run_vend"][-1]) == len(raw) << 16 and int(s["run_vbeg"][0]) == 0
    assert set(s["ms"]) == {"deflate", "crc", "assemble", "d2h", "index", "write"} and all(v >= 0 for v in s["ms"].values())
    f2 = io.BytesIO()
    s2 = vcf_write.write_piece(eng, f2, *args, slab_members=2)
    assert f2.getvalue() == raw and all(np.array_equal(s2[k], s[k]) for k in ("run_bin", "run_vbeg", "run_vend", "win_min"))
    f1 = io.BytesIO()
    vcf_write.write_piece(eng, f1, *args, slab_members=1)
    assert f1.getvalue() == raw


# ------------------------------------------------------------------ index
BORDERS = [1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26]


def _index_lines(rng, n):
    """n non-overlapping lines in position order: one over each of a 16 kb, 128 kb, 1 Mb, 8 Mb and 64 Mb border (where n allows), stretches
    longer than a window that nothing covers, one line of more than 40 windows, short lines around them"""
    special = [(b - int(rng.integers(1, 40)), b + int(rng.integers(1, 40))) for b in BORDERS]
    special.insert(2, (300_000, 300_000 + 41 * W14 + 77))
    if n == 1:
        return np.array([special[2][0]], np.int64), np.array([special[2][1]], np.int64)
    special = special[:min(len(special), max(1, n // 8))] if n < 48 else special
    per = max(0, (n - len(special)) // (len(special) + 1))
    beg, end, p = [], [], 9000
    for k in range(len(special) + 1):
        stop = special[k][0] if k < len(special) else 1 << 62
        m = per if k < len(special) else n - len(beg)
        for _ in range(m):
            ln = 1 if rng.random() < 0.4 else int(rng.integers(1, 900))
            skip = int(rng.integers(W14 + 1, 3 * W14)) if rng.random() < 0.02 else 0
            if p + skip + ln > stop:
                break
            p += skip
            beg.append(p)
            end.append(p + ln)
            p += ln
        if k < len(special):
            if len(beg) < n:
                beg.append(special[k][0])
                end.append(special[k][1])
            p = special[k][1]
    while len(beg) < n:                                                 # (a stretch was too short for its share)
        beg.append(p)
        end.append(p + 1)
        p += 1
    return np.asarray(beg, np.int64), np.asarray(end, np.int64)


def _index_inputs(rng, n):
    beg, end = _index_lines(rng, n)
    assert beg.size == n and np.all(beg[1:] >= end[:-1]) and np.all(end > beg)
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 400, n))]).astype(np.int64)
    nm = -(-int(off[-1]) // BGZF_BLOCK)
    foff = np.concatenate([[0], np.cumsum(rng.integers(100, 30_000, nm))]).astype(np.int64)
    return beg, end, off, foff


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 4097, 9000])
def test_index_runs_and_windows(eng, n):
    """(4,097 and 9,000 lines: more than one workgroup of the head-flag scan)"""
    rng = np.random.Generator(np.random.PCG64(n))
    beg, end, off, foff = _index_inputs(rng, n)
    if n >= 257:
        assert all(np.any((beg < b) & (end > b)) for b in BORDERS) and np.any(((end - 1) >> 14) - (beg >> 14) >= 40)
        assert np.any((beg[1:] >> 14) - ((end[:-1] - 1) >> 14) >= 2)    # a window no line overlaps
    u0 = 1234
    got = eng.lines_index(_dev(beg), _dev(end), _dev(off + u0), u0, _dev(foff))
    exp = W.lines_index(beg, end, off, foff)
    for k in ("run_bin", "run_vbeg", "run_vend", "win_min"):
        assert np.array_equal(got[k], exp[k]), k
    assert got["w0"] == exp["w0"] and got["run_bin"].dtype == np.int32 and got["win_min"].dtype == np.uint64
    if n >= 257:
        assert np.any(exp["win_min"] == W.BIG) and exp["run_bin"].size < n and len(set(exp["run_bin"].tolist())) < exp["run_bin"].size


def test_index_refuses_ends_that_do_not_ascend(eng):
    rng = np.random.Generator(np.random.PCG64(4))
    beg, end, off, foff = _index_inputs(rng, 300)
    end[100] = end[101] + 5
    with pytest.raises(ValueError, match="ends do not ascend"):
        eng.lines_index(_dev(beg), _dev(end), _dev(off), 0, _dev(foff))
    beg, end, off, foff = _index_inputs(rng, 900)
    assert foff.size >= 3
    with pytest.raises(ValueError, match="do not fit the members"):
        eng.lines_index(_dev(beg), _dev(end), _dev(off), 0, _dev(foff[:-1]))


# ------------------------------------------------------------------ end to end
def _files(vdir):
    return {f: open(os.path.join(str(vdir), f), "rb").read() for f in sorted(os.listdir(str(vdir))) if not os.path.isdir(os.path.join(str(vdir), f))}


def _check_own_index(gpath, contigs):
    """the .csi beside gpath == vcfio.csi_bytes, the per-record writer, on the file's own virtual offsets"""
    raw = open(gpath, "rb").read()
    hdr, recs = vcfio.read_vcf_gz(gpath)
    keys = [gvcf.parse_line(ln) for ln in recs]
    tid = np.array([contigs.index(k[0]) for k in keys])
    beg = np.array([k[1] - 1 for k in keys], np.int64)
    end = beg + np.array([k[2] for k in keys], np.int64)
    vb, ve = W.file_voffsets(raw, len("".join(hdr).encode()), [len(ln.encode()) for ln in recs])
    assert gzip.decompress(open(gpath + ".csi", "rb").read()) == vcfio.csi_bytes(contigs, tid, beg, end, vb, ve)
    assert W.inflate_members(raw)[0] == gzip.decompress(raw)
    return recs


def test_call_manager_with_the_device_writer_writes_the_host_writers_gvcf(eng, tmp_path):
    from nanocaller_amd import snpCaller
    from tests import gvcf_ref as R
    from tests.test_gvcf_gpu import _manager_params
    from tests.test_vcfio import _parse_csi, _read_range, _reg2bins
    from tests.util import load_world
    world = load_world("deep")
    regions = [(world.chrom, 1_000, 23_000, "diploid")]
    files = {}
    for tag in ("host", "device"):
        vdir = tmp_path / tag
        vdir.mkdir()
        p = _manager_params(world, regions, vdir, gvcf=True, gvcf_writer=tag)
        snpCaller.call_manager(p)
        files[tag] = _files(vdir)
    assert sorted(files["device"]) == sorted(files["host"]) and len(files["host"]) == 6
    for f in files["host"]:
        if ".g.vcf" not in f:
            assert files["device"][f] == files["host"][f], f
    assert gzip.decompress(files["device"]["t.snps.g.vcf.gz"]) == gzip.decompress(files["host"]["t.snps.g.vcf.gz"])
    inter = os.listdir(os.path.join(str(tmp_path / "device"), "intermediate_snp_files"))
    assert "t.1.snps.g.vcf" not in inter and "t.1.snps.g.vcf.bgzf" in inter and "t.1.snps.g.vcf.bgzf.npz" in inter
    assert "t.1.snps.g.vcf" in os.listdir(os.path.join(str(tmp_path / "host"), "intermediate_snp_files"))
    gpath = os.path.join(str(tmp_path / "device"), "t.snps.g.vcf.gz")
    recs = _check_own_index(gpath, [world.chrom])
    # the longest block's region query, as test_gvcf_gpu.py asks it of the host writer's file
    blocks = [R.parse_block(ln)[:2] + (ln,) for ln in recs if "\t<*>\t" in ln]
    s, e, line = max(blocks, key=lambda b: b[1] - b[0])
    mid = (s + e) // 2
    raw = files["device"]["t.snps.g.vcf.gz"]
    idx = _parse_csi(gzip.decompress(files["device"]["t.snps.g.vcf.gz.csi"]))
    found = []
    for x in _reg2bins(mid - 1, mid, 14, 5):
        for cb, ce in idx["refs"][0].get(x, (0, []))[1]:
            for rec in _read_range(raw, cb, ce).decode().splitlines(keepends=True):
                if "\t<*>\t" in rec:
                    bs, be = R.parse_block(rec)[:2]
                    if bs <= mid <= be:
                        found.append(rec)
    assert set(found) == {line} and len(blocks) > 300


def test_device_writer_on_a_bam_with_a_haploid_stretch_and_a_second_contig(eng, tmp_path):
    """diploid / haploid / diploid on one contig -- the diploid group's two runs of chunks become two pieces, the haploid group's piece goes between
    them -- and a second contig"""
    from nanocaller_amd import snpCaller
    from tests import bamio
    from tests.test_gvcf_gpu import _manager_params
    w1, w2 = bamio.make_bam_world(seed=9, length=40_000, depth=22), bamio.make_bam_world(seed=10, length=12_000, depth=18)
    rng = np.random.Generator(np.random.PCG64(2))
    bam, fa = str(tmp_path / "s.bam"), str(tmp_path / "r.fa")
    recs = bamio.world_to_records(w1, rng) + [dict(r, tid=1) for r in bamio.world_to_records(w2, rng)]
    bamio.write_bam(bam, "c1", w1.length, recs, other_refs=[("c2", w2.length)])
    bamio.write_fasta(fa, "c1", w1.ref, extra=[("c2", w2.ref)])
    regions = [("c1", 2_000, 14_000, "diploid"), ("c1", 14_001, 26_000, "haploid"), ("c1", 26_001, 38_000, "diploid"), ("c2", 1_000, 11_000, "diploid")]
    outs = {}
    for tag in ("host", "device"):
        vdir = tmp_path / tag
        vdir.mkdir()
        p = dict(_manager_params(bam, regions, vdir, gvcf=True, gvcf_writer=tag), fasta_path=fa)
        snpCaller.call_manager(p)
        outs[tag] = _files(vdir)
    assert gzip.decompress(outs["device"]["t.snps.g.vcf.gz"]) == gzip.decompress(outs["host"]["t.snps.g.vcf.gz"])
    for f in outs["host"]:
        if ".g.vcf" not in f:
            assert outs["device"][f] == outs["host"][f], f
    recs = _check_own_index(os.path.join(str(tmp_path / "device"), "t.snps.g.vcf.gz"), ["c1", "c2"])
    pieces = gvcf.load_pieces(os.path.join(str(tmp_path / "device"), "intermediate_snp_files", "t.1.snps.g.vcf.bgzf.npz"), "")
    assert [(q["contig"], q["first"] <= 14_000, q["last"]) for q in pieces if q["contig"] == "c1"][:2] == [("c1", True, 14_000), ("c1", False, 38_000)]
    assert len(pieces) == 4 and sum(q["lines"] for q in pieces) == len(recs) > 300
    hap = [ln for ln in recs if ln.startswith("c1\t") and 14_001 <= int(ln.split("\t")[1]) <= 26_000 and "\t<*>\t" in ln]
    assert hap and all(ln.rstrip("\n").split("\t")[9].split(":")[0] in ("0", ".") for ln in hap)


def test_an_unknown_writer_is_refused(eng, tmp_path):
    from nanocaller_amd import snpCaller
    from tests.test_gvcf_gpu import _manager_params
    from tests.util import load_world
    world = load_world("deep")
    p = _manager_params(world, [(world.chrom, 1_000, 5_000, "diploid")], tmp_path, gvcf=True, gvcf_writer="gpu")
    with pytest.raises(ValueError, match="gvcf_writer"):
        snpCaller.call_manager(p)
    assert not os.path.exists(os.path.join(str(tmp_path), "t.snps.vcf.gz"))
    # ... and is not read when the gVCF is off
    snpCaller.call_manager(dict(p, gvcf=False))
    assert os.path.exists(os.path.join(str(tmp_path), "t.snps.vcf.gz")) and not os.path.exists(os.path.join(str(tmp_path), "t.snps.g.vcf.gz"))

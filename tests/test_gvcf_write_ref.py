"""The host half of the gVCF's device writer without a GPU: hts_index.csi_from_summaries over pieces against
vcfio.csi_bytes, the per-record writer, fed with the file's own virtual offsets; gvcf.merge_pieces on host-made pieces against
gvcf.merge_worker_files on the same lines.  The pieces and their summaries come from tests/gvcf_write_ref.py."""
import gzip
import io
import os

import numpy as np
import pytest

from nanocaller_amd import gvcf, hts_index, vcfio
from nanocaller_amd.bgzf import BGZF_EOF
from tests import gvcf_write_ref as W

SEEDS = list(range(24))
NAMES = ["cA", "cEmpty", "cB"]
W14 = 1 << 14


def _contig_lines(rng, start, n, long_at=None):
    """n non-overlapping intervals in position order the way a gVCF has them: blocks of 1 to 3,000 columns, single-column records between
    them, now and then a stretch nothing covers (longer than a window), one block of more than 40 windows at `long_at`"""
    beg, end, p = [], [], start
    for k in range(n):
        if k == long_at:
            ln = 41 * W14 + int(rng.integers(0, 5000))
        elif rng.random() < 0.35:
            ln = 1
        else:
            ln = int(rng.integers(1, 3000))
        if rng.random() < 0.04:
            p += int(rng.integers(W14 + 1, 5 * W14))
        beg.append(p)
        end.append(p + ln)
        p += ln
    return np.asarray(beg, np.int64), np.asarray(end, np.int64)


def _case(seed):
    """three contigs (the middle one without lines), 1 to 5 pieces per contig; the split points of cA take one border inside a run of one bin
    and one where the bin changes whenever it has three pieces or more"""
    rng = np.random.Generator(np.random.PCG64(seed))
    contigs = []
    for tid, (start, n) in ((0, (int(rng.integers(0, 3000)), int(rng.integers(150, 400)))), (2, (3 * W14 + int(rng.integers(0, 9000)), int(rng.integers(40, 200))))):
        beg, end = _contig_lines(rng, start, n, long_at=int(rng.integers(0, n)) if tid == 0 else None)
        lines = [bytes(rng.integers(97, 123, int(rng.integers(20, 120))).astype(np.uint8)) + b"\n" for _ in range(n)]
        bins = np.array([W.reg2bin(int(b), int(e)) for b, e in zip(beg, end)])
        k = int(rng.integers(1, 6))
        same, diff = np.flatnonzero(bins[1:] == bins[:-1]) + 1, np.flatnonzero(bins[1:] != bins[:-1]) + 1
        cuts = set(rng.choice(np.arange(1, n), k - 1, replace=False).tolist()) if k > 1 else set()
        if tid == 0 and k >= 3:
            cuts = set(list(cuts)[:k - 3]) | {int(rng.choice(same)), int(rng.choice(diff))}
        edges = [0] + sorted(cuts) + [n]
        contigs.append(dict(tid=tid, beg=beg, end=end, lines=lines, bins=bins, edges=edges))
    return contigs


def _build(contigs, header=b"##fileformat=VCFv4.2\n#CHROM\n"):
    """the file (header members, the pieces, EOF) and the pieces' summaries per reference"""
    f = io.BytesIO()
    head, _ = W.members(header)
    f.write(head)
    per_ref = [[] for _ in NAMES]
    for c in contigs:
        for a, b in zip(c["edges"], c["edges"][1:]):
            at = f.tell()
            s = W.write_piece(f, c["lines"][a:b], c["beg"][a:b], c["end"][a:b])
            per_ref[c["tid"]].append(dict(s, offset=at))
    f.write(BGZF_EOF)
    return f.getvalue(), per_ref, len(header)


@pytest.fixture(scope="module")
def cases():
    return [_case(s) for s in SEEDS]


def _records(contigs):
    tid = np.concatenate([np.full(c["beg"].size, c["tid"]) for c in contigs])
    return tid, np.concatenate([c["beg"] for c in contigs]), np.concatenate([c["end"] for c in contigs]), [len(x) for c in contigs for x in c["lines"]]


def _sharp(cases):
    """what the comparison needs its inputs to hold, asserted on the inputs and the per-record reductions alone"""
    multi = merged = unmerged = empty_first = wide = 0
    for contigs in cases:
        for c in contigs:
            beg, end, bins = c["beg"], c["end"], c["bins"]
            vb = np.arange(beg.size, dtype=np.uint64)                   # consecutive lines: line i occupies [i, i + 1)
            ub, _, n_ch, _, _ = hts_index.bin_chunks(bins, vb, vb + np.uint64(1))
            # a leaf bin's parent holds the lines that straddle its 16 kb borders: runs of it, each between two runs of leaves
            multi += int((n_ch >= 2).sum())
            for e in c["edges"][1:-1]:
                merged += int(bins[e] == bins[e - 1])
                unmerged += int(bins[e] != bins[e - 1])
            lin = hts_index.linear_index(beg, end, vb, 14)
            first = hts_index.bin_first_window(ub, 5)
            empty_first += int(np.count_nonzero(lin[np.minimum(first, lin.size - 1)] == hts_index._BIG))
            wide += int(np.count_nonzero(((end - 1) >> 14) - (beg >> 14) + 1 >= 40))
    assert multi >= len(cases) and merged >= 3 and unmerged >= 3 and empty_first >= len(cases) and wide >= len(cases), (multi, merged, unmerged, empty_first, wide)
    assert {len(c["edges"]) - 1 for contigs in cases for c in contigs} == {1, 2, 3, 4, 5}


def test_index_from_summaries_equals_the_per_record_writer(cases):
    _sharp(cases)
    assert len(cases) >= 20
    for contigs in cases:
        raw, per_ref, hl = _build(contigs)
        tid, beg, end, line_len = _records(contigs)
        vb, ve = W.file_voffsets(raw, hl, line_len)
        want = vcfio.csi_bytes(NAMES, tid, beg, end, vb, ve)
        got = hts_index.csi_from_summaries(len(NAMES), per_ref, aux=vcfio.tabix_aux(NAMES))
        assert got == want
        text = gzip.decompress(raw)
        assert text[hl:] == b"".join(x for c in contigs for x in c["lines"])


def test_index_bytes_is_its_two_halves():
    """reference_summary + summary_bytes is what index_bytes writes, .bai and .csi (the split changes no byte: test_vcfio pins the .csi)"""
    contigs = _case(3)
    tid, beg, end, line_len = _records(contigs)
    raw, _, hl = _build(contigs)
    vb, ve = W.file_voffsets(raw, hl, line_len)
    for fmt in ("csi", "bai"):
        whole = hts_index.index_bytes(fmt, 3, tid, beg, end, np.zeros(tid.size, bool), None, vb, ve)
        parts = []
        for r in range(3):
            m = tid == r
            s = hts_index.reference_summary(beg[m], end[m], np.zeros(int(m.sum()), bool), hts_index.reg2bin(beg[m], end[m]), vb[m], ve[m]) if m.any() else None
            parts.append(hts_index.summary_bytes(fmt, s))
        assert b"".join(parts) in whole and len(whole) - len(b"".join(parts)) == (16 if fmt == "bai" else 28)


# ------------------------------------------------------------------ concatenation against the Python merge
def _variant(chrom, pos, k):
    return "%s\t%d\t.\tA\tG\t%d.5\tPASS\tPR=0.1,0.2,0.3,0.4;FQ=0.5\tGT:DP:VF\t0/1:%d:0.5\n" % (chrom, pos, 20 + k % 30, 10 + k % 7)


def _group_lines(rng, chrom, spans, haploid):
    """the lines of one (contig, ploidy) group in position order: blocks cut at records, over the group's chunk intervals
    -> [(1-based position, reference length the index covers, line)]"""
    out, k = [], 0
    for s, e in spans:
        p = s
        while p <= e:
            k += 1
            if rng.random() < 0.3:
                out.append((p, 1, _variant(chrom, p, k)))
                if rng.random() < 0.2:                                  # two records on one position keep their order
                    out.append((p, 1, _variant(chrom, p, k + 1)))
                p += 1
            else:
                q = min(e, p + int(rng.integers(0, 900)))
                out.append((p, q - p + 1, gvcf.block_line(chrom, p, q, "AGTC"[k % 4], 10 + k % 9, 30 + k % 60, 12, 0, gvcf.constants(), haploid)))
                p = q + 1
    return out


def _layout(tmp_path, shift_piece=None):
    """two workers; c1 is diploid / haploid / diploid (worker 1 holds the diploid group: two runs of chunks, worker 2 the haploid stretch between
    them), c2 is split between the workers.  Host side: the plain worker files as caller() writes them (group after group); device side: one
    piece per run of chunks, through gvcf.PieceFile.  -> (plain files, piece files)"""
    rng = np.random.Generator(np.random.PCG64(77))
    groups = {1: [("c1", False, [(1, 20_000), (20_001, 70_000), (150_001, 260_000)]), ("c2", False, [(5_000, 90_000)])],
              2: [("c1", True, [(70_001, 110_000), (110_001, 150_000)]), ("c2", False, [(90_001, 131_072), (131_073, 200_000)])]}
    plain, piece_files = [], []
    for wk, grps in groups.items():
        pp, bp = str(tmp_path / ("t.%d.snps.g.vcf" % wk)), str(tmp_path / ("t.%d.snps.g.vcf.bgzf" % wk))
        with open(pp, "w") as f, gvcf.PieceFile(bp) as out:
            for chrom, haploid, spans in grps:
                lines = _group_lines(rng, chrom, spans, haploid)
                f.write("".join(x[2] for x in lines))
                for s, e in gvcf.chunk_runs(spans):
                    mine = [x for x in lines if s <= x[0] <= e]
                    beg = np.array([x[0] - 1 for x in mine], np.int64)
                    end = beg + np.array([x[1] for x in mine], np.int64)
                    piece = W.write_piece(out, [x[2].encode() for x in mine], beg, end)
                    first = int(beg[0]) + 1 if (chrom, s) != shift_piece else int(beg[0]) + 1 - 30_000
                    out.add(piece, chrom, first, int(end[-1]))
        plain.append(pp)
        piece_files.append(bp)
    assert [len(gvcf.chunk_runs(s)) for g in groups.values() for _, _, s in g] == [2, 1, 1, 1]
    return plain, piece_files


def test_concatenated_pieces_inflate_to_what_the_python_merge_writes(tmp_path):
    plain, piece_files = _layout(tmp_path)
    contigs = ["c1", "c2", "c3"]
    host, dev = str(tmp_path / "host.g.vcf.gz"), str(tmp_path / "dev.g.vcf.gz")
    n_host = gvcf.merge_worker_files(plain, host, contigs, "S")
    n_dev = gvcf.merge_pieces(piece_files, dev, contigs, "S")
    want = gzip.decompress(open(host, "rb").read())
    raw = open(dev, "rb").read()
    assert n_dev == n_host > 500 and gzip.decompress(raw) == want
    assert raw.endswith(BGZF_EOF) and raw.count(BGZF_EOF) == 1
    # the index is the per-record writer's on the file's own offsets
    hdr, recs = vcfio.read_vcf_gz(dev)
    keys = [gvcf.parse_line(ln) for ln in recs]
    tid = np.array([contigs.index(k[0]) for k in keys])
    beg = np.array([k[1] - 1 for k in keys], np.int64)
    end = beg + np.array([k[2] for k in keys], np.int64)
    assert np.all(np.diff(tid) >= 0) and all(np.all(np.diff(beg[tid == r]) >= 0) for r in range(3))
    vb, ve = W.file_voffsets(raw, len("".join(hdr).encode()), [len(ln.encode()) for ln in recs])
    assert gzip.decompress(open(dev + ".csi", "rb").read()) == vcfio.csi_bytes(contigs, tid, beg, end, vb, ve)
    # the header has members of its own: the first piece starts a member
    assert W.inflate_members(raw)[0] == want and (vb[0] & np.uint64(0xffff)) == 0


def test_overlapping_pieces_are_refused(tmp_path):
    _, piece_files = _layout(tmp_path, shift_piece=("c1", 150_001))
    out = str(tmp_path / "dev.g.vcf.gz")
    with pytest.raises(ValueError, match=r"c1:70001-150000 .* and c1:120001-260000 .* overlap"):
        gvcf.merge_pieces(piece_files, out, ["c1", "c2"], "S")
    assert not os.path.exists(out)


def test_a_contig_the_header_does_not_name_is_refused(tmp_path):
    _, piece_files = _layout(tmp_path)
    with pytest.raises(ValueError, match="c2"):
        gvcf.merge_pieces(piece_files, str(tmp_path / "dev.g.vcf.gz"), ["c1"], "S")


def test_writer_option(monkeypatch):
    monkeypatch.delenv("NC_GVCF_WRITER", raising=False)
    assert gvcf.writer({}) == "host" and gvcf.writer(dict(gvcf_writer="host")) == "host" and gvcf.writer(dict(gvcf_writer="device")) == "device"
    monkeypatch.setenv("NC_GVCF_WRITER", "device")
    assert gvcf.writer({}) == "device" and gvcf.writer(dict(gvcf_writer="host")) == "host"
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError):
            gvcf.writer(dict(gvcf_writer=bad))
    monkeypatch.setenv("NC_GVCF_WRITER", "fast")
    with pytest.raises(ValueError):
        gvcf.writer({})


def test_variant_lines_and_chunk_runs():
    text = (_variant("c1", 5, 1) + "c1\t9\t.\tACGT\tA\t1\t.\t.\tGT\t0/1\n").encode()
    off, ref_len = gvcf.variant_lines(np.frombuffer(text, np.uint8))
    assert off.tolist() == [0, len(_variant("c1", 5, 1)), len(text)] and ref_len.tolist() == [1, 4]
    assert gvcf.chunk_runs([(11, 20), (1, 10), (30, 40), (35, 50), (52, 60)]) == [(1, 20), (30, 50), (52, 60)]

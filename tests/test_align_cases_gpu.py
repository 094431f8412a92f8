"""The device aligners of csrc/nc_msa.hip on the tie-heavy cases of tests/align_cases.py, one lane layout per call: the 16-lane register kernels
k_nw_fill16<4 | 8 | 11 | 17> with k_nw_trace16 / k_allele_trace16, and the lane-per-read pair k_nw_fill / k_nw_trace, against the host C++
(which tests/test_align_cases_ref.py ties to the Python restatement on the same cases) and against the reference's own allele_prediction.
The route a call takes follows from its longest window alone (nc_star_msa_tensor_dup, nc_allele_prediction_device): that bound is asserted.

What the tests notice, measured once on an MI355X with three one-line changes (each built apart, never committed):
  k_nw_fill16, extension flag `e_ext >= e_open` -> `>`:   the star calls cpl4 and cpl8, all three other scorings, the allele calls cpl4 and cpl8 fail
                                                          (under 25 / 1 an opening equals an extension on few paths: the scorings with open == extend
                                                          carry that rule for every layout)
  k_nw_fill16, `e > d` -> `e >= d` (diagonal against E):  every star call of the four register layouts, the lane-per-read comparison, the duplicates,
                                                          the other scorings, the allele calls cpl4 - cpl17 and the band-off tuples fail
  k_fill16q, d_1 and d_2 swapped on their way into acc:   every pipeline test fails (band off, band on through its re-runs, short windows, all
                                                          scoring corners); the nc_msa.hip tests pass, as they must
The two older uniform-random tests (test_indel_pass2.py: device star alignment, device allele prediction) also fail under the first two changes
-- their thousands of random pairs do meet both ties -- and pass under the third, which only the tests below reach."""
import numpy as np
import pytest

from nanocaller_amd import generate_indel_pileups as gip

import align_cases as ac
from test_align_cases_ref import allele_gold

pytestmark = pytest.mark.gpu

SYM = "AGTC-N"
_host = {}


def _engine():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


def _route(refs):
    n2 = max(len(w) for w in refs)
    return next(cls for cls, (lo, hi) in ac.BOUNDS.items() if lo <= n2 <= hi)


def _host_rows(sets, refs, scoring=None):
    """gip.star_aligner per set; a read base N is kept by the host aligner (for its caller to refuse) and is a gap on the device (sym_code,
    nc_msa.hip): compared as a gap"""
    key = (id(sets), scoring)
    if key not in _host:
        out = []
        for rd, w in zip(sets, refs):
            rows, rr = gip.star_aligner(["r%d" % k for k in range(len(rd))], rd, w, *(scoring or ()))
            out.append(([r.replace("N", "-") for r in rows], rr))
        _host[key] = (sets, out)                                                     # (keeps `sets` alive: its id is the key)
    return _host[key][1]


def _check_star(eng, sets, refs, got, scoring=None, tensors=True):
    x, cns, ncols, rows, rrs = got
    want = _host_rows(sets, refs, scoring)
    n = 0
    for s in range(len(sets)):
        hrows, hrr = want[s]
        assert "".join(SYM[c] for c in rrs[s]) == hrr, s
        assert ["".join(SYM[c] for c in row) for row in rows[s]] == hrows, (s, len(refs[s]))
        assert int(ncols[s]) == len(hrr)
        n += len(hrows)
    if tensors:                                                                      # x / cns: the rows -> tensor kernel on the host's rows
        import torch
        keep = [s for s in range(len(sets)) if sets[s]]
        code = {c: k for k, c in enumerate("AGTC-")}
        hr = [np.array([[code[c] for c in row] for row in want[s][0]], np.uint8) for s in keep]
        hrr = [np.array([code[c] for c in want[s][1]], np.uint8) for s in keep]
        x2, cns2 = eng.indel_tensor(hr, hrr)
        assert torch.equal(x[keep], x2)
        for k, s in enumerate(keep):
            assert np.array_equal(cns[s], cns2[k]), s
    return n


def _low(call):
    """the sets of a call whose window is the class's shortest: a call of its own, its longest window right above the previous route's bound"""
    lo = ac.BOUNDS[call.cls][0]
    keep = [s for s, w in enumerate(call.refs) if len(w) == lo]
    return [call.sets[s] for s in keep], [call.refs[s] for s in keep]


@pytest.mark.parametrize("name", list(ac.star_calls()))
def test_star_alignment_of_every_layout_equals_the_host(name, monkeypatch):
    monkeypatch.delenv("NC_MSA_LANE_PER_READ", raising=False)
    eng = _engine()
    c = ac.star_calls()[name]
    assert _route(c.refs) == c.cls and max(len(w) for w in c.refs) == ac.CLASSES[c.cls][-1]      # 64, 128, 176, 272 run <4>, <8>, <11>, <17>; 300 one lane per read
    n = _check_star(eng, c.sets, c.refs, eng.star_msa_tensor(c.sets, c.refs, want_rows=True))
    assert n >= 20
    if c.cls != "cpl4" and not name.endswith("_mix"):
        sets, refs = _low(c)
        assert _route(refs) == c.cls and max(len(w) for w in refs) == ac.BOUNDS[c.cls][0] and sum(len(rd) for rd in sets) >= 8      # 65, 129, 177, 273
        _check_star(eng, sets, refs, eng.star_msa_tensor(sets, refs, want_rows=True))


def test_lane_per_read_route_gives_the_register_routes_results(monkeypatch):
    """k_nw_fill / k_nw_trace where the register kernel would run (NC_MSA_LANE_PER_READ): the same rows, tensors and consensus"""
    import torch
    eng = _engine()
    for name in ("cpl11", "cpl4_mix"):
        c = ac.star_calls()[name]
        monkeypatch.delenv("NC_MSA_LANE_PER_READ", raising=False)
        fast = eng.star_msa_tensor(c.sets, c.refs, want_rows=True)
        monkeypatch.setenv("NC_MSA_LANE_PER_READ", "1")
        slow = eng.star_msa_tensor(c.sets, c.refs, want_rows=True)
        monkeypatch.delenv("NC_MSA_LANE_PER_READ")
        _check_star(eng, c.sets, c.refs, slow)
        keep = [s for s in range(len(c.sets)) if c.sets[s]]                          # (a set without reads has no tensor: 0 / 0)
        assert torch.equal(fast[0][keep], slow[0][keep]) and np.array_equal(fast[2], slow[2])
        assert all(np.array_equal(a, b) for a, b in zip(fast[1], slow[1])) and all(np.array_equal(a, b) for a, b in zip(fast[3], slow[3]))


def test_repeated_alignments_are_read_from_the_first_one():
    """al_dup: after every set the same window again with every other read of it -- a third of the alignments repeat an earlier one and are not
    computed; the results are those of the plain call"""
    import torch
    eng = _engine()
    c = ac.star_calls()["cpl11"]
    sets, refs, dup, a0 = [], [], [], 0
    for rd, w in zip(c.sets, c.refs):
        sets += [rd, rd[::2]]
        refs += [w, w]
        dup += [-1] * len(rd) + [a0 + 2 * k for k in range(len(rd[::2]))]
        a0 += len(rd) + len(rd[::2])
    dup = np.array(dup, np.int32)
    assert 0.3 < (dup >= 0).mean() < 0.45
    flat = [q for rd in sets for q in rd]
    read_off = np.zeros(len(flat) + 1, np.int32)
    np.cumsum([len(q) for q in flat], out=read_off[1:])
    set0 = np.zeros(len(sets) + 1, np.int32)
    np.cumsum([len(rd) for rd in sets], out=set0[1:])
    ref_off = np.zeros(len(refs) + 1, np.int32)
    np.cumsum([len(w) for w in refs], out=ref_off[1:])
    mc = max(len(w) + sum(len(q) for q in rd) for rd, w in zip(sets, refs))
    args = (len(sets), "".join(flat).encode(), read_off, set0, "".join(refs).encode(), ref_off, mc)
    x0, cns0, nc0 = eng.star_msa_tensor_flat(*args)
    x1, cns1, nc1 = eng.star_msa_tensor_flat(*args, al_dup=dup)
    keep = [s for s in range(len(sets)) if sets[s]]                                  # (a set without reads has no tensor: 0 / 0)
    assert torch.equal(x0[keep], x1[keep]) and np.array_equal(nc0, nc1) and all(np.array_equal(a, b) for a, b in zip(cns0, cns1))
    full = eng.star_msa_tensor(sets, refs, want_rows=True)                           # and the plain call is the host's
    _check_star(eng, sets, refs, full, tensors=False)
    assert torch.equal(full[0][keep], x0[keep])


@pytest.mark.parametrize("scoring", [(9, 1, 20, -10), (7, 7, 20, -10), (0, 0, 100, -100)])
def test_star_alignment_under_other_scorings(scoring, monkeypatch):
    """parasail's scoring, and gap opening == extension: there an opening and an extension tie at every gap cell"""
    monkeypatch.delenv("NC_MSA_LANE_PER_READ", raising=False)
    eng = _engine()
    kw = dict(zip(("open_", "extend", "match", "mismatch"), scoring))
    for name in ("cpl8", "cpl4_mix", "cpl11_mix", "cpl17_mix", "lane_mix"):          # every layout
        c = ac.star_calls()[name]
        _check_star(eng, c.sets, c.refs, eng.star_msa_tensor(c.sets, c.refs, want_rows=True, **kw), scoring=scoring, tensors=False)


@pytest.mark.parametrize("name", list(ac.allele_calls()))
def test_device_allele_prediction_on_the_tie_pairs(name):
    """nc_allele_prediction_device per layout == the reference's answer == the host batch; an empty string, a consensus over 1,000 bases and a
    window over 272 bases make the device call refuse the batch, and the host fallback returns the same"""
    from nanocaller_amd import _lib
    eng = _engine()
    alts, refs, mrs = ac.allele_calls()[name]
    want = [(r[3], r[4]) for r in allele_gold()[name]]
    assert [r[:3] for r in allele_gold()[name]] == [[a, r, m] for a, r, m in zip(alts, refs, mrs)]
    assert gip.allele_prediction_batch(alts, refs, mrs, eng=eng) == want
    assert gip.allele_prediction_batch(alts, refs, mrs) == want
    # which route: the device call itself accepts the batch, or answers NC_ERR_CAPACITY
    n = len(alts)
    aoff, roff = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    np.cumsum([len(a) for a in alts], out=aoff[1:])
    np.cumsum([len(r) for r in refs], out=roff[1:])
    mr, rl, al = np.ascontiguousarray(mrs, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
    rc = eng.L.nc_allele_prediction_device(eng.ctx, n, "".join(alts).encode(), _lib.npp(aoff), "".join(refs).encode(), _lib.npp(roff), _lib.npp(mr),
                                           _lib.npp(rl), _lib.npp(al))
    if name.startswith("fb_"):
        assert rc == _lib.NC_ERR_CAPACITY
    else:
        assert rc == _lib.NC_OK and _route(refs) == name and max(len(r) for r in refs) == ac.CLASSES[name][-1]
        assert [(None, None) if r < 0 else (w[:r], a[:k]) for w, a, r, k in zip(refs, alts, rl.tolist(), al.tolist())] == want


# ---------------------------------------------------------------------------------------------------- the packed kernels of the device pipeline
# csrc/nc_pipe_align.hip (k_fill16q<4 | 8 | 11 | 17>: two alignments per register in 16-bit arithmetic, the traceback code from four sign bits;
# k_fill_band<1 | 2> on 32 / 64 diagonals) and nc_pipe_trace.hip on a small world of runs and repeats (align_cases.tie_world): every site against
# the oracle's restatement, band on and band off, at the production windows, at windows short enough for the <4> and <8> templates, and under
# the scorings at the corners of what nc_indel_sites_scoring accepts.
PIPE = dict(mincov=4, maxcov=160, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6)
CHROM = "chrT"


@pytest.fixture(scope="module")
def tie_files(tmp_path_factory):
    import bamio
    ref, recs, feats = ac.tie_world()
    d = tmp_path_factory.mktemp("ties")
    bam, fa = str(d / "t.bam"), str(d / "t.fa")
    bamio.write_bam(bam, CHROM, len(ref), recs)
    bamio.write_fasta(fa, CHROM, ref)
    return ref, recs, bam, fa


def _dct(fa, **kw):
    d = dict(PIPE, seq="ont", fasta_path=fa, supplementary=False, exclude_bed=None, impute_indel_phase=False)
    d.update(kw)
    return d


def _device_sites(files, *, window_after=160, haploid=False, band=None, scoring=None):
    """the device pipeline on the whole contig -> (result of gip.indel_sites_device, its band statistics: alignments on 32 / 64 diagonals, on the
    full matrix by width, re-run after an edge touch)"""
    from nanocaller_amd import _lib
    ref, recs, bam, fa = files
    chunks = [dict(chrom=CHROM, start=1, end=len(ref), sam_path=bam)]
    eng, dp, reads_c, ctg, excl, mates = gip.indel_pack_for(_dct(fa), chunks, 0, by_name=True)
    assert eng.L.nc_indel_sites_band(eng.ctx, -1 if band is None else int(band), 0) == 0
    try:
        r = gip.indel_sites_device(eng, dp, reads_c, len(ctg["fasta"]), [(1, len(ref))], window_after=window_after, haploid=haploid, excl=excl,
                                   mates=mates, scoring=scoring, **PIPE)
        st = np.zeros(6, np.int64)
        assert eng.L.nc_indel_sites_band_stats(eng.ctx, _lib.npp(st)) == 0
    finally:
        eng.L.nc_indel_sites_band(eng.ctx, -1, 0)
        eng.L.nc_indel_sites_scoring(eng.ctx, *[int(v) for v in _lib.STAR_SCORING])
    return r, st


def _sites_equal_the_oracle(files, r, window_after, haploid, band, scoring=None):
    """EVERY site of the run: tensor bit for bit, phase, REF / ALT.  -> Counter of how the oracle aligned the sites' windows"""
    import collections
    import oracle_pool
    from util import device_alleles, oracle_alleles
    ref, recs, bam, fa = files
    beg = np.array([rc["pos0"] + 1 for rc in recs])
    end = beg + np.array([sum(n for op, n in rc["cigar"] if op in "MDN=X") for rc in recs])
    hap = np.array([rc["tags"].get("HP", 0) for rc in recs])
    ps = np.array([rc["tags"].get("PS", 0) for rc in recs])
    tasks = []
    for p in r["pos"].tolist():
        ids = np.nonzero((beg <= p) & (end > p))[0]
        tasks.append(oracle_pool.site_task(p, [recs[i] for i in ids], hap[ids], ps[ids], ref, window_after, PIPE["mincov"], PIPE["maxcov"],
                                           haploid=haploid, band=band, scoring=scoring))
    got = oracle_pool.map_sites(tasks)
    S = 1 if haploid else 3
    x = r["x"].cpu().numpy()
    how, bad = collections.Counter(), []
    for k, o in enumerate(got):
        p = int(r["pos"][k])
        assert o is not None, p
        ok = (np.array_equal(x[k].reshape(S, 5, 128, 2), o["x"]) and o["phase"] == int(r["phase"][k])
              and device_alleles(r, k) == oracle_alleles(o["cns"], o["win"], int(r["type"][k])))
        if not ok:
            bad.append(p)
        how.update(o["how"] if band else ["full"] * len(o["reads"]))
    assert not bad, "%d of %d sites differ from the oracle: %s" % (len(bad), len(got), bad[:12])
    return how


@pytest.mark.parametrize("variant", ["ont", "pacbio", "haploid"])
def test_tie_world_band_off_returns_the_host_routes_tuples(tie_files, variant, monkeypatch):
    """k_fill16q<11> (ONT, 161-base windows) / <17> (PacBio, 261) on the full matrix == the host-assembled route (nc_star_msa), tuple by tuple"""
    from test_indel_pipeline import _same_tuples
    ref, recs, bam, fa = tie_files
    dct = _dct(fa, seq="pacbio" if variant == "pacbio" else "ont")
    chunks = [dict(chrom=CHROM, start=s, end=min(len(ref), s + 2_999), sam_path=bam) for s in range(1, len(ref), 3_000)]
    gip._CONTIGS.clear()
    monkeypatch.setenv("NC_PIPE_BAND", "0")
    exp = gip.get_indel_testing_candidates_batch(dct, chunks, haploid=variant == "haploid", route="host")

    def boom(*a, **k):
        raise AssertionError("the host-assembled route ran where the device pipeline was expected")
    monkeypatch.setattr(gip, "_pass2_native", boom)
    got = gip.get_indel_testing_candidates_batch(dct, chunks, haploid=variant == "haploid")
    assert _same_tuples(got, exp) >= 25


def test_tie_world_every_site_equals_the_oracle_band_on_and_off(tie_files, monkeypatch, capsys):
    """the default route (k_fill_band<1> / <2>, k_trace_band12, the full-matrix re-run of edge touches and wide bands) == the oracle's banded
    restatement on every site, and with the band off == its full-matrix form (which the host route returns: the test above); all four ways a
    window can be aligned occur, by the device's own count and by the oracle's"""
    monkeypatch.delenv("NC_PIPE_BAND", raising=False)
    r, st = _device_sites(tie_files)
    assert 30 <= r["n"] <= 80 and int(st[:3].sum()) == r["n_alignments"]
    assert st[0] > 0 and st[1] > 0 and st[2] > 0 and st[3] > 0, st                       # 32 diagonals, 64, too wide, re-run after an edge touch
    how = _sites_equal_the_oracle(tie_files, r, 160, False, True)
    assert all(how[k] > 0 for k in (32, 64, "edge", "width")), how
    # (the oracle aligns a read once per set it sits in, the device once per site: the counts differ, the classes do not)
    f, sf = _device_sites(tie_files, band=0)
    assert not sf[:4].any() and f["n"] == r["n"] and np.array_equal(f["pos"], r["pos"])
    _sites_equal_the_oracle(tie_files, f, 160, False, False)
    with capsys.disabled():
        print("\n[tie world] %d sites, %d alignments; oracle classes %s; device band stats %s" % (r["n"], r["n_alignments"], dict(how), st[:4].tolist()))


@pytest.mark.parametrize("window_after", [62, 126])
def test_short_windows_run_the_narrow_templates(tie_files, window_after, monkeypatch):
    """windows of 63 and 127 reference bases: k_fill16q<4> / <8> with the band off, k_fill_band with it on -- every site against the oracle at
    the same window"""
    monkeypatch.delenv("NC_PIPE_BAND", raising=False)
    assert next(c for c, (lo, hi) in ac.BOUNDS.items() if lo <= window_after + 1 <= hi) == {62: "cpl4", 126: "cpl8"}[window_after]
    for band in (0, 1):
        r, st = _device_sites(tie_files, window_after=window_after, band=band)
        assert r["n"] >= 30 and (st[0] > 0) == bool(band)
        _sites_equal_the_oracle(tie_files, r, window_after, False, bool(band))


# 0 <= open <= 100, 0 <= extend <= 10, 0 <= match <= 46, -100 <= mismatch <= 0 (nc_indel_sites_scoring: the derivation is there).  match = 100
# wraps the biased 16-bit scores of k_fill_band after 128 matching bases, and open == extend == 25 was never inside the range: those corners are
# refused, and the corners that are accepted run.
CORNERS = [(100, 10, 46, -100), (0, 0, 46, -100), (100, 0, 1, 0), (10, 10, 20, -10)]
REFUSED = [(100, 10, 100, -100), (0, 0, 100, -100), (25, 25, 20, -10), (25, 1, 47, -10), (101, 1, 20, -10), (25, 11, 20, -10), (25, 1, 20, -101),
           (-1, 1, 20, -10), (25, 1, 20, 1)]


@pytest.mark.parametrize("scoring", CORNERS)
@pytest.mark.parametrize("band", [0, 1])
def test_scoring_corners(tie_files, scoring, band, monkeypatch):
    """the corners of the range nc_indel_sites_scoring accepts, band off and band on, every site against the oracle under the same scoring"""
    monkeypatch.delenv("NC_PIPE_BAND", raising=False)
    r, st = _device_sites(tie_files, band=band, scoring=scoring)
    assert r["n"] >= 30
    _sites_equal_the_oracle(tie_files, r, 160, False, bool(band), scoring=scoring)


def test_scorings_outside_the_16_bit_range_are_refused(tie_files):
    from nanocaller_amd import _lib
    eng = _engine()
    try:
        for sc in REFUSED:
            assert eng.L.nc_indel_sites_scoring(eng.ctx, *sc) == _lib.NC_ERR_ARG, sc
        for sc in CORNERS + [tuple(_lib.STAR_SCORING)]:
            assert eng.L.nc_indel_sites_scoring(eng.ctx, *sc) == _lib.NC_OK, sc
        with pytest.raises(_lib.NanoCallerHipError) as e:                          # and through the keyword: before anything is planned
            _device_sites(tie_files, scoring=REFUSED[0])
        assert e.value.status == _lib.NC_ERR_ARG
    finally:
        eng.L.nc_indel_sites_scoring(eng.ctx, *[int(v) for v in _lib.STAR_SCORING])

"""Genotyping a given list of indel sites on the device indel pipeline (nc_indel_set_sites, csrc/nc_pipe_listed.hip) against
the yardstick tests/indel_genotype_ref.py: pass 1 with the list restated column by column, pass 2 judged per anchor by the oracle's pure-Python
restatement (oracle.indel_site_ref, band=True).  The world is test_indel_pipeline's kind (bamio.make_pass2_world written to a BAM) at 30 kb, with an
unphased block, a run of N in the reference, a stretch without reads and an excluded interval, so that every class of listed column has members
(tests/test_indel_genotype_ref.py asserts that on the CPU)."""
import gzip
import os

import numpy as np
import pytest

from nanocaller_amd import generate_indel_pileups as gip
from nanocaller_amd import indel_device, indelCaller

import bamio
import indel_genotype_ref as R
import oracle_pool
from test_indel_pipeline import _params
from util import device_alleles, oracle_alleles

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    d = tmp_path_factory.mktemp("listed")
    w = R.listed_world()
    bam, fa = str(d / "g.bam"), str(d / "g.fa")
    all_recs = bamio.world_to_records(w, None)
    bamio.write_bam(bam, w.chrom, w.length, all_recs)
    bamio.write_fasta(fa, w.chrom, w.ref)
    kept = [i for i, rc in enumerate(all_recs) if not rc["flag"] & 0xF04]
    recs = [all_recs[i] for i in kept]
    e = dict(w=w, bam=bam, fa=fa, recs=recs, rec_of={r: k for k, r in enumerate(kept)},
             beg=np.array([rc["pos0"] + 1 for rc in recs]), hap=np.array([rc["tags"].get("HP", 0) for rc in recs]),
             ps=np.array([rc["tags"].get("PS", 0) for rc in recs]), judged={})
    e["end"] = e["beg"] + np.array([sum(n for op, n in rc["cigar"] if op in "MDN=X") for rc in recs])
    return e


def _dct(env, case, sites=None, only=False, **kw):
    w = env["w"]
    d = _params(env["fa"], mincov=case["mincov"], ins_t=case["ins_t"], del_t=case["del_t"], win_size=case["win_size"],
                small_win_size=case["small_win_size"], impute_indel_phase=bool(case.get("impute")),
                exclude_bed=[(w.chrom, a, b) for a, b in case["exclude"]] or None, **kw)
    if sites is not None:
        d["genotype_indel_sites"] = {w.chrom: (np.asarray(sites[0]), np.asarray(sites[1]))}
        d["genotype_indel_only"] = only
    return d


def _chunks(env, case):
    return [dict(chrom=env["w"].chrom, start=a, end=b, sam_path=env["bam"]) for a, b in case["chunks"]]


def _run(env, case, sites=None, only=False, **kw):
    r, ctg, order = gip.indel_sites_for_chunks(_dct(env, case, sites, only, **kw), _chunks(env, case), 0, bool(case.get("haploid")))
    assert order == list(range(len(case["chunks"])))
    return r


def _expected(env, case, sites, only):
    """the yardstick's anchors that survive pass 2, chunk by chunk -> [(chunk, anchor, type, source column, oracle's site)]"""
    w, haploid = env["w"], bool(case.get("haploid"))
    S = R.as_dict(*sites) if sites is not None else {}
    kw = {k: case[k] for k in ("mincov", "win_size", "small_win_size", "ins_t", "del_t")}
    cand = []
    for ci, (a, b) in enumerate(case["chunks"]):
        v, src, extra = R.scan_listed(w, a, b, exclude=case["exclude"], haploid=haploid, impute=bool(case.get("impute")), sites=S, only=only, **kw)
        for an in R.pass2_range(v, a, b, case["win_size"]):
            sets = tuple(tuple(x) for x in extra[an]) if an in extra else None
            cand.append((ci, an, v[an], src.get(an, 0), sets))
    # pass 2 per anchor by the oracle (the verdict depends on the anchor and, imputed, on its two read sets): once per module
    todo = sorted({(an, sets) for _, an, _, _, sets in cand if (haploid, an, sets) not in env["judged"]}, key=lambda t: (t[0], t[1] or ()))
    tasks = []
    for an, sets in todo:
        ids = np.nonzero((env["beg"] <= an) & (env["end"] > an))[0]
        hap, ps = env["hap"][ids], env["ps"][ids]
        if sets is not None:                                        # the imputed sets stand where the HP tags stand (:310-312)
            side = {env["rec_of"][r]: 1 for r in sets[0]}
            side.update({env["rec_of"][r]: 2 for r in sets[1]})
            hap = np.array([side.get(int(i), 0) for i in ids])
        tasks.append(oracle_pool.site_task(an, [env["recs"][i] for i in ids], hap, ps, w.ref, 160, case["mincov"], 160, haploid=haploid, band=True))
    for key, got in zip(todo, oracle_pool.map_sites(tasks)):
        env["judged"][(haploid,) + key] = got
    return [(ci, an, t, s, env["judged"][(haploid, an, sets)]) for ci, an, t, s, sets in cand if env["judged"][(haploid, an, sets)] is not None], len(cand)


def _assert_anchors(r, exp):
    got = list(zip(r["chunk"].tolist(), r["pos"].tolist(), r["type"].tolist(), r["src"].tolist()))
    assert got == [(ci, an, t, s) for ci, an, t, s, _ in exp]


def _assert_sites(r, exp, haploid):
    S = 1 if haploid else 3
    x = r["x"].cpu().numpy()
    for k, (ci, an, t, s, ob) in enumerate(exp):
        assert np.array_equal(x[k].reshape(S, 5, 128, 2), ob["x"]), an
        assert int(r["phase"][k]) == ob["phase"], an
        assert device_alleles(r, k) == oracle_alleles(ob["cns"], ob["win"], t), an


@pytest.mark.parametrize("only", [False, True], ids=["add", "only"])
@pytest.mark.parametrize("name", ["dip", "hap", "imp"])
def test_anchors_sites_and_sources_equal_the_yardstick(env, name, only):
    """fetched (chunk, pos, type, src) equal the yardstick's anchors that the oracle's pass 2 keeps -- an anchor the oracle rejects is absent, and
    nothing is present that the yardstick lacks --, with tensors, phase and the three allele pairs of every site"""
    case = R.CASES[name]
    sites = R.site_list(env["w"], case)
    exp, n_cand = _expected(env, case, sites, only)
    r = _run(env, case, sites, only)
    _assert_anchors(r, exp)
    _assert_sites(r, exp, bool(case.get("haploid")))
    forced = [e for e in exp if e[3] > 0]
    # forced sites exist, and so do anchors pass 2 rejects (the imputed case lies half in the unphased block, where a listed column opens the read
    # grouping and is no source, and has neither N nor thin pileups)
    assert len(forced) >= (3 if name == "imp" else 8) and (n_cand > len(exp) or name == "imp"), (len(forced), n_cand, len(exp))
    assert name != "imp" or sum(1 for e in exp if e[3] == 0) > (0 if only else 10)
    if only:
        assert all(e[3] > 0 or name == "imp" for e in exp)
    else:
        assert any(e[3] == 0 for e in exp)
    assert r["genotype_listed"] > r["genotype_anchored"] >= len({e[3] for e in forced})


@pytest.mark.parametrize("n", [1, 65])
def test_lists_of_one_and_of_a_wave_and_one(env, n):
    """a list of one column, and of 65 (one more than a wave of k_listed's grid covers in one block row), only mode: the yardstick's anchors"""
    case = R.CASES["dip"]
    pos, lng = R.site_list(env["w"], case)
    quiet = R.site_classes(env["w"], case)["no_event"]
    sites = (np.array([quiet[len(quiet) // 2]]), np.array([0], np.uint8)) if n == 1 else (pos[:65], lng[:65])
    exp, _ = _expected(env, case, sites, True)
    r = _run(env, case, sites, True)
    _assert_anchors(r, exp)
    assert len(exp) >= 1 and (n > 1 or (r["src"].tolist() == [int(sites[0][0])] and r["pos"].tolist() == [int(sites[0][0]) - 10]))


def _same(a, b, keys=("pos", "chunk", "type", "phase", "ref_len", "alt_len", "alt", "src")):
    assert a["n"] == b["n"]
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert bool((a["x"] == b["x"]).all())


def test_small_groups_and_both_ingest_routes_give_the_same(env, monkeypatch):
    from nanocaller_amd import generate_SNP_pileups as gsp
    case = R.CASES["dip"]
    sites = R.site_list(env["w"], case)
    a = _run(env, case, sites)
    assert (a["src"] > 0).sum() >= 8 and len(gip._DEV_INGEST) == 1
    monkeypatch.setenv("NC_PIPE_GROUP_AL", "700")
    _same(_run(env, case, sites), a)
    monkeypatch.delenv("NC_PIPE_GROUP_AL")
    gsp.release_contig()
    gip._CONTIGS.clear()
    b = _run(env, case, sites, device_ingest=False)
    assert gip._CONTIGS
    _same(b, a)


def test_no_state_is_carried_into_a_plain_run(env):
    """a plain run after a listed run equals the plain run before it, byte for byte, and carries no src; only mode with a list that names nothing
    on the contig returns no site"""
    case = R.CASES["dip"]
    before = _run(env, case)
    listed = _run(env, case, R.site_list(env["w"], case))
    after = _run(env, case)
    assert "src" not in before and "src" not in after and "genotype_listed" not in after
    _same(after, before)
    assert listed["n"] > before["n"] > 0
    d = _dct(env, case)
    d.update(genotype_indel_sites={"another_contig": [5, 6]}, genotype_indel_only=True)
    r, _, _ = gip.indel_sites_for_chunks(d, _chunks(env, case), 0, False)
    assert r["n"] == 0 and r["genotype_listed"] == 0
    _same(_run(env, case), before)


def test_out_of_grid_positions_write_nothing(env, tmp_path, monkeypatch):
    """a device-side list that also holds positions off the grid (0, negative, past the contig, beyond the chunks, the int32 limits): the same
    sites, and col_type with the 64 bytes of workspace before and after it -- the dump holds every chunk's slice and its neighbours' -- unchanged"""
    import torch
    from nanocaller_amd.engine import get_engine
    case = R.CASES["dip"]
    w = env["w"]
    d = _dct(env, case)
    chunks = _chunks(env, case)
    eng, dp, reads_c, ctg, excl, mates = gip.indel_pack_for(d, chunks, 0, by_name=True)
    pos, lng = R.site_list(w, case)
    ok = (pos >= 1) & (pos <= w.length)
    kw = dict(mincov=d["mincov"], maxcov=d["maxcov"], win_size=d["win_size"], small_win_size=d["small_win_size"], ins_t=d["ins_t"], del_t=d["del_t"],
              window_after=160, excl=excl, mates=mates)
    spans = [(c["start"], c["end"]) for c in chunks]
    dev = get_engine(0).device
    junk = np.array([0, -1, -3, w.length + 1, w.length + 9, 10 ** 9, 2 ** 31 - 1, -2 ** 31, dp.tile_pos0 - 1, dp.tile_pos0 + dp.n_tiles * dp.tile_size], np.int64)
    runs, dumps = [], []
    for tag, p, g in (("clean", pos[ok], lng[ok]), ("junk", np.concatenate([junk[:5], pos[ok], junk[5:]]), np.concatenate([np.ones(5, np.uint8), lng[ok], np.ones(5, np.uint8)]))):
        monkeypatch.setenv("NC_PIPE_DUMP", str(tmp_path / tag))
        runs.append(gip.indel_sites_device(eng, dp, reads_c, w.length, spans, sites=torch.from_numpy(p.astype(np.int32)).to(dev),
                                           sites_long=torch.from_numpy(g).to(dev), **kw))
        monkeypatch.delenv("NC_PIPE_DUMP")
        dumps.append(np.fromfile(str(tmp_path / (tag + ".col_type")), np.int8))
    _same(runs[1], runs[0])
    assert (runs[0]["src"] > 0).sum() >= 8
    ncol = sum(b - max(1, a) + 1 for a, b in spans)
    assert dumps[0].size == ncol + 128 and np.array_equal(dumps[0], dumps[1])
    ct = dumps[0][64:64 + ncol]
    assert set(np.unique(ct).tolist()) <= {-1, 0, 1, 4, 5} and (ct >= 4).sum() >= 8


@pytest.mark.parametrize("tile_size", [1024, 2048, 4096])
def test_both_scan_forms_and_every_tile_size(monkeypatch, tmp_path, tile_size):
    """the same list behind the tiled and the accumulate form of K7 on packs of every tile size (synthetic workload resident in HBM), with mincov
    at the haplotype depths of the 30x pileup so that the depth test decides: same sites, sources and tensors behind both forms; in only mode
    every listed column's decision byte is the yardstick's depth verdict on the workload's reads; natural anchors before a chunk's first forced
    column are those of the plain run"""
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_indel_device_workload
    from util import IndelReadsHost
    eng = get_engine(0)
    L = 120_000
    pack, reads_c, info = make_indel_device_workload(eng, L, depth=30.0, seed=4711, tile_size=tile_size)
    chunks = [(1, 30_123), (30_123, 70_900), (70_901, L)]
    kw = dict(mincov=13, maxcov=160, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6, window_after=160)
    rng = np.random.Generator(np.random.PCG64(5))
    g0 = pack.tile_pos0
    edges = [g0 + k * tile_size + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    sites = np.unique(np.concatenate([rng.integers(5_000, L - 300, 117), [30_123, 70_900, 70_901], edges]))
    lng = (sites % 4 == 0).astype(np.uint8)
    monkeypatch.delenv("NC_K7_EVENT_ATOMICS", raising=False)
    plain = gip.indel_sites_device(eng, pack, reads_c, L, chunks, **kw)
    new = gip.indel_sites_device(eng, pack, reads_c, L, chunks, sites=sites, sites_long=lng, **kw)
    monkeypatch.setenv("NC_K7_EVENT_ATOMICS", "1")
    old = gip.indel_sites_device(eng, pack, reads_c, L, chunks, sites=sites, sites_long=lng, **kw)
    monkeypatch.delenv("NC_K7_EVENT_ATOMICS")
    _same(new, old)
    src = new["src"]
    assert (src > 0).sum() >= 30 and set(src[src > 0].tolist()) <= set(sites.tolist())
    assert np.array_equal(new["pos"][src > 0], np.maximum(1, src[src > 0] - np.where(new["type"][src > 0] == 0, 40, 10)))
    for ci in range(len(chunks)):
        m, pm = new["chunk"] == ci, plain["chunk"] == ci
        first = src[m & (src > 0)].min() if (m & (src > 0)).any() else L + 1
        cut = first - 40 - 10                                         # anchors of columns before the first forced one
        assert np.array_equal(new["pos"][m & (new["pos"] < cut)], plain["pos"][pm & (plain["pos"] < cut)])
    only, ct = _col_type_behind_the_list(tmp_path, monkeypatch, "t%d" % tile_size, lambda: gip.indel_sites_device(
        eng, pack, reads_c, L, chunks, sites=sites, sites_long=lng, sites_only=True, **kw), chunks)
    assert only["n"] >= 30 and (only["src"] > 0).all()
    # the decision bytes: 4 / 5 by class exactly where the yardstick's depth test passes on the workload's own reads, -1 elsewhere
    verdict = R.depth_verdicts(R.world_of_device_workload(IndelReadsHost(pack, info)), sites.tolist(), mincov=kw["mincov"])
    off = np.cumsum([0] + [b - max(1, a) + 1 for a, b in chunks])
    n_forced = 0
    for v, g in zip(sites.tolist(), lng.tolist()):
        for ci, (a, b) in enumerate(chunks):
            if max(1, a) <= v <= b:
                assert int(ct[off[ci] + v - max(1, a)]) == ((4 if g else 5) if verdict[v] else -1), (v, ci)
                n_forced += verdict[v]
    assert int((ct >= 4).sum()) == n_forced and 20 <= sum(verdict.values()) <= len(sites) - 20      # the depth test decides both ways


@pytest.fixture(scope="module")
def mates_files(tmp_path_factory):
    import test_indel_mates as tim
    d = tmp_path_factory.mktemp("listedmates")
    w = bamio.world_from_arrays(tim.Z, "w_")
    w.names = ["r%07d" % i for i in tim.Z["w_name_id"]]
    bam, fa = str(d / "m.bam"), str(d / "m.fa")
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, None))
    bamio.write_fasta(fa, w.chrom, w.ref)
    return w, bam, fa, tim


def _col_type_behind_the_list(tmp_path, monkeypatch, tag, run, spans):
    """run() under NC_PIPE_DUMP -> (its result, the chunks' decision bytes behind k_listed, back to back)"""
    monkeypatch.setenv("NC_PIPE_DUMP", str(tmp_path / tag))
    r = run()
    monkeypatch.delenv("NC_PIPE_DUMP")
    d = np.fromfile(str(tmp_path / (tag + ".col_type")), np.int8)
    ncol = sum(b - max(1, a) + 1 for a, b in spans)
    assert d.size == ncol + 128
    return r, d[64:64 + ncol]


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_shared_names_count_once_per_column(mates_files, haploid, tmp_path, monkeypatch):
    """the mates world of tests/test_indel_mates.py with mincov raised to where the by-name and the per-alignment depths part (R.MATES_MINCOV;
    tests/test_indel_genotype_ref.py asserts they do): at every listed column where two alignments of a name overlap -- all those where the two
    countings disagree, and a sample of the others -- k_listed<true> forces the column exactly where the by-name yardstick's depth test passes,
    and nowhere else; the anchors that reach the output carry the by-name yardstick's types and sources"""
    w, bam, fa, tim = mates_files
    a, b = 1, 4_001
    dct = dict(tim.DCT, fasta_path=fa, mincov=R.MATES_MINCOV)
    cols = R.mates_columns(w, a, b)
    kw = dict(mincov=R.MATES_MINCOV, haploid=haploid, supplementary=bool(dct.get("supplementary")))
    by_name, per_al = R.depth_verdicts(w, cols, by_name=True, **kw), R.depth_verdicts(w, cols, by_name=False, **kw)
    differ = [v for v in cols if by_name[v] != per_al[v]]
    sites = np.array(sorted(set(differ) | set(cols[::15])), np.int64)
    assert haploid or len(differ) >= 20                                # (haploid: the depth is len(read_names), names counted as often as they occur)
    dct.update(genotype_indel_sites={w.chrom: sites}, genotype_indel_only=True)
    chunk = [dict(chrom=w.chrom, start=a, end=b, sam_path=bam)]
    (r, _, _), ct = _col_type_behind_the_list(tmp_path, monkeypatch, "m", lambda: gip.indel_sites_for_chunks(dct, chunk, 0, haploid), [(a, b)])
    assert set(np.unique(ct).tolist()) <= {-1, 5}
    assert {int(v): bool(ct[v - a] == 5) for v in sites} == {int(v): by_name[int(v)] for v in sites}
    assert int((ct == 5).sum()) == sum(by_name[int(v)] for v in sites) and (haploid or sum(by_name[int(v)] != per_al[int(v)] for v in sites) >= 20)
    skw = {k: dct[k] for k in ("mincov", "win_size", "small_win_size", "ins_t", "del_t")}
    exp_v, exp_src, _ = R.scan_listed(w, a, b, supplementary=kw["supplementary"], haploid=haploid, sites={int(p): False for p in sites}, only=True,
                                      by_name=True, **skw)
    got = dict(zip(r["pos"].tolist(), zip(r["type"].tolist(), r["src"].tolist())))
    want = {an: (exp_v[an], exp_src.get(an, 0)) for an in R.pass2_range(exp_v, a, b, skw["win_size"])}
    assert len(got) >= 10 and all(an in want and want[an] == v for an, v in got.items())


def test_end_to_end_records_reference_calls_and_merged_file(env, tmp_path, monkeypatch):
    """indel_chunks_vcf_text with a list: natural records before each chunk's first forced column are the plain run's bytes; each forced site has
    exactly one of a variant record at its anchor, a REF / LOW line at its column, or lies inside the previous record; the lines' Q is the Python
    formula on the run's probabilities; call_manager's merged file keeps the lines and its header has the two FILTER lines only with a list"""
    from nanocaller_amd import _lib
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.weights import Weights, get_indel_model
    case = R.CASES["dip"]
    w = env["w"]
    eng = get_engine(0)
    eng.load_weights(_lib.MODEL_INDEL, Weights(get_indel_model("ONT-HG002")))
    sites = R.site_list(w, case)
    chunks = _chunks(env, case)
    plain = gip.indel_chunks_vcf_text(_dct(env, case), chunks, 0, False, _lib.MODEL_INDEL)
    counts = {}
    got = gip.indel_chunks_vcf_text(_dct(env, case, sites), chunks, 0, False, _lib.MODEL_INDEL, counts)
    pos, chunk, src, probs = counts["pos"], counts["chunk"], counts["src"], counts["probs"]
    chrom = w.chrom.encode()
    n_lines = n_rec = n_inside = 0
    for ci, (tp, tg) in enumerate(zip(plain, got)):
        lp, lg = tp.splitlines(keepends=True), tg.splitlines(keepends=True)
        m = chunk == ci
        forced = src[m & (src > 0)]
        first = int(forced.min()) if forced.size else w.length + 1
        cut = first - 40 - 10
        head = lambda ls: [ln for ln in ls if int(ln.split(b"\t")[1]) < cut]      # noqa: E731
        assert head(lg) == head(lp)
        p_of = [int(ln.split(b"\t")[1]) for ln in lg]
        assert p_of == sorted(p_of)
        calls = {int(ln.split(b"\t")[1]): ln for ln in lg if ln.split(b"\t")[4] == b"."}
        recs = {int(ln.split(b"\t")[1]) for ln in lg if ln.split(b"\t")[4] != b"."}
        prev = 0
        for k in np.nonzero(m)[0]:
            pj, sj = int(pos[k]), int(src[k])
            ln_rec = [ln for ln in lg if int(ln.split(b"\t")[1]) == pj and ln.split(b"\t")[4] != b"."]
            if pj <= prev:
                n_inside += sj > 0
                assert not ln_rec and (sj == 0 or sj not in calls)
                continue
            if ln_rec:
                f = ln_rec[0].split(b"\t")
                prev = pj + max(len(f[3]), max(len(x) for x in f[4].split(b",")))
                n_rec += sj > 0
                assert sj == 0 or sj not in calls
            elif sj > 0:
                assert calls[sj] == indel_device.reference_call_line(chrom, sj, w.ref[sj - 1].encode(), probs[k], False)
                p0 = float(probs[k][0])
                q = min(99.0, -10.0 * np.log10(1e-6 + 1.0 - p0)) if p0 > 0.95 else 0.0
                assert calls[sj].split(b"\t")[5:7] == [b"%.2f" % q, b"REF" if p0 > 0.95 else b"LOW"]
                n_lines += 1
        assert len(calls) == sum(1 for k in np.nonzero(m)[0] if int(src[k]) in calls)
    assert n_lines >= 4 and n_lines + n_rec + n_inside == int((src > 0).sum())
    assert counts["genotype_inside"] == n_inside and 0 < counts["genotype_recorded"] <= counts["genotype_anchored"] < counts["genotype_listed"]
    # the whole caller: the merged file keeps the lines; the FILTER lines come with a list only
    outs = {}
    for tag, extra in (("plain", {}), ("listed", dict(genotype_indel_sites={w.chrom: (sites[0], sites[1])}))):
        out = str(tmp_path / tag)
        os.makedirs(out)
        regions = [(w.chrom, 1, 4000, "diploid")]
        ip = dict(chunks_list=[dict(chrom=w.chrom, start=a, end=b, ploidy="diploid") for a, b in case["chunks"]], mode="indels", snp_vcf=None,
                  regions_list=regions, sam_path=env["bam"], cpu=2, vcf_path=out, prefix="t", sample="SAMPLE", enable_whatshap=False, suppress_progress=True,
                  phase_qual_score=10, verbose=False, indel_model="ONT-HG002", **_dct(env, case), **extra)
        files = indelCaller.call_manager(ip)
        outs[tag] = [ln for ln in gzip.open(files["indels"], "rt")]
    has = lambda lines, key: any(ln.startswith("##FILTER=<ID=%s," % key) for ln in lines)      # noqa: E731
    assert has(outs["listed"], "REF") and has(outs["listed"], "LOW") and not has(outs["plain"], "REF") and not has(outs["plain"], "LOW")
    body = [ln for ln in outs["listed"] if not ln.startswith("#")]
    assert sum(1 for ln in body if ln.split("\t")[4] == ".") == n_lines
    assert n_lines > 0 and not any(ln.split("\t")[4] == "." for ln in outs["plain"] if not ln.startswith("#"))

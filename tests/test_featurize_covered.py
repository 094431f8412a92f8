"""k_featurize_pairs enumerates only the (read, column) pairs a read covers: read r of a site covers the columns [jlo, jhi) of the site's
ascending column list, the pairs of 64 reads are numbered by a prefix over jhi - jlo and swept 64 a step.  Each test compares the int16 device
route (tensors, dp, strand depths) array-equal with the oracle on a synthetic world, and first shows ON THE HOST (the oracle's neighbour picks and
the world's read extents) that the world holds the case the test is about."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PC_ROUND = 512                                                           # pairs one round of gathers in flight can hold (the issue's figure)


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


def _dct(seq="ont", maxcov=160, threshold=(0.4, 0.6), supplementary=False):
    return dict(mincov=4, maxcov=maxcov, min_allele_freq=0.15, min_nbr_sites=1, threshold=list(threshold), seq=seq, supplementary=supplementary,
                exclude_bed=None)


def _host_intervals(world, dct, region):
    """per candidate site: (v, columns ascending, nl, [(read, jlo, jhi)] of the sampled reads with a base at v) -- the kernel's enumeration
    restated from oracle.get_cnd_pos and the read extents (alignments keyed one by one: worlds without shared names)"""
    from oracle import oracle
    rc = oracle.ref_codes_with_exclusions(world)
    nbr, cpos, _, _ = oracle.snp_scan(world, rc, region["start"], region["end"], region["ploidy"], dct["mincov"], dct["min_allele_freq"],
                                      dct["threshold"], dct["supplementary"])
    keep = np.flatnonzero((world.read_flag & (0x704 if dct["supplementary"] else 0xF04)) == 0)
    rs, re_ = world.read_start[keep].astype(np.int64), world.read_end[keep].astype(np.int64)
    out = []
    for v in cpos.tolist():
        left, right = oracle.get_cnd_pos(v, nbr, dct["seq"])
        cols = np.array(sorted(left) + [v] + sorted(right), np.int64)
        assert np.all(np.diff(cols) > 0)
        cover = np.flatnonzero((rs <= v) & (v < re_))[:dct["maxcov"]]
        rows = []
        for k in cover.tolist():
            r = int(keep[k])
            if world.codes[world.read_off[r] + v - int(rs[k])] < 4:
                rows.append((r, int(np.searchsorted(cols, rs[k], "left")), int(np.searchsorted(cols, re_[k], "left"))))
        out.append((v, cols, len(left), rows))
    return out


def _pc(rows):
    return sum(jhi - jlo for _, jlo, jhi in rows)


def _device(eng, world, dct, region):
    import torch
    from nanocaller_amd.wire import build_wire_from_world, upload_wire
    dpk = upload_wire(eng, build_wire_from_world(world, supplementary=dct["supplementary"]))
    sites = eng.snp_scan(dpk, [(region["start"], region["end"])], mincov=dct["mincov"], min_allele_freq=dct["min_allele_freq"],
                         threshold=dct["threshold"])
    eng.snp_featurize(dpk, sites, seq=dct["seq"], maxcov=dct["maxcov"], min_nbr_sites=dct["min_nbr_sites"], int16=True)
    torch.cuda.synchronize()
    assert sites.x.dtype == torch.int16
    return dpk, sites


def _assert_equals_oracle(eng, world, dct, region, min_sites):
    from oracle import oracle
    pos, _, mat, dp, _, depth, fwd, rev = oracle.get_snp_testing_candidates(world, dct, region)
    dpk, sites = _device(eng, world, dct, region)
    assert len(pos) >= min_sites and bool(np.all(sites.valid.cpu().numpy()))
    assert np.array_equal(sites.pos, pos) and np.array_equal(sites.dp, dp)
    bad = np.flatnonzero((sites.x.cpu().numpy() != np.asarray(mat).astype(np.int16)).any(axis=(1, 2, 3)))
    assert bad.size == 0, "tensors differ from the oracle's at %d of %d sites, first at site %d" % (bad.size, len(pos), bad[0])
    assert np.array_equal(sites.fwd_dp.cpu().numpy(), fwd) and np.array_equal(sites.rev_dp.cpu().numpy(), rev)
    assert float(np.mean(sites.depth.cpu().numpy().astype(np.float64))) == depth
    return dpk, sites


_short = {}


def _short_world(depth=30):
    """ONT reads of ~1.5 kb: (world, region, host intervals, sites to expect at least).  depth 30: 120 kb; depth 100 (more than one group of 64
    sampled reads per site): 60 kb"""
    if depth not in _short:
        from nanocaller_amd.synth import make_world
        length, lo, hi, least = (120_000, 20_000, 100_000, 500) if depth == 30 else (60_000, 10_000, 50_000, 200)
        world = make_world(seed=5, length=length, depth=depth, read_len_scale=0.15)
        region = dict(chrom=world.chrom, start=lo, end=hi, ploidy="diploid")
        _short[depth] = (world, region, _host_intervals(world, _dct(), region), least)
    return _short[depth]


def _assert_groups(host, depth):
    """depth 100: some site samples more than 64 reads, so its pairs come from more than one group of reads"""
    nsel = max(len(rows) for _, _, _, rows in host)
    print("largest nsel %d" % nsel)
    assert nsel > 64 if depth > 30 else nsel <= 64


def test_short_reads_fewer_pairs_than_one_step(eng):
    world, region, host, least = _short_world()
    slots = sum(len(rows) * len(cols) for _, cols, _, rows in host)
    pcs = [_pc(rows) for _, _, _, rows in host]
    print("sites %d, covered %.3f of the pair slots, min Pc %d" % (len(host), sum(pcs) / slots, min(pcs)))
    assert sum(pcs) < 0.15 * slots
    assert any(0 < pc <= 64 for pc in pcs)
    _assert_equals_oracle(eng, world, _dct(), region, least)


def test_dense_coverage_more_pairs_than_one_round_in_flight(eng):
    from nanocaller_amd.synth import make_world
    world = make_world(seed=3, length=400_000, depth=30, tech="hifi")
    dct = _dct(seq="pacbio", threshold=(0.3, 0.7))
    region = dict(chrom=world.chrom, start=150_000, end=250_000, ploidy="diploid")
    pcs = [_pc(rows) for _, _, _, rows in _host_intervals(world, dct, region)]
    print("sites %d, mean Pc %.0f, max Pc %d" % (len(pcs), np.mean(pcs), max(pcs)))
    assert max(pcs) > PC_ROUND
    _assert_equals_oracle(eng, world, dct, region, 500)


def _with_extents(world, edits):
    """the world with read r cut down to [start, end) for every (r, start, end) of `edits` (inside its old extent), reads in start order again"""
    rs, re_ = world.read_start.copy(), world.read_end.copy()
    parts = [world.read_codes(r) for r in range(world.n_reads)]
    for r, s, e in edits:
        assert rs[r] <= s < e <= re_[r]
        parts[r] = parts[r][s - rs[r]:e - rs[r]]
        rs[r], re_[r] = s, e
    order = np.argsort(rs, kind="stable")
    w = copy.copy(world)
    w.read_start, w.read_end, w.read_flag = rs[order], re_[order], world.read_flag[order]
    w.names = [world.names[r] for r in order]
    parts = [parts[r] for r in order]
    w.read_off = np.zeros(world.n_reads + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=w.read_off[1:])
    w.codes = np.concatenate(parts)
    w.hap = None
    return w


@pytest.mark.parametrize("depth", [30, 100])
def test_interval_edges_start_on_a_column_end_on_a_column_centre_alone(eng, depth):
    world, region, host, least = _short_world(depth)
    _assert_groups(host, depth)

    def code(r, p):
        return world.codes[world.read_off[r] + p - int(world.read_start[r])]
    # a few reads cut so that they start / end exactly on a column of a site they cover (the first and last base of an alignment are bases)
    edits, used = [], set()
    for v, cols, nl, rows in host[::5]:
        for r, jlo, jhi in rows:
            if r in used:
                continue
            if len(edits) % 2 == 0 and jlo < nl and cols[jlo] > world.read_start[r] and code(r, cols[jlo]) < 4:
                edits.append((r, int(cols[jlo]), int(world.read_end[r])))
            elif len(edits) % 2 == 1 and jhi - 1 > nl and code(r, cols[jhi - 1] - 1) < 4:
                edits.append((r, int(world.read_start[r]), int(cols[jhi - 1])))
            else:
                continue
            used.add(r)
            break
    assert len(edits) >= 6
    w = _with_extents(world, edits)
    starts_on = ends_on = centre_only = 0
    for v, cols, nl, rows in _host_intervals(w, _dct(), region):
        for r, jlo, jhi in rows:
            assert jlo <= nl < jhi
            starts_on += jlo < nl and cols[jlo] == w.read_start[r]
            ends_on += jhi < len(cols) and cols[jhi] == w.read_end[r]              # the column the read ends on is not covered
            centre_only += jhi - jlo == 1
    print("pairs of (site, read): start on a column %d, end on a column %d, the centre alone %d" % (starts_on, ends_on, centre_only))
    assert starts_on > 0 and ends_on > 0 and centre_only > 0
    _assert_equals_oracle(eng, w, _dct(), region, least)


@pytest.mark.parametrize("maxcov", [255, 50])
def test_depth_at_the_cap(eng, maxcov):
    from nanocaller_amd.synth import make_world
    world = make_world(seed=9, length=24_000, depth=300, tech="hifi", read_len_scale=0.2)
    region = dict(chrom=world.chrom, start=4_000, end=20_000, ploidy="diploid")
    dct = _dct(seq="pacbio", maxcov=maxcov, threshold=(0.3, 0.7))
    host = _host_intervals(world, dct, region)
    nsel = [len(rows) for _, _, _, rows in host]
    print("sites %d, largest nsel %d, largest Pc %d" % (len(host), max(nsel), max(_pc(rows) for _, _, _, rows in host)))
    assert max(nsel) == maxcov                                             # (HiFi error rates: some site has no sampled read deleted at the centre)
    _, sites = _assert_equals_oracle(eng, world, dct, region, 50)
    assert int(sites.depth.max()) == maxcov


@pytest.mark.parametrize("case", ["contig_ends", "sparse_neighbours"])
def test_one_sided_and_empty_neighbourhoods(eng, case):
    """contig_ends: the chunk is the whole 30 kb contig, every site has a neighbour, the first and last sites on one side only.  sparse_neighbours:
    200 kb with four heterozygous sites and no systematic-error columns, so that candidates further than 50 kb from all of them (and a
    neighbour site whose only neighbour would be itself) have NO neighbour: ncols == 1, colL = [v], every read's interval is the centre alone,
    Pc == nsel.  Such a site is valid (min_nbr_sites = 1 counts the candidate itself) and is compared with the oracle like every other."""
    from nanocaller_amd.synth import make_world
    if case == "contig_ends":
        world = make_world(seed=13, length=30_000, depth=30, read_len_scale=0.15, sys_err_rate=0.002)
    else:
        world = make_world(seed=17, length=200_000, depth=30, read_len_scale=0.15, het_rate=2e-5, hom_rate=1 / 1500, sys_err_rate=0.0)
    region = dict(chrom=world.chrom, start=1, end=world.length, ploidy="diploid")
    host = _host_intervals(world, _dct(), region)
    no_left = sum(nl == 0 and len(cols) > 1 for _, cols, nl, _ in host)
    no_right = sum(nl == len(cols) - 1 and len(cols) > 1 for _, cols, nl, _ in host)
    alone = [i for i, (_, cols, _, _) in enumerate(host) if len(cols) == 1]
    print("sites %d: no left neighbour %d, no right neighbour %d, no neighbour at all %d" % (len(host), no_left, no_right, len(alone)))
    assert no_left > 0 and no_right > 0
    assert len(alone) == 0 if case == "contig_ends" else len(alone) >= 10
    _, sites = _assert_equals_oracle(eng, world, _dct(), region, 20)
    if alone:
        # the sites without neighbours came through as valid sites with a tensor of their own: centre column only, the sampled reads counted there
        x = sites.x.cpu().numpy()[alone]
        assert np.all(x[:, :, :20] == 0) and np.all(x[:, :, 21:] == 0)
        assert np.array_equal(np.abs(x[:, 1:5, 20, 0:4]).sum(axis=(1, 2)), [len(host[i][3]) for i in alone])


@pytest.mark.parametrize("depth", [30, 100])
def test_same_name_alignments_read_columns_their_own_span_misses(eng, depth):
    from oracle import oracle
    from test_mates import _share_names
    world, region, host, least = _short_world(depth)
    _assert_groups(host, depth)
    w = _share_names(world, seed=4, n_groups=40, reach=3_000)
    dct = _dct(supplementary=True)
    # a later alignment of a name covers a column of a site that the name's earlier alignment (the site's row) does not cover itself
    keep = (w.read_flag & 0x704) == 0
    by_name = {}
    for r in np.flatnonzero(keep).tolist():
        by_name.setdefault(w.names[r], []).append(r)
    plain = copy.copy(w)
    plain.names = None
    reaches = 0
    for v, cols, nl, rows in _host_intervals(plain, dct, region):
        for r, jlo, jhi in rows:
            for r2 in by_name[w.names[r]]:
                if r2 > r and not w.read_start[r2] <= v < w.read_end[r2]:
                    reaches += int(np.any((cols >= w.read_start[r2]) & (cols < w.read_end[r2]) & ((cols < w.read_start[r]) | (cols >= w.read_end[r]))))
    print("(site, row) pairs whose name reaches a column through a later alignment: %d" % reaches)
    assert reaches > 0
    dpk, _ = _assert_equals_oracle(eng, w, dct, region, least)
    assert dpk.mates is not None
    per_alignment = oracle.get_snp_testing_candidates(plain, dct, region)
    assert not np.array_equal(np.asarray(per_alignment[2]), np.asarray(oracle.get_snp_testing_candidates(w, dct, region)[2]))

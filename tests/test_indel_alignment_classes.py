"""Every alignment class of the device indel pipeline (csrc/nc_pipe.hip, nc_pipe_*.hip) against the oracle's restatement, site by site.

A read window is aligned to its reference window on 32 diagonals, on 64, or on the full matrix (listF): a band too wide for 64 diagonals,
or a banded path that touched an edge diagonal and was re-run.  The consensus alleles run on a band with a certificate, and on the full
matrix without one.  The rare classes are where a kernel goes wrong unseen, so each run below samples its sites by class over the whole
contig -- 64-diagonal, width, edge, windows a read end cuts short, allele fallbacks, and random sites -- and asserts how many sites of each
class it checked.  For every checked site: the tensor bit for bit, the phase, REF / ALT from allele_prediction on the oracle's consensus
strings, and for every alignment its read, window length, band and class (oracle.star_cigars_banded_ref's `how`); the device's classes come
from the NC_PIPE_DUMP class lists.  The oracle: oracle.indel_site_ref(..., band=True), pure Python, on a few spawned worker processes."""
import numpy as np
import pytest

from nanocaller_amd import generate_indel_pileups as gip

import oracle_pool
from util import IndelReadsHost, device_alleles, oracle_alleles

pytestmark = pytest.mark.gpu

CLASS = {0: 32, 1: 64, 2: "width", 3: "edge"}
STRATA = ("64", "width", "edge", "short", "allele_full", "random")
HARSH = dict(p_del=0.06, p_ins=0.04, max_len=50, het_indel=1 / 1500.0, hom_indel=1 / 4000.0)
QUOTA = dict(zip(STRATA, (12, 10, 10, 10, 8, 25)))
SMALL = dict(zip(STRATA, (3, 2, 2, 2, 2, 6)))

# run -> workload, pipeline settings, sites sampled per stratum, and the checked sites each stratum must reach (0: the class does not occur
# there -- edge re-runs are rarer than one in a thousand alignments of the default workload, and 260-base windows are too long for banded
# allele alignments)
RUNS = {
    "a_diploid_160": dict(L=400_000, seed=101, wa=160, need=dict(zip(STRATA, (10, 8, 0, 8, 6, 25)))),
    "b_diploid_260": dict(L=400_000, seed=202, wa=260, need=dict(zip(STRATA, (10, 8, 0, 8, 0, 25)))),
    "c_haploid_160": dict(L=300_000, seed=303, wa=160, haploid=True, need=dict(zip(STRATA, (10, 8, 0, 8, 4, 25)))),
    "d_haploid_260": dict(L=300_000, seed=404, wa=260, haploid=True, need=dict(zip(STRATA, (10, 8, 0, 8, 0, 25)))),
    "e_harsh_160": dict(L=300_000, seed=505, wa=160, wl=HARSH, need=dict(zip(STRATA, (10, 8, 8, 8, 6, 25)))),
    "f_maxcov9": dict(L=300_000, seed=606, wa=160, maxcov=9, need=dict(zip(STRATA, (10, 8, 0, 8, 6, 25)))),
    "g_depth300_maxcov300": dict(L=150_000, seed=707, wa=160, depth=300.0, maxcov=300, quota=SMALL, need=dict(zip(STRATA, (2, 1, 0, 2, 0, 6)))),
}


def _dump(path, n_al, n_sets):
    d = {k: np.fromfile("%s.%s" % (path, k), dt) for k, dt in (("cls", np.int8), ("al_site", np.int32), ("al_read", np.int32), ("n1", np.int32),
                                                             ("band_lo", np.int8), ("ab_cls", np.int8))}
    # every group's alignments and sets are in the files: they cover the run
    assert all(len(d[k]) == n_al for k in ("cls", "al_site", "al_read", "n1", "band_lo")), ({k: len(v) for k, v in d.items()}, n_al)
    assert len(d["ab_cls"]) == n_sets
    assert d["cls"].min() >= 0 and d["cls"].max() <= 3 and d["ab_cls"].min() >= 0
    return d


def _strata(d, n, S, wa):
    """per stratum: the sites it holds"""
    site = d["al_site"]
    has = lambda m: np.unique(site[m])                                          # noqa: E731
    return {"64": has(d["cls"] == 1), "width": has(d["cls"] == 2), "edge": has(d["cls"] == 3), "short": has(d["n1"] < wa),
            "allele_full": np.unique(np.nonzero(d["ab_cls"] == 3)[0] // S), "random": np.arange(n)}


@pytest.mark.parametrize("run", sorted(RUNS))
def test_sampled_sites_of_every_alignment_class_equal_the_oracle(run, tmp_path, monkeypatch, capsys):
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_indel_device_workload
    cfg = RUNS[run]
    L, wa, haploid, maxcov = cfg["L"], cfg["wa"], cfg.get("haploid", False), cfg.get("maxcov", 160)
    S = 1 if haploid else 3
    eng = get_engine(0)
    pack, reads_c, info = make_indel_device_workload(eng, L, depth=cfg.get("depth", 30.0), seed=cfg["seed"], **cfg.get("wl", {}))
    chunks = [(s, min(L, s + 100_000)) for s in range(1, L, 100_000)]
    monkeypatch.setenv("NC_PIPE_DUMP", str(tmp_path / "d"))
    r = gip.indel_sites_device(eng, pack, reads_c, L, chunks, mincov=4, maxcov=maxcov, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6,
                               window_after=wa, haploid=haploid)
    monkeypatch.delenv("NC_PIPE_DUMP")
    n = r["n"]
    assert n > 20
    d = _dump(tmp_path / "d", r["n_alignments"], n * S)
    strata = _strata(d, n, S, wa)
    with capsys.disabled():
        print("\n[%s] %d sites, %d alignments; sites per stratum %s" % (run, n, r["n_alignments"], {k: len(v) for k, v in strata.items()}))
    # the sample: per stratum sites drawn over the whole contig
    rng = np.random.default_rng(cfg["seed"])
    quota = cfg.get("quota", QUOTA)
    draw = {k: rng.choice(strata[k], size=min(quota[k], len(strata[k])), replace=False).tolist() for k in STRATA}
    pick = sorted(set().union(*draw.values()))
    host = IndelReadsHost(pack, info)
    tasks, ids_of = [], []
    for k in pick:
        p = int(r["pos"][k])
        recs, ids = host.records(p, p)
        tasks.append(oracle_pool.site_task(p, recs, host.hap[ids], host.ps[ids], host.ref, wa, 4, maxcov, haploid=haploid))
        ids_of.append(ids)
    got = oracle_pool.map_sites(tasks)
    x = r["x"][pick].cpu().numpy()
    order = np.argsort(d["al_site"], kind="stable")
    first = np.searchsorted(d["al_site"][order], np.arange(n + 1))
    n_al = {c: 0 for c in CLASS.values()}
    most = 0
    cut = 0
    for j, k in enumerate(pick):
        p, o = int(r["pos"][k]), got[j]
        assert o is not None, (run, p)
        assert np.array_equal(x[j].reshape(S, 5, 128, 2), o["x"]), (run, p)
        assert o["phase"] == int(r["phase"][k]), (run, p)
        assert device_alleles(r, k) == oracle_alleles(o["cns"], o["win"], int(r["type"][k])), (run, p)
        # the site's alignments: one per read of the union of its sets, on the class, band and window length of the oracle's
        dev = {int(d["al_read"][a]): (CLASS[int(d["cls"][a])], int(d["band_lo"][a]), int(d["n1"][a])) for a in order[first[k]:first[k + 1]]}
        ref = {}
        for (rk, n1), how, b in zip(o["reads"], o["how"], o["bands"]):
            ref[int(ids_of[j][rk])] = (how, b[0] if b else 0, n1)
        assert dev == ref, (run, p, [(a, dev.get(a), ref.get(a)) for a in sorted(set(dev) | set(ref)) if dev.get(a) != ref.get(a)][:6])
        for how, _, _ in dev.values():
            n_al[how] += 1
        most = max(most, len(dev))
        cut += len(ids_of[j]) > maxcov
    checked = {k: len(set(pick) & set(strata[k].tolist())) if k != "random" else len(draw[k]) for k in STRATA}
    with capsys.disabled():
        print("[%s] checked against the oracle: %d sites, per stratum %s; %d alignments, per class %s" % (
            run, len(pick), checked, sum(n_al.values()), n_al))
    for k in STRATA:
        assert checked[k] >= cfg["need"][k], (run, k, checked[k])
    if maxcov < 160:
        assert cut >= 3, cut                                                       # the first-maxcov cut took reads away at checked sites
    if maxcov > 255:
        assert most > 255, most                                                    # sets beyond a byte: k_site_tensor's 16-bit histogram form

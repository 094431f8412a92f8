"""Shared helpers for the test-suite (loading golden worlds / cases)."""
import os

import numpy as np

from nanocaller_amd.synth import World

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_worlds = {}


def load_world(name):
    if name not in _worlds:
        z = np.load(os.path.join(GOLD, "world_%s.npz" % name))
        R = z["read_start"].shape[0]
        _worlds[name] = World(chrom=str(z["chrom"]), ref=z["ref"].tobytes().decode(), read_start=z["read_start"],
                              read_end=z["read_end"], read_flag=z["read_flag"], read_off=z["read_off"],
                              codes=z["codes"], names=["r%07d" % i for i in range(R)])
        if "ev_off" in z:
            _worlds[name].meta.update(events=(z["ev_off"], z["ev_pos"], z["ev_len"]), hap=z["hap"], ps=z["ps"])
    return _worlds[name]


SNP_CASES = sorted(f[4:-4] for f in os.listdir(GOLD) if f.startswith("snp_") and f.endswith(".npz"))


def load_snp_case(case):
    z = np.load(os.path.join(GOLD, "snp_%s.npz" % case))
    world = load_world(str(z["world"]))
    if "name_id" in z:                                                   # the same alignments with shared read names / other flags (make_goldens.mates_world)
        import copy
        world = copy.copy(world)
        world.names = ["r%07d" % i for i in z["name_id"]]
        world.read_flag = z["read_flag"]
    dct = dict(threshold=[float(z["threshold"][0]), float(z["threshold"][1])], supplementary=bool(z["supplementary"]),
               mincov=int(z["mincov"]), maxcov=int(z["maxcov"]), min_allele_freq=float(z["min_allele_freq"]),
               min_nbr_sites=int(z["min_nbr_sites"]), seq=str(z["seq"]), exclude_bed=None)
    region = dict(chrom=world.chrom, start=int(z["start"]), end=int(z["end"]), ploidy=str(z["ploidy"]))
    exclude = [(world.chrom, int(a), int(b)) for a, b in z["exclude"]]
    gold = dict(pos=z["pos"], ref=z["ref"], mat=z["mat"].astype(np.float32), dp=z["dp"], freq=z["freq"],
                depth=float(z["depth"]), fwd_dp=z["fwd_dp"], rev_dp=z["rev_dp"])
    return world, dct, region, exclude, gold


def assert_tuple_matches_gold(out, gold):
    pos, ref, mat, dp, freq, depth, fwd, rev = out
    n = len(gold["pos"])
    assert len(pos) == n
    if n == 0:
        # reference returns empty lists and depth 0 (generate_SNP_pileups.py:193-197)
        for x in (ref, mat, dp, freq, fwd, rev):
            assert len(x) == 0
        assert depth == 0
        return
    assert np.array_equal(np.asarray(pos), gold["pos"])
    assert np.array_equal(np.asarray(ref), gold["ref"])
    assert np.asarray(mat).dtype == np.float32 and np.array_equal(np.asarray(mat), gold["mat"])
    assert np.array_equal(np.asarray(dp), gold["dp"])
    assert np.array_equal(np.asarray(freq), gold["freq"])          # float64, bit-exact
    assert float(depth) == gold["depth"]
    assert np.array_equal(np.asarray(fwd), gold["fwd_dp"])
    assert np.array_equal(np.asarray(rev), gold["rev_dp"])


def load_impute_world():
    """the indel world with unphased stretches + per-read inserted bases (inputs stored in indel_impute.npz)"""
    if "impute" not in _worlds:
        import copy
        from nanocaller_amd.synth import apply_impute_inputs
        z = np.load(os.path.join(GOLD, "indel_impute.npz"))
        base = load_world("indel")
        w = copy.copy(base)
        w.meta = dict(base.meta)
        _worlds["impute"] = apply_impute_inputs(w, z["hap"], z["ins_off"], z["ins_bases"])
    return _worlds["impute"]


def indel_impute_cases():
    z = np.load(os.path.join(GOLD, "indel_impute.npz"))
    out = []
    for k in range(int(z["n"])):
        xpos = z["s%d_xpos" % k]
        out.append(dict(start=int(z["s%d_start" % k]), end=int(z["s%d_end" % k]), mincov=int(z["s%d_mincov" % k]),
                        win_size=int(z["s%d_win_size" % k]), small_win_size=int(z["s%d_small_win_size" % k]),
                        ins_t=float(z["s%d_ins_t" % k]), del_t=float(z["s%d_del_t" % k]),
                        exclude=[(int(a), int(b)) for a, b in z["s%d_excl" % k]], pos=z["s%d_pos" % k], type=z["s%d_type" % k],
                        extra={int(p): (z["s%d_x%d_0" % (k, j)].tolist(), z["s%d_x%d_1" % (k, j)].tolist()) for j, p in enumerate(xpos)}))
    return out


def indel_scan_cases(haploid=False):
    z = np.load(os.path.join(GOLD, "indel_scan_hap.npz" if haploid else "indel_scan.npz"))
    out = []
    for k in range(int(z["n"])):
        out.append(dict(start=int(z["s%d_start" % k]), end=int(z["s%d_end" % k]), mincov=int(z["s%d_mincov" % k]),
                        win_size=int(z["s%d_win_size" % k]), small_win_size=int(z["s%d_small_win_size" % k]),
                        ins_t=float(z["s%d_ins_t" % k]), del_t=float(z["s%d_del_t" % k]),
                        exclude=[(int(a), int(b)) for a, b in z["s%d_excl" % k]], pos=z["s%d_pos" % k], type=z["s%d_type" % k]))
    return out


class IndelReadsHost:
    """Host copies of the reads of a synthetic device workload (synth_device.make_indel_device_workload) that start at or before `hi`
    (default: all of them), and the oracle's SAM-like records rebuilt from them (oracle.records_from_indel_pack) for the reads that
    overlap any [lo, hi].  Records keep the workload's read order -- the pipeline's pileup order, which the first-maxcov cut of a read
    set follows -- and come with the reads' global indices, HP and PS."""

    def __init__(self, pack, info, hi=None):
        s, e = info["read_start"], info["read_end"]
        r1 = len(s) if hi is None else int(np.searchsorted(s, hi, side="right"))
        self.s, self.e = s[:r1], e[:r1]
        self.hap, self.ps = np.asarray(info["hap"])[:r1], np.asarray(info["ps"])[:r1]
        self.slot = pack.reads["slot_off"][:r1 + 1].cpu().numpy()
        self.codes = pack.codes[:int(self.slot[-1])].cpu().numpy()
        self.ev_off = pack.events["ev_off"][:r1 + 1].cpu().numpy()
        n_ev = int(self.ev_off[-1])
        self.ev_pos = pack.events["ev_pos"][:n_ev].cpu().numpy()
        self.ev_len = pack.events["ev_len"][:n_ev].cpu().numpy()
        self.ins_off = info["tensors"]["ins_off"][:n_ev + 1].cpu().numpy()
        self.ins = info["tensors"]["ins_bases"][:max(int(self.ins_off[-1]), 1)].cpu().numpy()
        self.length = int(info["L"])
        # the reference as the oracle reads it: 1-based positions up to the last read's end (+ a window), soft-masked runs in lower case
        n = min(self.length, int(self.e.max()) + 400 if r1 else 0)
        ref = info["tensors"]["ref"][1:n + 1].cpu().numpy()
        masked = pack.ref_code[1:n + 1].cpu().numpy() == 4
        self.ref = np.where(masked, np.frombuffer(b"agtcn", np.uint8)[ref], np.frombuffer(b"AGTCN", np.uint8)[ref]).tobytes().decode()

    def overlapping(self, lo, hi):
        """global indices of the reads with start <= hi and end > lo, ascending"""
        r1 = int(np.searchsorted(self.s, hi, side="right"))
        return np.nonzero(self.e[:r1] > lo)[0]

    def records(self, lo, hi):
        """-> (records, read ids): oracle records of the reads overlapping [lo, hi], in read order"""
        from oracle import oracle
        ids = self.overlapping(lo, hi)
        s, e, slot, ev_off = self.s, self.e, self.slot, self.ev_off

        def codes_of(j):
            r = ids[j]
            o = int(slot[r]) + (int(s[r]) & 15)
            return self.codes[o:o + int(e[r] - s[r])]

        def ev_of(j):
            r = ids[j]
            return list(zip(self.ev_pos[ev_off[r]:ev_off[r + 1]].tolist(), self.ev_len[ev_off[r]:ev_off[r + 1]].tolist()))

        def ins_of(j, k):
            a = int(ev_off[ids[j]]) + k
            return self.ins[self.ins_off[a]:self.ins_off[a + 1]]
        return oracle.records_from_indel_pack(s[ids], e[ids], codes_of, ev_of, ins_of), ids


def device_alleles(r, k):
    """[(REF length, ALT string) or None per read set] of site k of a fetched gip.indel_sites_device result"""
    S = r["sets"]
    if "_aoff" not in r:
        r["_aoff"] = np.concatenate([[0], np.cumsum(np.maximum(np.asarray(r["alt_len"]).reshape(-1), 0))])
        r["_alt"] = np.frombuffer(b"AGTCN", np.uint8)[np.asarray(r["alt"])].tobytes().decode()
    out = []
    for t in range(S):
        rl, al, o = int(r["ref_len"][k, t]), int(r["alt_len"][k, t]), int(r["_aoff"][k * S + t])
        out.append(None if rl < 0 else (rl, r["_alt"][o:o + al]))
    return out


def oracle_alleles(cns, win, var_type):
    """device_alleles' form of allele_prediction on the oracle's consensus strings (max_range 40 for a type-0 site, else 10)"""
    from nanocaller_amd import generate_indel_pileups as gip
    out = []
    for c in cns:
        ref, alt = gip.allele_prediction(c, win, 40 if var_type == 0 else 10)
        assert ref is None or ref == win[:len(ref)]
        out.append(None if ref is None else (len(ref), alt))
    return out

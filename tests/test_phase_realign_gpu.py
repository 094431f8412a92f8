"""GPU: the phaser's alleles by local realignment (csrc/nc_happhase.hip k_hr_*, phase_contig(realign=True)) against the restatement
(tests/phase_realign_ref.py) entry for entry on reads with indel errors next to het SNPs, on both decode routes; the phaser and the
haplotagger on those entries against tests/phase_ref.py; the switch off changes nothing; phase_run end to end with the switch on."""
import gzip
import os
import struct

import numpy as np
import pytest

import bamio
from phase_realign_ref import compare_rules, entries, het_site_alleles, make_realign_world
from test_phase_gpu import _assert_equal_to_restatement, _indels, _reads_of, _snp_vcf, contig, eng  # noqa: F401  (contig: the 2 Mb fixture, on eng)

pytestmark = pytest.mark.gpu
LETTER = "AGTC"


def _write(w, d):
    recs = bamio.world_to_records(w, None)
    bam, fa = os.path.join(d, "untagged.bam"), os.path.join(d, "r.fa")
    bamio.write_bam(bam, w.chrom, w.length, [dict(r, tags={}) for r in recs], write_csi=True)
    bamio.write_fasta(fa, w.chrom, w.ref)
    return recs, bam, fa


def _site_records(w, pos, al, rng):
    """VCF records of the sites: 0/1 (REF, ALT), every seventh one as 1/2 (ALT and a third base)"""
    out = []
    for k, (p, (a0, a1)) in enumerate(zip(pos.tolist(), al.tolist())):
        if k % 7 == 3:
            third = [b for b in range(4) if b not in (a0, a1)][int(rng.integers(0, 2))]
            out.append("%s\t%d\t.\t%s\t%s,%s\t30.00\tPASS\t.\tGT:GQ\t1/2:30\n" % (w.chrom, p, LETTER[a0], LETTER[a1], LETTER[third]))
        else:
            out.append("%s\t%d\t.\t%s\t%s\t30.00\tPASS\t.\tGT:GQ\t0/1:30\n" % (w.chrom, p, LETTER[a0], LETTER[a1]))
    return out


@pytest.fixture(scope="module", params=[11, 12, 13])
def planted(request, tmp_path_factory):
    from nanocaller_amd.phase import het_sites, kept_reads
    seed = request.param
    w = make_realign_world(seed, length=120_000)
    d = str(tmp_path_factory.mktemp("realign%d" % seed))
    recs, bam, fa = _write(w, d)
    kept = kept_reads(w, False)[0]
    pos, al = het_site_alleles(w, kept)
    vcf = _site_records(w, pos, al, np.random.default_rng(seed))
    _, pos2, al2, kinds = het_sites(vcf, 10)
    assert np.array_equal(pos, pos2) and "1/2" in kinds
    col, rea = entries(w, kept, pos2, al2, "column"), entries(w, kept, pos2, al2, "realign")
    return dict(w=w, bam=bam, fa=fa, kept=kept, pos=pos2, al=al2, vcf=vcf, col=col, rea=rea, recs=recs)


def _truth(pl):
    w, pos, al = pl["w"], pl["pos"], pl["al"]
    at = {int(p): k for k, p in enumerate(pos.tolist())}
    return [{at[p]: (0 if c == al[at[p], 0] else 1 if c == al[at[p], 1] else None) for p, c in w.meta["truth_allele"][r].items() if p in at}
            for r in pl["kept"].tolist()]


@pytest.mark.parametrize("ingest", ["0", "1"])
def test_device_entries_equal_the_restatement(planted, monkeypatch, ingest):
    from nanocaller_amd import generate_indel_pileups as gip
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import name_hash, phase_contig
    pl = planted
    # the input must separate the rules before anything else is worth checking
    st = compare_rules(pl["col"], pl["rea"], _truth(pl))
    print("column rule vs realignment:", st)
    assert st["differ"] >= 0.01 * st["pairs"] and st["corrected"] > 0 and st["gained"] > 0
    monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
    release_contig()
    res = phase_contig(pl["bam"], pl["fa"], pl["w"].chrom, pl["vcf"], 10, False, realign=True)
    assert bool(gip._DEV_INGEST) == (ingest == "1")                     # the route asked for is the route taken
    assert np.array_equal(res.reads["hash"], name_hash([pl["w"].names[r] for r in pl["kept"].tolist()]))      # the same reads in the same order
    off, site, allele = res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]
    got = _reads_of(off, site, allele)
    bad = [r for r in range(len(got)) if got[r] != pl["rea"][r]]
    assert not bad, "reads whose entries differ: %d, first %d: device %s, restatement %s" % (len(bad), bad[0], got[bad[0]], pl["rea"][bad[0]])
    assert got != pl["col"]
    pos = pl["pos"]
    g = dict(side=res.reads["side"], site_block=res.sites["block"], site_phased=res.sites["phased"], site_h=res.sites["h"], site_ps=res.sites["ps"],
             block_first=np.searchsorted(pos, [b[0] for b in res.blocks]), block_last=np.searchsorted(pos, [b[1] for b in res.blocks]),
             block_ps=[b[2] for b in res.blocks], block_cost=[b[3] for b in res.blocks],
             group_hp=np.zeros(res.reads["group"].max() + 1, np.uint8), group_ps=np.zeros(res.reads["group"].max() + 1, np.int32))
    g["group_hp"][res.reads["group"]] = res.reads["hp"]
    g["group_ps"][res.reads["group"]] = res.reads["ps"]
    _assert_equal_to_restatement(g, pl["rea"], pos, res.reads["group"], 15)
    assert res.sites["phased"].sum() > 50 and (res.reads["hp"] > 0).sum() > 100


def test_malformed_events_are_a_status(planted):
    """event offsets that point past the event arrays: NC_ERR_ARG from the export (the kernel checks every index before it reads)"""
    import ctypes as C

    import torch

    from nanocaller_amd import _lib
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.phase import _realign_inputs
    pl = planted
    eng = get_engine(0)
    dp, (codes, reads_c, n_ev, n_ins, refc) = _realign_inputs(pl["bam"], pl["fa"], pl["w"].chrom, False, 0)
    ev_off = dp.events["ev_off"].clone()
    ev_off[ev_off.numel() // 2:] += n_ev + 1000
    bad = _lib.IndelReadsC()
    C.memmove(C.byref(bad), C.byref(reads_c), C.sizeof(bad))
    bad.ev_off = ev_off.data_ptr()
    grp = np.arange(reads_c.n_reads, dtype=np.int32)
    torch.cuda.synchronize()
    with pytest.raises(_lib.NanoCallerHipError, match="malformed"):
        eng.snp_phase(pl["pos"], pl["al"], grp, grp.size, realign=(codes, bad, n_ev, n_ins, refc))
    ok = eng.snp_phase(pl["pos"], pl["al"], grp, grp.size, realign=(codes, reads_c, n_ev, n_ins, refc))      # the context works on
    assert _reads_of(ok["entry_off"], ok["entry_site"], ok["entry_allele"]) == pl["rea"]


def test_switch_off_is_the_column_rule(contig, monkeypatch):  # noqa: F811
    """realign=False (whatever the environment says): the PhaseResult of the column rule, array for array; a World cannot be realigned"""
    from nanocaller_amd import _lib
    from nanocaller_amd.phase import phase_contig
    w, recs, res = contig
    monkeypatch.setenv("NC_PHASE_REALIGN", "1")
    again = phase_contig(w, None, w.chrom, recs, 10, False, realign=False)
    assert again.records == res.records and again.blocks == res.blocks
    for part in ("sites", "reads", "haplotags"):
        a, b = getattr(again, part), getattr(res, part)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), part
    pos, rec = res.sites["pos"], res.sites["record"]
    al = []
    for i in rec.tolist():
        f = recs[i].split("\t")
        pair = (f[3], f[4]) if f[9].split(":")[0] == "0/1" else tuple(f[4].split(","))
        al.append([LETTER.index(pair[0]), LETTER.index(pair[1])])
    col = entries(w, res.reads["index"], pos, np.array(al).reshape(-1, 2), "column")
    assert _reads_of(res.reads["entry_off"], res.reads["entry_site"], res.reads["entry_allele"]) == col
    with pytest.raises(_lib.NanoCallerHipError, match="BAM"):
        phase_contig(w, None, w.chrom, recs, 10, False, realign=True)


def _bam_tags(path):
    """{read name: (HP, PS)} of the records of a BAM that carry HP"""
    from nanocaller_amd.vcfio import bgzf_read
    from test_bam_write import bam_records, split_aux
    out = {}
    for rb in bam_records(bgzf_read(path))[1]:
        body = rb[4:]
        name = bytes(body[32:32 + body[8] - 1]).decode()
        f = dict(split_aux(rb)[1])
        if b"HP" in f:
            ps = f[b"PS"]
            val = struct.unpack_from({"C": "<B", "S": "<H", "I": "<I", "c": "<b", "s": "<h", "i": "<i"}[chr(ps[2])], ps, 3)[0]
            out[name] = (f[b"HP"][3], int(val))
    return out


@pytest.fixture(scope="module")
def e2e_world(tmp_path_factory):
    w = make_realign_world(21, length=150_000)
    d = str(tmp_path_factory.mktemp("realign_e2e"))
    recs, bam, fa = _write(w, d)
    return w, recs, bam, fa, d


@pytest.mark.parametrize("ingest", ["0", "1"])
def test_phase_run_with_realignment(e2e_world, monkeypatch, ingest):
    """mode 'all', phaser='device', phase_realign=True, phased_bam=True: the phased VCF, the haplotag table and the BAM's HP / PS are those of
    phase_contig(realign=True)"""
    from nanocaller_amd import indelCaller
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.phase import name_hash, phase_contig, tags_for_names
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
    monkeypatch.delenv("NC_PHASE_REALIGN", raising=False)
    monkeypatch.delenv("NC_PHASED_BAM", raising=False)
    w, recs, bam, fa, d = e2e_world
    snp_vcf = _snp_vcf(bam, fa, w.chrom, w.length, os.path.join(d, "snp" + ingest))
    files, _ = _indels(bam, fa, w.chrom, w.length, os.path.join(d, "on" + ingest), "all", snp_vcf, phaser="device", phase_realign=True, phased_bam=True)
    snps = [ln for ln in gzip.open(snp_vcf, "rt") if not ln.startswith("#")]
    release_contig()
    want = phase_contig(bam, fa, w.chrom, snps, 10, False, realign=True)
    plain = phase_contig(bam, fa, w.chrom, snps, 10, False)
    out = [ln for ln in gzip.open(files["snps"], "rt") if not ln.startswith("#")]
    phased = lambda lines: sorted(ln for ln in lines if "|" in ln.split("\t")[9].split(":")[0])       # noqa: E731
    assert len(phased(out)) > 50 and phased(out) == phased(want.records)
    ph = os.path.join(d, "on" + ingest, "intermediate_phase_files")
    names = [r["name"] for r in recs]
    hp, ps = tags_for_names(names, os.path.join(ph, "%s.haplotags.npz" % w.chrom))
    table = dict(zip(want.haplotags["hash"].tolist(), zip(want.haplotags["hp"].tolist(), want.haplotags["ps"].tolist())))
    exp = [table.get(int(h), (0, 0)) for h in name_hash(names)]
    assert (hp > 0).sum() > 100 and list(zip(hp.tolist(), ps.tolist())) == exp
    tags = _bam_tags(os.path.join(ph, "%s.phased.bam" % w.chrom))
    assert tags == {n: (int(a), int(b)) for n, a, b in zip(names, hp, ps) if a}
    # the switch reaches the files: the column rule's table is another one on this world
    assert not (np.array_equal(plain.haplotags["hash"], want.haplotags["hash"]) and np.array_equal(plain.haplotags["hp"], want.haplotags["hp"])
                and plain.records == want.records)


def test_phase_run_default_files_unchanged(e2e_world, monkeypatch):
    """without the key and the variable, and with phase_realign=False against NC_PHASE_REALIGN=1: the same phased VCF bytes and haplotag table"""
    from nanocaller_amd import indelCaller
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    monkeypatch.delenv("NC_PHASE_REALIGN", raising=False)
    w, recs, bam, fa, d = e2e_world
    snp_vcf = _snp_vcf(bam, fa, w.chrom, w.length, os.path.join(d, "snp_d"))
    f1, i1 = _indels(bam, fa, w.chrom, w.length, os.path.join(d, "def"), "all", snp_vcf, phaser="device")
    monkeypatch.setenv("NC_PHASE_REALIGN", "1")
    f2, i2 = _indels(bam, fa, w.chrom, w.length, os.path.join(d, "off"), "all", snp_vcf, phaser="device", phase_realign=False)
    rd = lambda p: gzip.open(p, "rb").read()                              # noqa: E731
    assert rd(f1["snps"]) == rd(f2["snps"]) and i1 == i2
    t = [np.load(os.path.join(d, k, "intermediate_phase_files", "%s.haplotags.npz" % w.chrom)) for k in ("def", "off")]
    assert all(np.array_equal(t[0][k], t[1][k]) for k in ("hash", "hp", "ps")) and t[0]["hash"].size > 50

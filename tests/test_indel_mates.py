"""Kept alignments that share a read name on the device indel pipeline (nc_indel_set_mates; the <.., MATES = true> forms of k_hap_depth_b,
k_event_tiles and k_sets) against the REFERENCE's own outputs: tests/golden/indel_ont_mates.npz holds the tuples of
get_indel_testing_candidates and get_indel_testing_candidates_haploid (generate_indel_pileups.py:129-371, haploid twin) on a world with split
reads under dct['supplementary'] = True, and on the same world with every name made unique (tools/make_indel_mates_golden.py)."""
import gzip
import importlib.util
import json
import os
import types

import numpy as np
import pytest

from nanocaller_amd import _lib
from nanocaller_amd import generate_indel_pileups as gip

import bamio

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "indel_ont_mates.npz")
Z = np.load(GOLD)
CHUNKS = json.loads(str(Z["chunks"]))
DCT = json.loads(str(Z["dct"]))


def _tool():
    spec = importlib.util.spec_from_file_location("make_indel_mates_golden", os.path.join(HERE, "..", "tools", "make_indel_mates_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_holds_a_differing_site_for_every_planted_case():
    """from the golden alone: every case a .. e has a site inside one of its plants whose by-name answer differs from the per-alignment one"""
    got = _tool().fixture_condition(Z)
    assert all(got.get(c, 0) >= 1 for c in "abcde"), got


def test_the_generator_reproduces_the_committed_golden(tmp_path):
    """the generator runs the reference's own code (skipped only where the reference's directory does not exist, decided before any work: every
    failure of the generator itself fails the test); every array of the file it writes equals the committed one byte for byte (the zip
    container carries the time of writing)"""
    import subprocess
    import sys
    if not os.path.isdir(_tool().REFERENCE_SRC):
        pytest.skip("the reference is absent")
    out = str(tmp_path / "again.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "..", "tools", "make_indel_mates_golden.py"), out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    assert sorted(z.files) == sorted(Z.files)
    for k in Z.files:
        assert z[k].dtype == Z[k].dtype and z[k].shape == Z[k].shape and z[k].tobytes() == Z[k].tobytes(), k


def _fake_pack(sizes, hap, ps):
    """what indel_mate_table reads of a pack, on the CPU: every kept alignment a member, names of `sizes` consecutive alignments each"""
    import torch
    n = sum(sizes)
    first = np.repeat(np.cumsum([0] + sizes[:-1]), sizes)
    last = first + np.repeat(sizes, sizes) - 1
    idx = np.arange(n)
    rec4 = np.zeros((n, 4), np.int32)
    rec4[:, 0], rec4[:, 1], rec4[:, 2] = 100 + idx, 200 + idx, np.where(idx == last, first, idx + 1)
    slot = torch.arange(n + 1, dtype=torch.int64) * 112
    dp = types.SimpleNamespace(mates=(slot[:n].clone(), torch.from_numpy(rec4)), reads=dict(n_reads=n, slot_off=slot),
                               events=dict(read_hap=torch.tensor(hap, dtype=torch.uint8)))
    return dp, torch.tensor(ps, dtype=torch.int32)


def test_the_table_holds_the_names_tags_and_refuses_a_name_of_more_than_64_alignments():
    """rule 1 on the CPU: a name's mask is the OR over its records' HP, its PS is that of its last record (0 when that one has no HP); the kernels
    walk a name's ring for 64 alignments, so a name of exactly 64 is taken and one of 65 is NC_ERR_UNSUPPORTED"""
    assert gip.MATE_RING_CAP == 64
    sizes = [2, 3, 64, 2]
    hap = [1, 0] + [2, 0, 1] + [0] * 63 + [2] + [0, 0]
    ps = [11, 12] + [21, 22, 23] + list(range(100, 164)) + [31, 32]
    key, rec = gip.indel_mate_table(*_fake_pack(sizes, hap, ps))
    rec = rec.numpy()
    assert key.tolist() == [112 * i for i in range(71)] and rec[:, 3].tolist() == list(range(71))
    assert rec[:2, 4].tolist() == [1, 1] and rec[:2, 5].tolist() == [0, 0]             # the last record has no HP: phase_dict[name] = None
    assert rec[2:5, 4].tolist() == [3, 3, 3] and rec[2:5, 5].tolist() == [23] * 3      # HP 2 and HP 1 under one name: in both sets
    assert (rec[5:69, 4] == 2).all() and (rec[5:69, 5] == 163).all()                   # only the 64th record is tagged
    assert rec[69:, 4].tolist() == [0, 0] and rec[69:, 5].tolist() == [0, 0]
    assert rec[:, 2].tolist() == [1, 0, 3, 4, 2] + list(range(6, 69)) + [5, 70, 69]     # the rings are the pack's
    with pytest.raises(_lib.NanoCallerHipError) as e:
        gip.indel_mate_table(*_fake_pack([2, 65], [0] * 67, [0] * 67))
    assert getattr(e.value, "status", None) == _lib.NC_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("indelmates")
    out = {}
    for tag in ("name", "uniq"):
        w = bamio.world_from_arrays(Z, "w_")
        if tag == "name":
            w.names = ["r%07d" % i for i in Z["w_name_id"]]
        bam, fa = str(d / ("%s.bam" % tag)), str(d / ("%s.fa" % tag))
        bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, None))
        bamio.write_fasta(fa, w.chrom, w.ref)
        out[tag] = (w, bam, fa)
    return out


def _expected(tag, ci, haploid):
    pre = "%s_c%d_" % (tag, ci)
    if haploid:
        return Z[pre + "hpos"].tolist(), [Z[pre + "hx"]], [tuple(a) for a in json.loads(str(Z[pre + "halleles"]))], None
    return (Z[pre + "pos"].tolist(), [Z[pre + "x%d" % i] for i in range(3)], [[tuple(t) for t in a] for a in json.loads(str(Z[pre + "alleles"]))],
            json.loads(str(Z[pre + "phase"])))


def _run(files, tag, haploid, ingest, **kw):
    w, bam, fa = files[tag]
    dct = dict(DCT, fasta_path=fa, device_ingest=ingest, **kw)
    chunks = [dict(chrom=w.chrom, start=a, end=b, sam_path=bam) for a, b in CHUNKS]
    return gip.get_indel_testing_candidates_batch(dct, chunks, haploid=haploid)


def _compare(got, tag, haploid):
    assert len(got) == len(CHUNKS)
    n = 0
    for ci, t in enumerate(got):
        pos, xs, alleles, phase = _expected(tag, ci, haploid)
        assert list(t[0]) == pos, (tag, ci)
        n += len(pos)
        if not pos:
            continue
        if haploid:
            assert [tuple(a) for a in t[2]] == alleles
            gx = [t[1]]
        else:
            assert [[tuple(x) for x in a] for a in t[4]] == alleles
            assert list(t[5]) == phase
            gx = list(t[1:4])
        for g, e in zip(gx, xs):
            assert np.array_equal(np.asarray(g).astype(np.float32), e)
    assert n > 20


@pytest.mark.gpu
@pytest.mark.parametrize("ingest", [False, True], ids=["host_decode", "device_ingest"])
@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_shared_names_equal_the_reference_tuples(files, haploid, ingest):
    """the device pipeline keys the shared names as the reference does: tuple for tuple, on both ingest routes"""
    _compare(_run(files, "name", haploid, ingest), "name", haploid)


@pytest.mark.gpu
@pytest.mark.parametrize("ingest", [False, True], ids=["host_decode", "device_ingest"])
@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_unique_names_give_the_per_alignment_tuples(files, haploid, ingest):
    """the same alignments under unique names: no table, the plain kernels, the per-alignment answer"""
    _compare(_run(files, "uniq", haploid, ingest), "uniq", haploid)


@pytest.mark.gpu
@pytest.mark.parametrize("ingest", [False, True], ids=["host_decode", "device_ingest"])
def test_impute_indel_phase_on_shared_names_is_still_refused(files, ingest):
    with pytest.raises(_lib.NanoCallerHipError) as e:
        _run(files, "name", False, ingest, impute_indel_phase=True)
    assert getattr(e.value, "status", None) == _lib.NC_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- the whole caller on an untagged BAM
@pytest.fixture(scope="module")
def untagged(files, tmp_path_factory):
    """the shared-name world without HP / PS, and the SNP calls the phaser starts from (snpCaller under supplementary=True)"""
    from nanocaller_amd import snpCaller
    from nanocaller_amd.utils import get_chunks
    d = str(tmp_path_factory.mktemp("indelmates_all"))
    w, _, fa = files["name"]
    recs = [dict(r, tags={}) for r in bamio.world_to_records(w, None)]
    bam = os.path.join(d, "untagged.bam")
    bamio.write_bam(bam, w.chrom, w.length, recs)
    regions = [(w.chrom, 1, w.length, "diploid")]
    sp = dict(chunks_list=get_chunks(regions, 2), regions_list=regions, sam_path=bam, fasta_path=fa, mincov=4, maxcov=160, min_allele_freq=0.15,
              min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=2, vcf_path=os.path.join(d, "snp"), prefix="s", sample="SAMPLE",
              seq="ont", supplementary=True, exclude_bed=None, suppress_progress=True, disable_coverage_normalization=False)
    return w, recs, bam, fa, d, snpCaller.call_manager(sp)


def _call_manager(bam, fa, w, out, mode, snp_vcf=None, **kw):
    from nanocaller_amd import indelCaller
    from nanocaller_amd.generate_SNP_pileups import release_contig
    from nanocaller_amd.utils import get_chunks
    release_contig()
    os.makedirs(out, exist_ok=True)
    regions = [(w.chrom, 1, w.length, "diploid")]
    ip = dict(chunks_list=get_chunks(regions, 2, max_chunk_size=10_000), mode=mode, snp_vcf=snp_vcf, regions_list=regions, sam_path=bam, fasta_path=fa,
              mincov=4, maxcov=160, indel_model="ONT-HG002", cpu=2, vcf_path=out, prefix="t", sample="SAMPLE", seq="ont", del_t=0.6, ins_t=0.4,
              impute_indel_phase=False, supplementary=True, exclude_bed=None, win_size=40, small_win_size=4, enable_whatshap=False,
              suppress_progress=True, phase_qual_score=10, verbose=False, **kw)
    files = indelCaller.call_manager(ip)
    return files, [ln for ln in gzip.open(files["indels"], "rt")]


@pytest.mark.gpu
@pytest.mark.parametrize("ingest", ["0", "1"], ids=["host_decode", "device_ingest"])
def test_call_manager_all_with_the_device_phaser_on_an_untagged_shared_name_bam(untagged, monkeypatch, ingest):
    """indelCaller.call_manager(mode='all', supplementary=True, phaser='device') on a BAM without HP / PS whose kept alignments share names:
    phased, haplotagged, and the indel half -- which answered NC_ERR_UNSUPPORTED -- completes and writes the indel VCF.  The haplotag table is
    per NAME, so every record of a name gets one HP / PS: a BAM whose records carry exactly those tags, called with mode='indels', must give the
    same indel VCF records byte for byte (the table's way into the name masks and PS of indel_mate_table against the BAM tags' way)."""
    from nanocaller_amd import indelCaller
    from nanocaller_amd.phase import tags_for_names
    monkeypatch.setattr(indelCaller, "_whatshap_available", lambda: False)
    monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
    seen = []
    plain = gip.indel_sites_device
    monkeypatch.setattr(gip, "indel_sites_device", lambda *a, **k: (seen.append(k.get("mates")), plain(*a, **k))[1])
    w, recs, bam, fa, d, snp_vcf = untagged
    files, got = _call_manager(bam, fa, w, os.path.join(d, "all" + ingest), "all", snp_vcf, phaser="device")
    assert os.path.exists(files["indels"]) and os.path.exists(files["final"])
    assert got and got[0].startswith("##fileformat=VCF") and any(ln.startswith("#CHROM") for ln in got)
    assert seen and all(m is not None and m[0].numel() >= 12 for m in seen)      # six planted pairs: the table went into every plan
    tags = os.path.join(d, "all" + ingest, "intermediate_phase_files", "%s.haplotags.npz" % w.chrom)
    assert os.path.exists(tags)
    hp, ps = tags_for_names([r["name"] for r in recs], tags)
    re_bam = os.path.join(d, "retagged%s.bam" % ingest)
    bamio.write_bam(re_bam, w.chrom, w.length, [dict(r, tags={"HP": int(h), "PS": int(p)} if h else {}) for r, h, p in zip(recs, hp, ps)])
    _, exp = _call_manager(re_bam, fa, w, os.path.join(d, "re" + ingest), "indels")
    body = lambda lines: [ln for ln in lines if not ln.startswith("#")]           # noqa: E731
    print("ingest %s: %d reads tagged of %d, %d indel records" % (ingest, int((hp > 0).sum()), len(recs), len(body(got))))
    assert body(got) == body(exp)

"""The yardstick of known-sites calling for indels (tests/indel_genotype_ref.py) and the host pieces of the feature, on the CPU: the restatement
against the C oracle and the reference's goldens, the classes of the lists the GPU tests use, the VCF parser and its cache, the text of the
reference-call line, and the refusal of a list on the host-assembled route."""
import gzip
import os

import numpy as np
import pytest

from nanocaller_amd import generate_indel_pileups as gip
from nanocaller_amd import genotype_sites as gs
from nanocaller_amd import indel_device, indelCaller
from oracle import oracle

import indel_genotype_ref as R
from util import indel_impute_cases, indel_scan_cases, load_impute_world, load_world

KW = ("mincov", "win_size", "small_win_size", "ins_t", "del_t")


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_with_an_empty_list_the_restatement_is_the_c_oracle(haploid):
    w = load_world("indel")
    n = 0
    for c in indel_scan_cases(haploid=haploid):
        kw = {k: c[k] for k in KW}
        v, src, extra = R.scan_listed(w, c["start"], c["end"], exclude=c["exclude"], haploid=haploid, **kw)
        vp, vt = oracle.indel_scan(w, c["start"], c["end"], exclude=c["exclude"], haploid=haploid, **kw)
        assert sorted(v) == vp.tolist() == c["pos"].tolist() and [v[a] for a in sorted(v)] == vt.tolist() == c["type"].tolist()
        assert not src and not extra
        n += len(v)
    assert n > 50


def test_with_an_empty_list_the_imputed_restatement_is_the_references_golden():
    w = load_impute_world()
    for c in indel_impute_cases():
        kw = {k: c[k] for k in KW}
        v, src, extra = R.scan_listed(w, c["start"], c["end"], exclude=c["exclude"], impute=True, **kw)
        assert sorted(v) == c["pos"].tolist() and [v[a] for a in sorted(v)] == c["type"].tolist() and not src
        assert {a: (list(x), list(y)) for a, (x, y) in extra.items()} == c["extra"]


@pytest.mark.parametrize("haploid", [False, True], ids=["diploid", "haploid"])
def test_only_mode_with_the_natural_source_columns_reproduces_the_natural_anchors(haploid):
    """S = the columns at which the natural walk wrote its anchors, with the classes of the rules that fired there: the list alone gives the same
    anchors, types included"""
    w = load_world("indel")
    n = 0
    for c in indel_scan_cases(haploid=haploid)[:4]:
        kw = {k: c[k] for k in KW}
        tr = {}
        v, _, _ = R.scan_listed(w, c["start"], c["end"], exclude=c["exclude"], haploid=haploid, trace=tr, **kw)
        S = {col: what == "long" for col, what in tr.items() if what in ("long", "small")}
        v2, src, _ = R.scan_listed(w, c["start"], c["end"], exclude=c["exclude"], haploid=haploid, sites=S, only=True, **kw)
        assert v2 == v and set(src) == set(v) and set(src.values()) <= set(S)
        n += len(v)
    assert n > 40


def test_every_class_of_listed_column_has_a_member_in_the_gpu_tests_lists():
    w = R.listed_world()
    seen = {c: 0 for c in R.CLASSES}
    for case in R.CASES.values():
        cl = R.site_classes(w, case)
        pos, lng = R.site_list(w, case)
        listed = set(pos.tolist())
        assert 90 <= len(pos) <= 140 or case["name"] == "imp"
        assert len(pos) > len(listed)                                  # a tenth listed twice
        for c, members in cl.items():
            seen[c] += len(listed & set(members))
        both = [p for p in cl["both_classes"] if sorted(lng[pos == p].tolist())[:1] == [0] and lng[pos == p].max() == 1]
        assert both and all(R.as_dict(pos, lng)[p] for p in both)     # listed with both classes: long
    assert all(n >= 1 for n in seen.values()), seen
    # the classes do what their names say in the walk WITH the list (the diploid case)
    case = R.CASES["dip"]
    S = R.as_dict(*R.site_list(w, case))
    kw = {k: case[k] for k in KW}
    cl = R.site_classes(w, case)
    tr, anchors, srcs = {}, {}, {}
    for a, b in case["chunks"]:
        v, src, _ = R.scan_listed(w, a, b, exclude=case["exclude"], sites=S, trace=tr, **kw)
        anchors.update(v)
        srcs.update(src)
    listed = lambda c: [p for p in cl[c] if p in S]                    # noqa: E731
    assert all(tr[p] == "forced" for p in listed("no_event") if p not in cl["in_listed_skip"][1::2] and tr[p] != "skipped")
    assert all(tr.get(p) in ("no_reads", None) for p in listed("no_reads")) and all(tr[p] == "excluded" for p in listed("excluded"))
    assert all(tr[p] in ("depth", "skipped") for p in listed("hap_below_mincov"))
    assert all(tr[p] in ("long", "skipped") for p in listed("natural_long"))
    assert 1 in anchors and srcs.get(1, 0) in range(1, 12)              # a column <= 10: the anchor is clipped to 1
    first, second = cl["in_listed_skip"][0], cl["in_listed_skip"][1]
    assert tr[first] == "forced" and tr[second] == "skipped" and second - first == 5
    assert all(p not in tr for p in cl["outside"] + cl["off_contig"])


def test_the_parser_takes_indel_lines_by_allele_length_and_caches_per_file(tmp_path):
    body = ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
            "c1\t100\t.\tA\tG\t.\t.\t.\n"                              # SNP: skipped
            "c1\t200\t.\tA\tAT\t.\t.\t.\n"                             # small
            "c1\t300\t.\tA" + "C" * 11 + "\tA\t.\t.\t.\n"              # an 11-base deletion: long
            "c1\t400\t.\tAC\tA,ACGTGTGTGTGTGT\t.\t.\t.\n"              # multi-allelic: -1 and +12 -> long
            "c1\t500\t.\tAC\tGT\t.\t.\t.\n"                            # MNP: no length change
            "c1\t600\t.\tA\tG,AT\t.\t.\t.\n"                           # SNP + insertion: listed, small
            "c1\t200\t.\tA\tA" + "T" * 12 + "\t.\t.\t.\n"              # the same column again, long: long wins
            "c2\t7\t.\tAAAAAAAAAAA\tA\t.\t.\t.\n")                     # exactly 10: small
    plain = tmp_path / "s.vcf"
    plain.write_text(body)
    got = gs.parse_indel_sites_vcf(str(plain))
    assert got["c1"][0].tolist() == [200, 300, 400, 600] and got["c1"][1].tolist() == [1, 1, 1, 0]
    assert got["c2"][0].tolist() == [7] and got["c2"][1].tolist() == [0]
    assert got["c1"][0].dtype == np.int32 and got["c1"][1].dtype == np.uint8
    # the SNP parser keeps its behaviour on the same file
    snps, skipped = gs.parse_sites_vcf(str(plain))
    assert snps["c1"].tolist() == [100, 200, 600] and skipped == 4
    # gzipped and bgzipped files
    gz = tmp_path / "s.vcf.gz"
    with gzip.open(gz, "wt") as f:
        f.write(body)
    from nanocaller_amd import vcfio
    bgz = str(tmp_path / "b.vcf.gz")
    hdr, recs = vcfio.read_vcf_gz(str(plain))
    vcfio.write_sorted_vcf(bgz, "".join(hdr), recs, ["c1", "c2"])
    for path in (str(gz), bgz):
        again = gs.parse_indel_sites_vcf(path)
        assert {c: (p.tolist(), g.tolist()) for c, (p, g) in again.items()} == {c: (p.tolist(), g.tolist()) for c, (p, g) in got.items()}
    # once per file; a rewritten file is read again
    a = gs.load_indel_sites_vcf(str(plain))
    assert gs.load_indel_sites_vcf(str(plain)) is a
    plain.write_text(body + "c2\t9\t.\tA\tAG\t.\t.\t.\n")
    os.utime(plain, ns=(1, 1))
    b = gs.load_indel_sites_vcf(str(plain))
    assert b is not a and b["c2"][0].tolist() == [7, 9]
    # the keys: a path, {contig: positions}, {contig: (positions, is_long)}; the environment stands in when the keys are absent
    p, g, only = gs.indel_sites_for(dict(genotype_indel_sites=str(plain)), "c2")
    assert p.tolist() == [7, 9] and g.tolist() == [0, 0] and only is False
    p, g, only = gs.indel_sites_for(dict(genotype_indel_sites={"c1": [9, 5, 5, 0, -3]}, genotype_indel_only=1), "c1")
    assert p.tolist() == [5, 9] and g.tolist() == [0, 0] and only is True
    p, g, only = gs.indel_sites_for(dict(genotype_indel_sites={"c1": ([9, 5, 5], [0, 0, 1])}), "c1")
    assert p.tolist() == [5, 9] and g.tolist() == [1, 0]
    assert gs.indel_sites_for(dict(genotype_indel_sites={"c1": [5]}), "c9")[0].size == 0
    assert gs.indel_sites_for({}, "c1") == (None, None, False)
    assert gs.sites_for(dict(genotype_indel_sites={"c1": [5]}), "c1") == (None, False)          # the SNP half does not read the indel key


def test_the_environment_stands_in_for_the_keys(tmp_path, monkeypatch):
    v = tmp_path / "e.vcf"
    v.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc1\t200\t.\tA\tAT\t.\t.\t.\n")
    monkeypatch.setenv("NC_GENOTYPE_INDEL_SITES", str(v))
    monkeypatch.setenv("NC_GENOTYPE_INDEL_ONLY", "1")
    p, g, only = gs.indel_sites_for({}, "c1")
    assert p.tolist() == [200] and only is True
    assert gs.indel_sites_for(dict(genotype_indel_sites=None), "c1") == (None, None, False)       # a key that is present decides


@pytest.mark.parametrize("haploid,prob,exp", [
    (False, [0.97, 0.01, 0.01, 0.01], b"chr9\t1234\t.\tG\t.\t15.23\tREF\t.\tGT:GQ\t./.:15.23\n"),
    (False, [1.0, 0.0, 0.0, 0.0], b"chr9\t1234\t.\tG\t.\t60.00\tREF\t.\tGT:GQ\t./.:60.00\n"),
    (False, [0.95, 0.05, 0.0, 0.0], b"chr9\t1234\t.\tG\t.\t0.00\tLOW\t.\tGT:GQ\t./.:0.00\n"),
    (True, [0.25], b"chr9\t1234\t.\tG\t.\t6.02\tREF\t.\tGT:GQ\t./.:6.02\n"),
    (True, [0.0], b"chr9\t1234\t.\tG\t.\t60.00\tREF\t.\tGT:GQ\t./.:60.00\n"),
    (True, [0.5], b"chr9\t1234\t.\tG\t.\t0.00\tLOW\t.\tGT:GQ\t./.:0.00\n"),
])
def test_the_reference_call_line(haploid, prob, exp):
    """min(99, -10 log10(1e-6 + 1 - 0.97)) = 15.23; a certain reference call is capped by the 1e-6: 60.00"""
    assert indel_device.reference_call_line(b"chr9", 1234, b"G", np.asarray(prob, np.float64), haploid) == exp
    assert indelCaller._non_snp(exp.decode()) and not indelCaller._non_snp("chr9\t5\t.\tA\tG\t1\tPASS\t.\tGT\t0/1\n")


def test_reference_calls_are_merged_by_position_and_never_move_prev():
    """_with_reference_calls on a made-up run: site 1 has a record; site 2 (forced) lies inside it; site 3 (forced) got no record -> one line at its
    column, after the record of site 4 that precedes that column; site 5 is natural without a record: nothing"""
    r = dict(pos=np.array([100, 105, 200, 205, 300], np.int32), chunk=np.zeros(5, np.int32), src=np.array([0, 115, 240, 0, 0], np.int32))
    text = b"c\t100\t.\tACGTACGTAC\tA\t9.00\tPASS\t.\tGT:GQ\t1/1:9.00\nc\t205\t.\tA\tAT\t9.00\tPASS\t.\tGT:GQ\t1/1:9.00\n"
    probs = np.array([[0.1, 0.9, 0, 0], [0.99, 0, 0, 0], [0.99, 0.01, 0, 0], [0.1, 0.9, 0, 0], [0.99, 0, 0, 0]], np.float32)
    ctg = dict(fasta_b=b"a" * 400)
    out = indel_device._with_reference_calls(r, probs, b"c", [text], ctg, False)
    lines = out[0].splitlines(keepends=True)
    assert [ln.split(b"\t")[1] for ln in lines] == [b"100", b"205", b"240"]
    assert lines[2] == indel_device.reference_call_line(b"c", 240, b"A", probs[2], False) and b"\tREF\t" in lines[2]
    assert r["genotype_inside"] == 1 and r["genotype_recorded"] == 1


def test_the_header_gains_the_two_filters_only_with_a_list():
    p = dict(sample="S")
    plain = indelCaller.indel_vcf_header(p, ["c1"])
    assert plain == indelCaller.INDEL_VCF_HEADER.format(contigs="##contig=<ID=c1>\n", sample="S")
    listed = indelCaller.indel_vcf_header(dict(p, genotype_indel_sites={"c1": [5]}), ["c1"])
    from nanocaller_amd.snpCaller import VCF_HEADER
    for key in ("REF", "LOW"):
        ln = [x for x in listed.split("\n") if x.startswith("##FILTER=<ID=%s," % key)]
        assert len(ln) == 1 and ln[0] + "\n" in VCF_HEADER and ("ID=%s," % key) not in plain
    assert listed.replace(indelCaller.INDEL_GENOTYPE_FILTERS, "") == plain


def test_a_list_and_a_host_part_raise():
    chunks = [dict(chrom="c1", start=1, end=1000, sam_path="x.bam"), dict(chrom="c1", start=1000, end=2000, sam_path="x.bam")]
    d = dict(genotype_indel_sites={"c1": [50]})
    assert gip.plan_routes(d, chunks, False) == [("device", [0, 1], d)]
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        gip.plan_routes(d, chunks, False, route="host")
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        gip.plan_routes(d, [dict(c, sam_path=object()) for c in chunks], False)                   # not a BAM path
    nested = [dict(chrom="c1", start=1, end=2000, sam_path="x.bam"), dict(chrom="c1", start=5, end=1000, sam_path="x.bam")]
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        gip.plan_routes(d, nested, False)
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        gip.plan_routes(dict(d, impute_indel_phase=True), chunks, False, route="split", mask=[True, False])
    # without a list the same plans stand
    assert gip.plan_routes({}, chunks, False, route="host") == [("host", [0, 1], {})]
    # the capacity redo of a device part is a host part too
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        gip._no_list_on_host(d, chunks)


def test_a_list_off_the_native_device_route_raises_in_indel_run_and_in_the_per_chunk_functions(tmp_path, monkeypatch):
    """an external aligner (MUSCLE on PATH makes it the default; aligner=) takes the per-chunk functions, which never see the plan of routes; the
    Python rules write no REF / LOW line: all of these raise before the GPU is opened, a list is never ignored"""
    import queue
    from nanocaller_amd.generate_indel_pileups_haploid import get_indel_testing_candidates_haploid
    listed = dict(genotype_indel_sites={"c1": [50]}, intermediate_indel_files_dir=str(tmp_path), prefix="t", indel_model="ONT-HG002")
    chunk = dict(chrom="c1", start=1, end=1000, sam_path="x.bam", ploidy="diploid")

    def run(params, **kw):
        jobs = queue.Queue()
        jobs.put(("indel", chunk))
        return indelCaller.indel_run(params, {}, jobs, queue.Queue(), [], **kw)
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        run(listed, aligner=gip.muscle_aligner)
    monkeypatch.setattr(gip, "default_aligner", lambda: gip.muscle_aligner)          # as with `muscle` on PATH
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        run(listed)
    monkeypatch.setattr(gip, "default_aligner", lambda: gip.star_aligner)
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        run(listed, rules="python")
    monkeypatch.setenv("NC_GENOTYPE_INDEL_SITES", str(tmp_path / "absent.vcf"))       # the environment's list counts too
    with pytest.raises(ValueError, match="genotype_indel_sites"):
        run({k: v for k, v in listed.items() if k != "genotype_indel_sites"}, aligner=gip.muscle_aligner)
    monkeypatch.delenv("NC_GENOTYPE_INDEL_SITES")
    assert not list(tmp_path.iterdir())                                                 # nothing was written
    for fn in (gip.get_indel_testing_candidates, get_indel_testing_candidates_haploid):
        with pytest.raises(ValueError, match="genotype_indel_sites"):
            fn(listed, chunk, aligner=gip.muscle_aligner)
        with pytest.raises(ValueError, match="genotype_indel_sites"):
            fn(listed, chunk)


def test_by_name_and_per_alignment_depths_part_on_the_shared_names_list():
    """the GPU test of shared names lists the columns where two alignments of a name overlap, at R.MATES_MINCOV: there the by-name depth test and
    the per-alignment one give different verdicts (in both directions: a name counted once, a name on both haplotype planes), so a kernel that
    counted alignments would fail it; at the mates golden's own mincov 4 they do not part, which is why the case raises it"""
    import bamio
    import test_indel_mates as tim
    w = bamio.world_from_arrays(tim.Z, "w_")
    w.names = ["r%07d" % i for i in tim.Z["w_name_id"]]
    cols = R.mates_columns(w, 1, 4_001)
    assert len(cols) > 500
    kw = dict(supplementary=True)
    a, b = R.depth_verdicts(w, cols, mincov=R.MATES_MINCOV, by_name=True, **kw), R.depth_verdicts(w, cols, mincov=R.MATES_MINCOV, by_name=False, **kw)
    differ = [v for v in cols if a[v] != b[v]]
    assert len(differ) >= 20 and any(a[v] for v in differ) and any(b[v] for v in differ)
    a4, b4 = R.depth_verdicts(w, cols[::5], mincov=4, by_name=True, **kw), R.depth_verdicts(w, cols[::5], mincov=4, by_name=False, **kw)
    assert a4 == b4
    # depth_verdicts is the walk's own depth test: a forced column of the full walk passes it
    tr = {}
    S = {v: False for v in cols[::15]}
    R.scan_listed(w, 1, 4_001, mincov=R.MATES_MINCOV, win_size=40, small_win_size=4, ins_t=0.4, del_t=0.6, sites=S, only=True, by_name=True, trace=tr, **kw)
    assert all(a[v] == (tr[v] == "forced") for v in S if tr.get(v) != "skipped") and sum(tr.get(v) == "forced" for v in S) > 10

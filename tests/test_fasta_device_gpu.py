"""GPU: the reference FASTA on the device (csrc/nc_fasta.hip k_fasta_decode, device_fasta.py) against the unchanged host code -- letters ==
bam.read_fasta_bytes on the plain file, scan codes == DeviceBam._ref_lut's rule placed on the grid, blind codes == phase._ref_codes -- on every
line length / terminator / contig length / grid offset at which the decoder takes another path, on bgzipped twins cut into members anywhere,
on files it must refuse (a status, never a fault), and end to end: the callers' output from a .fa.gz is that from its plain twin, byte for byte.
Every comparison is exact equality."""
import os
import queue

import numpy as np
import pytest

import bamio
import fastaio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    e = get_engine(0)
    e.use_torch_stream()
    return e


def scan_rule(letters, scan_pos0, scan_len, ga, gb):
    """DeviceBam._ref_lut's rule (upper-case AGTC -> 0..3, everything else 4) on the letters of [ga, gb], entry p - scan_pos0; 4 elsewhere"""
    lut = np.full(256, 4, np.uint8)
    for i, ch in enumerate("AGTC"):
        lut[ord(ch)] = i
    out = np.full(scan_len, 4, np.uint8)
    a = np.frombuffer(letters, np.uint8)
    for p in range(max(1, ga), min(len(a), gb) + 1):
        s = p - scan_pos0
        if 0 <= s < scan_len:
            out[s] = lut[a[p - 1]]
    return out


def scan_rule_fast(letters, scan_pos0, scan_len, ga, gb):
    """the same with slices (what the tests compare with; test_the_two_statements_of_the_scan_rule_agree ties it to the loop above)"""
    lut = np.full(256, 4, np.uint8)
    for i, ch in enumerate("AGTC"):
        lut[ord(ch)] = i
    out = np.full(scan_len, 4, np.uint8)
    a = np.frombuffer(letters, np.uint8)
    lo, hi = max(1, ga, scan_pos0), min(len(a), gb, scan_pos0 + scan_len - 1)
    if hi >= lo:
        out[lo - scan_pos0:hi - scan_pos0 + 1] = lut[a[lo - 1:hi]]
    return out


def grids(length):
    """(scan_pos0, scan_len, ga, gb): the grid on and off the 16-grid of the letters, inside and around the contig, [ga, gb] inside it where it
    has the room; a grid that starts before position 1; a grid none of the contig lies on"""
    out = []
    for pos0 in (1, 2, 17, 2049):
        ga, gb = (2, length - 1) if length >= 3 else (1, length)
        out.append((pos0, max(1, length - pos0 + 1 + 21), max(ga, pos0), gb))
        if pos0 in (2, 17):
            out.append((pos0, max(1, (length - pos0) // 2), ga + 3, gb)) # the grid ends inside the contig
    out.append((-30, length + 64, 1, length))
    out.append((1, 40, 5, 4))                                            # gb < ga: all 4
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """[(plain path, rows, {name: sequence})] as in test_fasta_formats"""
    root = tmp_path_factory.mktemp("fasta_device")
    rng = np.random.default_rng(12)
    out = []
    for lb in fastaio.LBS:
        for eol in ("\n", "\r\n"):
            for last_full, last_eol in ((True, False), (False, True)):
                p = str(root / ("lb%d_%s_%d%d.fa" % (lb, "lf" if eol == "\n" else "crlf", last_full, last_eol)))
                rows, seqs = fastaio.write_case_file(p, rng, lb, eol, last_full, last_eol)
                out.append((p, rows, seqs))
    for name, n, lb, eol in (("long", 200_003, 60, "\n"), ("long_crlf", 200_003, 61, "\r\n"), ("single", 5_000, 5_000, "\n")):
        p = str(root / (name + ".fa"))
        contigs = [("head a contig in front", fastaio.random_sequence(rng, 777)), (name + " the long one", fastaio.random_sequence(rng, n))]
        rows = fastaio.write_fasta_lines(p, contigs, lb, eol)
        out.append((p, rows, {h.split()[0]: s for h, s in contigs}))
    return out


def test_kernel_against_the_host_readers(eng, files):
    """nc_fasta_decode on the whole file image: every contig of every file, every grid"""
    import torch
    from nanocaller_amd.bam import read_fasta_bytes
    from nanocaller_amd.phase import _ref_codes
    n_calls = 0
    for p, rows, seqs in files:
        with open(p, "rb") as f:
            data = f.read()
        # (the image at an odd address as well: the staging loads align themselves on the address, not on the offset)
        pad = torch.from_numpy(np.frombuffer(b"\x00" * 3 + data, np.uint8).copy()).to(eng.device)
        for shift in ((3, 0) if "_01." in os.path.basename(p) else (3,)):
            raw = pad[shift:] if shift == 3 else pad[:]
            base = 0 if shift == 3 else 3
            for name, length, offset, lb, lw in rows:
                want = read_fasta_bytes(p, name)
                assert want == seqs[name].encode("ascii")
                letters = torch.full((length + 16,), 0xEE, dtype=torch.uint8, device=eng.device)
                blind = torch.full((length + 16,), 0xEE, dtype=torch.uint8, device=eng.device)
                eng.fasta_decode(raw, base + offset, length, lb, lw, letters=letters, blind=blind)
                n_calls += 1
                assert letters[:length].cpu().numpy().tobytes() == want
                assert np.array_equal(blind[:length].cpu().numpy(), _ref_codes(want.decode("ascii")))
                assert bool((letters[length:] == 0xEE).all()) and bool((blind[length:] == 0xEE).all())     # nothing behind the arrays' ends
                for pos0, scan_len, ga, gb in grids(length):
                    scan = torch.full((scan_len + 16,), 0xEE, dtype=torch.uint8, device=eng.device)
                    eng.fasta_decode(raw, base + offset, length, lb, lw, scan=scan[:scan_len], scan_pos0=pos0, ga=ga, gb=gb)
                    n_calls += 1
                    got = scan.cpu().numpy()
                    assert np.array_equal(got[:scan_len], scan_rule_fast(want, pos0, scan_len, ga, gb)), (p, name, pos0, scan_len, ga, gb)
                    assert (got[scan_len:] == 0xEE).all()
    assert n_calls > 2000


def test_the_two_statements_of_the_scan_rule_agree():
    rng = np.random.default_rng(1)
    s = fastaio.random_sequence(rng, 3000).encode("ascii")
    for pos0, scan_len, ga, gb in grids(3000):
        assert np.array_equal(scan_rule(s, pos0, scan_len, ga, gb), scan_rule_fast(s, pos0, scan_len, ga, gb))
    lut_rule = scan_rule(b"ACGTacgtNn*RY", 1, 13, 1, 13)
    assert lut_rule.tolist() == [0, 3, 1, 2, 4, 4, 4, 4, 4, 4, 4, 4, 4]


def _check_contig(c, want, tile_pos0=-14, tile=2048):
    from nanocaller_amd.phase import _ref_codes
    n = c.length
    assert n == len(want)
    assert c.letters.cpu().numpy().tobytes() == want
    assert np.array_equal(c.blind_codes.cpu().numpy(), _ref_codes(want.decode("ascii")))
    assert c.host_letters() == want
    ref_len = (n - tile_pos0 + tile) // tile * tile
    ga, gb = max(1, tile_pos0), min(n, tile_pos0 + ref_len - 1)
    got = c.scan_codes(tile_pos0, ref_len, ga, gb).cpu().numpy()
    assert np.array_equal(got, scan_rule_fast(want, tile_pos0, ref_len, ga, gb))


TWINS = [dict(sizes=(0xff00,), gzi=True), dict(sizes=(0xff00,), gzi=False), dict(sizes=None, gzi=False), dict(sizes=None, gzi=True, levels=(0,)),
         dict(sizes=None, gzi=True, levels=(6, 0, 1, 9)), dict(sizes=(0xff00,), gzi=True, levels=(0,))]


@pytest.mark.parametrize("twin", range(len(TWINS)))
def test_device_fasta_plain_and_bgzipped(eng, files, twin):
    """DeviceFasta.contig on the plain file and on its bgzipped twin (members of 0xff00 bytes; irregular members of 1 to 300 bytes whose cuts
    fall mid-line and between \\r and \\n; stored members; with .gzi and without): every contig starts and ends in the middle of members"""
    from nanocaller_amd import device_fasta, fasta
    from nanocaller_amd.bam import read_fasta_bytes
    rng = np.random.default_rng(200 + twin)
    kw = dict(TWINS[twin])
    picked = [f for f in files if any(t in os.path.basename(f[0]) for t in ("lb1_crlf_01", "lb17_crlf_10", "lb60_lf_01", "lb64_crlf_01", "long", "single"))]
    assert len(picked) == 7
    for p, rows, seqs in picked:
        if kw["sizes"] is None:
            kw["sizes"] = [int(x) for x in rng.integers(1, 301, 257)]
        gz = fastaio.bgzip_twin(p, **kw)
        fasta.forget()
        for path in ((p, gz) if twin == 0 else (gz,)):
            df = device_fasta.open_device_fasta(path, 0)
            for name in seqs:
                _check_contig(df.contig(name), read_fasta_bytes(p, name))
        device_fasta.release()
        for ext in ("", ".fai", ".gzi"):
            if os.path.exists(gz + ext):
                os.remove(gz + ext)


def test_illegal_inputs_are_a_status(eng, tmp_path):
    """a terminator slot holding a letter, a control byte among the bases, first + span one past raw_len: NC_ERR_ARG with the status word set,
    and the next call on the same context decodes as if nothing had been"""
    import torch
    from nanocaller_amd._lib import NanoCallerHipError
    rng = np.random.default_rng(5)
    seq = fastaio.random_sequence(rng, 9_000)
    p = str(tmp_path / "r.fa")
    (name, length, offset, lb, lw), = fastaio.write_fasta_lines(p, [("c", seq)], 60, "\r\n")
    data = np.frombuffer(open(p, "rb").read(), np.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=eng.device)

    def decode(arr, raw_len=None, first=offset):
        raw = torch.from_numpy(arr.copy()).to(eng.device)
        letters = torch.empty(length, dtype=torch.uint8, device=eng.device)
        scan = torch.empty(length, dtype=torch.uint8, device=eng.device)
        eng.fasta_decode(raw, first, length, lb, lw, letters=letters, scan=scan, blind=None, status=status, raw_len=raw_len)
        return letters.cpu().numpy().tobytes()
    assert decode(data) == seq.encode("ascii") and int(status.item()) == 0
    for what, at, byte, bit in (("\\r slot", offset + 60 + 40 * lw, ord("A"), 1), ("\\n slot", offset + 61 + 100 * lw, ord("G"), 1),
                                ("control byte", offset + 4_500 // 60 * lw + 7, 0x09, 2), ("byte above 0x7e", offset + 3, 0x80, 2)):
        bad = data.copy()
        bad[at] = byte
        with pytest.raises(NanoCallerHipError, match="does not describe this file"):
            decode(bad)
        assert int(status.item()) == bit, what
    span = ((length - 1) // lb) * lw + (length - 1) % lb + 1
    with pytest.raises(NanoCallerHipError, match="does not describe this file"):
        decode(data, raw_len=offset + span - 1)
    assert int(status.item()) == 4
    with pytest.raises(NanoCallerHipError, match="linebases"):
        eng.fasta_decode(torch.zeros(64, dtype=torch.uint8, device=eng.device), 0, 10, 0, 1, status=status)
    with pytest.raises(NanoCallerHipError, match="neither 1"):
        eng.fasta_decode(torch.zeros(64, dtype=torch.uint8, device=eng.device), 0, 10, 5, 8, status=status)
    assert decode(data, raw_len=offset + span) == seq.encode("ascii") and int(status.item()) == 0     # (the file's last terminator is not needed)


def test_a_member_with_a_wrong_crc_names_the_member(eng, tmp_path):
    from nanocaller_amd import device_fasta
    from nanocaller_amd._lib import NanoCallerHipError
    rng = np.random.default_rng(6)
    seq = fastaio.random_sequence(rng, 5_000)
    p = str(tmp_path / "s.fa")
    rows = fastaio.write_fasta_lines(p, [("a", seq)], 60)
    data = open(p, "rb").read()
    gz = p + ".gz"
    ent = fastaio.write_bgzf(gz, data, sizes=(700,), level=0)            # stored: a flipped byte leaves the stream valid, only the CRC tells
    fastaio.write_fai(gz + ".fai", rows)
    raw = bytearray(open(gz, "rb").read())
    raw[ent[2][0] + 18 + 5 + 100] ^= 0x01
    with open(gz, "wb") as f:
        f.write(bytes(raw))
    with pytest.raises(NanoCallerHipError, match="member at byte %d fails its CRC-32" % ent[2][0]):
        device_fasta.open_device_fasta(gz, 0).contig("a").letters
    device_fasta.release()
    good = fastaio.bgzip_twin(p, sizes=(700,), levels=(0,))
    assert device_fasta.open_device_fasta(good, 0).contig("a").host_letters() == seq.encode("ascii")
    device_fasta.release()


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def world_files(tmp_path_factory):
    """bamio.make_bam_world's BAM, its reference (a soft-masked run, a contig in front of it) as a plain FASTA and as its bgzipped twin"""
    d = tmp_path_factory.mktemp("fasta_e2e")
    w = bamio.make_bam_world(seed=5, length=60_000, depth=14)
    bam = str(d / "w.bam")
    bamio.write_bam(bam, w.chrom, w.length, bamio.world_to_records(w, np.random.default_rng(2)))
    ref = w.ref[:20_000] + w.ref[20_000:20_300].lower() + w.ref[20_300:]
    fa = str(d / "w.fa")
    rng = np.random.default_rng(3)
    fastaio.write_fasta_lines(fa, [("decoy a contig in front of the one the BAM names", fastaio.random_sequence(rng, 1_234)), (w.chrom + " the contig", ref)], 60)
    gz = fastaio.bgzip_twin(fa, sizes=(4093, 300, 1, 0xff00), levels=(6, 0), gzi=True)
    return w, bam, fa, gz, str(d)


def _snp_worker_file(bam, fa, w, out, **extra):
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp, snpCaller
    gsp.release_contig()
    device_bam.release()
    os.makedirs(out, exist_ok=True)
    chunks = [dict(chrom=w.chrom, start=s, end=min(w.length, s + 30_000), ploidy="diploid") for s in range(1, w.length, 30_000)]
    params = dict(chunks_list=chunks, regions_list=[(w.chrom, 1, w.length, "diploid")], sam_path=bam, fasta_path=fa, mincov=4, maxcov=160,
                  min_allele_freq=0.15, min_nbr_sites=1, threshold=[0.4, 0.6], snp_model="ONT-HG002", cpu=2, vcf_path=out, prefix="t",
                  sample="S", seq="ont", supplementary=False, exclude_bed=None, suppress_progress=True,
                  disable_coverage_normalization=False, intermediate_snp_files_dir=out, **extra)
    q = queue.Queue()
    for c in chunks:
        q.put(c)
    made = []
    snpCaller.caller(params, q, queue.Queue(), made)
    gsp.release_contig()
    return open(made[0], "rb").read()


@pytest.fixture()
def decode_calls(monkeypatch):
    """counts Engine.fasta_decode calls: which route a run took"""
    from nanocaller_amd.engine import Engine
    calls = []
    real = Engine.fasta_decode

    def spy(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(Engine, "fasta_decode", spy)
    return calls


def test_snp_caller_output_is_the_plain_twins(world_files, monkeypatch, decode_calls):
    w, bam, fa, gz, d = world_files
    monkeypatch.delenv("NC_DEVICE_INGEST", raising=False)
    monkeypatch.delenv("NC_DEVICE_FASTA", raising=False)
    plain = _snp_worker_file(bam, fa, w, os.path.join(d, "snp_plain"))
    assert plain.count(b"\n") > 50 and not decode_calls                  # the default for a plain file: the host reader, as before
    from_gz = _snp_worker_file(bam, gz, w, os.path.join(d, "snp_gz"))
    assert decode_calls and from_gz == plain
    del decode_calls[:]
    monkeypatch.setenv("NC_DEVICE_FASTA", "1")
    assert _snp_worker_file(bam, fa, w, os.path.join(d, "snp_plain_dev")) == plain and decode_calls
    del decode_calls[:]
    assert _snp_worker_file(bam, fa, w, os.path.join(d, "snp_plain_key_off"), device_fasta=False) == plain and not decode_calls
    monkeypatch.delenv("NC_DEVICE_FASTA")
    assert _snp_worker_file(bam, fa, w, os.path.join(d, "snp_plain_key_on"), device_fasta=True) == plain and decode_calls
    del decode_calls[:]
    monkeypatch.setenv("NC_DEVICE_INGEST", "0")
    assert _snp_worker_file(bam, gz, w, os.path.join(d, "snp_gz_host")) == plain and not decode_calls


def test_single_contig_entry_points(world_files, monkeypatch, decode_calls):
    """generate_SNP_pileups.device_pack_for with dct['device_ingest']: the pack's reference codes from the .fa.gz are the plain twin's"""
    import torch
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp
    w, bam, fa, gz, d = world_files
    monkeypatch.delenv("NC_DEVICE_FASTA", raising=False)
    packs = {}
    for tag, path in (("plain", fa), ("gz", gz)):
        gsp.release_contig()
        dp = gsp.device_pack_for(dict(sam_path=bam, fasta_path=path, supplementary=False, exclude_bed=[(w.chrom, 100, 180)], device_ingest=True), w.chrom)
        packs[tag] = (dp.ref_code.clone(), dp.codes.clone(), dp.tile_pos0)
        assert bool(decode_calls) == (tag == "gz")
    assert torch.equal(packs["plain"][0], packs["gz"][0]) and torch.equal(packs["plain"][1], packs["gz"][1])
    t0 = packs["gz"][2]
    assert bool((packs["gz"][0][100 - t0:180 - t0] == 4).all())           # the exclusion slices stay where they are
    assert bool((packs["gz"][0][20_001 - t0:20_301 - t0] == 4).all())     # soft-masked bases are not scanned
    gsp.release_contig()
    device_bam.release()


def test_indel_caller_output_is_the_plain_twins(world_files, monkeypatch, decode_calls):
    import gzip
    from test_phase_gpu import _indels
    w, bam, fa, gz, d = world_files
    monkeypatch.delenv("NC_DEVICE_FASTA", raising=False)
    outs = {}
    for tag, path, ingest in (("plain", fa, "1"), ("gz", gz, "1"), ("gz_host", gz, "0")):
        monkeypatch.setenv("NC_DEVICE_INGEST", ingest)
        del decode_calls[:]
        files, lines = _indels(bam, path, w.chrom, w.length, os.path.join(d, "indel_" + tag), "indels")
        outs[tag] = (lines, gzip.open(files["indels"], "rb").read())
        assert bool(decode_calls) == (tag == "gz")
    print("indel records: %d" % len(outs["plain"][0]))
    assert outs["gz"] == outs["plain"] and outs["gz_host"] == outs["plain"]
    assert len(outs["plain"][0]) > 0


def test_phase_contig_with_realignment(world_files, monkeypatch, decode_calls):
    from nanocaller_amd import device_bam, generate_SNP_pileups as gsp
    from nanocaller_amd.phase import phase_contig
    w, bam, fa, gz, d = world_files
    monkeypatch.delenv("NC_DEVICE_INGEST", raising=False)
    monkeypatch.delenv("NC_DEVICE_FASTA", raising=False)
    snps = [ln for ln in _snp_worker_file(bam, fa, w, os.path.join(d, "snp_for_phase")).decode().splitlines(True)]
    del decode_calls[:]
    res = {}
    for tag, path in (("plain", fa), ("gz", gz)):
        gsp.release_contig()
        device_bam.release()
        res[tag] = phase_contig(bam, path, w.chrom, snps, 10, False, realign=True)
        assert bool(decode_calls) == (tag == "gz")
    assert res["gz"].records == res["plain"].records
    assert sum("|" in ln.split("\t")[9].split(":")[0] for ln in res["plain"].records) > 0
    for k in ("hash", "hp", "ps"):
        assert np.array_equal(res["gz"].haplotags[k], res["plain"].haplotags[k])
    gsp.release_contig()
    device_bam.release()

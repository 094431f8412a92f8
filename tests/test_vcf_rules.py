"""CPU-only: genotype rules + VCF text (snpCaller.py:113-198) against lines written by the REFERENCE's own
caller() on canned probabilities (tests/golden/caller_vcf.npz), plus hand-enumerated edge cases."""
import os

import numpy as np

from nanocaller_amd import bgzf, snpCaller
from tests.util import GOLD


def test_diploid_lines_match_reference_caller():
    z = np.load(os.path.join(GOLD, "caller_vcf.npz"))
    lines = snpCaller.snp_vcf_lines("chr20", z["pos"], z["ref"], z["probs"], z["dp"], z["freq"], z["fwd"], z["rev"])
    gold = str(z["vcf_diploid"]).splitlines(keepends=True)
    assert len(gold) == 400 and lines == gold
    kinds = {ln.split("\t")[9].split(":")[0] for ln in gold}
    assert kinds == {"0/1", "1/2", "1/1", "./."}
    assert {ln.split("\t")[6] for ln in gold} == {"PASS", "REF", "LOW"}


def test_haploid_lines_match_reference_caller():
    z = np.load(os.path.join(GOLD, "caller_vcf.npz"))
    lines = snpCaller.snp_vcf_lines_haploid("chr20", z["pos"], z["ref"], z["hap_probs"], z["dp"], z["freq"])
    gold = str(z["vcf_haploid"]).splitlines(keepends=True)
    assert len(lines) == len(gold) == 400 and {ln.split("\t")[6] for ln in gold} == {"PASS", "REF"}
    # The golden was produced under numpy 2.x, where `1e-10 + 1 - np.float32(p)` stays float32; the reference's
    # pinned numpy<2 evaluates it in float64, which is what this build implements.  With the -100x
    # haploid multiplier that is a last-digit difference in QUAL: every other field must match exactly.
    for a, b in zip(lines, gold):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:5] == fb[:5] and fa[6:] == fb[6:]
        assert abs(float(fa[5]) - float(fb[5])) <= 2e-3


def _one(probs, ref, fwd=(5, 6, 7, 8), rev=(1, 2, 3, 4), dp=40, freq=0.25):
    out = snpCaller.snp_vcf_lines("c", [123], [ref], np.array([probs], np.float32), [dp], [freq],
                                  np.array([fwd], np.float64), np.array([rev], np.float64))
    assert len(out) == 1
    return out[0].rstrip("\n").split("\t")


def test_branch_table_appendix_d():
    # k>=2, top is ref -> 0/1 with ALT = second, QUAL from the second's probability
    f = _one([0.9, 0.8, 0.1, 0.2], ref=0)
    assert f[3:7] == ["A", "G", "%.3f" % (-10 * np.log10(1e-10 + 1 - float(np.float32(0.8)))), "PASS"]
    assert f[9] == "0/1:40:0.2000:6,8:5,6:1,2" and f[7] == "PR=0.9000,0.2000,0.8000,0.1000;FQ=0.2500"
    # k>=2, second is ref -> 0/1 with ALT = top, QUAL from the REF base's probability (snpCaller.py:140)
    f = _one([0.7, 0.95, 0.1, 0.2], ref=0)
    assert f[4] == "G" and f[5] == "%.3f" % (-10 * np.log10(1e-10 + 1 - float(np.float32(0.7)))) and f[9].startswith("0/1:")
    # k>=2, neither is ref -> 1/2, three-valued AD/ADF/ADR
    f = _one([0.7, 0.95, 0.1, 0.2], ref=3)
    assert f[4] == "G,A" and f[9] == "1/2:40:0.2000,0.1500:12,8,6:8,6,5:4,2,1"
    # k==1, not ref -> 1/1 ; k==1, ref -> REF ./. ; k==0 -> LOW with QUAL 0.000
    assert _one([0.1, 0.2, 0.97, 0.3], ref=0)[9].startswith("1/1:40:0.2500:6,10")
    f = _one([0.1, 0.2, 0.97, 0.3], ref=2)
    assert f[4] == "." and f[6] == "REF" and f[9] == "./.:40:.:.:.:."
    f = _one([0.1, 0.2, 0.4, 0.3], ref=2)
    assert f[5] == "0.000" and f[6] == "LOW"


def test_qual_saturation_follows_float64_semantics():
    # p == 1.0f: 1e-10 + 1 - 1 = 1e-10 in float64 -> -10*log10 = 100 -> capped at 99 (numpy<2 semantics)
    assert _one([1.0, 1.0, 0.0, 0.0], ref=0)[5] == "99.000"
    p = np.float32(1.0) - np.float32(2.0 ** -24)          # largest float32 below 1
    q = min(99, -10 * np.log10(1e-10 + 1 - float(p)))
    assert _one([p, 0.0, 0.0, 0.0], ref=1)[5] == "%.3f" % q
    hap = snpCaller.snp_vcf_lines_haploid("c", [5], [0], np.array([[0.0, 1.0, 0.0, 0.0]], np.float32), [9], [0.5])
    assert hap[0].split("\t")[5] == "999.000" and hap[0].split("\t")[9].startswith("1/1:9:0.5000:.:.:.")


def test_bgzf_writer_is_valid_gzip(tmp_path):
    import gzip
    data = b"".join(b"line %d\n" % i for i in range(50_000))
    p = str(tmp_path / "x.vcf.gz")
    snpCaller.bgzf_write(p, data)
    assert gzip.open(p, "rb").read() == data
    raw = open(p, "rb").read()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and raw[12:14] == b"BC" and raw.endswith(bgzf.BGZF_EOF)


def test_native_formatter_matches_python_rules_and_reference():
    """nc_snp_vcf_format == snp_vcf_lines (== the reference's caller() output) on the goldens and on 20k random sites
    including saturated probabilities and ties."""
    z = np.load(os.path.join(GOLD, "caller_vcf.npz"))
    txt = snpCaller.snp_vcf_text("chr20", z["pos"], z["ref"], z["probs"], z["dp"], z["freq"], z["fwd"], z["rev"]).decode()
    assert txt == str(z["vcf_diploid"])
    rng = np.random.Generator(np.random.PCG64(17))
    n = 20_000
    probs = rng.random((n, 4)).astype(np.float32)
    probs[rng.random((n, 4)) < 0.15] = 1.0
    probs[rng.random((n, 4)) < 0.15] = 0.0
    probs[::13] = np.float32(1.0) - np.float32(2.0 ** -24)
    ref = rng.integers(0, 4, size=n)
    pos = np.arange(1000, 1000 + n)
    dp = rng.integers(4, 200, size=n)
    freq = rng.random(n)
    fwd = rng.integers(0, 90, size=(n, 4))
    rev = rng.integers(0, 90, size=(n, 4))
    assert snpCaller.snp_vcf_text("c", pos, ref, probs, dp, freq, fwd, rev).decode() == \
        "".join(snpCaller.snp_vcf_lines("c", pos, ref, probs, dp, freq, fwd.astype(np.float64), rev.astype(np.float64)))
    hp = rng.dirichlet(np.ones(4) * 0.2, size=n).astype(np.float32)
    hp[::7] = np.float32([0, 1, 0, 0])
    assert snpCaller.snp_vcf_text("c", pos, ref, hp, dp, freq, haploid=True).decode() == \
        "".join(snpCaller.snp_vcf_lines_haploid("c", pos, ref, hp, dp, freq))


def test_native_number_formatting_is_printf_exact():
    """The formatter's '%.4f' / '%.3f' / '%d' replacements equal Python's on exact decimal ties (k / 2^n), values a ulp
    either side of a tie, tiny and saturated probabilities, tiny negative QUALs ('-0.000') and large depths."""
    rng = np.random.Generator(np.random.PCG64(23))
    ties = np.array([k / 2.0 ** b for b in range(5, 20) for k in rng.integers(1, 2 ** b, size=40)], np.float64)
    ties = ties[ties < 1.0]
    near = np.concatenate([np.nextafter(ties, 0.0), np.nextafter(ties, 1.0)])
    dec = np.round(rng.random(4000), 4) + 0.00005                      # decimal half-way points, not exact in binary
    special = np.array([0.0, 1.0, 0.5, 0.25, 0.03125, 0.00005, 0.99995, 0.999949999, 1e-12, 1e-7, 4.9e-5, 5.1e-5, 0.00015, 0.00025])
    vals = np.concatenate([ties, near, dec[dec < 1], special])
    n = len(vals) - len(vals) % 4
    vals = vals[:n]
    # haploid records: probabilities (float32) in PR=, freq (float64) in FQ= and the sample column, QUAL = -100*log10(1e-10 + 1 - p)
    hp = vals.astype(np.float32).reshape(-1, 4)
    hp[0] = np.float32([1e-12, 0, 0, 0])                               # QUAL = -100*log10(1 + 1e-10 - 1e-12) < 0 -> '-0.000'
    hp[1] = np.float32([0, 0, 0, 0])
    m = len(hp)
    pos = np.arange(1, m + 1) * 3999
    ref = rng.integers(0, 4, size=m)
    dp = rng.integers(4, 70000, size=m)
    freq = vals[:m]
    assert snpCaller.snp_vcf_text("chrT", pos, ref, hp, dp, freq, haploid=True).decode() == \
        "".join(snpCaller.snp_vcf_lines_haploid("chrT", pos, ref, hp, dp, freq))
    # diploid records: allele fractions (a + b) / d with small integers give many exact ties
    probs = rng.random((m, 4)).astype(np.float32)
    probs[rng.random((m, 4)) < 0.3] = 1.0
    fwd = rng.integers(0, 40, size=(m, 4))
    rev = rng.integers(0, 40, size=(m, 4))
    dp2 = rng.choice([16, 32, 64, 128, 160, 100, 37], size=m)
    assert snpCaller.snp_vcf_text("chrT", pos, ref, probs, dp2, freq, fwd, rev).decode() == \
        "".join(snpCaller.snp_vcf_lines("chrT", pos, ref, probs, dp2, freq, fwd.astype(np.float64), rev.astype(np.float64)))

"""The model of the device DEFLATE writer (tests/deflate_model.py) and the crafted members (tests/deflate_cases.py), on the CPU: every
payload the model writes is a legal stream that zlib inflates to the member, every limited code is complete, and every crafted member
reaches the edge it was built for -- a member that misses its edge fails here, so the GPU test (tests/test_deflate_device_gpu.py) cannot
pass on inputs that have drifted away from the paths they are meant to drive."""
import zlib

import pytest

import deflate_cases as D
from deflate_model import BGZF_MAX, CL_ORDER, code_lengths, deflate_model, limit_counts, min_redundancy_counts

NAMES = sorted(D.cases())


def _kraft(lens, maxbits):
    return sum(1 << (maxbits - ln) for ln in lens if ln)


def _matches(info):
    return [(p, t) for p, t in info["tokens"] if isinstance(t, tuple)]


@pytest.mark.parametrize("name", NAMES)
def test_payload_inflates_and_codes_are_complete(name):
    data = D.cases()[name]
    pay, info = D.model(name)
    assert zlib.decompress(pay, -15) == data
    assert len(pay) <= len(data) + 5
    for key, maxbits in (("lens_ll", 15), ("lens_d", 15), ("lens_cl", 7)):
        lens = info[key]
        assert max(lens) <= maxbits, key
        assert _kraft(lens, maxbits) == 1 << maxbits, key
    assert info["stored"] == (pay[0] & 7 == 1) and info["stored"] == (info["dyn_bytes"] >= len(data) + 5)
    pos = 0                                                               # the tokens tile the member
    for p, t in info["tokens"]:
        assert p == pos
        if isinstance(t, tuple):
            ln, d = t
            assert 3 <= ln <= 258 and 1 <= d <= min(p, 32768) and all(data[p + i] == data[p + i - d] for i in range(ln))
            pos += ln
        else:
            assert t == data[p]
            pos += 1
    assert pos == len(data)


def test_empty_and_refused():
    assert deflate_model(b"")[0] == b"\x03\x00"
    assert zlib.decompress(b"\x03\x00", -15) == b""
    with pytest.raises(ValueError):
        deflate_model(bytes(BGZF_MAX + 1))


def test_one_repeated_byte_is_3483_bytes():
    """the size tests/test_bam_write.py records as measured on the GPU"""
    assert len(D.model("same")[0]) == 3483


def test_limiter_on_small_codes():
    """Fibonacci weights 1 1 2 3 5 8 13 give a chain of depth 6; limited to 4 bits the counts per length are moved up to a complete code"""
    counts = min_redundancy_counts([1, 1, 2, 3, 5, 8, 13])
    assert counts == {6: 2, 5: 1, 4: 1, 3: 1, 2: 1, 1: 1}
    num = limit_counts(counts, 4)
    assert num == [0, 1, 0, 2, 4] and sum(c << (4 - ln) for ln, c in enumerate(num) if ln) == 16
    assert limit_counts({3: 2, 2: 1, 1: 1}, 7) == [0, 1, 1, 2, 0, 0, 0, 0]               # within the limit: unchanged
    lens, deep = code_lengths([5, 0, 5, 5, 5], 15)                          # equal frequencies: ranked by index, complete at 2 bits
    assert lens == [2, 0, 2, 2, 2] and deep == 2


@pytest.mark.parametrize("name,depth", [("deep7", 16), ("deep9", 17)])
def test_deep_literal_tree(name, depth):
    info = D.model(name)[1]
    assert len(D.cases()[name]) == {"deep7": 23552, "deep9": 61440}[name]
    assert info["n_match"] == 0
    assert info["depth_ll"] >= depth                                       # the 15-bit limiter has work to do
    assert max(info["lens_ll"]) == 15
    assert info["hclen"] == 19                                             # length 15 is the last of the code-length order
    assert info["hdist"] == 2 and not info["stored"]


def test_deep_code_length_tree():
    data = D.cases()["cltree"]
    info = D.model("cltree")[1]
    assert len(data) == 1023 and info["n_match"] == 0
    assert info["lens_ll"][:177] == D.deep_code_length_tree()[1] and info["lens_ll"][256] == 10
    assert info["cl_hist"] == {1: 2, 3: 2, 5: 7, 6: 6, 7: 29, 8: 13, 9: 43, 10: 78, 18: 1}
    assert info["depth_cl"] >= 8                                           # the 7-bit limiter has work to do
    assert max(info["lens_cl"]) == 7 and not info["stored"]


def test_distance_limit():
    for at in (32767, 32768):
        info = D.model("dist%d" % at)[1]
        assert info["max_dist"] == at
        assert (at, (64, at)) in info["tokens"]
    info = D.model("dist32768")[1]
    assert info["lens_d"][29] > 0 and info["hdist"] == 30                   # distance code 29 with all 13 extra bits set
    info = D.model("dist32769")[1]
    assert info["max_dist"] < 32768 and info["n_match"] > 0
    assert all(not isinstance(t, tuple) for p, t in info["tokens"] if 32769 <= p < 32769 + 64)


def test_length_limit_and_member_end():
    data, info = D.cases()["len_end"], D.model("len_end")[1]
    assert (2048, (258, 2048)) in info["tokens"]
    p, t = info["tokens"][-1]
    assert info["end_clipped"] > 0 and t == (len(data) - p, 2048) and t[0] < 258     # ended by len - p, not by a mismatch
    data, info = D.cases()["len_half"], D.model("len_half")[1]
    at = 32768 - 128
    assert (at, (258, at)) in info["tokens"]                                # starts in the first half, ends in the second
    assert info["end_clipped"] > 0 and info["tokens"][-1][1][1] == at


def test_cuts_of_both_kinds():
    infos = [D.model("period%d" % p)[1] for p in D.PERIODS]
    assert all(i["cut_match"] > 0 for i in infos)
    assert sum(i["cut_lit"] for i in infos) >= 2                            # periods 3 and 5: one and two bytes left
    assert D.model("period3")[1]["cut_lit"] == 1 and D.model("period5")[1]["cut_lit"] == 1
    assert any(t[0] == 3 for _, t in _matches(D.model("period1")[1]))       # three bytes left: still a match
    assert all(i["max_len"] == 258 for i in infos)
    assert D.model("period1025")[1]["max_dist"] == 1025


def test_sizes():
    for n in D.SIZES:
        assert len(D.cases()["acgt%d" % n]) == n and len(D.cases()["rand%d" % n]) == n
        pay, info = D.model("rand%d" % n)
        assert info["stored"] and len(pay) == n + 5
    assert not D.model("acgt31")[1]["stored"] and D.model("acgt5")[1]["stored"]
    for n in (32767, 32768, 32769, 65279, 65280):
        info = D.model("acgt%d" % n)[1]
        assert not info["stored"] and info["cut_match"] > 0 and info["cut_lit"] > 0
    assert any(p >= 32768 for p, _ in _matches(D.model("acgt65280")[1]))    # matches in the second half too


def test_header_shapes():
    infos = [D.model(n)[1] for n in NAMES if not D.model(n)[1]["empty"]]
    hclen = {i["hclen"] for i in infos}
    assert 18 in hclen and 19 in hclen and min(hclen) < 18
    hdist = {i["hdist"] for i in infos}
    assert 2 in hdist and 30 in hdist
    ops = set().union(*(i["ops"] for i in infos if not i["stored"]))
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= ops
    assert CL_ORDER[18] == 15 and CL_ORDER[17] == 1


def test_stored_threshold():
    """The stored block is chosen when the dynamic block has >= len + 5 bytes.  Measured: of the first 4,000 draws of deflate_cases.draw
    (200..600 bytes of a 200-symbol alphabet with skewed weights) 55 end one byte under the threshold and 67 exactly on it; draw 9 (551
    bytes, dynamic 555: margin -1, the dynamic block is kept) and draw 12 (425 bytes, dynamic 430: margin 0, stored) are the first of
    each.  Uniform draws of the same sizes all end 12..35 bytes on the stored side."""
    data, (pay, info) = D.cases()["thr_dynamic"], D.model("thr_dynamic")
    assert info["dyn_bytes"] - (len(data) + 5) == -1 and not info["stored"] and len(pay) == len(data) + 4
    data, (pay, info) = D.cases()["thr_stored"], D.model("thr_stored")
    assert info["dyn_bytes"] - (len(data) + 5) == 0 and info["stored"] and len(pay) == len(data) + 5


def test_long_launch_members_would_show_stale_code_lengths():
    """In the launch with more members than workgroups a workgroup writes `small40` behind `deep7` and `acgt65280` behind `small40`.  All three
    are dynamic blocks, and each predecessor gives lengths to symbols its successor does not use: lengths left over from the member before
    would change the successor's header, so the byte-for-byte comparison sees them."""
    used = {}
    for name in ("deep7", "small40", "acgt65280"):
        info = D.model(name)[1]
        assert not info["stored"]
        used[name] = {s for s, ln in enumerate(info["lens_ll"]) if ln}
    assert used["deep7"] - used["small40"] and used["small40"] - used["acgt65280"]
    assert D.model("small7")[1]["stored"] and D.model("rand1500")[1]["stored"]      # the stored path behind a dynamic member, too

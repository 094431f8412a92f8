"""The crafted DEFLATE streams of tests/deflate_craft.py proven on zlib alone (CPU): every legal one inflates to the bytes its tokens stand for and
really contains what it is named for -- asserted from its code lengths and tokens --, every illegal one is refused (or, where only the announced
length is wrong, comes out at another length).  tests/test_inflate_device.py then holds the device inflate to the same streams; this file plays for
them the part tests/test_cnn_probe_ref.py plays for the CNN probes."""
import zlib

import pytest

import deflate_craft as C

LAUNCHES = list(C.N_LEGAL)


def _used(case):
    """the code lengths of the symbols the stream really uses: (literal / length, distance), the end of block included"""
    ul, ud = [], []
    for b in case.blocks:
        if b["kind"] == 0:
            continue
        ul.append(b["ll"][256])
        for t in b["tokens"]:
            if type(t) is int:
                ul.append(b["ll"][t])
            else:
                ul.append(b["ll"][C.len_sym(t[0], b["as284"])[0]])
                ud.append(b["dl"][C.dist_sym(t[1])[0]])
    return ul, ud


def _matches(case):
    """(bytes before, length, distance, token index) of every match"""
    out, op = [], 0
    for i, t in enumerate(case.tokens):
        if type(t) is int:
            op += 1
        else:
            out.append((op, t[0], t[1], i))
            op += t[0]
    return out


def _device_tokens(case):
    """how many tokens the stream takes in a decoder that takes a literal's successor with it when that is a literal of at most 8 bits"""
    n = 0
    for b in case.blocks:
        tok, i = b["tokens"], 0
        while i < len(tok):
            pair = b["kind"] and type(tok[i]) is int and i + 1 < len(tok) and type(tok[i + 1]) is int and b["ll"][tok[i + 1]] <= 8
            i += 2 if pair else 1
            n += 1
    return n


def _check_claims(c):
    k = c.claims
    ul, ud = _used(c)
    m = _matches(c)
    if "max_used" in k:
        assert (max(ul), max(ud)) == k["max_used"], c.name
    if "len_syms" in k:
        b = c.blocks[0]
        assert len({C.len_sym(t[0])[0] for t in b["tokens"] if type(t) is not int}) == k["len_syms"], c.name
        ds = {C.dist_sym(t[1]) for t in b["tokens"] if type(t) is not int}
        assert len({s for s, _, _ in ds}) == k["dist_syms"], c.name
        for s in {s for s, _, _ in ds}:                                          # every distance symbol with its least and its most extra bits
            assert {(s, C.DEXT[s], 0), (s, C.DEXT[s], (1 << C.DEXT[s]) - 1)} <= ds, (c.name, s)
        assert sum(type(t) is not int for t in b["tokens"]) >= 2000 and sum(type(t) is int for t in b["tokens"]) >= 40_000
        assert {n for n in b["ll"] if n} == set(range(2, 16)) and b["ll"][256] == 15 and sum(n == 9 for n in b["ll"]) >= 256
        assert sorted(n for n in b["dl"] if n) == list(range(1, 15)) + [15, 15] and b["dl"][28] == b["dl"][29] == 15
        assert any(n <= 8 for n in b["ll"][257:] if n) and any(n > 8 for n in b["ll"][257:])
    if "run48" in k:
        b = c.blocks[0]
        bits = [C.token_bits(t, b["ll"], b["dl"]) for t in b["tokens"]]
        best = run = 0
        for v in bits:
            run = run + 1 if v == 48 else 0
            best = max(best, run)
        assert best >= 64 and best >= k["run48"], (c.name, best)
        assert sum(227 <= n <= 257 and 24_577 <= d <= 32_768 for _, n, d, _ in m) >= 120
        assert sum(type(t) is int for t in b["tokens"]) == 32_768
        assert b["ll"][283] == b["ll"][284] == b["dl"][28] == b["dl"][29] == 15
    if "lit_then_long" in k:
        b = c.blocks[0]
        t = b["tokens"]
        assert any(type(t[i]) is int and type(t[i + 1]) is int and b["ll"][t[i + 1]] > 8 for i in range(len(t) - 1)), c.name
    for f in ("nlen", "ndist", "ncl"):
        if f in k:
            assert c.blocks[0][f] == k[f], (c.name, f)
    if "one_dist" in k:
        dl = c.blocks[0]["dl"]
        assert [i for i, n in enumerate(dl) if n] == [k["one_dist"]] and dl[k["one_dist"]] == 1 and ud and set(ud) == {1}, c.name
    if "ops" in k:
        assert set(k["ops"]) <= set(c.blocks[-1]["ops"]), c.name
    if "run16_crosses" in k:
        b = c.blocks[0]
        seq, starts = C.ops_lengths(b["ops"])
        assert seq == b["ll"][:b["nlen"]] + b["dl"][:b["ndist"]]
        assert any(s == 16 and at < b["nlen"] < at + 3 + x for (s, x), at in zip(b["ops"], starts)), c.name
    if "shrinks" in k:
        a, b = c.blocks
        assert b["nlen"] < a["nlen"] and b["ndist"] < a["ndist"] and any(a["ll"][b["nlen"]:]) and any(a["dl"][b["ndist"]:])
    if "lengths" in k:
        lo, hi, least = k["lengths"]
        assert {n for _, n, d, _ in m if (d == 1 if least == 1 else d >= least)} == set(range(lo, hi + 1)), c.name
    if "as284" in k:
        b = c.blocks[0]
        assert b["as284"] and (b["ll"][285] != 0) == k["has285"] and any(n == 258 for _, n, _, _ in m), c.name
    if "dists" in k:
        want = {v for s in range(30) for v in (C.DB[s] - 1, C.DB[s], C.DB[s] + (1 << C.DEXT[s]) - 1) if v}
        assert want == set(k["dists"]) <= {d for _, _, d, _ in m} and 32_768 in want and len(want) == 56, c.name
    if "dist_eq_op" in k:
        assert any(op == d == k["dist_eq_op"] for op, _, d, _ in m), c.name
    if "chained" in k:
        n = sum(a[3] + 1 == b[3] and b[3] % 64 and b[0] - b[2] >= a[0] for a, b in zip(m, m[1:]))      # the source lies in the match before it, same step
        assert n >= 10, c.name
    if "bitoff" in k:
        assert [b["bitoff"] for b in c.blocks if b["kind"] == 0] == [k["bitoff"]], c.name
    if "size" in k:
        assert len(c.want) == k["size"], c.name
    if "ntok" in k:
        assert _device_tokens(c) == k["ntok"], c.name
    if "unpaired" in k:
        assert all(type(t) is int for t in c.tokens) and min(ul[1:]) > 8, c.name
    if "alternating" in k:
        assert all((type(a) is int) != (type(b) is int) for a, b in zip(c.tokens, c.tokens[1:])), c.name
    if "kinds" in k:
        assert {b["kind"] for b in c.blocks} == k["kinds"], c.name
    if "rle" in k:
        assert any(s >= 16 for s, _ in c.blocks[0]["ops"]) == k["rle"] or not c.want, c.name


@pytest.mark.parametrize("launch", LAUNCHES)
def test_every_crafted_legal_stream_is_zlibs_too(launch):
    cases = C.legal_launches()[launch]
    assert len(cases) == C.N_LEGAL[launch]
    for c in cases:
        assert zlib.decompress(c.z, -15) == c.want, c.name
        assert c.want == C.expand(c.tokens) and len(c.want) <= 65_536
        _check_claims(c)


def test_the_case_lists_are_whole():
    g = C.legal_launches()
    assert {k: len(v) for k, v in g.items()} == C.N_LEGAL and sum(C.N_LEGAL.values()) == 810
    names = [c.name for k, v in g.items() if not k.startswith("worst_rate_among") for c in v]
    assert len(set(names)) == len(names)
    claimed = {key for v in g.values() for c in v for key in c.claims}
    assert claimed >= {"max_used", "run48", "lit_then_long", "dist_eq_op", "ntok", "run16_crosses", "as284", "bitoff", "one_dist", "shrinks", "chained"}
    # every bit offset a stored block can be entered at; all 30 single distance codes; both 15-bit distance symbols' full range
    assert {c.claims["bitoff"] for c in g["stored"] if "bitoff" in c.claims} == set(range(8))
    assert sorted(c.claims["one_dist"] for c in g["headers"] if "one_dist" in c.claims) == list(range(30))
    assert {c.claims["dist_eq_op"] for c in g["lengths_distances"] if "dist_eq_op" in c.claims} == {1, 2, 4097, 16_384, 16_385, 32_768}
    rnd = g["random_codes"]
    assert sum(c.claims["rle"] for c in rnd) == 128 and max(len(c.want) for c in rnd) <= 8192
    assert max(max(b["ll"]) for c in rnd for b in c.blocks) == 15 and max(max(b["dl"]) for c in rnd for b in c.blocks) >= 9
    assert all(C.kraft(b["ll"]) == 32768 and b["ll"][256] for c in rnd for b in c.blocks)
    # the member map: distinct contents, counts off the 16 / 128 boundaries
    for k in ("map_300", "map_129", "map_17"):
        assert len({c.want for c in g[k]}) == len(g[k]) and len(g[k]) % 16 and len(g[k]) % 128
    assert len(g["worst_rate_among_short"]) == 16 and max(len(c.z) for c in g["worst_rate_among_short"] if c.name != "worst_rate") < 100


def test_every_crafted_illegal_stream_is_refused_by_zlib():
    ill = C.illegal_cases()
    assert len(ill) == C.N_ILLEGAL == 30
    assert sorted({st for _, _, _, st in ill}) == [1, 2, 3, 4, 5, 6]
    assert all(0 <= n <= 65_536 for _, _, n, _ in ill)
    for name, z, n, st in ill:
        if st in (4, 6):                                                         # a sound stream of another length than the one announced
            assert len(zlib.decompress(z, -15)) != n, name
            assert (len(zlib.decompress(z, -15)) > n) == (st == 4), name
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(z, -15)
            if st == 5:                                                          # cut short, not damaged: zlib runs out of input (Z_BUF_ERROR)
                with pytest.raises(zlib.error, match="incomplete or truncated"):
                    zlib.decompress(z, -15)


def test_the_writer_refuses_what_it_cannot_write():
    d = C.Deflate()
    with pytest.raises(C.CraftError):                                            # 258 needs symbol 285 -- or 284 + 31 on request -- and neither silently
        d.dynamic([65, (258, 1)], C.flat_lengths([65, 256, 284], 286), [1], final=True)
    with pytest.raises(C.CraftError):
        C.Deflate().dynamic([66], C.flat_lengths([65, 256], 286), [0], final=True)
    with pytest.raises(C.CraftError):
        C.Deflate().dynamic([65, (3, 2)], C.flat_lengths([65, 256, 257], 286), [1], final=True)
    with pytest.raises(C.CraftError):
        C.Deflate().dynamic([65], C.flat_lengths([65, 66], 286), [0], final=True)                  # no end-of-block code
    with pytest.raises(C.CraftError):
        C.expand([65, (3, 2)])
    z = C.Deflate().dynamic([65, (258, 1)], C.flat_lengths([65, 256, 284], 286), [1], final=True, as284=True).getvalue()
    assert zlib.decompress(z, -15) == b"A" * 259


def test_random_codes_are_complete_and_capped():
    import random
    rng = random.Random(1)
    deepest = 0
    for n in (2, 3, 17, 30, 100, 286):
        for _ in range(50):
            lens = C.random_code(rng, rng.sample(range(286), n), 286)
            assert C.kraft(lens) == 32768 and max(lens) <= 15 and sum(v > 0 for v in lens) == n
            deepest = max(deepest, max(lens))
    assert deepest == 15
    assert C.random_code(rng, [7], 30) == [0] * 7 + [1] + [0] * 22 and C.random_code(rng, [], 30) == [0] * 30

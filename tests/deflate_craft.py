"""A bit-level DEFLATE writer (RFC 1951) for tests, and the crafted streams of tests/test_deflate_craft_ref.py and tests/test_inflate_device.py.

zlib's compressor writes a narrow corner of the format; this writer writes the rest of it on purpose: code lengths chosen by the caller up to 15
bits in both alphabets, any code length code, run-length coded lengths or plain ones, length 258 as symbol 284 + 31 extra, stored blocks at any bit
offset, and -- through the raw header -- streams that are not DEFLATE at all.  It imports nothing of the code under test: the arbiter of every
stream made here is zlib's decompressor (tests/test_deflate_craft_ref.py), the device inflate is then held to the same bytes.

A token is an int (a literal byte) or a tuple (length, distance)."""
import bisect
import functools
import random

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DB = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                      # (288 symbols: 286 and 287 have codes and must not occur)
FIXED_D = [5] * 30


class CraftError(ValueError):
    pass


def len_sym(length, as284=False):
    """(symbol, extra bits, extra value) of a match length"""
    if not 3 <= length <= 258:
        raise CraftError("length %d" % length)
    if length == 258:
        return (284, 5, 31) if as284 else (285, 0, 0)
    i = bisect.bisect_right(LBASE, length, 0, 28) - 1
    return 257 + i, LEXT[i], length - LBASE[i]


def dist_sym(dist):
    if not 1 <= dist <= 32768:
        raise CraftError("distance %d" % dist)
    i = bisect.bisect_right(DB, dist) - 1
    return i, DEXT[i], dist - DB[i]


def expand(tokens):
    """the bytes a token list stands for"""
    out = bytearray()
    for t in tokens:
        if type(t) is int:
            out.append(t)
            continue
        n, d = t
        if d > len(out) or d < 1:
            raise CraftError("distance %d at %d" % (d, len(out)))
        if d >= n:
            s = len(out) - d
            out += out[s:s + n]
        else:
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 for a complete code"""
    return sum(1 << (15 - n) for n in lens if n)


def canon(lens):
    """canonical codes (RFC 1951 3.2.2) as (code with its first bit lowest, length) per symbol; an over-subscribed set still gets bits"""
    cnt = [0] * 17
    for n in lens:
        cnt[n] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + cnt[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lens:
        if not n:
            out.append((0, 0))
            continue
        c = nxt[n] & ((1 << n) - 1)
        nxt[n] += 1
        out.append((int(format(c, "0%db" % n)[::-1], 2), n))
    return out


def flat_lengths(symbols, total):
    """a complete code over `symbols` with lengths as equal as they get (one symbol: length 1, the legal incomplete form)"""
    lens, n = [0] * total, len(symbols)
    if n == 1:
        lens[symbols[0]] = 1
    elif n > 1:
        k = (n - 1).bit_length()
        short = (1 << k) - n
        for i, s in enumerate(symbols):
            lens[s] = k - 1 if i < short else k
    return lens


def random_code(rng, symbols, total, depth=15):
    """a random complete code over `symbols`: the Kraft budget is split leaf by leaf, no leaf below `depth`; never rejects"""
    n = len(symbols)
    if n < 2:
        return flat_lengths(symbols, total)
    leaves = [0]
    while len(leaves) < n:
        i = len(leaves) - 1 if rng.random() < 0.3 else rng.randrange(len(leaves))      # (the newest leaf, often: chains to the depth cap)
        if leaves[i] >= depth:
            i = leaves.index(min(leaves))                                             # (n <= 288 < 2^15: a leaf above the cap always exists)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    lens = [0] * total
    for s, d in zip(symbols, leaves):
        lens[s] = d
    assert kraft(lens) == 32768 and max(lens) <= depth
    return lens


def rle_ops(seq):
    """the lengths as code length symbols, greedily run-length coded: (symbol, extra value) with 16 = previous x 3-6, 17 = zero x 3-10, 18 = zero x 11-138"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r - 11))
                run -= r
            if run >= 3:
                ops.append((17, run - 3))
                run = 0
        else:
            ops.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r - 3))
                run -= r
        ops += [(v, 0)] * run
        i = j
    return ops


def ops_lengths(ops):
    """what a list of code length symbols decodes to, and where every op starts"""
    seq, starts = [], []
    for s, x in ops:
        starts.append(len(seq))
        if s < 16:
            seq.append(s)
        elif s == 16:
            seq += [seq[-1]] * (3 + x)
        else:
            seq += [0] * ((3 if s == 17 else 11) + x)
    return seq, starts


def token_bits(t, ll, dl, as284=False):
    if type(t) is int:
        return ll[t]
    s, e, _ = len_sym(t[0], as284)
    ds, de, _ = dist_sym(t[1])
    return ll[s] + e + dl[ds] + de


class Deflate:
    """one raw deflate stream, block by block.  `tokens` collects what the stream stands for, `blocks` what every block was made of"""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0
        self.tokens, self.blocks = [], []

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")

    def stored(self, data, final=False, len_field=None, nlen_field=None):
        self.bits(int(final), 1)
        self.bits(0, 2)
        off = self.bitpos & 7
        self.bits(0, -self.bitpos & 7)
        n = len(data) if len_field is None else len_field
        self.bits(n, 16)
        self.bits(n ^ 0xffff if nlen_field is None else nlen_field, 16)
        self.buf += data
        self.tokens += list(data)
        self.blocks.append(dict(kind=0, bitoff=off, tokens=list(data)))
        return self

    def symbols(self, tokens, ll, dl, as284=False, eob=True):
        """the tokens in the codes of ll / dl; a symbol without a code raises"""
        lc, dc = canon(ll), canon(dl)
        buf, acc, nb = self.buf, self.acc, self.n
        for t in tokens:
            if type(t) is int:
                c, n = lc[t]
                if not n:
                    raise CraftError("literal %d has no code" % t)
            else:
                s, e, x = len_sym(t[0], as284)
                c, n = lc[s] if s < len(lc) else (0, 0)
                ds, de, dx = dist_sym(t[1])
                dcode, dn = dc[ds] if ds < len(dc) else (0, 0)
                if not n or not dn:
                    raise CraftError("match %r: symbol %d / distance symbol %d without a code" % (t, s, ds))
                c |= x << n
                n += e
                c |= dcode << n
                n += dn
                c |= dx << n
                n += de
            acc |= c << nb
            nb += n
            while nb >= 8:
                buf.append(acc & 255)
                acc >>= 8
                nb -= 8
        self.acc, self.n = acc, nb
        if eob:
            c, n = lc[256]
            if not n:
                raise CraftError("no end-of-block code")
            self.bits(c, n)
        self.tokens += tokens
        return self

    def fixed(self, tokens, final=False, as284=False, eob=True):
        self.bits(int(final), 1)
        self.bits(1, 2)
        self.symbols(tokens, FIXED_LL, FIXED_D, as284, eob)
        self.blocks.append(dict(kind=1, ll=FIXED_LL, dl=FIXED_D, tokens=list(tokens), as284=as284))
        return self

    def raw_header(self, hlit, hdist, hclen, cl3, ops):
        """the escape hatch: the three count FIELDS as given, the code length code's lengths in transmission order, then code length symbols
        (symbol, extra value) in that code -- or ("raw", value, bits)"""
        self.bits(hlit, 5)
        self.bits(hdist, 5)
        self.bits(hclen, 4)
        cl = [0] * 19
        for i, v in enumerate(cl3):
            self.bits(v, 3)
            cl[CL_ORDER[i]] = v
        cc = canon(cl)
        for op in ops:
            if op[0] == "raw":
                self.bits(op[1], op[2])
                continue
            c, n = cc[op[0]]
            if not n:
                raise CraftError("code length symbol %d has no code" % op[0])
            self.bits(c, n)
            if op[0] >= 16:
                self.bits(op[1], (2, 3, 7)[op[0] - 16])
        return self

    def dynamic(self, tokens, ll, dl, final=False, cl=None, rle=False, as284=False, hclen=None, nlen=None, ndist=None, eob=True):
        """a dynamic block in the codes ll / dl (lengths per symbol); cl = the code length code's 19 lengths (default: a flat complete code over
        the symbols the header uses), hclen / nlen / ndist = counts larger than the lengths need"""
        ll, dl = list(ll) + [0] * (286 - len(ll)), list(dl) + [0] * (30 - len(dl))
        need_l = max([257] + [i + 1 for i, v in enumerate(ll) if v])
        need_d = max([1] + [i + 1 for i, v in enumerate(dl) if v])
        nlen, ndist = nlen or need_l, ndist or need_d
        if nlen < need_l or ndist < need_d:
            raise CraftError("counts cut the codes")
        seq = ll[:nlen] + dl[:ndist]
        ops = rle_ops(seq) if rle else [(v, 0) for v in seq]
        if cl is None:
            used = sorted({s for s, _ in ops})
            if len(used) < 2:
                used = sorted(set(used) | {0, 8})                              # (zlib refuses an incomplete code length code)
            cl = flat_lengths(used, 19)
        ncl = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
        if hclen is not None:
            if hclen < ncl:
                raise CraftError("HCLEN cuts the code length code")
            ncl = hclen
        self.bits(int(final), 1)
        self.bits(2, 2)
        self.raw_header(nlen - 257, ndist - 1, ncl - 4, [cl[s] for s in CL_ORDER[:ncl]], ops)
        self.symbols(tokens, ll, dl, as284, eob)
        self.blocks.append(dict(kind=2, ll=ll, dl=dl, tokens=list(tokens), as284=as284, ops=ops, nlen=nlen, ndist=ndist, ncl=ncl, cl=cl))
        return self


class Case:
    def __init__(self, name, d, claims=None):
        self.name, self.z, self.tokens, self.blocks = name, d.getvalue(), d.tokens, d.blocks
        self.want = expand(d.tokens)
        self.claims = claims or {}
        assert len(self.want) <= 65536, name


# ---- the legal streams ------------------------------------------------------------------------------------------------------------------
def _chain(syms, first=1):
    """lengths first, first + 1, ..., the last two equal: sums to 2^-(first - 1)"""
    ll = {}
    for i, s in enumerate(syms):
        ll[s] = min(first + i, first + len(syms) - 2)
    return ll


def _lens(total, *parts):
    out = [0] * total
    for p in parts:
        for s, n in p.items():
            assert out[s] == 0
            out[s] = n
    return out


def _lits(rng, n, alphabet):
    return [alphabet[rng.randrange(len(alphabet))] for _ in range(n)]


def _deep(name, dsyms):
    """the literal / length code chained to 15 bits (end of block and symbol 268 at 15, length symbols 257-261 inside the 8-bit table, 262-268
    outside it), the other half of the budget at 9 bits; the distance code 1 .. 14, 15, 15 over 14 symbols + 28 and 29"""
    rng = random.Random(name)
    nine = [s for s in range(241) if s not in (101, 116)] + list(range(269, 286))
    ll = _lens(286, _chain([101, 116] + list(range(257, 269)) + [256], 2), {s: 9 for s in nine})
    ll[256], ll[268] = 15, 15
    dl = _lens(30, _chain(dsyms + [28, 29]))
    assert kraft(ll) == 32768 and kraft(dl) == 32768 and ll[267] == 14 and dl[28] == dl[29] == 15
    alphabet = [s for s in range(256) if ll[s]]
    tok = _lits(rng, 40_000, alphabet)
    lenopts = [v for i in range(29) for v in {LBASE[i], LBASE[i] + (1 << LEXT[i]) - 1 - (i == 27)}]
    distopts = [v for s in dsyms + [28, 29] for v in {DB[s], DB[s] + (1 << DEXT[s]) - 1}]
    size, k = 40_000, 0
    for j, n in enumerate(sorted(lenopts)):
        for d in (distopts[j % len(distopts)], distopts[(j + 7) % len(distopts)]):
            tok.append((n, d))
            size += n
    while size < 65_536 - 12 and k < 4000:
        tok.append((3 + k % 8, distopts[k % len(distopts)]))
        size += 3 + k % 8
        if k % 5 == 0:
            tok.append(alphabet[k % len(alphabet)])
            size += 1
        k += 1
    return Case(name, Deflate().dynamic(tok, ll, dl, final=True), dict(max_used=(15, 15), len_syms=29, dist_syms=len(dsyms) + 2))


def _worst():
    """every match 48 bits: symbols 283 / 284 and 28 / 29 at 15 bits, 5 and 13 extra bits"""
    rng = random.Random(48)
    ll = _lens(286, _chain(list(range(257, 269)) + [256, 283, 284], 2), {s: 9 for s in range(256)})
    dl = _lens(30, _chain(list(range(14)) + [28, 29]))
    assert kraft(ll) == 32768 and ll[283] == ll[284] == 15 and dl[28] == dl[29] == 15
    tok = _lits(rng, 32_768, list(range(256)))
    for i in range(124):
        tok.append((227 + i * 7 % 31, 32_768 if i % 9 == 0 else 24_577 + i * 1237 % 8192))
    return Case("worst_rate", Deflate().dynamic(tok, ll, dl, final=True), dict(run48=120, max_used=(15, 15)))


def small_member(i, kind=None):
    """a short member whose bytes name it"""
    text = list(b"member %05d:" % i) + [i * 7 % 251, i % 256, (i >> 8) % 256] + [(5, 8), (3 + i % 9, 1 + i % 11)]
    d = Deflate()
    kind = i % 3 if kind is None else kind
    if kind == 0:
        d.stored(expand(text), final=True)
    elif kind == 1:
        d.fixed(text, final=True)
    else:
        lits = sorted({t for t in text if type(t) is int})
        ll = flat_lengths(lits + [256] + sorted({len_sym(t[0])[0] for t in text if type(t) is not int}), 286)
        d.dynamic(text, ll, flat_lengths(sorted({dist_sym(t[1])[0] for t in text if type(t) is not int}), 30), final=True, rle=bool(i & 1))
    return Case("small%d" % i, d)


# the literal / length code of the two-literal edges: 65 .. 70 at 1 .. 8 bits (with 257 and the end of block among them), 71 .. 78 at 9 .. 15
_TWO_LL = _lens(286, _chain([65, 66, 257, 67, 256, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78]))
_TWO_DL = [1]


def _two_cases():
    out = []

    def dyn(name, tok, **claims):
        out.append(Case("two_dyn_" + name, Deflate().dynamic(tok, _TWO_LL, _TWO_DL, final=True), claims))

    def fix(name, tok, **claims):
        out.append(Case("two_fix_" + name, Deflate().fixed(tok, final=True), claims))

    for mk, a, b, longs in ((dyn, 65, 66, list(range(71, 79))), (fix, 65, 66, [144, 200, 255])):
        mk("pair_last", [a, b] * 3)                                             # the last byte is the second literal of a pair: op + 2 == isize
        mk("pair_then_one", [a, b] * 3 + [a])                                   # odd size: a single literal behind a pair
        mk("lit_eob", [a])                                                      # a literal, then the end of block
        mk("lit_len", [a, (3, 1), b, (3, 1), a, a, (3, 1)])                     # a literal, then a length symbol
        mk("lit_long", [t for s in longs for t in (a, s)] + [a], lit_then_long=True)      # a literal, then a literal the table misses
        mk("long_lit", [t for s in longs for t in (s, a, b)], lit_then_long=True)         # the first through the walk, the second paired with nothing / the next
        mk("long_long", longs + longs[::-1], lit_then_long=True)
    return out


def _header_cases():
    rng = random.Random(12)
    out = []
    lits = list(range(32, 127))
    text = _lits(rng, 600, lits)
    # HLIT = 257: the end of block the only symbol that is no literal; one distance length, 0
    out.append(Case("hlit257_ndist1_len0", Deflate().dynamic(text, flat_lengths(lits + [256], 286), [0], final=True), dict(nlen=257, ndist=1)))
    ll285 = flat_lengths(lits + [256, 257, 270, 285], 286)
    out.append(Case("nlen286", Deflate().dynamic(text + [(258, 4), (3, 600), (24, 1)], ll285, flat_lengths([0, 3, 18], 30), final=True), dict(nlen=286)))
    # one distance code of length 1, every symbol in turn (ndist = symbol + 1)
    for s in range(30):
        hi = DB[s] + (1 << DEXT[s]) - 1
        tok = _lits(rng, hi, lits) + [(3, DB[s]), 65, (258, hi), (24, DB[s])]
        out.append(Case("one_dist_%d" % s, Deflate().dynamic(tok, ll285, flat_lengths([s], 30), final=True, rle=bool(s & 1)), dict(ndist=s + 1, one_dist=s)))
    dl30 = flat_lengths(list(range(30)), 30)
    far = _lits(rng, 33_000, lits)
    out.append(Case("ndist30", Deflate().dynamic(far + [((3, 24, 258)[s % 3], DB[s] + (1 << DEXT[s]) - 1) for s in range(30)], ll285, dl30, final=True, rle=True), dict(ndist=30)))
    # HCLEN: five lengths (16 17 18 0 8) is the least a legal block can have -- with four no length is non-zero, so no end of block; eight is
    # the field value 4; nineteen
    ll8 = _lens(286, {s: 8 for s in list(range(255)) + [256]})
    cl = [0] * 19
    cl[0] = cl[8] = 1
    out.append(Case("hclen5", Deflate().dynamic(_lits(rng, 300, list(range(255))), ll8, [0], final=True, cl=cl), dict(ncl=5)))
    ll9 = _lens(286, {s: 8 for s in range(200)}, {s: 9 for s in range(200, 232)}, {256: 7, 257: 7}, {s: 6 for s in range(258, 267)})
    assert kraft(ll9) == 32768
    cl = flat_lengths([0, 6, 7, 8, 9, 16, 17, 18], 19)
    out.append(Case("hclen8", Deflate().dynamic(_lits(rng, 300, list(range(232))), ll9, [0], final=True, cl=cl, rle=True), dict(ncl=8)))
    out.append(Case("hclen19", Deflate().dynamic(text + [(258, 5)], ll285, [0, 0, 0, 0, 1], final=True, cl=flat_lengths(list(range(19)), 19), rle=True), dict(ncl=19)))
    # the run-length symbols at their longest: 16 x 6, 17 x 10, 18 x 138, and a 16-run from the literal lengths into the distance lengths
    seven = list(range(7)) + list(range(17, 118)) + list(range(256, 274))
    llr = _lens(286, {s: 7 for s in seven}, {s: 8 for s in range(274, 278)})
    dlr = [8, 8, 7, 6, 5, 4, 3, 2, 1]
    assert kraft(llr) == 32768 and kraft(dlr) == 32768
    tok = _lits(rng, 700, [s for s in seven if s < 256]) + [(n, d) for n in (3, 12, 20, 43, 82) for d in (1, 2, 3, 4, 5, 7, 9, 13, 17)]
    out.append(Case("rle_longest_runs", Deflate().dynamic(tok, llr, dlr, final=True, rle=True), dict(ops=[(16, 3), (17, 7), (18, 127)], run16_crosses=True)))
    # zeros over 257 .. 285 with nlen = 286
    out.append(Case("zeros_257_285", Deflate().dynamic(text, flat_lengths(lits + [256], 286), [1], final=True, rle=True, nlen=286), dict(nlen=286, ops=[(18, 18)])))
    # two dynamic blocks, the second with fewer of both kinds of lengths: what the first left in the tables must be gone
    d = Deflate().dynamic(text + [(258, 5), (3, 600), (24, 9)], ll285, dl30, rle=True)
    d.dynamic(_lits(rng, 300, [65, 66, 67]) + [(3, 1), 65, (3, 2)], flat_lengths([65, 66, 67, 256, 257], 286), [1, 1], final=True)
    out.append(Case("two_blocks_shrinking", d, dict(shrinks=True)))
    return out


def _length_distance_cases():
    rng = random.Random(5)
    out = []
    tok = [7]
    for n in range(3, 259):
        tok += [n & 255, (n, 1)]
    out.append(Case("every_length_dist1", Deflate().fixed(tok, final=True), dict(lengths=(3, 258, 1))))
    tok = _lits(rng, 300, list(range(256)))
    for n in range(3, 259):
        tok += [(n, 259 + n % 37), n & 255]
    out.append(Case("every_length_far", Deflate().fixed(tok, final=True), dict(lengths=(3, 258, 259))))
    tok = _lits(rng, 300, list(range(256))) + [t for d in (2, 3, 5, 63, 64, 65, 129, 257) for t in ((258, d), d & 255, (100, d))]
    out.append(Case("overlapping", Deflate().fixed(tok, final=True)))
    tok = _lits(rng, 10, list(range(256))) + [(258, 3), 1, (258, 200)]
    out.append(Case("len258_as_284_31_with_285", Deflate().fixed(tok, final=True, as284=True), dict(as284=True, has285=True)))
    ll = flat_lengths(sorted(set(tok[:10]) | {1, 256, 284}), 286)
    out.append(Case("len258_as_284_31_without_285", Deflate().dynamic(tok, ll, flat_lengths([2, 15], 30), final=True, as284=True), dict(as284=True, has285=False)))
    ds = sorted({v for k in range(30) for v in (DB[k] - 1, DB[k], DB[k] + (1 << DEXT[k]) - 1) if v})
    tok = _lits(rng, 32_768, list(range(256))) + [t for d in ds for t in ((3, d), d & 255)]
    out.append(Case("distance_boundaries", Deflate().fixed(tok, final=True), dict(dists=ds)))
    for op in (1, 2, 4097, 16_384, 16_385, 32_768):
        tok = _lits(rng, op, list(range(256))) + [(10, op), 9, (70, op)]
        out.append(Case("dist_eq_op_%d" % op, Deflate().fixed(tok, final=True), dict(dist_eq_op=op)))
    tok = list(b"abcdefgh") + [(8, 8), (8, 8), (16, 16), (5, 3), (40, 37), (40, 40), (100, 7), (3, 100), (33, 1), (64, 64), (65, 64), (258, 258), (3, 3)] * 3
    out.append(Case("chained", Deflate().fixed(tok, final=True), dict(chained=True)))
    return out


def _stored_cases():
    rng = random.Random(9)
    out = []
    blob = bytes(rng.randrange(256) for _ in range(65_536))
    for k in range(9):                                                          # 9-bit literals: the stored header starts at bit (2 + k) mod 8
        d = Deflate().fixed([200] * k).stored(blob[100 * k:100 * k + 50 + k]).fixed([66, 67], final=True)
        out.append(Case("stored_after_%d" % k, d, dict(bitoff=(2 + k + 3) & 7)))
    out.append(Case("stored_len0", Deflate().stored(b"", final=True)))
    out.append(Case("stored_len1", Deflate().stored(b"\x5a", final=True)))
    out.append(Case("stored_len65535", Deflate().stored(blob[:65_535], final=True), dict(size=65_535)))
    out.append(Case("stored_65535_plus_1", Deflate().stored(blob[1:]).stored(blob[:1], final=True), dict(size=65_536, ntok=65_536)))
    lits = list(range(48, 58))
    d = Deflate().stored(blob[:300]).fixed(_lits(rng, 200, lits) + [(30, 250)]).dynamic(_lits(rng, 200, lits) + [(9, 400)], flat_lengths(lits + [256, 263], 286), [0] * 17 + [1])
    d.stored(b"").stored(blob[300:700]).dynamic([48, 49], flat_lengths([48, 49, 256], 286), [0]).fixed([(258, 1)], final=True)
    out.append(Case("interleaved", d, dict(kinds={0, 1, 2})))
    return out


def _size_cases():
    rng = random.Random(65)
    out = []
    ll = flat_lengths(list(range(64, 127)) + [256], 286)                          # 64 symbols at 6 bits: every literal pairs
    for n in (65_535, 65_536):
        out.append(Case("literals_fixed_%d" % n, Deflate().fixed(_lits(rng, n, list(range(144))), final=True), dict(size=n)))
        out.append(Case("literals_dynamic_%d" % n, Deflate().dynamic(_lits(rng, n, list(range(64, 127))), ll, [0], final=True), dict(size=n)))
        tok = _lits(rng, 1 + (n - 1) % 258, list(range(256))) + [(258, 1 + k % 200 if k % 3 else 1) for k in range((n - 1) // 258)]
        out.append(Case("matches_%d" % n, Deflate().fixed(tok, final=True), dict(size=n)))
        # literals of 9 bits miss the 8-bit table, so none is taken as the second of a pair: one token each, the workspace's capacity
        out.append(Case("single_literal_tokens_%d" % n, Deflate().fixed(_lits(rng, n, list(range(144, 256))), final=True), dict(size=n, ntok=n, unpaired=True)))
    # literal / 3-byte match alternating: no literal has a literal behind it
    tok = [t for k in range(16_384) for t in (k % 144, (3, 1 + k % 2))]
    out.append(Case("literal_match_alternating", Deflate().fixed(tok, final=True), dict(size=65_536, ntok=32_768, alternating=True)))
    return out


def _random_member(seed):
    rng = random.Random(seed)
    lits = rng.sample(range(256), rng.randrange(1, 257))
    lsyms = rng.sample(range(257, 286), rng.randrange(0, 30))
    dsyms = rng.sample(range(30), rng.randrange(0, 31)) if lsyms else []
    ll = random_code(rng, lits + [256] + lsyms, 286)
    dl = random_code(rng, dsyms, 30)
    size, tok, op = rng.randrange(0, 7900), [], 0
    while op < size:
        ds = [s for s in dsyms if DB[s] <= op]
        if ds and rng.random() < 0.4:
            s, q = rng.choice(lsyms) - 257, rng.choice(ds)
            n = 258 if s == 28 else LBASE[s] + rng.randrange(1 << LEXT[s])
            n -= n == 258 and s == 27                                             # (258 is symbol 285's; 284 + 31 has cases of its own)
            d = min(op, DB[q] + rng.randrange(1 << DEXT[q]))
            tok.append((n, d))
            op += n
        else:
            tok.append(rng.choice(lits))
            op += 1
    return Case("random%d" % seed, Deflate().dynamic(tok, ll, dl, final=True, rle=bool(seed & 1)), dict(rle=bool(seed & 1)))


@functools.lru_cache(maxsize=None)
def legal_launches():
    """name -> the members of one launch.  Every legal stream of the issue, grouped as the device test launches them"""
    worst = _worst()
    g = {}
    g["deep_codes"] = [_deep("deep_a", list(range(14))), _deep("deep_b", list(range(14, 28)))]
    g["worst_rate_alone"] = [worst]
    g["worst_rate_among_short"] = [small_member(i) for i in range(7)] + [worst] + [small_member(i) for i in range(7, 15)]
    g["two_literals"] = _two_cases()
    g["headers"] = _header_cases()
    g["lengths_distances"] = _length_distance_cases()
    g["stored"] = _stored_cases()
    g["sizes"] = _size_cases()
    g["random_codes"] = [_random_member(1000 + k) for k in range(256)]
    g["map_300"] = [small_member(i) for i in range(300)]
    g["map_129"] = [small_member(1000 + i) for i in range(129)]
    g["map_17"] = [small_member(2000 + i) for i in range(17)]
    return g


N_LEGAL = {"deep_codes": 2, "worst_rate_alone": 1, "worst_rate_among_short": 16, "two_literals": 14, "headers": 39, "lengths_distances": 13, "stored": 14,
           "sizes": 9, "random_codes": 256, "map_300": 300, "map_129": 129, "map_17": 17}


# ---- the illegal streams: (name, payload, announced size, the status InflateArgs documents) ---------------------------------------------------
_PAD = b"\0\0\0\0"                 # behind a stream that ends in an error: a decoder may look a whole 15-bit code ahead before it gives up


def _dyn_raw(hlit, hdist, cl, ops, hclen=None):
    """final dynamic block from a raw header; cl = the 19 code length code lengths by symbol"""
    ncl = hclen or max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
    d = Deflate()
    d.bits(1, 1)
    d.bits(2, 2)
    return d.raw_header(hlit, hdist, ncl - 4, [cl[s] for s in CL_ORDER[:ncl]], ops)


@functools.lru_cache(maxsize=None)
def illegal_cases():
    rng = random.Random(13)
    out = []
    cl_flat = flat_lengths(list(range(19)), 19)
    plain = [(8, 0)] * 255 + [(0, 0), (8, 0)]                                      # 257 literal / length lengths: 0 .. 254 and 256 at 8 bits -- complete
    # -- 1: block type, stored length
    d = Deflate()
    d.bits(1, 1)
    d.bits(3, 2)
    out.append(("block_type_3", d.getvalue() + _PAD, 10, 1))
    out.append(("len_nlen_mismatch", Deflate().stored(b"abcdefgh", final=True, nlen_field=0xfff6).getvalue(), 8, 1))
    # -- 2: code lengths
    for f in (30, 31):
        out.append(("hlit_field_%d" % f, _dyn_raw(f, 0, cl_flat, plain + [(0, 0)] * 40).getvalue() + _PAD, 100, 2))
        out.append(("hdist_field_%d" % f, _dyn_raw(0, f, cl_flat, plain + [(1, 0)] * 40).getvalue() + _PAD, 100, 2))
    cl = [0] * 19
    cl[0] = cl[8] = cl[18] = 1
    out.append(("cl_code_oversubscribed", _dyn_raw(0, 0, cl, [("raw", 0, 64)]).getvalue() + _PAD, 100, 2))
    out.append(("ll_code_oversubscribed", _dyn_raw(0, 0, cl_flat, plain[:254] + [(7, 0), (0, 0), (8, 0), (0, 0)]).symbols([1, 2], [8] * 257, [], eob=False).getvalue() + _PAD, 100, 2))
    out.append(("dist_code_oversubscribed", _dyn_raw(0, 2, cl_flat, plain + [(1, 0)] * 3).symbols([1, 2], [8] * 257, [], eob=False).getvalue() + _PAD, 100, 2))
    out.append(("repeat_first", _dyn_raw(0, 0, cl_flat, [(16, 0)] + plain).getvalue() + _PAD, 100, 2))
    out.append(("repeat_past_the_end", _dyn_raw(0, 0, cl_flat, plain[:250] + [(18, 0)]).getvalue() + _PAD, 100, 2))
    out.append(("no_end_of_block_code", _dyn_raw(0, 0, cl_flat, [(8, 0)] * 256 + [(0, 0), (0, 0)]).symbols([1, 2], [8] * 256, [], eob=False).getvalue() + _PAD, 100, 2))
    cl = [0] * 19
    cl[0], cl[8] = 1, 2                                                             # codes 0 and 10: 11 is no code
    out.append(("cl_symbol_without_code", _dyn_raw(0, 0, cl, [(8, 0), (0, 0), ("raw", 0xffff, 16)]).getvalue() + _PAD, 100, 2))
    cl = [0] * 19
    cl[0] = cl[18] = 1                                                              # HCLEN = 4: no length can be non-zero, so no end of block
    out.append(("hclen4_all_zero", _dyn_raw(0, 0, cl, [(18, 127), (18, 109)], hclen=4).getvalue() + _PAD, 100, 2))
    # -- 3: symbols and distances
    for s in (286, 287):
        d = Deflate()
        d.bits(1, 1)
        d.bits(1, 2)
        d.symbols([65, 66, 67], FIXED_LL, FIXED_D, eob=False).symbols([s], FIXED_LL, [], eob=False)
        out.append(("fixed_symbol_%d" % s, d.getvalue() + _PAD, 100, 3))
    for s in (30, 31):
        d = Deflate()
        d.bits(1, 1)
        d.bits(1, 2)
        d.symbols([65, 66, 67, 257], FIXED_LL, FIXED_D, eob=False).bits(int(format(s, "05b")[::-1], 2), 5)
        out.append(("fixed_distance_%d" % s, d.getvalue() + _PAD, 100, 3))
    for op in (0, 1, 32_767):
        d = Deflate()
        d.bits(1, 1)
        d.bits(1, 2)
        lits = _lits(rng, op, list(range(256)))
        d.symbols(lits, FIXED_LL, FIXED_D, eob=False)
        c, n = canon(FIXED_LL)[257]
        d.bits(c, n)
        ds, de, dx = dist_sym(op + 1)
        d.bits(canon(FIXED_D)[ds][0], 5)
        d.bits(dx, de)
        d.symbols([], FIXED_LL, FIXED_D)
        out.append(("distance_op_plus_1_at_%d" % op, d.getvalue() + _PAD, op + 3, 3))
    ll = flat_lengths([65, 66, 256, 257], 286)
    d = Deflate()
    d.dynamic([65, 66, 65], ll, [0], final=True, eob=False).symbols([257], ll, [], eob=False).bits(0, 7)
    d.symbols([], ll, [])
    out.append(("distance_symbol_without_a_distance_code", d.getvalue() + _PAD, 6, 3))
    # -- 4: output overrun
    out.append(("stored_one_too_many", Deflate().stored(b"abcdefgh", final=True).getvalue(), 7, 4))
    out.append(("single_literal_too_many", Deflate().fixed([65], final=True).getvalue(), 0, 4))
    out.append(("match_too_long", Deflate().fixed([65, (10, 1)], final=True).getvalue(), 5, 4))
    out.append(("literal_after_pair_too_many", Deflate().fixed([65, 66, 67], final=True).getvalue(), 2, 4))
    # -- 5: the stream ends early
    tok = _lits(rng, 2000, list(range(97, 123)))
    whole = Deflate().dynamic(tok, flat_lengths(list(range(97, 123)) + [256], 286), [0], final=True)
    z = whole.getvalue()
    out.append(("cut_in_header", z[:1], 2000, 5))
    out.append(("cut_in_code_lengths", z[:25], 2000, 5))
    out.append(("cut_mid_symbol", z[:len(z) // 2], 2000, 5))
    # -- 6: a whole stream of another length
    out.append(("one_byte_short_of_isize", z, 2001, 6))
    return out


N_ILLEGAL = 30

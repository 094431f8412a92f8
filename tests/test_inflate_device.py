"""DEFLATE on the device (csrc/nc_inflate.hip, one lane per BGZF member) against zlib: every block type and the streams zlib's strategies make,
members at unaligned offsets, the members of the spec-assembled BAM fixture, damaged inputs (reported, never a crash) -- and the legal streams
zlib's compressor never writes, with the illegal ones next to them, from the bit-level writer of tests/deflate_craft.py (each proven on zlib's
decompressor by tests/test_deflate_craft_ref.py)."""
import os
import zlib

import numpy as np
import pytest

import deflate_craft as C

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def _run(payloads, sizes, phases=(3,)):
    import torch
    from nanocaller_amd.engine import get_engine
    eng = get_engine(0)
    rng = np.random.default_rng(1)
    off, blob = [], bytearray()
    for p in payloads:
        blob += bytes(rng.integers(0, 256, size=int(rng.integers(0, 7))).astype(np.uint8))      # unaligned starts, junk between members
        off.append(len(blob))
        blob += p
    blob += bytes(16)
    ooff = np.zeros(len(payloads) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64) + 3, out=ooff[1:])                                      # (3 spare bytes between outputs: overruns would show)
    dev = eng.device
    d_comp = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(dev)
    d_coff = torch.tensor(off, dtype=torch.int64, device=dev)
    d_clen = torch.tensor([len(p) for p in payloads], dtype=torch.int32, device=dev)
    d_out = torch.full((int(ooff[-1]) + 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_ooff = torch.from_numpy(ooff[:-1].copy()).to(dev)
    d_isize = torch.tensor(list(sizes), dtype=torch.int32, device=dev)
    d_st = torch.full((len(payloads),), -1, dtype=torch.int32, device=dev)
    d_tok = torch.empty(((len(payloads) + 63) // 64) << 22, dtype=torch.int32, device=dev)
    d_ntok = torch.zeros(len(payloads), dtype=torch.int32, device=dev)
    eng.use_torch_stream()
    args = (len(payloads), d_comp.data_ptr(), d_coff.data_ptr(), d_clen.data_ptr(), d_out.data_ptr(), d_ooff.data_ptr(), d_isize.data_ptr(), d_st.data_ptr(),
            d_tok.data_ptr(), d_ntok.data_ptr())
    for ph in phases:                                                                              # (3: the one call; 1 then 2: the two launches apart, as device_bam.py makes them)
        rc = eng.L.nc_inflate_device(eng.ctx, *args) if ph == 3 else eng.L.nc_inflate_device_phase(eng.ctx, ph, *args)
        assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), ooff, d_st.cpu().numpy()


def _cases():
    rng = np.random.default_rng(7)
    text = (b"chr20\t1234567\t.\tA\tG\t33.10\tPASS\t.\tGT:DP:FQ\t0/1:31:0.4839\n" * 900)[:60_000]
    dna4 = bytes(rng.integers(0, 256, size=65_280).astype(np.uint8))                              # packed bases: incompressible
    qual = bytes((rng.normal(20, 6, size=65_280).clip(0, 60)).astype(np.uint8))                    # quality-like: entropy coded, few matches
    runs = b"".join(bytes([int(b)]) * int(n) for b, n in zip(rng.integers(0, 4, 400), rng.integers(1, 400, 400)))[:65_280]
    far = bytes(rng.integers(0, 256, size=20_000).astype(np.uint8))                                # matches at distance 20,000 / 31,000: older than k_lz's
    far2 = bytes(rng.integers(0, 256, size=31_000).astype(np.uint8))                               # 16 KB ring, read back from HBM
    data = [b"", b"A", b"AB" * 3, bytes(65_280), text, dna4, qual, runs, bytes(range(256)) * 255, far * 3, (far2 * 3)[:65_280], (qual[:9_000] + far[:9_000]) * 3]
    out = []
    for d in data:
        for kw in (dict(level=6), dict(level=1), dict(level=9), dict(level=0), dict(level=6, strategy=zlib.Z_FIXED), dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY),
                   dict(level=6, strategy=zlib.Z_RLE), dict(level=6, strategy=zlib.Z_FILTERED), dict(level=9, mem=1)):
            out.append((d, _deflate(d, **kw)))
    # several deflate blocks in one member (Z_FULL_FLUSH between pieces: stored + dynamic + fixed in one stream)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    multi = c.compress(text[:20_000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(dna4[:20_000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(runs[:20_000]) + c.flush()
    out.append((text[:20_000] + dna4[:20_000] + runs[:20_000], multi))
    return out


def test_device_inflate_equals_zlib():
    cases = _cases()
    out, ooff, st = _run([p for _, p in cases], [len(d) for d, _ in cases])
    assert not st.any(), np.nonzero(st)[0][:10]
    for k, (d, _) in enumerate(cases):
        got = out[ooff[k]:ooff[k] + len(d)].tobytes()
        assert got == d, k
        assert out[ooff[k] + len(d):ooff[k] + len(d) + 3].tolist() == [0xEE] * 3, k               # nothing written past the announced size
    kinds = {(p[0] >> 1) & 3 for _, p in cases if p}
    assert kinds == {0, 1, 2}


def test_runs_of_empty_stored_blocks_do_not_starve_the_stream_window():
    """legal deflate: dozens of empty stored blocks in a row (repeated sync flushes; 5 bytes each, no symbol loop runs) between real blocks --
    the per-lane window of the compressed stream is topped up per block header, not only inside the symbol loops"""
    rng = np.random.default_rng(11)
    a = bytes((rng.normal(20, 6, size=9_000).clip(0, 60)).astype(np.uint8))
    b = (b"chr20\t1234567\t.\tA\tG\t33.10\n" * 400)[:9_000]
    cases = []
    for n_empty in (1, 30, 64, 200):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        empty = b"\x00\x00\x00\xff\xff"                                                         # BFINAL = 0, BTYPE = 00, padding; LEN = 0, NLEN = 0xffff
        z = c.compress(a) + c.flush(zlib.Z_SYNC_FLUSH)                                            # (byte-aligned behind a sync flush: zlib itself writes one empty stored block there)
        z += empty * n_empty
        z += c.compress(b) + c.flush(zlib.Z_FULL_FLUSH)
        z += empty * n_empty
        z += c.compress(a[:100]) + c.flush()
        assert zlib.decompress(z, -15) == a + b + a[:100]
        cases.append((a + b + a[:100], z))
    out, ooff, st = _run([p for _, p in cases], [len(d) for d, _ in cases])
    assert not st.any(), st
    for k, (d, _) in enumerate(cases):
        assert out[ooff[k]:ooff[k] + len(d)].tobytes() == d, k


def test_device_inflate_on_the_members_of_the_spec_fixture():
    raw = open(os.path.join(G, "spec.bam"), "rb").read()
    pay, want, o = [], [], 0
    while o < len(raw):
        bsize = int.from_bytes(raw[o + 16:o + 18], "little") + 1
        p = raw[o + 18:o + bsize - 8]
        pay.append(p)
        want.append(zlib.decompress(p, -15))
        assert len(want[-1]) == int.from_bytes(raw[o + bsize - 4:o + bsize], "little")
        o += bsize
    out, ooff, st = _run(pay, [len(w) for w in want])
    assert not st.any() and len(pay) > 30
    assert b"".join(out[ooff[k]:ooff[k] + len(w)].tobytes() for k, w in enumerate(want)) == b"".join(want)


def test_damaged_members_are_reported():
    d = (b"ACGTTGCA" * 4000)[:30_000]
    good = _deflate(d)
    rng = np.random.default_rng(3)
    junk = bytes(rng.integers(0, 256, size=400).astype(np.uint8))
    cases = [(good, len(d)), (good, len(d) - 1), (good, len(d) + 1), (good[:len(good) // 2], len(d)), (junk, 5_000), (b"\x07", 10), (good, len(d))]
    out, ooff, st = _run([p for p, _ in cases], [n for _, n in cases])
    assert st[0] == 0 and st[-1] == 0 and all(st[1:-1] != 0), st
    assert out[ooff[0]:ooff[0] + len(d)].tobytes() == d and out[ooff[6]:ooff[6] + len(d)].tobytes() == d
    for k, (_, n) in enumerate(cases):
        assert out[ooff[k] + n:ooff[k] + n + 3].tolist() == [0xEE] * 3, k                         # even a damaged member stays inside its own output


def _crc_status(payloads, datas, trailers):
    """nc_bgzf_crc_device over hand-laid members: payload + trailer (CRC-32, ISIZE) back to back in one buffer, inflated bytes in another"""
    import torch
    from nanocaller_amd.engine import get_engine
    eng = get_engine(0)
    blob, coff = bytearray(), []
    for p, t in zip(payloads, trailers):
        blob += b"\x55" * (len(blob) % 3)                                                        # unaligned members
        coff.append(len(blob))
        blob += p + t
    blob += bytes(16)
    sizes = [len(d) for d in datas]
    ooff = np.zeros(len(datas) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64) + 1, out=ooff[1:])                                      # (odd gaps: every alignment of a member's first byte)
    raw = np.full(int(ooff[-1]) + 16, 0xEE, np.uint8)
    for k, d in enumerate(datas):
        raw[ooff[k]:ooff[k] + len(d)] = np.frombuffer(d, np.uint8)
    dev = eng.device
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(dev)                                 # noqa: E731
    d_comp, d_out = t(np.frombuffer(bytes(blob), np.uint8).copy(), np.uint8), t(raw, np.uint8)
    d_coff, d_clen, d_ooff, d_isize = t(coff, np.int64), t([len(p) for p in payloads], np.int32), t(ooff[:-1].copy(), np.int64), t(sizes, np.int32)
    d_st = torch.zeros(len(datas), dtype=torch.int32, device=dev)
    eng.use_torch_stream()
    rc = eng.L.nc_bgzf_crc_device(eng.ctx, len(datas), d_comp.data_ptr(), d_coff.data_ptr(), d_clen.data_ptr(), d_out.data_ptr(), d_ooff.data_ptr(),
                                  d_isize.data_ptr(), d_st.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return d_st.cpu().numpy()


def test_device_crc32_equals_zlibs_and_reports_a_damaged_member():
    """k_crc32 (slice-by-4 per lane over 1024-byte slices cut from the member's end, tree combine by x^(8192 * 2^l) mod P) against zlib.crc32 on every
    length class: empty, shorter than a dword, one slice and a bit, exact multiples of 1024, the BGZF maximum 65,280 and 65,536; then the same
    members with one bit of data flipped, and with a wrong trailer: status 7"""
    rng = np.random.default_rng(5)
    lens = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 1023, 1024, 1025, 2048, 4097, 10_000, 30_001, 65_279, 65_280, 65_535, 65_536]
    datas = [bytes(rng.integers(0, 256, size=n).astype(np.uint8)) for n in lens]
    pay = [bytes(rng.integers(0, 256, size=int(rng.integers(1, 40))).astype(np.uint8)) for _ in lens]      # (the payload bytes themselves are not read)
    good = [int(zlib.crc32(d)).to_bytes(4, "little") + len(d).to_bytes(4, "little") for d in datas]
    st = _crc_status(pay, datas, good)
    assert not st.any(), [lens[k] for k in np.nonzero(st)[0]]
    flipped = []
    for d in datas:
        if d:
            b = bytearray(d)
            k = int(rng.integers(0, len(b)))
            b[k] ^= 1 << int(rng.integers(0, 8))
            flipped.append(bytes(b))
        else:
            flipped.append(d)
    st = _crc_status(pay, flipped, good)
    assert all((s == 7) == (n > 0) for s, n in zip(st.tolist(), lens)), st
    bad_trailer = [(int(zlib.crc32(d)) ^ 0x00010000).to_bytes(4, "little") + len(d).to_bytes(4, "little") for d in datas]
    st = _crc_status(pay, datas, bad_trailer)
    assert (st == 7).all()


PHASES = pytest.mark.parametrize("phases", [(3,), (1, 2)], ids=["one_call", "huffman_then_matches"])


@PHASES
@pytest.mark.parametrize("launch", list(C.N_LEGAL))
def test_crafted_legal_streams_inflate_to_their_tokens(launch, phases):
    """The legal DEFLATE zlib's compressor does not write, one launch per group of tests/deflate_craft.py (what each stream holds is asserted on the
    CPU by tests/test_deflate_craft_ref.py): status 0, the bytes of `expand`, the three guard bytes behind every output intact -- through
    nc_inflate_device and through nc_inflate_device_phase(1) then (2), the production route's two launches.
      deep_codes              15-bit codes in both alphabets behind the 8- / 5-bit first-level tables (slow_from, walk_start, the ninth-bit mask hi[])
      worst_rate_*            124 matches of 48 bits back to back: the per-lane stream window (tick / refill) at its least slack; alone in its
                              workgroup, and as one of 16 lanes of which 15 finish at once
      two_literals            the second literal of a step (`two`): op + 2 == isize, an odd size, a successor that is the end of block, a length
                              symbol, or a literal the table misses -- dynamic and fixed
      headers                 nlen 257 / 286, ndist 1 (length 0, and length 1 for each of the 30 symbols) / 30, 5 / 8 / 19 code length code lengths (4 cannot
                              be legal: no length could be non-zero; it is among the illegal streams), 16 x 6 / 17 x 10 / 18 x 138, a 16-run from
                              the literal into the distance lengths, zeros over 257-285, a second block with fewer lengths than the first (the nibbles)
      lengths_distances       every length at distance 1 and beyond 258, 258 as 284 + 31, every distance symbol's edges, distance == op around
                              k_lz's ring and flush sizes (distance 32,768 read back from HBM at its first byte), matches chained inside a step
      stored                  take(bc & 7) at every bit offset, LEN 0 / 1 / 65,535, 65,536 tokens from two stored blocks, all three types in one member
      sizes                   65,535 / 65,536 bytes as literals, as matches, and as that many single-literal tokens (9-bit literals never pair): the
                              token workspace's capacity; literal / 3-byte match alternating
      random_codes            256 members of seeded random complete codes (depth <= 15) and random tokens, half with run-length coded lengths
      map_300 / _129 / _17    k_lz's block -> member permutation beyond 128 members and off its 16 / 128 boundaries: distinct contents everywhere
    Not among them, on purpose: an INCOMPLETE literal / length or distance set of several symbols whose unused codes never occur.  The kernel
    accepts it (huff_build's comment), zlib refuses it; neither list has such a stream."""
    cases = C.legal_launches()[launch]
    assert len(cases) == C.N_LEGAL[launch]
    out, ooff, st = _run([c.z for c in cases], [len(c.want) for c in cases], phases)
    assert st.tolist() == [0] * len(cases), [(c.name, int(s)) for c, s in zip(cases, st) if s][:10]
    for k, c in enumerate(cases):
        n = len(c.want)
        assert out[ooff[k]:ooff[k] + n].tobytes() == c.want, c.name
        assert out[ooff[k] + n:ooff[k] + n + 3].tolist() == [0xEE] * 3, c.name


@PHASES
def test_crafted_illegal_streams_get_their_documented_status(phases):
    """every stream zlib refuses (and the sound ones of another length than announced) ends in the status InflateArgs documents for it -- exactly
    --, writes nothing past its announced size, and the good members before and behind it come out right.  Status 5 is every member whose
    decoding consumed bits behind its payload's end, whatever those bits were (here: a few random bytes and the next member)."""
    ill = C.illegal_cases()
    assert len(ill) == C.N_ILLEGAL
    good = [C.small_member(3000 + i) for i in range(len(ill) + 1)]
    pay, sizes = [good[0].z], [len(good[0].want)]
    for (_, z, n, _), g in zip(ill, good[1:]):
        pay += [z, g.z]
        sizes += [n, len(g.want)]
    out, ooff, st = _run(pay, sizes, phases)
    got = {name: int(st[2 * k + 1]) for k, (name, _, _, _) in enumerate(ill)}
    assert got == {name: want for name, _, _, want in ill}
    for k, g in enumerate(good):
        assert st[2 * k] == 0 and out[ooff[2 * k]:ooff[2 * k] + len(g.want)].tobytes() == g.want, k
    for k, n in enumerate(sizes):
        assert out[ooff[k] + n:ooff[k] + n + 3].tolist() == [0xEE] * 3, k

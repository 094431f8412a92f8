"""The device DEFLATE writer (k_deflate, k_member_crc, k_scan_excl, k_assemble of csrc/nc_bamwrite.hip) against its specification, the
Python model of tests/deflate_model.py: every payload byte for byte, on the members of tests/deflate_cases.py (each proven to reach its edge
by tests/test_deflate_model_ref.py), with more members than workgroups in one launch, twice over; the CRC-32 at every source alignment;
the file assembly above 1,024 members.  No tolerance anywhere: every comparison is exact.

Measured: the stored-threshold members are draws 9 and 12 of deflate_cases.draw, one byte under and exactly on the threshold (margins -1
and 0; test_deflate_model_ref.test_stored_threshold).  Run times on one MI355X, the model's work included: test_payload_equals_model
0.7 s (+ 1.9 s for the engine, once per module), test_more_members_than_workgroups 0.04 s, test_deterministic 0.1 s, test_crc_sweep
under 0.01 s, test_assembly_above_1024_members 0.4 s."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import deflate_cases as D
from test_inflate_device import _run as _inflate_device

pytestmark = pytest.mark.gpu
SLOT = 65536
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def eng():
    from nanocaller_amd.engine import get_engine
    return get_engine(0)


def _launch(eng, blob, ioff, ilen, ctx=None):
    """nc_bgzf_deflate_device on the test's own buffers: every payload slot prefilled with 0xEE, clen / status / crc with -7.
    -> (slots [n, 65536] as a device tensor, clen, status, crc as numpy)"""
    import torch
    dev = eng.device
    n = len(ilen)
    d_in = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    d_ioff = torch.tensor(list(ioff), dtype=torch.int64, device=dev)
    d_ilen = torch.tensor(list(ilen), dtype=torch.int32, device=dev)
    pay = torch.full((n * SLOT,), 0xEE, dtype=torch.uint8, device=dev)
    poff = torch.arange(n, dtype=torch.int64, device=dev) * SLOT
    clen, st, crc = (torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    if ctx is None:
        eng.use_torch_stream()
        ctx = eng.ctx
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.L.nc_bgzf_deflate_device(ctx, n, p(d_in), p(d_ioff), p(d_ilen), p(pay), p(poff), p(clen), p(crc), p(st))
    assert rc == 0
    torch.cuda.synchronize()
    return pay.view(n, SLOT), clen.cpu().numpy(), st.cpu().numpy(), crc.cpu().numpy().view(np.uint32)


def _pack(members):
    """members back to back (so their sources start at every alignment), 16 spare bytes behind"""
    ilen = [len(m) for m in members]
    ioff = np.concatenate([[0], np.cumsum(ilen)[:-1]]).astype(np.int64)
    return b"".join(members) + bytes(16), ioff, ilen


def _slot(payload):
    s = np.full(SLOT, 0xEE, np.uint8)
    s[:len(payload)] = np.frombuffer(payload, np.uint8)
    return s


def _diff(got, want):
    """where a slot differs from the model's, in words"""
    bad = np.flatnonzero(got != want)
    return "first difference at byte %d of %d differing (kernel %s, model %s)" % (bad[0], bad.size, got[bad[0]:bad[0] + 8].tolist(),
                                                                                  want[bad[0]:bad[0] + 8].tolist())


def test_payload_equals_model(eng):
    names = sorted(D.cases())
    members = [D.cases()[k] for k in names]
    slots, clen, st, crc = _launch(eng, *_pack(members))
    slots = slots.cpu().numpy()
    wrong = []
    for k, name in enumerate(names):
        want = D.model(name)[0]
        if st[k] != 0 or clen[k] != len(want):
            wrong.append("%s: status %d, clen %d (model: %d bytes)" % (name, st[k], clen[k], len(want)))
        elif not np.array_equal(slots[k], _slot(want)):                   # the payload, and 0xEE from clen to the slot's end
            wrong.append("%s: %s" % (name, _diff(slots[k], _slot(want))))
        if int(crc[k]) != zlib.crc32(members[k]):
            wrong.append("%s: CRC-32 %08x, zlib's %08x" % (name, crc[k], zlib.crc32(members[k])))
    assert not wrong, "\n".join(wrong)
    pays = [slots[k, :clen[k]].tobytes() for k in range(len(names))]
    for m, p in zip(members, pays):
        assert zlib.decompress(p, -15) == m
    out, ooff, ist = _inflate_device(pays, [len(m) for m in members])     # and through the device reader
    assert not ist.any()
    for k, m in enumerate(members):
        assert out[ooff[k]:ooff[k] + len(m)].tobytes() == m, names[k]


KINDS = ("acgt65280", "small7", "empty", "rand1500", "negative", "too_long", "deep7", "small40")


def _many(cus):
    """2 * cus + 3 members of 8 kinds over 6 distinct contents: workgroup g takes members g, g + cus, g + 2 cus, kinds (g + round) mod 8 --
    a full member before a 7-byte one, the deep-tree member before a 40-byte one, refused and empty members before and behind real ones"""
    content = {k: D.cases()[k] for k in KINDS if k in D.cases()}
    content["empty"] = b""
    at, blob = {}, bytearray()
    for k, m in content.items():
        at[k] = len(blob)
        blob += m
    at["negative"], at["too_long"] = 1, 0
    blob += bytes(0xff01 + 16 - min(len(blob), 0xff01 + 16))
    length = dict({k: len(m) for k, m in content.items()}, negative=-1, too_long=0xff01)
    kinds = [KINDS[(b % cus + b // cus) % 8] for b in range(2 * cus + 3)]
    return bytes(blob), [at[k] for k in kinds], [length[k] for k in kinds], kinds, content


def _check_many(kinds, content, slots, clen, st):
    pays = {k: D.model(k)[0] if k in D.cases() else D.deflate_model(content[k])[0] for k in content}
    want = {k: (_slot(p), len(p), 0) for k, p in pays.items()}
    want["negative"] = want["too_long"] = (_slot(b""), 0, 1)              # refused: status 1, clen 0, the slot untouched
    wrong = []
    for b, k in enumerate(kinds):
        w, c, s = want[k]
        if st[b] != s or clen[b] != c:
            wrong.append("member %d (%s): status %d, clen %d (model: %d, %d)" % (b, k, st[b], clen[b], s, c))
        elif not np.array_equal(slots[b], w):
            wrong.append("member %d (%s): %s" % (b, k, _diff(slots[b], w)))
    assert not wrong, "%d members wrong\n" % len(wrong) + "\n".join(wrong[:20])


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_more_members_than_workgroups(eng):
    blob, ioff, ilen, kinds, content = _many(_cus())
    assert len(kinds) > 2 * _cus() and set(kinds) == set(KINDS)
    slots, clen, st, crc = _launch(eng, blob, ioff, ilen)
    _check_many(kinds, content, slots.cpu().numpy(), clen, st)
    for b, k in enumerate(kinds):
        if k in content:
            assert int(crc[b]) == zlib.crc32(content[k]), (b, k)


def test_deterministic(eng):
    import torch
    blob, ioff, ilen, kinds, content = _many(_cus())
    a = _launch(eng, blob, ioff, ilen)
    b = _launch(eng, blob, ioff, ilen)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a fresh context whose token buffer first serves other members (every workgroup's tokens then are another member's leftovers)
    ctx = C.c_void_p()
    assert eng.L.nc_ctx_create(eng.device.index, C.byref(ctx)) == 0
    try:
        assert eng.L.nc_ctx_set_stream(ctx, C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)) == 0
        oblob, ooff, olen = _pack([D.cases()[k] for k in ("same", "dist32768", "acgt65279", "period33")])
        _launch(eng, oblob, list(ooff) * (_cus() // 2), olen * (_cus() // 2), ctx=ctx)
        c = _launch(eng, blob, ioff, ilen, ctx=ctx)
    finally:
        eng.L.nc_ctx_destroy(ctx)
    assert torch.equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
    _check_many(kinds, content, c[0].cpu().numpy(), c[1], c[2])


def test_crc_sweep(eng):
    import torch
    rng = np.random.default_rng(31)
    members = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in list(range(521)) + [65279, 65280]]
    blob, ioff, ilen = _pack(members)
    assert {int(o) % 4 for o in ioff} == {0, 1, 2, 3}
    dev = eng.device
    d_in = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    d_ioff = torch.from_numpy(ioff).to(dev)
    d_ilen = torch.tensor(ilen, dtype=torch.int32, device=dev)
    crc = torch.zeros(len(members), dtype=torch.int32, device=dev)
    eng.use_torch_stream()
    eng.bgzf_crc32(d_in, d_ioff, d_ilen, crc)
    torch.cuda.synchronize()
    got = crc.cpu().numpy().view(np.uint32)
    want = np.array([zlib.crc32(m) for m in members], np.uint32)
    assert np.array_equal(got, want), "lengths %s" % [ilen[k] for k in np.flatnonzero(got != want)[:20]]


def test_assembly_above_1024_members(eng):
    import torch
    from nanocaller_amd.bam_write import PAYLOAD_SLOT, deflate_members
    rng = np.random.default_rng(32)
    members = [rng.integers(65, 70, int(n)).astype(np.uint8).tobytes() for n in rng.integers(1, 41, 2500)]
    blob, ioff, ilen = _pack(members)
    dev = eng.device
    eng.use_torch_stream()
    d_in = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    pay, poff, clen, crc, st, d_ilen = deflate_members(eng, d_in, ioff, np.array(ilen, np.int32))
    assert int(st.count_nonzero().item()) == 0
    n = len(members)
    foff = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    eng.bgzf_assemble(pay, poff, clen, crc, d_ilen, foff)                  # the offsets alone, then the image
    torch.cuda.synchronize()
    c = clen.cpu().numpy()
    want_foff = np.concatenate([[0], np.cumsum(c.astype(np.int64) + 26)])
    assert np.array_equal(foff.cpu().numpy(), want_foff)
    file = torch.full((int(want_foff[-1]) + 28 + 8,), 0xEE, dtype=torch.uint8, device=dev)
    foff.fill_(-7)
    eng.bgzf_assemble(pay, poff, clen, crc, d_ilen, foff, file)
    torch.cuda.synchronize()
    assert np.array_equal(foff.cpu().numpy(), want_foff)
    p, cr = pay.cpu().numpy(), crc.cpu().numpy().view(np.uint32)
    image = bytearray()
    for k, m in enumerate(members):
        payload = p[k * PAYLOAD_SLOT:k * PAYLOAD_SLOT + int(c[k])].tobytes()
        assert payload == D.deflate_model(m)[0] and int(cr[k]) == zlib.crc32(m)
        image += struct.pack("<4BI2BH2B2H", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(payload) + 25) + payload
        image += struct.pack("<II", zlib.crc32(m), len(m))
    image += EOF_BLOCK
    got = file.cpu().numpy()
    assert got[:len(image)].tobytes() == bytes(image)
    assert got[len(image):].tolist() == [0xEE] * 8
    assert gzip.decompress(bytes(image)) == b"".join(members)

    # no member at all: the EOF block alone
    foff0 = torch.full((1,), -7, dtype=torch.int64, device=dev)
    file0 = torch.full((28 + 8,), 0xEE, dtype=torch.uint8, device=dev)
    empty32 = torch.zeros(0, dtype=torch.int32, device=dev)
    eng.bgzf_assemble(torch.zeros(1, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), empty32, empty32, empty32, foff0, file0)
    torch.cuda.synchronize()
    assert foff0.cpu().tolist() == [0]
    assert file0.cpu().numpy().tobytes() == EOF_BLOCK + b"\xee" * 8

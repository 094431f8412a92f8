"""Members crafted for the edges of the device DEFLATE writer, shared by tests/test_deflate_model_ref.py (the model proves every claim on
the CPU) and tests/test_deflate_device_gpu.py (the kernel against the model).  `cases()` -> {name: bytes}; `model(name)` -> the model's
(payload, info), computed once per process."""
import functools

import numpy as np

from deflate_model import deflate_model

SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769, 65279, 65280)
PERIODS = (1, 3, 5, 33, 1025)
FIB = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89)


def deep_literal_tree(n_main):
    """1,024-byte batches of 256 groups `m m m p`; every batch's partners `p` occur in no other batch, so no 4-gram of a batch occurs in an
    earlier one: no match.  Partner and main counts follow Fibonacci's numbers: a literal tree deeper than 15."""
    main = [377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711][:n_main]
    n_batch = -(-sum(main) // 768)
    main[-1] += 768 * n_batch - sum(main)
    sym = iter(range(256))
    partners = []
    b0 = [next(sym) for _ in FIB]
    partners.append(sum(([s] * c for s, c in zip(b0, FIB)), []))
    partners[0] += [next(sym)] * (256 - len(partners[0]))
    for c in (144, 233):
        s, f = next(sym), next(sym)
        partners.append([s] * c + [f] * (256 - c))
    while len(partners) < n_batch:
        partners.append([next(sym)] * 256)
    ms = [next(sym) for _ in main]
    mains = np.repeat(np.array(ms, np.uint8), main).reshape(-1, 3)
    out = np.empty((n_batch * 256, 4), np.uint8)
    out[:, :3] = mains
    out[:, 3] = np.array(partners, np.uint8).reshape(-1)
    return out.tobytes()


def deep_code_length_tree():
    """1,023 bytes (one batch: no candidates) whose byte counts are 2^(10 - l): the literal code's lengths are exactly l, and consecutive byte
    values never share one, so the run-length coding has no repeats and the code-length alphabet's frequencies are the skewed counts below"""
    left = {3: 2, 5: 7, 6: 6, 7: 29, 8: 13, 9: 43, 10: 77}
    lens, prev = [], 0
    while any(left.values()):
        ln = max((l for l in left if left[l] and l != prev), key=lambda l: (left[l], -l))
        lens.append(ln)
        left[ln] -= 1
        prev = ln
    data = np.repeat(np.arange(len(lens), dtype=np.uint8), [1 << (10 - l) for l in lens])
    np.random.default_rng(11).shuffle(data)
    return data.tobytes(), lens


def distance_limit(second_at):
    rng = np.random.default_rng(21)
    block = rng.integers(100, 256, 64).astype(np.uint8).tobytes()
    fill = rng.integers(0, 2, second_at - 64).astype(np.uint8).tobytes()
    tail = rng.integers(2, 100, 50).astype(np.uint8).tobytes()
    return block + fill + block + tail


def length_limit(second_at):
    """a 300-byte block, a gap, the block again up to the member's last byte (the gap of bytes 0 / 1 only: its few 4-grams leave the block's
    hash heads alone)"""
    rng = np.random.default_rng(22)
    block = rng.integers(100, 256, 300).astype(np.uint8).tobytes()
    return block + rng.integers(0, 2, second_at - 300).astype(np.uint8).tobytes() + block


# From the second batch on every segment of a periodic member starts a 258-byte match, so segment k's entry is 32 k + 226 and every cut
# leaves 32 bytes -- but for the first segment whose match is clipped by the member's end: it keeps (len - 2) mod 32 bytes.  The lengths
# below make that 3 (a 3-byte match), 1 and 2 (literals), and 6.
PERIOD_LEN = {1: 4997, 3: 4995, 5: 4996, 33: 5000, 1025: 5000}


def periodic(period):
    n = PERIOD_LEN[period]
    unit = np.random.default_rng(23 + period).integers(0, 256, period).astype(np.uint8).tobytes()
    return (unit * (n // period + 1))[:n]


def acgt_runs(n):
    rng = np.random.default_rng(24)
    out = bytearray()
    while len(out) < n:
        out += bytes(b"ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(1, 60))))
        out += bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.integers(1, 40))
    return bytes(out[:n])


def draw(seed):
    """the stored-threshold search's draw number `seed`: 200..600 bytes of a 200-symbol alphabet, the symbols' weights skewed by a drawn
    exponent (uniform draws all end 12..35 bytes on the stored side; the skew spreads the sizes over both sides)"""
    rng = np.random.default_rng(1000 + seed)
    w = rng.random(200) ** rng.uniform(0.0, 3.0)
    return rng.choice(200, int(rng.integers(200, 601)), p=w / w.sum()).astype(np.uint8).tobytes()


# the draws of `draw` nearest to the stored threshold on each side (test_deflate_model_ref.test_stored_threshold states how they were found)
THRESHOLD_DYNAMIC, THRESHOLD_STORED = 9, 12


@functools.lru_cache(maxsize=None)
def cases():
    c = {"same": b"A" * 0xff00, "deep7": deep_literal_tree(7), "deep9": deep_literal_tree(9), "cltree": deep_code_length_tree()[0]}
    for at in (32767, 32768, 32769):
        c["dist%d" % at] = distance_limit(at)
    c["len_end"] = length_limit(2048)
    c["len_half"] = length_limit(32768 - 128)
    for p in PERIODS:
        c["period%d" % p] = periodic(p)
    acgt, rand = acgt_runs(0xff00), np.random.default_rng(25).integers(0, 256, 0xff00).astype(np.uint8).tobytes()
    for n in SIZES:
        c["acgt%d" % n] = acgt[:n]
        c["rand%d" % n] = rand[:n]
    c["thr_dynamic"] = draw(THRESHOLD_DYNAMIC)
    c["thr_stored"] = draw(THRESHOLD_STORED)
    # (the launch with more members than workgroups; the 40 bytes are a dynamic block of symbols that no larger member uses)
    c.update(small7=acgt[100:107], small40=b"xyxxyzzy" * 5, rand1500=rand[3000:4500])
    return c


@functools.lru_cache(maxsize=None)
def model(name):
    return deflate_model(cases()[name])

"""Wall time of the haplotagged-BAM writer (nanocaller_amd/bam_write.py, csrc/nc_bamwrite.hip) on a chr20-sized ONT-like contig (64.4 Mb,
30x, tools/ont_like_bam.make_files) with a haplotag table that tags about half of the read names.  The input is loaded into HBM first
(untimed: the phaser has it resident when phase_run writes).  Reports per-stage milliseconds, k_deflate's input rate, the compressed size
against zlib level 1 on the same members, and that zlib baseline's wall time on 16 host threads.  Prints one JSON line.
Usage: python tools/bench_phased_bam.py [--length L] [--reps N]"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nanocaller_amd.bam_write import BGZF_BLOCK, member_spans, write_haplotagged_bam  # noqa: E402
from nanocaller_amd.device_bam import M_HASH_HI, M_HASH_LO, open_device_bam  # noqa: E402
from nanocaller_amd.engine import get_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    from ont_like_bam import make_files
    eng = get_engine(0)
    eng.use_torch_stream()
    tmp = a.dir or tempfile.mkdtemp(prefix="pbam")
    bam, refs, _, stats = make_files(eng, tmp, 1, a.length, depth=a.depth)
    chrom = refs[0][0]
    db = open_device_bam(bam, 0, contigs=[chrom])
    lo, hi = db.tid_range[0]
    h = np.unique(db.meta[M_HASH_LO, lo:hi].astype(np.uint32).astype(np.uint64) | (db.meta[M_HASH_HI, lo:hi].astype(np.uint32).astype(np.uint64) << np.uint64(32)))
    rng = np.random.default_rng(1)
    pick = rng.random(h.size) < 0.5
    tags = dict(hash=h[pick], hp=rng.integers(1, 3, int(pick.sum())).astype(np.uint8), ps=rng.integers(1, a.length, int(pick.sum())).astype(np.int32))
    out = os.path.join(tmp, "phased.bam")
    runs = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = write_haplotagged_bam(bam, chrom, tags, out)
        runs.append((time.perf_counter() - t, r))
    runs = runs[1:]
    best = min(runs, key=lambda x: x[0])[1]
    ms = best["ms"]
    # after timing: zlib level 1 over the same members (header members, then the record stream cut at 0xff00), 16 threads
    import gzip
    blob = gzip.decompress(open(out, "rb").read())
    hl = best["header_bytes"]
    ho, hln = member_spans(hl)
    ro, rln = member_spans(len(blob) - hl, base=hl)
    spans = list(zip(np.concatenate([ho, ro]).tolist(), np.concatenate([hln, rln]).tolist()))

    def z1(s):
        return len(zlib.compress(blob[s[0]:s[0] + s[1]], 1)) - 6            # (the raw-deflate payload: no zlib header / Adler-32)
    with ThreadPoolExecutor(16) as pool:
        t = time.perf_counter()
        zl = sum(pool.map(z1, spans))
        t_z = time.perf_counter() - t
    payload = best["bytes_out"] - 26 * best["members"] - 28
    dev_ms = ms["retag"] + ms["deflate"] + ms["crc"] + ms["assemble"]
    print(json.dumps(dict(
        workload="chr20-sized ONT-like contig, %.1f Mb, %.0fx" % (a.length / 1e6, a.depth), records=best["records"], tagged=best["tagged"],
        input_bam_bytes=stats["bam_bytes"], inflated_bytes_in=len(blob) - hl + 0, inflated_bytes_out=best["inflated_bytes"],
        members=best["members"], compressed_bytes=best["bytes_out"], payload_vs_zlib1=round(payload / zl, 4),
        ms={k: round(v, 2) for k, v in ms.items()}, device_stages_ms=round(dev_ms, 2),
        deflate_GBps=round(best["inflated_bytes"] / (ms["deflate"] * 1e-3) / 1e9, 2),
        wall_s=[round(x[0], 3) for x in runs], host_zlib1_16_threads_s=round(t_z, 3), block=BGZF_BLOCK)))


if __name__ == "__main__":
    main()

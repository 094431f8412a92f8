#!/usr/bin/env python3
"""The gVCF's two writers on the chr20-sized synthetic contig of tools/bench_gvcf.py, and bench.py's headline on this build
against the parent commit with the option off.

    python tools/bench_gvcf_write.py [--parent DIR] [--pairs K] [--length L] [--reps N] [--variant-every V] [--host-merge-lines M] [--out profiles/gvcf_write.json]

One process, the pack resident in HBM, the per-column words held (Engine.refconf_columns) as caller() holds them for a group; a synthetic
variant line every V columns stands for the group's records.  After a warm-up the two writers run alternating, N times each:

    host     span 1: gvcf.group_blocks + gvcf.splice to the plain worker file            span 2: gvcf.merge_worker_files to .g.vcf.gz + .csi
    device   span 1: gvcf.group_pieces to the worker's piece file + its sidecar           span 2: gvcf.merge_pieces to .g.vcf.gz + .csi

both by the host clock around the whole span, the files on --tmp (default: the system's temporary directory).  The Python merge of the host
writer parses every line: above --host-merge-lines lines it is not run (null in the report) and the device writer's file is then checked against
the plain worker file instead of the merged one.  Per stage of the device writer (device events, summed over the pieces): blocks, text, merge,
deflate, crc, assemble, d2h, index; write by the host clock.  The merge kernel alone is timed over N calls, beside a device-to-device copy of the
same bytes; the compressed size is set beside the host compressor's (nc_bgzf_compress, level 6) on the same text.

--parent DIR: a built checkout of the parent commit; bench.py --gpus 1 --steps S --warmup W in fresh child processes, K pairs, alternating, as
tools/bench_gvcf.py does.
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), reps=int(a.size))


def writers(args):
    import numpy as np
    import torch
    from nanocaller_amd import gvcf, vcfio
    from nanocaller_amd.engine import get_engine
    from nanocaller_amd.synth_device import make_device_workload
    from nanocaller_amd.utils import get_chunks
    eng = get_engine(0)
    L = args.length
    pack, info = make_device_workload(eng, L, depth=30.0, tech="ont", seed=4811)
    spans = [(c["start"], c["end"]) for c in get_chunks([("chr20", 1, L, "diploid")], cpu=16)]
    cfg = gvcf.settings({})
    held = eng.refconf_columns(pack)
    pos = np.arange(args.variant_every, L - 1, args.variant_every, dtype=np.int64)
    vtext = "".join("chr20\t%d\t.\tA\tG\t31.25\tPASS\tPR=0.01,0.02,0.96,0.01;FQ=0.4375\tGT:DP:FQ\t0/1:32:0.4375\n" % p for p in pos.tolist()).encode()
    tmp = tempfile.mkdtemp(prefix="gvcf_write_", dir=args.tmp)
    out = {"workload": "chr20-sized synthetic ONT 30x contig (bench.py's), %d bp, pack resident in HBM, one variant line every %d columns" % (L, args.variant_every),
           "variant_lines": int(pos.size)}
    plain, pieces = os.path.join(tmp, "t.1.snps.g.vcf"), os.path.join(tmp, "t.1.snps.g.vcf.bgzf")
    host_gz, dev_gz = os.path.join(tmp, "host.g.vcf.gz"), os.path.join(tmp, "dev.g.vcf.gz")

    def host_span1():
        text, off, start = gvcf.group_blocks(eng, held, "chr20", False, spans, pos, cfg)
        with open(plain, "wb") as f:
            for piece in gvcf.splice(text, off, start, vtext, pos):
                f.write(piece)
        return int(off.size - 1 + pos.size)

    def device_span1():
        with gvcf.PieceFile(pieces) as pf:
            made = gvcf.group_pieces(eng, pf, held, "chr20", False, spans, vtext, pos, cfg, slab_members=args.slab_members)
        return pf, made

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    t = {k: [] for k in ("host_span1", "host_span2", "device_span1", "device_span2")}
    stage = {}
    lines = None
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        lines, ms = clock(host_span1)
        do_merge = lines <= args.host_merge_lines
        if keep:
            t["host_span1"].append(ms)
        if do_merge:
            _, ms = clock(lambda: gvcf.merge_worker_files([plain], host_gz, ["chr20"], "S"))
            if keep:
                t["host_span2"].append(ms)
        (pf, made), ms = clock(device_span1)
        if keep:
            t["device_span1"].append(ms)
            for k, v in pf.ms.items():
                stage.setdefault(k, []).append(v)
        n_dev, ms = clock(lambda: gvcf.merge_pieces([pieces], dev_gz, ["chr20"], "S"))
        if keep:
            t["device_span2"].append(ms)
        print("pass %d of %d: %d lines" % (i + 1, args.warmup + args.reps, lines), {k: round(v[-1]) for k, v in t.items() if v}, file=sys.stderr, flush=True)
        out.update(lines=lines, device_lines=int(n_dev), pieces=len(made), members=int(sum(p["members"] for p in made)),
                   text_bytes=int(sum(p["text_bytes"] for p in made)), piece_bytes=int(sum(p["bytes"] for p in made)),
                   plain_file_bytes=os.path.getsize(plain), device_file_bytes=os.path.getsize(dev_gz))
    # the two writers wrote the same lines
    body = gzip.open(dev_gz, "rb").read()
    body = body[body.index(b"\n#CHROM") + 1:]
    body = body[body.index(b"\n") + 1:]
    if t["host_span2"]:
        want = gzip.open(host_gz, "rb").read()
        out["device_file_equals"] = "the host writer's merged file, inflated"
        assert want.endswith(body) and len(want) - len(body) == len(gvcf.header(["chr20"], "S").encode())
        out["host_file_bytes"] = os.path.getsize(host_gz)
    else:
        out["device_file_equals"] = "the host writer's plain worker file (the Python merge was not run at %d lines)" % lines
        assert open(plain, "rb").read() == body
    assert lines == out["device_lines"]
    for k, v in t.items():
        out[k] = stats(v) if v else None
    out["device_stages"] = {k: stats(v) for k, v in sorted(stage.items())}
    # the merge kernel alone, beside a copy of the same bytes inside HBM
    blocks = eng.refconf_blocks(held[0], held[2], spans, np.stack([pos, pos], 1).astype(np.int32), error=cfg["error"], bands=cfg["bands"], device_out=True)
    text, off = eng.refconf_text(blocks, held[1], held[2], "chr20", error=cfg["error"], device_out=True)
    beg = blocks[:, 0].to(torch.int64) - 1
    a = (text, off, beg, beg, blocks[:, 1].to(torch.int64))
    voff, ref_len = gvcf.variant_lines(np.frombuffer(vtext, np.uint8))
    b = tuple(torch.from_numpy(np.array(x)).to(eng.device) for x in (np.frombuffer(vtext, np.uint8), voff, pos - 1, pos - 1, pos - 1 + ref_len))
    mk, cp = [], []
    for i in range(args.warmup + args.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        m = eng.lines_merge(a, b)
        e[1].record()
        dst = torch.empty_like(m[0])
        e[2].record()
        dst.copy_(m[0])
        e[3].record()
        e[3].synchronize()
        if i >= args.warmup:
            mk.append(e[0].elapsed_time(e[1]))
            cp.append(e[2].elapsed_time(e[3]))
        nbytes = int(m[0].numel())
        if i + 1 < args.warmup + args.reps:
            del m, dst
    out["merge_call"] = dict(stats(mk), bytes=nbytes, gb_per_s=nbytes / 1e6 / float(np.median(mk)),
                             what="Engine.lines_merge: allocation, both kernels and the wait for the status, by events")
    out["hbm_copy"] = dict(stats(cp), bytes=nbytes, gb_per_s=nbytes / 1e6 / float(np.median(cp)), what="Tensor.copy_ of the merged text, device to device")
    t0 = time.perf_counter()
    comp, _ = vcfio.bgzf_compress(m[0].cpu().numpy())
    out["host_compressor"] = dict(bytes=int(comp.size), ms=(time.perf_counter() - t0) * 1e3, what="nc_bgzf_compress level 6 on the merged text (with its EOF block)")
    out["device_over_host_compressed_size"] = out["piece_bytes"] / float(comp.size)
    for fn in os.listdir(tmp):
        os.unlink(os.path.join(tmp, fn))
    os.rmdir(tmp)
    return out


def headline(tree, args):
    env = dict(os.environ, PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("NC_GVCF", None)
    env.pop("NC_GVCF_WRITER", None)
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.bench_warmup)],
                       env=env, cwd=tree, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    if p.returncode != 0:
        raise SystemExit("bench.py (%s) failed with status %d" % (tree, p.returncode))
    return float(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])["value"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent", help="a built checkout of the parent commit (bench.py's headline is measured on both builds)")
    ap.add_argument("--pairs", type=int, default=3, help="with --parent: pairs of bench.py processes (parent, this build), alternating")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--length", type=int, default=64_444_167)
    ap.add_argument("--variant-every", type=int, default=1000)
    ap.add_argument("--host-merge-lines", type=int, default=6_000_000, help="the host writer's Python merge is run up to this many lines")
    ap.add_argument("--slab-members", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=1000)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gvcf_write.json"))
    ap.add_argument("--headline-only", action="store_true", help="with --parent: keep the writers' figures --out already holds and add the headline to them")
    ap.add_argument("--writers-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.writers_child:
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(writers(args)), flush=True)
        return
    if args.headline_only:
        with open(args.out) as f:
            res = json.load(f)
    else:
        # the writers in a child of their own: one process holds the GPU at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--writers-child"]
        for k in ("length", "variant_every", "host_merge_lines", "slab_members", "reps", "warmup"):
            cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
        if args.tmp:
            cmd += ["--tmp", args.tmp]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
        if p.returncode != 0:
            raise SystemExit("the writers' child failed with status %d" % p.returncode)
        res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    if args.parent:
        by = {"parent": [], "this": []}
        for _ in range(args.pairs):
            by["parent"].append(headline(os.path.abspath(args.parent), args))
            by["this"].append(headline(ROOT, args))
            print("headline so far", by, file=sys.stderr, flush=True)
        res["headline_by_process"] = dict(by, what="bench.py --gpus 1 --steps %d --warmup %d, sites/s of each process in the order run, gvcf off" % (args.steps, args.bench_warmup))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The pure-Python restatement of indel sites (oracle.indel_site_ref, band=True) on a few worker processes.

Workers are started by `spawn` and import this module, which imports numpy and the oracle only: they never open the GPU.
A task carries its site's records and the reference window, not the whole contig."""
import multiprocessing
import os

from oracle import oracle

MAX_WORKERS = 8


def site_task(p, recs, hap, ps, ref, window_after, mincov, maxcov, haploid=False, band=True, scoring=None):
    """the arguments of one site_ref call: `ref` is the contig's reference (1-based positions as a string's offsets + 1); only the window
    of the site travels"""
    end = min(len(ref), p + window_after + 1)
    return (p, recs, [int(v) for v in hap], [int(v) for v in ps], p - 1, ref[p - 1:end], window_after, mincov, maxcov, haploid, band) + (
        (tuple(scoring),) if scoring is not None else ())


def site_ref(task):
    """-> None when the site fails the oracle's set-size tests, else dict: x, cns, win, phase, and per alignment of the star alignment
    (set by set, as indel_site_ref aligns them): record index, window length, how it was aligned (32 / 64 / 'width' / 'edge') and the band
    (lo, B) or None its CIGAR gives"""
    p, recs, hap, ps, off, piece, window_after, mincov, maxcov, haploid, band = task[:11]
    kw = dict(scoring=task[11]) if len(task) > 11 else {}                 # (the star alignment's scoring; default: oracle.indel_site_ref's own)
    ref = "N" * off + piece
    how, reads = [], []
    got = oracle.indel_site_ref(recs, hap, ps, ref, p, window_after, mincov, maxcov, haploid=haploid, band=band, how_out=how, reads_out=reads, **kw)
    if got is None:
        return None
    x, cns, win, phase = got
    bands = [oracle.band_of(*oracle.window_band_ref(recs[k], p, window_after), n1, len(win)) for k, n1 in reads] if band else []
    return dict(x=x, cns=cns, win=win, phase=phase, reads=reads, how=how, bands=bands)


def map_sites(tasks):
    """site_ref over the tasks, in order, on min(8, usable CPUs) spawned workers (in this process for a handful of tasks)"""
    tasks = list(tasks)
    n = min(MAX_WORKERS, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count() or 1, len(tasks))
    if n <= 1 or len(tasks) < 4:
        return [site_ref(t) for t in tasks]
    with multiprocessing.get_context("spawn").Pool(n) as pool:
        return pool.map(site_ref, tasks, chunksize=1)

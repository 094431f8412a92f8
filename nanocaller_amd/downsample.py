"""Which reads a pileup deeper than maxcov keeps: the seeded uniform sample of `downsample='uniform'`, in numpy.

The rule (include/nanocaller_hip.h, nc_set_downsample).  For the pileup at the 1-based column `pos`, a set id (0: the SNP
pileup and the indel caller's `all` set, haploid included; 1: the HP 1 set; 2: the HP 2 set), its n entries in pack (= file) order and k = maxcov:

    base   = mix32(pos, seed ^ SETC[set_id])
    key(j) = mix32(j, base)                      0 <= j < n

With n <= k every entry is taken; otherwise the sample is the k entries of the smallest keys, kept in pileup order.  For a fixed seed mix32 is a
bijection of its first argument, so the keys of distinct j differ and the sample is well defined.  The device draws the same sample inside the
featurisers and the indel plan; this module is for users who want to know which reads a site saw, and for the tools.
"""
import os

import numpy as np

SETC = (0x00000000, 0x68E31DA4, 0xB5297A4D)
DEFAULT_SEED = 812            # the number the reference meant to seed its sampler with
MODES = {'first': 0, 'uniform': 1}


def mix32(p, seed):
    """the 32-bit mixer of csrc/nc_sample.h on an int or an array of ints `p` (taken modulo 2^32) -> uint32 of the same shape"""
    with np.errstate(over='ignore'):
        x = (np.asarray(p).astype(np.int64) & 0xffffffff).astype(np.uint32) * np.uint32(0x9E3779B1) ^ np.uint32(int(seed) & 0xffffffff)
        x = (x ^ (x >> np.uint32(16))) * np.uint32(0x85EBCA6B)
        x = (x ^ (x >> np.uint32(13))) * np.uint32(0xC2B2AE35)
        return x ^ (x >> np.uint32(16))


def sample_keys(seed, pos, set_id, n):
    """key(0 .. n - 1) of the pileup at `pos` for the set `set_id`"""
    base = int(mix32(int(pos), (int(seed) ^ SETC[set_id]) & 0xffffffff))
    return mix32(np.arange(int(n), dtype=np.int64), base)


def sample_indices(seed, pos, set_id, n, k):
    """ordinals (ascending, int64) of the entries that the pileup of n entries at the 1-based column `pos` keeps for the set `set_id` at maxcov = k"""
    if set_id not in (0, 1, 2):
        raise ValueError("set_id is 0 (SNP pileup / all), 1 (HP 1) or 2 (HP 2), not %r" % (set_id,))
    n, k = int(n), int(k)
    if k < 1 or n < 0:
        raise ValueError("sample_indices needs n >= 0 and k >= 1")
    if n <= k:
        return np.arange(n, dtype=np.int64)
    keys = sample_keys(seed, pos, set_id, n)
    return np.sort(np.argpartition(keys, k - 1)[:k]).astype(np.int64)


def resolve(params):
    """(mode, seed) of a caller's params: the keys 'downsample' ('first' | 'uniform') and 'downsample_seed', else NC_DOWNSAMPLE / NC_DOWNSAMPLE_SEED,
    else ('first', 812).  ValueError for anything else: the option is never ignored."""
    params = params or {}
    mode = params.get('downsample')
    if mode is None:
        mode = os.environ.get('NC_DOWNSAMPLE') or 'first'
    if mode not in MODES:
        raise ValueError("downsample must be 'first' or 'uniform', not %r" % (mode,))
    seed = params.get('downsample_seed')
    if seed is None:
        env = os.environ.get('NC_DOWNSAMPLE_SEED')
        seed = int(env) if env not in (None, '') else DEFAULT_SEED
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("downsample_seed must be an int, not %r" % (seed,))
    return mode, int(seed) & 0xffffffff


def for_pack(params, mates, chrom):
    """what Engine.snp_featurize(downsample=) / indel_sites_device(downsample=) take for these params: None ('first': nothing is set, every launch
    is the plain one) or (mode, seed).  `mates`: the pack's shared-names table or None; 'uniform' has no form that keys alignments by name."""
    mode, seed = resolve(params)
    if mode == 'first':
        return None
    if mates is not None:
        raise ValueError("downsample='uniform' is not available on a contig whose kept alignments share read names (%s)" % chrom)
    return mode, seed


def refuse_uniform(params, what):
    """the routes that have no uniform sample raise where the option asks for one"""
    if resolve(params)[0] == 'uniform':
        raise ValueError("downsample='uniform' is not available with %s" % what)

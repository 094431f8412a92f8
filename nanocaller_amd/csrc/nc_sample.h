// Seeded sampling on the device (gfx950): the 32-bit mixer of the scan's background sampling, and the uniform sample without replacement that the
// featurisers and the indel plan draw above maxcov (nc_set_downsample).
//
// The rule.  For the pileup at the 1-based column v, a set id s (0: the SNP pileup and the indel caller's `all` set, 1: HP 1, 2: HP 2) and k = maxcov:
//     base   = mix32(v, seed ^ NC_SAMPLE_SETC[s])
//     key(j) = mix32(j, base)            j = the entry's ordinal in the pileup (pack order = file order), 0 <= j < n
// and for n > k the sample is the k entries of the smallest keys, in pileup order.  For a fixed seed mix32 is a bijection of its first argument (an odd
// multiply, an xor with a constant, two xorshift-multiply rounds, an xorshift), so the keys of distinct ordinals differ and there are no ties: exactly k
// keys are <= the k-th smallest, which is all a kernel has to know (nc_sample_threshold).
#pragma once
#include "nc_common.h"

// a function of the 1-based position (or the ordinal) and the seed alone (DESIGN.md sections 20 and 23)
__device__ __forceinline__ uint32_t mix32(int32_t p, uint32_t seed)
{
    uint32_t x = ((uint32_t)p * 0x9E3779B1u) ^ seed;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t nc_sample_base(int32_t v, uint32_t seed, int set)
{
    return mix32(v, seed ^ (set == 0 ? 0x00000000u : set == 1 ? 0x68E31DA4u : 0xB5297A4Du));
}

// The k-th smallest (1 <= k <= n) of key(0 .. n - 1), from (base, n, k) alone: no global memory is read.  One wave; every lane calls it with the same
// arguments and gets the same value (the workgroup holds at most four waves, each with a histogram of its own).  A radix select, most significant byte
// first: lanes as ordinals, 64 a step, count the keys that agree with the bytes fixed so far into 256 bins of LDS; lane L then holds bins 4 L .. 4 L + 3,
// an inclusive scan of the lanes' sums finds the lane and a walk over its four bins the bin that holds rank k.  Four rounds of n / 64 steps.
__device__ __forceinline__ uint32_t nc_sample_threshold(uint32_t base, int n, int k)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[4][256];
    uint32_t *hist = hist_all[(threadIdx.x >> 6) & 3];
    const int lane = threadIdx.x & 63;
    uint32_t prefix = 0, mask = 0;
    int rank = k;                                                    // 1-based rank among the keys that agree with `prefix` under `mask`
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        *reinterpret_cast<uint4 *>(hist + 4 * lane) = make_uint4(0u, 0u, 0u, 0u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const uint32_t key = mix32(j, base);
            if (j < n && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint4 c = *reinterpret_cast<const uint4 *>(hist + 4 * lane);
        const int sum = (int)(c.x + c.y + c.z + c.w);
        const int incl = nc_wave_incl_scan(sum);
        // the first lane whose inclusive count reaches the rank holds the bin (the last lane's count is that of all keys in play, >= rank)
        const int L = __builtin_ctzll(__ballot(incl >= rank) | (1ull << 63));
        int below = incl - sum, bin = 4 * lane;
        if (below + (int)c.x < rank) { below += (int)c.x; bin++;
            if (below + (int)c.y < rank) { below += (int)c.y; bin++;
                if (below + (int)c.z < rank) { below += (int)c.z; bin++; } } }
        bin = __shfl(bin, L, 64);
        below = __shfl(below, L, 64);
        prefix |= (uint32_t)bin << shift;
        mask |= 255u << shift;
        rank -= below;
        __builtin_amdgcn_wave_barrier();                             // (every lane has read its bins before the next round clears them)
    }
    return prefix;
}

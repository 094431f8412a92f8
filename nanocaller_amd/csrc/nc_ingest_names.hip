// Read names on the device: which kept alignments of a contig share a read name, from the inflated record stream in HBM (nc_ingest.hip has
// the records' offsets and a 64-bit hash of every name).  The reference keys a column's pileup, the strand table and the neighbour lookups
// by NAME (generate_SNP_pileups.py:141-143,175,185,223,232); the host route groups the decoded names (nc_decoded_name_groups, nc_bam.cpp).
// Here the host, which holds the hashes, hands over the alignments whose hash occurs more than once, sorted by (hash, file order):
//   k_name_confirm   one wave per run of equal hashes (the wave of a run's first candidate; the others leave at once).  Lanes take the
//                    members; the run is walked in file order, and every name that has not occurred before in the run (a "leader") is
//                    compared by the later members that have found no equal yet -- length first, then the bytes, dword-wise.  Equal hashes
//                    alone never merge two names: a collision splits the run into several groups.
#include "nc_common.h"

namespace {

constexpr int WPB = 4;                                                 // waves (candidates) per workgroup

// len bytes at a and at b (both anywhere inside the stream: records are packed, nothing is aligned).  a's dwords are read aligned; b's are
// too when it sits on the same byte of its dword, else two aligned dwords of b are shifted together -- never a byte outside [b - 3, b + len).
__device__ __forceinline__ bool names_equal(const uint8_t *a, const uint8_t *b, int len)
{
    int t = 0;
    const int head = min(len, (int)((4 - ((uintptr_t)a & 3)) & 3));
    for (; t < head; t++)
        if (a[t] != b[t]) return false;
    const int d = (int)((uintptr_t)(b + t) & 3);
    if (d == 0) {
        for (; t + 4 <= len; t += 4)
            if (*(const uint32_t *)(a + t) != *(const uint32_t *)(b + t)) return false;
    } else if (t + 8 <= len) {
        const uint32_t *bw = (const uint32_t *)(b + t - d);
        uint32_t lo = *bw;
        for (; t + 8 <= len; t += 4) {                                 // (the second dword ends at b + t + 7 - d: inside the name)
            const uint32_t hi = *++bw;
            if (*(const uint32_t *)(a + t) != ((lo >> (8 * d)) | (hi << (32 - 8 * d)))) return false;
            lo = hi;
        }
    }
    for (; t < len; t++)
        if (a[t] != b[t]) return false;
    return true;
}

// the name of candidate i: -> its length without the NUL (l_read_name - 1), *name = its first byte; -1 (and a status bit) when the record
// does not lie inside the stream
__device__ __forceinline__ int name_of(const uint8_t *raw, int64_t raw_len, const int64_t *rec_off, int64_t i, const uint8_t **name, int32_t *status)
{
    const int64_t o = rec_off[i];
    int len = -1;
    if (o >= 0 && o <= raw_len - 36) {
        const uint8_t *p = raw + o;
        const int64_t bs = (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        const int l_name = p[12];
        if (l_name >= 1 && bs >= 32 + l_name && o + 4 + bs <= raw_len) len = l_name - 1;
    }
    if (len < 0) atomicOr(status, 1);
    *name = raw + (len < 0 ? 0 : o + 36);
    return len;
}

__global__ __launch_bounds__(64 * WPB) void k_name_confirm(const uint8_t *raw, int64_t raw_len, int64_t n_cand, const int64_t *rec_off, const uint64_t *hash,
                                                           int32_t *gid, int32_t *status)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);  // the run's first candidate
    if (s >= n_cand) return;
    const uint64_t h = hash[s];
    if (s > 0 && hash[s - 1] == h) return;                             // inside a run: its first candidate's wave has it
    int64_t e = s + 1;                                                 // the run's end
    for (;;) {
        const int64_t i = e + lane;
        const uint64_t m = __ballot(i < n_cand && hash[i] == h);
        const int c = m == ~0ull ? 64 : __builtin_ctzll(~m);
        e += c;
        if (c < 64) break;
    }
    const int64_t n = e - s;
    // 64 members at a time.  gid of a member: -1 while it is a leader nobody equals, its own index once somebody does, else the leader's index.
    // Leaders of finished tiles are read back from gid (written by this wave: fenced, and read past the vector cache).
#pragma unroll 1
    for (int64_t t0 = 0; t0 < n; t0 += 64) {
        const int64_t j = s + t0 + lane;
        const bool act = t0 + lane < n;
        const uint8_t *nm = raw;
        const int len = act ? name_of(raw, raw_len, rec_off, j, &nm, status) : -1;
        int32_t mine = -1;
        bool shared = false;
#pragma unroll 1
        for (int64_t u0 = 0; u0 < t0; u0 += 64) {                       // the leaders of the tiles before this one
            const int64_t k = s + u0 + lane;
            const int32_t g = __hip_atomic_load(gid + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint8_t *knm = raw;
            const int klen = name_of(raw, raw_len, rec_off, k, &knm, status);
            uint64_t lead = __ballot(klen >= 0 && (g == -1 || g == (int32_t)k));
#pragma unroll 1
            while (lead) {
                const int q = __builtin_ctzll(lead);
                lead &= lead - 1;
                const int qlen = __shfl(klen, q);
                const uint8_t *qnm = raw + __shfl((long long)(knm - raw), q);
                if (act && mine < 0 && len == qlen && names_equal(nm, qnm, len)) {
                    mine = (int32_t)(s + u0 + q);
                    gid[mine] = mine;                                  // (every lane that finds this leader stores the same value)
                }
            }
        }
        const int tile_n = n - t0 < 64 ? (int)(n - t0) : 64;
#pragma unroll 1
        for (int q = 0; q + 1 < tile_n; q++) {                         // this tile, in file order
            const int qlen = __shfl(len, q);
            const bool is_lead = __shfl(mine, q) < 0 && qlen >= 0;
            if (!is_lead) continue;
            const uint8_t *qnm = raw + __shfl((long long)(nm - raw), q);
            const bool hit = act && lane > q && mine < 0 && len == qlen && names_equal(nm, qnm, len);
            if (hit) mine = (int32_t)(s + t0 + q);
            if (__ballot(hit) && lane == q) shared = true;
        }
        if (act) gid[j] = mine >= 0 ? mine : shared ? (int32_t)j : -1;
        if (t0 + 64 < n) __threadfence();
    }
}

}   // namespace

extern "C" {

// gid[i] = the first candidate (file order) whose read name equals candidate i's, -1 when no other candidate carries it -- see the header.
// Runs on the context's OWN stream and waits for it: a thread that prepares the next contig calls this while another one enqueues on
// ctx->stream, so nothing of the launch stream is touched (or waited for).  The inputs must be complete when the call is made.
int nc_bam_name_groups(nc_ctx *ctx, const uint8_t *d_raw, int64_t raw_len, int64_t n_cand, const int64_t *d_rec_off, const uint64_t *d_hash, int32_t *d_gid,
                       int32_t *d_status)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_cand < 0 || n_cand > INT32_MAX - 64 || raw_len < 0 || (n_cand && (!d_raw || !d_rec_off || !d_hash || !d_gid || !d_status)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_bam_name_groups: bad argument");
    if (n_cand == 0) return NC_OK;                                     // no candidates: no launch
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->own_stream;
    NC_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_name_confirm, dim3((unsigned)((n_cand + WPB - 1) / WPB)), dim3(64 * WPB), 0, st, d_raw, raw_len, n_cand, d_rec_off, d_hash, d_gid, d_status);
    NC_HIP(ctx, hipGetLastError());
    int32_t bad = 0;
    NC_HIP(ctx, hipMemcpyAsync(&bad, d_status, sizeof bad, hipMemcpyDeviceToHost, st));
    NC_HIP(ctx, hipStreamSynchronize(st));
    if (bad) return NC_ERR_ARG;                                        // (no message: ctx->err belongs to the launching thread)
    return NC_OK;
}

}   // extern "C"

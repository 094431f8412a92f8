// Indexing a BAM on the device: the record boundaries of an inflated record stream WITHOUT chain starts, and the fields a .bai / .csi is
// assembled from (device_bam.build_index; DESIGN.md section 6 "Indexing an unindexed BAM").
//
// A record only says where the next one starts.  nc_bam_walk (nc_ingest.hip) cuts that chain at the entries of an index; with no index
// there is one start and one lane.  Here the chain is found by speculation that is then proved:
//   k_candidates  every byte position of the piece is tested for a plausible record header (block_size, refID and pos against the header's
//                 reference list, l_read_name and its NUL, next_refID, the field lengths against block_size; the record whole inside the
//                 piece).  The first two fields are tested from a tile in LDS -- they reject all but a few positions in a million -- the
//                 rest from global memory.  One bit per position, one 64-bit word per wave ballot.
//   k_links       the candidates in order (ranks of the bitmap), and for each the candidate its block_size leads to, or "none".
//   k_round       reachability from the first record by pointer doubling: in round k every marked candidate marks the one 2^k links on and
//                 every link is replaced by two links.  log2(candidates) launches instead of one dependent load per record.
//   k_collect     the marked candidates in order: the record offsets.
//   k_verify      the proof, one lane per record: out[0] is the given first record, out[i] + 4 + block_size(out[i]) == out[i + 1], and
//                 the last successor is where the chain leaves the piece (no whole record starts there).  Links are only ever followed from
//                 the first record, so what is marked IS on the serial chain; what the proof adds is that nothing of it is missing: a
//                 legal record the predicate does not accept (a pos beyond its reference's length, a next_refID outside the header) ends
//                 the speculative chain early.  Then, and only then, k_serial walks the piece as nc_bam_walk's one lane would.
//   k_index_fields  per record: virtual offsets of its first byte and of the byte behind it (binary search in the member table), the
//                 0-based span htslib indexes it under, its bin, and the coordinate order against the record before it.
// Every offset is compared with the piece's length before it is read.
#include "nc_common.h"

namespace {

__device__ __forceinline__ uint32_t ldu32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
__device__ __forceinline__ int32_t ld32(const uint8_t *p) { return (int32_t)ldu32(p); }

constexpr int TILE = 4096;                                             // positions per workgroup of 256 lanes (64 bitmap words)
constexpr int HALO = 16;                                               // the LDS test reads 8 bytes from a position

// the whole test, from global memory.  A record that is not whole inside [0, len) is no candidate: the chain leaves the piece there.
__device__ bool plausible(const uint8_t *raw, int64_t len, int64_t p, int32_t n_ref, const int32_t *ref_len)
{
    if (p + 36 > len) return false;
    const uint8_t *r = raw + p;
    const int32_t bs = ld32(r);
    if (bs < 32 || p + 4 + (int64_t)bs > len) return false;
    const int32_t refid = ld32(r + 4), pos = ld32(r + 8);
    if (refid < -1 || refid >= n_ref || pos < -1) return false;
    if (refid >= 0 && pos >= ref_len[refid]) return false;
    const int l_name = r[12], n_cig = r[16] | (r[17] << 8);
    const int32_t l_seq = ld32(r + 20), next_ref = ld32(r + 24), next_pos = ld32(r + 28);
    if (l_name < 1 || l_seq < 0 || next_ref < -1 || next_ref >= n_ref || next_pos < -1) return false;
    if (32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + l_seq > bs) return false;
    return r[36 + l_name - 1] == 0;                                    // (inside block_size, hence inside the piece)
}

__global__ __launch_bounds__(256) void k_candidates(const uint8_t *raw, int64_t len, int64_t readable, int32_t n_ref, const int32_t *ref_len,
                                                    uint64_t *words, int32_t *cnt)
{
    __shared__ uint32_t s[(TILE + HALO) / 4];
    const int64_t base = (int64_t)blockIdx.x * TILE;
    const int t = threadIdx.x;
    {   // the tile, 16 bytes per lane; bytes behind `readable` are not touched (zeros: a block_size of 0 is no candidate)
        uint4 v = make_uint4(0, 0, 0, 0);
        const int64_t o = base + 16 * (int64_t)t;
        if (o + 16 <= readable) v = *reinterpret_cast<const uint4 *>(raw + o);
        s[4 * t] = v.x; s[4 * t + 1] = v.y; s[4 * t + 2] = v.z; s[4 * t + 3] = v.w;
        if (t < HALO / 4) {
            const int64_t h = base + TILE + 4 * (int64_t)t;
            s[TILE / 4 + t] = h + 4 <= readable ? *reinterpret_cast<const uint32_t *>(raw + h) : 0u;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < TILE / 256; k++) {
        const int a = k * 256 + t;
        const int64_t p = base + a;
        const uint32_t w0 = s[a >> 2], w1 = s[(a >> 2) + 1], w2 = s[(a >> 2) + 2];
        const int32_t bs = (int32_t)__builtin_amdgcn_alignbyte(w1, w0, a & 3);
        const int32_t refid = (int32_t)__builtin_amdgcn_alignbyte(w2, w1, a & 3);
        bool ok = bs >= 32 && (uint32_t)(refid + 1) <= (uint32_t)n_ref && p + 36 <= len;
        if (ok) ok = plausible(raw, len, p, n_ref, ref_len);
        const uint64_t m = __ballot(ok);
        if ((t & 63) == 0) {
            const int64_t w = (base + k * 256 + (t & ~63)) >> 6;
            words[w] = m;
            cnt[w] = __popcll(m);
        }
    }
}

// candidate index of position q (a set bit), from the exclusive ranks of the words
__device__ __forceinline__ int32_t cand_index(const uint64_t *words, const int32_t *rank, int64_t q, uint64_t m)
{
    return rank[q >> 6] + __popcll(m & ((1ull << (q & 63)) - 1ull));
}

__global__ __launch_bounds__(256) void k_links(const uint8_t *raw, int64_t len, int64_t n_words, const uint64_t *words, const int32_t *rank, int32_t n_cand,
                                               int64_t *pos, int32_t *jump)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    uint64_t m = words[w];
    int32_t c = rank[w];
    while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const int64_t p = w * 64 + b;                                  // (a candidate: whole inside the piece)
        const int64_t q = p + 4 + (int64_t)ld32(raw + p);
        int32_t nxt = n_cand;
        if (q + 36 <= len) {
            const uint64_t mq = words[q >> 6];
            if ((mq >> (q & 63)) & 1) nxt = cand_index(words, rank, q, mq);
        }
        pos[c] = p;
        jump[c] = nxt;
        c++;
    }
}

__global__ void k_seed(int64_t len, int64_t first, const uint64_t *words, const int32_t *rank, int32_t n_cand, int32_t *jump_a, int32_t *jump_b,
                       int32_t *mark)
{
    jump_a[n_cand] = jump_b[n_cand] = n_cand;                          // "none" leads nowhere
    if (first >= 0 && first + 36 <= len) {
        const uint64_t m = words[first >> 6];
        if ((m >> (first & 63)) & 1) mark[cand_index(words, rank, first, m)] = 1;
    }
}

// One round of the doubling.  A mark another lane sets in this round may already be seen here: what it then marks lies further on the same
// chain, never off it.
__global__ __launch_bounds__(256) void k_round(int32_t n_cand, const int32_t *jump, int32_t *jump_next, int32_t *mark)
{
    const int32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cand) return;
    const int32_t j = jump[c];
    if (j < n_cand) {
        if (mark[c]) mark[j] = 1;
        jump_next[c] = jump[j];
    } else jump_next[c] = n_cand;
}

__global__ __launch_bounds__(256) void k_collect(int32_t n_cand, const int64_t *pos, const int32_t *mark, const int32_t *mark_rank, int64_t *out)
{
    const int32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c < n_cand && mark[c]) out[mark_rank[c] - 1] = pos[c];
}

// res[0]: bit 0 the proof failed, NC_BAMIDX_* status bits (valid when bit 0 is clear); res[1]: where the chain leaves the piece
__device__ void chain_exit(const uint8_t *raw, int64_t len, int64_t q, int32_t last, unsigned long long *res)
{
    res[1] = (unsigned long long)q;
    if (q + 4 <= len) {
        const int32_t bs = ld32(raw + q);
        if (bs < 32) atomicOr(res, (unsigned long long)NC_BAMIDX_BAD_BLOCK_SIZE);
        else if (q + 4 + (int64_t)bs <= len) atomicOr(res, 1ull);      // a whole record the speculation did not reach
        else if (last) atomicOr(res, (unsigned long long)NC_BAMIDX_TRUNCATED);
    } else if (last && q != len) atomicOr(res, (unsigned long long)NC_BAMIDX_TRUNCATED);
}

__global__ __launch_bounds__(256) void k_verify(const uint8_t *raw, int64_t len, int64_t first, int64_t n_rec, const int64_t *out, int32_t last,
                                                unsigned long long *res)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n_rec == 0) {
        if (i == 0) chain_exit(raw, len, first, last, res);
        return;
    }
    if (i >= n_rec) return;
    const int64_t p = out[i];
    bool bad = (i == 0 && p != first) || p < 0 || p + 36 > len;
    int64_t succ = 0;
    if (!bad) {
        const int32_t bs = ld32(raw + p);
        succ = p + 4 + (int64_t)bs;
        bad = bs < 32 || succ > len || (i + 1 < n_rec && out[i + 1] != succ);
    }
    if (bad) atomicOr(res, 1ull);
    else if (i + 1 == n_rec) chain_exit(raw, len, succ, last, res);
}

// the exact serial chain, one lane: res[0] status bits, res[1] where it leaves the piece, res[2] records
template <bool FILL>
__global__ void k_serial(const uint8_t *raw, int64_t len, int64_t first, int32_t last, int64_t *out, unsigned long long *res)
{
    int64_t p = first, n = 0;
    unsigned long long st = 0;
    while (p + 4 <= len) {
        const int32_t bs = ld32(raw + p);
        if (bs < 32) { st |= NC_BAMIDX_BAD_BLOCK_SIZE; break; }
        if (p + 4 + (int64_t)bs > len) break;
        if (FILL) out[n] = p;
        n++;
        p += 4 + (int64_t)bs;
    }
    if (last && p != len && !st) st |= NC_BAMIDX_TRUNCATED;
    res[0] = st;
    res[1] = (unsigned long long)p;
    res[2] = (unsigned long long)n;
}

// virtual offset (SAMv1 4.1.1) of stream offset x: a position at a member boundary belongs to the first member that starts there (an empty
// one included), as bgzf_tell gives it after a block has been read to its end.  ooff / foff have n_mem + 1 entries.
__device__ uint64_t voffset(int64_t x, int32_t n_mem, const int64_t *ooff, const int64_t *foff)
{
    int32_t lo = 0, hi = n_mem;                                        // first index with ooff[index] >= x (x <= ooff[n_mem])
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (ooff[mid] >= x) hi = mid;
        else lo = mid + 1;
    }
    if (ooff[lo] == x) return (uint64_t)foff[lo] << 16;
    return (uint64_t)foff[lo - 1] << 16 | (uint64_t)(x - ooff[lo - 1]);
}

__global__ __launch_bounds__(256) void k_index_fields(const uint8_t *raw, int64_t n_rec, const int64_t *rec_off, int64_t stream_base, const int32_t *meta,
                                                      int32_t n_ref, int32_t n_mem, const int64_t *ooff, const int64_t *foff, int32_t has_prev,
                                                      int32_t prev_refid, int32_t prev_pos, int32_t min_shift, int32_t depth, int64_t *voff,
                                                      int32_t *fields, int32_t *status)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const int32_t refid = meta[r], pos = meta[n_rec + r], flag = meta[2 * n_rec + r], rlen = meta[3 * n_rec + r];
    int32_t st = 0;
    if (refid < -1 || refid >= n_ref || pos < -1) st |= NC_BAMIDX_BAD_REFID;
    if (r > 0 || has_prev) {
        const int32_t qr = r > 0 ? meta[r - 1] : prev_refid, qp = r > 0 ? meta[n_rec + r - 1] : prev_pos;
        if ((uint32_t)qr > (uint32_t)refid || (qr == refid && refid >= 0 && qp > pos)) st |= NC_BAMIDX_UNSORTED;   // (-1, the unplaced, sorts last)
    }
    if (st) atomicOr(status, st);
    const int64_t g = stream_base + rec_off[r];
    const int64_t ge = g + 4 + (int64_t)ld32(raw + rec_off[r]);
    if (g < ooff[0] || ge > ooff[n_mem]) { atomicOr(status, NC_BAMIDX_BAD_MEMBERS); return; }
    voff[r] = (int64_t)voffset(g, n_mem, ooff, foff);
    voff[n_rec + r] = (int64_t)voffset(ge, n_mem, ooff, foff);
    // the span htslib indexes the record under (bam_endpos: one base for an unmapped or span-less record; [-1, 0) goes to [0, 1))
    int64_t beg = pos < 0 ? 0 : pos;
    int64_t end = (int64_t)pos + ((flag & 4) || rlen <= 0 ? 1 : rlen);
    if (end <= beg) end = beg + 1;
    int32_t bin = 0;
    {
        int s = min_shift;
        int64_t t = ((1ll << (depth * 3)) - 1) / 7;
        const int64_t e = end - 1;
        for (int lv = depth; lv > 0; lv--) {
            if (beg >> s == e >> s) { bin = (int32_t)(t + (beg >> s)); break; }
            s += 3;
            t -= 1ll << ((lv - 1) * 3);
        }
    }
    fields[r] = bin;
    fields[n_rec + r] = (int32_t)beg;
    fields[2 * n_rec + r] = (int32_t)end;
}

}   // namespace

extern "C" {

int nc_bamidx_candidates(nc_ctx *ctx, const uint8_t *d_raw, int64_t len, int64_t readable, int32_t n_ref, const int32_t *d_ref_len, uint64_t *d_words,
                         int32_t *d_cnt)
{
    if (!ctx) return NC_ERR_ARG;
    if (len < 0 || readable < len || n_ref < 0 || (n_ref && !d_ref_len) || (len && (!d_raw || !d_words || !d_cnt)) || ((uintptr_t)d_raw & 15))
        return nc_fail(ctx, NC_ERR_ARG, "nc_bamidx_candidates: bad argument (the stream must be 16-byte aligned)");
    if (len == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_candidates, dim3((unsigned)((len + TILE - 1) / TILE)), dim3(256), 0, ctx->stream, d_raw, len, readable, n_ref, d_ref_len, d_words,
                       d_cnt);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_bamidx_chain(nc_ctx *ctx, const uint8_t *d_raw, int64_t len, int64_t first, const uint64_t *d_words, const int32_t *d_rank, int32_t n_cand,
                    int64_t *d_pos, int32_t *d_jump, int32_t *d_mark)
{
    if (!ctx) return NC_ERR_ARG;
    if (len <= 0 || n_cand < 0 || first < 0 || !d_raw || !d_words || !d_rank || !d_pos || !d_jump || !d_mark)
        return nc_fail(ctx, NC_ERR_ARG, "nc_bamidx_chain: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n_words = (len + TILE - 1) / TILE * (TILE / 64);
    int32_t *ja = d_jump, *jb = d_jump + (n_cand + 1);
    NC_HIP(ctx, hipMemsetAsync(d_mark, 0, sizeof(int32_t) * ((size_t)n_cand + 1), ctx->stream));
    hipLaunchKernelGGL(k_links, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, ctx->stream, d_raw, len, n_words, d_words, d_rank, n_cand, d_pos, ja);
    hipLaunchKernelGGL(k_seed, dim3(1), dim3(1), 0, ctx->stream, len, first, d_words, d_rank, n_cand, ja, jb, d_mark);
    for (int64_t reach = 1; reach < n_cand; reach <<= 1) {             // after the round: every record fewer than 2 * reach links from the first
        hipLaunchKernelGGL(k_round, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, ctx->stream, n_cand, ja, jb, d_mark);
        int32_t *t = ja;
        ja = jb;
        jb = t;
    }
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_bamidx_collect(nc_ctx *ctx, int32_t n_cand, const int64_t *d_pos, const int32_t *d_mark, const int32_t *d_mark_rank, int64_t *d_out)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_cand < 0 || (n_cand && (!d_pos || !d_mark || !d_mark_rank || !d_out))) return nc_fail(ctx, NC_ERR_ARG, "nc_bamidx_collect: bad argument");
    if (n_cand == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_collect, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, ctx->stream, n_cand, d_pos, d_mark, d_mark_rank, d_out);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_bamidx_verify(nc_ctx *ctx, const uint8_t *d_raw, int64_t len, int64_t first, int64_t n_rec, const int64_t *d_out, int32_t last, int64_t *d_res)
{
    if (!ctx) return NC_ERR_ARG;
    if (len < 0 || first < 0 || n_rec < 0 || !d_res || (len && !d_raw) || (n_rec && !d_out)) return nc_fail(ctx, NC_ERR_ARG, "nc_bamidx_verify: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemsetAsync(d_res, 0, 3 * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(k_verify, dim3((unsigned)((n_rec + 255) / 256 + (n_rec == 0))), dim3(256), 0, ctx->stream, d_raw, len, first, n_rec, d_out, last,
                       reinterpret_cast<unsigned long long *>(d_res));
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_bamidx_serial(nc_ctx *ctx, const uint8_t *d_raw, int64_t len, int64_t first, int32_t last, int64_t *d_out, int64_t *d_res)
{
    if (!ctx) return NC_ERR_ARG;
    if (len < 0 || first < 0 || !d_res || (len && !d_raw)) return nc_fail(ctx, NC_ERR_ARG, "nc_bamidx_serial: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long *res = reinterpret_cast<unsigned long long *>(d_res);
    if (d_out) hipLaunchKernelGGL(k_serial<true>, dim3(1), dim3(1), 0, ctx->stream, d_raw, len, first, last, d_out, res);
    else hipLaunchKernelGGL(k_serial<false>, dim3(1), dim3(1), 0, ctx->stream, d_raw, len, first, last, d_out, res);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_bamidx_fields(nc_ctx *ctx, const uint8_t *d_raw, int64_t n_rec, const int64_t *d_rec_off, int64_t stream_base, const int32_t *d_meta, int32_t n_ref,
                     int32_t n_mem, const int64_t *d_mem_ooff, const int64_t *d_mem_foff, int32_t has_prev, int32_t prev_refid, int32_t prev_pos,
                     int32_t min_shift, int32_t depth, int64_t *d_voff, int32_t *d_fields, int32_t *d_status)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_rec < 0 || n_mem < 1 || min_shift < 1 || depth < 1 || min_shift + 3 * depth > 62 ||
        (n_rec && (!d_raw || !d_rec_off || !d_meta || !d_mem_ooff || !d_mem_foff || !d_voff || !d_fields || !d_status)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_bamidx_fields: bad argument");
    if (n_rec == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_index_fields, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, ctx->stream, d_raw, n_rec, d_rec_off, stream_base, d_meta, n_ref,
                       n_mem, d_mem_ooff, d_mem_foff, has_prev, prev_refid, prev_pos, min_shift, depth, d_voff, d_fields, d_status);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

}   // extern "C"

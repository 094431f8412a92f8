// Text lines on the device (gfx950): the stable merge of two position-sorted lists of lines, and a BGZF piece's share of a CSI index reduced to
// what the index stores.  The unit knows lines, keys and 0-based intervals, nothing of what the lines say; DESIGN.md section 22.
//
//   k_merge_rank   one lane per input line: its place in the merged list from a binary search in the OTHER list's keys (B's lines in front at
//                  equal keys), and with the place the merged byte offset = its own offset + the other list's offset at the searched rank.  No
//                  prefix sum and no atomics: every output word has one writer.
//   k_merge_copy   partitioned by OUTPUT bytes: a workgroup owns MG_SPAN bytes of the merged text, finds the lines of its span in the merged
//                  offsets and fills it in aligned 16-byte stores.  A 16-byte piece that lies in one line is five aligned dword loads funnelled
//                  by the source's misalignment; one that crosses a line end (or the text's end) is put together byte by byte.
//   k_idx_heads / k_idx_scan   head flags (a line whose bin differs from the line before it) and their prefix sum: every line's run.  The checks
//                  of the preconditions ride along (ends and begins ascend, the offsets fit the members).
//   k_idx_runs     the runs compacted in file order: bin, virtual offset of the first line's first byte and of the byte behind the last line.
//   k_idx_windows  one lane per 2^min_shift window: the first line whose end lies behind the window's start (binary search in the ascending
//                  ends) is the line with the smallest virtual offset that can overlap it; it does when it begins in front of the window's end.
#include "nc_common.h"

namespace {

constexpr int MG_THREADS = 256, MG_SPAN = 16384;              // output bytes per workgroup of k_merge_copy
constexpr int IX_THREADS = 256, IX_ITEMS = 16, IX_TILE = IX_THREADS * IX_ITEMS;
constexpr int64_t MEMBER = 0xff00;                            // uncompressed bytes of every member but a piece's last (BGZF_BLOCK)

struct Lines {
    const uint8_t *text;
    const int64_t *off, *key, *beg, *end;
    int64_t n;
};

// first index whose element is >= v (lower) or > v (upper)
__device__ __forceinline__ int64_t lower_bound(const int64_t *a, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (a[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

__device__ __forceinline__ int64_t upper_bound(const int64_t *a, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (a[m] <= v) lo = m + 1; else hi = m;
    }
    return lo;
}

// status words (int32 each, zeroed by the caller, written with plain stores of 1): 0 the offsets do not add up to out_bytes, 1 a list's offsets
// descend, 2 a list's keys descend
__global__ __launch_bounds__(256) void k_merge_rank(Lines A, Lines B, int64_t out_bytes, int64_t *__restrict__ out_off, int64_t *__restrict__ out_beg,
                                                    int64_t *__restrict__ out_end, int32_t *__restrict__ out_src, int32_t *__restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, n = A.n + B.n;
    if (t > n) return;
    const int64_t a0 = A.n ? A.off[0] : 0, b0 = B.n ? B.off[0] : 0;
    if (t == n) {
        const int64_t total = (A.n ? A.off[A.n] - a0 : 0) + (B.n ? B.off[B.n] - b0 : 0);
        out_off[n] = total;
        if (total != out_bytes) status[0] = 1;
        return;
    }
    const bool is_a = t < A.n;
    const Lines &S = is_a ? A : B;
    const int64_t i = is_a ? t : t - A.n;
    const int64_t key = S.key[i];
    if (S.off[i + 1] < S.off[i]) status[1] = 1;
    if (i && S.key[i - 1] > key) status[2] = 1;
    // A's line follows every B line whose key is <= its own; B's line follows every A line whose key is smaller
    const int64_t other = is_a ? upper_bound(B.key, B.n, key) : lower_bound(A.key, A.n, key);
    const int64_t r = i + other;
    const int64_t o_other = is_a ? (B.n ? B.off[other] - b0 : 0) : (A.n ? A.off[other] - a0 : 0);
    out_off[r] = S.off[i] - (is_a ? a0 : b0) + o_other;
    out_beg[r] = S.beg[i];
    out_end[r] = S.end[i];
    out_src[r] = (int32_t)t;
}

// 16 bytes from p (any alignment) as four dwords, read in aligned dwords
__device__ __forceinline__ uint4 load16(const uint8_t *p)
{
    const int sh = (int)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
    if (sh == 0) return make_uint4(d0, d1, d2, d3);
    const uint32_t d4 = q[4];                                  // (holds byte 16 - sh .. of the piece: inside the source)
    return make_uint4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh), __builtin_amdgcn_alignbyte(d3, d2, sh),
                      __builtin_amdgcn_alignbyte(d4, d3, sh));
}

__global__ __launch_bounds__(MG_THREADS) void k_merge_copy(Lines A, Lines B, int64_t total, const int64_t *__restrict__ out_off,
                                                           const int32_t *__restrict__ out_src, const int32_t *__restrict__ status,
                                                           uint8_t *__restrict__ out)
{
    if (status[0] | status[1] | status[2]) return;             // (the offsets cannot be trusted: nothing is read through them)
    const int64_t n = A.n + B.n;
    const int64_t s0 = (int64_t)blockIdx.x * MG_SPAN, s1 = min(total, s0 + MG_SPAN);
    // the lines that hold the span's first and last byte (an empty line shares its offset with the line behind it: the last of them holds the byte)
    const int64_t r_lo = upper_bound(out_off, n + 1, s0) - 1, r_hi = upper_bound(out_off, n + 1, s1 - 1) - 1;
    for (int64_t o = s0 + 16 * (int64_t)threadIdx.x; o < s1; o += 16 * MG_THREADS) {
        const int m = (int)min((int64_t)16, s1 - o);
        int64_t r = r_lo + upper_bound(out_off + r_lo, r_hi - r_lo + 1, o) - 1;
        int32_t s = out_src[r];
        const uint8_t *src = (s < A.n ? A.text + A.off[s] : B.text + B.off[s - A.n]) - out_off[r];      // + merged offset = the byte
        int64_t line_end = out_off[r + 1];
        if (m == 16 && o + 16 <= line_end) {
            *reinterpret_cast<uint4 *>(out + o) = load16(src + o);
            continue;
        }
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < m) {
                const int64_t pos = o + k;
                while (pos >= line_end && r < n - 1) {
                    r++;
                    s = out_src[r];
                    src = (s < A.n ? A.text + A.off[s] : B.text + B.off[s - A.n]) - out_off[r];
                    line_end = out_off[r + 1];
                }
                w[k >> 2] |= (uint32_t)src[pos] << (8 * (k & 3));
            }
        }
        if (m == 16) {
            *reinterpret_cast<uint4 *>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int k = 0; k < m; k++) out[o + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the index of a piece
// hts_reg2bin of the 0-based half-open [beg, end)
__device__ __forceinline__ int32_t reg2bin(int64_t beg, int64_t end, int min_shift, int depth)
{
    end--;
    int s = min_shift;
    int64_t t = ((1ll << (depth * 3)) - 1) / 7;
    for (int l = depth; l > 0; l--) {
        if ((beg >> s) == (end >> s)) return (int32_t)(t + (beg >> s));
        s += 3;
        t -= 1ll << ((l - 1) * 3);
    }
    return 0;
}

// virtual offset, relative to the piece, of byte q of the piece's text: a byte on a member border is the next member's first
__device__ __forceinline__ uint64_t voff(int64_t q, const int64_t *__restrict__ foff)
{
    const int64_t m = q / MEMBER;
    return (uint64_t)foff[m] << 16 | (uint64_t)(q - m * MEMBER);
}

// work: [0, n) every line's inclusive head count inside its tile (k_idx_scan's sums make it the run), [n + 1, n + 1 + n_tiles) the tiles' sums,
// then four words: the number of runs, and three status words (ends descend, begins descend, an interval or an offset out of range)
__global__ __launch_bounds__(IX_THREADS) void k_idx_heads(int64_t n, const int64_t *__restrict__ beg, const int64_t *__restrict__ end,
                                                          const int64_t *__restrict__ line_off, int64_t u0, int64_t text_cap, int min_shift, int depth,
                                                          int32_t *__restrict__ work, int32_t *__restrict__ tile_sum, int32_t *__restrict__ tail)
{
    __shared__ int32_t sh[IX_THREADS];
    const int64_t i0 = (int64_t)blockIdx.x * IX_TILE + (int64_t)threadIdx.x * IX_ITEMS;
    uint32_t heads = 0;
    int32_t prev = (i0 > 0 && i0 < n) ? reg2bin(beg[i0 - 1], end[i0 - 1], min_shift, depth) : -1;
    for (int k = 0; k < IX_ITEMS; k++) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        const int64_t b = beg[i], e = end[i], q = line_off[i] - u0, q1 = line_off[i + 1] - u0;
        if (b < 0 || e <= b || q < 0 || q1 < q || q1 > text_cap) tail[3] = 1;
        if (i && end[i - 1] > e) tail[1] = 1;
        if (i && beg[i - 1] > b) tail[2] = 1;
        const int32_t bin = reg2bin(b, e, min_shift, depth);
        if (i == 0 || bin != prev) heads |= 1u << k;
        prev = bin;
    }
    const int32_t mine = __popc(heads);
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < IX_THREADS; d <<= 1) {                   // inclusive scan of the threads' counts
        const int32_t v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t c = sh[threadIdx.x] - mine;
    for (int k = 0; k < IX_ITEMS; k++) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        c += (heads >> k) & 1;
        work[i] = c;
    }
    if (threadIdx.x == IX_THREADS - 1) tile_sum[blockIdx.x] = sh[IX_THREADS - 1];
}

// exclusive prefix sums of the tiles' sums, in place; tail[0] = the total
__global__ __launch_bounds__(1024) void k_idx_scan(int32_t n_tiles, int32_t *__restrict__ tile_sum, int32_t *__restrict__ tail)
{
    __shared__ int32_t sh[1024];
    int32_t carry = 0;
    for (int32_t base = 0; base < n_tiles; base += 1024) {
        const int32_t i = base + threadIdx.x;
        const int32_t mine = i < n_tiles ? tile_sum[i] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int32_t v = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += v;
            __syncthreads();
        }
        if (i < n_tiles) tile_sum[i] = carry + sh[threadIdx.x] - mine;
        carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) tail[0] = carry;
}

__global__ __launch_bounds__(256) void k_idx_runs(int64_t n, const int64_t *__restrict__ beg, const int64_t *__restrict__ end,
                                                  const int64_t *__restrict__ line_off, int64_t u0, int32_t n_members, const int64_t *__restrict__ foff,
                                                  int min_shift, int depth, const int32_t *__restrict__ work, const int32_t *__restrict__ tile_pre,
                                                  int32_t n_runs, int32_t *__restrict__ run_bin, uint64_t *__restrict__ run_vbeg,
                                                  uint64_t *__restrict__ run_vend)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t r = work[i] + tile_pre[i / IX_TILE] - 1;
    if (r < 0 || r >= n_runs) return;
    const bool head = i == 0 || work[i - 1] + tile_pre[(i - 1) / IX_TILE] - 1 != r;
    const bool last = i == n - 1 || work[i + 1] + tile_pre[(i + 1) / IX_TILE] - 1 != r;
    if (head) {
        run_bin[r] = reg2bin(beg[i], end[i], min_shift, depth);
        run_vbeg[r] = voff(line_off[i] - u0, foff);
    }
    if (last) run_vend[r] = i == n - 1 ? (uint64_t)foff[n_members] << 16 : voff(line_off[i + 1] - u0, foff);
}

__global__ __launch_bounds__(256) void k_idx_windows(int64_t n, const int64_t *__restrict__ beg, const int64_t *__restrict__ end,
                                                     const int64_t *__restrict__ line_off, int64_t u0, const int64_t *__restrict__ foff, int min_shift,
                                                     int64_t w_first, int64_t n_win, uint64_t *__restrict__ win_min)
{
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_win) return;
    const int64_t lo = (w_first + w) << min_shift, hi = lo + (1ll << min_shift);
    const int64_t j = upper_bound(end, n, lo);                      // the first line that ends behind the window's first position
    win_min[w] = (j < n && beg[j] < hi) ? voff(line_off[j] - u0, foff) : ~0ull;
}

}   // namespace

extern "C" int nc_lines_merge(nc_ctx *ctx, int64_t na, const uint8_t *d_a_text, const int64_t *d_a_off, const int64_t *d_a_key, const int64_t *d_a_beg,
                              const int64_t *d_a_end, int64_t nb, const uint8_t *d_b_text, const int64_t *d_b_off, const int64_t *d_b_key,
                              const int64_t *d_b_beg, const int64_t *d_b_end, int64_t out_bytes, uint8_t *d_out_text, int64_t *d_out_off,
                              int64_t *d_out_beg, int64_t *d_out_end, int32_t *d_out_src, int32_t *d_status)
{
    if (!ctx) return NC_ERR_ARG;
    if (na < 0 || nb < 0 || na + nb > INT32_MAX || out_bytes < 0 || !d_out_off || !d_status ||
        (na && (!d_a_text || !d_a_off || !d_a_key || !d_a_beg || !d_a_end)) || (nb && (!d_b_text || !d_b_off || !d_b_key || !d_b_beg || !d_b_end)) ||
        ((na + nb) && (!d_out_beg || !d_out_end || !d_out_src)) || (out_bytes && !d_out_text) || ((uintptr_t)d_out_text & 15))
        return nc_fail(ctx, NC_ERR_ARG, "nc_lines_merge: bad argument (the merged text must be 16-byte aligned)");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const Lines A = {d_a_text, d_a_off, d_a_key, d_a_beg, d_a_end, na}, B = {d_b_text, d_b_off, d_b_key, d_b_beg, d_b_end, nb};
    const int64_t n = na + nb;
    hipLaunchKernelGGL(k_merge_rank, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, ctx->stream, A, B, out_bytes, d_out_off, d_out_beg, d_out_end,
                       d_out_src, d_status);
    NC_HIP(ctx, hipGetLastError());
    if (out_bytes) {
        if ((out_bytes + MG_SPAN - 1) / MG_SPAN > INT32_MAX) return nc_fail(ctx, NC_ERR_ARG, "nc_lines_merge: text too large");
        hipLaunchKernelGGL(k_merge_copy, dim3((unsigned)((out_bytes + MG_SPAN - 1) / MG_SPAN)), dim3(MG_THREADS), 0, ctx->stream, A, B, out_bytes,
                           (const int64_t *)d_out_off, (const int32_t *)d_out_src, (const int32_t *)d_status, d_out_text);
        NC_HIP(ctx, hipGetLastError());
    }
    return NC_OK;
}

extern "C" int nc_lines_index(nc_ctx *ctx, int64_t n, const int64_t *d_beg, const int64_t *d_end, const int64_t *d_line_off, int64_t u0,
                              int32_t n_members, const int64_t *d_foff, int32_t min_shift, int32_t depth, int32_t *d_work, int64_t *info_host,
                              int32_t *d_run_bin, uint64_t *d_run_vbeg, uint64_t *d_run_vend, uint64_t *d_win_min)
{
    if (!ctx) return NC_ERR_ARG;
    if (n < 0 || n > INT32_MAX || n_members < 0 || !info_host || min_shift < 1 || depth < 1 || depth > 8 || min_shift + 3 * depth > 48 ||
        (n && (!d_beg || !d_end || !d_line_off || !d_foff || !d_work || n_members < 1)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_lines_index: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t n_tiles = (int32_t)((n + IX_TILE - 1) / IX_TILE);
    int32_t *tile_sum = d_work + n + 1, *tail = tile_sum + n_tiles;
    if (!d_run_bin && !d_win_min) {                              // sizes
        info_host[0] = info_host[1] = info_host[2] = info_host[3] = 0;
        if (n == 0) return NC_OK;
        NC_HIP(ctx, hipMemsetAsync(tail, 0, 16, ctx->stream));
        hipLaunchKernelGGL(k_idx_heads, dim3(n_tiles), dim3(IX_THREADS), 0, ctx->stream, n, d_beg, d_end, d_line_off, u0, (int64_t)n_members * MEMBER,
                           min_shift, depth, d_work, tile_sum, tail);
        NC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_idx_scan, dim3(1), dim3(1024), 0, ctx->stream, n_tiles, tile_sum, tail);
        NC_HIP(ctx, hipGetLastError());
        int32_t t[4] = {0, 0, 0, 0};
        int64_t first_beg = 0, last_end = 0;
        NC_HIP(ctx, hipMemcpyAsync(t, tail, 16, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(&first_beg, d_beg, 8, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(&last_end, d_end + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        info_host[3] = (t[1] ? 1 : 0) | (t[2] ? 2 : 0) | (t[3] ? 4 : 0);
        if (info_host[3]) return NC_OK;                          // (the caller words the error)
        const int64_t w0 = first_beg >> min_shift, w1 = (last_end - 1) >> min_shift;
        if (w1 - w0 + 1 > INT32_MAX) return nc_fail(ctx, NC_ERR_ARG, "nc_lines_index: %lld windows", (long long)(w1 - w0 + 1));
        info_host[0] = t[0];
        info_host[1] = w0;
        info_host[2] = w1 - w0 + 1;
        return NC_OK;
    }
    if (n == 0) return NC_OK;
    const int64_t n_runs = info_host[0], w_first = info_host[1], n_win = info_host[2];
    if (info_host[3] || n_runs < 1 || n_runs > n || n_win < 1 || n_win > INT32_MAX || !d_run_bin || !d_run_vbeg || !d_run_vend || !d_win_min)
        return nc_fail(ctx, NC_ERR_ARG, "nc_lines_index: the second call takes the sizes of the first and all four outputs");
    hipLaunchKernelGGL(k_idx_runs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, d_beg, d_end, d_line_off, u0, n_members, d_foff,
                       min_shift, depth, (const int32_t *)d_work, (const int32_t *)tile_sum, (int32_t)n_runs, d_run_bin, d_run_vbeg, d_run_vend);
    NC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_idx_windows, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, ctx->stream, n, d_beg, d_end, d_line_off, u0, d_foff,
                       min_shift, w_first, n_win, d_win_min);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

// K7, the accumulate form (nc_indel.hip says when it is taken): the stand-alone scan's, and the only one with impute_indel_phase and with
// chunks off the pack's tile grid.  After the depths (k_hap_depth_b, 32-bit rows): k_yield_rank_b ranks a chunk's yielded columns, k_event_intervals_w
// adds every read's window-end intervals into the chunk's eight difference arrays in HBM (atomics into zeros: the workspace is cleared first),
// k_prefix_rows_b scans them into window counts and k_indel_decide_b takes the columns' decisions.
#include "nc_indel.h"

namespace {

// block-wide scan helper shared by the two per-chunk scans below: returns this thread's inclusive prefix inside the block
// and the block total (16 waves)
__device__ __forceinline__ int block_scan_1024(int v, int *wsum, int &tot)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
    inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int wp = 0;
    tot = 0;
    for (int w = 0; w < 16; w++) {
        const int s = wsum[w];
        if (w < wv) wp += s;
        tot += s;
    }
    return wp + inc;
}

// one workgroup per chunk: exclusive scan of the "column is yielded" flag -> rank among yielded columns; ny at rank[ncol]
__global__ __launch_bounds__(1024) void k_yield_rank_b(const IndelChunk *__restrict__ ck, char *__restrict__ ws, const uint8_t *__restrict__ excl,
                                                       int32_t grid_lo)
{
    __shared__ int wsum[16];
    __shared__ int carry;
    const IndelChunk c = ck[blockIdx.x];
    const int32_t ncol = c.ncol;
    const int32_t *depth = ck_depth(ws, c);
    int32_t *rank = ck_rank(ws, c);
    const int32_t excl_off = c.lo - grid_lo;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < ncol; base += 1024) {
        const int i = base + threadIdx.x;
        int v = 0;
        if (i < ncol) {
            const int tot = depth[i] + depth[ncol + i] + depth[2 * (int64_t)ncol + i];
            v = tot > 0 && !(excl && excl[excl_off + i]);
        }
        int tot;
        const int inc = block_scan_1024(v, wsum, tot);
        const int cc = carry;
        if (i < ncol) rank[i] = v ? cc + inc - v : -1;               // -1: not yielded
        __syncthreads();
        if (threadIdx.x == 0) carry = cc + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) rank[ncol] = carry;
}

// Merges the window-end intervals [e, e+w-1] of a kept read's qualifying events (a read counts once per window, set-union semantics of
// :254-264) and adds them to the per-(class, haplotype) difference arrays of every chunk its events fall into (chunks are ascending and may
// overlap).  One WAVE per read with the read's events across the lanes (one thread walking a read's ~400 events: 10 ms per chr20-sized
// contig, latency-bound).  The merged intervals of a (read, class, chunk) are the union of equal-length
// intervals [k, k + w - 1] over its qualifying events in rank order: an event OPENS an interval iff no qualifying event of the class
// precedes it within w - 1 ranks, and CLOSES one (at k + w) iff none follows within w - 1 ranks -- two local look-ups per event.
__global__ __launch_bounds__(256) void k_event_intervals_w(int32_t n_reads, const int32_t *__restrict__ ev_off, const int32_t *__restrict__ ev_pos,
                                                           const int32_t *__restrict__ ev_len, const uint8_t *__restrict__ read_hap,
                                                           const IndelChunk *__restrict__ ck, int32_t n_chunks, char *__restrict__ ws, int32_t win,
                                                           int32_t small_win, int32_t haploid, int32_t impute)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const int hp = read_hap[r];
    const bool tagged = haploid || hp == 1 || hp == 2;
    if (!tagged && !impute) return;
    const int h = haploid ? 0 : hp - 1;
    const int ea = ev_off[r], eb = ev_off[r + 1];
    auto qualifies = [](int32_t sl, int cls) {
        const int32_t ln = sl < 0 ? -sl : sl;
        const bool ins = sl > 0;
        return cls < 2 ? (ln > 2 && ln <= 50 && ins == (cls == 1)) : (ln <= 10 && ins == (cls == 3));
    };
    if (ea >= eb) return;
    // first chunk with hi >= the read's first event: one search per read on the scalar unit; an event's own first chunk is at most a
    // few steps further (a search per event was ten dependent loads, half of this kernel's time)
    int a0 = 0;
    {
        const int32_t p_first = __builtin_amdgcn_readfirstlane(ev_pos[ea]);
        int b = n_chunks;
        while (a0 < b) {
            const int m = (a0 + b) >> 1;
            if (ck[m].hi < p_first) a0 = m + 1; else b = m;
        }
    }
    for (int e = ea + lane; e < eb; e += 64) {
        const int32_t p = ev_pos[e], sl = ev_len[e];
        int a = a0;
        while (a < n_chunks && ck[a].hi < p) a++;
        for (int ci = a; ci < n_chunks && ck[ci].lo <= p; ci++) {
            const IndelChunk c = ck[ci];
            if (impute) atomicAdd(&ck_cnt(ws, c)[(int64_t)(sl > 0 ? 1 : 2) * c.ncol + (p - c.lo)], 1);      // :279-284, every read
            if (!tagged) continue;
            const int32_t *rank = ck_rank(ws, c);
            const int k = rank[p - c.lo];
            if (k < 0) continue;                                      // excluded column
            int32_t *diff = ck_diff(ws, c);
#pragma unroll
            for (int cls = 0; cls < 4; cls++) {
                if (!qualifies(sl, cls)) continue;
                const int w = cls < 2 ? win : small_win;
                bool has_prev = false, has_next = false;
                for (int e2 = e - 1; e2 >= ea; e2--) {
                    const int32_t p2 = ev_pos[e2];
                    if (p2 < c.lo) break;
                    const int k2 = rank[p2 - c.lo];
                    if (k2 < 0) continue;
                    if (k - k2 > w - 1) break;
                    if (qualifies(ev_len[e2], cls)) { has_prev = true; break; }
                }
                for (int e2 = e + 1; e2 < eb; e2++) {
                    const int32_t p2 = ev_pos[e2];
                    if (p2 > c.hi) break;
                    const int k2 = rank[p2 - c.lo];
                    if (k2 < 0) continue;
                    if (k2 - k > w - 1) break;
                    if (qualifies(ev_len[e2], cls)) { has_next = true; break; }
                }
                if (!has_prev) atomicAdd(&diff[(int64_t)(cls * 2 + h) * c.nd + k], 1);
                if (!has_next) atomicAdd(&diff[(int64_t)(cls * 2 + h) * c.nd + k + w], -1);
            }
        }
    }
}

// in-place inclusive prefix sum of each of the 8 difference arrays of each chunk (one workgroup per array)
__global__ __launch_bounds__(1024) void k_prefix_rows_b(const IndelChunk *__restrict__ ck, char *__restrict__ ws)
{
    __shared__ int wsum[16];
    __shared__ int carry;
    const IndelChunk c = ck[blockIdx.y];
    const int32_t nd = c.nd;
    int32_t *row = ck_diff(ws, c) + (int64_t)blockIdx.x * nd;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nd; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nd ? row[i] : 0;
        int tot;
        const int inc = block_scan_1024(v, wsum, tot);
        const int cc = carry;
        if (i < nd) row[i] = cc + inc;
        __syncthreads();
        if (threadIdx.x == 0) carry = cc + tot;
        __syncthreads();
    }
}

// per-column decision of :252-275 (float64 divide-and-compare, as in the reference); with impute_indel_phase also the
// column-level part of :278-284 (type 2: the read grouping of :285-304 is left to the host for these few columns)
__global__ void k_indel_decide_b(const IndelChunk *__restrict__ ck, char *__restrict__ ws, int32_t mincov, double ins_t, double del_t,
                                 int32_t haploid, int32_t impute, int8_t *__restrict__ col_type_all)
{
    const IndelChunk c = ck[blockIdx.y];
    const int32_t ncol = c.ncol, nd = c.nd;
    const int32_t *depth = ck_depth(ws, c), *rank = ck_rank(ws, c), *U = ck_diff(ws, c);
    int8_t *col_type = col_type_all + c.coloff;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ncol; i += gridDim.x * blockDim.x) {
        const int k = rank[i];
        const int n0 = depth[i], n1 = depth[ncol + i];
        int8_t type = indel_decide(k, n0, n1, [&](int cls, int h) { return U[(int64_t)(cls * 2 + h) * nd + k]; }, mincov, ins_t, del_t, haploid);
        const bool ruled = haploid || (k >= 0 && n0 >= mincov && n1 >= mincov);                         // :252-275 applied; otherwise (impute_indel_phase) :278-284
        if (!ruled && impute && k >= 0) {
            const int tot = n0 + n1 + depth[2 * (int64_t)ncol + i];
            if (tot >= 2 * mincov && tot > 0) {                                                          // :278
                const int32_t *cnt = ck_cnt(ws, c);
                const double del_f = (double)(cnt[i] + cnt[2 * (int64_t)ncol + i]) / (double)tot;        // '-' and '*' (:282)
                const double ins_f = (double)cnt[(int64_t)ncol + i] / (double)tot;                       // '+' (:283)
                if (del_t <= del_f || ins_t <= ins_f) type = 2;                                          // :284
            }
        }
        col_type[i] = type;
    }
}

}   // namespace

int nc_indel_launch_accum(nc_ctx *ctx, const IndelGroup &g)
{
    const nc_indel_events *ev = g.ev;
    const nc_indel_scan_params *prm = g.prm;
    // this form accumulates into zeros (the tiled one writes every word it reads)
    NC_HIP(ctx, hipMemsetAsync(g.ws, 0, g.zero_bytes, ctx->stream));
    NC_TRY(nc_indel_launch_depths(ctx, g, nullptr, IndelMates{nullptr, nullptr, 0}));
    hipLaunchKernelGGL(k_yield_rank_b, dim3(g.ng), dim3(1024), 0, ctx->stream, g.ck_dev, g.ws, g.excl, g.pack->tile_pos0);
    if (ev->n_reads > 0)
        hipLaunchKernelGGL(k_event_intervals_w, dim3((ev->n_reads + 3) / 4), dim3(256), 0, ctx->stream, ev->n_reads, ev->ev_off, ev->ev_pos,
                           ev->ev_len, ev->read_hap, g.ck_dev, g.ng, g.ws, prm->win_size, prm->small_win_size, prm->haploid, g.impute);
    hipLaunchKernelGGL(k_prefix_rows_b, dim3(8, g.ng), dim3(1024), 0, ctx->stream, g.ck_dev, g.ws);
    hipLaunchKernelGGL(k_indel_decide_b, dim3(g.ng == 1 ? 512 : 64, g.ng), dim3(256), 0, ctx->stream, g.ck_dev, g.ws, prm->mincov, prm->ins_t, prm->del_t,
                       prm->haploid, g.impute, g.ctype);
    return NC_OK;
}

// K7: indel candidate window scan (pass 1 of get_indel_testing_candidates, reference generate_indel_pileups.py:197-276), gfx950.  The driver:
// the group plan and launch, nc_indel_scan[_batch], and the kernels both forms run first (k_blk_chunks, k_hap_depth_b).  What the units share: nc_indel.h.
//
// A group of chunks runs in one of two forms:
//   tiled       nc_indel_tiles.hip   k_blk_base, [k_read_cursors, k_entry_rows, k_decide_tables], k_event_tiles: one workgroup per 1024 columns
//                                    counts the windows' reads in LDS and decides its columns; nothing but depths and ranks goes through HBM
//   accumulate  nc_indel_accum.hip   k_yield_rank_b, k_event_intervals_w, k_prefix_rows_b, k_indel_decide_b: interval ends added into zeroed
//                                    difference arrays in HBM with atomics, scanned, then decided
// The tiled form is taken when the caller is the device pipeline's plan (it hands over the map tile entry -> read: slot offsets, read bounds, an
// error word), impute_indel_phase is off, NC_K7_EVENT_ATOMICS is not set, every chunk lies inside the pack's tile grid, and there are reads and
// tile-blocks at all.  Everything else -- the stand-alone nc_indel_scan[_batch], impute_indel_phase, chunks off the grid -- takes the accumulate
// form.  Alignments that share read names are keyed by name in the tiled form only: such a group is refused when it would take the other.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "nc_indel.h"

namespace {

__device__ __forceinline__ uint32_t lut8i(uint32_t x, uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, x); }

// chunk of every tile-block (k_hap_depth_b's block index; k_event_tiles' / SPT): a workgroup finds its chunk by one load instead of a bisection of
// ten dependent scalar loads over the descriptors
__global__ void k_blk_chunks(const IndelChunk *__restrict__ ck, int32_t n_chunks, int32_t nblk, int32_t *__restrict__ blk_chunk)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int b0 = ck[c].blk0, b1 = c + 1 < n_chunks ? ck[c + 1].blk0 : nblk;
    for (int b = b0; b < b1; b++) blk_chunk[b] = c;
}

// per-column depth by haplotype tag; same access scheme as k_scan (one aligned dwordx4 of codes per read and lane).
// STAR: count the reads whose code is 4 (deleted at this column) of all haplotypes instead, into cnt[0]
// MATES: the pack holds alignments that share read names (entries with bit 3 of base_flag; nc_indel_set_mates).  len_seq_0 / len_seq_1 are sizes of
// name SETS (:219-223): such an alignment counts on the planes of its NAME's haplotype mask (both when records of the name carry HP 1 and HP 2),
// and not at the columns an earlier alignment of the name is present at.  (Haploid: the depth is len(read_names), duplicates included.)
template <int BLOCK, bool STAR, bool MATES>
__global__ __launch_bounds__(BLOCK) void k_hap_depth_b(const uint8_t *__restrict__ codes, const int32_t *__restrict__ tile_off,
                                                       const nc_tile_entry *__restrict__ tile_ent, int32_t tile_pos0,
                                                       const IndelChunk *__restrict__ ck, const int32_t *__restrict__ blk_chunk, char *__restrict__ ws, int32_t haploid,
                                                       const uint8_t *__restrict__ excl, int32_t grid_lo, int32_t *__restrict__ blk_yield, IndelMates mt)
{
    constexpr int TILE = BLOCK * 16;
    const IndelChunk c = ck[blk_chunk[blockIdx.x]];
    const int t = c.tile0 + ((int)blockIdx.x - c.blk0);
    const int32_t lo = c.lo, hi = c.hi, ncol = c.ncol;
    int32_t *depth = STAR ? ck_cnt(ws, c) : ck_depth(ws, c);
    const int32_t P0 = tile_pos0 + t * TILE + threadIdx.x * 16;
    uint32_t acc[3][4], wide[3][8];
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int d = 0; d < 4; d++) acc[q][d] = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) wide[q][d] = 0;
    }
    const int e0 = tile_off[t], e1 = tile_off[t + 1];
    int e = e0;
    while (e < e1) {
        const int lim = min(e1, e + 255);
#pragma unroll 8
        for (; e < lim; e++) {                                         // (eight reads' loads in flight, as in k_scan)
            const nc_tile_entry ent = tile_ent[e];
            const int32_t slo = ent.start & ~15, shi = (ent.end + 15) & ~15;
            uint4 v = make_uint4(0x07070707u, 0x07070707u, 0x07070707u, 0x07070707u);
            if (P0 >= slo && P0 < shi) v = *reinterpret_cast<const uint4 *>(codes + (ent.base_flag & ~int64_t(15)) + P0);
            const int hp = __builtin_amdgcn_readfirstlane((int)((ent.base_flag >> 1) & 3));           // wave-uniform: the plane is chosen by scalar branches
            const int plane = (STAR || haploid) ? 0 : hp == 1 ? 0 : hp == 2 ? 1 : 2;       // haploid: one read set, tags ignored
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t pres[4];
#pragma unroll
            for (int d = 0; d < 4; d++) pres[d] = STAR ? lut8i(w[d], 0u, 0x00000001u) : lut8i(w[d], 0x01010101u, 0x00000001u);   // code 4 | codes 0..4 -> 1
            if constexpr (MATES && !STAR) {
                if ((ent.base_flag & 8) && !haploid) {
                    const int self = imate_find(mt, (ent.base_flag & ~int64_t(15)) + slo);
                    if (self >= 0) {
                        int j = imate_get(mt, self).next;
                        for (int guard = 0; guard < 64 && j != self && j >= 0 && j < mt.n; guard++) {      // (a damaged ring must not hang the wave)
                            const IndelMate o = imate_get(mt, j);
                            if (j < self && P0 >= (o.start & ~15) && P0 < ((o.end + 15) & ~15)) {
                                const uint4 ov = *reinterpret_cast<const uint4 *>(codes + (mt.key[j] - (o.start & ~15)) + P0);
                                pres[0] &= ~lut8i(ov.x, 0x01010101u, 0x00000001u);
                                pres[1] &= ~lut8i(ov.y, 0x01010101u, 0x00000001u);
                                pres[2] &= ~lut8i(ov.z, 0x01010101u, 0x00000001u);
                                pres[3] &= ~lut8i(ov.w, 0x01010101u, 0x00000001u);
                            }
                            j = o.next;
                        }
                        const int nm = imate_get(mt, self).hap & 3;
#pragma unroll
                        for (int d = 0; d < 4; d++) {
                            if (nm & 1) acc[0][d] += pres[d];
                            if (nm & 2) acc[1][d] += pres[d];
                            if (!nm) acc[2][d] += pres[d];
                        }
                        continue;
                    }
                }
            }
            if (STAR || plane == 0) {
#pragma unroll
                for (int d = 0; d < 4; d++) acc[0][d] += pres[d];
            } else if (plane == 1) {
#pragma unroll
                for (int d = 0; d < 4; d++) acc[1][d] += pres[d];
            } else {
#pragma unroll
                for (int d = 0; d < 4; d++) acc[2][d] += pres[d];
            }
        }
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int d = 0; d < 4; d++) {
                wide[q][2 * d] += acc[q][d] & 0x00FF00FFu;
                wide[q][2 * d + 1] += (acc[q][d] >> 8) & 0x00FF00FFu;
                acc[q][d] = 0;
            }
    }
    // a lane holds 16 consecutive positions: through LDS (17-word pitch) so that a store instruction writes 64 consecutive positions
    // (a lane storing its own 16 made every instruction 64 four-byte pieces of 64 different lines: 1.26 GB written for 0.77)
    __shared__ int32_t tr[STAR ? 1 : 3][BLOCK * 17];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int d = i >> 2, k = i & 3, wi = 2 * d + (k & 1), sh = (k >> 1) * 16;
#pragma unroll
        for (int q = 0; q < (STAR ? 1 : 3); q++) tr[q][threadIdx.x * 17 + i] = (int32_t)((wide[q][wi] >> sh) & 0xFFFF);
    }
    __syncthreads();
    const int32_t T0 = tile_pos0 + t * TILE;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = r * BLOCK + threadIdx.x;                        // position T0 + j = lane j / 16, element j % 16
        const int32_t p = T0 + j;
        if (p < lo || p > hi) continue;
        if (!STAR && blk_yield) {                                     // the tiled route: 16-bit rows (the counters above are 16-bit fields already)
#pragma unroll
            for (int q = 0; q < 3; q++) reinterpret_cast<uint16_t *>(depth)[(int64_t)q * ncol + (p - lo)] = (uint16_t)tr[q][(j >> 4) * 17 + (j & 15)];
        } else {
#pragma unroll
            for (int q = 0; q < (STAR ? 1 : 3); q++) depth[(int64_t)q * ncol + (p - lo)] = tr[q][(j >> 4) * 17 + (j & 15)];
        }
    }
    if constexpr (!STAR) {
        if (!blk_yield) return;
        // The rank of a column among the chunk's yielded ones (depth > 0, not excluded), LOCAL to this tile-block: a lane has its 16 columns' depths
        // in registers.  The block's count goes to blk_yield, k_blk_base scans the counts of a chunk's blocks, and k_event_tiles adds the base of a
        // column's block (k_yield_rank_b walked a chunk in 98 dependent rounds of load -> scan: 0.30 ms per chr20-sized contig, all latency).
        int fl[16], sum = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int d = i >> 2, k = i & 3, wi = 2 * d + (k & 1), sh = (k >> 1) * 16;
            const int32_t p = P0 + i;
            const int tot = (int)(((wide[0][wi] >> sh) & 0xFFFF) + ((wide[1][wi] >> sh) & 0xFFFF) + ((wide[2][wi] >> sh) & 0xFFFF));
            bool y = p >= lo && p <= hi && tot > 0;
            if (y && excl) y = excl[(lo - grid_lo) + (p - lo)] == 0;
            fl[i] = y;
            sum += y;
        }
        __shared__ int wtot[BLOCK / 64];
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        int inc = sum;
        inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
        if (lane == 63) wtot[wv] = inc;
        __syncthreads();                                              // (also: every depth row has left tr)
        int wp = 0, all = 0;
#pragma unroll
        for (int q = 0; q < BLOCK / 64; q++) {
            if (q < wv) wp += wtot[q];
            all += wtot[q];
        }
        int run = wp + inc - sum;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            tr[0][threadIdx.x * 17 + i] = fl[i] ? run : -1;
            run += fl[i];
        }
        if (threadIdx.x == 0) blk_yield[blockIdx.x] = all;
        __syncthreads();
        int16_t *rank = reinterpret_cast<int16_t *>(ck_rank(ws, c));   // (local to the block: < 4096; -1 = not yielded)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = r * BLOCK + threadIdx.x;
            const int32_t p = T0 + j;
            if (p < lo || p > hi) continue;
            rank[p - lo] = (int16_t)tr[0][(j >> 4) * 17 + (j & 15)];
        }
    }
}

}   // namespace

int nc_indel_check(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const nc_indel_scan_params *prm, const char *who)
{
    if (!pack || !ev || !prm) return nc_fail(ctx, NC_ERR_ARG, "%s: bad argument", who);
    const int tile = pack->tile_size;
    if (!(tile == 1024 || tile == 2048 || tile == 4096)) return nc_fail(ctx, NC_ERR_ARG, "%s: malformed read pack", who);
    if (prm->win_size < 1 || prm->small_win_size < 1 || prm->win_size > 4096) return nc_fail(ctx, NC_ERR_ARG, "%s: window sizes", who);
    return NC_OK;
}

// workspace per group of chunks: a twelfth of the device memory that is free at the first call, between 6 and 24 GiB (a chr1-sized contig's
// columns need 12 GB: one group, one launch of every K7 kernel -- and ONE pass of the cursor tables' kernels over the tile index -- instead of two)
// (per context, after hipSetDevice: a process that drives several GPUs sizes each one's workspace from that GPU; what this context's workspace
// already holds counts as free, and a budget the device can no longer serve -- other buffers grew since -- shrinks to what is free now)
static size_t indel_budget(nc_ctx *ctx)
{
    size_t mfree = 0, mtotal = 0;
    if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) mfree = (size_t)72 << 30;
    const size_t avail = mfree + ctx->k7.ws.cap;
    const size_t want = std::min<size_t>((size_t)24 << 30, std::max<size_t>((size_t)6 << 30, avail / 12));
    if (ctx->k7.budget == 0 || (ctx->k7.budget_shrunk && want <= avail / 2)) {      // first plan, or memory has been freed since a low moment
        ctx->k7.budget = want;
        ctx->k7.budget_shrunk = false;
    }
    if (ctx->k7.budget > avail / 2) {
        ctx->k7.budget = std::max<size_t>((size_t)256 << 20, avail / 2);
        ctx->k7.budget_shrunk = true;
    }
    return ctx->k7.budget;
}

// The group that starts the chunk list: as many chunks as the budget holds, and where their parts lie in the workspace
struct GroupPlan {
    int32_t consumed = 0;            // chunks taken
    int32_t nblk = 0;                // their tile-blocks
    int64_t ncols = 0;               // their columns
    bool clipped = false;            // a chunk reaches past the pack's tile grid (columns no kernel of the tile index visits)
    size_t o_type, o_ck, o_blk, total;       // workspace: the chunks' slices | col_type | descriptors | blk_chunk, blk_yield, blk_base | end
};
static GroupPlan indel_group_plan(const nc_readpack *pack, int32_t n_chunks, const int32_t *starts, const int32_t *ends, int32_t win_size, int impute,
                                  size_t budget, std::vector<IndelChunk> &ck)
{
    const int tile = pack->tile_size;
    const int32_t grid_lo = pack->tile_pos0, grid_hi = pack->tile_pos0 + pack->n_tiles * tile - 1;
    GroupPlan g;
    ck.clear();
    size_t wsb = 0;
    for (; g.consumed < n_chunks; g.consumed++) {
        IndelChunk k;
        k.lo = starts[g.consumed] < 1 ? 1 : starts[g.consumed];
        k.hi = ends[g.consumed];
        k.ncol = k.hi - k.lo + 1;
        k.nd = k.ncol + win_size + 2;
        const size_t need = ((size_t)3 * k.ncol * 4 + ((size_t)k.ncol + 1) * 4 + (size_t)8 * k.nd * 4 + (impute ? (size_t)3 * k.ncol * 4 : 0) + 15) & ~(size_t)15;
        if (!ck.empty() && (wsb + need + (size_t)g.ncols + k.ncol > budget || ck.size() >= 32768)) break;   // gridDim.y < 65536
        k.ws = (int64_t)wsb;
        k.coloff = g.ncols;
        const int32_t clo = k.lo > grid_lo ? k.lo : grid_lo, chi = k.hi < grid_hi ? k.hi : grid_hi;
        k.tile0 = chi >= clo ? (clo - grid_lo) / tile : 0;
        k.blk0 = g.nblk;
        g.nblk += chi >= clo ? (chi - grid_lo) / tile - k.tile0 + 1 : 0;
        if (k.lo < grid_lo || k.hi > grid_hi) g.clipped = true;
        wsb += need;
        g.ncols += k.ncol;
        ck.push_back(k);
    }
    g.o_type = wsb;
    g.o_ck = (g.o_type + (size_t)g.ncols + 15) & ~(size_t)15;
    g.o_blk = g.o_ck + ((ck.size() * sizeof(IndelChunk) + 15) & ~(size_t)15);
    g.total = g.o_blk + (size_t)g.nblk * 4 * 3;
    return g;
}

// k_hap_depth_b for the pack's tile size: a lane holds 16 columns, so 1024 / 2048 / 4096-column tiles take 64 / 128 / 256 lanes
template <bool STAR, bool MATES>
static void launch_hap_depth(hipStream_t st, const IndelGroup &g, int32_t *blk_yield, const IndelMates &mt)
{
    const nc_readpack *pack = g.pack;
    const int B = pack->tile_size / 16;
    auto kernel = B == 64 ? k_hap_depth_b<64, STAR, MATES> : B == 128 ? k_hap_depth_b<128, STAR, MATES> : k_hap_depth_b<256, STAR, MATES>;
    hipLaunchKernelGGL(kernel, dim3(g.nblk), dim3(B), 0, st, pack->codes, pack->tile_off, pack->tile_ent, pack->tile_pos0, g.ck_dev, g.blk, g.ws,
                       g.prm->haploid, g.excl, pack->tile_pos0, STAR ? nullptr : blk_yield, mt);
}

int nc_indel_launch_depths(nc_ctx *ctx, const IndelGroup &g, int32_t *blk_yield, const IndelMates &mt)
{
    NC_TRY(nc_h2d_pieces(ctx, g.ck_dev, g.ck->data(), (size_t)g.ng * sizeof(IndelChunk), ctx->stream));   // by copy kernel: never behind an upload in flight
    if (g.nblk == 0) return NC_OK;
    hipLaunchKernelGGL(k_blk_chunks, dim3((g.ng + 255) / 256), dim3(256), 0, ctx->stream, g.ck_dev, g.ng, g.nblk, g.blk);
    if (mt.n > 0) launch_hap_depth<false, true>(ctx->stream, g, blk_yield, mt);
    else launch_hap_depth<false, false>(ctx->stream, g, blk_yield, mt);
    if (g.impute) launch_hap_depth<true, false>(ctx->stream, g, blk_yield, mt);
    return NC_OK;
}

// the launches of one group (up to and including the per-column decisions, which stay on the device at out->ctype; chunk
// descriptors in out->ck, on the device at out->ck_dev); no synchronisation
int nc_indel_scan_group_launch(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const uint8_t *excl_dev, int32_t n_chunks,
                               const int32_t *starts, const int32_t *ends, const nc_indel_scan_params *prm, const IndelPipeIn *pipe, IndelGroupOut *out)
{
    if (!(pipe && pipe->reuse_tables)) ctx->k7.ent_of = nullptr;
    const int impute = prm->impute && !prm->haploid;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const GroupPlan p = indel_group_plan(pack, n_chunks, starts, ends, prm->win_size, impute, indel_budget(ctx), out->ck);
    out->consumed = p.consumed;
    NC_TRY(nc_ensure(ctx, ctx->k7.ws, p.total));
    char *ws = (char *)ctx->k7.ws.p;
    // the form (this file's header); NC_K7_EVENT_ATOMICS: the accumulate form on the pipeline too, for A/B checks (read per call: tests flip it)
    const bool tiles = pipe && pipe->slot_off && pipe->rd_start && pipe->rd_end && pipe->err_bits && !impute && !getenv("NC_K7_EVENT_ATOMICS") &&
                       !p.clipped && ev->n_reads > 0 && p.nblk > 0 && pack->tile_size % EV_SUB == 0;
    // alignments that share read names (nc_indel_set_mates): keyed by name in the tiled form only
    if (pipe && pipe->mates.n > 0 && !tiles)
        return nc_fail(ctx, NC_ERR_UNSUPPORTED, "alignments that share read names: the indel scan keys them by name on its tiled route only (no impute_indel_phase, chunks inside the pack's tile grid)");
    IndelGroup g;
    g.pack = pack; g.ev = ev; g.prm = prm; g.excl = excl_dev; g.impute = impute;
    g.ck = &out->ck; g.ck_dev = (IndelChunk *)(ws + p.o_ck); g.ng = (int32_t)out->ck.size(); g.nblk = p.nblk;
    g.ws = ws; g.zero_bytes = p.o_type; g.ctype = (int8_t *)(ws + p.o_type); g.blk = (int32_t *)(ws + p.o_blk);
    NC_TRY(tiles ? nc_indel_launch_tiles(ctx, g, *pipe) : nc_indel_launch_accum(ctx, g));
    NC_HIP(ctx, hipGetLastError());
    out->ck_dev = g.ck_dev;
    out->ctype = g.ctype;
    return NC_OK;
}

// one group of ascending chunks: a single set of launches, one device-to-host copy per run of back-to-back outputs
static int indel_scan_group(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const uint8_t *excl_dev, int32_t n_chunks,
                            const int32_t *starts, const int32_t *ends, const nc_indel_scan_params *prm, int8_t *col_type_host,
                            const int64_t *col_off, int32_t *consumed)
{
    IndelGroupOut out;
    NC_TRY(nc_indel_scan_group_launch(ctx, pack, ev, excl_dev, n_chunks, starts, ends, prm, nullptr, &out));
    *consumed = out.consumed;
    const std::vector<IndelChunk> &ck = out.ck;
    const int8_t *ctype = out.ctype;
    const int32_t ng = (int32_t)ck.size();
    for (int32_t k = 0; k < ng;) {                                   // runs of chunks laid out back to back on the host as well
        int32_t j = k + 1;
        while (j < ng && col_off[j] - col_off[k] == ck[(size_t)j].coloff - ck[(size_t)k].coloff) j++;
        const int64_t nbytes = ck[(size_t)j - 1].coloff + ck[(size_t)j - 1].ncol - ck[(size_t)k].coloff;
        NC_HIP(ctx, hipMemcpyAsync(col_type_host + col_off[k], ctype + ck[(size_t)k].coloff, (size_t)nbytes, hipMemcpyDeviceToHost, ctx->stream));
        k = j;
    }
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

// Many chunks of one contig per call: every chunk keeps the reference's per-chunk semantics (fresh window deques at the
// chunk start).  Runs of chunks ascending in start and end go into the same launches, the chunk being a grid dimension.
extern "C" int nc_indel_scan_batch(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const uint8_t *excl_dev,
                                   int32_t n_chunks, const int32_t *starts, const int32_t *ends, const nc_indel_scan_params *prm,
                                   int8_t *col_type_host, const int64_t *col_off)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_chunks < 0 || (n_chunks && (!starts || !ends || !col_type_host || !col_off))) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_scan_batch: bad argument");
    NC_TRY(nc_indel_check(ctx, pack, ev, prm, "nc_indel_scan_batch"));
    if (n_chunks == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    for (int32_t c = 0; c < n_chunks; c++)
        if (ends[c] < starts[c]) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_scan_batch: chunk %d has end < start", c);
    NcTimer tm(ctx, 3);
    int32_t c0 = 0;
    while (c0 < n_chunks) {
        int32_t c1 = c0 + 1;                                         // maximal ascending run
        while (c1 < n_chunks && starts[c1] >= starts[c1 - 1] && ends[c1] >= ends[c1 - 1]) c1++;
        while (c0 < c1) {
            int32_t used = 0;
            NC_TRY(indel_scan_group(ctx, pack, ev, excl_dev, c1 - c0, starts + c0, ends + c0, prm, col_type_host, col_off + c0, &used));
            c0 += used;
        }
    }
    tm.stop();
    return NC_OK;
}

extern "C" int nc_indel_scan(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const uint8_t *excl_dev, int32_t start,
                             int32_t end, const nc_indel_scan_params *prm, int8_t *col_type_host)
{
    if (!ctx) return NC_ERR_ARG;
    if (!col_type_host || end < start) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_scan: bad argument");
    const int64_t off = 0;
    return nc_indel_scan_batch(ctx, pack, ev, excl_dev, 1, &start, &end, prm, col_type_host, &off);
}

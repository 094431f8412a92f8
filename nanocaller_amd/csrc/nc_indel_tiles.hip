// K7, the tiled form (nc_indel.hip says when it is taken): the device pipeline's.  The same result as the accumulate form without global atomics
// (k_event_intervals_w spends 4.8 of its 5.1 ms per chr20-sized contig in ~150 M scattered atomic adds): k_event_tiles, one workgroup per 1024
// columns of a chunk.  It takes the reads of the tile index that overlap its columns (and the columns before them whose windows reach in: the last
// wmax - 1 yielded columns), finds each read's events there from the cursor tables, gives every event to a lane, accumulates the interval ends in LDS
// (clipped to the block's ranks: what a read covers INSIDE the block does not depend on events outside the margin), scans the eight rows into the
// window counts U[class, haplotype][rank] and takes the columns' decisions from them: the counts never reach HBM (2 GB written and 2 GB read per
// chr20-sized contig) and the workspace needs no zeroing.  Needs the map tile entry -> read (slot_off of the wire pack), which the device pipeline has.
// Before it: k_hap_depth_b (16-bit depth rows, block-local ranks) and k_blk_base; once per pack the cursor tables (k_read_cursors, k_entry_rows)
// and the decision tables (k_decide_tables).
#include <algorithm>
#include <cstdlib>

#include "nc_indel.h"

namespace {

// exclusive scan of the yielded-column counts of a chunk's tile-blocks (one wave per chunk) -> the rank of the first yielded column of every block
__global__ __launch_bounds__(256) void k_blk_base(const IndelChunk *__restrict__ ck, int32_t n_chunks, int32_t nblk, const int32_t *__restrict__ blk_yield,
                                                  int32_t *__restrict__ blk_base, char *__restrict__ ws)
{
    const int ci = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ci >= n_chunks) return;
    const IndelChunk c = ck[ci];
    const int b0 = c.blk0, b1 = ci + 1 < n_chunks ? ck[ci + 1].blk0 : nblk;
    int carry = 0;
    for (int b = b0; b < b1; b += 64) {
        const int v = b + lane < b1 ? blk_yield[b + lane] : 0;
        int inc = v;
        inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
        if (b + lane < b1) blk_base[b + lane] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) ck_rank(ws, c)[c.ncol] = carry;                    // ny, as k_yield_rank_b leaves it
}

// Decisions without divisions.  fl(U / n) >= t is monotone in the integer U, so for every depth n < DEC_N there is a smallest count that passes:
// k_decide_tables finds it with the reference's own float64 divide-and-compare (bisection over U; 65535 = none), once per call for del_t and
// ins_t, and a column's eight ratio tests become table look-ups.  The sum rule (f2 + f3 >= 0.9) is decided in integers when the exact sum is not
// 0.9 itself (then it is at least 1 / (10 n) > 1e-6 away, against rounding errors below 1e-12), else by the float64 expression.  indel_decide
// (the division form) stays for depths beyond the table and as the other routes' kernel: test_tiled_event_windows_equal_the_atomic_form compares them.
constexpr int DEC_N = 1024;
__global__ void k_decide_tables(double del_t, double ins_t, uint16_t *__restrict__ tab)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * DEC_N) return;
    const int n = i % DEC_N;
    const double t = i < DEC_N ? del_t : ins_t;
    int v;
    if (n == 0) v = 0.0 >= t ? 0 : 65535;                            // (n == 0: the ratio is 0.0 by definition)
    else {
        int lo = 0, hi = 65535;                                       // smallest U in [0, 65535) with U / n >= t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)mid / (double)n >= t) hi = mid; else lo = mid + 1;
        }
        v = lo;
    }
    tab[i] = (uint16_t)v;
}
template <class UF>
__device__ __forceinline__ int8_t indel_decide_tab(int k, int n0, int n1, UF U, int32_t mincov, double ins_t, double del_t, int32_t haploid,
                                                   const uint16_t *tdel, const uint16_t *tins, int dec_n)
{
    if (n0 >= dec_n || n1 >= dec_n) return indel_decide(k, n0, n1, U, mincov, ins_t, del_t, haploid);
    auto sum_rule = [&](int u2, int u3, int n) {
        if (n <= 0) return false;
        const int a = 10 * (u2 + u3), b = 9 * n;
        if (a != b) return a > b;
        return ((double)u2 / (double)n + (double)u3 / (double)n) >= 0.9;
    };
    if (haploid) {
        if (k >= 0 && n0 >= mincov && n0 > 0) {
            const int td = tdel[n0], ti = tins[n0];
            if (U(0, 0) >= td || U(1, 0) >= ti) return 0;
            if (U(2, 0) >= td || U(3, 0) >= ti || sum_rule(U(2, 0), U(3, 0), n0)) return 1;
        }
    } else if (k >= 0 && n0 >= mincov && n1 >= mincov) {
        const int td0 = tdel[n0], ti0 = tins[n0], td1 = tdel[n1], ti1 = tins[n1];
        if (U(0, 0) >= td0 || U(0, 1) >= td1 || U(1, 0) >= ti0 || U(1, 1) >= ti1) return 0;
        if (U(2, 0) >= td0 || U(2, 1) >= td1 || U(3, 0) >= ti0 || U(3, 1) >= ti1 || sum_rule(U(2, 0), U(3, 0), n0) || sum_rule(U(2, 1), U(3, 1), n1)) return 1;
    }
    return -1;
}

constexpr int EV_MARGIN = 256, EV_CAP = 2048, EV_NT = 512;          // (EV_SUB: nc_indel.h)

// read index of every tile entry (its slot offset is unique) and its event cursors: for the tile's 1024-column blocks h = 0 .. SPT-1 (and the
// one after the tile) the first event of the read at or after (tile start + 1024 h - EV_BACK).  Once per call (k_read_cursors + k_entry_rows), so that
// the blocks of k_event_tiles find an entry's events by a walk of a few steps instead of two bisections each (a third of that kernel).
// Row of an entry (NC_ENT_CUR_PITCH(SPT) words): [0 .. SPT] those cursors, [SPT + 1] / [SPT + 2] the read's event range, [SPT + 3 + h] the
// first event at or after the START of block h + 1 (exact: where block h's events end)
constexpr int EV_BACK = 64;

// The table is made WITHOUT random probes (bisecting every entry's read was ~35 probes into 276 MB of event positions, 2.2 GB fetched per
// chr20-sized contig, TA busy 0.82).  k_read_cursors streams the events once, one wave per read: event i is the first one at or after every
// block boundary B (and B - EV_BACK) that lies in (position of event i - 1, position of event i]; boundaries behind the last event get the
// read's event count.  A read's boundaries are those of the tiles it overlaps; its part of the table starts at rc_off(r) = slot offset / 1024
// + (2 SPT + 2) r (slots are at least as long as the reads: the parts do not overlap, no scan needed).  k_entry_rows then copies an entry's row.
__device__ __forceinline__ int64_t rc_off(int64_t slot_off, int r, int SPT) { return (slot_off >> 10) + (int64_t)(2 * SPT + 2) * r; }

__global__ __launch_bounds__(256) void k_read_cursors(int32_t n_reads, const int32_t *__restrict__ rd_start, const int32_t *__restrict__ rd_end,
                                                      const int64_t *__restrict__ slot_off, const int32_t *__restrict__ ev_off,
                                                      const int32_t *__restrict__ ev_pos, int32_t tile_pos0, int32_t tile_size,
                                                      int32_t *__restrict__ rc_lo, int32_t *__restrict__ rc_hi)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n_reads) return;
    const int SPT = tile_size / 1024;
    const int32_t rs = rd_start[r], re = rd_end[r];
    const int ea = ev_off[r], eb = ev_off[r + 1];
    const int ta = (rs - tile_pos0) / tile_size, tb = (max(re - 1, rs) - tile_pos0) / tile_size;
    const int g0 = ta * SPT, cnt = (tb - ta + 1) * SPT + 1;         // boundaries g0 .. g0 + cnt - 1 at tile_pos0 + 1024 g
    int32_t *lo = rc_lo + rc_off(slot_off[r], r, SPT), *hi = rc_hi + rc_off(slot_off[r], r, SPT);
    constexpr int RU = 4;                                            // (a lane's loads of four rounds in flight together)
    for (int ib = ea + lane; ib <= eb; ib += 64 * RU) {              // (i == eb: the end of the list, behind every event)
        int32_t pp[RU], pc[RU];
#pragma unroll
        for (int u = 0; u < RU; u++) {
            const int i = ib + 64 * u;
            pp[u] = i > ea && i <= eb ? ev_pos[i - 1] : 0;
            pc[u] = i < eb ? ev_pos[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < RU; u++) {
            const int i = ib + 64 * u;
            if (i > eb) break;
            const bool first = i == ea, last = i == eb;
            // boundaries B with pp < B - back <= pc  <=>  floor((pp + back - p0) / 1024) < k + g0 <= floor((pc + back - p0) / 1024)
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const int back = w == 0 ? EV_BACK : 0;
                int k0 = first ? 0 : ((pp[u] + back - tile_pos0) >> 10) + 1 - g0;
                int k1 = last ? cnt - 1 : ((pc[u] + back - tile_pos0) >> 10) - g0;
                k0 = max(k0, 0);
                k1 = min(k1, cnt - 1);
                int32_t *dst = w == 0 ? lo : hi;
                for (int k = k0; k <= k1; k++) dst[k] = i;
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_entry_rows(const int32_t *__restrict__ tile_off, const nc_tile_entry *__restrict__ tile_ent, int32_t tile_pos0,
                                                   int32_t tile_size, const int64_t *__restrict__ slot_off, int32_t n_reads,
                                                   const int32_t *__restrict__ ev_off, const int32_t *__restrict__ rc_lo, const int32_t *__restrict__ rc_hi,
                                                   const int32_t *__restrict__ rd_start, const int32_t *__restrict__ rd_end,
                                                   int32_t *__restrict__ ent_read, int32_t *__restrict__ ent_cur)
{
    const int t = blockIdx.x, SPT = tile_size / 1024;
    for (int e = tile_off[t] + (int)threadIdx.x; e < tile_off[t + 1]; e += 64) {
        const nc_tile_entry ent = tile_ent[e];
        const int64_t so = (ent.base_flag & ~int64_t(15)) + (ent.start & ~15);
        int lo = 0, hi = n_reads;
        while (lo < hi) {                                              // (1.3 MB of slot offsets: the probes stay in L2)
            const int mid = (lo + hi) >> 1;
            if (slot_off[mid] < so) lo = mid + 1; else hi = mid;
        }
        const int r = lo;
        ent_read[e] = r;
        const int32_t rs = rd_start[r], re = rd_end[r];               // (the table's geometry is the read table's, as k_read_cursors took it)
        const int ta = (rs - tile_pos0) / tile_size, tb = (max(re - 1, rs) - tile_pos0) / tile_size;
        const int cnt = (tb - ta + 1) * SPT + 1;
        const int64_t off = rc_off(slot_off[r], r, SPT);
        int32_t *row = ent_cur + (int64_t)e * NC_ENT_CUR_PITCH(SPT);
        const int kb = (t - ta) * SPT;                                 // boundary index of the tile's first block (clamped: a tile before / behind the read)
        for (int h = 0; h <= SPT; h++) {
            const int k = min(max(kb + h, 0), cnt - 1);
            row[h] = rc_lo[off + k];
            if (h > 0) row[SPT + 3 + (h - 1)] = rc_hi[off + k];
        }
        row[SPT + 1] = ev_off[r];
        row[SPT + 2] = ev_off[r + 1];
    }
}

// the classes (bit cls) an event of signed length sl qualifies for: 0 / 1 deletions / insertions of 3 .. 50 bases, 2 / 3 of at most 10
__device__ __forceinline__ uint32_t ev_qmask(int32_t sl)
{
    const int32_t ln = sl < 0 ? -sl : sl;
    const bool ins = sl > 0;
    return ((ln > 2 && ln <= 50) ? (ins ? 2u : 1u) : 0u) | (ln <= 10 ? (ins ? 8u : 4u) : 0u);
}
// k_event_tiles<true>: an event's owner is its read NAME (:225-235 build sets of names).  For the event `ev` (column p, rank k, classes qm) of table
// member `self`: the classes for which another alignment of the name holds a qualifying event within the class's window before it (-> prevf) / after
// it (-> nextf), in the order (column, table index); rkf(column) = its rank or -1, lo_pos / hi_pos = the columns rkf covers.
template <class RK>
__device__ __forceinline__ void mate_neighbours(const IndelMates &mt, int self, int32_t p, int k, uint32_t qm, int win, int small_win,
                                                const int32_t *__restrict__ ev_off, const int32_t *__restrict__ ev_pos, const int32_t *__restrict__ ev_len,
                                                int32_t lo_pos, int32_t hi_pos, RK rkf, uint32_t &prevf, uint32_t &nextf)
{
    int j = imate_get(mt, self).next;
    for (int guard = 0; guard < 64 && j != self && j >= 0 && j < mt.n; guard++) {
        const IndelMate o = imate_get(mt, j);
        const int ea = ev_off[o.read], eb = ev_off[o.read + 1];
        const int32_t want = j < self ? p + 1 : p;                    // first event of j that comes after this one
        int x = ea, y = eb;
        while (x < y) { const int mid = (x + y) >> 1; if (ev_pos[mid] < want) x = mid + 1; else y = mid; }
        uint32_t need = qm & ~prevf;
        for (int e2 = x - 1; e2 >= ea && need; e2--) {
            const int32_t p2 = ev_pos[e2];
            if (p2 < lo_pos) break;
            const int k2 = rkf(p2);
            if (k2 < 0) continue;
            const int d = k - k2;
            if (d > win - 1) need &= ~3u;
            if (d > small_win - 1) need &= ~12u;
            const uint32_t f = ev_qmask(ev_len[e2]) & need;
            prevf |= f;
            need &= ~f;
        }
        need = qm & ~nextf;
        for (int e2 = x; e2 < eb && need; e2++) {
            const int32_t p2 = ev_pos[e2];
            if (p2 > hi_pos) break;
            const int k2 = rkf(p2);
            if (k2 < 0) continue;
            const int d = k2 - k;
            if (d > win - 1) need &= ~3u;
            if (d > small_win - 1) need &= ~12u;
            const uint32_t f = ev_qmask(ev_len[e2]) & need;
            nextf |= f;
            need &= ~f;
        }
        j = o.next;
    }
}

// MATES: entries with bit 3 of base_flag (nc_indel_set_mates) are keyed by name: tagged by the name's haplotype mask (en_h 2 = both rows), and an
// event opens / closes a window interval only if no alignment of the name holds a qualifying event within the window before / after it.
template <bool MATES>
__global__ __launch_bounds__(EV_NT, 8) void k_event_tiles(const int32_t *__restrict__ tile_off, const nc_tile_entry *__restrict__ tile_ent, int32_t tile_pos0,
                                                     int32_t tile_size, const int32_t *__restrict__ ent_read, const int32_t *__restrict__ ent_cur,
                                                     const int32_t *__restrict__ ev_off, const int32_t *__restrict__ ev_pos,
                                                     const int32_t *__restrict__ ev_len, const uint8_t *__restrict__ read_hap,
                                                     const IndelChunk *__restrict__ ck, const int32_t *__restrict__ blk_chunk, char *__restrict__ ws, int32_t win,
                                                     int32_t small_win, int32_t haploid, int32_t mincov, double ins_t, double del_t,
                                                     int8_t *__restrict__ col_type_all, int32_t *__restrict__ err_bits, const uint16_t *__restrict__ dec_tab,
                                                     const int32_t *__restrict__ blk_base, int32_t dec_n, IndelMates mt)
{
    // interval ends per (class, haplotype) row and rank as 16-bit fields, two ranks per word, each biased by 0x4000: +1 is an atomic add and
    // -1 an atomic SUBTRACT of the field's unit, so neither carries into the neighbour field (16 KB instead of 32: a fourth workgroup per CU)
    __shared__ uint32_t difw[8][EV_SUB / 2];
    auto dif_add = [&](int row, int i) { atomicAdd(&difw[row][i >> 1], 1u << (16 * (i & 1))); };
    auto dif_sub = [&](int row, int i) { atomicSub(&difw[row][i >> 1], 1u << (16 * (i & 1))); };
    __shared__ int32_t rkw[EV_SUB + EV_MARGIN];
    __shared__ int32_t en_e0[256], en_pre[257], en_lim[256];
    __shared__ uint8_t en_h[256];
    __shared__ int32_t en_mate[MATES ? 256 : 1];                     // (MATES) the entry's row in the table of shared names, -1: its name is its own
    // hp tag / table row of an entry: the name's haplotype mask for a shared name (3: records with HP 1 and with HP 2)
    auto name_tag = [&](const nc_tile_entry &en, int &hp) {
        int row = -1;
        if ((en.base_flag & 8) && (row = imate_find(mt, (en.base_flag & ~int64_t(15)) + (en.start & ~15))) >= 0) hp = haploid ? hp : imate_get(mt, row).hap & 3;
        return row;
    };
    __shared__ int32_t evk[EV_CAP];                                  // the batch's events: rank of the column (-1 excluded), classes they qualify for
    __shared__ uint8_t evq[EV_CAP];
    __shared__ uint8_t own[EV_CAP];                                  // entry (of the batch's 256) every event of the batch belongs to
    __shared__ int32_t sh_k0, sh_k1, sh_mlo, wsum[EV_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int SPT = tile_size / EV_SUB;
    const IndelChunk c = ck[blk_chunk[(int)blockIdx.x / SPT]];
    const int rel = (int)blockIdx.x - c.blk0 * SPT, t = c.tile0 + rel / SPT;
    const int32_t s_lo = tile_pos0 + t * tile_size + (rel % SPT) * EV_SUB;
    const int32_t b_lo = max(s_lo, c.lo), b_hi = min(s_lo + EV_SUB - 1, c.hi);
    if (b_lo > b_hi) return;
    const int16_t *rank = reinterpret_cast<const int16_t *>(ck_rank(ws, c));      // 16-bit rows, ranks local to their tile-block (k_hap_depth_b)
    const int32_t w_lo = max(c.lo, b_lo - EV_MARGIN);             // LDS window of the rank array
    if (tid == 0) { sh_k0 = INT32_MAX; sh_k1 = -1; sh_mlo = c.lo; }
    for (int i = tid; i < 8 * EV_SUB / 2; i += EV_NT) (&difw[0][0])[i] = 0x40004000u;
    // The entries of the block, FAST form: events from the cursor EV_BACK columns before the block to the exact cursor of the next block's start
    // -- no load depends on the margin, so the entry + cursor-row loads run beside the rank window's.  Events outside [c.lo, b_hi] are dropped one
    // by one (rkf below); events before the margin but inside the chunk are harmless: their intervals end before the block's first rank and are
    // clipped to it (+1 and -1 cancel), and a chain they extend to the left covers the same ranks of the block.  The fast form holds when the margin
    // starts at or after m_fix (block-uniform; else: excluded / empty stretches) and the tiles' entries fit one batch; otherwise the general walk.
    const int32_t m_fix = max(c.lo, b_lo - EV_BACK);
    const int t_fix = max(0, (m_fix - tile_pos0) / tile_size);    // t or t - 1
    const int fe0 = tile_off[t_fix], fe_t = tile_off[t], fe1 = tile_off[t + 1];
    const bool fast_ok = fe1 - fe0 <= 256;
    nc_tile_entry f_ent = {0, 0, 0};
    int f_x0 = 0, f_x1 = 0;
    const bool f_on = fast_ok && tid < 256 && fe0 + tid < fe1;
    const int f_tt = fe0 + tid >= fe_t ? t : t_fix;
    if (f_on) {
        const int e = fe0 + tid;
        f_ent = tile_ent[e];
        const int32_t *row = ent_cur + (int64_t)e * NC_ENT_CUR_PITCH(SPT);
        const int hq = rel % SPT;
        f_x0 = f_tt == t ? row[hq] : row[SPT];
        f_x1 = f_tt == t ? row[SPT + 3 + hq] : row[SPT + 2];
    }
    __syncthreads();
    {
        int32_t kmin = INT32_MAX, kmax = -1;                         // first / last yielded rank of the block's own columns
        constexpr int RKU = (EV_SUB + EV_MARGIN + EV_NT - 1) / EV_NT;     // (a thread's ranks in one round trip)
        int32_t rr[RKU];
#pragma unroll
        for (int u = 0; u < RKU; u++) {
            const int i = tid + u * EV_NT;
            rr[u] = i <= b_hi - w_lo ? (int32_t)rank[w_lo + i - c.lo] : -1;
        }
        // the ranks in HBM are local to their tile-block (k_hap_depth_b): the window lies in at most two blocks of the chunk
        const int wb0 = c.blk0 + (w_lo - tile_pos0) / tile_size - c.tile0;
        const int32_t edge = tile_pos0 + ((w_lo - tile_pos0) / tile_size + 1) * tile_size;      // first column of the second block
        const int32_t base0 = blk_base[wb0], base1 = edge <= b_hi ? blk_base[wb0 + 1] : 0;
#pragma unroll
        for (int u = 0; u < RKU; u++) {
            const int i = tid + u * EV_NT;
            if (rr[u] >= 0) rr[u] += w_lo + i >= edge ? base1 : base0;
        }
#pragma unroll
        for (int u = 0; u < RKU; u++) {
            const int i = tid + u * EV_NT;
            if (i > b_hi - w_lo) break;
            const int32_t r = rr[u];
            rkw[i] = r;
            if (r >= 0 && w_lo + i >= b_lo) { kmin = min(kmin, r); kmax = max(kmax, r); }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            kmin = min(kmin, __shfl_xor(kmin, o, 64));
            kmax = max(kmax, __shfl_xor(kmax, o, 64));
        }
        if (lane == 0) { atomicMin(&sh_k0, kmin); atomicMax(&sh_k1, kmax); }
    }
    int f_cnt = 0;                                                   // (everything but `fast` itself is known here: one register lives on)
    {
        const int32_t ft_lo = tile_pos0 + f_tt * tile_size;
        const bool mine = f_tt == t || f_ent.end <= ft_lo + tile_size;
        int hp = (int)((f_ent.base_flag >> 1) & 3);
        int row = -1;
        if constexpr (MATES) { if (f_on) row = name_tag(f_ent, hp); }
        if (f_on && mine && f_ent.start <= b_hi && f_ent.end > m_fix && (haploid || hp == 1 || hp == 2 || (MATES && hp == 3))) {
            f_cnt = max(f_x1 - f_x0, 0);
            en_e0[tid] = f_x0;
            en_lim[tid] = f_x1;
            en_h[tid] = (uint8_t)(haploid ? 0 : hp - 1);
            if constexpr (MATES) en_mate[tid] = row;
        }
    }
    __syncthreads();
    const int32_t k0 = sh_k0, nk = sh_k1 - k0 + 1;
    int8_t *col_type = col_type_all + c.coloff;
    if (sh_k1 < 0) {                                                 // no yielded column here
        for (int i = b_lo + tid; i <= b_hi; i += EV_NT) col_type[i - c.lo] = -1;
        return;
    }
    auto rk = [&](int32_t p) {                                       // (written so that the common case is a plain LDS read, not a flat load)
        int32_t k = rkw[max(p - w_lo, 0)];
        if (p < w_lo) {
            k = (int32_t)rank[p - c.lo];
            if (k >= 0) k += blk_base[c.blk0 + (p - tile_pos0) / tile_size - c.tile0];
        }
        return k;
    };
    const int wmax = max(win, small_win);
    if (wv == 0) {
        // margin: the columns before b_lo holding the ranks k0 - (wmax - 1) .. k0 - 1 -> its first column (walk back, 64 columns a step)
        const int32_t need = k0 - (wmax - 1);
        int32_t mlo = c.lo;
        for (int32_t base = b_lo - 1; base >= c.lo; base -= 64) {
            const int32_t pos = base - lane;
            const int32_t r = pos >= c.lo ? rk(pos) : -1;
            const uint64_t m = __ballot(r >= 0 && r < need);       // columns already outside the margin: the nearest one ends it
            if (m) { mlo = base - (int)__builtin_ctzll(m) + 1; break; }
        }
        if (lane == 0) sh_mlo = mlo;
    }
    __syncthreads();
    const int32_t m_lo = sh_mlo;
    auto qualifies = [](int32_t sl, int cls) {
        const int32_t ln = sl < 0 ? -sl : sl;
        const bool ins = sl > 0;
        return cls < 2 ? (ln > 2 && ln <= 50 && ins == (cls == 1)) : (ln <= 10 && ins == (cls == 3));
    };
    auto rkf = [&](int32_t p) { return (p < c.lo || p > b_hi) ? -1 : rk(p); };      // (an event off the block's columns counts as on an excluded one)
    const bool fast = fast_ok && m_lo >= m_fix;
    if (fe1 - fe0 > 16000 && tid == 0) atomicOr(err_bits, 8);    // more reads than a 16-bit field counts interval ends for: the caller takes the other route
    const int t_first = fast ? t : max(0, (m_lo - tile_pos0) / tile_size);
    for (int tt = t_first; tt <= t; tt++) {
        const int32_t tt_lo = tile_pos0 + tt * tile_size;
        const int e0 = fast ? fe0 : tile_off[tt], e1 = fast ? fe0 + 1 : tile_off[tt + 1];          // (fast: one batch)
        if (e1 - e0 > 16000 && tid == 0) atomicOr(err_bits, 8);
        for (int eb0 = e0; eb0 < e1; eb0 += 256) {
            // ---- one entry per thread: its read, the read's events in [m_lo, b_hi]
            int cnt = 0;
            const int e = eb0 + tid;
            if (fast) cnt = f_cnt;
            else
            if (tid < 256 && e < e1) {
                // two levels of loads: the entry and its row of the cursor table (cursors of this block and the next, the read's event range); then the
                // events either side of both cursors, all at once.  The haplotype tag sits in the entry.  (Round 4 walked: entry -> read -> tag, event
                // range -> cursors -> one event per step: eight dependent loads per workgroup, a third of the kernel.)
                const nc_tile_entry ent = tile_ent[e];
                const int32_t *cur = ent_cur + (int64_t)e * NC_ENT_CUR_PITCH(SPT);
                const int hq = tt == t ? rel % SPT : SPT;
                int x0 = cur[hq], x1 = tt == t ? cur[hq + 1] : cur[SPT + 2];
                const int ea = cur[SPT + 1], eb = cur[SPT + 2];
                // a read is taken at the LAST of these tiles that lists it: tile t's entry knows where the block's events begin and end
                // (k_entry_rows), an entry of an earlier tile is of a read that ends before tile t
                const bool mine = tt == t || ent.end <= tt_lo + tile_size;
                int hp = (int)((ent.base_flag >> 1) & 3);
                int row = -1;
                if constexpr (MATES) row = name_tag(ent, hp);
                if (mine && ent.start <= b_hi && ent.end > m_lo && (haploid || hp == 1 || hp == 2 || (MATES && hp == 3))) {
                    if constexpr (MATES) en_mate[tid] = row;
                    if (tt < t - 1) {                                         // (a margin longer than a tile: excluded stretch)
                        x0 = ea;
                        int y0 = eb;
                        while (x0 < y0) {
                            const int m0 = (x0 + y0) >> 1;
                            if (ev_pos[m0] < m_lo) x0 = m0 + 1; else y0 = m0;
                        }
                    }
                    // the cursors stand EV_BACK columns before their block
                    const int32_t p0m = x0 > ea ? ev_pos[x0 - 1] : INT32_MIN, p1m = x1 > ea ? ev_pos[x1 - 1] : INT32_MIN;
                    int32_t q0[4], q1[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { q0[u] = x0 + u < eb ? ev_pos[x0 + u] : INT32_MAX; q1[u] = x1 + u < eb ? ev_pos[x1 + u] : INT32_MAX; }
                    int adv0 = 0, adv1 = 0;
#pragma unroll
                    for (int u = 0; u < 4; u++) { adv0 += q0[u] < m_lo ? 1 : 0; adv1 += q1[u] <= b_hi ? 1 : 0; }       // (ascending: prefixes)
                    const int nx0 = x0 + adv0;
                    const bool slow = p0m >= m_lo || adv0 == 4 || adv1 == 4 || x1 < nx0 || (x1 > nx0 && p1m > b_hi);
                    if (!slow) { x0 = nx0; x1 += adv1; }
                    else {                                                   // the general walk
                        while (x0 > ea && ev_pos[x0 - 1] >= m_lo) x0--;
                        while (x0 < eb && ev_pos[x0] < m_lo) x0++;
                        x1 = max(x1, x0);
                        while (x1 > x0 && ev_pos[x1 - 1] > b_hi) x1--;
                        while (x1 < eb && ev_pos[x1] <= b_hi) x1++;
                    }
                    cnt = x1 - x0;
                    en_e0[tid] = x0;
                    en_lim[tid] = x1;
                    en_h[tid] = (uint8_t)(haploid ? 0 : hp - 1);
                }
            }
            // ---- exclusive prefix of the counts over the 256 entries
            int inc = cnt;
            inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
            if (lane == 63 && wv < 4) wsum[wv] = inc;
            __syncthreads();
            int wp = 0;
            for (int q = 0; q < wv && q < 4; q++) wp += wsum[q];
            if (tid < 256) en_pre[tid] = wp + inc - cnt;
            const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            if (tid == 0) en_pre[256] = total;
            // (an event finds its entry by one LDS read: two bisections of eight dependent reads each per event were a third of this kernel)
            if (tid < 256 && total <= EV_CAP) for (int u = 0; u < cnt; u++) own[wp + inc - cnt + u] = (uint8_t)tid;
            __syncthreads();
            // ---- one event per thread
            if (total <= EV_CAP) {
                // the batch's events into LDS (independent loads), then every look-up at a neighbour is an LDS read
                constexpr int EVU = 4;                                            // (a thread's events in one round trip to HBM)
                for (int base = 0; base < total; base += EVU * EV_NT) {
                    int32_t e_pos[EVU], e_len[EVU];
#pragma unroll
                    for (int u = 0; u < EVU; u++) {
                        const int idx = base + tid + u * EV_NT;
                        if (idx < total) {
                            const int lo = own[idx];
                            const int ev = en_e0[lo] + (idx - en_pre[lo]);
                            e_pos[u] = ev_pos[ev];
                            e_len[u] = ev_len[ev];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < EVU; u++) {
                        const int idx = base + tid + u * EV_NT;
                        if (idx < total) {
                            const int32_t sl = e_len[u];
                            evk[idx] = rkf(e_pos[u]);
                            evq[idx] = (uint8_t)((qualifies(sl, 0) ? 1 : 0) | (qualifies(sl, 1) ? 2 : 0) | (qualifies(sl, 2) ? 4 : 0) | (qualifies(sl, 3) ? 8 : 0));
                        }
                    }
                }
                __syncthreads();
                for (int idx = tid; idx < total; idx += EV_NT) {
                    const int k = evk[idx], qm = evq[idx];
                    if (k < 0 || qm == 0) continue;
                    const int lo = own[idx];
                    const int i0 = en_pre[lo], i1 = en_pre[lo + 1], h = en_h[lo];
                    // one walk back and one forward for all the classes the event qualifies for (a class leaves the search when the distance passes
                    // its window: the ranks only grow apart) instead of two loops per class: the per-class form was 0.9 of this kernel's 2.2 ms
                    uint32_t prevf = 0, nextf = 0, need = (uint32_t)qm;
                    for (int i2 = idx - 1; i2 >= i0 && need; i2--) {
                        const int k2 = evk[i2];
                        if (k2 < 0) continue;
                        const int d = k - k2;
                        if (d > win - 1) need &= ~3u;
                        if (d > small_win - 1) need &= ~12u;
                        const uint32_t f = (uint32_t)evq[i2] & need;
                        prevf |= f;
                        need &= ~f;
                    }
                    need = (uint32_t)qm;
                    for (int i2 = idx + 1; i2 < i1 && need; i2++) {
                        const int k2 = evk[i2];
                        if (k2 < 0) continue;
                        const int d = k2 - k;
                        if (d > win - 1) need &= ~3u;
                        if (d > small_win - 1) need &= ~12u;
                        const uint32_t f = (uint32_t)evq[i2] & need;
                        nextf |= f;
                        need &= ~f;
                    }
                    if constexpr (MATES) {
                        if (en_mate[lo] >= 0) {
                            const int32_t p = ev_pos[en_e0[lo] + (idx - i0)];
                            mate_neighbours(mt, en_mate[lo], p, k, (uint32_t)qm, win, small_win, ev_off, ev_pos, ev_len, c.lo, b_hi, rkf, prevf, nextf);
                        }
                    }
#pragma unroll
                    for (int cls = 0; cls < 4; cls++) {
                        if (!((qm >> cls) & 1)) continue;
                        const int w = cls < 2 ? win : small_win;
                        if constexpr (MATES) {                               // (h = 2: the name is in both hap sets)
                            for (int hh = (h == 1 ? 1 : 0); hh <= (h == 0 ? 0 : 1); hh++) {
                                if (!((prevf >> cls) & 1)) dif_add(cls * 2 + hh, max(k, k0) - k0);
                                if (!((nextf >> cls) & 1) && max(k + w, k0) - k0 < nk) dif_sub(cls * 2 + hh, max(k + w, k0) - k0);
                            }
                            continue;
                        }
                        if (!((prevf >> cls) & 1)) dif_add(cls * 2 + h, max(k, k0) - k0);
                        if (!((nextf >> cls) & 1) && max(k + w, k0) - k0 < nk) dif_sub(cls * 2 + h, max(k + w, k0) - k0);
                    }
                }
            } else
            for (int idx = tid; idx < total; idx += EV_NT) {                        // (a batch of more events than the LDS arrays hold: straight from HBM)
                int lo = 0, hi = 255;                                             // last entry whose prefix is <= idx
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (en_pre[mid] <= idx) lo = mid; else hi = mid - 1;
                }
                const int j = lo, ef = en_e0[j], el = en_lim[j], h = en_h[j];
                const int ev = ef + (idx - en_pre[j]);
                const int32_t p = ev_pos[ev], sl = ev_len[ev];
                const int k = rkf(p);
                if (k < 0) continue;                                              // excluded column
                uint32_t m_prev = 0, m_next = 0;
                if constexpr (MATES) {
                    if (en_mate[j] >= 0) mate_neighbours(mt, en_mate[j], p, k, ev_qmask(sl), win, small_win, ev_off, ev_pos, ev_len, c.lo, b_hi, rkf, m_prev, m_next);
                }
#pragma unroll
                for (int cls = 0; cls < 4; cls++) {
                    if (!qualifies(sl, cls)) continue;
                    const int w = cls < 2 ? win : small_win;
                    bool has_prev = MATES && ((m_prev >> cls) & 1), has_next = MATES && ((m_next >> cls) & 1);
                    for (int e2 = ev - 1; e2 >= ef; e2--) {
                        const int k2 = rkf(ev_pos[e2]);
                        if (k2 < 0) continue;
                        if (k - k2 > w - 1) break;
                        if (qualifies(ev_len[e2], cls)) { has_prev = true; break; }
                    }
                    for (int e2 = ev + 1; e2 < el; e2++) {
                        const int k2 = rkf(ev_pos[e2]);
                        if (k2 < 0) continue;
                        if (k2 - k > w - 1) break;
                        if (qualifies(ev_len[e2], cls)) { has_next = true; break; }
                    }
                    // ends clipped to the block's first rank: a margin event whose own window stops short of the block may still open the
                    // chain a later margin event continues into it (+1 and -1 on rank k0 cancel when nothing does)
                    if constexpr (MATES) {
                        for (int hh = (h == 1 ? 1 : 0); hh <= (h == 0 ? 0 : 1); hh++) {
                            if (!has_prev) dif_add(cls * 2 + hh, max(k, k0) - k0);
                            if (!has_next && max(k + w, k0) - k0 < nk) dif_sub(cls * 2 + hh, max(k + w, k0) - k0);
                        }
                        continue;
                    }
                    if (!has_prev) dif_add(cls * 2 + h, max(k, k0) - k0);
                    if (!has_next && max(k + w, k0) - k0 < nk) dif_sub(cls * 2 + h, max(k + w, k0) - k0);
                }
            }
            __syncthreads();
        }
    }
    const uint16_t *depth = reinterpret_cast<const uint16_t *>(ck_depth(ws, c));
    constexpr int DCOL = EV_SUB / EV_NT;
    int dn0[DCOL], dn1[DCOL];
#pragma unroll
    for (int u = 0; u < DCOL; u++) {                                 // (all of a thread's depth loads in one round trip, under the scan)
        const int i = b_lo + tid + u * EV_NT;
        dn0[u] = i <= b_hi ? (int)depth[i - c.lo] : 0;
        dn1[u] = i <= b_hi ? (int)depth[c.ncol + (i - c.lo)] : 0;
    }
    // the decision tables over the batch's event ranks (free now); the barrier after the scan publishes them
    uint16_t *dtab = reinterpret_cast<uint16_t *>(evk);
    static_assert(sizeof(int32_t) * EV_CAP >= 2 * DEC_N * sizeof(uint16_t), "k_event_tiles: the decision tables fit the event ranks' array");
    for (int i = tid; i < 2 * DEC_N / 2; i += EV_NT) reinterpret_cast<uint32_t *>(dtab)[i] = reinterpret_cast<const uint32_t *>(dec_tab)[i];
    // ---- inclusive scan of the eight rows: dif becomes U[class, haplotype][rank - k0]
    // a wave per row: each lane sums 16 consecutive ranks, one scan over the 64 lane totals, then the lane's 16 window counts (in place)
    for (int row = wv; row < 8; row += EV_NT / 64) {
        int v[EV_SUB / 64], tot = 0;
#pragma unroll
        for (int q = 0; q < EV_SUB / 64; q++) {
            const int i = lane * (EV_SUB / 64) + q;
            v[q] = i < nk ? (int)((difw[row][i >> 1] >> (16 * (i & 1))) & 0xffffu) - 0x4000 : 0;
            tot += v[q];
        }
        int inc = tot;
        inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
        int run = inc - tot;
        uint16_t *U16 = reinterpret_cast<uint16_t *>(&difw[row][0]);        // the window counts (0 .. reads of the block) over the fields they came from:
#pragma unroll                                                        // a lane rewrites the 16 ranks (8 words) it has just read
        for (int q = 0; q < EV_SUB / 64; q++) {
            run += v[q];
            U16[lane * (EV_SUB / 64) + q] = (uint16_t)run;
        }
    }
    __syncthreads();
    // the columns' decisions (k_indel_decide_b's, without the window counts' trip through HBM)
#pragma unroll
    for (int u = 0; u < DCOL; u++) {
        const int i = b_lo + tid + u * EV_NT;
        if (i > b_hi) break;
        const int k = rkw[i - w_lo];
        const int n0 = dn0[u], n1 = dn1[u];
        col_type[i - c.lo] = indel_decide_tab(k, n0, n1, [&](int cls, int h) { return (int)reinterpret_cast<const uint16_t *>(&difw[cls * 2 + h][0])[k - k0]; },
                                              mincov, ins_t, del_t, haploid, dtab, dtab + DEC_N, dec_n);
    }
}

}   // namespace

// k_blk_base, the cursor and decision tables (made at a pack's first group, reused by its later ones), k_event_tiles
int nc_indel_launch_tiles(nc_ctx *ctx, const IndelGroup &g, const IndelPipeIn &pipe)
{
    const nc_readpack *pack = g.pack;
    const nc_indel_events *ev = g.ev;
    const nc_indel_scan_params *prm = g.prm;
    const int tile = pack->tile_size, SPT = tile / EV_SUB;
    const IndelMates mt = pipe.mates.n > 0 ? pipe.mates : IndelMates{nullptr, nullptr, 0};
    int32_t *blk_chunk = g.blk, *blk_yield = g.blk + g.nblk, *blk_base = g.blk + 2 * (size_t)g.nblk;
    NC_TRY(nc_indel_launch_depths(ctx, g, blk_yield, mt));
    hipLaunchKernelGGL(k_blk_base, dim3((g.ng + 3) / 4), dim3(256), 0, ctx->stream, g.ck_dev, g.ng, g.nblk, blk_yield, blk_base, g.ws);
    const size_t tab_words = (size_t)pack->n_entries * (size_t)(NC_ENT_CUR_PITCH(SPT) + 1) + 2 * DEC_N / 2;
    const size_t rc_words = (size_t)(pack->codes_len >> 10) + (size_t)(2 * SPT + 2) * (size_t)ev->n_reads + 8;      // per table (rc_off)
    const bool have = pipe.reuse_tables && ctx->k7.ent_of == pack->tile_ent && ctx->k7.ent_read.p;
    if (!have) NC_TRY(nc_ensure(ctx, ctx->k7.ent_read, 4 * (tab_words + 2 * rc_words)));
    int32_t *ent_read = (int32_t *)ctx->k7.ent_read.p, *ent_cur = ent_read + pack->n_entries;
    uint16_t *dec_tab = reinterpret_cast<uint16_t *>(ent_cur + (size_t)pack->n_entries * NC_ENT_CUR_PITCH(SPT));
    if (!have) {
        int32_t *rc_lo = ent_read + tab_words, *rc_hi = rc_lo + rc_words;
        hipLaunchKernelGGL(k_read_cursors, dim3((unsigned)((ev->n_reads + 3) / 4)), dim3(256), 0, ctx->stream, ev->n_reads, pipe.rd_start, pipe.rd_end,
                           pipe.slot_off, ev->ev_off, ev->ev_pos, pack->tile_pos0, tile, rc_lo, rc_hi);
        hipLaunchKernelGGL(k_entry_rows, dim3((unsigned)pack->n_tiles), dim3(64), 0, ctx->stream, pack->tile_off, pack->tile_ent, pack->tile_pos0, tile,
                           pipe.slot_off, ev->n_reads, ev->ev_off, rc_lo, rc_hi, pipe.rd_start, pipe.rd_end, ent_read, ent_cur);
        hipLaunchKernelGGL(k_decide_tables, dim3(2 * DEC_N / 256), dim3(256), 0, ctx->stream, prm->del_t, prm->ins_t, dec_tab);
    }
    // depths the tables serve (NC_K7_DEC_N < 1024: tests send ordinary depths down the division form; read per call)
    const char *dn = getenv("NC_K7_DEC_N");
    const int32_t dec_n = dn ? std::max(0, std::min(DEC_N, atoi(dn))) : DEC_N;
    ctx->k7.ent_of = pack->tile_ent;                                  // (the device pipeline's k_sets / k_windows use the tables too)
    ctx->k7.ent_spt = SPT;
    auto kernel = mt.n > 0 ? k_event_tiles<true> : k_event_tiles<false>;
    hipLaunchKernelGGL(kernel, dim3(g.nblk * SPT), dim3(EV_NT), 0, ctx->stream, pack->tile_off, pack->tile_ent, pack->tile_pos0, tile,
                       ent_read, ent_cur, ev->ev_off, ev->ev_pos, ev->ev_len, ev->read_hap, g.ck_dev, blk_chunk, g.ws, prm->win_size,
                       prm->small_win_size, prm->haploid, prm->mincov, prm->ins_t, prm->del_t, g.ctype, pipe.err_bits, dec_tab, blk_base, dec_n, mt);
    return NC_OK;
}

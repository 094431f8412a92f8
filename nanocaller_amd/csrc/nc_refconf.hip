// Reference-confidence blocks of a gVCF (gfx950): per-column counts from the resident read pack, the blocks of one GQ band between the variant
// records, and their record text.  The model is stated in include/nanocaller_hip.h and DESIGN.md section 21; all of it is integer arithmetic.
//
//   k_rc_columns   streams the pack once the way k_scan does (one workgroup per tile, 16 columns per lane, aligned 16-byte loads, byte-lane
//                  accumulators widened every 255 reads) and counts two planes: "present" and "equals the column's own reference code" (the codes
//                  XORed with the reference bytes: a match is byte 0).  One uint32 per column, n | alt << 16.
//   k_rc_blocks    16 columns per lane, 4096 per workgroup.  A block's aggregate is a segmented reduction (a head column resets it) of two minima:
//                  n, and (GQ << 32 | column).  <false>: the workgroup's summary and its number of heads; k_rc_tile_scan: the exclusive segmented scan
//                  of the summaries in one single-workgroup launch (a block may span thousands of workgroups); <true>: the same walk with the carry,
//                  every block written by the lanes that hold its head (start) and its tail (everything else) at the head's rank.
//   k_rc_line_len / k_rc_scan64 / k_rc_line_add / k_rc_line_write   the records' text: line lengths from digit counts, their prefix sum, the bytes.
#include <algorithm>
#include <vector>

#include "nc_common.h"

struct nc_refconf_state {
    DevBuf cut_bits, tile_sum, tile_pre, region, totals, blocks, wg_sum;
    // what nc_refconf_blocks leaves for nc_refconf_fetch
    bool have = false;
    const uint32_t *words = nullptr;
    int32_t tile_pos0 = 0, n_region = 0, n_tiles = 0;
    int64_t npos = 0, n_blocks = 0;
    nc_refconf_params prm;
};

namespace {

constexpr int RC_BLOCK = 256, RC_TILE = RC_BLOCK * 16;
constexpr int RC_CLOSED = 31;                                  // the state of a column that is not open (0: no-call, 1 + band: called)

__device__ __forceinline__ uint32_t lut8(uint32_t x, uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, x); }

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_rc_columns(const uint8_t *__restrict__ codes, const int32_t *__restrict__ tile_off,
                                                      const nc_tile_entry *__restrict__ tile_ent, int32_t tile_pos0,
                                                      const uint8_t *__restrict__ ref_code, uint32_t *__restrict__ words)
{
    constexpr int TILE = BLOCK * 16;
    const int t = blockIdx.x;
    const int64_t col0 = (int64_t)t * TILE + threadIdx.x * 16;
    const int32_t P0 = (int32_t)((int64_t)tile_pos0 + col0);
    const uint4 rv = *reinterpret_cast<const uint4 *>(ref_code + col0);
    const uint32_t rw[4] = {rv.x, rv.y, rv.z, rv.w};
    uint32_t rx[4];                                            // the XOR mask: codes and masked reference bytes stay selectors 0..7
#pragma unroll
    for (int d = 0; d < 4; d++) rx[d] = rw[d] & 0x07070707u;
    uint32_t acc_n[4] = {0, 0, 0, 0}, acc_r[4] = {0, 0, 0, 0};
    uint32_t wide_n[8], wide_r[8];
#pragma unroll
    for (int d = 0; d < 8; d++) wide_n[d] = wide_r[d] = 0;
    const int e0 = tile_off[t], e1 = tile_off[t + 1];
    int e = e0;
    while (e < e1) {
        const int lim = min(e1, e + 255);
#pragma unroll 8
        for (; e < lim; e++) {
            const nc_tile_entry ent = tile_ent[e];            // wave-uniform -> scalar loads
            const int32_t lo = ent.start & ~15, hi = (ent.end + 15) & ~15;
            uint4 v = make_uint4(0x07070707u, 0x07070707u, 0x07070707u, 0x07070707u);
            if (P0 >= lo && P0 < hi) v = *reinterpret_cast<const uint4 *>(codes + (ent.base_flag & ~int64_t(15)) + P0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < 4; d++) {
                acc_n[d] += lut8(w[d], 0x01010101u, 0x00000001u);          // codes 0..4
                acc_r[d] += lut8(w[d] ^ rx[d], 0x00000001u, 0u);           // code == reference code (absent 7 and deletion 4 never XOR to 0 with r < 4)
            }
        }
#pragma unroll
        for (int d = 0; d < 4; d++) {
            wide_n[2 * d] += acc_n[d] & 0x00FF00FFu;                       // positions 4d+0 (lo16), 4d+2 (hi16)
            wide_n[2 * d + 1] += (acc_n[d] >> 8) & 0x00FF00FFu;            // positions 4d+1, 4d+3
            wide_r[2 * d] += acc_r[d] & 0x00FF00FFu;
            wide_r[2 * d + 1] += (acc_r[d] >> 8) & 0x00FF00FFu;
            acc_n[d] = acc_r[d] = 0;
        }
    }
    uint32_t out[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int d = i >> 2, k = i & 3;
        const int wi = 2 * d + (k & 1), sh = (k >> 1) * 16;
        const uint32_t r = (rw[d] >> (8 * k)) & 0xFF;
        const uint32_t n = (wide_n[wi] >> sh) & 0xFFFF, rf = (wide_r[wi] >> sh) & 0xFFFF;
        out[i] = r < 4 ? (n | ((n - rf) << 16)) : 0xFFFFFFFFu;
    }
    uint4 *o = reinterpret_cast<uint4 *>(words + col0);
#pragma unroll
    for (int d = 0; d < 4; d++) o[d] = make_uint4(out[4 * d], out[4 * d + 1], out[4 * d + 2], out[4 * d + 3]);
}

// ------------------------------------------------------------------ blocks
struct RcP {
    int32_t cm, cx, ch, haploid, n_bands;
    int32_t band[16];
};

// (what crosses lanes, waves and workgroups) a run's aggregate since its last head: F = the run holds a head
struct RcAgg {
    int32_t F;
    int32_t dp;
    unsigned long long key;
};
struct RcTile {                                                // 24 bytes
    int32_t F, heads, dp, pad;
    unsigned long long key;
};

__device__ __forceinline__ RcAgg rc_identity() { return RcAgg{0, INT32_MAX, ~0ull}; }
// a (earlier) then b (later)
__device__ __forceinline__ RcAgg rc_combine(const RcAgg &a, const RcAgg &b)
{
    if (b.F) return b;
    return RcAgg{a.F, min(a.dp, b.dp), a.key < b.key ? a.key : b.key};
}

// inclusive segmented scan over the 64 lanes of a wave
__device__ __forceinline__ RcAgg rc_wave_incl(RcAgg v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        RcAgg p;
        p.F = __shfl_up(v.F, off);
        p.dp = __shfl_up(v.dp, off);
        p.key = __shfl_up(v.key, off);
        if (lane >= off) v = rc_combine(p, v);
    }
    return v;
}

// the column's state (0 no-call, 1 + band) and GQ from its word
__device__ __forceinline__ int rc_classify(uint32_t w, const RcP &p, const uint8_t *band_lut, uint32_t &gq)
{
    const int64_t n = w & 0xFFFF, alt = w >> 16, ref = n - alt;
    const int64_t s00 = ref * p.cm + alt * p.cx, s11 = ref * p.cx + alt * p.cm, s01 = n * p.ch;
    const int64_t other = p.haploid ? s11 : (s01 < s11 ? s01 : s11);
    gq = 0;
    if (n == 0 || s00 > other) return 0;
    const int64_t d = other - s00;
    gq = d >= 99000 ? 99u : (uint32_t)d / 1000u;
    return 1 + band_lut[gq];
}

// is grid column g inside the region (n_reg sorted disjoint intervals [ra, rb] in grid columns)?  -> index of the first interval with rb >= g
__device__ __forceinline__ int rc_region_lb(const int32_t *__restrict__ rb, int n_reg, int64_t g)
{
    int lo = 0, hi = n_reg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rb[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the state of ONE grid column (the column in front of a lane's 16 and the one behind them)
__device__ __forceinline__ int rc_col_state(int64_t g, int64_t npos, const uint32_t *__restrict__ words, const uint16_t *__restrict__ cut16,
                                            const int32_t *__restrict__ ra, const int32_t *__restrict__ rb, int n_reg, const RcP &p,
                                            const uint8_t *band_lut)
{
    if (g < 0 || g >= npos) return RC_CLOSED;
    const int k = rc_region_lb(rb, n_reg, g);
    if (k >= n_reg || ra[k] > g) return RC_CLOSED;
    if ((cut16[g >> 4] >> (g & 15)) & 1) return RC_CLOSED;
    const uint32_t w = words[g];
    if (w == 0xFFFFFFFFu) return RC_CLOSED;
    uint32_t gq;
    return rc_classify(w, p, band_lut, gq);
}

template <bool WRITE>
__global__ __launch_bounds__(RC_BLOCK) void k_rc_blocks(const uint32_t *__restrict__ words, int32_t tile_pos0, int64_t npos,
                                                        const uint16_t *__restrict__ cut16, const int32_t *__restrict__ ra,
                                                        const int32_t *__restrict__ rb, int n_reg, RcP p, RcTile *__restrict__ tile_sum,
                                                        const RcTile *__restrict__ tile_pre, int32_t *__restrict__ out, int64_t n_blocks)
{
    __shared__ uint8_t band_lut[128];
    __shared__ RcAgg wagg[RC_BLOCK / 64];
    __shared__ int32_t wcnt[RC_BLOCK / 64];
    if (threadIdx.x < 100) {
        int b = 0;
        for (int k = 1; k < p.n_bands; k++)
            if (p.band[k] <= (int)threadIdx.x) b = k;
        band_lut[threadIdx.x] = (uint8_t)b;
    }
    __syncthreads();
    const int t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t g0 = (int64_t)t * RC_TILE + threadIdx.x * 16;

    // the lane's 16 columns: state, n, GQ
    uint8_t st[16];
    uint16_t cn[16];
    uint8_t cg[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { st[i] = RC_CLOSED; cn[i] = 0; cg[i] = 0; }
    int prev = RC_CLOSED, next = RC_CLOSED;
    if (g0 < npos) {                                           // (npos is a multiple of 16: a lane is inside the grid or outside it)
        uint32_t open = 0;
        for (int k = rc_region_lb(rb, n_reg, g0); k < n_reg && ra[k] <= g0 + 15; k++) {
            const int a = (int)(max((int64_t)ra[k], g0) - g0), b = (int)(min((int64_t)rb[k], g0 + 15) - g0);
            open |= (0xFFFFu >> (15 - b)) & (0xFFFFu << a);
        }
        open &= ~(uint32_t)cut16[g0 >> 4] & 0xFFFFu;
        const uint4 *wp = reinterpret_cast<const uint4 *>(words + g0);
        uint32_t w[16];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint4 v = wp[d];
            w[4 * d] = v.x; w[4 * d + 1] = v.y; w[4 * d + 2] = v.z; w[4 * d + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (((open >> i) & 1) && w[i] != 0xFFFFFFFFu) {
                uint32_t gq;
                st[i] = (uint8_t)rc_classify(w[i], p, band_lut, gq);
                cn[i] = (uint16_t)(w[i] & 0xFFFF);
                cg[i] = (uint8_t)gq;
            }
        }
        prev = rc_col_state(g0 - 1, npos, words, cut16, ra, rb, n_reg, p, band_lut);
        next = rc_col_state(g0 + 16, npos, words, cut16, ra, rb, n_reg, p, band_lut);
    }

    // the lane's own aggregate and number of heads
    RcAgg mine = rc_identity();
    int heads = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (st[i] == RC_CLOSED) continue;
        const int before = i ? st[i - 1] : prev;
        const RcAgg el{1, (int32_t)cn[i], ((unsigned long long)cg[i] << 32) | (uint32_t)(g0 + i)};
        if (before != st[i]) { mine = el; heads++; }
        else mine = RcAgg{mine.F, min(mine.dp, el.dp), mine.key < el.key ? mine.key : el.key};
    }
    const RcAgg incl = rc_wave_incl(mine, lane);
    const int hincl = nc_wave_incl_scan(heads);
    if (lane == 63) { wagg[wv] = incl; wcnt[wv] = hincl; }
    __syncthreads();
    RcAgg carry = rc_identity();
    int hpre = 0;
    if constexpr (WRITE) {
        const RcTile tp = tile_pre[t];
        carry = RcAgg{tp.F, tp.dp, tp.key};
        hpre = tp.heads;
    }
    RcAgg tot = rc_identity();
    int htot = 0;
#pragma unroll
    for (int k = 0; k < RC_BLOCK / 64; k++) {
        if (k < wv) { carry = rc_combine(carry, wagg[k]); hpre += wcnt[k]; }
        tot = rc_combine(tot, wagg[k]);
        htot += wcnt[k];
    }
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) tile_sum[t] = RcTile{tot.F, htot, tot.dp, 0, tot.key};
        return;
    } else {
        RcAgg ex;
        ex.F = __shfl_up(incl.F, 1);
        ex.dp = __shfl_up(incl.dp, 1);
        ex.key = __shfl_up(incl.key, 1);
        if (lane == 0) ex = rc_identity();
        RcAgg cur = rc_combine(carry, ex);
        int64_t idx = (int64_t)hpre + hincl - heads;           // heads in front of this lane
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (st[i] == RC_CLOSED) continue;
            const int before = i ? st[i - 1] : prev, after = i < 15 ? st[i + 1] : next;
            const int32_t pos = (int32_t)((int64_t)tile_pos0 + g0 + i);
            const RcAgg el{1, (int32_t)cn[i], ((unsigned long long)cg[i] << 32) | (uint32_t)(g0 + i)};
            if (before != st[i]) {
                cur = el;
                if (idx >= 0 && idx < n_blocks) out[idx * 6] = pos;
                idx++;
            } else {
                cur = RcAgg{1, min(cur.dp, el.dp), cur.key < el.key ? cur.key : el.key};
            }
            if (after != st[i]) {
                const int64_t b = idx - 1;
                const int64_t at = (int64_t)(uint32_t)cur.key;    // the leftmost column that attains the block's minimum GQ
                if (b >= 0 && b < n_blocks && at < npos) {
                    const uint32_t w = words[at];
                    out[b * 6 + 1] = pos;
                    out[b * 6 + 2] = cur.dp;
                    out[b * 6 + 3] = (int32_t)(cur.key >> 32);
                    out[b * 6 + 4] = (int32_t)(w & 0xFFFF);
                    out[b * 6 + 5] = (int32_t)(w >> 16);
                }
            }
        }
    }
}

// exclusive segmented scan of the workgroup summaries + exclusive prefix of their head counts, one workgroup: a thread owns a contiguous run
__global__ __launch_bounds__(1024) void k_rc_tile_scan(const RcTile *__restrict__ sum, RcTile *__restrict__ pre, int n, int64_t *__restrict__ totals)
{
    __shared__ RcAgg wagg[16];
    __shared__ int32_t wcnt[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per = (n + 1023) / 1024;
    const int b0 = min(n, (int)threadIdx.x * per), b1 = min(n, b0 + per);
    RcAgg mine = rc_identity();
    int heads = 0;
    for (int i = b0; i < b1; i++) {
        const RcTile s = sum[i];
        mine = rc_combine(mine, RcAgg{s.F, s.dp, s.key});
        heads += s.heads;
    }
    const RcAgg incl = rc_wave_incl(mine, lane);
    const int hincl = nc_wave_incl_scan(heads);
    if (lane == 63) { wagg[wv] = incl; wcnt[wv] = hincl; }
    __syncthreads();
    RcAgg carry = rc_identity();
    int hpre = 0, htot = 0;
    for (int k = 0; k < 16; k++) {
        if (k < wv) { carry = rc_combine(carry, wagg[k]); hpre += wcnt[k]; }
        htot += wcnt[k];
    }
    RcAgg ex;
    ex.F = __shfl_up(incl.F, 1);
    ex.dp = __shfl_up(incl.dp, 1);
    ex.key = __shfl_up(incl.key, 1);
    if (lane == 0) ex = rc_identity();
    RcAgg cur = rc_combine(carry, ex);
    int hc = hpre + hincl - heads;
    for (int i = b0; i < b1; i++) {
        const RcTile s = sum[i];
        pre[i] = RcTile{cur.F, hc, cur.dp, 0, cur.key};
        cur = rc_combine(cur, RcAgg{s.F, s.dp, s.key});
        hc += s.heads;
    }
    if (threadIdx.x == 0) totals[0] = htot;
}

// the cut intervals as a bitmap on the grid (zeroed before): one thread per interval, whole 32-bit words at a time
__global__ __launch_bounds__(256) void k_rc_cut_bits(int32_t n, const int32_t *__restrict__ cs, const int32_t *__restrict__ ce, int32_t tile_pos0,
                                                     int64_t npos, uint32_t *__restrict__ bits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t a = max((int64_t)cs[i] - tile_pos0, (int64_t)0), b = min((int64_t)ce[i] - tile_pos0, npos - 1);
    for (int64_t g = a; g <= b;) {
        const int64_t word = g >> 5;
        const int lo = (int)(g & 31), hi = (int)min((int64_t)31, b - (word << 5));
        atomicOr(&bits[word], (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo));
        g = (word + 1) << 5;
    }
}

// ------------------------------------------------------------------ text
struct RcChrom {
    int32_t len;
    char c[256];
};

__device__ __forceinline__ int rc_digits(uint32_t v)
{
    int d = 1;
    if (v >= 10u) d = 2;
    if (v >= 100u) d = 3;
    if (v >= 1000u) d = 4;
    if (v >= 10000u) d = 5;
    if (v >= 100000u) d = 6;
    if (v >= 1000000u) d = 7;
    if (v >= 10000000u) d = 8;
    if (v >= 100000000u) d = 9;
    if (v >= 1000000000u) d = 10;
    return d;
}

__device__ __forceinline__ uint8_t *rc_put_uint(uint8_t *o, uint32_t v)
{
    const int d = rc_digits(v);
    for (int k = d - 1; k >= 0; k--) {
        o[k] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return o + d;
}

__device__ __forceinline__ uint8_t *rc_put_str(uint8_t *o, const char *s, int n)
{
    for (int k = 0; k < n; k++) o[k] = (uint8_t)s[k];
    return o + n;
}

__device__ __forceinline__ uint32_t rc_pl(int64_t d) { return d >= 9999000 ? 9999u : (uint32_t)d / 1000u; }

// a block's genotype fields from n and alt of its column of minimum GQ: -> no-call?, pl[3] (two of them when haploid)
__device__ __forceinline__ bool rc_fields(int32_t n_at, int32_t alt_at, const RcP &p, uint32_t pl[3])
{
    const int64_t n = n_at, alt = alt_at, ref = n - alt;
    const int64_t s00 = ref * p.cm + alt * p.cx, s11 = ref * p.cx + alt * p.cm, s01 = n * p.ch;
    const int64_t other = p.haploid ? s11 : (s01 < s11 ? s01 : s11);
    const int64_t m = s00 < other ? s00 : other;
    pl[0] = rc_pl(s00 - m);
    if (p.haploid) { pl[1] = rc_pl(s11 - m); pl[2] = 0; }
    else { pl[1] = rc_pl(s01 - m); pl[2] = rc_pl(s11 - m); }
    return n == 0 || s00 > other;
}

__device__ __forceinline__ int rc_line_len(const int32_t *b, const RcP &p, int chrom_len)
{
    uint32_t pl[3];
    rc_fields(b[4], b[5], p, pl);
    // CHROM \t start "\t.\tR\t" "<*>\t0\t.\tEND=" end "\tGT:GQ:MIN_DP:PL\t" GT : gq : min_dp : pl0 , pl1 [, pl2] \n
    int len = chrom_len + 1 + rc_digits((uint32_t)b[0]) + 5 + 12 + rc_digits((uint32_t)b[1]) + 17 + (p.haploid ? 1 : 3) + 1 + rc_digits((uint32_t)b[3]) + 1 +
              rc_digits((uint32_t)b[2]) + 1 + rc_digits(pl[0]) + 1 + rc_digits(pl[1]) + 1;
    if (!p.haploid) len += 1 + rc_digits(pl[2]);
    return len;
}

// line lengths and their exclusive prefix inside a workgroup of 1024 lines; the workgroup's total to wg_sum
__global__ __launch_bounds__(1024) void k_rc_line_len(int64_t n, const int32_t *__restrict__ blocks, RcP p, int chrom_len, int64_t *__restrict__ line_off,
                                                      int64_t *__restrict__ wg_sum)
{
    __shared__ int32_t wsum[16];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int len = 0;
    if (i < n) {
        int32_t b[6];
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = blocks[i * 6 + k];
        len = rc_line_len(b, p, chrom_len);
    }
    const int incl = nc_wave_incl_scan(len);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int k = 0; k < 16; k++) {
        if (k < wv) pre += wsum[k];
        tot += wsum[k];
    }
    if (i < n) line_off[i] = pre + incl - len;
    if (threadIdx.x == 0) wg_sum[blockIdx.x] = tot;
}

// in-place exclusive scan of n int64 sums by one workgroup (a thread owns a contiguous run); the total to totals[1]
__global__ __launch_bounds__(1024) void k_rc_scan64(int64_t *__restrict__ v, int n, int64_t *__restrict__ totals)
{
    __shared__ long long wsum[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per = (n + 1023) / 1024;
    const int b0 = min(n, (int)threadIdx.x * per), b1 = min(n, b0 + per);
    long long mine = 0;
    for (int i = b0; i < b1; i++) mine += v[i];
    long long incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long q = __shfl_up(incl, off);
        if (lane >= off) incl += q;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    long long pre = 0, tot = 0;
    for (int k = 0; k < 16; k++) {
        if (k < wv) pre += wsum[k];
        tot += wsum[k];
    }
    long long cur = pre + incl - mine;
    for (int i = b0; i < b1; i++) {
        const long long x = v[i];
        v[i] = cur;
        cur += x;
    }
    if (threadIdx.x == 0) totals[1] = tot;
}

__global__ __launch_bounds__(1024) void k_rc_line_add(int64_t n, int64_t *__restrict__ line_off, const int64_t *__restrict__ wg_sum,
                                                      const int64_t *__restrict__ totals)
{
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    if (i < n) line_off[i] += wg_sum[blockIdx.x];
    if (i == n) line_off[n] = totals[1];
}

__global__ __launch_bounds__(256) void k_rc_line_write(int64_t n, const int32_t *__restrict__ blocks, const uint8_t *__restrict__ ref_code,
                                                       int32_t tile_pos0, int64_t npos, RcP p, RcChrom chrom, const int64_t *__restrict__ line_off,
                                                       uint8_t *__restrict__ text, int64_t text_cap)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t b[6];
#pragma unroll
    for (int k = 0; k < 6; k++) b[k] = blocks[i * 6 + k];
    const int64_t o0 = line_off[i], o1 = line_off[i + 1];
    // the offsets must be the ones k_rc_line_len made for these very blocks: a line that would not fit its slot is not written
    if (o0 < 0 || o1 > text_cap || o1 - o0 != rc_line_len(b, p, chrom.len)) return;
    uint32_t pl[3];
    const bool nocall = rc_fields(b[4], b[5], p, pl);
    const int64_t g = (int64_t)b[0] - tile_pos0;
    const uint32_t r = g >= 0 && g < npos ? ref_code[g] : 4u;
    uint8_t *o = text + o0;
    o = rc_put_str(o, chrom.c, chrom.len);
    *o++ = '\t';
    o = rc_put_uint(o, (uint32_t)b[0]);
    *o++ = '\t'; *o++ = '.'; *o++ = '\t';
    *o++ = r < 4 ? (uint8_t)"AGTC"[r] : (uint8_t)'N';
    *o++ = '\t';
    o = rc_put_str(o, "<*>\t0\t.\tEND=", 12);
    o = rc_put_uint(o, (uint32_t)b[1]);
    o = rc_put_str(o, "\tGT:GQ:MIN_DP:PL\t", 17);
    if (p.haploid) *o++ = nocall ? '.' : '0';
    else { *o++ = nocall ? '.' : '0'; *o++ = '/'; *o++ = nocall ? '.' : '0'; }
    *o++ = ':';
    o = rc_put_uint(o, (uint32_t)b[3]);
    *o++ = ':';
    o = rc_put_uint(o, (uint32_t)b[2]);
    *o++ = ':';
    o = rc_put_uint(o, pl[0]);
    *o++ = ',';
    o = rc_put_uint(o, pl[1]);
    if (!p.haploid) { *o++ = ','; o = rc_put_uint(o, pl[2]); }
    *o++ = '\n';
}

int rc_params(nc_ctx *ctx, const nc_refconf_params *params, RcP &p)
{
    if (!params || params->n_bands < 1 || params->n_bands > 16 || params->band[0] != 0 || params->c_m < 0 || params->c_x < 0 || params->c_h < 0)
        return nc_fail(ctx, NC_ERR_ARG, "nc_refconf: bad parameters (1..16 band edges, the first one 0; constants >= 0)");
    for (int k = 1; k < params->n_bands; k++)
        if (params->band[k] <= params->band[k - 1]) return nc_fail(ctx, NC_ERR_ARG, "nc_refconf: band edges must ascend");
    p.cm = params->c_m; p.cx = params->c_x; p.ch = params->c_h;
    p.haploid = params->haploid ? 1 : 0;
    p.n_bands = params->n_bands;
    for (int k = 0; k < 16; k++) p.band[k] = k < params->n_bands ? params->band[k] : INT32_MAX;
    return NC_OK;
}

nc_refconf_state *rc_state(nc_ctx *ctx)
{
    if (!ctx->refconf) ctx->refconf = new nc_refconf_state();
    return ctx->refconf;
}

}   // namespace

void nc_refconf_destroy(nc_ctx *ctx)
{
    delete ctx->refconf;                                          // (its DevBufs free themselves; the device is current)
    ctx->refconf = nullptr;
}

extern "C" {

int nc_refconf_columns(nc_ctx *ctx, const nc_readpack *pack, const uint8_t *d_ref_code, int32_t tile_pos0, int64_t npos, uint32_t *d_words)
{
    if (!ctx) return NC_ERR_ARG;
    if (!pack || !d_ref_code || !d_words) return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_columns: null argument");
    const int tile = pack->tile_size;
    if (!(tile == 1024 || tile == 2048 || tile == 4096) || pack->n_tiles <= 0 || !pack->codes || !pack->tile_off ||
        (pack->n_entries && !pack->tile_ent) || (pack->tile_pos0 & 15))
        return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_columns: malformed read pack");
    if (tile_pos0 != pack->tile_pos0 || npos != (int64_t)pack->n_tiles * tile || ((uintptr_t)d_words & 15) || ((uintptr_t)d_ref_code & 15))
        return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_columns: the words and the reference codes must lie on the pack's tile grid (%d, %lld columns), 16-byte aligned",
                       pack->tile_pos0, (long long)pack->n_tiles * tile);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    if (tile == 1024)
        hipLaunchKernelGGL((k_rc_columns<64>), dim3(pack->n_tiles), dim3(64), 0, ctx->stream, pack->codes, pack->tile_off, pack->tile_ent,
                           pack->tile_pos0, d_ref_code, d_words);
    else if (tile == 2048)
        hipLaunchKernelGGL((k_rc_columns<128>), dim3(pack->n_tiles), dim3(128), 0, ctx->stream, pack->codes, pack->tile_off, pack->tile_ent,
                           pack->tile_pos0, d_ref_code, d_words);
    else
        hipLaunchKernelGGL((k_rc_columns<256>), dim3(pack->n_tiles), dim3(256), 0, ctx->stream, pack->codes, pack->tile_off, pack->tile_ent,
                           pack->tile_pos0, d_ref_code, d_words);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_refconf_blocks(nc_ctx *ctx, const uint32_t *d_words, int32_t tile_pos0, int64_t npos, int32_t n_chunks, const int32_t *chunk_start_host,
                      const int32_t *chunk_end_host, int32_t n_cut, const int32_t *d_cut_start, const int32_t *d_cut_end,
                      const nc_refconf_params *params, int64_t *n_blocks)
{
    if (!ctx) return NC_ERR_ARG;
    if (!d_words || !n_blocks || n_chunks < 0 || (n_chunks && (!chunk_start_host || !chunk_end_host)) || n_cut < 0 ||
        (n_cut && (!d_cut_start || !d_cut_end)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_blocks: null argument");
    if (npos <= 0 || (npos & 15) || npos > (int64_t)INT32_MAX - 4096 || (tile_pos0 & 15) || ((uintptr_t)d_words & 15))
        return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_blocks: the grid must start on a multiple of 16, hold a multiple of 16 columns and be 16-byte aligned");
    RcP p;
    NC_TRY(rc_params(ctx, params, p));
    NC_HIP(ctx, hipSetDevice(ctx->device));
    nc_refconf_state *s = rc_state(ctx);
    s->have = false;
    // the region: the chunks' union in grid columns, sorted, overlapping and abutting intervals merged
    std::vector<std::pair<int64_t, int64_t>> iv;
    for (int c = 0; c < n_chunks; c++) {
        const int64_t a = std::max<int64_t>((int64_t)chunk_start_host[c] - tile_pos0, 0), b = std::min<int64_t>((int64_t)chunk_end_host[c] - tile_pos0, npos - 1);
        if (b >= a) iv.emplace_back(a, b);
    }
    std::sort(iv.begin(), iv.end());
    std::vector<int32_t> reg;                                     // starts, then ends
    {
        std::vector<int32_t> ra, rb;
        for (const auto &x : iv) {
            if (!ra.empty() && x.first <= (int64_t)rb.back() + 1) rb.back() = (int32_t)std::max<int64_t>(rb.back(), x.second);
            else { ra.push_back((int32_t)x.first); rb.push_back((int32_t)x.second); }
        }
        reg = ra;
        reg.insert(reg.end(), rb.begin(), rb.end());
    }
    const int n_reg = (int)(reg.size() / 2);
    const int n_tiles = (int)((npos + RC_TILE - 1) / RC_TILE);
    NC_TRY(nc_ensure(ctx, s->region, reg.size() * 4 + 16));
    NC_TRY(nc_ensure(ctx, s->cut_bits, (size_t)(npos / 8) + 16));
    NC_TRY(nc_ensure(ctx, s->tile_sum, (size_t)n_tiles * sizeof(RcTile)));
    NC_TRY(nc_ensure(ctx, s->tile_pre, (size_t)n_tiles * sizeof(RcTile)));
    NC_TRY(nc_ensure(ctx, s->totals, 16));
    if (n_reg) NC_TRY(nc_h2d_pieces(ctx, s->region.p, reg.data(), reg.size() * 4, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));               // (reg leaves scope; the staging ring copies on call, this is for the large case)
    NC_HIP(ctx, hipMemsetAsync(s->cut_bits.p, 0, (size_t)(npos / 8) + 16, ctx->stream));
    if (n_cut) {
        hipLaunchKernelGGL(k_rc_cut_bits, dim3((n_cut + 255) / 256), dim3(256), 0, ctx->stream, n_cut, d_cut_start, d_cut_end, tile_pos0, npos,
                           (uint32_t *)s->cut_bits.p);
        NC_HIP(ctx, hipGetLastError());
    }
    const int32_t *ra = (const int32_t *)s->region.p, *rb = ra + n_reg;
    hipLaunchKernelGGL((k_rc_blocks<false>), dim3(n_tiles), dim3(RC_BLOCK), 0, ctx->stream, d_words, tile_pos0, npos, (const uint16_t *)s->cut_bits.p,
                       ra, rb, n_reg, p, (RcTile *)s->tile_sum.p, (const RcTile *)nullptr, (int32_t *)nullptr, (int64_t)0);
    NC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rc_tile_scan, dim3(1), dim3(1024), 0, ctx->stream, (const RcTile *)s->tile_sum.p, (RcTile *)s->tile_pre.p, n_tiles,
                       (int64_t *)s->totals.p);
    NC_HIP(ctx, hipGetLastError());
    int64_t tot = 0;
    NC_HIP(ctx, hipMemcpyAsync(&tot, s->totals.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->words = d_words;
    s->tile_pos0 = tile_pos0;
    s->npos = npos;
    s->n_region = n_reg;
    s->n_tiles = n_tiles;
    s->n_blocks = tot;
    s->prm = *params;
    s->have = true;
    *n_blocks = tot;
    return NC_OK;
}

int nc_refconf_fetch(nc_ctx *ctx, int32_t *d_or_host_out)
{
    if (!ctx) return NC_ERR_ARG;
    nc_refconf_state *s = ctx->refconf;
    if (!s || !s->have) return nc_fail(ctx, NC_ERR_STATE, "nc_refconf_fetch: no nc_refconf_blocks on this context");
    s->have = false;
    if (s->n_blocks == 0) return NC_OK;
    if (!d_or_host_out) return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_fetch: null argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipPointerAttribute_t at;
    bool on_device = false;
    if (hipPointerGetAttributes(&at, d_or_host_out) == hipSuccess) on_device = at.type == hipMemoryTypeDevice;
    else (void)hipGetLastError();                                 // an ordinary host pointer is not an error
    const size_t bytes = (size_t)s->n_blocks * 24;
    int32_t *out = d_or_host_out;
    if (!on_device) {
        NC_TRY(nc_ensure(ctx, s->blocks, bytes));
        out = (int32_t *)s->blocks.p;
    }
    RcP p;
    NC_TRY(rc_params(ctx, &s->prm, p));
    const int32_t *ra = (const int32_t *)s->region.p, *rb = ra + s->n_region;
    hipLaunchKernelGGL((k_rc_blocks<true>), dim3(s->n_tiles), dim3(RC_BLOCK), 0, ctx->stream, s->words, s->tile_pos0, s->npos,
                       (const uint16_t *)s->cut_bits.p, ra, rb, s->n_region, p, (RcTile *)nullptr, (const RcTile *)s->tile_pre.p, out, s->n_blocks);
    NC_HIP(ctx, hipGetLastError());
    if (!on_device) NC_HIP(ctx, hipMemcpyAsync(d_or_host_out, out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

int nc_refconf_text(nc_ctx *ctx, int64_t n_blocks, const int32_t *d_blocks, const uint8_t *d_ref_code, int32_t tile_pos0, int64_t npos,
                    const char *chrom, const nc_refconf_params *params, int64_t *d_line_off, uint8_t *d_text, int64_t text_cap, int64_t *n_bytes)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_blocks < 0 || n_blocks > INT32_MAX || !chrom || !d_line_off || (n_blocks && (!d_blocks || !d_ref_code)) || (!d_text && !n_bytes))
        return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_text: bad argument");
    RcP p;
    NC_TRY(rc_params(ctx, params, p));
    RcChrom ch;
    const size_t cl = strlen(chrom);
    if (cl == 0 || cl > sizeof ch.c) return nc_fail(ctx, NC_ERR_ARG, "nc_refconf_text: contig names hold 1..256 bytes");
    memset(&ch, 0, sizeof ch);
    ch.len = (int32_t)cl;
    memcpy(ch.c, chrom, cl);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    nc_refconf_state *s = rc_state(ctx);
    if (!d_text) {
        const int n_wg = (int)((n_blocks + 1 + 1023) / 1024);     // (+ 1: the thread that writes line_off[n_blocks])
        NC_TRY(nc_ensure(ctx, s->wg_sum, (size_t)n_wg * 8));
        NC_TRY(nc_ensure(ctx, s->totals, 16));
        hipLaunchKernelGGL(k_rc_line_len, dim3(n_wg), dim3(1024), 0, ctx->stream, n_blocks, d_blocks, p, ch.len, d_line_off, (int64_t *)s->wg_sum.p);
        NC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_rc_scan64, dim3(1), dim3(1024), 0, ctx->stream, (int64_t *)s->wg_sum.p, n_wg, (int64_t *)s->totals.p);
        NC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_rc_line_add, dim3(n_wg), dim3(1024), 0, ctx->stream, n_blocks, d_line_off, (const int64_t *)s->wg_sum.p,
                           (const int64_t *)s->totals.p);
        NC_HIP(ctx, hipGetLastError());
        int64_t tot = 0;
        NC_HIP(ctx, hipMemcpyAsync(&tot, (const char *)s->totals.p + 8, 8, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *n_bytes = tot;
        return NC_OK;
    }
    if (n_blocks) {
        hipLaunchKernelGGL(k_rc_line_write, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, ctx->stream, n_blocks, d_blocks, d_ref_code,
                           tile_pos0, npos, p, ch, (const int64_t *)d_line_off, d_text, text_cap);
        NC_HIP(ctx, hipGetLastError());
    }
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

}   // extern "C"

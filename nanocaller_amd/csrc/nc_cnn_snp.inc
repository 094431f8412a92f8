// The split-precision kernels of the SNP models (gfx950; see nc_cnn.h), their layout constants and role tables, and the packers of their
// weight fragments:
//   k5_trunk_p3    conv1-conv3, pixel form: float32 tensors, or int16 tensors under NC_TRUNK_LIN=0
//   k5_trunk_lin   the same with conv1 by linearity: int16 tensors (the product path)
//   k6_fc1_h3      fc1
// Both trunks are persistent, wave-specialised, one workgroup per CU, with their weights resident in VGPRs.  The packed blob of a model
// (nc_weights::packed_h) is [H_PACKED_BYTES: both trunks | FC_PACKED_BYTES: k6_fc1_h3 | L_PACKED_BYTES: conv1 of k5_trunk_lin].
#include <cstdlib>

#include <hip/hip_ext.h>

#include "nc_cnn.h"

namespace {

// =====================================================================================================================
// fp16x3 trunk (k5_trunk_p3, k5_trunk_lin): persistent and weight-stationary like k4_conv12, on the 16x-rate matrix pipe.
// Every fp32 operand v is split as v = hi + lo with hi = fp16(v), lo = fp16(v - hi) (22 significand bits) and a product
// is evaluated as hi*hi + hi*lo + lo*hi with fp32 accumulation in v_mfma_f32_16x16x32_f16 (the dropped lo*lo term is
// 2^-22 relative).  Weights are multiplied by a power of two S on the host before splitting, so their low parts stay
// normal fp16 numbers; accumulators carry S*value and are rescaled (exactly) in the epilogue.  Emulated on the CPU
// with the real weights this is indistinguishable from fp32 rounding (max |dp| 9e-7 vs 9e-7 for plain fp32, DESIGN.md);
// activations peak near 1.5e3 for every model of the zoo (fp16 max 65504), and are clamped for safety.
//
// LDS layout ("chunk planar", tools/trunk_layout.py checks every access pattern against the gfx950 bank model): all
// operands live in 16-byte SLOTS of 8 halves and every MFMA operand fragment is ONE ds_read_b128 per lane.
//   X   [9 rows x 57] slots, slot = one pixel of the zero-padded 9x45 input.  Two planes with the hi/lo parts of the 5
//       channels interleaved so that the three split products of a tap take TWO MFMAs:
//         XA = [h0 h1 h2 h3 h4 l0 l1 l2]  x  WA = [H0 H1 H2 H3 H4 H0 H1 H2]
//         XB = [l3 l4 h0 h1 h2 h3 h4  0]  x  WB = [H3 H4 L0 L1 L2 L3 L4  0]     (h/l: input, H/L: weight)
//       A K group = 4 taps (lane group g reads the pixel of tap g).  The 25 taps of the 5x5 kernel form 7 groups whose
//       lane-group pairs (g0,g1)/(g2,g3) are horizontally adjacent taps or taps 112 slots apart (row pitch 57 = 41+16),
//       the two cases ds_read_b128's 16-lane groups serve without bank conflicts; the 1x5 and 5x1 kernels reuse the
//       fragments of the groups that contain their taps (2 + 3 groups, zero weights elsewhere): 24 MFMAs per 16 positions.
//   A1  [6 chunks][221 slots]: chunk = 8 of the 48 conv1 channels, slot = h*44 + w.  conv2 (stride 2 in w) reads it
//       conflict-free with tiles (row y, x = 0..15) x 4 + one tile of the 16 left-over columns; chunk pitch is odd.
//   A2  [4 chunks][119 slots], slot = y*26 + x; conv3's lane -> position map is a table (C3_SLOT/C3_OUT).
// =====================================================================================================================
constexpr int T_RX = 57, T_XS = 9 * T_RX;                // X slots per padded row / per plane
constexpr int T_R1 = 44, T_PL1 = 221;                     // A1 slots per row / per chunk plane (6 chunks)
constexpr int T_R2 = 26, T_PL2 = 119;                     // A2 slots per row / per chunk plane (4 chunks)
constexpr int T_NW1 = 24, T_NW2 = 18, T_NW3 = 24;         // fragments: conv1 (7+7 5x5, 2+2 1x5, 3+3 5x1), conv2 (9 x 2), conv3 (6 x 4)
constexpr int T_FRAG = 64 * 8;                            // halves per fragment
constexpr int T_XPLANE = T_XS * 8, T_A1PLANE = 6 * T_PL1 * 8, T_A2PLANE = 4 * T_PL2 * 8;   // halves between the two planes of a buffer
// packed blob: [conv1 24 frags][conv2 hi 18][conv2 lo 18][conv3 hi 24][conv3 lo 24] halves, then f32 b1*S[48] b2*S[32]
// b3*S[64] 1/S pad[3], then int32 C3_SLOT[32], C3_OUT[32]
constexpr int H_PACKED_BYTES = 2 * T_FRAG * (T_NW1 + 2 * T_NW2 + 2 * T_NW3) + 4 * (48 + 32 + 64 + 4) + 4 * 64;
// conv1 K groups: tap (dy, dx) of lane group g, as the slot offset dy * T_RX + dx (tools/trunk_layout.py)
constexpr int C1_TAPS[7][4][2] = {{{2, 0}, {2, 1}, {2, 3}, {2, 4}}, {{0, 4}, {2, 2}, {1, 4}, {3, 2}}, {{0, 2}, {0, 3}, {1, 2}, {1, 3}},
                                  {{4, 2}, {4, 3}, {4, 4}, {4, 4}}, {{0, 0}, {0, 1}, {1, 0}, {1, 1}}, {{3, 0}, {3, 1}, {3, 3}, {3, 4}},
                                  {{4, 0}, {4, 1}, {4, 0}, {4, 1}}};
constexpr int C3_SLOT[32] = {60, 34, 32, 8, 28, 26, 68, 16, 2, 54, 14, 56, 6, 62, 52, 58, 30, 36, 34, 6, 4, 66, 38, 0, 66, 42, 8, 12, 10, 40, 64, 34};
constexpr int C3_OUT[32] = {22, 13, 12, 4, 10, 9, 26, 8, 1, 19, 7, 20, 3, 23, 18, 21, 11, 14, -1, -1, 2, 25, 15, 0, -1, 17, -1, 6, 5, 16, 24, -1};

// four 16-bit fields (one per lane group g): offset in halves of the operand slot of K group G
__host__ __device__ constexpr uint64_t c1_tap_pack(int G)
{
    uint64_t v = 0;
    for (int q = 0; q < 4; q++) v |= (uint64_t)((C1_TAPS[G][q][0] * T_RX + C1_TAPS[G][q][1]) * 8) << (16 * q);
    return v;
}
__host__ __device__ constexpr uint64_t c2_off_pack(int G)
{
    uint64_t v = 0;
    for (int q = 0; q < 4; q++) {
        const int idx = 4 * G + q, tap = idx / 6, ch = idx - tap * 6;            // K chunk = (tap, chunk of 8 channels)
        v |= (uint64_t)((ch * T_PL1 + (tap / 3) * T_R1 + (tap % 3)) * 8) << (16 * q);
    }
    return v;
}
// D[channel 4g + r][position c16] += W[channel][k] * X[k][position]
#define NC_MFMA(ACC, W, X) ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(W, X, ACC, 0, 0, 0);

// conv1 of NT tiles of 16 positions: tile_first, tile_first + 4, ... and, when tile_last >= 0, tile_last as the last one.
// w1 = the 24 resident fragments:
// [0..6] 5x5 WA, [7..13] 5x5 WB, [14,15] 1x5 WA (groups 0,1), [16,17] 1x5 WB, [18..20] 5x1 WA (groups 1,2,3), [21..23] 5x1 WB
// KL: which kernels' output channels the LAST tile computes -- bit 0 the 1x5 kernel's 16 (4 MFMAs per tile, K groups 0,1), bit 1
// the 5x1 kernel's (6 MFMAs, groups 1..3), bit 2 the 5x5 kernel's (14 MFMAs, all groups).  A tile can so be shared by two
// waves to even out the SIMDs, and its MFMAs are interleaved with those of the wave's full tiles (a partial tile on its own
// is one chain of dependent MFMAs: latency-bound).
template <int NT, int KL = 7>
__device__ __forceinline__ void t_conv1(const _Float16 *XA, _Float16 *A1H, const h8 (&w1)[T_NW1],
                                        const float *__restrict__ b1s, const h_epi &epi, int tile_first, int lane, int tile_last = -1)
{
    // kernel mask and K-group range of tile tm
#define C1_KM(tm) ((tm) == NT - 1 ? KL : 7)
#define C1_GHI(tm) ((C1_KM(tm) & 4) ? 7 : ((C1_KM(tm) & 2) ? 4 : 2))
    const int g = lane >> 4, c16 = lane & 15;
    int xbase[NT], obase[NT];
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
        const int p = ((tm == NT - 1 && tile_last >= 0) ? tile_last : tile_first + 4 * tm) * 16 + c16;
        const int pr = p < 205 ? p : 204;
        const int h = pr / 41, w = pr - h * 41;
        xbase[tm] = (h * T_RX + w) * 8;                              // halves; tap (dy,dx) of pixel (h,w) is padded pixel (h+dy, w+dx)
        // positions 205..207 (tile 12) go to the three unused slots at the end of row 4
        obase[tm] = ((g >> 1) * T_PL1 + (p < 205 ? h * T_R1 + w : 4 * T_R1 + 41 + (p - 205))) * 8 + (g & 1) * 4;
        // opaque per call: keeps site-loop invariant address arithmetic from being hoisted out of the site loop (spills)
        asm volatile("" : "+v"(xbase[tm]), "+v"(obase[tm]));
    }
    const int sh = 16 * g;                                             // field of this lane group in the packed offset constants
    f32x4v acc1[NT], acc2[NT], acc3[NT];
    {
        const f32x4v x1 = *reinterpret_cast<const f32x4v *>(b1s + 4 * g), x2 = *reinterpret_cast<const f32x4v *>(b1s + 16 + 4 * g),
                     x3 = *reinterpret_cast<const f32x4v *>(b1s + 32 + 4 * g);
#pragma unroll
        for (int tm = 0; tm < NT; tm++) { acc1[tm] = x1; acc2[tm] = x2; acc3[tm] = x3; }
    }
    // software pipeline: the ds_reads of group G + 1 are issued before the MFMAs of group G (register double buffer)
    constexpr int DP = 1, NB = DP + 1;
    h8 xa[NB][NT], xb[NB][NT];
    auto load1 = [&](int G, int slot) {
        const int toff = (int)((c1_tap_pack(G) >> sh) & 0xffffu);       // halves
#pragma unroll
        for (int tm = 0; tm < NT; tm++) {
            if (G >= C1_GHI(tm)) continue;
            xa[slot][tm] = lds_h8(XA + xbase[tm] + toff);
            xb[slot][tm] = lds_h8(XA + xbase[tm] + toff + T_XPLANE);
        }
    };
    constexpr int NG = NT > 1 ? 7 : C1_GHI(0);
#pragma unroll
    for (int G = 0; G < DP && G < NG; G++) load1(G, G % NB);
#pragma unroll
    for (int G = 0; G < NG; G++) {
        const int cur = G % NB;
        if (G + DP < NG) load1(G + DP, (G + DP) % NB);
        __builtin_amdgcn_sched_barrier(0);
        // independent accumulators interleaved: no MFMA depends on the one issued just before it
#pragma unroll
        for (int tm = 0; tm < NT; tm++) if (C1_KM(tm) & 4) { NC_MFMA(acc3[tm], w1[G], xa[cur][tm]) }
        if (G < 2) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (C1_KM(tm) & 1) { NC_MFMA(acc1[tm], w1[14 + G], xa[cur][tm]) }
        }
        if (G >= 1 && G <= 3) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (C1_KM(tm) & 2) { NC_MFMA(acc2[tm], w1[18 + G - 1], xa[cur][tm]) }
        }
#pragma unroll
        for (int tm = 0; tm < NT; tm++) if (C1_KM(tm) & 4) { NC_MFMA(acc3[tm], w1[7 + G], xb[cur][tm]) }
        if (G < 2) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (C1_KM(tm) & 1) { NC_MFMA(acc1[tm], w1[16 + G], xb[cur][tm]) }
        }
        if (G >= 1 && G <= 3) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (C1_KM(tm) & 2) { NC_MFMA(acc2[tm], w1[21 + G - 1], xb[cur][tm]) }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
        const int o = obase[tm];
        if (C1_KM(tm) & 1) split4_store(selu4_scaled(acc1[tm], epi), A1H + o, A1H + o + T_A1PLANE);
        if (C1_KM(tm) & 2) split4_store(selu4_scaled(acc2[tm], epi), A1H + o + 2 * T_PL1 * 8, A1H + o + 2 * T_PL1 * 8 + T_A1PLANE);
        if (C1_KM(tm) & 4) split4_store(selu4_scaled(acc3[tm], epi), A1H + o + 4 * T_PL1 * 8, A1H + o + 4 * T_PL1 * 8 + T_A1PLANE);
    }
#undef C1_KM
#undef C1_GHI
}

// ---- the three-stage form of the trunk (k5_trunk_p3): conv1, conv2 and conv3 work on three consecutive sites, ONE workgroup barrier per
// site.  A conv2 wave computes all 32 output channels of its tiles and a conv3 wave 32 of the 64, so that every operand fragment read from
// LDS feeds 6 MFMAs instead of 3 (338 instead of 458 ds_read_b128 per site: the LDS pipe at 128 B/clk is as loaded as the matrix pipe).
// conv2, wave CW of two: tiles CW and CW + 2 in full, and channel half CW of tile 4 (columns 16..19 of the four rows)
// the accumulators of a conv2 wave between its MFMA loop and its epilogue
struct c2_acc { f32x4v a[2][2], a4; };
template <int CW>
__device__ __forceinline__ void t_conv2_pair_mma(const _Float16 *A1H, const h8 (&wh)[9][2], const h8 (&wl)[9][2], const float *__restrict__ b2s, int lane, c2_acc &o)
{
    const int g = lane >> 4, c16 = lane & 15, sh = 16 * g;
    int abase[3];
#pragma unroll
    for (int tm = 0; tm < 3; tm++) {
        const int t = tm < 2 ? CW + 2 * tm : 4;
        const int y = t < 4 ? t : (c16 & 3), x = t < 4 ? c16 : 16 + (c16 >> 2);
        abase[tm] = (y * T_R1 + 2 * x) * 8;
        asm volatile("" : "+v"(abase[tm]));
    }
    f32x4v acc[2][2], acc4;
    {
        const f32x4v b0 = *reinterpret_cast<const f32x4v *>(b2s + 4 * g), b1 = *reinterpret_cast<const f32x4v *>(b2s + 16 + 4 * g);
        acc[0][0] = b0; acc[1][0] = b0; acc[0][1] = b1; acc[1][1] = b1;
        acc4 = CW ? b1 : b0;
    }
    constexpr int DP = 1, NB = DP + 1;                                 // K groups requested ahead of the one being multiplied / register buffers
    h8 ah[NB][3], al[NB][3];
    auto load2 = [&](int G, int slot) {
        const int off = (int)((c2_off_pack(G) >> sh) & 0xffffu);
#pragma unroll
        for (int tm = 0; tm < 3; tm++) {
            ah[slot][tm] = lds_h8(A1H + abase[tm] + off);
            al[slot][tm] = lds_h8(A1H + abase[tm] + off + T_A1PLANE);
        }
    };
#pragma unroll
    for (int G = 0; G < DP; G++) load2(G, G % NB);
#pragma unroll
    for (int G = 0; G < 9; G++) {
        const int cur = G % NB;
        if (G + DP < 9) load2(G + DP, (G + DP) % NB);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tm = 0; tm < 2; tm++) { NC_MFMA(acc[tm][0], wh[G][0], ah[cur][tm]) NC_MFMA(acc[tm][1], wh[G][1], ah[cur][tm]) }
        NC_MFMA(acc4, wh[G][CW], ah[cur][2])
#pragma unroll
        for (int tm = 0; tm < 2; tm++) { NC_MFMA(acc[tm][0], wh[G][0], al[cur][tm]) NC_MFMA(acc[tm][1], wh[G][1], al[cur][tm]) }
        NC_MFMA(acc4, wh[G][CW], al[cur][2])
#pragma unroll
        for (int tm = 0; tm < 2; tm++) { NC_MFMA(acc[tm][0], wl[G][0], ah[cur][tm]) NC_MFMA(acc[tm][1], wl[G][1], ah[cur][tm]) }
        NC_MFMA(acc4, wl[G][CW], ah[cur][2])
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) o.a[tm][tn] = acc[tm][tn];
    o.a4 = acc4;
}
template <int CW>
__device__ __forceinline__ void t_conv2_pair_epi(_Float16 *A2H, const h_epi &epi, int lane, const c2_acc &o)
{
    const int g = lane >> 4, c16 = lane & 15;
    int obase[3];
#pragma unroll
    for (int tm = 0; tm < 3; tm++) {
        const int t = tm < 2 ? CW + 2 * tm : 4;
        const int y = t < 4 ? t : (c16 & 3), x = t < 4 ? c16 : 16 + (c16 >> 2);
        obase[tm] = ((g >> 1) * T_PL2 + y * T_R2 + x) * 8 + (g & 1) * 4;              // channel half 0; half 1: + 2 * T_PL2 * 8
        asm volatile("" : "+v"(obase[tm]));
    }
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) {
            const int oo = obase[tm] + tn * 2 * T_PL2 * 8;
            split4_store(selu4_scaled(o.a[tm][tn], epi), A2H + oo, A2H + oo + T_A2PLANE);
        }
    {
        const int oo = obase[2] + CW * 2 * T_PL2 * 8;
        split4_store(selu4_scaled(o.a4, epi), A2H + oo, A2H + oo + T_A2PLANE);
    }
}
template <int CW>
__device__ __forceinline__ void t_conv2_pair(const _Float16 *A1H, _Float16 *A2H, const h8 (&wh)[9][2], const h8 (&wl)[9][2],
                                             const float *__restrict__ b2s, const h_epi &epi, int lane)
{
    c2_acc o;
    t_conv2_pair_mma<CW>(A1H, wh, wl, b2s, lane, o);
    t_conv2_pair_epi<CW>(A2H, epi, lane, o);
}

// conv3, wave CW of two: output channels 32 CW .. 32 CW + 31 of both position tiles
struct c3_acc { f32x4v a[2][2]; };
template <int CW>
__device__ __forceinline__ void t_conv3_pair_mma(const _Float16 *A2H, const h8 (&w3h)[6][2], const h8 (&w3l)[6][2], const float *__restrict__ b3s, const int (&c3slot)[2], int lane,
                                                 c3_acc &o)
{
    const int g = lane >> 4;
    int abase[2];
#pragma unroll
    for (int tm = 0; tm < 2; tm++) {
        abase[tm] = (g * T_PL2 + c3slot[tm]) * 8;
        asm volatile("" : "+v"(abase[tm]));
    }
    f32x4v acc[2][2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        acc[0][tn] = *reinterpret_cast<const f32x4v *>(b3s + (2 * CW + tn) * 16 + 4 * g);
        acc[1][tn] = acc[0][tn];
    }
    constexpr int DP = 1, NB = DP + 1;                                 // K groups requested ahead of the one being multiplied / register buffers
    h8 ah[NB][2], al[NB][2];
    auto load3 = [&](int G, int slot) {
        const int off = ((G / 3) * T_R2 + (G % 3)) * 8;
#pragma unroll
        for (int tm = 0; tm < 2; tm++) {
            ah[slot][tm] = lds_h8(A2H + abase[tm] + off);
            al[slot][tm] = lds_h8(A2H + abase[tm] + off + T_A2PLANE);
        }
    };
#pragma unroll
    for (int G = 0; G < DP; G++) load3(G, G % NB);
#pragma unroll
    for (int G = 0; G < 6; G++) {
        const int cur = G % NB;
        if (G + DP < 6) load3(G + DP, (G + DP) % NB);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tm = 0; tm < 2; tm++) { NC_MFMA(acc[tm][0], w3h[G][0], ah[cur][tm]) NC_MFMA(acc[tm][1], w3h[G][1], ah[cur][tm]) }
#pragma unroll
        for (int tm = 0; tm < 2; tm++) { NC_MFMA(acc[tm][0], w3h[G][0], al[cur][tm]) NC_MFMA(acc[tm][1], w3h[G][1], al[cur][tm]) }
#pragma unroll
        for (int tm = 0; tm < 2; tm++) { NC_MFMA(acc[tm][0], w3l[G][0], ah[cur][tm]) NC_MFMA(acc[tm][1], w3l[G][1], ah[cur][tm]) }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) o.a[tm][tn] = acc[tm][tn];
}
template <int CW>
__device__ __forceinline__ void t_conv3_pair_epi(const h_epi &epi, float *__restrict__ out_site, const int (&c3out)[2], int lane, const c3_acc &o)
{
    const int g = lane >> 4;
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
        if (c3out[tm] >= 0) {
#pragma unroll
            for (int tn = 0; tn < 2; tn++)
                *reinterpret_cast<f32x4v *>(out_site + c3out[tm] * 64 + (2 * CW + tn) * 16 + 4 * g) = selu4_scaled(o.a[tm][tn], epi);
        }
}
template <int CW>
__device__ __forceinline__ void t_conv3_pair(const _Float16 *A2H, const h8 (&w3h)[6][2], const h8 (&w3l)[6][2], const float *__restrict__ b3s,
                                             const h_epi &epi, float *__restrict__ out_site, const int (&c3slot)[2], const int (&c3out)[2], int lane)
{
    c3_acc o;
    t_conv3_pair_mma<CW>(A2H, w3h, w3l, b3s, c3slot, lane, o);
    t_conv3_pair_epi<CW>(epi, out_site, c3out, lane, o);
}

// Three roles, one barrier per site (the default trunk since round 5).  Step s:
//   waves 4-7: conv1 of site s (X[s & 1] -> A1[s & 1]); waves 4, 5 three tiles (72 MFMAs), waves 6, 7 three tiles + their part of tile 12 (86 / 82);
//   waves 0, 1: conv2 of site s - 1 (A1[(s - 1) & 1] -> A2[(s - 1) & 1]), all 32 channels of two tiles + one channel half of tile 4 (135 MFMAs);
//   waves 2, 3: staging of site s + 1 into X[(s + 1) & 1] (two pixels per thread, loads issued a step earlier), then conv3 of site s - 2
//               (A2[s & 1] -> HBM; 32 of the 64 channels each, 72 MFMAs).
// Every wave's weight fragments stay in its registers (conv1 96, conv2 144, conv3 96 VGPRs).  Waves w and w + 4 share a SIMD (tools/ubench/simdmap.hip):
// 207 / 207 / 158 / 154 MFMAs per SIMD and site.  What sets the step is the longest single-wave chain {requests, MFMAs, epilogue}, not a pipe: the roles
// are cut so that the chains are even (per-wave phase times: profiles/r06_trunk_phases.md), and the MFMA-heaviest role sits on the OLDEST waves,
// whose instructions the issue arbiter prefers (a younger wave's MFMAs starve behind an older wave's vector burst, not the other way round).
template <bool X16>
__global__ __launch_bounds__(512) void k5_trunk_p3(const float *__restrict__ x, const uint8_t *__restrict__ wp, float *__restrict__ a3,
                                                   int64_t n_sites, const double *__restrict__ scale, int scale_mode, int64_t site0, float x_limit,
                                                   uint8_t *__restrict__ range_sites)
{
    __shared__ __attribute__((aligned(16))) _Float16 X[2][2 * T_XPLANE];
    __shared__ __attribute__((aligned(16))) _Float16 A1[2][2 * T_A1PLANE];
    __shared__ __attribute__((aligned(16))) _Float16 A2[2][2 * T_A2PLANE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint4 *w1f = reinterpret_cast<const uint4 *>(wp), *w2h = w1f + T_NW1 * 64, *w2l = w2h + T_NW2 * 64, *w3h = w2l + T_NW2 * 64,
                *w3l = w3h + T_NW3 * 64;
    __shared__ __attribute__((aligned(16))) float BIAS[48 + 32 + 64];
    const float *bg = reinterpret_cast<const float *>(w3l + T_NW3 * 64);
    const float *b1s = BIAS, *b2s = BIAS + 48, *b3s = BIAS + 80;
    const int *c3tab = reinterpret_cast<const int *>(bg + 48 + 32 + 68);
    const float inv_s = bg[48 + 32 + 64];
    if (threadIdx.x < 48 + 32 + 64) BIAS[threadIdx.x] = bg[threadIdx.x];
    const h_epi epi = {inv_s * 1.44269504088896341f, inv_s * SELU_L, 60000.0f / (inv_s * SELU_L)};
    const int64_t n_k = (n_sites - blockIdx.x + gridDim.x - 1) / gridDim.x;        // sites of this workgroup (>= 1)
    for (int i = threadIdx.x; i < 4 * T_XS; i += 512) *reinterpret_cast<uint4 *>(&X[0][0] + i * 8) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    // staging, by the two conv3 waves (the lightest role): thread t of the 128 owns pixels t and t + 128 (< 205).  prefetch() only issues the loads
    // of a site's tensor; commit() converts them a step later (scale, range guard, fp16 hi / lo) and writes the two operand planes of X
    auto stage_px = [&](int j) { const int t = (int)threadIdx.x - 128 + 128 * j; return t < 205 ? t : 204; };
    if (wv >= 4) {
        // ------------------------------------------------------------------ conv1 of site s: 13 tiles as 3 / 3 / 3 / 3 + tile 12 shared by waves 0, 1
        h8 w1[T_NW1];
#pragma unroll
        for (int q = 0; q < T_NW1; q++) w1[q] = as_h8(w1f[q * 64 + lane]);
        __syncthreads();                                                           // P0
        for (int64_t s = 0; s < n_k + 2; s++) {
            if (s < n_k) {
                const int buf = (int)(s & 1);
                // waves 4, 5 (beside the conv2 waves: 135 MFMAs) three tiles, waves 6, 7 (beside the conv3 waves: 72) three tiles + their part of tile 12
                if (wv == 6) t_conv1<4, 4>(X[buf], A1[buf], w1, b1s, epi, 0, lane, 12);     // tiles 0, 4, 8, the 5x5 channels of tile 12
                else if (wv == 7) t_conv1<4, 3>(X[buf], A1[buf], w1, b1s, epi, 1, lane, 12);  // tiles 1, 5, 9, the 1x5 + 5x1 channels of tile 12
                else t_conv1<3>(X[buf], A1[buf], w1, b1s, epi, wv - 2, lane);           // tiles 2, 6, 10 / 3, 7, 11
            }
            __syncthreads();
        }
    } else if (wv < 2) {
        // ------------------------------------------------------------------ conv2 of site s - 1
        h8 c2h[9][2], c2l[9][2];
#pragma unroll
        for (int q = 0; q < 9; q++)
#pragma unroll
            for (int tn = 0; tn < 2; tn++) { c2h[q][tn] = as_h8(w2h[(q * 2 + tn) * 64 + lane]); c2l[q][tn] = as_h8(w2l[(q * 2 + tn) * 64 + lane]); }
        __syncthreads();                                                           // P0
        for (int64_t s = 0; s < n_k + 2; s++) {
            if (s >= 1 && s - 1 < n_k) {
                const int buf = (int)((s - 1) & 1);
                if (wv == 0) t_conv2_pair<0>(A1[buf], A2[buf], c2h, c2l, b2s, epi, lane);
                else t_conv2_pair<1>(A1[buf], A2[buf], c2h, c2l, b2s, epi, lane);
            }
            __syncthreads();
        }
    } else {
        // ------------------------------------------------------------------ staging of site s + 1, conv3 of site s - 2
        const int cw = wv - 2;
        h8 c3h[6][2], c3l[6][2];
#pragma unroll
        for (int q = 0; q < 6; q++)
#pragma unroll
            for (int tn = 0; tn < 2; tn++) {
                c3h[q][tn] = as_h8(w3h[(q * 4 + 2 * cw + tn) * 64 + lane]);
                c3l[q][tn] = as_h8(w3l[(q * 4 + 2 * cw + tn) * 64 + lane]);
            }
        const int c3slot[2] = {c3tab[lane & 15], c3tab[16 + (lane & 15)]}, c3out[2] = {c3tab[32 + (lane & 15)], c3tab[48 + (lane & 15)]};
        const int st = (int)threadIdx.x - 128;                                    // 0..127
        float pre[2][5];
        uint32_t raw[2][3];
        double pre_sd = 1.0;
        int64_t pre_site = 0;
        auto prefetch = [&](int64_t site) {
            pre_site = site;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int px = stage_px(j);
                if constexpr (X16) {
                    const int16_t *xs = reinterpret_cast<const int16_t *>(x) + site * NC_SNP_TENSOR + px * 5;       // 2-byte aligned
                    typedef uint32_t __attribute__((aligned(2))) u32_a2;
                    raw[j][0] = *reinterpret_cast<const u32_a2 *>(xs);
                    raw[j][1] = *reinterpret_cast<const u32_a2 *>(xs + 2);
                    raw[j][2] = (uint32_t)(uint16_t)xs[4];
                } else {
                    const float *xs = x + site * NC_SNP_TENSOR + px * 5;
#pragma unroll
                    for (int u = 0; u < 5; u++) pre[j][u] = xs[u];
                }
            }
            if (scale) pre_sd = scale[site0 + site];
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (st + 128 * j >= 205) continue;
                const int px = st + 128 * j, ph = px / 41, pw = px - ph * 41;
                const int xslot = ((ph + 2) * T_RX + pw + 2) * 8;
                float v5[5];
                if constexpr (X16) {
                    v5[0] = (float)(int16_t)(raw[j][0] & 0xffffu); v5[1] = (float)(int16_t)(raw[j][0] >> 16);
                    v5[2] = (float)(int16_t)(raw[j][1] & 0xffffu); v5[3] = (float)(int16_t)(raw[j][1] >> 16);
                    v5[4] = (float)(int16_t)raw[j][2];
                } else {
#pragma unroll
                    for (int u = 0; u < 5; u++) v5[u] = pre[j][u];
                }
                const double md = (scale && ph > 0) ? pre_sd : 1.0;               // snpCaller.py:93-96
                const float mf = (float)md;
                if (scale_mode == 0) {
#pragma unroll
                    for (int u = 0; u < 4; u++) v5[u] *= mf;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; u++) v5[u] = (float)((double)v5[u] * md);
                }
                const float amax = fmaxf(fmaxf(fmaxf(fabsf(v5[0]), fabsf(v5[1])), fmaxf(fabsf(v5[2]), fabsf(v5[3]))), fabsf(v5[4]));
                if (range_sites && !(amax <= x_limit)) range_sites[site0 + pre_site] = 1;
                _Float16 hi[5], lo[5];
#pragma unroll
                for (int u = 0; u < 5; u++) {
                    float v = v5[u];
                    v = fminf(fmaxf(v, -65504.0f), 65504.0f);
                    hi[u] = (_Float16)v;
                    lo[u] = (_Float16)(v - (float)hi[u]);
                }
                const h8 sa = {hi[0], hi[1], hi[2], hi[3], hi[4], lo[0], lo[1], lo[2]};
                const h8 sb = {lo[3], lo[4], hi[0], hi[1], hi[2], hi[3], hi[4], (_Float16)0.0f};
                *reinterpret_cast<h8 *>(&X[buf][xslot]) = sa;
                *reinterpret_cast<h8 *>(&X[buf][xslot + T_XPLANE]) = sb;
            }
        };
        int64_t site = blockIdx.x;                                                 // the site conv3 works on next
        prefetch(blockIdx.x);
        commit(0);
        if (n_k > 1) prefetch((int64_t)blockIdx.x + gridDim.x);
        __syncthreads();                                                           // P0
        for (int64_t s = 0; s < n_k + 2; s++) {
            // the other X buffer's last reader was conv1 of site s - 1 (a barrier ago); site s + 1's loads were issued a step ago
            if (s + 1 < n_k) commit((int)((s + 1) & 1));
            if (s + 2 < n_k) prefetch((int64_t)blockIdx.x + (s + 2) * gridDim.x);
            if (s >= 2) {
                const int buf = (int)(s & 1);
                float *out_site = a3 + site * (27 * 64);
                if (cw == 0) t_conv3_pair<0>(A2[buf], c3h, c3l, b3s, epi, out_site, c3slot, c3out, lane);
                else t_conv3_pair<1>(A2[buf], c3h, c3l, b3s, epi, out_site, c3slot, c3out, lane);
                site += gridDim.x;
            }
            __syncthreads();
        }
    }
}
// =====================================================================================================================
// k5_trunk_lin: the three-stage trunk with conv1 BY LINEARITY (round 6; VERDICT r5 #1b / #1c).
//
// The int16 site tensor is exact in fp16 (|x| <= 2048) and conv1 is linear, so the coverage scale s (snpCaller.py:93-96) does not have
// to be multiplied into the operand (which makes it a 22-bit number: hi + lo planes, three products): with
//     pre-activation = b + s * SUM(W x_scaled) + SUM(W u_unscaled) = s * [ b / s + SUM(W x) + SUM(W (u / s)) ]
// the scaled entries (rows 1-4, channels 0-3) enter the MFMA as the INTEGERS they are -- two products (x Wh + x Wl), no lo plane -- the few
// unscaled ones (channel 4 = the reference-base marker, and row 0 = the one-hot reference row) enter as u * rho, rho = 1 / s split into fp16
// hi / lo, and s itself folds into the epilogue's constants (the accumulators already carry a scale S).  Operand layout: a "record" per
// (image row r, column w) = the 5 pixels (r, w-2 .. w+2) x 6 values [x0 x1 x2 x3 hi(u4 rho) lo(u4 rho)] = 30 of 32 K slots = ONE K group per
// 5-tap kernel row (the pixel form of k5_trunk_p3 spends 7 K groups x 2 planes on the 25 taps); row 0 has its own records (hi and lo plane of
// u rho, same K layout, same weight fragments).  Kernel rows that fall on the `same` padding of the 5-row image for every position of a tile are
// not executed at all.  Per site: conv1 199 MFMAs (312 before) and 83 operand reads (182): 613 MFMAs (726), 239 ds_read_b128 (338).
// LDS: X buffer = P1 [4 slots][176 records] + P0 hi / lo [4][48] each (slot-planar: the 16 positions of a tile read 16 consecutive 16-byte slots).
constexpr int L_NR1 = 176, L_NR0 = 48;                                       // records per slot plane (multiples of 16): 4 x 41 = 164 + zero / dump records; 41 + ...
constexpr int L_P0H = 4 * L_NR1 * 8, L_P0L = L_P0H + 4 * L_NR0 * 8, L_XBUF = L_P0L + 4 * L_NR0 * 8;   // halves
constexpr int L_Z1 = 164, L_Z0 = 41, L_DUMP1 = 170, L_DUMP0 = 44;           // all-zero records (read by lanes whose kernel row is off the image); write-only dump records
constexpr int T_NW1L = 17;                                                   // conv1 fragments: 5x5 hi / lo per kernel row, 1x5 hi / lo, 5x1 groups A, B (hi / lo), C (hi)
enum { LW_5H = 0, LW_5L = 5, LW_1H = 10, LW_1L = 11, LW_2HA = 12, LW_2LA = 13, LW_2HB = 14, LW_2LB = 15, LW_2HC = 16 };
constexpr int L_PACKED_BYTES = 2 * T_FRAG * T_NW1L;
constexpr int L_DXO[5] = {0, -2, -1, 1, 2};                                  // pixel i of a record is column w + L_DXO[i] (the centre first: slot 0 serves the 5x1 kernel)
// which tiles of 16 positions a conv1 wave computes (position p = 16 t + lane % 16 = 41 h + w)
// `part` = which of a tile's three accumulators the wave computes (1: the 1x5 kernel's 16 channels, 2: the 5x1 kernel's, 4: the 5x5 kernel's): the 13th
// tile (positions 192..204: 10 MFMAs but a full 12 activations per lane) is split by kernel over three waves, 36 / 40 / 40 / 40 activations per lane
// instead of 48 / 36 / 36 / 36 -- the conv1 waves' epilogues are the pole of the step (profiles/r06_trunk_phases.md)
struct c1l_role { int nt; int tile[5]; int part[5]; };
constexpr c1l_role C1L_ROLES[4] = {{3, {0, 4, 8, 0, 0}, {7, 7, 7, 0, 0}}, {4, {1, 5, 9, 12, 0}, {7, 7, 7, 1, 0}}, {4, {2, 6, 10, 12, 0}, {7, 7, 7, 2, 0}},
                                   {4, {3, 7, 11, 12, 0}, {7, 7, 7, 4, 0}}};
constexpr int c1l_hlo(int t) { return (16 * t) / 41; }
constexpr int c1l_hhi(int t) { return (16 * t + 15 > 204 ? 204 : 16 * t + 15) / 41; }
constexpr bool c1l_v1(int h, int dy) { return h + dy - 2 >= 1 && h + dy - 2 <= 4; }
constexpr bool c1l_v0(int h, int dy) { return h + dy - 2 == 0; }
constexpr bool c1l_need1(int t, int dy) { return c1l_v1(c1l_hlo(t), dy) || c1l_v1(c1l_hhi(t), dy); }
constexpr bool c1l_all1(int t, int dy) { return c1l_v1(c1l_hlo(t), dy) && c1l_v1(c1l_hhi(t), dy); }
constexpr bool c1l_need0(int t, int dy) { return c1l_v0(c1l_hlo(t), dy) || c1l_v0(c1l_hhi(t), dy); }
constexpr bool c1l_all0(int t, int dy) { return c1l_v0(c1l_hlo(t), dy) && c1l_v0(c1l_hhi(t), dy); }
constexpr bool c1l_low(int t) { return c1l_hlo(t) <= 2; }                    // some position of the tile has image row 0 under a 5x1 tap (groups B, C)
constexpr int c1l_n0(int role, int dy) { int n = 0; for (int tm = 0; tm < C1L_ROLES[role].nt; tm++) n += c1l_need0(C1L_ROLES[role].tile[tm], dy) ? 1 : 0; return n; }
constexpr int c1l_mfma_tile(int t)
{
    int n = 0;
    for (int dy = 0; dy < 5; dy++) n += (c1l_need1(t, dy) ? 2 : 0) + (c1l_need0(t, dy) ? 3 : 0) + (dy == 2 ? (c1l_need1(t, dy) ? 2 : 0) + (c1l_need0(t, dy) ? 3 : 0) : 0);
    return n + 2 + (c1l_low(t) ? 3 : 0);
}
constexpr bool c1l_roles_cover()                                             // every accumulator of every tile is exactly one wave's
{
    for (int t = 0; t < 13; t++) {
        int seen = 0;
        for (int r = 0; r < 4; r++)
            for (int tm = 0; tm < C1L_ROLES[r].nt; tm++)
                if (C1L_ROLES[r].tile[tm] == t) { if (seen & C1L_ROLES[r].part[tm]) return false; seen |= C1L_ROLES[r].part[tm]; }
        if (seen != 7) return false;
    }
    return true;
}
static_assert(c1l_roles_cover(), "C1L_ROLES: the roles do not cover the 13 tiles x 3 kernels exactly once");
constexpr int c1l_mfma_site() { int n = 0; for (int t = 0; t < 13; t++) n += c1l_mfma_tile(t); return n; }
// MFMAs per site (nc_snp_trunk_info).  conv2: 10 (position tile, channel tile) pairs x 9 K groups x 3 products; conv3: 8 pairs x 6 x 3; conv1 of the
// pixel-form trunk: T_NW1 per tile of 16 positions
constexpr int C23_MFMA_PER_SITE = 10 * 27 + 8 * 18;
constexpr int L_MFMA_PER_SITE = c1l_mfma_site() + C23_MFMA_PER_SITE, T_MFMA_PER_SITE = 13 * T_NW1 + C23_MFMA_PER_SITE;

// the MFMAs of the tiles of a conv1 role (7 steps)
template <int ROLE, int NT = C1L_ROLES[ROLE].nt>
__device__ __forceinline__ void c1l_mma(const _Float16 *XB, const h8 (&wl)[T_NW1L], const float *__restrict__ b1s, float rho, int lane, f32x4v (&acc1)[NT], f32x4v (&acc2)[NT],
                                        f32x4v (&acc3)[NT], int (&obase)[NT])
{
    auto tile_of = [](int tm) constexpr { return C1L_ROLES[ROLE].tile[tm]; };
    auto part_of = [](int tm) constexpr { return C1L_ROLES[ROLE].part[tm]; };
    auto k55 = [&](int tm) constexpr { return (part_of(tm) & 4) != 0; };            // the 5x5 kernel's accumulator of this tile is this wave's
    auto k15 = [&](int tm) constexpr { return (part_of(tm) & 1) != 0; };
    auto k51 = [&](int tm) constexpr { return (part_of(tm) & 2) != 0; };
    auto use = [&](int tm, int s) constexpr { return k55(tm) || (s == 2 && k15(tm)); };   // the kernel row's operand is needed
    const int g = lane >> 4, c16 = lane & 15;
    int pr8[NT], w8[NT], hrow[NT];
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
        const int t = tile_of(tm);
        const int p = 16 * t + c16, pr = p < 205 ? p : 204;
        const int h = c1l_hlo(t) == c1l_hhi(t) ? c1l_hlo(t) : (pr >= 41 * c1l_hhi(t) ? c1l_hhi(t) : c1l_hlo(t));
        const int w = pr - 41 * h;
        hrow[tm] = h;
        pr8[tm] = (pr - 123) * 8;                                      // halves; record of kernel row dy = pr - 123 + 41 dy  (= (h + dy - 3) * 41 + w)
        w8[tm] = w * 8;
        // positions 205..207 (tile 12) go to the three unused slots at the end of row 4
        obase[tm] = ((g >> 1) * T_PL1 + (p < 205 ? h * T_R1 + w : 4 * T_R1 + 41 + (p - 205))) * 8 + (g & 1) * 4;
        asm volatile("" : "+v"(pr8[tm]), "+v"(w8[tm]), "+v"(obase[tm]), "+v"(hrow[tm]));     // (keeps the address arithmetic inside the site loop: no spills)
    }
    const int g1 = g * L_NR1 * 8, g0 = L_P0H + g * L_NR0 * 8;          // this lane group's slot plane
    auto a1 = [&](int tm, int dy) -> int {                             // operand of the 5-tap kernel row dy, rows 1..4
        const int t = tile_of(tm);
        int a = g1 + pr8[tm] + 41 * 8 * dy;
        if (!c1l_all1(t, dy)) { const int r = hrow[tm] + dy - 2; a = (r >= 1 && r <= 4) ? a : g1 + L_Z1 * 8; }
        return a;
    };
    auto a0 = [&](int tm, int dy) -> int {                             // the same of image row 0 (hi plane; the lo plane is L_P0L - L_P0H further)
        const int t = tile_of(tm);
        int a = g0 + w8[tm];
        if (!c1l_all0(t, dy)) a = (hrow[tm] + dy - 2 == 0) ? a : g0 + L_Z0 * 8;
        return a;
    };
    // 5x1 kernel: lane group g reads slot 0 (the centre pixel) of the record of ITS kernel row.  A: rows dy = g of P1.  B: g = 0: dy = 4 of P1;
    // g = 1..3: dy = g - 1 of the row-0 hi plane.  C: g = 0..2: dy = g of the row-0 lo plane.
    auto aA = [&](int tm) -> int { const int r = hrow[tm] + g - 2; return (r >= 1 && r <= 4) ? pr8[tm] + 41 * 8 * g : L_Z1 * 8; };
    auto aB = [&](int tm) -> int {
        const int h = hrow[tm];
        const int p1 = h <= 2 ? pr8[tm] + 41 * 8 * 4 : L_Z1 * 8, p0 = L_P0H + (h == 3 - g ? w8[tm] : L_Z0 * 8);
        return g == 0 ? p1 : p0;
    };
    auto aC = [&](int tm) -> int { return L_P0L + ((g < 3 && hrow[tm] == 2 - g) ? w8[tm] : L_Z0 * 8); };
    {
        const f32x4v x1 = *reinterpret_cast<const f32x4v *>(b1s + 4 * g) * rho, x2 = *reinterpret_cast<const f32x4v *>(b1s + 16 + 4 * g) * rho,
                     x3 = *reinterpret_cast<const f32x4v *>(b1s + 32 + 4 * g) * rho;
#pragma unroll
        for (int tm = 0; tm < NT; tm++) { acc1[tm] = x1; acc2[tm] = x2; acc3[tm] = x3; }
    }
    // steps 0..4: the 5-tap kernel rows dy (5x5 kernel; dy == 2 also feeds the 1x5 kernel); step 5: 5x1 group A; step 6: 5x1 groups B and C.
    // The operands of step s + DP are requested before the MFMAs of step s (register buffers).
    constexpr int DP = 1, NB = DP + 1;                      // steps requested ahead of the one being multiplied / register buffers
    h8 x1[NB][NT], xh[NB][2], xl[NB][2], xc[NT];
    auto load = [&](int s, int slot) {
        if (s < 5) {
            int n0 = 0;
#pragma unroll
            for (int tm = 0; tm < NT; tm++) {
                const int t = tile_of(tm);
                if (!use(tm, s)) continue;
                if (c1l_need1(t, s)) x1[slot][tm] = lds_h8(XB + a1(tm, s));
                if (c1l_need0(t, s)) { const int a = a0(tm, s); xh[slot][n0] = lds_h8(XB + a); xl[slot][n0] = lds_h8(XB + a + (L_P0L - L_P0H)); n0++; }
            }
        } else if (s == 5) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k51(tm)) x1[slot][tm] = lds_h8(XB + aA(tm));
        } else {
#pragma unroll
            for (int tm = 0; tm < NT; tm++)
                if (k51(tm) && c1l_low(tile_of(tm))) { x1[slot][tm] = lds_h8(XB + aB(tm)); xc[tm] = lds_h8(XB + aC(tm)); }
        }
    };
#pragma unroll
    for (int s = 0; s < DP; s++) load(s, s % NB);
#pragma unroll
    for (int s = 0; s < 7; s++) {
        const int cur = s % NB;
        if (s + DP < 7) load(s + DP, (s + DP) % NB);
        __builtin_amdgcn_sched_barrier(0);
        if (s < 5) {
            // independent accumulators interleaved; the three products of a row-0 operand pair are spread over the step
            // (n0: index of the tile's row-0 operand pair among those this wave loaded for the step)
            int n0 = 0;
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k55(tm) && c1l_need1(tile_of(tm), s)) { NC_MFMA(acc3[tm], wl[LW_5H + s], x1[cur][tm]) }
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (use(tm, s) && c1l_need0(tile_of(tm), s)) { if (k55(tm)) { NC_MFMA(acc3[tm], wl[LW_5H + s], xh[cur][n0]) } if (s == 2 && k15(tm)) { NC_MFMA(acc1[tm], wl[LW_1H], xh[cur][n0]) } n0++; }
            if (s == 2) {
#pragma unroll
                for (int tm = 0; tm < NT; tm++) if (k15(tm) && c1l_need1(tile_of(tm), s)) { NC_MFMA(acc1[tm], wl[LW_1H], x1[cur][tm]) }
            }
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k55(tm) && c1l_need1(tile_of(tm), s)) { NC_MFMA(acc3[tm], wl[LW_5L + s], x1[cur][tm]) }
            n0 = 0;
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (use(tm, s) && c1l_need0(tile_of(tm), s)) { if (k55(tm)) { NC_MFMA(acc3[tm], wl[LW_5H + s], xl[cur][n0]) } if (s == 2 && k15(tm)) { NC_MFMA(acc1[tm], wl[LW_1H], xl[cur][n0]) } n0++; }
            if (s == 2) {
#pragma unroll
                for (int tm = 0; tm < NT; tm++) if (k15(tm) && c1l_need1(tile_of(tm), s)) { NC_MFMA(acc1[tm], wl[LW_1L], x1[cur][tm]) }
            }
            n0 = 0;
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (use(tm, s) && c1l_need0(tile_of(tm), s)) { if (k55(tm)) { NC_MFMA(acc3[tm], wl[LW_5L + s], xh[cur][n0]) } if (s == 2 && k15(tm)) { NC_MFMA(acc1[tm], wl[LW_1L], xh[cur][n0]) } n0++; }
        } else if (s == 5) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k51(tm)) { NC_MFMA(acc2[tm], wl[LW_2HA], x1[cur][tm]) }
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k51(tm)) { NC_MFMA(acc2[tm], wl[LW_2LA], x1[cur][tm]) }
        } else {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k51(tm) && c1l_low(tile_of(tm))) { NC_MFMA(acc2[tm], wl[LW_2HB], x1[cur][tm]) }
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k51(tm) && c1l_low(tile_of(tm))) { NC_MFMA(acc2[tm], wl[LW_2HC], xc[tm]) }
#pragma unroll
            for (int tm = 0; tm < NT; tm++) if (k51(tm) && c1l_low(tile_of(tm))) { NC_MFMA(acc2[tm], wl[LW_2LB], x1[cur][tm]) }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// the epilogue of one accumulator of a conv1 tile: which = 0 the 1x5 kernel's 16 channels, 1 the 5x1 kernel's, 2 the 5x5 kernel's
__device__ __forceinline__ void c1l_epi_one(const f32x4v &acc, int which, int o, const h_epi &epi, _Float16 *A1H)
{
    split4_store(selu4_scaled(acc, epi), A1H + o + which * 2 * T_PL1 * 8, A1H + o + which * 2 * T_PL1 * 8 + T_A1PLANE);
}

template <int ROLE>
__device__ __forceinline__ void t_conv1_lin(const _Float16 *XB, _Float16 *A1H, const h8 (&wl)[T_NW1L], const float *__restrict__ b1s, const h_epi &epi, float rho, int lane)
{
    constexpr int NT = C1L_ROLES[ROLE].nt;
    static_assert(c1l_n0(ROLE, 0) <= 2 && c1l_n0(ROLE, 1) <= 2 && c1l_n0(ROLE, 2) <= 2, "t_conv1_lin: at most two row-0 operand pairs per kernel row and wave");
    f32x4v acc1[NT], acc2[NT], acc3[NT];
    int obase[NT];
    c1l_mma<ROLE>(XB, wl, b1s, rho, lane, acc1, acc2, acc3, obase);
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
        if (C1L_ROLES[ROLE].part[tm] & 1) c1l_epi_one(acc1[tm], 0, obase[tm], epi, A1H);
        if (C1L_ROLES[ROLE].part[tm] & 2) c1l_epi_one(acc2[tm], 1, obase[tm], epi, A1H);
        if (C1L_ROLES[ROLE].part[tm] & 4) c1l_epi_one(acc3[tm], 2, obase[tm], epi, A1H);
    }
}

// fp16 hi / lo of a float as one packed dword (lo in the upper half)
__device__ __forceinline__ uint32_t split_pack(float v)
{
    v = fminf(fmaxf(v, -65504.0f), 65504.0f);
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    return (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)__builtin_bit_cast(uint16_t, l) << 16);
}

__global__ __launch_bounds__(512) void k5_trunk_lin(const int16_t *__restrict__ x, const uint8_t *__restrict__ wp, const uint8_t *__restrict__ wlin, float *__restrict__ a3,
                                                    int64_t n_sites, const double *__restrict__ scale, int64_t site0, float x_limit, uint8_t *__restrict__ range_sites)
{
    __shared__ __attribute__((aligned(16))) _Float16 X[2][L_XBUF];
    __shared__ __attribute__((aligned(16))) _Float16 A1[2][2 * T_A1PLANE];
    __shared__ __attribute__((aligned(16))) _Float16 A2[2][2 * T_A2PLANE];
    __shared__ __attribute__((aligned(16))) float BIAS[48 + 32 + 64];
    // role of a hardware wave (roles 0, 1: conv2; 2, 3: staging + conv3; 4..7: conv1 roles 0..3).  Waves w and w + 4 share a SIMD and the lower-numbered one
    // is the older, which the issue arbiter prefers (MI355X_MICROARCH.md, two waves per SIMD): LIN_PERM lists the role of hardware waves 0..7.
    constexpr int LIN_PERM[8] = {2, 3, 4, 5, 6, 7, 0, 1};
    const int lane = threadIdx.x & 63, wv = LIN_PERM[threadIdx.x >> 6];
    const uint4 *w1f = reinterpret_cast<const uint4 *>(wp), *w2h = w1f + T_NW1 * 64, *w2l = w2h + T_NW2 * 64, *w3h = w2l + T_NW2 * 64, *w3l = w3h + T_NW3 * 64;
    const uint4 *wlf = reinterpret_cast<const uint4 *>(wlin);
    const float *bg = reinterpret_cast<const float *>(w3l + T_NW3 * 64);
    const float *b1s = BIAS, *b2s = BIAS + 48, *b3s = BIAS + 80;
    const int *c3tab = reinterpret_cast<const int *>(bg + 48 + 32 + 68);
    const float inv_s = bg[48 + 32 + 64];
    if (threadIdx.x < 48 + 32 + 64) BIAS[threadIdx.x] = bg[threadIdx.x];
    const h_epi epi = {inv_s * 1.44269504088896341f, inv_s * SELU_L, 60000.0f / (inv_s * SELU_L)};
    const int64_t n_k = (n_sites - blockIdx.x + gridDim.x - 1) / gridDim.x;        // sites of this workgroup (>= 1)
    for (int i = threadIdx.x; i < 2 * L_XBUF / 8; i += 512) *reinterpret_cast<uint4 *>(&X[0][0] + i * 8) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    // coverage scale of a site (snpCaller.py:93-96): s as float (numpy's float32 product in both modes up to one rounding of the operand, which this
    // kernel does not perform at all), 1 without a scale array
    auto site_scale = [&](int64_t k) -> float { return scale ? (float)scale[site0 + blockIdx.x + k * gridDim.x] : 1.0f; };
    const int64_t n_steps = n_k + 2;
    if (wv >= 4) {
        // ------------------------------------------------------------------ conv1 of site s
        h8 wl[T_NW1L];
#pragma unroll
        for (int q = 0; q < T_NW1L; q++) wl[q] = as_h8(wlf[q * 64 + lane]);
        float s_next = site_scale(0);
        __syncthreads();                                                           // P0
        for (int64_t s = 0; s < n_steps; s++) {
            if (s < n_k) {
                const int buf = (int)(s & 1);
                const float sf = s_next, rho = 1.0f / sf;
                if (s + 1 < n_k) s_next = site_scale(s + 1);                       // (a scalar load: a step ahead of its use)
                const h_epi e1 = {epi.c1 * sf, epi.c2 * sf, epi.c3 * rho};         // the accumulators hold S / s x (pre-activation)
                if (wv == 4) t_conv1_lin<0>(X[buf], A1[buf], wl, b1s, e1, rho, lane);
                else if (wv == 5) t_conv1_lin<1>(X[buf], A1[buf], wl, b1s, e1, rho, lane);
                else if (wv == 6) t_conv1_lin<2>(X[buf], A1[buf], wl, b1s, e1, rho, lane);
                else t_conv1_lin<3>(X[buf], A1[buf], wl, b1s, e1, rho, lane);
            }
            __syncthreads();
        }
    } else if (wv < 2) {
        // ------------------------------------------------------------------ conv2 of site s - 1
        h8 c2h[9][2], c2l[9][2];
#pragma unroll
        for (int q = 0; q < 9; q++)
#pragma unroll
            for (int tn = 0; tn < 2; tn++) { c2h[q][tn] = as_h8(w2h[(q * 2 + tn) * 64 + lane]); c2l[q][tn] = as_h8(w2l[(q * 2 + tn) * 64 + lane]); }
        __syncthreads();                                                           // P0
        for (int64_t s = 0; s < n_steps; s++) {
            if (s >= 1 && s - 1 < n_k) {
                const int buf = (int)((s - 1) & 1);
                if (wv == 0) t_conv2_pair<0>(A1[buf], A2[buf], c2h, c2l, b2s, epi, lane);
                else t_conv2_pair<1>(A1[buf], A2[buf], c2h, c2l, b2s, epi, lane);
            }
            __syncthreads();
        }
    } else {
        // ------------------------------------------------------------------ staging of site s + 1, conv3 of site s - 2
        const int cw = wv - 2;
        h8 c3h[6][2], c3l[6][2];
#pragma unroll
        for (int q = 0; q < 6; q++)
#pragma unroll
            for (int tn = 0; tn < 2; tn++) {
                c3h[q][tn] = as_h8(w3h[(q * 4 + 2 * cw + tn) * 64 + lane]);
                c3l[q][tn] = as_h8(w3l[(q * 4 + 2 * cw + tn) * 64 + lane]);
            }
        const int c3slot[2] = {c3tab[lane & 15], c3tab[16 + (lane & 15)]}, c3out[2] = {c3tab[32 + (lane & 15)], c3tab[48 + (lane & 15)]};
        const int st = (wv - 2) * 64 + lane;                                      // 0..127: pixels st and st + 128 (< 205) of the 5 x 41 image
        uint32_t raw[2][3];
        float pre_s = 1.0f;
        int64_t pre_site = 0;
        auto prefetch = [&](int64_t k) {                                           // issues the loads of the workgroup's k-th site; commit() converts them a step later
            const int64_t site = (int64_t)blockIdx.x + k * gridDim.x;
            pre_site = site;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int t = st + 128 * j, px = t < 205 ? t : 204;
                const int16_t *xs = x + site * NC_SNP_TENSOR + px * 5;             // 2-byte aligned
                typedef uint32_t __attribute__((aligned(2))) u32_a2;
                raw[j][0] = *reinterpret_cast<const u32_a2 *>(xs);
                raw[j][1] = *reinterpret_cast<const u32_a2 *>(xs + 2);
                raw[j][2] = (uint32_t)(uint16_t)xs[4];
            }
            pre_s = site_scale(k);
        };
        auto commit = [&](int buf) {
            const float sf = pre_s, rho = 1.0f / sf;
            _Float16 *XB = &X[buf][0];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (st + 128 * j >= 205) continue;
                const int px = st + 128 * j, ph = px / 41, pw = px - ph * 41;
                const int v0 = (int16_t)(raw[j][0] & 0xffffu), v1 = (int16_t)(raw[j][0] >> 16), v2 = (int16_t)(raw[j][1] & 0xffffu), v3 = (int16_t)(raw[j][1] >> 16),
                          v4 = (int16_t)raw[j][2];
                const int m4 = max(max(abs(v0), abs(v1)), max(abs(v2), abs(v3)));
                // range guard: the scaled entries as the epilogue sees them (|x| s), the unscaled ones as they are; integers beyond fp16's exact range
                // (2048) cannot take this kernel at all.  Flagged sites are computed again by the exact fp32 trunk (nc_cnn_range_watch).
                // An unscaled entry travels as u * rho in fp16 hi + lo: it must stay inside fp16's range, and rho's lo half must not sink into the
                // subnormals (s <= 64; a scale that is not a positive finite number takes the exact trunk as well).
                const float un = ph > 0 ? fabsf((float)v4) : fmaxf((float)m4, fabsf((float)v4));
                const float amax = ph > 0 ? fmaxf((float)m4 * sf, un) : un;
                if (range_sites && (!(amax <= x_limit) || (ph > 0 && m4 > 2048) || !(un * rho <= 60000.0f) || !(sf > 0.0f && sf <= 64.0f)))
                    range_sites[site0 + pre_site] = 1;
                // the pixel's 6 K values as three dwords per plane
                uint32_t d[2][3];
                const uint32_t u4 = split_pack((float)v4 * rho);
                if (ph > 0) {
                    const h2 q01 = {(_Float16)(float)v0, (_Float16)(float)v1}, q23 = {(_Float16)(float)v2, (_Float16)(float)v3};      // exact: |v| <= 2048
                    d[0][0] = __builtin_bit_cast(uint32_t, q01); d[0][1] = __builtin_bit_cast(uint32_t, q23); d[0][2] = u4;              // [x0 x1 x2 x3 hi(u4 rho) lo(u4 rho)]
                } else {
                    const uint32_t u0 = split_pack((float)v0 * rho), u1 = split_pack((float)v1 * rho), u2 = split_pack((float)v2 * rho), u3 = split_pack((float)v3 * rho);
                    d[0][0] = (u0 & 0xffffu) | (u1 << 16); d[0][1] = (u2 & 0xffffu) | (u3 << 16); d[0][2] = u4 & 0xffffu;                // hi plane [h0 h1 h2 h3 h4 0]
                    d[1][0] = (u0 >> 16) | (u1 & 0xffff0000u); d[1][1] = (u2 >> 16) | (u3 & 0xffff0000u); d[1][2] = u4 >> 16;            // lo plane [l0 l1 l2 l3 l4 0]
                }
                // the pixel is element i of the records of columns w' = pw - L_DXO[i] of its row: K slots 6 i .. 6 i + 5 of that record
                const int nr = ph > 0 ? L_NR1 : L_NR0, rec0 = ph > 0 ? (ph - 1) * 41 : 0, dump = ph > 0 ? L_DUMP1 : L_DUMP0, pbase = ph > 0 ? 0 : L_P0H;
#pragma unroll
                for (int i = 0; i < 5; i++) {
                    const int wq = pw - L_DXO[i];
                    const int rec = (wq >= 0 && wq <= 40) ? rec0 + wq : dump;
                    constexpr int NPL = 2;
#pragma unroll
                    for (int pl = 0; pl < NPL; pl++) {
                        if (pl == 1 && ph > 0) continue;
                        _Float16 *rb = XB + pbase + pl * (L_P0L - L_P0H) + rec * 8;
                        const int k0 = 6 * i, sl = k0 >> 3, of = k0 & 7;            // first K slot: 16-byte slot sl, half `of` (0, 6, 4, 2, 0)
                        _Float16 *q0 = rb + sl * nr * 8 + of;
                        if (of == 0) { *reinterpret_cast<uint2 *>(q0) = make_uint2(d[pl][0], d[pl][1]); *reinterpret_cast<uint32_t *>(q0 + 4) = d[pl][2]; }
                        else if (of == 6) { *reinterpret_cast<uint32_t *>(q0) = d[pl][0]; *reinterpret_cast<uint2 *>(rb + (sl + 1) * nr * 8) = make_uint2(d[pl][1], d[pl][2]); }
                        else if (of == 4) { *reinterpret_cast<uint2 *>(q0) = make_uint2(d[pl][0], d[pl][1]); *reinterpret_cast<uint32_t *>(rb + (sl + 1) * nr * 8) = d[pl][2]; }
                        else { *reinterpret_cast<uint32_t *>(q0) = d[pl][0]; *reinterpret_cast<uint2 *>(q0 + 2) = make_uint2(d[pl][1], d[pl][2]); }
                    }
                }
            }
        };
        int64_t site = blockIdx.x;                                                 // the site conv3's epilogue stores next
        prefetch(0);
        commit(0);
        if (n_k > 1) prefetch(1);
        __syncthreads();                                                           // P0
        for (int64_t s = 0; s < n_steps; s++) {
            // the other X buffer's last reader was conv1 of site s - 1 (a barrier ago); site s + 1's loads were issued a step ago
            if (s + 1 < n_k) commit((int)((s + 1) & 1));
            if (s + 2 < n_k) prefetch(s + 2);
            if (s >= 2) {
                const int buf = (int)(s & 1);
                float *out_site = a3 + site * (27 * 64);
                if (cw == 0) t_conv3_pair<0>(A2[buf], c3h, c3l, b3s, epi, out_site, c3slot, c3out, lane);
                else t_conv3_pair<1>(A2[buf], c3h, c3l, b3s, epi, out_site, c3slot, c3out, lane);
                site += gridDim.x;
            }
            __syncthreads();
        }
    }
}

#undef NC_MFMA

// ---- fc1 on the same split-precision scheme: out[site][48] = selu(W^T a3 + b), K = 1728 = 54 groups of 32.
// A workgroup owns 64 sites (4 position... site tiles of 16) so that every weight fragment read from L2 feeds 4 MFMAs per
// product; the four waves split K and combine through LDS.  The fp32 activations are split into fp16 hi/lo on load (each
// lane reads the 8 K values of its site as two dwordx4: the four lane groups of a site cover one 128-byte line).
constexpr int FC_K = 1728, FC_G = FC_K / 32, FC_TM = 4, FC_TN = 3;
constexpr int FC_PACKED_BYTES = 2 * FC_G * FC_TN * T_FRAG * 2 + 4 * 64;        // hi + lo fragments, then b*S[48], 1/S
__device__ __forceinline__ void split8(const float4 &a, const float4 &b, h8 &hi, h8 &lo)
{
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t uh[4], ul[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const float x0 = v[2 * p], x1 = v[2 * p + 1];                  // selu outputs clamped to fp16 range by the trunk's conv3 epilogue
        const h2 h = __builtin_convertvector((f32x2v){x0, x1}, h2);
        uh[p] = __builtin_bit_cast(uint32_t, h);
        const f32x2v d = {sub_h_lo(x0, uh[p]), sub_h_hi(x1, uh[p])};
        ul[p] = __builtin_bit_cast(uint32_t, (h2)__builtin_convertvector(d, h2));
    }
    hi = as_h8(make_uint4(uh[0], uh[1], uh[2], uh[3]));
    lo = as_h8(make_uint4(ul[0], ul[1], ul[2], ul[3]));
}

__global__ __launch_bounds__(256) void k6_fc1_h3(const float *__restrict__ in, const uint8_t *__restrict__ wp, float *__restrict__ out, int64_t n)
{
    __shared__ f32x4v red[3][FC_TM][FC_TN][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, c16 = lane & 15;
    const uint4 *wh = reinterpret_cast<const uint4 *>(wp), *wl = wh + FC_G * FC_TN * 64;
    const float *bs = reinterpret_cast<const float *>(wl + FC_G * FC_TN * 64);
    const float inv_s = bs[48];
    const int64_t tile0 = (int64_t)blockIdx.x * (FC_TM * 16);
    const float *ip[FC_TM];
#pragma unroll
    for (int tm = 0; tm < FC_TM; tm++) {
        int64_t s = tile0 + tm * 16 + c16;
        if (s >= n) s = n - 1;
        ip[tm] = in + s * FC_K + 8 * g;
    }
    f32x4v acc[FC_TM][FC_TN];
#pragma unroll
    for (int tn = 0; tn < FC_TN; tn++) {
        f32x4v b = {0.0f, 0.0f, 0.0f, 0.0f};
        if (wv == 0) b = *reinterpret_cast<const f32x4v *>(bs + tn * 16 + 4 * g);
#pragma unroll
        for (int tm = 0; tm < FC_TM; tm++) acc[tm][tn] = b;
    }
    const int j0 = (FC_G * wv) / 4, j1 = (FC_G * (wv + 1)) / 4;
#pragma unroll 2
    for (int G = j0; G < j1; G++) {
        float4 a0[FC_TM], a1[FC_TM];
#pragma unroll
        for (int tm = 0; tm < FC_TM; tm++) {
            a0[tm] = *reinterpret_cast<const float4 *>(ip[tm] + 32 * G);
            a1[tm] = *reinterpret_cast<const float4 *>(ip[tm] + 32 * G + 4);
        }
        h8 bh[FC_TN], bl[FC_TN];
#pragma unroll
        for (int tn = 0; tn < FC_TN; tn++) {
            bh[tn] = as_h8(wh[(G * FC_TN + tn) * 64 + lane]);
            bl[tn] = as_h8(wl[(G * FC_TN + tn) * 64 + lane]);
        }
#pragma unroll
        for (int tm = 0; tm < FC_TM; tm++) {
            h8 xh, xl;
            split8(a0[tm], a1[tm], xh, xl);
#pragma unroll
            for (int tn = 0; tn < FC_TN; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[tn], xh, acc[tm][tn], 0, 0, 0);
#pragma unroll
            for (int tn = 0; tn < FC_TN; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[tn], xl, acc[tm][tn], 0, 0, 0);
#pragma unroll
            for (int tn = 0; tn < FC_TN; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[tn], xh, acc[tm][tn], 0, 0, 0);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int tm = 0; tm < FC_TM; tm++)
#pragma unroll
            for (int tn = 0; tn < FC_TN; tn++) red[wv - 1][tm][tn][lane] = acc[tm][tn];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int tm = 0; tm < FC_TM; tm++) {
            const int64_t s = tile0 + tm * 16 + c16;                   // D[channel 4g + r][site c16]
#pragma unroll
            for (int tn = 0; tn < FC_TN; tn++) {
                const f32x4v v = (acc[tm][tn] + red[0][tm][tn][lane] + red[1][tm][tn][lane] + red[2][tm][tn][lane]) * inv_s;
                if (s < n) *reinterpret_cast<f32x4v *>(out + s * 48 + tn * 16 + 4 * g) = (f32x4v){selu(v[0]), selu(v[1]), selu(v[2]), selu(v[3])};
            }
        }
    }
}

}   // namespace

SnpTrunk nc_cnn_snp_trunk_select(const nc_ctx *ctx)
{
    if (ctx->cnn_exact_fp32) return {NC_TRUNK_FP32, T_MFMA_PER_SITE};
    const char *el = getenv("NC_TRUNK_LIN");
    if (ctx->x_i16 && !(el && el[0] == '0')) return {NC_TRUNK_LIN, L_MFMA_PER_SITE};
    return {NC_TRUNK_P3, T_MFMA_PER_SITE};
}

void nc_cnn_launch_k5_trunk(int kernel_id, const SnpTrunkArgs &a, const uint8_t *packed_h)
{
    const unsigned nblk = (unsigned)(a.nb < 256 ? a.nb : 256);          // one 512-thread workgroup per CU
    if (kernel_id == NC_TRUNK_LIN)
        // both scale modes are the same arithmetic here: the scale multiplies the accumulators, not the operand
        hipExtLaunchKernelGGL(k5_trunk_lin, dim3(nblk), dim3(512), 0, a.stream, a.ev0, a.ev1, 0, a.x_i16, packed_h, packed_h + H_PACKED_BYTES + FC_PACKED_BYTES, a.a3,
                              a.nb, a.scale, a.site0, a.x_limit, a.range_sites);
    else if (a.x_i16)                                                    // (k5_trunk_p3<true> takes its int16 tensors through the float pointer)
        hipExtLaunchKernelGGL(k5_trunk_p3<true>, dim3(nblk), dim3(512), 0, a.stream, a.ev0, a.ev1, 0, reinterpret_cast<const float *>(a.x_i16), packed_h, a.a3, a.nb,
                              a.scale, a.scale_mode, a.site0, a.x_limit, a.range_sites);
    else
        hipExtLaunchKernelGGL(k5_trunk_p3<false>, dim3(nblk), dim3(512), 0, a.stream, a.ev0, a.ev1, 0, a.x_f32, packed_h, a.a3, a.nb, a.scale, a.scale_mode, a.site0,
                              a.x_limit, a.range_sites);
}

void nc_cnn_launch_fc1_h3(hipStream_t st, const float *a3, const uint8_t *packed_h, float *f1, int64_t nb)
{
    hipLaunchKernelGGL(k6_fc1_h3, dim3(blocks_for(nb, 16 * FC_TM)), dim3(256), 0, st, a3, packed_h + H_PACKED_BYTES, f1, nb);
}

// ---- host: the three packers.  Canonical blob of an SNP model: k11 [5][5][16] b11 k12 [5][5][16] b12 k13 [25][5][16] b13 k2 [6][48][32] b2
// k3 [6][32][64] b3 kf [1728][48] bf, then the heads.
namespace {

struct SnpBlob {
    const float *k11, *b11, *k12, *b12, *k13, *b13, *k2, *b2, *k3, *b3, *kf, *bf;
    explicit SnpBlob(const float *w)
        : k11(w), b11(k11 + 400), k12(b11 + 16), b12(k12 + 400), k13(b12 + 16), b13(k13 + 2000), k2(b13 + 16), b2(k2 + 6 * 48 * 32), k3(b2 + 32), b3(k3 + 6 * 32 * 64),
          kf(b3 + 64), bf(kf + FC_K * 48)
    {
    }
};

// fragments of the k5 trunks (conv1 in the pixel form of k5_trunk_p3), the biases x S, 1 / S, conv3's lane -> position tables
void pack_trunk(const SnpBlob &m, const H3Scale &sc, uint8_t *dst)
{
    _Float16 *w1f = reinterpret_cast<_Float16 *>(dst), *w2h = w1f + T_NW1 * T_FRAG, *w2l = w2h + T_NW2 * T_FRAG, *w3h = w2l + T_NW2 * T_FRAG, *w3l = w3h + T_NW3 * T_FRAG;
    float *b1s = reinterpret_cast<float *>(w3l + T_NW3 * T_FRAG), *b2s = b1s + 48, *b3s = b2s + 32;
    int32_t *c3tab = reinterpret_cast<int32_t *>(b3s + 68);
    // conv1 fragment pair (WA at fragment fa, WB at fragment fb) of one lane: kw[ci] = the 5 channel weights of its tap
    auto put_tap = [&](int fa, int fb, int lane, const float *kw /* 5 or nullptr */) {
        _Float16 H[5], L[5];
        for (int ci = 0; ci < 5; ci++) sc.split(kw ? kw[ci] : 0.0f, H[ci], L[ci]);
        _Float16 *A = w1f + ((size_t)fa * 64 + lane) * 8, *B = w1f + ((size_t)fb * 64 + lane) * 8;
        const _Float16 wa[8] = {H[0], H[1], H[2], H[3], H[4], H[0], H[1], H[2]};
        const _Float16 wb[8] = {H[3], H[4], L[0], L[1], L[2], L[3], L[4], (_Float16)0.0f};
        for (int j = 0; j < 8; j++) { A[j] = wa[j]; B[j] = wb[j]; }
    };
    for (int lane = 0; lane < 64; lane++) {
        const int g = lane >> 4, c = lane & 15;
        for (int G = 0; G < 7; G++) {
            const int dy = C1_TAPS[G][g][0], dx = C1_TAPS[G][g][1];
            // a tap listed twice in a group (dummy lanes) carries its weights only at its first occurrence
            bool first = true;
            for (int q = 0; q < g; q++) first = first && !(C1_TAPS[G][q][0] == dy && C1_TAPS[G][q][1] == dx);
            float kw[5];
            for (int ci = 0; ci < 5; ci++) kw[ci] = m.k13[((dy * 5 + dx) * 5 + ci) * 16 + c];
            put_tap(G, 7 + G, lane, first ? kw : nullptr);
            if (G < 2) {                                                         // 1x5 kernel: taps of image row dy == 2
                for (int ci = 0; ci < 5; ci++) kw[ci] = m.k11[(dx * 5 + ci) * 16 + c];
                put_tap(14 + G, 16 + G, lane, (first && dy == 2) ? kw : nullptr);
            }
            if (G >= 1 && G <= 3) {                                              // 5x1 kernel: taps of image column dx == 2
                for (int ci = 0; ci < 5; ci++) kw[ci] = m.k12[(dy * 5 + ci) * 16 + c];
                put_tap(18 + G - 1, 21 + G - 1, lane, (first && dx == 2) ? kw : nullptr);
            }
        }
        for (int j = 0; j < 8; j++) {
            for (int G = 0; G < 9; G++) {
                const int idx = 4 * G + g, tap = idx / 6, ch = (idx % 6) * 8 + j;
                for (int tn = 0; tn < 2; tn++) {
                    const size_t o = ((size_t)(G * 2 + tn) * 64 + lane) * 8 + j;
                    sc.split(m.k2[(tap * 48 + ch) * 32 + tn * 16 + c], w2h[o], w2l[o]);
                }
            }
            for (int G = 0; G < 6; G++)
                for (int tn = 0; tn < 4; tn++) {
                    const size_t o = ((size_t)(G * 4 + tn) * 64 + lane) * 8 + j;
                    sc.split(m.k3[(G * 32 + 8 * g + j) * 64 + tn * 16 + c], w3h[o], w3l[o]);
                }
        }
    }
    const float S = sc.S;
    for (int c = 0; c < 16; c++) { b1s[c] = m.b11[c] * S; b1s[16 + c] = m.b12[c] * S; b1s[32 + c] = m.b13[c] * S; }
    for (int c = 0; c < 32; c++) b2s[c] = m.b2[c] * S;
    for (int c = 0; c < 64; c++) b3s[c] = m.b3[c] * S;
    b3s[64] = 1.0f / S;
    for (int i = 0; i < 32; i++) { c3tab[i] = C3_SLOT[i]; c3tab[32 + i] = C3_OUT[i]; }
}

// fc1 fragments for k6_fc1_h3: own power-of-two scale, A operand = W^T (row = output unit, K = 32 G + 8 g + j)
void pack_fc1(const SnpBlob &m, uint8_t *dst)
{
    const H3Scale sc(m.kf, m.bf + 48, 1024.0f);
    _Float16 *fh = reinterpret_cast<_Float16 *>(dst), *fl = fh + (size_t)FC_G * FC_TN * T_FRAG;
    float *fbs = reinterpret_cast<float *>(fl + (size_t)FC_G * FC_TN * T_FRAG);
    for (int G = 0; G < FC_G; G++)
        for (int tn = 0; tn < FC_TN; tn++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int g = lane >> 4, c = lane & 15;
                    const size_t o = ((size_t)(G * FC_TN + tn) * 64 + lane) * 8 + j;
                    sc.split(m.kf[(size_t)(32 * G + 8 * g + j) * 48 + tn * 16 + c], fh[o], fl[o]);
                }
    for (int c = 0; c < 48; c++) fbs[c] = m.bf[c] * sc.S;
    fbs[48] = 1.0f / sc.S;
}

// conv1 fragments of k5_trunk_lin (record form): K slot k = 6 i + v of a 5-tap kernel row = pixel i (column offset L_DXO[i]), value v of
// [x0 x1 x2 x3 hi(u4 rho) lo(u4 rho)]; the lo-weight fragment has no entry for v = 5 (lo x lo is dropped, as everywhere)
void pack_lin(const SnpBlob &m, const H3Scale &sc, uint8_t *dst)
{
    _Float16 *lf = reinterpret_cast<_Float16 *>(dst);
    auto lput = [&](int frag, int lane, int j, _Float16 v) { lf[((size_t)frag * 64 + lane) * 8 + j] = v; };
    const _Float16 Z = (_Float16)0.0f;
    for (int lane = 0; lane < 64; lane++) {
        const int g = lane >> 4, c = lane & 15;
        for (int j = 0; j < 8; j++) {
            _Float16 H, L;
            const int k = 8 * g + j;
            if (k < 30) {
                const int i = k / 6, v = k % 6, dx = 2 + L_DXO[i], ci = v < 4 ? v : 4;
                for (int dy = 0; dy < 5; dy++) {
                    sc.split(m.k13[((dy * 5 + dx) * 5 + ci) * 16 + c], H, L);
                    lput(LW_5H + dy, lane, j, H);
                    lput(LW_5L + dy, lane, j, v == 5 ? Z : L);
                }
                sc.split(m.k11[(dx * 5 + ci) * 16 + c], H, L);
                lput(LW_1H, lane, j, H);
                lput(LW_1L, lane, j, v == 5 ? Z : L);
            }
            // 5x1 kernel: slot 0 of a record = the centre pixel's six values (+ two of another pixel: zero weights)
            if (j < 6) {
                const int ci = j < 4 ? j : 4;
                sc.split(m.k12[(g * 5 + ci) * 16 + c], H, L);                       // group A: kernel row dy = g, rows 1..4
                lput(LW_2HA, lane, j, H);
                lput(LW_2LA, lane, j, j == 5 ? Z : L);
                const int dyb = g == 0 ? 4 : g - 1;                             // group B: g = 0: dy = 4 of rows 1..4; g >= 1: dy = g - 1 of the row-0 hi plane
                sc.split(m.k12[(dyb * 5 + ci) * 16 + c], H, L);
                lput(LW_2HB, lane, j, (g > 0 && j == 5) ? Z : H);
                lput(LW_2LB, lane, j, j == 5 ? Z : L);
                if (g < 3) {                                                     // group C: dy = g of the row-0 lo plane
                    sc.split(m.k12[(g * 5 + ci) * 16 + c], H, L);
                    lput(LW_2HC, lane, j, j == 5 ? Z : H);
                }
            }
        }
    }
}

}   // namespace

std::vector<uint8_t> nc_cnn_pack_snp_h3(const float *blob)
{
    const SnpBlob m(blob);
    const H3Scale sc(blob, m.b3 + 64, 1024.0f);                           // one scale for conv1-conv3 (both forms of conv1)
    std::vector<uint8_t> hp((size_t)H_PACKED_BYTES + FC_PACKED_BYTES + L_PACKED_BYTES, 0);
    pack_trunk(m, sc, hp.data());
    pack_fc1(m, hp.data() + H_PACKED_BYTES);
    pack_lin(m, sc, hp.data() + H_PACKED_BYTES + FC_PACKED_BYTES);
    return hp;
}

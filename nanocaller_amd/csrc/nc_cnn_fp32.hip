// The exact-fp32 forms of the CNN (gfx950; see nc_cnn.h): v_mfma_f32_16x16x4_f32 is bit for bit an fmaf chain.
//   k2_conv1_x4 + k7_conv23_mfma x 2   the indel trunk (nc_set_cnn_precision(ctx, 1), or a model whose range bound does not cover |x| <= 1)
//   k4_conv12                          the SNP trunk (conv1-conv3), with the F12_* layout of its weight fragments and their packer
//   k3_fc1<48, 1> / <32, 2>            fc1 of the SNP models in exact mode / of the indel models always
#include <hip/hip_ext.h>

#include "nc_cnn.h"

namespace {

// conv1 of the indel models (CI = 2, W a multiple of 4), four x-adjacent output positions per thread: the 5 x 8 input
// window of the four positions is loaded once (20 dwordx4 instead of 100 8-byte loads) and every weight, a wave-uniform
// scalar operand, feeds four FMAs.  The fmaf chain of an output runs in the reference's order (tap-major, channel-minor).
// Canonical weights: k11[1][5][CI][C1] b11 k12[5][1][CI][C1] b12 k13[5][5][CI][C1] b13.  Output NHWC [site][H][W][3*C1].
template <int H, int W, int C1>
__global__ __launch_bounds__(256) void k2_conv1_x4(const float *__restrict__ x, const float *__restrict__ w, float *__restrict__ out, int64_t npos)
{
    static_assert(W % 4 == 0 && C1 == 8, "k2_conv1_x4: shape");
    constexpr int CI = 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t * 4 >= npos) return;
    const int64_t g0 = t * 4, site = g0 / (H * W);
    const int r = (int)(g0 - site * (H * W));
    const int h = r / W, x0 = r - h * W;                                  // x0 % 4 == 0
    const float *xs = x + site * (H * W * CI);
    const float *k11 = w, *b11 = k11 + 5 * CI * C1;
    const float *k12 = b11 + C1, *b12 = k12 + 5 * CI * C1;
    const float *k13 = b12 + C1, *b13 = k13 + 25 * CI * C1;
    float a1[4][C1], a2[4][C1], a3[4][C1];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int o = 0; o < C1; o++) { a1[p][o] = b11[o]; a2[p][o] = b12[o]; a3[p][o] = b13[o]; }
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int iy = h + dy;
        // pixels x0-2 .. x0+5 of row iy, two channels each: 16 floats (zero outside the image)
        float win[16];
        const bool row_in = iy >= 0 && iy < H;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int px = x0 - 2 + 2 * q;                                 // pixel pair (px, px + 1): both inside or both outside
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row_in && px >= 0 && px + 1 < W) v = *reinterpret_cast<const float4 *>(xs + ((int64_t)iy * W + px) * CI);
            win[4 * q] = v.x; win[4 * q + 1] = v.y; win[4 * q + 2] = v.z; win[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
#pragma unroll
            for (int c = 0; c < CI; c++) {
                const float *w3 = k13 + (((dy + 2) * 5 + (dx + 2)) * CI + c) * C1;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const float xv = win[(p + dx + 2) * CI + c];
#pragma unroll
                    for (int o = 0; o < C1; o++) a3[p][o] = fmaf(xv, w3[o], a3[p][o]);
                }
                if (dy == 0) {
                    const float *w1 = k11 + ((dx + 2) * CI + c) * C1;
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const float xv = win[(p + dx + 2) * CI + c];
#pragma unroll
                        for (int o = 0; o < C1; o++) a1[p][o] = fmaf(xv, w1[o], a1[p][o]);
                    }
                }
                if (dx == 0) {
                    const float *w2 = k12 + ((dy + 2) * CI + c) * C1;
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const float xv = win[(p + 2) * CI + c];
#pragma unroll
                        for (int o = 0; o < C1; o++) a2[p][o] = fmaf(xv, w2[o], a2[p][o]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        float4 *op = reinterpret_cast<float4 *>(out + (g0 + p) * (3 * C1));
#pragma unroll
        for (int o = 0; o < C1; o += 4) {
            op[o / 4] = make_float4(selu(a1[p][o]), selu(a1[p][o + 1]), selu(a1[p][o + 2]), selu(a1[p][o + 3]));
            op[(C1 + o) / 4] = make_float4(selu(a2[p][o]), selu(a2[p][o + 1]), selu(a2[p][o + 2]), selu(a2[p][o + 3]));
            op[(2 * C1 + o) / 4] = make_float4(selu(a3[p][o]), selu(a3[p][o + 1]), selu(a3[p][o + 2]), selu(a3[p][o + 3]));
        }
    }
}

// ---- MFMA forms (SNP trunk).  fp32-in/fp32-accumulate MFMA is bit-for-bit an fmaf chain (exact fp32).
// GEMM view: M = output positions or sites (A fragment: one activation per lane), N = output channels (B fragment:
// one weight per lane), K = (tap, ci) walked in a permuted order so that the 4 consecutive input channels a lane
// loads as ONE dwordx4 feed 4 consecutive MFMAs.

// fc1 as v_mfma_f32_16x16x4: M = 16 sites per tile, N = F/16 tiles, K walked in groups of 16 (quarter-wave q takes
// k in [16j+4q, 16j+4q+4) as one dwordx4).  lane l: A[row l&15][k l>>4], B[k l>>4][col l&15]; C: col l&15, row 4*(l>>4)+r.
// Split-K: the four waves of a workgroup share the same 16*TM sites and each takes a quarter of K; partial sums are
// combined through LDS (K = 1728 would otherwise be one 40k-cycle dependent chain per wave).
template <int F, int TM>
__global__ __launch_bounds__(256) void k3_fc1(const float *__restrict__ in, int K, const float *__restrict__ wk, const float *__restrict__ wb,
                                              float *__restrict__ out, int64_t n)
{
    constexpr int TN = F / 16;
    __shared__ float red[3][TM][TN][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = lane >> 4, c16 = lane & 15;
    const int64_t tile0 = (int64_t)blockIdx.x * (TM * 16);
    const float *ip[TM];
#pragma unroll
    for (int tm = 0; tm < TM; tm++) {
        int64_t s = tile0 + tm * 16 + c16;
        if (s >= n) s = n - 1;
        ip[tm] = in + s * K + 4 * q;
    }
    f32x4v acc[TM][TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const float b = wv == 0 ? wb[tn * 16 + c16] : 0.0f;
#pragma unroll
        for (int tm = 0; tm < TM; tm++) acc[tm][tn] = (f32x4v){b, b, b, b};
    }
    const float *wl = wk + (4 * q) * F + c16;
    const int ng = K / 16;
    const int j0 = (ng * wv) / 4, j1 = (ng * (wv + 1)) / 4;
    // The loads of group j + NS - 1 are issued before the MFMAs of group j: a wave keeps NS - 1 groups (activations from HBM,
    // weights from L2) in flight instead of waiting for each group's loads with nothing behind them.
    constexpr int NS = TM <= 2 ? 4 : 2;
    float4 a[NS][TM];
    float b[NS][4][TN];
    auto ld = [&](int st, int j) {
        j = min(j, j1 - 1);                                             // (past the end: the last group again, unused)
#pragma unroll
        for (int tm = 0; tm < TM; tm++) a[st][tm] = *reinterpret_cast<const float4 *>(ip[tm] + 16 * j);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int tn = 0; tn < TN; tn++) b[st][i][tn] = wl[(int64_t)(16 * j + i) * F + tn * 16];
    };
    if (j0 < j1) {
#pragma unroll
        for (int st = 0; st < NS - 1; st++) ld(st, j0 + st);
    }
    auto mm = [&](int u) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int tm = 0; tm < TM; tm++) {
                const float av = i == 0 ? a[u][tm].x : i == 1 ? a[u][tm].y : i == 2 ? a[u][tm].z : a[u][tm].w;
#pragma unroll
                for (int tn = 0; tn < TN; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[u][i][tn], acc[tm][tn], 0, 0, 0);
            }
    };
    int j = j0;
    for (; j + NS <= j1; j += NS) {                                     // whole rounds: no branch between a load and its use
#pragma unroll
        for (int u = 0; u < NS; u++) {
            ld((u + NS - 1) % NS, j + u + NS - 1);
            __builtin_amdgcn_sched_barrier(0);                          // (the scheduler otherwise sinks these loads below the products)
            mm(u);
        }
    }
#pragma unroll
    for (int u = 0; u < NS - 1; u++)                                    // the last groups are already on their way (stage u = group j + u)
        if (j + u < j1) mm(u);
    if (wv > 0) {
#pragma unroll
        for (int tm = 0; tm < TM; tm++)
#pragma unroll
            for (int tn = 0; tn < TN; tn++)
#pragma unroll
                for (int r = 0; r < 4; r++) red[wv - 1][tm][tn][r][lane] = acc[tm][tn][r];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t s = tile0 + tm * 16 + 4 * q + r;
#pragma unroll
                for (int tn = 0; tn < TN; tn++) {
                    const float v = acc[tm][tn][r] + red[0][tm][tn][r][lane] + red[1][tm][tn][r][lane] + red[2][tm][tn][r][lane];
                    if (s < n) out[s * F + tn * 16 + c16] = selu(v);
                }
            }
        }
    }
}


// ---- conv2 / conv3 of the indel models as an implicit GEMM on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, bit-for-bit an
// fmaf chain): M = output positions (one tile of 16 per wave iteration), N = CO, K = 6*CI (tap-major) walked in groups of
// 16.  A lane's float4 = 4 consecutive input channels of one tap and feeds 4 MFMA steps: K slot kq of step j is
// k = 16 G + 4 kq + j, for the activation and the weight operand alike.  The weights of the layer live in LDS in fragment
// order (one ds_read_b128 per 4 MFMAs).  in NHWC [site][HI][WI][CI], weights [2][3][CI][CO], out NHWC [site][HO][WO][CO].
template <int HI, int WI, int CI, int CO>
__global__ __launch_bounds__(256) void k7_conv23_mfma(const float *__restrict__ in, const float *__restrict__ wk, const float *__restrict__ wb,
                                                      float *__restrict__ out, int64_t npos)
{
    constexpr int HO = HI - 1, WO = (WI - 3) / 2 + 1, K = 6 * CI, NG = K / 16, TN = CO / 16;
    static_assert(CI % 4 == 0 && K % 16 == 0 && CO % 16 == 0, "k7_conv23_mfma: shape");
    __shared__ float4 wf[NG][TN][64];
    for (int idx = threadIdx.x; idx < NG * TN * 64; idx += 256) {
        const int l = idx & 63, tn = (idx >> 6) % TN, G = (idx >> 6) / TN;
        const int k0 = 16 * G + 4 * (l >> 4), col = tn * 16 + (l & 15);
        wf[G][tn][l] = make_float4(wk[(k0 + 0) * CO + col], wk[(k0 + 1) * CO + col], wk[(k0 + 2) * CO + col], wk[(k0 + 3) * CO + col]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kq = lane >> 4, c16 = lane & 15;
    const int64_t ntiles = (npos + 15) / 16;
    float bias[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) bias[tn] = wb[tn * 16 + c16];
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        int64_t m = tile * 16 + c16;
        if (m >= npos) m = npos - 1;
        const int64_t site = m / (HO * WO);
        const int r = (int)(m - site * (HO * WO));
        const int y = r / WO, xq = r - y * WO;
        const float *ip = in + ((site * HI + y) * WI + 2 * xq) * CI;
        f32x4v acc[TN];
#pragma unroll
        for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4v){bias[tn], bias[tn], bias[tn], bias[tn]};
#pragma unroll
        for (int G = 0; G < NG; G++) {
            const int k0 = 16 * G + 4 * kq, tap = k0 / CI, ci = k0 - tap * CI;
            const float4 a = *reinterpret_cast<const float4 *>(ip + ((tap / 3) * WI + (tap % 3)) * CI + ci);
#pragma unroll
            for (int tn = 0; tn < TN; tn++) {
                const float4 b = wf[G][tn][lane];
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[tn], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int64_t pos = tile * 16 + 4 * kq + rr;             // D[row 4 kq + rr = position][col c16 = channel]
            if (pos < npos) {
#pragma unroll
                for (int tn = 0; tn < TN; tn++) out[pos * CO + tn * 16 + c16] = selu(acc[tn][rr]);
            }
        }
    }
}

// ---- fused conv1 + conv2 for the SNP trunk (5x41x5 input): the 205x48 conv1 activation lives only in LDS.
// Per site: (1) the input is staged, coverage-scaled, into a zero-padded [9][45][5] LDS image; (2) conv1 runs as
// v_mfma_f32_16x16x4 over 13 tiles of 16 positions: K is laid out as 5 input rows x 28 (25 real (dx,ci) values, which
// are CONTIGUOUS in the NHWC image, + 3 zero-weight slots) = 35 steps for the 5x5 kernel; the 1x5 kernel reuses the
// A fragments of row dy=2 (7 more MFMAs), the 5x1 kernel those of steps ls=2,3 of every row (10 more MFMAs, zero
// weights outside dx=2): 52 MFMAs per tile, 35 ds_read_b32; (3) conv2 (2x3, stride (1,2)) reads its A fragments from
// the LDS activation with one ds_read_b128 per 4 MFMAs.  Weight (B) fragments are pre-packed in fragment order
// (one coalesced 256-B read per MFMA).  lane l: A[row l&15][k l>>4], B[k l>>4][col l&15], C/D col l&15, row 4*(l>>4)+r.
constexpr int F12_XP = 2032;             // padded input image (9*45*5 = 2025, +7 so zero-weight slots stay in range)
constexpr int F12_CP = 52;               // channel pitch of the LDS activation (48 + 4: keeps ds_read_b128 aligned, spreads banks)
constexpr int F12_W1P = 52 * 64;         // conv1 B fragments
constexpr int F12_W2P = 6 * 3 * 4 * 2 * 64;
constexpr int F12_W3P = 48 * 4 * 64;      // conv3 B fragments: [step 48][tn 4][lane 64]
constexpr int F12_CP2 = 36;               // channel pitch of the LDS conv2 activation (32 + 4)
constexpr int F12_PACKED = F12_W1P + 48 + F12_W2P + 32 + F12_W3P + 64;

template <int NT>
__device__ __forceinline__ void f12_conv1_pass(const float *Xp, float *A1, const float (&w1r)[52], const float *__restrict__ b1,
                                               int tile_first, int lane)
{
    const int kq = lane >> 4, c16 = lane & 15;
    int rowbase[NT];
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
        int p = (tile_first + 4 * tm) * 16 + c16;
        p = p < 205 ? p : 204;
        const int h = p / 41, w = p - h * 41;
        rowbase[tm] = (h * 45 + w) * 5 + kq;
    }
    f32x4v acc1[NT], acc2[NT], acc3[NT];
    {
        const float x1 = b1[c16], x2 = b1[16 + c16], x3 = b1[32 + c16];
#pragma unroll
        for (int tm = 0; tm < NT; tm++) {
            acc1[tm] = (f32x4v){x1, x1, x1, x1};
            acc2[tm] = (f32x4v){x2, x2, x2, x2};
            acc3[tm] = (f32x4v){x3, x3, x3, x3};
        }
    }
#pragma unroll
    for (int s = 0; s < 35; s++) {
        const int dy = s / 7, ls = s % 7;
        float a[NT];
#pragma unroll
        for (int tm = 0; tm < NT; tm++) a[tm] = Xp[rowbase[tm] + dy * 225 + 4 * ls];
#pragma unroll
        for (int tm = 0; tm < NT; tm++) acc3[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tm], w1r[s], acc3[tm], 0, 0, 0);
        if (dy == 2) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++) acc1[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tm], w1r[35 + ls], acc1[tm], 0, 0, 0);
        }
        if (ls == 2 || ls == 3) {
#pragma unroll
            for (int tm = 0; tm < NT; tm++)
                acc2[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tm], w1r[42 + dy * 2 + (ls - 2)], acc2[tm], 0, 0, 0);
        }
    }
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int pos = (tile_first + 4 * tm) * 16 + 4 * kq + r;
            if (pos < 205) {
                float *o = A1 + pos * F12_CP + c16;
                o[0] = selu(acc1[tm][r]);
                o[16] = selu(acc2[tm][r]);
                o[32] = selu(acc3[tm][r]);
            }
        }
    }
}

template <int NT>
__device__ __forceinline__ void f12_conv2(const float *A1, const float (&w2r)[72], const float *__restrict__ b2,
                                          float *A2, int wv, int lane)
{
    const int kq = lane >> 4, c16 = lane & 15, tn = wv & 1, t0 = wv >> 1;
    int abase[NT];
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
        const int p = (t0 + 2 * tm) * 16 + c16;          // < 80
        const int y = p / 20, x = p - y * 20;
        abase[tm] = (y * 41 + 2 * x) * F12_CP + 4 * kq;
    }
    f32x4v acc[NT];
    {
        const float b = b2[tn * 16 + c16];
#pragma unroll
        for (int tm = 0; tm < NT; tm++) acc[tm] = (f32x4v){b, b, b, b};
    }
#pragma unroll
    for (int tap = 0; tap < 6; tap++) {
        const int toff = ((tap / 3) * 41 + (tap % 3)) * F12_CP;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float4 a[NT];
#pragma unroll
            for (int tm = 0; tm < NT; tm++) a[tm] = *reinterpret_cast<const float4 *>(A1 + abase[tm] + toff + 16 * j);
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int tm = 0; tm < NT; tm++) {
                    const float av = i == 0 ? a[tm].x : i == 1 ? a[tm].y : i == 2 ? a[tm].z : a[tm].w;
                    acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w2r[(tap * 3 + j) * 4 + i], acc[tm], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int tm = 0; tm < NT; tm++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int po = (t0 + 2 * tm) * 16 + 4 * kq + r;
            A2[po * F12_CP2 + tn * 16 + c16] = selu(acc[tm][r]);
        }
    }
}

// conv3 (2x3, stride (1,2): 4x20x32 -> 3x9x64) out of the LDS conv2 activation: 27 positions = 2 tiles of 16, wave w
// owns output channels [16w, 16w+16); its 48 weight fragments are streamed from L2 (the register file is full).
__device__ __forceinline__ void f12_conv3(const float *A2, const float *__restrict__ w3p, const float *__restrict__ b3,
                                          float *__restrict__ out_site, int wv, int lane)
{
    const int kq = lane >> 4, c16 = lane & 15;
    int abase[2];
#pragma unroll
    for (int tm = 0; tm < 2; tm++) {
        int p = tm * 16 + c16;
        p = p < 27 ? p : 26;
        const int y = p / 9, x = p - y * 9;
        abase[tm] = (y * 20 + 2 * x) * F12_CP2 + 4 * kq;
    }
    f32x4v acc[2];
    {
        const float b = b3[wv * 16 + c16];
        acc[0] = (f32x4v){b, b, b, b};
        acc[1] = acc[0];
    }
    const float *wl = w3p + wv * 64 + lane;
#pragma unroll 1
    for (int tap = 0; tap < 6; tap++) {
        const int toff = ((tap / 3) * 20 + (tap % 3)) * F12_CP2;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            float4 a[2];
#pragma unroll
            for (int tm = 0; tm < 2; tm++) a[tm] = *reinterpret_cast<const float4 *>(A2 + abase[tm] + toff + 16 * j);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float b = wl[((tap * 2 + j) * 4 + i) * 256];
#pragma unroll
                for (int tm = 0; tm < 2; tm++) {
                    const float av = i == 0 ? a[tm].x : i == 1 ? a[tm].y : i == 2 ? a[tm].z : a[tm].w;
                    acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[tm], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int tm = 0; tm < 2; tm++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int po = tm * 16 + 4 * kq + r;
            if (po < 27) out_site[po * 64 + wv * 16 + c16] = selu(acc[tm][r]);
        }
    }
}

// Weight-stationary and persistent: every wave loads its 52 conv1 and 72 conv2 weight fragments into registers ONCE
// (124 VGPRs) and then walks sites; in steady state the only memory traffic is the 4.1 KB input tensor in, the 10 KB
// conv2 activation out, and LDS.  Two workgroups (8 waves) per CU.
__global__ __launch_bounds__(256, 2) void k4_conv12(const float *__restrict__ x, const float *__restrict__ wp, float *__restrict__ a3,
                                                    int64_t n_sites, const double *__restrict__ scale, int scale_mode, int64_t site0)
{
    __shared__ __attribute__((aligned(16))) float Xp[F12_XP];
    __shared__ __attribute__((aligned(16))) float A1[205 * F12_CP];
    __shared__ __attribute__((aligned(16))) float A2[80 * F12_CP2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *w1p = wp, *b1 = wp + F12_W1P, *w2p = b1 + 48, *b2 = w2p + F12_W2P, *w3p = b2 + 32, *b3 = w3p + F12_W3P;
    float w1r[52], w2r[72];
#pragma unroll
    for (int s = 0; s < 52; s++) w1r[s] = w1p[s * 64 + lane];
#pragma unroll
    for (int s = 0; s < 72; s++) w2r[s] = w2p[(s * 2 + (wv & 1)) * 64 + lane];
    for (int i = threadIdx.x; i < F12_XP; i += 256) Xp[i] = 0.0f;
    __syncthreads();
    // staging is split: the global loads of the NEXT site are issued at the top of an iteration (5 values per thread,
    // held in registers while conv1 runs) and written, scaled, into the padded LDS image once conv1 has released it
    float pre[5];
    float pre_sf = 1.0f;
    double pre_sd = 1.0;
    auto prefetch = [&](int64_t site) {
        const float *xs = x + site * NC_SNP_TENSOR;
#pragma unroll
        for (int u = 0; u < 5; u++) {
            const int i = threadIdx.x + u * 256;
            pre[u] = i < NC_SNP_TENSOR ? xs[i] : 0.0f;
        }
        if (scale) { pre_sd = scale[site0 + site]; pre_sf = (float)pre_sd; }
    };
    auto commit = [&]() {
#pragma unroll
        for (int u = 0; u < 5; u++) {
            const int i = threadIdx.x + u * 256;
            if (i < NC_SNP_TENSOR) {
                const int h = i / 205, rem = i - h * 205, w = rem / 5, c = rem - w * 5;
                float v = pre[u];
                if (scale && h > 0 && c < 4) v = scale_mode == 0 ? v * pre_sf : (float)((double)v * pre_sd);    // snpCaller.py:93-96
                Xp[((h + 2) * 45 + (w + 2)) * 5 + c] = v;
            }
        }
    };
    int64_t site = blockIdx.x;
    if (site < n_sites) { prefetch(site); commit(); }
    __syncthreads();
    for (; site < n_sites; site += gridDim.x) {
        const int64_t nxt = site + gridDim.x;
        if (nxt < n_sites) prefetch(nxt);
        // conv1: 13 tiles of 16 positions; wave w owns tiles w, w+4, w+8 (and 12 for wave 0)
        f12_conv1_pass<2>(Xp, A1, w1r, b1, wv, lane);
        if (wv == 0) f12_conv1_pass<2>(Xp, A1, w1r, b1, 8, lane);
        else f12_conv1_pass<1>(Xp, A1, w1r, b1, 8 + wv, lane);
        __syncthreads();
        // the padded input is free again: write the next site's image while conv2 runs out of A1
        if (nxt < n_sites) commit();
        if (wv < 2) f12_conv2<3>(A1, w2r, b2, A2, wv, lane);
        else f12_conv2<2>(A1, w2r, b2, A2, wv, lane);
        __syncthreads();
        // conv3 reads A2; the next iteration's conv1 only touches Xp / A1, and A2 is not rewritten before the barrier
        // that follows that conv1, so no third barrier is needed
        f12_conv3(A2, w3p, b3, a3 + site * (27 * 64), wv, lane);
    }
}

template <int H>
void launch_indel_convs(hipStream_t st, const float *x, const float *w, float *a1, float *a2, float *a3, int64_t nb)
{
    constexpr int W = 128, CI = 2, C1 = 8, C2 = 32, C3 = 48, H2 = H - 1, W2 = (W - 3) / 2 + 1, H3 = H2 - 1, W3 = (W2 - 3) / 2 + 1;
    const float *k2 = w + (5 + 5 + 25) * CI * C1 + 3 * C1, *b2 = k2 + 2 * 3 * 3 * C1 * C2, *k3 = b2 + C2, *b3 = k3 + 2 * 3 * C2 * C3;
    const int64_t np1 = nb * H * W, np2 = nb * H2 * W2, np3 = nb * H3 * W3;
    auto grid = [](int64_t npos) { const int64_t t = (npos + 63) / 64; return dim3((unsigned)(t < 2048 ? t : 2048)); };
    hipLaunchKernelGGL((k2_conv1_x4<H, W, C1>), dim3(blocks_for(np1 / 4)), dim3(256), 0, st, x, w, a1, np1);
    hipLaunchKernelGGL((k7_conv23_mfma<H, W, 3 * C1, C2>), grid(np2), dim3(256), 0, st, a1, k2, b2, a2, np2);
    hipLaunchKernelGGL((k7_conv23_mfma<H2, W2, C2, C3>), grid(np3), dim3(256), 0, st, a2, k3, b3, a3, np3);
}

}   // namespace

void nc_cnn_launch_indel_convs_fp32(hipStream_t st, int H, const float *x, const float *w, float *a1, float *a2, float *a3, int64_t nb)
{
    if (H == 15) launch_indel_convs<15>(st, x, w, a1, a2, a3, nb);
    else launch_indel_convs<5>(st, x, w, a1, a2, a3, nb);
}

void nc_cnn_launch_fc1_fp32(hipStream_t st, int F, const float *a3, int K, const float *kf, const float *bf, float *f1, int64_t nb)
{
    if (F == 48) hipLaunchKernelGGL((k3_fc1<48, 1>), dim3(blocks_for(nb, 16)), dim3(256), 0, st, a3, K, kf, bf, f1, nb);
    else hipLaunchKernelGGL((k3_fc1<32, 2>), dim3(blocks_for(nb, 32)), dim3(256), 0, st, a3, K, kf, bf, f1, nb);
}

void nc_cnn_launch_k4_conv12(const SnpTrunkArgs &a, const float *packed)
{
    const unsigned nblk = (unsigned)(a.nb < 512 ? a.nb : 512);          // 2 resident workgroups per CU, persistent over sites
    hipExtLaunchKernelGGL(k4_conv12, dim3(nblk), dim3(256), 0, a.stream, a.ev0, a.ev1, 0, a.x_f32, packed, a.a3, a.nb, a.scale, a.scale_mode, a.site0);
}

// B fragments of k4_conv12 in (step, lane) order: [conv1 F12_W1P][b1 48][conv2 F12_W2P][b2 32][conv3 F12_W3P][b3 64]
std::vector<float> nc_cnn_pack_k4(const float *blob)
{
    std::vector<float> pk((size_t)F12_PACKED, 0.0f);
    const float *k11 = blob, *b11 = k11 + 400, *k12 = b11 + 16, *b12 = k12 + 400, *k13 = b12 + 16, *b13 = k13 + 2000;
    const float *k2 = b13 + 16, *b2 = k2 + 2 * 3 * 48 * 32;
    float *w1p = pk.data(), *b1 = w1p + F12_W1P, *w2p = b1 + 48, *b2p = w2p + F12_W2P, *w3p = b2p + 32, *b3p = w3p + F12_W3P;
    const float *k3 = b2 + 32, *b3 = k3 + 2 * 3 * 32 * 64;
    for (int lane = 0; lane < 64; lane++) {
        const int kq = lane >> 4, c = lane & 15;
        for (int s = 0; s < 35; s++) {
            const int dy = s / 7, kl = 4 * (s % 7) + kq;
            if (kl < 25) w1p[s * 64 + lane] = k13[((dy * 5 + kl / 5) * 5 + kl % 5) * 16 + c];
        }
        for (int ls = 0; ls < 7; ls++) {
            const int kl = 4 * ls + kq;
            if (kl < 25) w1p[(35 + ls) * 64 + lane] = k11[kl * 16 + c];
        }
        for (int dy = 0; dy < 5; dy++)
            for (int t = 0; t < 2; t++) {
                const int kl = 4 * (2 + t) + kq;
                if (kl >= 10 && kl < 15) w1p[(42 + dy * 2 + t) * 64 + lane] = k12[(dy * 5 + (kl - 10)) * 16 + c];
            }
        for (int tap = 0; tap < 6; tap++)
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < 4; i++)
                    for (int tn = 0; tn < 2; tn++)
                        w2p[((((tap * 3 + j) * 4 + i) * 2) + tn) * 64 + lane] = k2[(tap * 48 + 16 * j + 4 * kq + i) * 32 + tn * 16 + c];
        for (int tap = 0; tap < 6; tap++)
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 4; i++)
                    for (int tn = 0; tn < 4; tn++)
                        w3p[(((tap * 2 + j) * 4 + i) * 4 + tn) * 64 + lane] = k3[(tap * 32 + 16 * j + 4 * kq + i) * 64 + tn * 16 + c];
    }
    for (int c = 0; c < 16; c++) { b1[c] = b11[c]; b1[16 + c] = b12[c]; b1[32 + c] = b13[c]; }
    for (int c = 0; c < 32; c++) b2p[c] = b2[c];
    for (int c = 0; c < 64; c++) b3p[c] = b3[c];
    return pk;
}

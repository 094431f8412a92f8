// What the two indel training units share (nc_train_indel.hip: the diploid model, [15][128][2] -> 4 classes; nc_train_hap_indel.hip: the haploid
// model, [5][128][2] -> 1 logit): every kernel but k_heads, templated on the blob B = indel_blob<rows, outputs>, and the host side of a handle.
// The two networks have the same layers (conv1 as 1x5 | 5x1 | 5x5 to 24 channels, conv2 to 32, conv3 to 48, fc1 to 32, fc2 to 24, fc3); the
// row count sets the flattened size NF (19,344 / 4,464) and with it every offset behind fc1's kernel.  DESIGN.md sections 18 and 19.
//
// Sums over sites run in a fixed order.  fc1's kernel has no slabs: one workgroup owns 16 U::FCW_J of its rows and walks all sites of the slice,
// a contiguous quarter per wave, combined through LDS in wave order and added to the earlier slices' sum.  The other parameters go through
// slabs of SLAB = 16 consecutive sites, which k_params adds in slab order.  No atomics.  Sites past n are never read.
// lane l of an MFMA: A[row l&15][k l>>4], B[k l>>4][col l&15], C/D col l&15, row 4*(l>>4)+r (the lane maps of nc_cnn_fp32.hip).
#pragma once
#include "nc_train.h"

namespace {

constexpr int SLAB = 16;                                   // sites per slab of the small parameters: four per wave
constexpr int64_t DEFAULT_SLICE = 1024;                    // sites whose activations the workspace holds at once
constexpr int W = 128, F1 = 32, F2 = 24;
// canonical blob offsets of the convolutions (weights.LAYER_SPECS[KIND_INDEL], [KIND_INDEL_HAP]: kernel then bias of every layer)
constexpr int O_K11 = 0, O_B11 = 80, O_K12 = 88, O_B12 = 168, O_K13 = 176, O_B13 = 576, O_K2 = 584, O_B2 = 5192, O_K3 = 5224, O_B3 = 14440;
constexpr int O_KF = 14488;

template <int ROWS, int NOUT>
struct indel_blob {
    static constexpr int H = ROWS, NC = NOUT, XT = H * W * 2;                                     // the input tensor
    static constexpr int N1 = H * W * 24, P2 = (H - 1) * 63, N2 = P2 * 32, P3 = (H - 2) * 31, NF = P3 * 48;   // floats per site: conv1 - conv3 outputs
    static constexpr int O_BF = O_KF + NF * F1, O_FC2 = O_BF + F1, O_FC2B = O_FC2 + F1 * F2, O_FC3 = O_FC2B + F2, O_FC3B = O_FC3 + F2 * NC;
    static constexpr int NPAR = O_FC3B + NC;
    static constexpr int NFK = O_BF - O_KF;                // fc1's kernel, kept out of the slabs
    static constexpr int NSM = NPAR - NFK;                 // floats per slab: blob index i -> i below fc1's kernel, i - NFK behind it
    // per-site record of the layers behind fc1: activations [f1 masked 32 | fc2 24], gradients at the pre-activations [fc2 24 | logits NC]
    static constexpr int TA = 56, TA_FC2 = 32, TD = F2 + NC, TD_Z = F2;
    static constexpr int NSMALL = F1 + NPAR - O_FC2;       // fc1's bias, fc2, fc3 with their biases
    __device__ static __forceinline__ bool is_bias(int i)
    {
        if (i < O_K2) return (i >= O_B11 && i < O_K12) || (i >= O_B12 && i < O_K13) || i >= O_B13;
        if (i < O_KF) return (i >= O_B2 && i < O_K3) || i >= O_B3;
        if (i < O_BF) return false;
        if (i < O_FC2) return true;
        if (i < O_FC3) return i >= O_FC2B;
        return i >= O_FC3B;
    }
};

// conv1 (1x5, 5x1, 5x5, same padding; 2 -> 8 channels each): k2_conv1_x4 of nc_cnn_fp32.hip, four x-adjacent output positions per thread,
// weights as wave-uniform operands, with the accurate exponential in the SELU.  out NHWC [site][H][128][24]
template <int H>
__global__ __launch_bounds__(256) void k_conv1_fwd(const float *__restrict__ x, const float *__restrict__ w, float *__restrict__ out, int64_t npos)
{
    constexpr int CI = 2, C1 = 8, XT = H * W * 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t * 4 >= npos) return;
    const int64_t g0 = t * 4, site = g0 / (H * W);
    const int r = (int)(g0 - site * (H * W));
    const int h = r / W, x0 = r - h * W;                                  // x0 % 4 == 0
    const float *xs = x + site * XT;
    const float *k11 = w + O_K11, *b11 = w + O_B11, *k12 = w + O_K12, *b12 = w + O_B12, *k13 = w + O_K13, *b13 = w + O_B13;
    float a1[4][C1], a2[4][C1], a3[4][C1];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int o = 0; o < C1; o++) { a1[p][o] = b11[o]; a2[p][o] = b12[o]; a3[p][o] = b13[o]; }
#pragma unroll 1
    for (int dy = -2; dy <= 2; dy++) {
        const int iy = h + dy;
        float win[16];                                                     // pixels x0 - 2 .. x0 + 5 of row iy, two channels each
        const bool row_in = iy >= 0 && iy < H;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int px = x0 - 2 + 2 * q;                                 // pixel pair (px, px + 1): both inside or both outside
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row_in && px >= 0 && px + 1 < W) v = *reinterpret_cast<const float4 *>(xs + (iy * W + px) * CI);
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
            op[o / 4] = make_float4(selu_acc(a1[p][o]), selu_acc(a1[p][o + 1]), selu_acc(a1[p][o + 2]), selu_acc(a1[p][o + 3]));
            op[(C1 + o) / 4] = make_float4(selu_acc(a2[p][o]), selu_acc(a2[p][o + 1]), selu_acc(a2[p][o + 2]), selu_acc(a2[p][o + 3]));
            op[(2 * C1 + o) / 4] = make_float4(selu_acc(a3[p][o]), selu_acc(a3[p][o + 1]), selu_acc(a3[p][o + 2]), selu_acc(a3[p][o + 3]));
        }
    }
}

// fc1 forward: k3_fc1's form (M = 16 sites, N = 32, split-K combined through LDS in wave order) with K = NF split over 16 waves: at 19,344 a
// wave's dependent chain is 76 groups of 16 instead of 302, and a batch of 256 sites still fills 256 waves.  It also writes SELU' of its 32
// units, taken from the pre-activation it holds (selud_pre).
constexpr int FW = 16;
template <int NF>
__global__ __launch_bounds__(64 * FW) void k_fc1_fwd(const float *__restrict__ in, const float *__restrict__ wk, const float *__restrict__ wb,
                                                     float *__restrict__ out, float *__restrict__ dout, int64_t n)
{
    constexpr int TN = 2, NG = NF / 16;
    static_assert(NF % 16 == 0, "k_fc1_fwd: shape");
    __shared__ float red[FW - 1][TN][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int64_t tile0 = (int64_t)blockIdx.x * 16;
    int64_t s = tile0 + c16;
    if (s >= n) s = n - 1;
    const float *ip = in + s * NF + 4 * q;
    const float *wl = wk + (4 * q) * F1 + c16;
    f32x4v acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const float b = wv == 0 ? wb[tn * 16 + c16] : 0.0f;
        acc[tn] = (f32x4v){b, b, b, b};
    }
    const int j0 = (NG * wv) / FW, j1 = (NG * (wv + 1)) / FW;
#pragma unroll 4
    for (int j = j0; j < j1; j++) {
        const float4 a = *reinterpret_cast<const float4 *>(ip + 16 * j);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float av = i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : a.w;
#pragma unroll
            for (int tn = 0; tn < TN; tn++) acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wl[(16 * j + i) * F1 + tn * 16], acc[tn], 0, 0, 0);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int tn = 0; tn < TN; tn++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wv - 1][tn][r][lane] = acc[tn][r];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t so = tile0 + 4 * q + r;
#pragma unroll
            for (int tn = 0; tn < TN; tn++) {
                float v = acc[tn][r];
                for (int k = 0; k < FW - 1; k++) v += red[k][tn][r][lane];
                if (so < n) {
                    out[so * F1 + tn * 16 + c16] = selu_acc(v);
                    dout[so * F1 + tn * 16 + c16] = selud_pre(v);
                }
            }
        }
    }
}

template <int NI, int NO>
__device__ __forceinline__ void dense(const float (&in)[NI], const float *__restrict__ k, const float *__restrict__ b, float (&out)[NO])
{
#pragma unroll
    for (int o = 0; o < NO; o++) out[o] = b[o];
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int o = 0; o < NO; o++) out[o] = fmaf(in[i], k[i * NO + o], out[o]);
}

// weight gradients of fc1's bias and of fc2, fc3 with their biases (924 / 849 parameters), one parameter per lane, the slab's sites in order
template <class B>
__global__ __launch_bounds__(256) void k_small_wgrad(const float *__restrict__ tact, const float *__restrict__ tdel, const float *__restrict__ df1,
                                                     int64_t n, float *__restrict__ slabs)
{
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= B::NSMALL) return;
    const int gi = t < F1 ? B::O_BF + t : B::O_FC2 + (t - F1);
    // in: -1 the constant 1 (bias), else an offset in the activation record; del: an offset in the gradient record, or -1 - o for d fc1
    int in = -1, del = 0;
    if (gi < B::O_FC2) del = -1 - t;
    else if (gi < B::O_FC2B) { in = (gi - B::O_FC2) / F2; del = (gi - B::O_FC2) % F2; }
    else if (gi < B::O_FC3) del = gi - B::O_FC2B;
    else if (gi < B::O_FC3B) { in = B::TA_FC2 + (gi - B::O_FC3) / B::NC; del = B::TD_Z + (gi - B::O_FC3) % B::NC; }
    else del = B::TD_Z + gi - B::O_FC3B;
    const int64_t s0 = (int64_t)blockIdx.x * SLAB, s1 = s0 + SLAB < n ? s0 + SLAB : n;
    float acc = 0.0f;
    for (int64_t s = s0; s < s1; s++) {
        const float d = del < 0 ? df1[s * F1 + (-1 - del)] : tdel[s * B::TD + del];
        const float a = in >= 0 ? tact[s * B::TA + in] : 1.0f;
        acc = fmaf(a, d, acc);
    }
    slabs[(int64_t)blockIdx.x * B::NSM + gi - B::NFK] = acc;
}

// fc1 weight gradient dW[k][o] = sum_s a3[s][k] d[s][o] over the slice: M = k, N = 32, K = sites, four per MFMA.  One workgroup per 16 J
// consecutive k: a lane loads k0 + J (l & 15) .. + J - 1 of one site in one load (J = 4: a dwordx4, a wave reads 256 contiguous bytes per
// site), so tile j of the J holds the rows k0 + J r + j.  Every activation is read once and nothing but the gradient itself is written: there
// are no slabs.  The four waves take a contiguous quarter of the slice's sites each, rounded up to a multiple of four, and combine through
// LDS in wave order; with `accum` the sum of the earlier slices is added last.  (NF + 16 J - 1) / (16 J) workgroups: 303 at 19,344 with
// J = 4; at 4,464 70 with J = 4, 140 with J = 2, 279 with J = 1 (the units choose: U::FCW_J).
template <int NF, int J>
__global__ __launch_bounds__(256) void k_fc1_wgrad(const float *__restrict__ a3, const float *__restrict__ df1, int64_t n, int accum, float *__restrict__ g)
{
    static_assert(NF % 4 == 0 && (J == 1 || J == 2 || J == 4), "k_fc1_wgrad: shape");
    __shared__ float red[3][J][2][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int k0 = blockIdx.x * (16 * J), kl = k0 + J * c16;
    const bool kin = kl < NF;                                           // NF % J == 0: a lane's J rows are inside together
    const int64_t quarter = ((n + 15) / 16) * 4, s_begin = wv * quarter, s_stop = s_begin + quarter < n ? s_begin + quarter : n;
    f32x4v acc[J][2];
#pragma unroll
    for (int j = 0; j < J; j++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) acc[j][tn] = (f32x4v){0, 0, 0, 0};
#pragma unroll 4
    for (int64_t s4 = s_begin; s4 < s_stop; s4 += 4) {
        const int64_t s = s4 + q;
        const bool ok = s < n;
        float a[J];
#pragma unroll
        for (int j = 0; j < J; j++) a[j] = 0.0f;
        if (ok && kin) {
            const float *ap = a3 + s * NF + kl;
            if constexpr (J == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(ap);
                a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
            } else if constexpr (J == 2) {
                const float2 v = *reinterpret_cast<const float2 *>(ap);
                a[0] = v.x; a[1] = v.y;
            } else {
                a[0] = *ap;
            }
        }
        const float b0 = ok ? df1[s * F1 + c16] : 0.0f, b1 = ok ? df1[s * F1 + 16 + c16] : 0.0f;
#pragma unroll
        for (int j = 0; j < J; j++) {
            acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b0, acc[j][0], 0, 0, 0);
            acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b1, acc[j][1], 0, 0, 0);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < J; j++)
#pragma unroll
            for (int tn = 0; tn < 2; tn++)
#pragma unroll
                for (int r = 0; r < 4; r++) red[wv - 1][j][tn][r][lane] = acc[j][tn][r];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int j = 0; j < J; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int k = k0 + J * (4 * q + r) + j;
                if (k < NF) {
#pragma unroll
                    for (int tn = 0; tn < 2; tn++) {
                        float v = ((acc[j][tn][r] + red[0][j][tn][r][lane]) + red[1][j][tn][r][lane]) + red[2][j][tn][r][lane];
                        float *o = g + O_KF + k * F1 + tn * 16 + c16;
                        if (accum) v += *o;
                        *o = v;
                    }
                }
            }
    }
}

// fc1 data gradient d3[s][k] = SELU'(a3[s][k]) sum_o W[k][o] d[s][o]: M = k (the weights as the A operand, so a lane's four results are four
// consecutive k of one site: one dwordx4 store), N = 16 sites, K = 32 in float4 pieces (slot q of step (j, i) is o = 16 j + 4 q + i).
// grid (16-site tiles, DG_Y): the NF / 16 k tiles are dealt to the 4 DG_Y waves of a tile's workgroups in turn.
constexpr int DG_Y = 16;
template <int NF>
__global__ __launch_bounds__(256) void k_fc1_dgrad(const float *__restrict__ wk, const float *__restrict__ df1, const float *__restrict__ a3, int64_t n,
                                                   float *__restrict__ d3)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int64_t s = (int64_t)blockIdx.x * 16 + c16, sc = s < n ? s : n - 1;
    float4 bd[2];
#pragma unroll
    for (int j = 0; j < 2; j++) bd[j] = *reinterpret_cast<const float4 *>(df1 + sc * F1 + 16 * j + 4 * q);
    for (int kt = blockIdx.y * 4 + wv; kt < NF / 16; kt += 4 * DG_Y) {
        f32x4v acc = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const float4 a = *reinterpret_cast<const float4 *>(wk + (kt * 16 + c16) * F1 + 16 * j + 4 * q);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bd[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bd[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bd[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bd[j].w, acc, 0, 0, 0);
        }
        if (s < n) {
            const int64_t o = s * NF + kt * 16 + 4 * q;
            const float4 y = *reinterpret_cast<const float4 *>(a3 + o);
            *reinterpret_cast<float4 *>(d3 + o) = make_float4(acc[0] * selud(y.x), acc[1] * selud(y.y), acc[2] * selud(y.z), acc[3] * selud(y.w));
        }
    }
}

// conv1's three kernels and their biases of one slab, as one cross-correlation of the 5x5 window with all 24 channels: M = (tap, ci) rows of
// the 5x5 window, 50 of them, row 50 the constant 1 (the biases), N = the 24 channels in two tiles, K = output positions, four per MFMA; a tap
// outside the image enters as zero.  The 1x5 kernel (channels 0..7) is the window's middle row, the 5x1 kernel (8..15) its middle column, the
// 5x5 kernel (16..23) all of it; the other products are computed and dropped.  grid (slabs, 4 M tiles); a workgroup's 16 waves take one site of
// the slab each (H * 32 dependent steps per wave) and combine through LDS in wave order.  NSM: the slab stride.
constexpr int C1W = SLAB;
template <int H, int NSM>
__global__ __launch_bounds__(64 * C1W) void k_conv1_wgrad(const float *__restrict__ x, const float *__restrict__ d1, int64_t n, float *__restrict__ slabs)
{
    __shared__ float red[C1W - 1][2][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int ma = blockIdx.y * 16 + c16, tapa = ma / 2;                // this lane's A row
    const int kind = ma < 50 ? 0 : ma == 50 ? 1 : 2;                    // 0: a tap, 1: the bias row, 2: padding
    const int dyo = tapa / 5 - 2, dxo = tapa % 5 - 2, off = (dyo * W + dxo) * 2 + (ma & 1);
    const bool bin = 16 + c16 < 24;
    const int64_t p0 = ((int64_t)blockIdx.x * SLAB + wv) * (H * W), pend = n * (H * W);
    f32x4v acc[2] = {(f32x4v){0, 0, 0, 0}, (f32x4v){0, 0, 0, 0}};
#pragma unroll 8
    for (int st = 0; st < (H * W) / 4; st++) {
        const int64_t p = p0 + 4 * st + q;
        const bool ok = p < pend;
        const int r = (int)(p % (H * W)), h = r / W, wx = r - h * W;
        const int iy = h + dyo, ix = wx + dxo;
        float a = 0.0f;
        if (ok && kind == 1) a = 1.0f;
        if (ok && kind == 0 && iy >= 0 && iy < H && ix >= 0 && ix < W) a = x[p * 2 + off];
        const float b0 = ok ? d1[p * 24 + c16] : 0.0f, b1 = ok && bin ? d1[p * 24 + 16 + c16] : 0.0f;
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[1], 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int tn = 0; tn < 2; tn++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wv - 1][tn][r][lane] = acc[tn][r];
    }
    __syncthreads();
    if (wv == 0) {
        float *out = slabs + (int64_t)blockIdx.x * NSM;
#pragma unroll
        for (int tn = 0; tn < 2; tn++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = blockIdx.y * 16 + 4 * q + r, ch = tn * 16 + c16, tap = m / 2, ci = m & 1, o = ch & 7;
                float v = acc[tn][r];
                for (int k = 0; k < C1W - 1; k++) v += red[k][tn][r][lane];
                if (m > 50 || ch >= 24) continue;
                if (ch < 8) {                                           // 1x5: the window's row dy = 2
                    if (m == 50) out[O_B11 + o] = v;
                    else if (tap / 5 == 2) out[O_K11 + ((tap % 5) * 2 + ci) * 8 + o] = v;
                } else if (ch < 16) {                                   // 5x1: the window's column dx = 2
                    if (m == 50) out[O_B12 + o] = v;
                    else if (tap % 5 == 2) out[O_K12 + ((tap / 5) * 2 + ci) * 8 + o] = v;
                } else {
                    if (m == 50) out[O_B13 + o] = v;
                    else out[O_K13 + m * 8 + o] = v;
                }
            }
    }
}

// sum over kernel entries of w^2, in WSQ_BLOCKS contiguous pieces: strided partial sums combined by a fixed tree -> part[blockIdx.x]
constexpr int WSQ_BLOCKS = 64;
template <class B>
__global__ __launch_bounds__(256) void k_wsq(const float *__restrict__ w, double *__restrict__ part)
{
    constexpr int WSQ_PIECE = (B::NPAR + WSQ_BLOCKS - 1) / WSQ_BLOCKS;
    __shared__ double red[256];
    const int i0 = blockIdx.x * WSQ_PIECE, i1 = i0 + WSQ_PIECE < B::NPAR ? i0 + WSQ_PIECE : B::NPAR;
    double ww = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256)
        if (!B::is_bias(i)) ww += (double)w[i] * (double)w[i];
    red[threadIdx.x] = ww;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// the two loss terms [cost, CE]: the batch mean of the per-site cross-entropies and gamma * sum over kernel entries of w^2 / 2 (k_wsq's
// pieces); one workgroup, strided partial sums combined by a fixed tree
__global__ __launch_bounds__(1024) void k_loss_reduce(const float *__restrict__ loss, int64_t n, const double *__restrict__ wsq, float gamma, float *__restrict__ out2)
{
    __shared__ double red[2][1024];
    double ce = 0.0;
    for (int64_t s = threadIdx.x; s < n; s += 1024) ce += (double)loss[s];
    const double ww = threadIdx.x < WSQ_BLOCKS ? wsq[threadIdx.x] : 0.0;
    red[0][threadIdx.x] = ce;
    red[1][threadIdx.x] = ww;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if (threadIdx.x < k) {
            red[0][threadIdx.x] += red[0][threadIdx.x + k];
            red[1][threadIdx.x] += red[1][threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double c = red[0][0] / (double)n;
        out2[0] = (float)(c + 0.5 * (double)gamma * red[1][0]);
        out2[1] = (float)c;
    }
}

// One parameter per lane, k_params of nc_train.hip with these units' two kinds of sum: an entry of fc1's kernel takes its gradient from gacc
// (k_fc1_wgrad has summed it), every other one gacc (earlier slices, with `partial`) + the slabs in slab order; + gamma w on kernel entries
// with `reg`; written to g_out (may be NULL); with `step` the Adam update in TensorFlow's form, w -= lr_t m / (sqrt(v) + eps).
template <class B>
__global__ __launch_bounds__(256) void k_params(const float *__restrict__ gacc, int partial, const float *__restrict__ slabs, int ns, int reg, float gamma,
                                                float *__restrict__ g_out, int step, float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                float lr_t, float b1, float b2, float eps)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B::NPAR) return;
    const bool fk = i >= O_KF && i < B::O_BF;
    float g = fk || partial ? gacc[i] : 0.0f;
    if (!fk) {
        const int si = i < O_KF ? i : i - B::NFK;
        for (int k = 0; k < ns; k++) g += slabs[(int64_t)k * B::NSM + si];
    }
    const float wi = w[i];
    if (reg && !B::is_bias(i)) g = fmaf(gamma, wi, g);
    if (g_out) g_out[i] = g;
    if (step) {
        const float mi = fmaf(b1, m[i], (1.0f - b1) * g), vi = fmaf(b2, v[i], (1.0f - b2) * g * g);
        m[i] = mi;
        v[i] = vi;
        w[i] = wi - lr_t * mi / (sqrtf(vi) + eps);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host side of a handle
struct indel_train_state : train_state {
    float *a1, *a2, *a3, *f1, *f1d, *tact, *tdel, *df1, *d1, *d2, *d3, *slabs, *loss, *loss2, *wsq;   // loss2: cost, CE, the bad-label flag
};

inline dim3 tile_grid(int64_t npos)
{
    const int64_t t = (npos + 63) / 64;
    return dim3((unsigned)(t < 2048 ? t : 2048));
}

// A unit U names its blob (U::B), its entry points' prefix (U::NAME), the model it accepts (U::KIND, U::MODEL), what a label outside the classes
// is called where one is looked for on the device (U::BAD_LABELS, else null: the flag in loss2[2] that U::heads sets; the call then always
// waits), how many 16-row tiles of fc1's weight gradient a workgroup owns (U::FCW_J) and launches its k_heads:
//   static void heads(indel_train_state *, hipStream_t, int64_t nb, const uint8_t *mask, float inv_keep, const uint8_t *label, float inv_n,
//                     float *probs, float *loss)
template <class U>
struct indel_train {
    using B = typename U::B;

    // conv1 - fc1 of `nb` sites (a slice) into the workspace
    static void forward_trunk(indel_train_state *tr, int64_t nb, const float *x)
    {
        hipStream_t st = tr->ctx->stream;
        hipLaunchKernelGGL(k_conv1_fwd<B::H>, dim3(blocks_for(nb * (B::H * W) / 4)), dim3(256), 0, st, x, tr->w, tr->a1, nb * (B::H * W));
        hipLaunchKernelGGL((k_conv23_fwd<B::H, W, 24, 32>), tile_grid(nb * B::P2), dim3(256), 0, st, tr->a1, tr->w + O_K2, tr->w + O_B2, tr->a2, nb * B::P2);
        hipLaunchKernelGGL((k_conv23_fwd<B::H - 1, 63, 32, 48>), tile_grid(nb * B::P3), dim3(256), 0, st, tr->a2, tr->w + O_K3, tr->w + O_B3, tr->a3, nb * B::P3);
        hipLaunchKernelGGL(k_fc1_fwd<B::NF>, dim3(blocks_for(nb, 16)), dim3(64 * FW), 0, st, tr->a3, tr->w + O_KF, tr->w + B::O_BF, tr->f1, tr->f1d, nb);
    }

    template <class H>
    static int create(nc_ctx *ctx, int32_t kind, int64_t max_batch, int64_t slice_sites, H **out)
    {
        if (!ctx || !out) return NC_ERR_ARG;
        *out = nullptr;
        if (kind != U::KIND)
            return nc_fail(ctx, NC_ERR_UNSUPPORTED, "%s_create: only the %s model (kind %d) is trained here, not kind %d", U::NAME, U::MODEL, U::KIND, kind);
        if (max_batch < 1 || slice_sites < 0) return nc_fail(ctx, NC_ERR_ARG, "%s_create: max_batch / slice_sites", U::NAME);
        return train_create(ctx, max_batch, out, [slice_sites](indel_train_state *tr) {
            tr->slice = slice_sites > 0 ? slice_sites : DEFAULT_SLICE;
            if (tr->slice > tr->max_batch) tr->slice = tr->max_batch;
            const size_t sl = (size_t)tr->slice, ns = (sl + SLAB - 1) / SLAB;
            const size_t sizes[] = {sl * B::N1, sl * B::N2, sl * B::NF, sl * F1, sl * F1, sl * B::TA, sl * B::TD, sl * F1, sl * B::N1, sl * B::N2, sl * B::NF,
                                    ns * B::NSM, (size_t)tr->max_batch, 8, 2 * WSQ_BLOCKS};
            float **const ptrs[] = {&tr->a1, &tr->a2, &tr->a3, &tr->f1, &tr->f1d, &tr->tact, &tr->tdel, &tr->df1, &tr->d1, &tr->d2, &tr->d3, &tr->slabs, &tr->loss,
                                    &tr->loss2, &tr->wsq};
            return train_alloc(tr, U::NAME, B::NPAR, sizes, ptrs);
        });
    }

    static int forward(indel_train_state *tr, int64_t n, const float *x_dev, const uint8_t *keep_mask_dev, float keep, float *probs_dev)
    {
        NC_TRY(train_check_call(tr, U::NAME, "forward", n, x_dev && probs_dev, keep));
        nc_ctx *ctx = tr->ctx;
        NC_HIP(ctx, hipSetDevice(ctx->device));
        if (keep == 1.0f) keep_mask_dev = nullptr;
        for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
            const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
            forward_trunk(tr, nb, x_dev + s0 * B::XT);
            U::heads(tr, ctx->stream, nb, keep_mask_dev ? keep_mask_dev + s0 * F1 : nullptr, 1.0f / keep, nullptr, 0.0f, probs_dev + s0 * B::NC, tr->loss);
        }
        NC_HIP(ctx, hipGetLastError());
        return NC_OK;
    }

    static int loss_grad(indel_train_state *tr, int64_t n, const float *x_dev, const uint8_t *keep_mask_dev, float keep, const uint8_t *label_dev, float gamma,
                         float *loss2_host, float *grad_dev)
    {
        NC_TRY(train_check_call(tr, U::NAME, "loss_grad", n, x_dev && label_dev, keep));
        nc_ctx *ctx = tr->ctx;
        NC_HIP(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        if (keep == 1.0f) keep_mask_dev = nullptr;
        tr->have_grad = tr->partial = false;
        if (U::BAD_LABELS) NC_HIP(ctx, hipMemsetAsync(tr->loss2, 0, 8 * 4, st));
        for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
            const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
            const unsigned ns = (unsigned)((nb + SLAB - 1) / SLAB);
            const float *x = x_dev + s0 * B::XT;
            train_mark(tr, TS_FWD);
            forward_trunk(tr, nb, x);
            train_mark(tr, TS_HEADS);
            U::heads(tr, st, nb, keep_mask_dev ? keep_mask_dev + s0 * F1 : nullptr, 1.0f / keep, label_dev + s0, 1.0f / (float)n, nullptr, tr->loss + s0);
            hipLaunchKernelGGL(k_small_wgrad<B>, dim3(ns, blocks_for(B::NSMALL)), dim3(256), 0, st, tr->tact, tr->tdel, tr->df1, nb, tr->slabs);
            train_mark(tr, TS_FC1);
            hipLaunchKernelGGL((k_fc1_wgrad<B::NF, U::FCW_J>), dim3((B::NF + 16 * U::FCW_J - 1) / (16 * U::FCW_J)), dim3(256), 0, st, tr->a3, tr->df1, nb, s0 > 0 ? 1 : 0, tr->g);
            hipLaunchKernelGGL(k_fc1_dgrad<B::NF>, dim3(blocks_for(nb, 16), DG_Y), dim3(256), 0, st, tr->w + O_KF, tr->df1, tr->a3, nb, tr->d3);
            train_mark(tr, TS_CONV3);
            hipLaunchKernelGGL((k_conv_wgrad<B::H - 1, 63, 32, 48, 2, SLAB, B::NSM>), dim3(ns, 6), dim3(256), 0, st, tr->a2, tr->d3, nb, (int)O_K3, tr->slabs);
            hipLaunchKernelGGL((k_bias_grad<48, B::P3, SLAB, B::NSM>), dim3(ns), dim3(256), 0, st, tr->d3, nb, (int)O_B3, tr->slabs);
            hipLaunchKernelGGL((k_conv_dgrad<B::H - 1, 63, 32, 48>), tile_grid(nb * B::P2), dim3(256), 0, st, tr->d3, tr->w + O_K3, tr->a2, tr->d2, nb * B::P2);
            train_mark(tr, TS_CONV2);
            hipLaunchKernelGGL((k_conv_wgrad<B::H, W, 24, 32, 3, SLAB, B::NSM>), dim3(ns, 3), dim3(256), 0, st, tr->a1, tr->d2, nb, (int)O_K2, tr->slabs);
            hipLaunchKernelGGL((k_bias_grad<32, B::P2, SLAB, B::NSM>), dim3(ns), dim3(256), 0, st, tr->d2, nb, (int)O_B2, tr->slabs);
            hipLaunchKernelGGL((k_conv_dgrad<B::H, W, 24, 32>), tile_grid(nb * (B::H * W)), dim3(256), 0, st, tr->d2, tr->w + O_K2, tr->a1, tr->d1, nb * (B::H * W));
            train_mark(tr, TS_CONV1);
            hipLaunchKernelGGL((k_conv1_wgrad<B::H, B::NSM>), dim3(ns, 4), dim3(64 * C1W), 0, st, x, tr->d1, nb, tr->slabs);
            train_mark(tr, TS_PARAMS);
            if (s0 + nb < n) {                                          // not the last slice: fold its slabs into g, the workspace is reused
                hipLaunchKernelGGL(k_params<B>, dim3(blocks_for(B::NPAR)), dim3(256), 0, st, tr->g, tr->partial ? 1 : 0, tr->slabs, (int)ns, 0, 0.0f, tr->g, 0,
                                   tr->w, tr->m, tr->v, 0.0f, 0.0f, 0.0f, 0.0f);
                tr->partial = true;
            } else {
                tr->pending_ns = (int)ns;
                tr->pending_gamma = gamma;
            }
        }
        if (grad_dev)
            hipLaunchKernelGGL(k_params<B>, dim3(blocks_for(B::NPAR)), dim3(256), 0, st, tr->g, tr->partial ? 1 : 0, tr->slabs, tr->pending_ns, 1, gamma, grad_dev, 0,
                               tr->w, tr->m, tr->v, 0.0f, 0.0f, 0.0f, 0.0f);
        hipLaunchKernelGGL(k_wsq<B>, dim3(WSQ_BLOCKS), dim3(256), 0, st, tr->w, reinterpret_cast<double *>(tr->wsq));
        hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(1024), 0, st, tr->loss, n, reinterpret_cast<const double *>(tr->wsq), gamma, tr->loss2);
        train_mark(tr, TS_N);
        NC_HIP(ctx, hipGetLastError());
        return train_finish_loss_grad(tr, U::NAME, tr->loss2, 2, U::BAD_LABELS, loss2_host);
    }

    static int adam(indel_train_state *tr, float lr, float beta1, float beta2, float eps)
    {
        if (!tr) return NC_ERR_ARG;
        nc_ctx *ctx = tr->ctx;
        if (!tr->have_grad) return nc_fail(ctx, NC_ERR_STATE, "%s_adam: no gradient (%s_loss_grad comes first, once per step)", U::NAME, U::NAME);
        NC_HIP(ctx, hipSetDevice(ctx->device));
        tr->t++;
        hipLaunchKernelGGL(k_params<B>, dim3(blocks_for(B::NPAR)), dim3(256), 0, ctx->stream, tr->g, tr->partial ? 1 : 0, tr->slabs, tr->pending_ns, 1, tr->pending_gamma,
                           (float *)nullptr, 1, tr->w, tr->m, tr->v, train_lr_t(lr, beta1, beta2, tr->t), beta1, beta2, eps);
        NC_HIP(ctx, hipGetLastError());
        tr->have_grad = false;
        return NC_OK;
    }
};

}   // namespace

// The trunk the two SNP training units share (nc_train.hip: the diploid model, nc_train_hap.hip: the haploid model): conv1 as 1x5 | 5x1 | 5x5
// to 48 channels, conv2 to [4][20][32], conv3 to [3][9][64], fc1 1,728 -> 48.  Both blobs (weights.LAYER_SPECS[KIND_SNP], [KIND_SNP_HAP]) begin
// with these layers, kernel then bias of each, so the trunk's offsets are the same numbers in both and stand here once; what differs is what
// follows fc1 and with it NPAR, the floats per gradient slab, a template parameter of the two kernels that write slabs.
// lane l of an MFMA: A[row l&15][k l>>4], B[k l>>4][col l&15], C/D col l&15, row 4*(l>>4)+r (the lane maps of nc_cnn_fp32.hip).
#pragma once
#include "nc_train.h"

namespace {

constexpr int SLAB = 64;                                   // sites per slab = 4 MFMA tiles of 16
constexpr int64_t MAX_SLICE = 4096;                        // sites whose activations the workspace holds at once
// canonical blob offsets of the trunk; O_TRUNK_END = the first float behind fc1's bias
constexpr int O_K11 = 0, O_B11 = 400, O_K12 = 416, O_B12 = 816, O_K13 = 832, O_B13 = 2832, O_K2 = 2848, O_B2 = 12064, O_K3 = 12096, O_B3 = 24384;
constexpr int O_KF = 24448, O_BF = 107392, O_TRUNK_END = 107440;
constexpr int N1 = 205 * 48, N2 = 80 * 32, N3 = 27 * 64, XS = 1028;   // floats per site: conv1 - conv3 outputs, the scaled input (padded)

__device__ __forceinline__ bool trunk_is_bias(int i)      // i < O_TRUNK_END
{
    if (i < O_K2) return (i >= O_B11 && i < O_K12) || (i >= O_B12 && i < O_K13) || i >= O_B13;
    if (i < O_KF) return (i >= O_B2 && i < O_K3) || i >= O_B3;
    return i >= O_BF;
}

// the coverage scale of nc_snp_forward, mode 0 (snpCaller.py:93-96): rows 1..4, channels 0..3
__global__ __launch_bounds__(256) void k_scale_x(const float *__restrict__ x, const double *__restrict__ scale, float *__restrict__ xs, int64_t n)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * 1025) return;
    const int64_t s = g / 1025;
    const int i = (int)(g - s * 1025), h = i / 205, c = i % 5;
    float v = x[g];
    if (h > 0 && c < 4) v *= (float)scale[s];
    xs[s * XS + i] = v;
}

// conv1 (1x5, 5x1, 5x5, same padding) of one output position per lane; weights are wave-uniform operands.  x: [site][pitch]
__global__ __launch_bounds__(256) void k_conv1_fwd(const float *__restrict__ x, int pitch, const float *__restrict__ w, float *__restrict__ a1, int64_t npos)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= npos) return;
    const int64_t site = g / 205;
    const int r = (int)(g - site * 205), h = r / 41, x0 = r - h * 41;
    const float *xs = x + site * pitch;
    float acc[48];
#pragma unroll
    for (int o = 0; o < 16; o++) { acc[o] = w[O_B11 + o]; acc[16 + o] = w[O_B12 + o]; acc[32 + o] = w[O_B13 + o]; }
#pragma unroll 1
    for (int dy = 0; dy < 5; dy++) {
        const int iy = h + dy - 2;
#pragma unroll 1
        for (int dx = 0; dx < 5; dx++) {
            const int ix = x0 + dx - 2;
            const bool in = iy >= 0 && iy < 5 && ix >= 0 && ix < 41;
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const float xv = in ? xs[(iy * 41 + ix) * 5 + c] : 0.0f;
                const float *w3 = w + O_K13 + ((dy * 5 + dx) * 5 + c) * 16;
#pragma unroll
                for (int o = 0; o < 16; o++) acc[32 + o] = fmaf(xv, w3[o], acc[32 + o]);
                if (dy == 2) {
                    const float *w1 = w + O_K11 + (dx * 5 + c) * 16;
#pragma unroll
                    for (int o = 0; o < 16; o++) acc[o] = fmaf(xv, w1[o], acc[o]);
                }
                if (dx == 2) {
                    const float *w2 = w + O_K12 + (dy * 5 + c) * 16;
#pragma unroll
                    for (int o = 0; o < 16; o++) acc[16 + o] = fmaf(xv, w2[o], acc[16 + o]);
                }
            }
        }
    }
    float4 *op = reinterpret_cast<float4 *>(a1 + g * 48);
#pragma unroll
    for (int o = 0; o < 48; o += 4) op[o / 4] = make_float4(selu_acc(acc[o]), selu_acc(acc[o + 1]), selu_acc(acc[o + 2]), selu_acc(acc[o + 3]));
}

// fc1 forward: k3_fc1<48, 1> of nc_cnn_fp32.hip (M = 16 sites, split-K over the four waves, combined through LDS) without its load pipeline.
// It also writes SELU' of its 48 units, taken from the pre-activation it holds (see selud_pre).
__global__ __launch_bounds__(256) void k_fc1_fwd(const float *__restrict__ in, const float *__restrict__ wk, const float *__restrict__ wb,
                                                 float *__restrict__ out, float *__restrict__ dout, int64_t n)
{
    constexpr int F = 48, TN = 3, K = N3;
    __shared__ float red[3][TN][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int64_t tile0 = (int64_t)blockIdx.x * 16;
    int64_t s = tile0 + c16;
    if (s >= n) s = n - 1;
    const float *ip = in + s * K + 4 * q;
    const float *wl = wk + (4 * q) * F + c16;
    f32x4v acc[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const float b = wv == 0 ? wb[tn * 16 + c16] : 0.0f;
        acc[tn] = (f32x4v){b, b, b, b};
    }
    constexpr int NG = K / 16;                                           // 108 groups of 16: 27 per wave
    for (int j = wv * (NG / 4); j < (wv + 1) * (NG / 4); j++) {
        const float4 a = *reinterpret_cast<const float4 *>(ip + 16 * j);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float av = i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : a.w;
#pragma unroll
            for (int tn = 0; tn < TN; tn++) acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wl[(16 * j + i) * F + tn * 16], acc[tn], 0, 0, 0);
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
                const float v = acc[tn][r] + red[0][tn][r][lane] + red[1][tn][r][lane] + red[2][tn][r][lane];
                if (so < n) {
                    out[so * F + tn * 16 + c16] = selu_acc(v);
                    dout[so * F + tn * 16 + c16] = selud_pre(v);
                }
            }
        }
    }
}

template <int NI, int NO>
__device__ __forceinline__ void dense(const float (&in)[NI], const float *__restrict__ k, const float *__restrict__ b, float (&out)[NO], bool act,
                                      float *deriv = nullptr)
{
#pragma unroll
    for (int o = 0; o < NO; o++) out[o] = b[o];
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int o = 0; o < NO; o++) out[o] = fmaf(in[i], k[i * NO + o], out[o]);
    if (act) {
#pragma unroll
        for (int o = 0; o < NO; o++) {
            if (deriv) deriv[o] = selud_pre(out[o]);
            out[o] = selu_acc(out[o]);
        }
    }
}

// fc1 weight gradient dW[k][o] = sum_s a3[s][k] d[s][o] of one slab: M = k (108 tiles of 16), N = 48, K = the slab's 64 sites (16 steps).
// grid (slabs, 9): 36 waves per slab, three k tiles each; a wave holds the slab's d fragments in registers.
template <int NPAR>
__global__ __launch_bounds__(256) void k_fc1_wgrad(const float *__restrict__ a3, const float *__restrict__ df1, int64_t n, float *__restrict__ slabs)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int64_t sb = (int64_t)blockIdx.x * SLAB;
    float b[16][3];
#pragma unroll
    for (int st = 0; st < 16; st++) {
        const int64_t s = sb + 4 * st + q;
#pragma unroll
        for (int tn = 0; tn < 3; tn++) b[st][tn] = s < n ? df1[s * 48 + tn * 16 + c16] : 0.0f;
    }
    float *out = slabs + (int64_t)blockIdx.x * NPAR + O_KF;
    for (int kt = blockIdx.y * 4 + wv; kt < 108; kt += 36) {
        f32x4v acc[3] = {(f32x4v){0, 0, 0, 0}, (f32x4v){0, 0, 0, 0}, (f32x4v){0, 0, 0, 0}};
#pragma unroll
        for (int st = 0; st < 16; st++) {
            const int64_t s = sb + 4 * st + q;
            const float a = s < n ? a3[s * N3 + kt * 16 + c16] : 0.0f;
#pragma unroll
            for (int tn = 0; tn < 3; tn++) acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[st][tn], acc[tn], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int tn = 0; tn < 3; tn++) out[(kt * 16 + 4 * q + r) * 48 + tn * 16 + c16] = acc[tn][r];
    }
}

// fc1 data gradient d3[s][k] = SELU'(a3[s][k]) sum_o W[k][o] d[s][o]: M = k (the weights as the A operand, so a lane's four results are four
// consecutive k of one site: one dwordx4 store), N = 16 sites, K = 48 in float4 pieces (slot q of step (j, i) is o = 16 j + 4 q + i).
__global__ __launch_bounds__(256) void k_fc1_dgrad(const float *__restrict__ wk, const float *__restrict__ df1, const float *__restrict__ a3, int64_t n,
                                                   float *__restrict__ d3)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int64_t s = (int64_t)blockIdx.x * 16 + c16, sc = s < n ? s : n - 1;
    float4 bd[3];
#pragma unroll
    for (int j = 0; j < 3; j++) bd[j] = *reinterpret_cast<const float4 *>(df1 + sc * 48 + 16 * j + 4 * q);
    for (int kt = wv * 27; kt < wv * 27 + 27; kt++) {
        f32x4v acc = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float4 a = *reinterpret_cast<const float4 *>(wk + (kt * 16 + c16) * 48 + 16 * j + 4 * q);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bd[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bd[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bd[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bd[j].w, acc, 0, 0, 0);
        }
        if (s < n) {
            const int64_t o = s * N3 + kt * 16 + 4 * q;
            const float4 y = *reinterpret_cast<const float4 *>(a3 + o);
            *reinterpret_cast<float4 *>(d3 + o) = make_float4(acc[0] * selud(y.x), acc[1] * selud(y.y), acc[2] * selud(y.z), acc[3] * selud(y.w));
        }
    }
}

// conv1's three kernels (1x5, 5x1, 5x5, same padding) and their biases of one slab: M = (tap, ci) rows of one kernel, 25 or 125 of them, N = its 16
// output channels, K = output positions, four per MFMA; a tap outside the image enters as zero.  A kernel's bias follows it in the blob, so
// the bias is row 25 / 125: its A operand is the constant 1.  grid (slabs, 6): y = 0..3 the 5x5 kernel's rows 32 y .. 32 y + 31, y = 4 the 1x5,
// y = 5 the 5x1 kernel; the four waves take 16 sites of the slab each and combine through LDS in wave order.  x: [site][pitch]
template <int NPAR>
__global__ __launch_bounds__(256) void k_conv1_wgrad(const float *__restrict__ x, int pitch, const float *__restrict__ d1, int64_t n, float *__restrict__ slabs)
{
    __shared__ float red[3][2][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int br = blockIdx.y < 4 ? 2 : blockIdx.y - 4;                                     // 0: 1x5, 1: 5x1, 2: 5x5 = channels 16 br .. 16 br + 15
    const int nrows = br == 2 ? 125 : 25, base = br == 0 ? O_K11 : br == 1 ? O_K12 : O_K13, m0 = blockIdx.y < 4 ? 32 * blockIdx.y : 0;
    int kind[2], off[2], dyo[2], dxo[2];                                                    // kind 0: a tap, 1: the bias row, 2: padding
#pragma unroll
    for (int mw = 0; mw < 2; mw++) {
        const int m = m0 + 16 * mw + c16, tap = m / 5;
        kind[mw] = m < nrows ? 0 : m == nrows ? 1 : 2;
        dyo[mw] = (br == 2 ? tap / 5 : br == 1 ? tap : 2) - 2;
        dxo[mw] = (br == 2 ? tap % 5 : br == 0 ? tap : 2) - 2;
        off[mw] = (dyo[mw] * 41 + dxo[mw]) * 5 + m % 5;
    }
    const int64_t p0 = ((int64_t)blockIdx.x * SLAB + 16 * wv) * 205, pend = n * 205;
    f32x4v acc[2] = {(f32x4v){0, 0, 0, 0}, (f32x4v){0, 0, 0, 0}};
#pragma unroll 4
    for (int st = 0; st < 4 * 205; st++) {
        const int64_t p = p0 + 4 * st + q;
        const bool ok = p < pend;
        const int64_t site = p / 205;
        const int r = (int)(p - site * 205), h = r / 41, w = r - h * 41;
        const float *xs = x + site * pitch + r * 5;
        float a[2];
#pragma unroll
        for (int mw = 0; mw < 2; mw++) {
            const int iy = h + dyo[mw], ix = w + dxo[mw];
            a[mw] = 0.0f;
            if (ok && kind[mw] == 1) a[mw] = 1.0f;
            if (ok && kind[mw] == 0 && iy >= 0 && iy < 5 && ix >= 0 && ix < 41) a[mw] = xs[off[mw]];
        }
        const float b = ok ? d1[p * 48 + 16 * br + c16] : 0.0f;
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b, acc[1], 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int mw = 0; mw < 2; mw++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wv - 1][mw][r][lane] = acc[mw][r];
    }
    __syncthreads();
    if (wv == 0) {
        float *out = slabs + (int64_t)blockIdx.x * NPAR + base;
#pragma unroll
        for (int mw = 0; mw < 2; mw++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = m0 + 16 * mw + 4 * q + r;
                if (m <= nrows) out[m * 16 + c16] = ((acc[mw][r] + red[0][mw][r][lane]) + red[1][mw][r][lane]) + red[2][mw][r][lane];
            }
    }
}

// What a unit's loss_grad launches around its own heads kernels, on the unit's stream.  The buffers of one workspace slice:
struct snp_trunk_ws {
    float *w, *xs, *a1, *a2, *a3, *f1, *f1d, *df1, *d1, *d2, *d3, *slabs;
};

inline dim3 snp_tile_grid(int64_t npos)
{
    const int64_t t = (npos + 63) / 64;
    return dim3((unsigned)(t < 2048 ? t : 2048));
}

// conv1 - fc1 of `nb` sites (a slice) into the workspace
inline void snp_trunk_forward(const snp_trunk_ws &t, hipStream_t st, int64_t nb, const float *x, const double *scale)
{
    int pitch = 1025;
    if (scale) {
        hipLaunchKernelGGL(k_scale_x, dim3(blocks_for(nb * 1025)), dim3(256), 0, st, x, scale, t.xs, nb);
        x = t.xs;
        pitch = XS;
    }
    hipLaunchKernelGGL(k_conv1_fwd, dim3(blocks_for(nb * 205)), dim3(256), 0, st, x, pitch, t.w, t.a1, nb * 205);
    hipLaunchKernelGGL((k_conv23_fwd<5, 41, 48, 32>), snp_tile_grid(nb * 80), dim3(256), 0, st, t.a1, t.w + O_K2, t.w + O_B2, t.a2, nb * 80);
    hipLaunchKernelGGL((k_conv23_fwd<4, 20, 32, 64>), snp_tile_grid(nb * 27), dim3(256), 0, st, t.a2, t.w + O_K3, t.w + O_B3, t.a3, nb * 27);
    hipLaunchKernelGGL(k_fc1_fwd, dim3(blocks_for(nb, 16)), dim3(256), 0, st, t.a3, t.w + O_KF, t.w + O_BF, t.f1, t.f1d, nb);
}

// The trunk's gradients of a slice from d fc1 (t.df1) down to conv1's kernels, into the slice's slabs.  x / pitch: the input conv1 read;
// stage(i) is called before stage i = 0 fc1, 1 conv3, 2 conv2, 3 conv1 (the units record their timing events there).
template <int NPAR, typename Stage>
inline void snp_trunk_backward(const snp_trunk_ws &t, hipStream_t st, int64_t nb, const float *x, int pitch, Stage stage)
{
    const unsigned ns = (unsigned)((nb + SLAB - 1) / SLAB);
    stage(0);
    hipLaunchKernelGGL(k_fc1_wgrad<NPAR>, dim3(ns, 9), dim3(256), 0, st, t.a3, t.df1, nb, t.slabs);
    hipLaunchKernelGGL(k_fc1_dgrad, dim3(blocks_for(nb, 16)), dim3(256), 0, st, t.w + O_KF, t.df1, t.a3, nb, t.d3);
    stage(1);
    hipLaunchKernelGGL((k_conv_wgrad<4, 20, 32, 64, 2, SLAB, NPAR>), dim3(ns, 6), dim3(256), 0, st, t.a2, t.d3, nb, (int)O_K3, t.slabs);
    hipLaunchKernelGGL((k_bias_grad<64, 27, SLAB, NPAR>), dim3(ns), dim3(256), 0, st, t.d3, nb, (int)O_B3, t.slabs);
    hipLaunchKernelGGL((k_conv_dgrad<4, 20, 32, 64>), snp_tile_grid(nb * 80), dim3(256), 0, st, t.d3, t.w + O_K3, t.a2, t.d2, nb * 80);
    stage(2);
    hipLaunchKernelGGL((k_conv_wgrad<5, 41, 48, 32, 3, SLAB, NPAR>), dim3(ns, 6), dim3(256), 0, st, t.a1, t.d2, nb, (int)O_K2, t.slabs);
    hipLaunchKernelGGL((k_bias_grad<32, 80, SLAB, NPAR>), dim3(ns), dim3(256), 0, st, t.d2, nb, (int)O_B2, t.slabs);
    hipLaunchKernelGGL((k_conv_dgrad<5, 41, 48, 32>), snp_tile_grid(nb * 205), dim3(256), 0, st, t.d2, t.w + O_K2, t.a1, t.d1, nb * 205);
    stage(3);
    hipLaunchKernelGGL(k_conv1_wgrad<NPAR>, dim3(ns, 6), dim3(256), 0, st, x, pitch, t.d1, nb, t.slabs);
}

}   // namespace

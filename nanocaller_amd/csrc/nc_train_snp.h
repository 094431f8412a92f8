// The trunk the two SNP training units share (nc_train.hip: the diploid model, nc_train_hap.hip: the haploid model): conv1 as 1x5 | 5x1 | 5x5
// to 48 channels, conv2 to [4][20][32], conv3 to [3][9][64], fc1 1,728 -> 48.  Both blobs (weights.LAYER_SPECS[KIND_SNP], [KIND_SNP_HAP]) begin
// with these layers, kernel then bias of each, so the trunk's offsets are the same numbers in both and stand here once; what differs is what
// follows fc1 and with it NPAR, the floats per gradient slab, a template parameter of the two kernels that write slabs.
// Behind the kernels: k_params and the host side of a handle, snp_train<U>, over the unit U that each .hip file supplies with its kernels
// behind fc1 (as indel_train<U> of nc_train_indel.h; what no family owns is in nc_train.h).
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

// One parameter per lane: gradient = g_in (earlier slices, may be NULL) + the slabs in slab order (+ gamma w on kernel entries with `reg`);
// written to g_out (may be NULL); with `step` the Adam update in TensorFlow's form, w -= lr_t m / (sqrt(v) + eps).
template <class U>
__global__ __launch_bounds__(256) void k_params(const float *__restrict__ g_in, const float *__restrict__ slabs, int ns, int reg, float gamma,
                                                float *__restrict__ g_out, int step, float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                float lr_t, float b1, float b2, float eps)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= U::NPAR) return;
    float g = g_in ? g_in[i] : 0.0f;
    for (int k = 0; k < ns; k++) g += slabs[(int64_t)k * U::NPAR + i];
    const float wi = w[i];
    if (reg && !U::is_bias(i)) g = fmaf(gamma, wi, g);
    if (g_out) g_out[i] = g;
    if (step) {
        const float mi = fmaf(b1, m[i], (1.0f - b1) * g), vi = fmaf(b2, v[i], (1.0f - b2) * g * g);
        m[i] = mi;
        v[i] = vi;
        w[i] = wi - lr_t * mi / (sqrtf(vi) + eps);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host side of a handle
struct snp_train_state : train_state {
    float *xs, *a1, *a2, *a3, *f1, *f1d, *tact, *tdel, *df1, *d1, *d2, *d3, *slabs, *loss, *lossv;   // lossv: the loss terms, then the bad-label flag
};

inline dim3 snp_tile_grid(int64_t npos)
{
    const int64_t t = (npos + 63) / 64;
    return dim3((unsigned)(t < 2048 ? t : 2048));
}

// A unit U names its blob (U::NPAR, U::is_bias, the per-site records U::TA and U::TD, U::NSMALL = the parameters of its k_small_wgrad), its
// labels (U::NLAB per site, as many per-site losses) and loss terms (U::NLOSS), its entry points' prefix (U::NAME), the model it accepts
// (U::KIND, U::MODEL) and what a label outside the classes is called (U::BAD_LABELS; null where labels are not looked at on the device: then
// loss_grad waits only when the losses are asked for).  It launches its own kernels behind fc1:
//   static void heads(snp_train_state *, hipStream_t, int64_t nb, const int32_t *ref_code, const uint8_t *mask, float inv_keep,
//                     const uint8_t *label, float inv_n, float *probs, float *gt, float *loss)     (sets lossv[NLOSS] on a bad label)
//   static void small_wgrad(snp_train_state *, hipStream_t, unsigned ns, const int32_t *ref_code, int64_t nb)
//   static void loss_reduce(snp_train_state *, hipStream_t, int64_t n, float gamma)                (loss -> lossv[0 .. NLOSS))
template <class U>
struct snp_train {
    static constexpr int NPAR = U::NPAR;

    // conv1 - fc1 of `nb` sites (a slice) into the workspace; returns the input conv1 read and sets its pitch
    static const float *forward_trunk(snp_train_state *t, int64_t nb, const float *x, const double *scale, int &pitch)
    {
        hipStream_t st = t->ctx->stream;
        pitch = 1025;
        if (scale) {
            hipLaunchKernelGGL(k_scale_x, dim3(blocks_for(nb * 1025)), dim3(256), 0, st, x, scale, t->xs, nb);
            x = t->xs;
            pitch = XS;
        }
        hipLaunchKernelGGL(k_conv1_fwd, dim3(blocks_for(nb * 205)), dim3(256), 0, st, x, pitch, t->w, t->a1, nb * 205);
        hipLaunchKernelGGL((k_conv23_fwd<5, 41, 48, 32>), snp_tile_grid(nb * 80), dim3(256), 0, st, t->a1, t->w + O_K2, t->w + O_B2, t->a2, nb * 80);
        hipLaunchKernelGGL((k_conv23_fwd<4, 20, 32, 64>), snp_tile_grid(nb * 27), dim3(256), 0, st, t->a2, t->w + O_K3, t->w + O_B3, t->a3, nb * 27);
        hipLaunchKernelGGL(k_fc1_fwd, dim3(blocks_for(nb, 16)), dim3(256), 0, st, t->a3, t->w + O_KF, t->w + O_BF, t->f1, t->f1d, nb);
        return x;
    }

    template <class H>
    static int create(nc_ctx *ctx, int32_t kind, int64_t max_batch, H **out)
    {
        if (!ctx || !out) return NC_ERR_ARG;
        *out = nullptr;
        if (kind != U::KIND)
            return nc_fail(ctx, NC_ERR_UNSUPPORTED, "%s_create: only the %s model (kind %d) is trained here, not kind %d", U::NAME, U::MODEL, U::KIND, kind);
        if (max_batch < 1) return nc_fail(ctx, NC_ERR_ARG, "%s_create: max_batch", U::NAME);
        return train_create(ctx, max_batch, out, [](snp_train_state *tr) {
            tr->slice = tr->max_batch < MAX_SLICE ? tr->max_batch : MAX_SLICE;
            const size_t sl = (size_t)tr->slice, ns = (sl + SLAB - 1) / SLAB;
            const size_t sizes[] = {sl * XS, sl * N1, sl * N2, sl * N3, sl * 48, sl * 48, sl * U::TA, sl * U::TD, sl * 48, sl * N1, sl * N2, sl * N3, ns * NPAR,
                                    (size_t)tr->max_batch * U::NLAB, 8};
            float **const ptrs[] = {&tr->xs, &tr->a1, &tr->a2, &tr->a3, &tr->f1, &tr->f1d, &tr->tact, &tr->tdel, &tr->df1, &tr->d1, &tr->d2, &tr->d3, &tr->slabs,
                                    &tr->loss, &tr->lossv};
            return train_alloc(tr, U::NAME, NPAR, sizes, ptrs);
        });
    }

    // gt_dev: the diploid model's genotype output, null for the haploid one
    static int forward(snp_train_state *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                       float keep, float *probs_dev, float *gt_dev)
    {
        NC_TRY(train_check_call(tr, U::NAME, "forward", n, x_dev && ref_code_dev && probs_dev, keep));
        nc_ctx *ctx = tr->ctx;
        NC_HIP(ctx, hipSetDevice(ctx->device));
        if (keep == 1.0f) keep_mask_dev = nullptr;
        for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
            const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
            int pitch;
            forward_trunk(tr, nb, x_dev + s0 * NC_SNP_TENSOR, scale_dev ? scale_dev + s0 : nullptr, pitch);
            U::heads(tr, ctx->stream, nb, ref_code_dev + s0, keep_mask_dev ? keep_mask_dev + s0 * 48 : nullptr, 1.0f / keep, nullptr, 0.0f, probs_dev + s0 * 4,
                     gt_dev ? gt_dev + s0 * 2 : nullptr, tr->loss);
        }
        NC_HIP(ctx, hipGetLastError());
        return NC_OK;
    }

    static int loss_grad(snp_train_state *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                         float keep, const uint8_t *label_dev, float gamma, float *loss_host, float *grad_dev)
    {
        NC_TRY(train_check_call(tr, U::NAME, "loss_grad", n, x_dev && ref_code_dev && label_dev, keep));
        nc_ctx *ctx = tr->ctx;
        NC_HIP(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        if (keep == 1.0f) keep_mask_dev = nullptr;
        tr->have_grad = tr->partial = false;
        if (U::BAD_LABELS) NC_HIP(ctx, hipMemsetAsync(tr->lossv, 0, 8 * 4, st));
        for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
            const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
            const unsigned ns = (unsigned)((nb + SLAB - 1) / SLAB);
            train_mark(tr, TS_FWD);
            int pitch;
            const float *x = forward_trunk(tr, nb, x_dev + s0 * NC_SNP_TENSOR, scale_dev ? scale_dev + s0 : nullptr, pitch);
            train_mark(tr, TS_HEADS);
            U::heads(tr, st, nb, ref_code_dev + s0, keep_mask_dev ? keep_mask_dev + s0 * 48 : nullptr, 1.0f / keep, label_dev + s0 * U::NLAB, 1.0f / (float)n,
                     nullptr, nullptr, tr->loss + s0 * U::NLAB);
            U::small_wgrad(tr, st, ns, ref_code_dev + s0, nb);
            train_mark(tr, TS_FC1);
            hipLaunchKernelGGL(k_fc1_wgrad<NPAR>, dim3(ns, 9), dim3(256), 0, st, tr->a3, tr->df1, nb, tr->slabs);
            hipLaunchKernelGGL(k_fc1_dgrad, dim3(blocks_for(nb, 16)), dim3(256), 0, st, tr->w + O_KF, tr->df1, tr->a3, nb, tr->d3);
            train_mark(tr, TS_CONV3);
            hipLaunchKernelGGL((k_conv_wgrad<4, 20, 32, 64, 2, SLAB, NPAR>), dim3(ns, 6), dim3(256), 0, st, tr->a2, tr->d3, nb, (int)O_K3, tr->slabs);
            hipLaunchKernelGGL((k_bias_grad<64, 27, SLAB, NPAR>), dim3(ns), dim3(256), 0, st, tr->d3, nb, (int)O_B3, tr->slabs);
            hipLaunchKernelGGL((k_conv_dgrad<4, 20, 32, 64>), snp_tile_grid(nb * 80), dim3(256), 0, st, tr->d3, tr->w + O_K3, tr->a2, tr->d2, nb * 80);
            train_mark(tr, TS_CONV2);
            hipLaunchKernelGGL((k_conv_wgrad<5, 41, 48, 32, 3, SLAB, NPAR>), dim3(ns, 6), dim3(256), 0, st, tr->a1, tr->d2, nb, (int)O_K2, tr->slabs);
            hipLaunchKernelGGL((k_bias_grad<32, 80, SLAB, NPAR>), dim3(ns), dim3(256), 0, st, tr->d2, nb, (int)O_B2, tr->slabs);
            hipLaunchKernelGGL((k_conv_dgrad<5, 41, 48, 32>), snp_tile_grid(nb * 205), dim3(256), 0, st, tr->d2, tr->w + O_K2, tr->a1, tr->d1, nb * 205);
            train_mark(tr, TS_CONV1);
            hipLaunchKernelGGL(k_conv1_wgrad<NPAR>, dim3(ns, 6), dim3(256), 0, st, x, pitch, tr->d1, nb, tr->slabs);
            train_mark(tr, TS_PARAMS);
            if (s0 + nb < n) {                                          // not the last slice: fold its slabs into g, the workspace is reused
                hipLaunchKernelGGL(k_params<U>, dim3(blocks_for(NPAR)), dim3(256), 0, st, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, (int)ns, 0, 0.0f,
                                   tr->g, 0, tr->w, tr->m, tr->v, 0.0f, 0.0f, 0.0f, 0.0f);
                tr->partial = true;
            } else {
                tr->pending_ns = (int)ns;
                tr->pending_gamma = gamma;
            }
        }
        if (grad_dev)
            hipLaunchKernelGGL(k_params<U>, dim3(blocks_for(NPAR)), dim3(256), 0, st, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, tr->pending_ns, 1, gamma,
                               grad_dev, 0, tr->w, tr->m, tr->v, 0.0f, 0.0f, 0.0f, 0.0f);
        U::loss_reduce(tr, st, n, gamma);
        train_mark(tr, TS_N);
        NC_HIP(ctx, hipGetLastError());
        return train_finish_loss_grad(tr, U::NAME, tr->lossv, U::NLOSS, U::BAD_LABELS, loss_host);
    }

    static int adam(snp_train_state *tr, float lr, float beta1, float beta2, float eps)
    {
        if (!tr) return NC_ERR_ARG;
        nc_ctx *ctx = tr->ctx;
        if (!tr->have_grad) return nc_fail(ctx, NC_ERR_STATE, "%s_adam: no gradient (%s_loss_grad comes first, once per step)", U::NAME, U::NAME);
        NC_HIP(ctx, hipSetDevice(ctx->device));
        tr->t++;
        hipLaunchKernelGGL(k_params<U>, dim3(blocks_for(NPAR)), dim3(256), 0, ctx->stream, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, tr->pending_ns, 1,
                           tr->pending_gamma, (float *)nullptr, 1, tr->w, tr->m, tr->v, train_lr_t(lr, beta1, beta2, tr->t), beta1, beta2, eps);
        NC_HIP(ctx, hipGetLastError());
        tr->have_grad = false;
        return NC_OK;
    }
};

}   // namespace

// CNN forward for the four NanoCaller models (gfx950): the driver.  Head kernels, the range guard, nc_load_weights, the forward entry
// points and the two trunk drivers; the trunk and fc1 kernels and the packers of their weights are in the units nc_cnn.h lists.
//
// Restates model_architect.py:36-64, model_architect_SNP_haploid.py:33-53, model_architect_indel.py:28-48,
// model_architect_indels_haploid.py:29-48: three parallel `same` convs (1x5, 5x1, 5x5)
// -> concat -> two `valid` 2x3 convs with stride (1,2) -> flatten -> dense layers; SELU everywhere.
//
// One path per model family and precision.  The default is split precision ("f16x3"): every fp32 product is evaluated as
// hi*hi + hi*lo + lo*hi of fp16 halves on v_mfma_f32_16x16x32_f16 with fp32 accumulation; the exact-fp32 forms
// use v_mfma_f32_16x16x4_f32, which is bit for bit an fmaf chain.
//   SNP trunk (conv1-conv3), split precision: k5_trunk_lin (int16 tensors: conv1 by linearity) or k5_trunk_p3 (float32
//             tensors, or NC_TRUNK_LIN=0); persistent, wave-specialised, one workgroup per CU, weights resident in VGPRs.
//   SNP trunk, exact fp32: k4_conv12.
//   SNP fc1: k6_fc1_h3 (split precision) or k3_fc1<48, 1> (exact fp32).
//   indel trunk, split precision: k10_indel_trunk_h3 (the three convs, rows streamed through LDS rings); exact fp32 (also when
//             the weights' range bound does not cover |x| <= 1): k2_conv1_x4 + k7_conv23_mfma x 2.  Indel fc1: k3_fc1<32, 2>.
//   heads: k_snp_heads, k_snp_hap_heads, k_indel_heads (per-site scalar code, accurate expf).
#include <algorithm>

#include "nc_cnn.h"

namespace {

__device__ __forceinline__ void dense_small(const float *in, int n_in, const float *k, const float *b, int n_out, float *out, bool act)
{
    for (int o = 0; o < n_out; o++) {
        float acc = b[o];
        for (int i = 0; i < n_in; i++) acc = fmaf(in[i], k[i * n_out + o], acc);
        out[o] = act ? selu_acc(acc) : acc;
    }
}

__device__ __forceinline__ void softmax_small(float *x, int n)
{
    float m = x[0];
    for (int i = 1; i < n; i++) m = fmaxf(m, x[i]);
    float sum = 0.0f;
    for (int i = 0; i < n; i++) { x[i] = expf(x[i] - m); sum += x[i]; }
    for (int i = 0; i < n; i++) x[i] = x[i] / sum;
}

// SNP diploid tail: fa, four allele heads, fc2, fc3, GT (model_architect.py:53-62). w = pointer to fa.k
__global__ __launch_bounds__(256) void k_snp_heads(const float *__restrict__ fc1, const float *__restrict__ w,
                                                   const int32_t *__restrict__ ref_code, int64_t n, float *__restrict__ probs,
                                                   float *__restrict__ gt)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    float f1[48], fa[16], in17[17], heads[4][2], fc2[16], in24[24], fc3[8], g[2];
    for (int i = 0; i < 48; i++) f1[i] = fc1[s * 48 + i];
    const float *p = w;
    dense_small(f1, 48, p, p + 768, 16, fa, true);
    p += 768 + 16;
    for (int i = 0; i < 16; i++) in17[i] = fa[i];
    const int rc = ref_code[s];
    for (int h = 0; h < 4; h++) {
        in17[16] = rc == h ? 1.0f : 0.0f;
        dense_small(in17, 17, p, p + 34, 2, heads[h], false);
        p += 34 + 2;
        softmax_small(heads[h], 2);
        probs[s * 4 + h] = heads[h][1];
    }
    dense_small(f1, 48, p, p + 768, 16, fc2, true);
    p += 768 + 16;
    for (int i = 0; i < 16; i++) in24[i] = fc2[i];
    for (int h = 0; h < 4; h++) { in24[16 + 2 * h] = heads[h][0]; in24[17 + 2 * h] = heads[h][1]; }
    dense_small(in24, 24, p, p + 192, 8, fc3, true);
    p += 192 + 8;
    dense_small(fc3, 8, p, p + 16, 2, g, false);
    softmax_small(g, 2);
    if (gt) { gt[s * 2] = g[0]; gt[s * 2 + 1] = g[1]; }
}

// haploid SNP tail: fc2, fc3 = Dense(4, selu) on [fc2, ref one-hot], softmax (model_architect_SNP_haploid.py:49-51)
__global__ __launch_bounds__(256) void k_snp_hap_heads(const float *__restrict__ fc1, const float *__restrict__ w,
                                                       const int32_t *__restrict__ ref_code, int64_t n, float *__restrict__ probs)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    float f1[48], in20[20], out[4];
    for (int i = 0; i < 48; i++) f1[i] = fc1[s * 48 + i];
    const float *p = w;
    dense_small(f1, 48, p, p + 768, 16, in20, true);
    p += 768 + 16;
    const int rc = ref_code[s];
    for (int b = 0; b < 4; b++) in20[16 + b] = rc == b ? 1.0f : 0.0f;
    dense_small(in20, 20, p, p + 80, 4, out, true);
    softmax_small(out, 4);
    for (int b = 0; b < 4; b++) probs[s * 4 + b] = out[b];
}

// indel tail: fc2 (32->24 selu), fc3 (24->4 softmax | 24->1 sigmoid)
__global__ __launch_bounds__(256) void k_indel_heads(const float *__restrict__ fc1, const float *__restrict__ w, int nout, int64_t n,
                                                     float *__restrict__ probs)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    float f1[32], f2[24], out[4];
    for (int i = 0; i < 32; i++) f1[i] = fc1[s * 32 + i];
    const float *p = w;
    dense_small(f1, 32, p, p + 768, 24, f2, true);
    p += 768 + 24;
    dense_small(f2, 24, p, p + 24 * nout, nout, out, false);
    if (nout == 4) {
        softmax_small(out, 4);
        for (int b = 0; b < 4; b++) probs[s * 4 + b] = out[b];
    } else {
        probs[s] = 1.0f / (1.0f + expf(-out[0]));
    }
}

const size_t NPARAM[4] = {109370, 108308, 634420, 158185};

// conv1-conv3 + fc1 of `nb` SNP sites starting at site s0 of the call's arrays -> *f1_out [nb][48]; *tail = the heads' weights
int run_snp_trunk(nc_ctx *ctx, const nc_weights &w, int64_t s0, int64_t nb, const void *x_dev, const double *scale, int scale_mode, const float **f1_out, const float **tail)
{
    constexpr int64_t n3 = 3 * 9 * 64, F = 48;
    NC_TRY(nc_ensure(ctx, ctx->cnn_c, (size_t)(nb * (n3 + F)) * 4 + 64));
    float *a3 = (float *)ctx->cnn_c.p, *f1 = a3 + ((nb * n3 + 3) & ~int64_t(3));
    const float *kf = w.dev + (400 + 16) * 2 + 2000 + 16 + 6 * 48 * 32 + 32 + 6 * 32 * 64 + 64, *bf = kf + n3 * F;
    *tail = bf + F;
    *f1_out = f1;
    SnpTrunkArgs a = {ctx->stream, nullptr, nullptr, nullptr, nullptr, a3, nb, s0, scale, scale_mode, w.x_limit, ctx->range_sites};
    if (ctx->x_i16) a.x_i16 = (const int16_t *)x_dev + s0 * NC_SNP_TENSOR;
    else a.x_f32 = (const float *)x_dev + s0 * NC_SNP_TENSOR;
    // timing mode: the start / stop events ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL), so they
    // read the kernel's execution time and put no barrier packets between the launches of a batch
    if (ctx->timing && ctx->n_kev + 2 <= 128) {
        for (int e = 0; e < 2; e++)
            if (!ctx->kev[ctx->n_kev + e]) NC_HIP(ctx, hipEventCreate(&ctx->kev[ctx->n_kev + e]));
        a.ev0 = ctx->kev[ctx->n_kev];
        a.ev1 = ctx->kev[ctx->n_kev + 1];
        ctx->n_kev += 2;
    }
    const SnpTrunk t = nc_cnn_snp_trunk_select(ctx);
    if (t.kernel_id == NC_TRUNK_FP32) {
        nc_cnn_launch_k4_conv12(a, w.packed);
        nc_cnn_launch_fc1_fp32(ctx->stream, F, a3, (int)n3, kf, bf, f1, nb);
    } else {
        nc_cnn_launch_k5_trunk(t.kernel_id, a, (const uint8_t *)w.packed_h);
        nc_cnn_launch_fc1_h3(ctx->stream, a3, (const uint8_t *)w.packed_h, f1, nb);
    }
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

// the same of `nb` indel sites (tensors [H][128][2], H = 15 or 5) -> *f1_out [nb][32]: k10_indel_trunk_h3, or the exact fp32 kernels
// (k2_conv1_x4 + k7_conv23_mfma x 2) in exact mode and for a model whose range bound does not cover msa()'s frequencies, |x| <= 1
// (x_limit < 1: none of the shipped ones)
int run_indel_trunk(nc_ctx *ctx, const nc_weights &w, int H, int64_t nb, const float *x_batch, const float **f1_out, const float **tail)
{
    constexpr int W = 128, CI = 2, C1 = 8, C2 = 32, C3 = 48, F = 32, W2 = (W - 3) / 2 + 1, W3 = (W2 - 3) / 2 + 1;
    const int64_t n1 = (int64_t)H * W * 3 * C1, n2 = (int64_t)(H - 1) * W2 * C2, n3 = (int64_t)(H - 2) * W3 * C3;
    const bool h3 = !ctx->cnn_exact_fp32 && w.x_limit >= 1.0f;
    if (!h3) {
        NC_TRY(nc_ensure(ctx, ctx->cnn_a, (size_t)(nb * n1) * 4));
        NC_TRY(nc_ensure(ctx, ctx->cnn_b, (size_t)(nb * n2) * 4));
    }
    NC_TRY(nc_ensure(ctx, ctx->cnn_c, (size_t)(nb * (n3 + F)) * 4 + 64));
    float *a3 = (float *)ctx->cnn_c.p, *f1 = a3 + ((nb * n3 + 3) & ~int64_t(3));
    const float *kf = w.dev + (5 + 5 + 25) * CI * C1 + 3 * C1 + 6 * 3 * C1 * C2 + C2 + 6 * C2 * C3 + C3, *bf = kf + n3 * F;
    *tail = bf + F;
    *f1_out = f1;
    if (h3) NC_TRY(nc_cnn_launch_k10(ctx, H, x_batch, (const uint8_t *)w.packed_h, a3, nb));
    else nc_cnn_launch_indel_convs_fp32(ctx->stream, H, x_batch, w.dev, (float *)ctx->cnn_a.p, (float *)ctx->cnn_b.p, a3, nb);
    nc_cnn_launch_fc1_fp32(ctx->stream, F, a3, (int)n3, kf, bf, f1, nb);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

// Range guard of the split-precision kernels: their epilogues clamp activations at 6e4 (fp16).  With L_l = the largest L1 norm of
// an output channel's weights and |selu(v)| <= max(lambda |v|, lambda alpha), an input bounded by X bounds every activation:
//   a_l = max(lambda (L_l a_{l-1} + max|b_l|), lambda alpha),  a_0 = X;    x_limit = the largest X with max a_l < 6e4.
float cnn_x_limit(int kind, const float *blob)
{
    const bool snp = kind == NC_MODEL_SNP || kind == NC_MODEL_SNP_HAP;
    const int CI = snp ? 5 : 2, C1 = snp ? 16 : 8, C2 = 32, C3 = snp ? 64 : 48;
    auto l1 = [](const float *k, int n_in, int cout) {
        double best = 0;
        for (int c = 0; c < cout; c++) {
            double acc = 0;
            for (int i = 0; i < n_in; i++) acc += std::fabs((double)k[(size_t)i * cout + c]);
            best = std::max(best, acc);
        }
        return best;
    };
    auto amax = [](const float *b, int n) { double m = 0; for (int i = 0; i < n; i++) m = std::max(m, std::fabs((double)b[i])); return m; };
    const float *k11 = blob, *b11 = k11 + 5 * CI * C1, *k12 = b11 + C1, *b12 = k12 + 5 * CI * C1, *k13 = b12 + C1, *b13 = k13 + 25 * CI * C1;
    const float *k2 = b13 + C1, *b2 = k2 + 6 * 3 * C1 * C2, *k3 = b2 + C2, *b3 = k3 + 6 * C2 * C3;
    const double L1 = std::max(l1(k11, 5 * CI, C1), std::max(l1(k12, 5 * CI, C1), l1(k13, 25 * CI, C1)));
    const double B1 = std::max(amax(b11, C1), std::max(amax(b12, C1), amax(b13, C1)));
    const double L2 = l1(k2, 6 * 3 * C1, C2), B2 = amax(b2, C2), L3 = l1(k3, 6 * C2, C3), B3 = amax(b3, C3);
    const double LAM = 1.0507009873554805, LA = LAM * 1.6732632423543772, CAP = 60000.0 * 0.999;
    auto worst = [&](double X) {
        const double a1 = std::max(LAM * (L1 * X + B1), LA), a2 = std::max(LAM * (L2 * a1 + B2), LA), a3 = std::max(LAM * (L3 * a2 + B3), LA);
        // the indel kernel clamps conv1's and conv2's outputs only (conv3 leaves k10_indel_trunk_h3 as fp32)
        return snp ? std::max(a1, std::max(a2, a3)) : std::max(a1, a2);
    };
    double lo = 0.0, hi = 1e6;
    if (worst(0.0) >= CAP) hi = 0.0;
    for (int it = 0; it < 60 && hi > 0.0; it++) {
        const double mid = 0.5 * (lo + hi);
        if (worst(mid) < CAP) lo = mid; else hi = mid;
    }
    return (float)lo;
}

// a weight blob on the device: allocated at the model's first load, rewritten by a later one
int upload_blob(nc_ctx *ctx, void **dev, const void *host, size_t bytes, const char *what)
{
    if (!*dev) {
        hipError_t e = hipMalloc(dev, bytes);
        if (e != hipSuccess) return nc_fail(ctx, NC_ERR_NOMEM, "hipMalloc %s: %s", what, hipGetErrorString(e));
    }
    NC_HIP(ctx, hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

}   // namespace

extern "C" {

int nc_load_weights(nc_ctx *ctx, int32_t kind, const float *blob_host, size_t n_floats)
{
    if (!ctx) return NC_ERR_ARG;
    if (kind < 0 || kind > 3 || !blob_host) return nc_fail(ctx, NC_ERR_ARG, "nc_load_weights: bad argument");
    if (n_floats != NPARAM[kind])
        return nc_fail(ctx, NC_ERR_ARG, "nc_load_weights: kind %d expects %zu floats, got %zu", kind, NPARAM[kind], n_floats);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    nc_weights &w = ctx->w[kind];
    NC_TRY(upload_blob(ctx, (void **)&w.dev, blob_host, n_floats * 4, "weights"));
    w.n = n_floats;
    w.x_limit = cnn_x_limit(kind, blob_host);
    if (kind == NC_MODEL_SNP || kind == NC_MODEL_SNP_HAP) {
        const std::vector<float> pk = nc_cnn_pack_k4(blob_host);
        NC_TRY(upload_blob(ctx, (void **)&w.packed, pk.data(), pk.size() * 4, "packed weights"));
        const std::vector<uint8_t> hp = nc_cnn_pack_snp_h3(blob_host);
        NC_TRY(upload_blob(ctx, &w.packed_h, hp.data(), hp.size(), "packed fp16 weights"));
    } else {
        const std::vector<uint8_t> hp = nc_cnn_pack_indel_h3(blob_host);
        NC_TRY(upload_blob(ctx, &w.packed_h, hp.data(), hp.size(), "packed fp16 weights"));
    }
    return NC_OK;
}


int nc_snp_forward(nc_ctx *ctx, int32_t kind, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev,
                   int32_t scale_mode, float *probs_dev, float *gt_dev)
{
    return nc_snp_forward_drain(ctx, kind, n, x_dev, ref_code_dev, scale_dev, scale_mode, probs_dev, gt_dev, nullptr, nullptr, nullptr);
}

int nc_snp_forward_drain(nc_ctx *ctx, int32_t kind, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev,
                         int32_t scale_mode, float *probs_dev, float *gt_dev, void *copy_stream, float *probs_host, float *gt_host)
{
    if (!ctx) return NC_ERR_ARG;
    if (probs_host && !copy_stream) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_forward_drain: host drain needs a copy stream");
    if (kind != NC_MODEL_SNP && kind != NC_MODEL_SNP_HAP) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_forward: not an SNP model kind");
    if (!ctx->w[kind].dev) return nc_fail(ctx, NC_ERR_STATE, "nc_snp_forward: weights of kind %d not loaded", kind);
    if (n < 0 || (n && (!x_dev || !ref_code_dev || !probs_dev))) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_forward: null argument");
    if (scale_mode != 0 && scale_mode != 1) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_forward: scale_mode");
    if (ctx->x_i16 && ctx->cnn_exact_fp32) return nc_fail(ctx, NC_ERR_STATE, "nc_snp_forward: int16 tensors are read by the split-precision trunk only");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NcTimer tm(ctx, 2);
    if (ctx->timing) nc_timing_resolve(ctx, 4);   // fold an earlier call's per-launch events in before they are re-used
    ctx->n_kev = 0;
    // 262,144 sites per batch (1.8 GB of conv3 activations): the kernel boundaries between trunk, fc1 and heads cost ~40 us per
    // batch, and a batch still drains to the host while the next one computes; one launch for a whole 625k-site contig is
    // slower again (the trunk itself loses 3 % on a 4.3 GB activation buffer)
    const int64_t BATCH = 262144;
    for (int64_t s0 = 0; s0 < n; s0 += BATCH) {
        const int64_t nb = n - s0 < BATCH ? n - s0 : BATCH;
        const float *tail = nullptr, *f1 = nullptr;
        NC_TRY(run_snp_trunk(ctx, ctx->w[kind], s0, nb, x_dev, scale_dev, scale_mode, &f1, &tail));   // (x_dev: int16 tensors after nc_set_tensor_format)
        if (kind == NC_MODEL_SNP)
            hipLaunchKernelGGL(k_snp_heads, dim3(blocks_for(nb)), dim3(256), 0, ctx->stream, f1, tail, ref_code_dev + s0, nb,
                               probs_dev + s0 * 4, gt_dev ? gt_dev + s0 * 2 : nullptr);
        else
            hipLaunchKernelGGL(k_snp_hap_heads, dim3(blocks_for(nb)), dim3(256), 0, ctx->stream, f1, tail, ref_code_dev + s0, nb,
                               probs_dev + s0 * 4);
        NC_HIP(ctx, hipGetLastError());
        if (probs_host) {                    // drain this batch on the copy stream while the next batch computes
            const int slot = (int)((s0 / BATCH) & 3);
            if (!ctx->drain_ev[slot]) NC_HIP(ctx, hipEventCreateWithFlags(&ctx->drain_ev[slot], hipEventDisableTiming));
            NC_HIP(ctx, hipEventRecord(ctx->drain_ev[slot], ctx->stream));
            NC_HIP(ctx, hipStreamWaitEvent((hipStream_t)copy_stream, ctx->drain_ev[slot], 0));
            NC_TRY(nc_d2h(ctx, probs_host + s0 * 4, probs_dev + s0 * 4, (size_t)nb * 16, (hipStream_t)copy_stream));
            if (gt_host && gt_dev)
                NC_TRY(nc_d2h(ctx, gt_host + s0 * 2, gt_dev + s0 * 2, (size_t)nb * 8, (hipStream_t)copy_stream));
        }
    }
    tm.stop();
    if (ctx->timing) ctx->kev_pending = true;     // resolved by nc_last_kernel_ms(4 / 5)
    return NC_OK;
}

int nc_cnn_x_limit(nc_ctx *ctx, int32_t kind, float *x_limit)
{
    if (!ctx || kind < 0 || kind > 3 || !x_limit) return NC_ERR_ARG;
    if (!ctx->w[kind].dev) return nc_fail(ctx, NC_ERR_STATE, "nc_cnn_x_limit: weights of kind %d not loaded", kind);
    *x_limit = ctx->w[kind].x_limit;
    return NC_OK;
}

int nc_snp_trunk_info(nc_ctx *ctx, int32_t *mfma_per_site, int32_t *kernel_id)
{
    if (!ctx) return NC_ERR_ARG;
    const SnpTrunk t = nc_cnn_snp_trunk_select(ctx);
    if (mfma_per_site) *mfma_per_site = t.mfma_per_site;
    if (kernel_id) *kernel_id = t.kernel_id;
    return NC_OK;
}

int nc_cnn_range_watch(nc_ctx *ctx, uint8_t *site_flags_dev)
{
    if (!ctx) return NC_ERR_ARG;
    ctx->range_sites = site_flags_dev;
    return NC_OK;
}

int nc_indel_forward(nc_ctx *ctx, int32_t kind, int64_t n, const float *x_dev, float *probs_dev)
{
    if (!ctx) return NC_ERR_ARG;
    if (kind != NC_MODEL_INDEL && kind != NC_MODEL_INDEL_HAP) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_forward: not an indel model kind");
    if (!ctx->w[kind].dev) return nc_fail(ctx, NC_ERR_STATE, "nc_indel_forward: weights of kind %d not loaded", kind);
    if (n < 0 || (n && (!x_dev || !probs_dev))) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_forward: null argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const int nout = kind == NC_MODEL_INDEL ? 4 : 1;
    const int H = kind == NC_MODEL_INDEL ? 15 : 5;
    const int64_t xs = H * 128 * 2;
    NcTimer tm(ctx, 2);
    // batch = what the conv3 activations (fc1's input, 77 KB / 18 KB per site) may take in HBM: ~5 GB
    const int64_t BATCH = kind == NC_MODEL_INDEL ? 65536 : 262144;
    for (int64_t s0 = 0; s0 < n; s0 += BATCH) {
        const int64_t nb = n - s0 < BATCH ? n - s0 : BATCH;
        const float *tail = nullptr, *f1 = nullptr;
        NC_TRY(run_indel_trunk(ctx, ctx->w[kind], H, nb, x_dev + s0 * xs, &f1, &tail));
        hipLaunchKernelGGL(k_indel_heads, dim3(blocks_for(nb)), dim3(256), 0, ctx->stream, f1, tail, nout, nb, probs_dev + s0 * nout);
        NC_HIP(ctx, hipGetLastError());
    }
    tm.stop();
    return NC_OK;
}

}   // extern "C"

// Training of the diploid SNP model (gfx950): forward with stored activations, backward, TensorFlow-form Adam.  DESIGN.md section 17.
//
// The function is the deployed model's (model_architect.py:36-64, what nc_snp_forward computes for NC_MODEL_SNP): the four allele heads feed fc3 as
// softmax outputs, dropout sits behind fc1's SELU.  Everything is fp32 with fp32 accumulation; v_mfma_f32_16x16x4_f32 is bit for bit an fmaf chain.
// lane l of an MFMA: A[row l&15][k l>>4], B[k l>>4][col l&15], C/D col l&15, row 4*(l>>4)+r (the lane maps of nc_cnn_fp32.hip).
//
//   forward     k_scale_x, k_conv1_fwd, k_conv23_fwd x 2 (k7_conv23_mfma's form; nc_train.h), k_fc1_fwd (k3_fc1<48, 1>'s form), k_heads
//   backward    k_heads (losses -> d fc1, one site per lane), k_small_wgrad (fc1 bias + the layers behind fc1),
//               k_fc1_wgrad / k_fc1_dgrad, k_conv_wgrad / k_conv_dgrad x 2, k_bias_grad x 2, k_conv1_wgrad (all MFMA but the bias sums)
//   parameters  k_loss_reduce (the six loss terms), k_params (slab sum + gamma w on kernel entries + Adam step; nc_train_snp.h)
//
// Sums over sites run in a fixed order: a slab = the gradient of SLAB = 64 consecutive sites in blob order, written by one workgroup per
// parameter range (the four waves of a workgroup combine through LDS in wave order); k_params adds the slabs in slab order.  No atomics.
// Sites past n are never read: their operands enter every product as zeros.
// The trunk's kernels (conv1 - fc1 and their gradients), k_params, SLAB, the trunk's blob offsets and the host side of a handle (snp_train<unit>)
// are in nc_train_snp.h, shared with nc_train_hap.hip; here are the kernels behind fc1 and the unit that names this blob.
#include "nc_train_snp.h"

namespace {

constexpr int NPAR = 109370;
// canonical blob offsets behind the trunk (weights.LAYER_SPECS[KIND_SNP]: kernel then bias of every layer)
constexpr int O_FA = O_TRUNK_END, O_FAB = 108208, O_HEAD = 108224, O_FC2 = 108368, O_FC2B = 109136;
constexpr int O_FC3 = 109152, O_FC3B = 109344, O_GT = 109352, O_GTB = 109368;
// per-site record of the layers behind fc1: activations [f1 masked 48 | fa 16 | head logits 8 | head softmax 8 | fc2 16 | fc3 8] ...
constexpr int TA = 104, TA_FA = 48, TA_Z = 64, TA_P = 72, TA_FC2 = 80, TA_FC3 = 96;
// ... and gradients at the pre-activations [fa 16 | head logits 8 | fc2 16 | fc3 8 | GT logits 2 | pad 2]
constexpr int TD = 52, TD_H = 16, TD_FC2 = 24, TD_FC3 = 40, TD_GT = 48;

__device__ __forceinline__ bool is_bias(int i)
{
    if (i < O_FA) return trunk_is_bias(i);
    if (i < O_FAB) return false;
    if (i < O_HEAD) return true;
    if (i < O_FC2) return (i - O_HEAD) % 36 >= 34;
    if (i < O_FC3) return i >= O_FC2B;
    return (i >= O_FC3B && i < O_GT) || i >= O_GTB;
}

// softmax of a pair of logits; returns log(exp z0 + exp z1)
__device__ __forceinline__ float softmax2(float z0, float z1, float &p0, float &p1)
{
    const float m = fmaxf(z0, z1), e0 = expf(z0 - m), e1 = expf(z1 - m), sum = e0 + e1;
    p0 = e0 / sum;
    p1 = e1 / sum;
    return m + logf(sum);
}

// Everything behind fc1 of one site per lane: dropout, fa, the four heads, fc2, fc3, GT (model_architect.py:53-62); with labels also the five
// cross-entropies and the chain back to fc1's pre-activation: softmax Jacobians of the heads into fc3, the mask, SELU' (f1d: fc1's).  inv_n = 1 / batch.
__global__ __launch_bounds__(64) void k_heads(const float *__restrict__ f1, const float *__restrict__ f1d, const float *__restrict__ w, const int32_t *__restrict__ ref_code,
                                              const uint8_t *__restrict__ mask, float inv_keep, const uint8_t *__restrict__ label, float inv_n, int64_t n,
                                              float *__restrict__ probs, float *__restrict__ gt, float *__restrict__ tact, float *__restrict__ tdel,
                                              float *__restrict__ df1, float *__restrict__ loss)
{
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    float f1m[48], fa[16], in17[17], z[8], p[8], fc2[16], in24[24], fc3[8], g[2], pg[2], fad[16], fc2d[16], fc3d[8];
#pragma unroll
    for (int i = 0; i < 48; i++) f1m[i] = mask ? f1[s * 48 + i] * (mask[s * 48 + i] ? inv_keep : 0.0f) : f1[s * 48 + i];
    dense<48, 16>(f1m, w + O_FA, w + O_FAB, fa, true, fad);
#pragma unroll
    for (int i = 0; i < 16; i++) in17[i] = fa[i];
    const int rc = ref_code[s];
    float lse[5];
#pragma unroll
    for (int h = 0; h < 4; h++) {
        in17[16] = rc == h ? 1.0f : 0.0f;
        float zz[2];
        dense<17, 2>(in17, w + O_HEAD + 36 * h, w + O_HEAD + 36 * h + 34, zz, false);
        z[2 * h] = zz[0];
        z[2 * h + 1] = zz[1];
        lse[h] = softmax2(zz[0], zz[1], p[2 * h], p[2 * h + 1]);
        if (probs) probs[s * 4 + h] = p[2 * h + 1];
    }
    dense<48, 16>(f1m, w + O_FC2, w + O_FC2B, fc2, true, fc2d);
#pragma unroll
    for (int i = 0; i < 16; i++) in24[i] = fc2[i];
#pragma unroll
    for (int i = 0; i < 8; i++) in24[16 + i] = p[i];
    dense<24, 8>(in24, w + O_FC3, w + O_FC3B, fc3, true, fc3d);
    dense<8, 2>(fc3, w + O_GT, w + O_GTB, g, false);
    lse[4] = softmax2(g[0], g[1], pg[0], pg[1]);
    if (gt) { gt[s * 2] = pg[0]; gt[s * 2 + 1] = pg[1]; }
    if (!label) return;
    float *ta = tact + s * TA;
#pragma unroll
    for (int i = 0; i < 48; i++) ta[i] = f1m[i];
#pragma unroll
    for (int i = 0; i < 16; i++) { ta[TA_FA + i] = fa[i]; ta[TA_FC2 + i] = fc2[i]; }
#pragma unroll
    for (int i = 0; i < 8; i++) { ta[TA_Z + i] = z[i]; ta[TA_P + i] = p[i]; ta[TA_FC3 + i] = fc3[i]; }

    float dz[8], dg[2], dfc3[8], din24[24], dfc2[16], dfa[16];
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const int lab = label[s * 5 + h] ? 1 : 0;
        loss[s * 5 + h] = lse[h] - (lab ? z[2 * h + 1] : z[2 * h]);
        dz[2 * h] = (p[2 * h] - (lab ? 0.0f : 1.0f)) * inv_n;
        dz[2 * h + 1] = (p[2 * h + 1] - (lab ? 1.0f : 0.0f)) * inv_n;
    }
    {
        const int lab = label[s * 5 + 4] ? 1 : 0;
        loss[s * 5 + 4] = lse[4] - (lab ? g[1] : g[0]);
        dg[0] = (pg[0] - (lab ? 0.0f : 1.0f)) * inv_n;
        dg[1] = (pg[1] - (lab ? 1.0f : 0.0f)) * inv_n;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) dfc3[i] = fmaf(w[O_GT + 2 * i], dg[0], w[O_GT + 2 * i + 1] * dg[1]) * fc3d[i];
#pragma unroll
    for (int i = 0; i < 24; i++) {
        float a = 0.0f;
#pragma unroll
        for (int o = 0; o < 8; o++) a = fmaf(w[O_FC3 + i * 8 + o], dfc3[o], a);
        din24[i] = a;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) dfc2[i] = din24[i] * fc2d[i];
#pragma unroll
    for (int h = 0; h < 4; h++) {                                       // the GT loss through the softmax of head h
        const float d0 = din24[16 + 2 * h], d1 = din24[17 + 2 * h], dot = fmaf(p[2 * h], d0, p[2 * h + 1] * d1);
        dz[2 * h] = fmaf(p[2 * h], d0 - dot, dz[2 * h]);
        dz[2 * h + 1] = fmaf(p[2 * h + 1], d1 - dot, dz[2 * h + 1]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        float a = 0.0f;
#pragma unroll
        for (int h = 0; h < 4; h++) {
            a = fmaf(w[O_HEAD + 36 * h + 2 * i], dz[2 * h], a);
            a = fmaf(w[O_HEAD + 36 * h + 2 * i + 1], dz[2 * h + 1], a);
        }
        dfa[i] = a * fad[i];
    }
    float *td = tdel + s * TD;
#pragma unroll
    for (int i = 0; i < 16; i++) { td[i] = dfa[i]; td[TD_FC2 + i] = dfc2[i]; }
#pragma unroll
    for (int i = 0; i < 8; i++) { td[TD_H + i] = dz[i]; td[TD_FC3 + i] = dfc3[i]; }
    td[TD_GT] = dg[0];
    td[TD_GT + 1] = dg[1];
#pragma unroll
    for (int i = 0; i < 48; i++) {
        float a = 0.0f;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            a = fmaf(w[O_FA + i * 16 + o], dfa[o], a);
            a = fmaf(w[O_FC2 + i * 16 + o], dfc2[o], a);
        }
        const float mk = mask ? (mask[s * 48 + i] ? inv_keep : 0.0f) : 1.0f;
        df1[s * 48 + i] = a * mk * f1d[s * 48 + i];
    }
}

// weight gradients of fc1's bias and of every layer behind fc1 (1978 parameters), one parameter per lane, the slab's sites in order
__global__ __launch_bounds__(256) void k_small_wgrad(const float *__restrict__ tact, const float *__restrict__ tdel, const float *__restrict__ df1,
                                                     const int32_t *__restrict__ ref_code, int64_t n, float *__restrict__ slabs)
{
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= 48 + NPAR - O_FA) return;
    const int gi = t < 48 ? O_BF + t : O_FA + (t - 48);
    // in: -1 the constant 1 (bias), -2 - h the reference one-hot of head h, else an offset in the activation record; del: an offset in
    // the gradient record, or -1 - o for d fc1
    int in = -1, del = 0;
    if (gi < O_FA) del = -1 - t;
    else if (gi < O_FAB) { in = (gi - O_FA) / 16; del = (gi - O_FA) % 16; }
    else if (gi < O_HEAD) del = gi - O_FAB;
    else if (gi < O_FC2) {
        const int h = (gi - O_HEAD) / 36, r = (gi - O_HEAD) % 36;
        if (r < 34) { in = r / 2 < 16 ? TA_FA + r / 2 : -2 - h; del = TD_H + 2 * h + r % 2; }
        else del = TD_H + 2 * h + (r - 34);
    }
    else if (gi < O_FC2B) { in = (gi - O_FC2) / 16; del = TD_FC2 + (gi - O_FC2) % 16; }
    else if (gi < O_FC3) del = TD_FC2 + gi - O_FC2B;
    else if (gi < O_FC3B) { const int i = (gi - O_FC3) / 8; in = i < 16 ? TA_FC2 + i : TA_P + i - 16; del = TD_FC3 + (gi - O_FC3) % 8; }
    else if (gi < O_GT) del = TD_FC3 + gi - O_FC3B;
    else if (gi < O_GTB) { in = TA_FC3 + (gi - O_GT) / 2; del = TD_GT + (gi - O_GT) % 2; }
    else del = TD_GT + gi - O_GTB;
    const int64_t s0 = (int64_t)blockIdx.x * SLAB, s1 = s0 + SLAB < n ? s0 + SLAB : n;
    float acc = 0.0f;
    for (int64_t s = s0; s < s1; s++) {
        const float d = del < 0 ? df1[s * 48 + (-1 - del)] : tdel[s * TD + del];
        const float a = in >= 0 ? tact[s * TA + in] : in == -1 ? 1.0f : (ref_code[s] == -2 - in ? 1.0f : 0.0f);
        acc = fmaf(a, d, acc);
    }
    slabs[(int64_t)blockIdx.x * NPAR + gi] = acc;
}

// the six loss terms [cost, GT, A, G, T, C]: batch means of the per-site cross-entropies and gamma * sum over kernel entries of w^2 / 2; one
// workgroup, strided partial sums combined by a fixed tree
__global__ __launch_bounds__(256) void k_loss_reduce(const float *__restrict__ loss, int64_t n, const float *__restrict__ w, float gamma, float *__restrict__ out6)
{
    __shared__ double red[6][256];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t s = threadIdx.x; s < n; s += 256)
#pragma unroll
        for (int j = 0; j < 5; j++) acc[j] += (double)loss[s * 5 + j];
    for (int i = threadIdx.x; i < NPAR; i += 256)
        if (!is_bias(i)) acc[5] += (double)w[i] * (double)w[i];
#pragma unroll
    for (int j = 0; j < 6; j++) red[j][threadIdx.x] = acc[j];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k)
#pragma unroll
            for (int j = 0; j < 6; j++) red[j][threadIdx.x] += red[j][threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double a = red[0][0] / (double)n, g = red[1][0] / (double)n, t = red[2][0] / (double)n, c = red[3][0] / (double)n, gt = red[4][0] / (double)n;
        out6[0] = (float)(a + g + t + c + gt + 0.5 * (double)gamma * red[5][0]);
        out6[1] = (float)gt;
        out6[2] = (float)a;
        out6[3] = (float)g;
        out6[4] = (float)t;
        out6[5] = (float)c;
    }
}

struct unit {
    static constexpr const char *NAME = "nc_train", *MODEL = "diploid SNP", *BAD_LABELS = nullptr;   // (a label is a bit: none is out of range)
    static constexpr int KIND = NC_MODEL_SNP, NPAR = ::NPAR, TA = ::TA, TD = ::TD, NSMALL = 48 + NPAR - O_FA, NLAB = 5, NLOSS = 6;
    __device__ static __forceinline__ bool is_bias(int i) { return ::is_bias(i); }
    static void heads(snp_train_state *tr, hipStream_t st, int64_t nb, const int32_t *ref_code, const uint8_t *mask, float inv_keep, const uint8_t *label,
                      float inv_n, float *probs, float *gt, float *loss)
    {
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, st, tr->f1, tr->f1d, tr->w, ref_code, mask, inv_keep, label, inv_n, nb, probs, gt,
                           tr->tact, tr->tdel, tr->df1, loss);
    }
    static void small_wgrad(snp_train_state *tr, hipStream_t st, unsigned ns, const int32_t *ref_code, int64_t nb)
    {
        hipLaunchKernelGGL(k_small_wgrad, dim3(ns, blocks_for(NSMALL)), dim3(256), 0, st, tr->tact, tr->tdel, tr->df1, ref_code, nb, tr->slabs);
    }
    static void loss_reduce(snp_train_state *tr, hipStream_t st, int64_t n, float gamma)
    {
        hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, st, tr->loss, n, tr->w, gamma, tr->lossv);
    }
};
using T = snp_train<unit>;

}   // namespace

struct nc_train : snp_train_state {};

extern "C" {

int nc_train_create(nc_ctx *ctx, int32_t kind, int64_t max_batch, nc_train **out) { return T::create(ctx, kind, max_batch, out); }
int nc_train_free(nc_train *tr) { return train_free(tr); }
int nc_train_set_weights(nc_train *tr, const float *blob_host, size_t n_floats) { return train_set_weights(tr, unit::NAME, NPAR, blob_host, n_floats); }
int nc_train_get_weights(nc_train *tr, float *blob_host, size_t n_floats) { return train_get_weights(tr, unit::NAME, NPAR, blob_host, n_floats); }

int nc_train_forward(nc_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                     float keep, float *probs_dev, float *gt_dev)
{
    return T::forward(tr, n, x_dev, ref_code_dev, scale_dev, keep_mask_dev, keep, probs_dev, gt_dev);
}

int nc_train_loss_grad(nc_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                       float keep, const uint8_t *label_dev, float gamma, float *loss6_host, float *grad_dev)
{
    return T::loss_grad(tr, n, x_dev, ref_code_dev, scale_dev, keep_mask_dev, keep, label_dev, gamma, loss6_host, grad_dev);
}

int nc_train_adam(nc_train *tr, float lr, float beta1, float beta2, float eps) { return T::adam(tr, lr, beta1, beta2, eps); }

int nc_train_info(nc_train *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    return train_info(tr, slice_sites, workspace_bytes, steps);
}

int nc_train_stage_ms(nc_train *tr, int32_t on, float *ms7) { return train_stage_ms(tr, on, ms7); }

}   // extern "C"

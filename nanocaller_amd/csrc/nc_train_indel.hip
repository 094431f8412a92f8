// Training of the diploid indel model (gfx950): forward with stored activations, backward, TensorFlow-form Adam.  DESIGN.md section 18.
//
// The function is the deployed model's (model_architect_indel.py:28-48, what nc_indel_forward computes for NC_MODEL_INDEL): dropout sits behind
// fc1's SELU, the loss is the 4-way softmax cross-entropy.  Everything is fp32 with fp32 accumulation; v_mfma_f32_16x16x4_f32 is bit for bit an
// fmaf chain.  The input is the pipeline's tensor [15][128][2] as it is.
//
//   forward     k_conv1_fwd (k2_conv1_x4's form), k_conv23_fwd x 2 (nc_train.h), k_fc1_fwd (k3_fc1's split-K form over 16 waves), k_heads
//   backward    k_heads (loss -> d fc1, one site per lane), k_small_wgrad (fc1 bias, fc2, fc3), k_fc1_wgrad / k_fc1_dgrad,
//               k_conv_wgrad / k_conv_dgrad / k_bias_grad x 2 (nc_train.h), k_conv1_wgrad (all MFMA but the bias sums)
//   parameters  k_wsq + k_loss_reduce (cost, CE), k_params (slab sum + gamma w on kernel entries + Adam step)
//
// Every kernel but k_heads, and the host side of a handle, are in nc_train_indel.h, shared with the haploid unit (nc_train_hap_indel.hip) and
// instantiated here for the blob of 15 rows and 4 classes: 634,420 parameters, 619,008 of them fc1's kernel.  How the sums over sites are
// ordered is said there.
#include "nc_train_indel.h"

namespace {

using B = indel_blob<15, 4>;
constexpr int NC = B::NC, TA = B::TA, TA_FC2 = B::TA_FC2, TD = B::TD, TD_Z = B::TD_Z, O_FC2 = B::O_FC2, O_FC2B = B::O_FC2B, O_FC3 = B::O_FC3, O_FC3B = B::O_FC3B;
static_assert(B::NPAR == 634420 && B::NF == 19344 && B::NSMALL == 924, "the diploid indel blob");

// Everything behind fc1 of one site per lane: dropout, fc2, fc3, softmax (model_architect_indel.py:42-48); with labels also the cross-entropy
// and the chain back to fc1's pre-activation: fc3, SELU' of fc2, fc2, the mask, SELU' of fc1 (f1d).  inv_n = 1 / batch.
__global__ __launch_bounds__(64) void k_heads(const float *__restrict__ f1, const float *__restrict__ f1d, const float *__restrict__ w,
                                              const uint8_t *__restrict__ mask, float inv_keep, const uint8_t *__restrict__ label, float inv_n, int64_t n,
                                              float *__restrict__ probs, float *__restrict__ tact, float *__restrict__ tdel, float *__restrict__ df1,
                                              float *__restrict__ loss)
{
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    float f1m[F1], fc2[F2], fc2d[F2], z[NC], p[NC];
#pragma unroll
    for (int i = 0; i < F1; i++) f1m[i] = mask ? f1[s * F1 + i] * (mask[s * F1 + i] ? inv_keep : 0.0f) : f1[s * F1 + i];
    dense<F1, F2>(f1m, w + O_FC2, w + O_FC2B, fc2);
#pragma unroll
    for (int i = 0; i < F2; i++) {
        fc2d[i] = selud_pre(fc2[i]);
        fc2[i] = selu_acc(fc2[i]);
    }
    dense<F2, NC>(fc2, w + O_FC3, w + O_FC3B, z);
    const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < NC; i++) { p[i] = expf(z[i] - m); sum += p[i]; }
#pragma unroll
    for (int i = 0; i < NC; i++) p[i] /= sum;
    if (probs) *reinterpret_cast<float4 *>(probs + s * NC) = make_float4(p[0], p[1], p[2], p[3]);
    if (!label) return;
    const int lab = label[s];
    float zl = 0.0f, dz[NC], dfc2[F2];
#pragma unroll
    for (int i = 0; i < NC; i++) {
        if (i == lab) zl = z[i];
        dz[i] = (p[i] - (i == lab ? 1.0f : 0.0f)) * inv_n;
    }
    loss[s] = (m + logf(sum)) - zl;
#pragma unroll
    for (int i = 0; i < F2; i++) {
        float a = 0.0f;
#pragma unroll
        for (int o = 0; o < NC; o++) a = fmaf(w[O_FC3 + i * NC + o], dz[o], a);
        dfc2[i] = a * fc2d[i];
    }
    float *ta = tact + s * TA, *td = tdel + s * TD;
#pragma unroll
    for (int i = 0; i < F1; i++) ta[i] = f1m[i];
#pragma unroll
    for (int i = 0; i < F2; i++) { ta[TA_FC2 + i] = fc2[i]; td[i] = dfc2[i]; }
#pragma unroll
    for (int i = 0; i < NC; i++) td[TD_Z + i] = dz[i];
#pragma unroll
    for (int i = 0; i < F1; i++) {
        float a = 0.0f;
#pragma unroll
        for (int o = 0; o < F2; o++) a = fmaf(w[O_FC2 + i * F2 + o], dfc2[o], a);
        const float mk = mask ? (mask[s * F1 + i] ? inv_keep : 0.0f) : 1.0f;
        df1[s * F1 + i] = a * mk * f1d[s * F1 + i];
    }
}

struct unit {
    using B = ::B;
    static constexpr const char *NAME = "nc_indel_train", *MODEL = "diploid indel", *BAD_LABELS = nullptr;   // (IndelTrainer looks at the labels on the host)
    static constexpr int KIND = NC_MODEL_INDEL;
    static constexpr int FCW_J = 4;                                    // 64 rows of fc1's weight gradient per workgroup: 303 workgroups
    static void heads(indel_train_state *tr, hipStream_t st, int64_t nb, const uint8_t *mask, float inv_keep, const uint8_t *label, float inv_n, float *probs,
                      float *loss)
    {
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, st, tr->f1, tr->f1d, tr->w, mask, inv_keep, label, inv_n, nb, probs, tr->tact, tr->tdel,
                           tr->df1, loss);
    }
};
using T = indel_train<unit>;

}   // namespace

struct nc_indel_train : indel_train_state {};

extern "C" {

int nc_indel_train_create(nc_ctx *ctx, int32_t kind, int64_t max_batch, int64_t slice_sites, nc_indel_train **out)
{
    return T::create(ctx, kind, max_batch, slice_sites, out);
}

int nc_indel_train_free(nc_indel_train *tr) { return train_free(tr); }
int nc_indel_train_set_weights(nc_indel_train *tr, const float *blob_host, size_t n_floats) { return train_set_weights(tr, unit::NAME, B::NPAR, blob_host, n_floats); }
int nc_indel_train_get_weights(nc_indel_train *tr, float *blob_host, size_t n_floats) { return train_get_weights(tr, unit::NAME, B::NPAR, blob_host, n_floats); }

int nc_indel_train_forward(nc_indel_train *tr, int64_t n, const float *x_dev, const uint8_t *keep_mask_dev, float keep, float *probs_dev)
{
    return T::forward(tr, n, x_dev, keep_mask_dev, keep, probs_dev);
}

int nc_indel_train_loss_grad(nc_indel_train *tr, int64_t n, const float *x_dev, const uint8_t *keep_mask_dev, float keep, const uint8_t *label_dev,
                             float gamma, float *loss2_host, float *grad_dev)
{
    return T::loss_grad(tr, n, x_dev, keep_mask_dev, keep, label_dev, gamma, loss2_host, grad_dev);
}

int nc_indel_train_adam(nc_indel_train *tr, float lr, float beta1, float beta2, float eps) { return T::adam(tr, lr, beta1, beta2, eps); }

int nc_indel_train_info(nc_indel_train *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    return train_info(tr, slice_sites, workspace_bytes, steps);
}

int nc_indel_train_stage_ms(nc_indel_train *tr, int32_t on, float *ms7) { return train_stage_ms(tr, on, ms7); }

}   // extern "C"

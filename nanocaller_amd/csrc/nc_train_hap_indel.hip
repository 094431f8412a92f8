// Training of the haploid indel model (gfx950): forward with stored activations, backward, TensorFlow-form Adam.  DESIGN.md section 19.
//
// The function is the deployed model's (model_architect_indels_haploid.py:29-48, what nc_indel_forward computes for NC_MODEL_INDEL_HAP): the
// diploid indel model's layers on one row group, [5][128][2] -> conv1 24 -> conv2 [4][63][32] -> conv3 [3][31][48] -> 4,464 -> fc1 32 (SELU,
// dropout behind it) -> fc2 24 (SELU) -> fc3 1 -> sigmoid: the probability that the site holds an indel.  The loss is the binary
// cross-entropy, taken from the logit.  fp32 throughout.
//
// Every kernel but k_heads, and the host side of a handle, are nc_train_indel.h's, instantiated for the blob of 5 rows and 1 output: 158,185
// parameters, 142,848 of them fc1's kernel; the sums over sites are ordered as said there.
#include "nc_train_indel.h"

namespace {

using B = indel_blob<5, 1>;
static_assert(B::NPAR == 158185 && B::NF == 4464 && B::NSMALL == 849 && B::P2 == 252 && B::P3 == 93, "the haploid indel blob");

// Everything behind fc1 of one site per lane: dropout, fc2, fc3, sigmoid; with labels also the binary cross-entropy softplus(z) - y z and the
// chain back to fc1's pre-activation: (p - y) / n, fc3, SELU' of fc2, fc2, the mask, SELU' of fc1 (f1d).  inv_n = 1 / batch.
// A label above 1 sets *bad and gives the site no loss and no gradient.
__global__ __launch_bounds__(64) void k_heads(const float *__restrict__ f1, const float *__restrict__ f1d, const float *__restrict__ w,
                                              const uint8_t *__restrict__ mask, float inv_keep, const uint8_t *__restrict__ label, float inv_n, int64_t n,
                                              float *__restrict__ probs, float *__restrict__ tact, float *__restrict__ tdel, float *__restrict__ df1,
                                              float *__restrict__ loss, float *__restrict__ bad)
{
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    float f1m[F1], fc2[F2], fc2d[F2], z1[1];
#pragma unroll
    for (int i = 0; i < F1; i++) f1m[i] = mask ? f1[s * F1 + i] * (mask[s * F1 + i] ? inv_keep : 0.0f) : f1[s * F1 + i];
    dense<F1, F2>(f1m, w + B::O_FC2, w + B::O_FC2B, fc2);
#pragma unroll
    for (int i = 0; i < F2; i++) {
        fc2d[i] = selud_pre(fc2[i]);
        fc2[i] = selu_acc(fc2[i]);
    }
    dense<F2, 1>(fc2, w + B::O_FC3, w + B::O_FC3B, z1);
    const float z = z1[0], e = expf(-fabsf(z)), p = z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
    if (probs) probs[s] = p;
    if (!label) return;
    const int lab = label[s];
    const bool lab_ok = lab < 2;
    if (!lab_ok) *bad = 1.0f;
    const float y = lab == 1 ? 1.0f : 0.0f;
    loss[s] = lab_ok ? (fmaxf(z, 0.0f) + log1pf(e)) - y * z : 0.0f;
    const float dz = lab_ok ? (p - y) * inv_n : 0.0f;
    float dfc2[F2];
#pragma unroll
    for (int i = 0; i < F2; i++) dfc2[i] = w[B::O_FC3 + i] * dz * fc2d[i];
    float *ta = tact + s * B::TA, *td = tdel + s * B::TD;
#pragma unroll
    for (int i = 0; i < F1; i++) ta[i] = f1m[i];
#pragma unroll
    for (int i = 0; i < F2; i++) { ta[B::TA_FC2 + i] = fc2[i]; td[i] = dfc2[i]; }
    td[B::TD_Z] = dz;
#pragma unroll
    for (int i = 0; i < F1; i++) {
        float a = 0.0f;
#pragma unroll
        for (int o = 0; o < F2; o++) a = fmaf(w[B::O_FC2 + i * F2 + o], dfc2[o], a);
        const float mk = mask ? (mask[s * F1 + i] ? inv_keep : 0.0f) : 1.0f;
        df1[s * F1 + i] = a * mk * f1d[s * F1 + i];
    }
}

struct unit {
    using B = ::B;
    static constexpr const char *NAME = "nc_hap_indel_train", *MODEL = "haploid indel", *BAD_LABELS = "0 .. 1";
    static constexpr int KIND = NC_MODEL_INDEL_HAP;
    static constexpr int FCW_J = 4;
    static void heads(indel_train_state *tr, hipStream_t st, int64_t nb, const uint8_t *mask, float inv_keep, const uint8_t *label, float inv_n, float *probs,
                      float *loss)
    {
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, st, tr->f1, tr->f1d, tr->w, mask, inv_keep, label, inv_n, nb, probs, tr->tact, tr->tdel,
                           tr->df1, loss, tr->loss2 + 2);
    }
};
using T = indel_train<unit>;

}   // namespace

struct nc_hap_indel_train : indel_train_state {};

extern "C" {

int nc_hap_indel_train_create(nc_ctx *ctx, int32_t kind, int64_t max_batch, int64_t slice_sites, nc_hap_indel_train **out)
{
    return T::create(ctx, kind, max_batch, slice_sites, out);
}

int nc_hap_indel_train_free(nc_hap_indel_train *tr) { return train_free(tr); }
int nc_hap_indel_train_set_weights(nc_hap_indel_train *tr, const float *blob_host, size_t n_floats) { return train_set_weights(tr, unit::NAME, B::NPAR, blob_host, n_floats); }
int nc_hap_indel_train_get_weights(nc_hap_indel_train *tr, float *blob_host, size_t n_floats) { return train_get_weights(tr, unit::NAME, B::NPAR, blob_host, n_floats); }

int nc_hap_indel_train_forward(nc_hap_indel_train *tr, int64_t n, const float *x_dev, const uint8_t *keep_mask_dev, float keep, float *probs_dev)
{
    return T::forward(tr, n, x_dev, keep_mask_dev, keep, probs_dev);
}

int nc_hap_indel_train_loss_grad(nc_hap_indel_train *tr, int64_t n, const float *x_dev, const uint8_t *keep_mask_dev, float keep, const uint8_t *label_dev,
                                 float gamma, float *loss2_host, float *grad_dev)
{
    return T::loss_grad(tr, n, x_dev, keep_mask_dev, keep, label_dev, gamma, loss2_host, grad_dev);
}

int nc_hap_indel_train_adam(nc_hap_indel_train *tr, float lr, float beta1, float beta2, float eps) { return T::adam(tr, lr, beta1, beta2, eps); }

int nc_hap_indel_train_info(nc_hap_indel_train *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    return train_info(tr, slice_sites, workspace_bytes, steps);
}

int nc_hap_indel_train_stage_ms(nc_hap_indel_train *tr, int32_t on, float *ms7) { return train_stage_ms(tr, on, ms7); }

}   // extern "C"

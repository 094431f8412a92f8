// Training of the haploid SNP model (gfx950): forward with stored activations, backward, TensorFlow-form Adam.  DESIGN.md section 19.
//
// The function is the deployed model's (model_architect_SNP_haploid.py:33-53, what nc_snp_forward computes for NC_MODEL_SNP_HAP): the diploid SNP
// model's trunk through fc1, dropout behind fc1's SELU, fc2 48 -> 16 with SELU, fc3 on concat(fc2, one-hot reference base) 20 -> 4 with SELU,
// softmax over the four SELU outputs.  The loss is the 4-way cross-entropy of the site's base (A0 G1 T2 C3).  fp32 throughout.
//
//   forward     the trunk of nc_train_snp.h (k_scale_x, k_conv1_fwd, k_conv23_fwd x 2, k_fc1_fwd), k_heads
//   backward    k_heads (loss -> d fc1, one site per lane; through fc3's SELU), k_small_wgrad (fc1's bias, fc2, fc3: 916 parameters),
//               the trunk's gradient kernels (nc_train_snp.h)
//   parameters  k_loss_reduce (cost, CE), k_params (slab sum + gamma w on kernel entries + Adam step; nc_train_snp.h)
//
// Sums over sites run in a fixed order, as in nc_train.hip: slabs of SLAB = 64 sites in blob order, one lane of one workgroup per parameter,
// waves combined through LDS in wave order, slabs and slices added in order.  No atomics.  Sites past n are never read.
// The host side of a handle is snp_train<unit> of nc_train_snp.h; here are the kernels behind fc1 and the unit that names this blob.
#include "nc_train_snp.h"

namespace {

constexpr int NPAR = 108308;
// canonical blob offsets behind the trunk (weights.LAYER_SPECS[KIND_SNP_HAP])
constexpr int O_FC2 = O_TRUNK_END, O_FC2B = 108208, O_FC3 = 108224, O_FC3B = 108304;
constexpr int NSMALL = 48 + NPAR - O_FC2;                  // fc1's bias + everything behind fc1
// per-site record of the layers behind fc1: activations [f1 masked 48 | fc2 16], gradients at the pre-activations [fc2 16 | fc3 4]
constexpr int TA = 64, TA_FC2 = 48, TD = 20, TD_FC3 = 16;

__device__ __forceinline__ bool is_bias(int i)
{
    if (i < O_FC2) return trunk_is_bias(i);
    if (i < O_FC3) return i >= O_FC2B;
    return i >= O_FC3B;
}

// Everything behind fc1 of one site per lane: dropout, fc2, fc3 on [fc2 | reference one-hot] with its SELU, softmax; with labels also the
// cross-entropy and the chain back to fc1's pre-activation: softmax, SELU' of fc3, fc3, SELU' of fc2, fc2, the mask, SELU' of fc1 (f1d).
// inv_n = 1 / batch.  A label outside 0..3 sets *bad and gives the site no loss and no gradient.
__global__ __launch_bounds__(64) void k_heads(const float *__restrict__ f1, const float *__restrict__ f1d, const float *__restrict__ w, const int32_t *__restrict__ ref_code,
                                              const uint8_t *__restrict__ mask, float inv_keep, const uint8_t *__restrict__ label, float inv_n, int64_t n,
                                              float *__restrict__ probs, float *__restrict__ tact, float *__restrict__ tdel, float *__restrict__ df1,
                                              float *__restrict__ loss, float *__restrict__ bad)
{
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    float f1m[48], fc2[16], fc2d[16], in20[20], a[4], ad[4], p[4];
#pragma unroll
    for (int i = 0; i < 48; i++) f1m[i] = mask ? f1[s * 48 + i] * (mask[s * 48 + i] ? inv_keep : 0.0f) : f1[s * 48 + i];
    dense<48, 16>(f1m, w + O_FC2, w + O_FC2B, fc2, true, fc2d);
    const int rc = ref_code[s];
#pragma unroll
    for (int i = 0; i < 16; i++) in20[i] = fc2[i];
#pragma unroll
    for (int i = 0; i < 4; i++) in20[16 + i] = rc == i ? 1.0f : 0.0f;
    dense<20, 4>(in20, w + O_FC3, w + O_FC3B, a, true, ad);
    const float m = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) { p[i] = expf(a[i] - m); sum += p[i]; }
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] /= sum;
    if (probs) *reinterpret_cast<float4 *>(probs + s * 4) = make_float4(p[0], p[1], p[2], p[3]);
    if (!label) return;
    const int lab = label[s];
    const bool lab_ok = lab < 4;
    if (!lab_ok) *bad = 1.0f;
    float al = 0.0f, dz[4], dfc2[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i == lab) al = a[i];
        dz[i] = lab_ok ? (p[i] - (i == lab ? 1.0f : 0.0f)) * inv_n * ad[i] : 0.0f;
    }
    loss[s] = lab_ok ? (m + logf(sum)) - al : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        float g = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; o++) g = fmaf(w[O_FC3 + i * 4 + o], dz[o], g);
        dfc2[i] = g * fc2d[i];
    }
    float *ta = tact + s * TA, *td = tdel + s * TD;
#pragma unroll
    for (int i = 0; i < 48; i++) ta[i] = f1m[i];
#pragma unroll
    for (int i = 0; i < 16; i++) { ta[TA_FC2 + i] = fc2[i]; td[i] = dfc2[i]; }
#pragma unroll
    for (int i = 0; i < 4; i++) td[TD_FC3 + i] = dz[i];
#pragma unroll
    for (int i = 0; i < 48; i++) {
        float g = 0.0f;
#pragma unroll
        for (int o = 0; o < 16; o++) g = fmaf(w[O_FC2 + i * 16 + o], dfc2[o], g);
        const float mk = mask ? (mask[s * 48 + i] ? inv_keep : 0.0f) : 1.0f;
        df1[s * 48 + i] = g * mk * f1d[s * 48 + i];
    }
}

// weight gradients of fc1's bias and of fc2, fc3 with their biases (916 parameters), one parameter per lane, the slab's sites in order
__global__ __launch_bounds__(256) void k_small_wgrad(const float *__restrict__ tact, const float *__restrict__ tdel, const float *__restrict__ df1,
                                                     const int32_t *__restrict__ ref_code, int64_t n, float *__restrict__ slabs)
{
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= NSMALL) return;
    const int gi = t < 48 ? O_BF + t : O_FC2 + (t - 48);
    // in: -1 the constant 1 (bias), -2 - b the reference one-hot of base b, else an offset in the activation record; del: an offset in the
    // gradient record, or -1 - o for d fc1
    int in = -1, del = 0;
    if (gi < O_FC2) del = -1 - t;
    else if (gi < O_FC2B) { in = (gi - O_FC2) / 16; del = (gi - O_FC2) % 16; }
    else if (gi < O_FC3) del = gi - O_FC2B;
    else if (gi < O_FC3B) { const int i = (gi - O_FC3) / 4; in = i < 16 ? TA_FC2 + i : -2 - (i - 16); del = TD_FC3 + (gi - O_FC3) % 4; }
    else del = TD_FC3 + gi - O_FC3B;
    const int64_t s0 = (int64_t)blockIdx.x * SLAB, s1 = s0 + SLAB < n ? s0 + SLAB : n;
    float acc = 0.0f;
    for (int64_t s = s0; s < s1; s++) {
        const float d = del < 0 ? df1[s * 48 + (-1 - del)] : tdel[s * TD + del];
        const float a = in >= 0 ? tact[s * TA + in] : in == -1 ? 1.0f : (ref_code[s] == -2 - in ? 1.0f : 0.0f);
        acc = fmaf(a, d, acc);
    }
    slabs[(int64_t)blockIdx.x * NPAR + gi] = acc;
}

// the two loss terms [cost, CE] (out2[2], the bad-label flag, is k_heads' to write): the batch mean of the per-site cross-entropies and
// gamma * sum over kernel entries of w^2 / 2; one workgroup, strided partial sums combined by a fixed tree
__global__ __launch_bounds__(256) void k_loss_reduce(const float *__restrict__ loss, int64_t n, const float *__restrict__ w, float gamma, float *__restrict__ out2)
{
    __shared__ double red[2][256];
    double ce = 0.0, ww = 0.0;
    for (int64_t s = threadIdx.x; s < n; s += 256) ce += (double)loss[s];
    for (int i = threadIdx.x; i < NPAR; i += 256)
        if (!is_bias(i)) ww += (double)w[i] * (double)w[i];
    red[0][threadIdx.x] = ce;
    red[1][threadIdx.x] = ww;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
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

struct unit {
    static constexpr const char *NAME = "nc_hap_train", *MODEL = "haploid SNP", *BAD_LABELS = "0 .. 3 (A0 G1 T2 C3)";
    static constexpr int KIND = NC_MODEL_SNP_HAP, NPAR = ::NPAR, TA = ::TA, TD = ::TD, NSMALL = ::NSMALL, NLAB = 1, NLOSS = 2;
    __device__ static __forceinline__ bool is_bias(int i) { return ::is_bias(i); }
    static void heads(snp_train_state *tr, hipStream_t st, int64_t nb, const int32_t *ref_code, const uint8_t *mask, float inv_keep, const uint8_t *label,
                      float inv_n, float *probs, float *, float *loss)
    {
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, st, tr->f1, tr->f1d, tr->w, ref_code, mask, inv_keep, label, inv_n, nb, probs, tr->tact,
                           tr->tdel, tr->df1, loss, tr->lossv + NLOSS);
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

struct nc_hap_train : snp_train_state {};

extern "C" {

int nc_hap_train_create(nc_ctx *ctx, int32_t kind, int64_t max_batch, nc_hap_train **out) { return T::create(ctx, kind, max_batch, out); }
int nc_hap_train_free(nc_hap_train *tr) { return train_free(tr); }
int nc_hap_train_set_weights(nc_hap_train *tr, const float *blob_host, size_t n_floats) { return train_set_weights(tr, unit::NAME, NPAR, blob_host, n_floats); }
int nc_hap_train_get_weights(nc_hap_train *tr, float *blob_host, size_t n_floats) { return train_get_weights(tr, unit::NAME, NPAR, blob_host, n_floats); }

int nc_hap_train_forward(nc_hap_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                         float keep, float *probs_dev)
{
    return T::forward(tr, n, x_dev, ref_code_dev, scale_dev, keep_mask_dev, keep, probs_dev, nullptr);
}

int nc_hap_train_loss_grad(nc_hap_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                           float keep, const uint8_t *label_dev, float gamma, float *loss2_host, float *grad_dev)
{
    return T::loss_grad(tr, n, x_dev, ref_code_dev, scale_dev, keep_mask_dev, keep, label_dev, gamma, loss2_host, grad_dev);
}

int nc_hap_train_adam(nc_hap_train *tr, float lr, float beta1, float beta2, float eps) { return T::adam(tr, lr, beta1, beta2, eps); }

int nc_hap_train_info(nc_hap_train *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    return train_info(tr, slice_sites, workspace_bytes, steps);
}

int nc_hap_train_stage_ms(nc_hap_train *tr, int32_t on, float *ms7) { return train_stage_ms(tr, on, ms7); }

}   // extern "C"

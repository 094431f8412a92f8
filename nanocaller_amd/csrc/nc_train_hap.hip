// Training of the haploid SNP model (gfx950): forward with stored activations, backward, TensorFlow-form Adam.  DESIGN.md section 19.
//
// The function is the deployed model's (model_architect_SNP_haploid.py:33-53, what nc_snp_forward computes for NC_MODEL_SNP_HAP): the diploid SNP
// model's trunk through fc1, dropout behind fc1's SELU, fc2 48 -> 16 with SELU, fc3 on concat(fc2, one-hot reference base) 20 -> 4 with SELU,
// softmax over the four SELU outputs.  The loss is the 4-way cross-entropy of the site's base (A0 G1 T2 C3).  fp32 throughout.
//
//   forward     the trunk of nc_train_snp.h (k_scale_x, k_conv1_fwd, k_conv23_fwd x 2, k_fc1_fwd), k_heads
//   backward    k_heads (loss -> d fc1, one site per lane; through fc3's SELU), k_small_wgrad (fc1's bias, fc2, fc3: 916 parameters),
//               the trunk's gradient kernels (snp_trunk_backward)
//   parameters  k_loss_reduce (cost, CE), k_params (slab sum + gamma w on kernel entries + Adam step)
//
// Sums over sites run in a fixed order, as in nc_train.hip: slabs of SLAB = 64 sites in blob order, one lane of one workgroup per parameter,
// waves combined through LDS in wave order, slabs and slices added in order.  No atomics.  Sites past n are never read.
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

// One parameter per lane, k_params of nc_train.hip for this blob: gradient = g_in (earlier slices, may be NULL) + the slabs in slab order
// (+ gamma w on kernel entries with `reg`); written to g_out (may be NULL); with `step` the Adam update in TensorFlow's form.
__global__ __launch_bounds__(256) void k_params(const float *__restrict__ g_in, const float *__restrict__ slabs, int ns, int reg, float gamma,
                                                float *__restrict__ g_out, int step, float *__restrict__ w, float *__restrict__ m, float *__restrict__ v,
                                                float lr_t, float b1, float b2, float eps)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NPAR) return;
    float g = g_in ? g_in[i] : 0.0f;
    for (int k = 0; k < ns; k++) g += slabs[(int64_t)k * NPAR + i];
    const float wi = w[i];
    if (reg && !is_bias(i)) g = fmaf(gamma, wi, g);
    if (g_out) g_out[i] = g;
    if (step) {
        const float mi = fmaf(b1, m[i], (1.0f - b1) * g), vi = fmaf(b2, v[i], (1.0f - b2) * g * g);
        m[i] = mi;
        v[i] = vi;
        w[i] = wi - lr_t * mi / (sqrtf(vi) + eps);
    }
}

}   // namespace

enum { TS_FWD = 0, TS_HEADS, TS_FC1, TS_CONV3, TS_CONV2, TS_CONV1, TS_PARAMS, TS_N };

struct nc_hap_train {
    nc_ctx *ctx = nullptr;
    int64_t max_batch = 0, slice = 0;
    size_t ws_bytes = 0;
    float *w = nullptr, *m = nullptr, *v = nullptr, *g = nullptr;      // fp32 state in blob order
    float *ws = nullptr;                                               // one allocation: the buffers below
    float *xs, *a1, *a2, *a3, *f1, *f1d, *tact, *tdel, *df1, *d1, *d2, *d3, *slabs, *loss, *loss2;   // loss2: cost, CE, bad-label flag
    int64_t t = 0;                                                     // Adam steps taken
    // the gradient of the last nc_hap_train_loss_grad = (partial ? g : 0) + the pending slabs + gamma w: summed by nc_hap_train_adam's own kernel
    bool have_grad = false, partial = false;
    int pending_ns = 0;
    float pending_gamma = 0.0f;
    int timing = 0;
    hipEvent_t ev[TS_N + 1] = {nullptr};
};

namespace {

void mark(nc_hap_train *tr, int i)
{
    if (tr->timing) (void)hipEventRecord(tr->ev[i], tr->ctx->stream);
}

int check_call(nc_hap_train *tr, const char *what, int64_t n, const void *x, const void *rc, float keep)
{
    if (!tr) return NC_ERR_ARG;
    if (n < 1 || n > tr->max_batch) return nc_fail(tr->ctx, NC_ERR_ARG, "%s: n = %lld outside 1 .. max_batch = %lld", what, (long long)n, (long long)tr->max_batch);
    if (!x || !rc) return nc_fail(tr->ctx, NC_ERR_ARG, "%s: null argument", what);
    if (!(keep > 0.0f && keep <= 1.0f)) return nc_fail(tr->ctx, NC_ERR_ARG, "%s: keep = %g outside (0, 1]", what, (double)keep);
    return NC_OK;
}

snp_trunk_ws trunk_of(nc_hap_train *tr)
{
    return {tr->w, tr->xs, tr->a1, tr->a2, tr->a3, tr->f1, tr->f1d, tr->df1, tr->d1, tr->d2, tr->d3, tr->slabs};
}

}   // namespace

extern "C" {

int nc_hap_train_create(nc_ctx *ctx, int32_t kind, int64_t max_batch, nc_hap_train **out)
{
    if (!ctx || !out) return NC_ERR_ARG;
    *out = nullptr;
    if (kind != NC_MODEL_SNP_HAP)
        return nc_fail(ctx, NC_ERR_UNSUPPORTED, "nc_hap_train_create: only the haploid SNP model (kind %d) is trained here, not kind %d", NC_MODEL_SNP_HAP, kind);
    if (max_batch < 1) return nc_fail(ctx, NC_ERR_ARG, "nc_hap_train_create: max_batch");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    nc_hap_train *tr = new nc_hap_train;
    tr->ctx = ctx;
    tr->max_batch = max_batch;
    tr->slice = max_batch < MAX_SLICE ? max_batch : MAX_SLICE;
    const size_t sl = (size_t)tr->slice, ns = (sl + SLAB - 1) / SLAB;
    size_t sizes[] = {sl * XS, sl * N1, sl * N2, sl * N3, sl * 48, sl * 48, sl * TA, sl * TD, sl * 48, sl * N1, sl * N2, sl * N3, ns * NPAR, (size_t)max_batch, 8};
    float **ptrs[] = {&tr->xs, &tr->a1, &tr->a2, &tr->a3, &tr->f1, &tr->f1d, &tr->tact, &tr->tdel, &tr->df1, &tr->d1, &tr->d2, &tr->d3, &tr->slabs, &tr->loss, &tr->loss2};
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~size_t(63);
    tr->ws_bytes = total * 4;
    hipError_t e = hipMalloc((void **)&tr->ws, tr->ws_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->w, (size_t)NPAR * 4 * 4);
    if (e != hipSuccess) {
        if (tr->ws) (void)hipFree(tr->ws);
        delete tr;
        return nc_fail(ctx, NC_ERR_NOMEM, "nc_hap_train_create: hipMalloc of %zu bytes: %s", total * 4, hipGetErrorString(e));
    }
    tr->m = tr->w + NPAR;
    tr->v = tr->m + NPAR;
    tr->g = tr->v + NPAR;
    size_t off = 0;
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++) {
        *ptrs[i] = tr->ws + off;
        off += (sizes[i] + 63) & ~size_t(63);
    }
    e = hipMemsetAsync(tr->w, 0, (size_t)NPAR * 4 * 4, ctx->stream);
    for (int i = 0; i <= TS_N && e == hipSuccess; i++) e = hipEventCreate(&tr->ev[i]);
    if (e != hipSuccess) {
        (void)nc_hap_train_free(tr);                                    // (frees what exists: the two allocations and the events made so far)
        return nc_fail(ctx, NC_ERR_HIP, "nc_hap_train_create: %s", hipGetErrorString(e));
    }
    *out = tr;
    return NC_OK;
}

int nc_hap_train_free(nc_hap_train *tr)
{
    if (!tr) return NC_OK;
    (void)hipSetDevice(tr->ctx->device);
    (void)hipStreamSynchronize(tr->ctx->stream);
    for (int i = 0; i <= TS_N; i++)
        if (tr->ev[i]) (void)hipEventDestroy(tr->ev[i]);
    if (tr->ws) (void)hipFree(tr->ws);
    if (tr->w) (void)hipFree(tr->w);
    delete tr;
    return NC_OK;
}

int nc_hap_train_set_weights(nc_hap_train *tr, const float *blob_host, size_t n_floats)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!blob_host || n_floats != (size_t)NPAR) return nc_fail(ctx, NC_ERR_ARG, "nc_hap_train_set_weights: expects %d floats", NPAR);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemcpyAsync(tr->w, blob_host, (size_t)NPAR * 4, hipMemcpyHostToDevice, ctx->stream));
    NC_HIP(ctx, hipMemsetAsync(tr->m, 0, (size_t)NPAR * 4 * 3, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tr->t = 0;
    tr->have_grad = false;
    return NC_OK;
}

int nc_hap_train_get_weights(nc_hap_train *tr, float *blob_host, size_t n_floats)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!blob_host || n_floats != (size_t)NPAR) return nc_fail(ctx, NC_ERR_ARG, "nc_hap_train_get_weights: expects %d floats", NPAR);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemcpyAsync(blob_host, tr->w, (size_t)NPAR * 4, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

int nc_hap_train_forward(nc_hap_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                         float keep, float *probs_dev)
{
    NC_TRY(check_call(tr, "nc_hap_train_forward", n, x_dev, ref_code_dev, keep));
    nc_ctx *ctx = tr->ctx;
    if (!probs_dev) return nc_fail(ctx, NC_ERR_ARG, "nc_hap_train_forward: null argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    if (keep == 1.0f) keep_mask_dev = nullptr;
    for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
        const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
        snp_trunk_forward(trunk_of(tr), ctx->stream, nb, x_dev + s0 * NC_SNP_TENSOR, scale_dev ? scale_dev + s0 : nullptr);
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, ctx->stream, tr->f1, tr->f1d, tr->w, ref_code_dev + s0,
                           keep_mask_dev ? keep_mask_dev + s0 * 48 : nullptr, 1.0f / keep, (const uint8_t *)nullptr, 0.0f, nb, probs_dev + s0 * 4, tr->tact,
                           tr->tdel, tr->df1, tr->loss, tr->loss2 + 2);
    }
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_hap_train_loss_grad(nc_hap_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                           float keep, const uint8_t *label_dev, float gamma, float *loss2_host, float *grad_dev)
{
    NC_TRY(check_call(tr, "nc_hap_train_loss_grad", n, x_dev, ref_code_dev, keep));
    nc_ctx *ctx = tr->ctx;
    if (!label_dev) return nc_fail(ctx, NC_ERR_ARG, "nc_hap_train_loss_grad: null argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (keep == 1.0f) keep_mask_dev = nullptr;
    tr->have_grad = tr->partial = false;
    NC_HIP(ctx, hipMemsetAsync(tr->loss2, 0, 8 * 4, st));
    for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
        const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
        const unsigned ns = (unsigned)((nb + SLAB - 1) / SLAB);
        const float *x = x_dev + s0 * NC_SNP_TENSOR;
        mark(tr, TS_FWD);
        snp_trunk_forward(trunk_of(tr), st, nb, x, scale_dev ? scale_dev + s0 : nullptr);
        mark(tr, TS_HEADS);
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, st, tr->f1, tr->f1d, tr->w, ref_code_dev + s0,
                           keep_mask_dev ? keep_mask_dev + s0 * 48 : nullptr, 1.0f / keep, label_dev + s0, 1.0f / (float)n, nb, (float *)nullptr, tr->tact,
                           tr->tdel, tr->df1, tr->loss + s0, tr->loss2 + 2);
        hipLaunchKernelGGL(k_small_wgrad, dim3(ns, blocks_for(NSMALL)), dim3(256), 0, st, tr->tact, tr->tdel, tr->df1, ref_code_dev + s0, nb, tr->slabs);
        snp_trunk_backward<NPAR>(trunk_of(tr), st, nb, scale_dev ? tr->xs : x, scale_dev ? XS : 1025, [&](int i) { mark(tr, TS_FC1 + i); });
        mark(tr, TS_PARAMS);
        if (s0 + nb < n) {                                              // not the last slice: fold its slabs into g, the workspace is reused
            hipLaunchKernelGGL(k_params, dim3(blocks_for(NPAR)), dim3(256), 0, st, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, (int)ns, 0, 0.0f,
                               tr->g, 0, tr->w, tr->m, tr->v, 0.0f, 0.0f, 0.0f, 0.0f);
            tr->partial = true;
        } else {
            tr->pending_ns = (int)ns;
            tr->pending_gamma = gamma;
        }
    }
    if (grad_dev)
        hipLaunchKernelGGL(k_params, dim3(blocks_for(NPAR)), dim3(256), 0, st, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, tr->pending_ns, 1, gamma,
                           grad_dev, 0, tr->w, tr->m, tr->v, 0.0f, 0.0f, 0.0f, 0.0f);
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, st, tr->loss, n, tr->w, gamma, tr->loss2);
    mark(tr, TS_N);
    NC_HIP(ctx, hipGetLastError());
    // the labels are on the device: the flag k_heads sets comes back with the losses, so this call always waits
    float l3[3] = {0.0f, 0.0f, 0.0f};
    NC_HIP(ctx, hipMemcpyAsync(l3, tr->loss2, 3 * 4, hipMemcpyDeviceToHost, st));
    NC_HIP(ctx, hipStreamSynchronize(st));
    if (l3[2] != 0.0f) return nc_fail(ctx, NC_ERR_ARG, "nc_hap_train_loss_grad: a label outside 0 .. 3 (A0 G1 T2 C3)");
    tr->have_grad = true;
    if (loss2_host) {
        loss2_host[0] = l3[0];
        loss2_host[1] = l3[1];
    }
    return NC_OK;
}

int nc_hap_train_adam(nc_hap_train *tr, float lr, float beta1, float beta2, float eps)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!tr->have_grad) return nc_fail(ctx, NC_ERR_STATE, "nc_hap_train_adam: no gradient (nc_hap_train_loss_grad comes first, once per step)");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    tr->t++;
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)tr->t)) / (1.0 - std::pow((double)beta1, (double)tr->t)));
    hipLaunchKernelGGL(k_params, dim3(blocks_for(NPAR)), dim3(256), 0, ctx->stream, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, tr->pending_ns, 1,
                       tr->pending_gamma, (float *)nullptr, 1, tr->w, tr->m, tr->v, lr_t, beta1, beta2, eps);
    NC_HIP(ctx, hipGetLastError());
    tr->have_grad = false;
    return NC_OK;
}

int nc_hap_train_info(nc_hap_train *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    if (!tr) return NC_ERR_ARG;
    if (slice_sites) *slice_sites = tr->slice;
    if (workspace_bytes) *workspace_bytes = (int64_t)tr->ws_bytes;
    if (steps) *steps = tr->t;
    return NC_OK;
}

int nc_hap_train_stage_ms(nc_hap_train *tr, int32_t on, float *ms7)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (ms7 && tr->timing) {
        NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < TS_N; i++) {
            ms7[i] = 0.0f;
            NC_HIP(ctx, hipEventElapsedTime(&ms7[i], tr->ev[i], tr->ev[i + 1]));
        }
    }
    tr->timing = on;
    return NC_OK;
}

}   // extern "C"

// Training of the diploid SNP model (gfx950): forward with stored activations, backward, TensorFlow-form Adam.  DESIGN.md section 17.
//
// The function is the deployed model's (model_architect.py:36-64, what nc_snp_forward computes for NC_MODEL_SNP): the four allele heads feed fc3 as
// softmax outputs, dropout sits behind fc1's SELU.  Everything is fp32 with fp32 accumulation; v_mfma_f32_16x16x4_f32 is bit for bit an fmaf chain.
// lane l of an MFMA: A[row l&15][k l>>4], B[k l>>4][col l&15], C/D col l&15, row 4*(l>>4)+r (the lane maps of nc_cnn_fp32.hip).
//
//   forward     k_scale_x, k_conv1_fwd, k_conv23_fwd x 2 (k7_conv23_mfma's form; nc_train.h), k_fc1_fwd (k3_fc1<48, 1>'s form), k_heads
//   backward    k_heads (losses -> d fc1, one site per lane), k_small_wgrad (fc1 bias + the layers behind fc1),
//               k_fc1_wgrad / k_fc1_dgrad, k_conv_wgrad / k_conv_dgrad x 2, k_bias_grad x 2, k_conv1_wgrad (all MFMA but the bias sums)
//   parameters  k_loss_reduce (the six loss terms), k_params (slab sum + gamma w on kernel entries + Adam step)
//
// Sums over sites run in a fixed order: a slab = the gradient of SLAB = 64 consecutive sites in blob order, written by one workgroup per
// parameter range (the four waves of a workgroup combine through LDS in wave order); k_params adds the slabs in slab order.  No atomics.
// Sites past n are never read: their operands enter every product as zeros.
// The trunk's kernels (conv1 - fc1 and their gradients), SLAB and the trunk's blob offsets are in nc_train_snp.h, shared with nc_train_hap.hip.
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

// One parameter per lane: gradient = g_in (earlier slices, may be NULL) + the slabs in slab order (+ gamma w on kernel entries with `reg`);
// written to g_out (may be NULL); with `step` the Adam update in TensorFlow's form, w -= lr_t m / (sqrt(v) + eps).
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

struct nc_train {
    nc_ctx *ctx = nullptr;
    int64_t max_batch = 0, slice = 0;
    size_t ws_bytes = 0;
    float *w = nullptr, *m = nullptr, *v = nullptr, *g = nullptr;      // fp32 state in blob order
    float *ws = nullptr;                                               // one allocation: the buffers below
    float *xs, *a1, *a2, *a3, *f1, *f1d, *tact, *tdel, *df1, *d1, *d2, *d3, *slabs, *loss, *loss6;
    int64_t t = 0;                                                     // Adam steps taken
    // the gradient of the last nc_train_loss_grad = (partial ? g : 0) + the pending slabs + gamma w: summed by nc_train_adam's own kernel
    bool have_grad = false, partial = false;
    int pending_ns = 0;
    float pending_gamma = 0.0f;
    int timing = 0;
    hipEvent_t ev[TS_N + 1] = {nullptr};
    float stage_ms[TS_N] = {0};
};

namespace {

void mark(nc_train *tr, int i)
{
    if (tr->timing) (void)hipEventRecord(tr->ev[i], tr->ctx->stream);
}

int check_call(nc_train *tr, const char *what, int64_t n, const void *x, const void *rc)
{
    if (!tr) return NC_ERR_ARG;
    if (n < 1 || n > tr->max_batch) return nc_fail(tr->ctx, NC_ERR_ARG, "%s: n = %lld outside 1 .. max_batch = %lld", what, (long long)n, (long long)tr->max_batch);
    if (!x || !rc) return nc_fail(tr->ctx, NC_ERR_ARG, "%s: null argument", what);
    return NC_OK;
}

snp_trunk_ws trunk_of(nc_train *tr)
{
    return {tr->w, tr->xs, tr->a1, tr->a2, tr->a3, tr->f1, tr->f1d, tr->df1, tr->d1, tr->d2, tr->d3, tr->slabs};
}

// conv1 - fc1 of `nb` sites (a slice) into the workspace
void forward_trunk(nc_train *tr, int64_t nb, const float *x, const double *scale)
{
    snp_trunk_forward(trunk_of(tr), tr->ctx->stream, nb, x, scale);
}

}   // namespace

extern "C" {

int nc_train_create(nc_ctx *ctx, int32_t kind, int64_t max_batch, nc_train **out)
{
    if (!ctx || !out) return NC_ERR_ARG;
    *out = nullptr;
    if (kind != NC_MODEL_SNP)
        return nc_fail(ctx, NC_ERR_UNSUPPORTED, "nc_train_create: only the diploid SNP model (kind %d) is trained, not kind %d", NC_MODEL_SNP, kind);
    if (max_batch < 1) return nc_fail(ctx, NC_ERR_ARG, "nc_train_create: max_batch");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    nc_train *tr = new nc_train;
    tr->ctx = ctx;
    tr->max_batch = max_batch;
    tr->slice = max_batch < MAX_SLICE ? max_batch : MAX_SLICE;
    const int64_t ns = (tr->slice + SLAB - 1) / SLAB;
    size_t sizes[] = {(size_t)tr->slice * XS, (size_t)tr->slice * N1, (size_t)tr->slice * N2, (size_t)tr->slice * N3, (size_t)tr->slice * 48,
                      (size_t)tr->slice * 48, (size_t)tr->slice * TA, (size_t)tr->slice * TD, (size_t)tr->slice * 48, (size_t)tr->slice * N1, (size_t)tr->slice * N2,
                      (size_t)tr->slice * N3, (size_t)ns * NPAR, (size_t)max_batch * 5, 8};
    float **ptrs[] = {&tr->xs, &tr->a1, &tr->a2, &tr->a3, &tr->f1, &tr->f1d, &tr->tact, &tr->tdel, &tr->df1, &tr->d1, &tr->d2, &tr->d3, &tr->slabs, &tr->loss, &tr->loss6};
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~size_t(63);
    tr->ws_bytes = total * 4;
    hipError_t e = hipMalloc((void **)&tr->ws, tr->ws_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->w, (size_t)NPAR * 4 * 4);
    if (e != hipSuccess) {
        if (tr->ws) (void)hipFree(tr->ws);
        delete tr;
        return nc_fail(ctx, NC_ERR_NOMEM, "nc_train_create: hipMalloc of %zu bytes: %s", total * 4, hipGetErrorString(e));
    }
    tr->m = tr->w + NPAR;
    tr->v = tr->m + NPAR;
    tr->g = tr->v + NPAR;
    size_t off = 0;
    for (size_t i = 0; i < sizeof sizes / sizeof sizes[0]; i++) {
        *ptrs[i] = tr->ws + off;
        off += (sizes[i] + 63) & ~size_t(63);
    }
    NC_HIP(ctx, hipMemsetAsync(tr->w, 0, (size_t)NPAR * 4 * 4, ctx->stream));
    for (int i = 0; i <= TS_N; i++) NC_HIP(ctx, hipEventCreate(&tr->ev[i]));
    *out = tr;
    return NC_OK;
}

int nc_train_free(nc_train *tr)
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

int nc_train_set_weights(nc_train *tr, const float *blob_host, size_t n_floats)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!blob_host || n_floats != (size_t)NPAR) return nc_fail(ctx, NC_ERR_ARG, "nc_train_set_weights: expects %d floats", NPAR);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemcpyAsync(tr->w, blob_host, (size_t)NPAR * 4, hipMemcpyHostToDevice, ctx->stream));
    NC_HIP(ctx, hipMemsetAsync(tr->m, 0, (size_t)NPAR * 4 * 3, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tr->t = 0;
    tr->have_grad = false;
    return NC_OK;
}

int nc_train_get_weights(nc_train *tr, float *blob_host, size_t n_floats)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!blob_host || n_floats != (size_t)NPAR) return nc_fail(ctx, NC_ERR_ARG, "nc_train_get_weights: expects %d floats", NPAR);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemcpyAsync(blob_host, tr->w, (size_t)NPAR * 4, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

int nc_train_forward(nc_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                     float keep, float *probs_dev, float *gt_dev)
{
    NC_TRY(check_call(tr, "nc_train_forward", n, x_dev, ref_code_dev));
    nc_ctx *ctx = tr->ctx;
    if (!probs_dev || !(keep > 0.0f && keep <= 1.0f)) return nc_fail(ctx, NC_ERR_ARG, "nc_train_forward: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    if (keep == 1.0f) keep_mask_dev = nullptr;
    for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
        const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
        forward_trunk(tr, nb, x_dev + s0 * NC_SNP_TENSOR, scale_dev ? scale_dev + s0 : nullptr);
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, ctx->stream, tr->f1, tr->f1d, tr->w, ref_code_dev + s0,
                           keep_mask_dev ? keep_mask_dev + s0 * 48 : nullptr, 1.0f / keep, (const uint8_t *)nullptr, 0.0f, nb, probs_dev + s0 * 4,
                           gt_dev ? gt_dev + s0 * 2 : nullptr, tr->tact, tr->tdel, tr->df1, tr->loss);
    }
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

int nc_train_loss_grad(nc_train *tr, int64_t n, const float *x_dev, const int32_t *ref_code_dev, const double *scale_dev, const uint8_t *keep_mask_dev,
                       float keep, const uint8_t *label_dev, float gamma, float *loss6_host, float *grad_dev)
{
    NC_TRY(check_call(tr, "nc_train_loss_grad", n, x_dev, ref_code_dev));
    nc_ctx *ctx = tr->ctx;
    if (!label_dev || !(keep > 0.0f && keep <= 1.0f)) return nc_fail(ctx, NC_ERR_ARG, "nc_train_loss_grad: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (keep == 1.0f) keep_mask_dev = nullptr;
    tr->have_grad = tr->partial = false;
    for (int64_t s0 = 0; s0 < n; s0 += tr->slice) {
        const int64_t nb = n - s0 < tr->slice ? n - s0 : tr->slice;
        const unsigned ns = (unsigned)((nb + SLAB - 1) / SLAB);
        const float *x = x_dev + s0 * NC_SNP_TENSOR;
        mark(tr, TS_FWD);
        forward_trunk(tr, nb, x, scale_dev ? scale_dev + s0 : nullptr);
        const float *xin = scale_dev ? tr->xs : x;
        const int pitch = scale_dev ? XS : 1025;
        mark(tr, TS_HEADS);
        hipLaunchKernelGGL(k_heads, dim3(blocks_for(nb, 64)), dim3(64), 0, st, tr->f1, tr->f1d, tr->w, ref_code_dev + s0,
                           keep_mask_dev ? keep_mask_dev + s0 * 48 : nullptr, 1.0f / keep, label_dev + s0 * 5, 1.0f / (float)n, nb, (float *)nullptr,
                           (float *)nullptr, tr->tact, tr->tdel, tr->df1, tr->loss + s0 * 5);
        hipLaunchKernelGGL(k_small_wgrad, dim3(ns, blocks_for(48 + NPAR - O_FA)), dim3(256), 0, st, tr->tact, tr->tdel, tr->df1, ref_code_dev + s0, nb, tr->slabs);
        snp_trunk_backward<NPAR>(trunk_of(tr), st, nb, xin, pitch, [&](int i) { mark(tr, TS_FC1 + i); });
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
    hipLaunchKernelGGL(k_loss_reduce, dim3(1), dim3(256), 0, st, tr->loss, n, tr->w, gamma, tr->loss6);
    mark(tr, TS_N);
    NC_HIP(ctx, hipGetLastError());
    tr->have_grad = true;
    if (loss6_host) {
        NC_HIP(ctx, hipMemcpyAsync(loss6_host, tr->loss6, 6 * 4, hipMemcpyDeviceToHost, st));
        NC_HIP(ctx, hipStreamSynchronize(st));
    }
    return NC_OK;
}

int nc_train_adam(nc_train *tr, float lr, float beta1, float beta2, float eps)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!tr->have_grad) return nc_fail(ctx, NC_ERR_STATE, "nc_train_adam: no gradient (nc_train_loss_grad comes first, once per step)");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    tr->t++;
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)tr->t)) / (1.0 - std::pow((double)beta1, (double)tr->t)));
    hipLaunchKernelGGL(k_params, dim3(blocks_for(NPAR)), dim3(256), 0, ctx->stream, tr->partial ? tr->g : (const float *)nullptr, tr->slabs, tr->pending_ns, 1,
                       tr->pending_gamma, (float *)nullptr, 1, tr->w, tr->m, tr->v, lr_t, beta1, beta2, eps);
    NC_HIP(ctx, hipGetLastError());
    tr->have_grad = false;
    return NC_OK;
}

int nc_train_info(nc_train *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    if (!tr) return NC_ERR_ARG;
    if (slice_sites) *slice_sites = tr->slice;
    if (workspace_bytes) *workspace_bytes = (int64_t)tr->ws_bytes;
    if (steps) *steps = tr->t;
    return NC_OK;
}

int nc_train_stage_ms(nc_train *tr, int32_t on, float *ms7)
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

// What the four training units share (nc_train.hip, nc_train_hap.hip: the diploid and haploid SNP models through nc_train_snp.h;
// nc_train_indel.hip, nc_train_hap_indel.hip: the two indel models through nc_train_indel.h): SELU's derivative, the shape-templated kernels of the
// 2x3 stride-(1,2) convolutions, and the family-independent host half of a handle (train_state and the train_* functions at the end).
// Each unit instantiates the kernels in its own anonymous namespace.
// SLAB = sites per gradient slab, NPAR = floats per slab (the stride of `slabs`): template parameters here, constants of the including unit.
// lane l of an MFMA: A[row l&15][k l>>4], B[k l>>4][col l&15], C/D col l&15, row 4*(l>>4)+r (the lane maps of nc_cnn_fp32.hip).
#pragma once
#include "nc_cnn.h"

namespace {

__device__ __forceinline__ float selud(float y) { return y > 0.0f ? SELU_L : y + SELU_LA; }   // SELU' from SELU's output
// SELU' from the pre-activation, for the dense layers (fc1, fa, fc2, fc3), whose units can sit at -lambda alpha on every site of a batch: there
// y + lambda alpha cancels to rounding noise of 1e-7 where the derivative is 1e-6, the unit's bias gradient is that noise, and Adam's division by
// sqrt(v) turns it into full-size steps (measured: five steps on ONT-HG002, fc1's bias off by 7.6e-4 against 9e-6 with this form).  192 bytes per
// site for fc1; the other three are in registers anyway.  The convolutions, 99.7 % of the stored activations, take SELU' from the output.
__device__ __forceinline__ float selud_pre(float x) { return x > 0.0f ? SELU_L : SELU_LA * expf(x); }

// conv2 / conv3 forward: k7_conv23_mfma of nc_cnn_fp32.hip (implicit GEMM, M = output positions, N = CO, K = 6 CI tap-major in groups of 16,
// weights in LDS in fragment order) with the accurate exponential in the SELU.
template <int HI, int WI, int CI, int CO>
__global__ __launch_bounds__(256) void k_conv23_fwd(const float *__restrict__ in, const float *__restrict__ wk, const float *__restrict__ wb,
                                                    float *__restrict__ out, int64_t npos)
{
    constexpr int HO = HI - 1, WO = (WI - 3) / 2 + 1, K = 6 * CI, NG = K / 16, TN = CO / 16;
    static_assert(CI % 4 == 0 && K % 16 == 0 && CO % 16 == 0, "k_conv23_fwd: shape");
    __shared__ float4 wf[NG][TN][64];
    for (int idx = threadIdx.x; idx < NG * TN * 64; idx += 256) {
        const int l = idx & 63, tn = (idx >> 6) % TN, G = (idx >> 6) / TN;
        const int k0 = 16 * G + 4 * (l >> 4), col = tn * 16 + (l & 15);
        wf[G][tn][l] = make_float4(wk[(k0 + 0) * CO + col], wk[(k0 + 1) * CO + col], wk[(k0 + 2) * CO + col], wk[(k0 + 3) * CO + col]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kq = lane >> 4, c16 = lane & 15;
    const int64_t ntiles = (npos + 15) / 16;
    float bias[TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) bias[tn] = wb[tn * 16 + c16];
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        int64_t m = tile * 16 + c16;
        if (m >= npos) m = npos - 1;
        const int64_t site = m / (HO * WO);
        const int r = (int)(m - site * (HO * WO));
        const int y = r / WO, xq = r - y * WO;
        const float *ip = in + ((site * HI + y) * WI + 2 * xq) * CI;
        f32x4v acc[TN];
#pragma unroll
        for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4v){bias[tn], bias[tn], bias[tn], bias[tn]};
#pragma unroll
        for (int G = 0; G < NG; G++) {
            const int k0 = 16 * G + 4 * kq, tap = k0 / CI, ci = k0 - tap * CI;
            const float4 a = *reinterpret_cast<const float4 *>(ip + ((tap / 3) * WI + (tap % 3)) * CI + ci);
#pragma unroll
            for (int tn = 0; tn < TN; tn++) {
                const float4 b = wf[G][tn][lane];
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[tn], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int64_t pos = tile * 16 + 4 * kq + rr;
            if (pos < npos) {
#pragma unroll
                for (int tn = 0; tn < TN; tn++) out[pos * CO + tn * 16 + c16] = selu_acc(acc[tn][rr]);
            }
        }
    }
}

// Weight gradient of a 2x3 stride-(1,2) valid convolution, dW[tap][ci][co] = sum over output positions of in[.. tap ..][ci] d[pos][co], of one
// slab: M = (tap, ci) in tiles of 16 (a lane's row m = tile * 16 + (l & 15) names its own tap and channel, so CI need not be a multiple of
// 16), N = CO, K = output positions, four per MFMA.  grid (slabs, M tiles / MW): the four waves of a workgroup take SLAB / 4 sites of the
// slab each and combine through LDS in wave order.
template <int HI, int WI, int CI, int CO, int MW, int SLAB, int NPAR>
__global__ __launch_bounds__(256) void k_conv_wgrad(const float *__restrict__ in, const float *__restrict__ d, int64_t n, int koff, float *__restrict__ slabs)
{
    constexpr int HO = HI - 1, WO = (WI - 3) / 2 + 1, NPOS = HO * WO, TN = CO / 16;
    static_assert((6 * CI) % 16 == 0 && CO % 16 == 0 && (6 * CI / 16) % MW == 0 && SLAB % 16 == 0, "k_conv_wgrad: shape");
    __shared__ float red[3][MW][TN][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const int64_t p0 = ((int64_t)blockIdx.x * SLAB + (SLAB / 4) * wv) * NPOS, pend = n * NPOS;
    int aoff[MW];
#pragma unroll
    for (int mw = 0; mw < MW; mw++) {
        const int m = (blockIdx.y * MW + mw) * 16 + c16, tap = m / CI, ci = m - tap * CI;
        aoff[mw] = ((tap / 3) * WI + (tap % 3)) * CI + ci;
    }
    f32x4v acc[MW][TN];
#pragma unroll
    for (int mw = 0; mw < MW; mw++)
#pragma unroll
        for (int tn = 0; tn < TN; tn++) acc[mw][tn] = (f32x4v){0, 0, 0, 0};
#pragma unroll 2
    for (int st = 0; st < (SLAB / 16) * NPOS; st++) {
        const int64_t p = p0 + 4 * st + q;
        const bool ok = p < pend;
        const int64_t site = p / NPOS;
        const int r = (int)(p - site * NPOS), y = r / WO, x = r - y * WO;
        const float *ip = in + ((site * HI + y) * WI + 2 * x) * CI;
        float a[MW], b[TN];
#pragma unroll
        for (int mw = 0; mw < MW; mw++) a[mw] = ok ? ip[aoff[mw]] : 0.0f;
#pragma unroll
        for (int tn = 0; tn < TN; tn++) b[tn] = ok ? d[p * CO + tn * 16 + c16] : 0.0f;
#pragma unroll
        for (int mw = 0; mw < MW; mw++)
#pragma unroll
            for (int tn = 0; tn < TN; tn++) acc[mw][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mw], b[tn], acc[mw][tn], 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int mw = 0; mw < MW; mw++)
#pragma unroll
            for (int tn = 0; tn < TN; tn++)
#pragma unroll
                for (int r = 0; r < 4; r++) red[wv - 1][mw][tn][r][lane] = acc[mw][tn][r];
    }
    __syncthreads();
    if (wv == 0) {
        float *out = slabs + (int64_t)blockIdx.x * NPAR + koff;
#pragma unroll
        for (int mw = 0; mw < MW; mw++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m = (blockIdx.y * MW + mw) * 16 + 4 * q + r;
#pragma unroll
                for (int tn = 0; tn < TN; tn++)
                    out[m * CO + tn * 16 + c16] = ((acc[mw][tn][r] + red[0][mw][tn][r][lane]) + red[1][mw][tn][r][lane]) + red[2][mw][tn][r][lane];
            }
    }
}

// Data gradient of the same convolution (the transposed convolution), times SELU' of the layer below: M = input positions, N = CI in tiles of
// 16 (columns past CI carry zero weights and are not stored), K = (tap, co) in groups of 16; a tap that does not reach an output position
// from this input position enters as zeros.  The weights sit in LDS in fragment order, transposed:
// wf[G][tn][lane] = W[tap][ci = 16 tn + (lane & 15)][co0 .. co0 + 3].
template <int HI, int WI, int CI, int CO>
__global__ __launch_bounds__(256) void k_conv_dgrad(const float *__restrict__ d, const float *__restrict__ wk, const float *__restrict__ act,
                                                    float *__restrict__ out, int64_t npos)
{
    constexpr int HO = HI - 1, WO = (WI - 3) / 2 + 1, K = 6 * CO, NG = K / 16, TN = (CI + 15) / 16;
    static_assert(CI % 8 == 0 && CO % 16 == 0, "k_conv_dgrad: shape");
    __shared__ float4 wf[NG][TN][64];
    for (int idx = threadIdx.x; idx < NG * TN * 64; idx += 256) {
        const int l = idx & 63, tn = (idx >> 6) % TN, G = (idx >> 6) / TN;
        const int k0 = 16 * G + 4 * (l >> 4), tap = k0 / CO, co = k0 - tap * CO, ci = tn * 16 + (l & 15);
        wf[G][tn][l] = ci < CI ? *reinterpret_cast<const float4 *>(wk + (tap * CI + ci) * CO + co) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kq = lane >> 4, c16 = lane & 15;
    const int64_t ntiles = (npos + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        int64_t m = tile * 16 + c16;
        if (m >= npos) m = npos - 1;
        const int64_t site = m / (HI * WI);
        const int r = (int)(m - site * (HI * WI)), yi = r / WI, xi = r - yi * WI;
        const float *dp = d + site * (HO * WO * CO);
        f32x4v acc[TN];
#pragma unroll
        for (int tn = 0; tn < TN; tn++) acc[tn] = (f32x4v){0, 0, 0, 0};
#pragma unroll
        for (int G = 0; G < NG; G++) {
            const int tap = (16 * G) / CO, co = 16 * G - tap * CO + 4 * kq;
            const int y = yi - tap / 3, xx = xi - tap % 3;
            const bool ok = y >= 0 && y < HO && xx >= 0 && (xx & 1) == 0 && (xx >> 1) < WO;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ok) a = *reinterpret_cast<const float4 *>(dp + (y * WO + (xx >> 1)) * CO + co);
#pragma unroll
            for (int tn = 0; tn < TN; tn++) {
                const float4 b = wf[G][tn][lane];
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[tn], 0, 0, 0);
                acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[tn], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int64_t pos = tile * 16 + 4 * kq + rr;
            if (pos < npos) {
#pragma unroll
                for (int tn = 0; tn < TN; tn++) {
                    if (tn * 16 + c16 < CI) {
                        const int64_t o = pos * CI + tn * 16 + c16;
                        out[o] = acc[tn][rr] * selud(act[o]);
                    }
                }
            }
        }
    }
}

// bias gradient of a convolution, db[c] = sum over the slab's positions of d[pos][c]: 256 / C strided partial sums per channel,
// combined in order (the threads past C * (256 / C) idle)
template <int C, int NPOS, int SLAB, int NPAR>
__global__ __launch_bounds__(256) void k_bias_grad(const float *__restrict__ d, int64_t n, int boff, float *__restrict__ slabs)
{
    constexpr int NP = 256 / C;
    __shared__ float red[NP][C];
    const int c = threadIdx.x % C, part = threadIdx.x / C;
    const int64_t s0 = (int64_t)blockIdx.x * SLAB, s1 = s0 + SLAB < n ? s0 + SLAB : n;
    float acc = 0.0f;
    if (part < NP) {
#pragma unroll 8
        for (int64_t p = s0 * NPOS + part; p < s1 * NPOS; p += NP) acc += d[p * C + c];   // (unrolled: eight loads in flight, the adds stay in order)
        red[part][c] = acc;
    }
    __syncthreads();
    if (part == 0) {
        float v = red[0][c];
        for (int k = 1; k < NP; k++) v += red[k][c];
        slabs[(int64_t)blockIdx.x * NPAR + boff + c] = v;
    }
}

// ------------------------------------------------------------------------------------- the host side of a handle, whatever the model family
enum { TS_FWD = 0, TS_HEADS, TS_FC1, TS_CONV3, TS_CONV2, TS_CONV1, TS_PARAMS, TS_N };

// A family derives its state from this and adds the pointers of its workspace buffers.
struct train_state {
    nc_ctx *ctx = nullptr;
    int64_t max_batch = 0, slice = 0;
    size_t ws_bytes = 0;
    float *w = nullptr, *m = nullptr, *v = nullptr, *g = nullptr;      // fp32 state in blob order
    float *ws = nullptr;                                               // one allocation: the family's buffers
    int64_t t = 0;                                                     // Adam steps taken
    // the gradient of the last loss_grad = g (what of it the family keeps there; with `partial` also the earlier slices' sums) + the pending
    // slabs + gamma w: summed by the adam call's own kernel
    bool have_grad = false, partial = false;
    int pending_ns = 0;
    float pending_gamma = 0.0f;
    int timing = 0;
    hipEvent_t ev[TS_N + 1] = {nullptr};
};

inline void train_mark(train_state *tr, int i)
{
    if (tr->timing) (void)hipEventRecord(tr->ev[i], tr->ctx->stream);
}

// The allocations and events of a handle whose ctx, max_batch and slice are set: *ptrs[i] = sizes[i] floats of one allocation, each piece
// rounded up to 64 floats, and w | m | v | g = 4 npar zeroed floats of another.  After a failure the caller calls train_release.
template <size_t N>
inline int train_alloc(train_state *tr, const char *name, int npar, const size_t (&sizes)[N], float **const (&ptrs)[N])
{
    nc_ctx *ctx = tr->ctx;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~size_t(63);
    tr->ws_bytes = total * 4;
    hipError_t e = hipMalloc((void **)&tr->ws, tr->ws_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&tr->w, (size_t)npar * 4 * 4);
    if (e != hipSuccess) return nc_fail(ctx, NC_ERR_NOMEM, "%s_create: hipMalloc of %zu bytes: %s", name, total * 4, hipGetErrorString(e));
    tr->m = tr->w + npar;
    tr->v = tr->m + npar;
    tr->g = tr->v + npar;
    size_t off = 0;
    for (size_t i = 0; i < N; i++) {
        *ptrs[i] = tr->ws + off;
        off += (sizes[i] + 63) & ~size_t(63);
    }
    NC_HIP(ctx, hipMemsetAsync(tr->w, 0, (size_t)npar * 4 * 4, ctx->stream));
    for (int i = 0; i <= TS_N; i++) NC_HIP(ctx, hipEventCreate(&tr->ev[i]));
    return NC_OK;
}

// (also after a train_alloc that failed half way: every member is null or owned)
inline void train_release(train_state *tr)
{
    (void)hipSetDevice(tr->ctx->device);
    (void)hipStreamSynchronize(tr->ctx->stream);
    for (int i = 0; i <= TS_N; i++)
        if (tr->ev[i]) (void)hipEventDestroy(tr->ev[i]);
    if (tr->ws) (void)hipFree(tr->ws);
    if (tr->w) (void)hipFree(tr->w);
}

// What every create() does around train_alloc: H is the handle type of the ABI, a family's state and nothing more; init(tr) sets the slice
// and allocates.
template <class H, class Init>
inline int train_create(nc_ctx *ctx, int64_t max_batch, H **out, Init init)
{
    H *tr = new H;
    tr->ctx = ctx;
    tr->max_batch = max_batch;
    const int rc = init(tr);
    if (rc != NC_OK) {
        train_release(tr);
        delete tr;
        return rc;
    }
    *out = tr;
    return NC_OK;
}

template <class H>
inline int train_free(H *tr)
{
    if (!tr) return NC_OK;
    train_release(tr);
    delete tr;
    return NC_OK;
}

inline int train_check_call(train_state *tr, const char *name, const char *fn, int64_t n, bool have_inputs, float keep)
{
    if (!tr) return NC_ERR_ARG;
    if (n < 1 || n > tr->max_batch)
        return nc_fail(tr->ctx, NC_ERR_ARG, "%s_%s: n = %lld outside 1 .. max_batch = %lld", name, fn, (long long)n, (long long)tr->max_batch);
    if (!have_inputs) return nc_fail(tr->ctx, NC_ERR_ARG, "%s_%s: null argument", name, fn);
    if (!(keep > 0.0f && keep <= 1.0f)) return nc_fail(tr->ctx, NC_ERR_ARG, "%s_%s: keep = %g outside (0, 1]", name, fn, (double)keep);
    return NC_OK;
}

inline int train_set_weights(train_state *tr, const char *name, int npar, const float *blob_host, size_t n_floats)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!blob_host || n_floats != (size_t)npar) return nc_fail(ctx, NC_ERR_ARG, "%s_set_weights: expects %d floats", name, npar);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemcpyAsync(tr->w, blob_host, (size_t)npar * 4, hipMemcpyHostToDevice, ctx->stream));
    NC_HIP(ctx, hipMemsetAsync(tr->m, 0, (size_t)npar * 4 * 3, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    tr->t = 0;
    tr->have_grad = false;
    return NC_OK;
}

inline int train_get_weights(train_state *tr, const char *name, int npar, float *blob_host, size_t n_floats)
{
    if (!tr) return NC_ERR_ARG;
    nc_ctx *ctx = tr->ctx;
    if (!blob_host || n_floats != (size_t)npar) return nc_fail(ctx, NC_ERR_ARG, "%s_get_weights: expects %d floats", name, npar);
    NC_HIP(ctx, hipSetDevice(ctx->device));
    NC_HIP(ctx, hipMemcpyAsync(blob_host, tr->w, (size_t)npar * 4, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

// The end of a loss_grad whose kernels are enqueued: lossv = the `nloss` loss terms on the device.  With `bad_labels` (what a bad label is, for
// the error text) lossv[nloss] is the flag the heads kernel sets for a label outside the classes: the labels are on the device, so the call
// always waits, and a bad label leaves no gradient pending.  Without, it waits only when the caller wants the losses.
inline int train_finish_loss_grad(train_state *tr, const char *name, const float *lossv, int nloss, const char *bad_labels, float *loss_host)
{
    nc_ctx *ctx = tr->ctx;
    hipStream_t st = ctx->stream;
    if (bad_labels) {
        float l[8] = {0.0f};
        NC_HIP(ctx, hipMemcpyAsync(l, lossv, (size_t)(nloss + 1) * 4, hipMemcpyDeviceToHost, st));
        NC_HIP(ctx, hipStreamSynchronize(st));
        if (l[nloss] != 0.0f) return nc_fail(ctx, NC_ERR_ARG, "%s_loss_grad: a label outside %s", name, bad_labels);
        tr->have_grad = true;
        for (int i = 0; loss_host && i < nloss; i++) loss_host[i] = l[i];
        return NC_OK;
    }
    tr->have_grad = true;
    if (loss_host) {
        NC_HIP(ctx, hipMemcpyAsync(loss_host, lossv, (size_t)nloss * 4, hipMemcpyDeviceToHost, st));
        NC_HIP(ctx, hipStreamSynchronize(st));
    }
    return NC_OK;
}

// Adam's step size in TensorFlow's form after `t` steps
inline float train_lr_t(float lr, float beta1, float beta2, int64_t t)
{
    return (float)((double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)t)) / (1.0 - std::pow((double)beta1, (double)t)));
}

inline int train_info(train_state *tr, int64_t *slice_sites, int64_t *workspace_bytes, int64_t *steps)
{
    if (!tr) return NC_ERR_ARG;
    if (slice_sites) *slice_sites = tr->slice;
    if (workspace_bytes) *workspace_bytes = (int64_t)tr->ws_bytes;
    if (steps) *steps = tr->t;
    return NC_OK;
}

inline int train_stage_ms(train_state *tr, int32_t on, float *ms7)
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

}   // namespace

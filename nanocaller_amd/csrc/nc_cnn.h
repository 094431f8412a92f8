// CNN forward of the four NanoCaller models (gfx950): what its translation units share.  The kernels live in the anonymous namespaces of
// their units; the driver (nc_cnn.hip) reaches them through the nc_cnn_launch_* functions and their weight packers through the nc_cnn_pack_*
// functions declared at the end of this file.  A packer lives in the unit of the kernel that reads its layout.
//
//   nc_cnn_fp32.hip   exact fp32: k2_conv1_x4, k7_conv23_mfma (indel convs), k4_conv12 (SNP trunk, its F12_* layout and packer), k3_fc1
//   nc_cnn_h3.hip     the split-precision kernels, one unit of two files (the reason is in its header):
//     nc_cnn_snp.inc    SNP: k5_trunk_p3, k5_trunk_lin, k6_fc1_h3, their layout constants, role tables and packers;
//                     which of the SNP trunks a context runs (nc_cnn_snp_trunk_select)
//     nc_cnn_indel.inc  indel: k10_indel_trunk_h3, H3Layer, its packers
//   nc_cnn.hip        head kernels, range guard, nc_load_weights, the forward entry points and the two trunk drivers
//
// Here: SELU, the vector types and the split-precision primitives of both families (a product is hi*hi + hi*lo + lo*hi of fp16 halves,
// DESIGN.md), on the host the one "scale + hi / lo split" of a weight.
#pragma once
#include <cmath>
#include <vector>

#include "nc_common.h"

constexpr float SELU_L = 1.0507009873554805f;
constexpr float SELU_LA = 1.0507009873554805f * 1.6732632423543772f;

// SELU.  The trunk's 14k activations per site use the hardware exponential (v_exp_f32 after a multiply by log2 e,
// relative error ~1e-6 at most for x in [-20, 0]: absolute error of the negative branch < 2e-6); the tiny heads
// use the accurate expf.  Parity tests hold the end-to-end probabilities far inside 1e-4.
__device__ __forceinline__ float selu(float x) { return x > 0.0f ? SELU_L * x : SELU_LA * (__expf(x) - 1.0f); }
__device__ __forceinline__ float selu_acc(float x) { return x > 0.0f ? SELU_L * x : SELU_LA * (expf(x) - 1.0f); }

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h8 as_h8(uint4 v) { union { uint4 u; h8 h; } c; c.u = v; return c.h; }
__device__ __forceinline__ h8 lds_h8(const _Float16 *p) { return *reinterpret_cast<const h8 *>(p); }
// Epilogue constants: accumulators hold S * (conv + bias);
//   selu(a / S) = L * max(a, 0) / S + L*A * (exp(min(a, 0) / S) - 1)
// c1 = log2(e) / S, c2 = L / S, c3 = clamp of max(a, 0) that keeps the result inside fp16 range.
struct h_epi { float c1, c2, c3; };
// exp2 with the VOP3 clamp modifier (result clamped to [0,1]): clamp01(exp2(x)) == exp2(min(x, 0)), one instruction
__device__ __forceinline__ float exp2_clamp01(float x) { float r; asm("v_exp_f32_e64 %0, %1 clamp" : "=v"(r) : "v"(x)); return r; }
// v - float(lo / hi half of a packed f16 pair): v_fma_mix_f32 reads the f16 operand directly (no separate v_cvt_f32_f16)
__device__ __forceinline__ float sub_h_lo(float v, uint32_t hpk) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpk), "v"(v)); return r; }
__device__ __forceinline__ float sub_h_hi(float v, uint32_t hpk) { float r; asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpk), "v"(v)); return r; }
__device__ __forceinline__ f32x4v selu4_scaled(const f32x4v &acc, const h_epi &k)
{
    f32x4v s;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float a = acc[r];
        const float e = exp2_clamp01(a * k.c1);                       // exp(min(a, 0) / S)
        const float pos = __builtin_amdgcn_fmed3f(a, 0.0f, k.c3);
        const float neg = fmaf(e, SELU_LA, -SELU_LA);                 // exactly 0 for a >= 0
        s[r] = fmaf(pos, k.c2, neg);
    }
    return s;
}
// The MFMAs are issued with the weights as the A operand, so a lane's four accumulator registers are four CONSECUTIVE
// channels (4g .. 4g+3) of ONE position (c16): hi and lo halves go out as one ds_write_b64 each, no cross-lane traffic.
__device__ __forceinline__ void split4_store(const f32x4v &v, _Float16 *hp, _Float16 *lp)
{
    const h2 h01 = __builtin_convertvector((f32x2v){v[0], v[1]}, h2), h23 = __builtin_convertvector((f32x2v){v[2], v[3]}, h2);   // v_cvt_pk_f16_f32, RNE
    const uint32_t u01 = __builtin_bit_cast(uint32_t, h01), u23 = __builtin_bit_cast(uint32_t, h23);
    const f32x2v d01 = {sub_h_lo(v[0], u01), sub_h_hi(v[1], u01)}, d23 = {sub_h_lo(v[2], u23), sub_h_hi(v[3], u23)};              // exact in fp32
    const h2 l01 = __builtin_convertvector(d01, h2), l23 = __builtin_convertvector(d23, h2);
    *reinterpret_cast<uint2 *>(hp) = make_uint2(u01, u23);
    *reinterpret_cast<uint2 *>(lp) = make_uint2(__builtin_bit_cast(uint32_t, l01), __builtin_bit_cast(uint32_t, l23));
}

// host: weights enter the split-precision kernels multiplied by a power of two S, so that their low halves stay normal fp16 numbers:
// the largest S <= s0 with max |w| S <= 16384 over the floats [w0, w1); split() gives fp16 hi and lo (of the remainder) of v S.
struct H3Scale {
    float S;
    H3Scale(const float *w0, const float *w1, float s0) : S(s0)
    {
        float wmax = 0.0f;
        for (const float *q = w0; q < w1; q++) wmax = std::fmax(wmax, std::fabs(*q));
        while (S > 1.0f && wmax * S > 16384.0f) S *= 0.5f;
    }
    void split(float v, _Float16 &h, _Float16 &l) const
    {
        const float sv = v * S;
        h = (_Float16)sv;
        l = (_Float16)(sv - (float)h);
    }
};

inline unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// ---- SNP trunks.  Kernel ids as nc_snp_trunk_info reports them.
enum { NC_TRUNK_FP32 = 0, NC_TRUNK_P3 = 2, NC_TRUNK_LIN = 3 };
struct SnpTrunk { int kernel_id, mfma_per_site; };
// the trunk the context's next nc_snp_forward runs: k4_conv12 in exact-fp32 mode, else k5_trunk_lin (conv1 by linearity; int16 tensors only)
// unless NC_TRUNK_LIN=0; float32 tensors take k5_trunk_p3 (their entries need not be integers)
SnpTrunk nc_cnn_snp_trunk_select(const nc_ctx *ctx);
// one launch of a trunk over the `nb` sites of a batch -> a3 [nb][27][64]
struct SnpTrunkArgs {
    hipStream_t stream;
    hipEvent_t ev0, ev1;               // timing mode: start / stop events on the kernel's own dispatch packet (null otherwise)
    const float *x_f32;                // the batch's tensors: float32, or
    const int16_t *x_i16;              // int16 (nc_set_tensor_format), the other pointer null
    float *a3;
    int64_t nb, site0;                 // site0: the batch's first site in scale[] and range_sites[]
    const double *scale;
    int scale_mode;
    float x_limit;
    uint8_t *range_sites;
};
void nc_cnn_launch_k4_conv12(const SnpTrunkArgs &a, const float *packed);                       // nc_cnn_fp32.hip
void nc_cnn_launch_k5_trunk(int kernel_id, const SnpTrunkArgs &a, const uint8_t *packed_h);      // nc_cnn_snp.inc: NC_TRUNK_P3 / NC_TRUNK_LIN
void nc_cnn_launch_fc1_h3(hipStream_t st, const float *a3, const uint8_t *packed_h, float *f1, int64_t nb);
std::vector<float> nc_cnn_pack_k4(const float *blob);              // nc_weights::packed of an SNP model
std::vector<uint8_t> nc_cnn_pack_snp_h3(const float *blob);        // nc_weights::packed_h of an SNP model: [k5 trunks | k6_fc1_h3 | k5_trunk_lin's conv1]

// ---- exact-fp32 fc1 (nc_cnn_fp32.hip): F = 48 (SNP, K = 1728) or 32 (indel) outputs
void nc_cnn_launch_fc1_fp32(hipStream_t st, int F, const float *a3, int K, const float *kf, const float *bf, float *f1, int64_t nb);

// ---- indel trunks, image height H = 15 (diploid) or 5 (haploid)
void nc_cnn_launch_indel_convs_fp32(hipStream_t st, int H, const float *x, const float *w, float *a1, float *a2, float *a3, int64_t nb);   // nc_cnn_fp32.hip
int nc_cnn_launch_k10(nc_ctx *ctx, int H, const float *x, const uint8_t *packed_h, float *a3, int64_t nb);                                  // nc_cnn_indel.inc
std::vector<uint8_t> nc_cnn_pack_indel_h3(const float *blob);      // nc_weights::packed_h of an indel model: [conv2 | conv3 | conv1]

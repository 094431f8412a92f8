// What the phaser (nc_happhase.hip) and its allele detector by realignment (nc_hprealign.hip) share: the phasing handle, the prefix kernel
// that turns per-read counts into offsets, per-call device scratch.
#pragma once
#include "nc_common.h"

#include <chrono>
#include <vector>

namespace {

constexpr int HP_THREADS = 1024;

__device__ __forceinline__ int32_t hp_lower_bound(const int32_t *a, int32_t lo, int32_t hi, int32_t v)
{
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(HP_THREADS) void k_hp_scan(const int32_t *__restrict__ cnt, int32_t n, int64_t *__restrict__ off)
{
    __shared__ int32_t wsum[HP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t carry = 0;
    if (tid == 0) off[0] = 0;
    for (int32_t base = 0; base < n; base += HP_THREADS) {
        const int32_t i = base + tid;
        const int32_t inc = nc_wave_incl_scan(i < n ? cnt[i] : 0);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int32_t pre = 0, tot = 0;
        for (int k = 0; k < HP_THREADS / 64; k++) {
            const int32_t s = wsum[k];
            pre += k < w ? s : 0;
            tot += s;
        }
        if (i < n) off[i + 1] = carry + pre + inc;
        carry += tot;
        __syncthreads();
    }
}

inline double hp_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct nc_phase {
    nc_ctx *ctx = nullptr;
    int32_t n_reads = 0, n_sites = 0, n_groups = 0;
    std::vector<int32_t> site_pos;
    std::vector<int64_t> off;
    std::vector<int32_t> esite;
    std::vector<uint8_t> eal;
    int64_t *d_off = nullptr;
    int32_t *d_site = nullptr;
    uint8_t *d_al = nullptr;
    std::vector<int8_t> side;
    std::vector<int32_t> site_block, site_ps, block_first, block_last, block_ps;
    std::vector<uint8_t> site_h, site_phased, group_hp;
    std::vector<uint8_t> site_gt;          // nc_snp_phase_solve_gt only: the outcome per site (0 het, 1 / 2 homozygous first / second allele)
    std::vector<int64_t> block_cost;
    std::vector<int32_t> group_ps;
    // the weighted model (nc_snp_phase_set_weights / nc_snp_phase_weights_from_bam): per entry its weight 0..93, per read its MAPQ (0 when the
    // weights came from the host) and whether read selection may accept it; d_w = the weights beside d_site / d_al
    std::vector<uint8_t> ew, rmapq, rok;
    uint8_t *d_w = nullptr;
    bool weighted = false;
    float ms[4] = {0, 0, 0, 0};
    bool solved = false;
};

// device scratch of one call, released on every return path
struct HpScratch {
    std::vector<void *> p;
    ~HpScratch()
    {
        for (void *q : p) (void)hipFree(q);
    }
    template <class T>
    int get(nc_ctx *ctx, T **out, size_t n)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, n * sizeof(T) + 16);
        if (e != hipSuccess) return nc_fail(ctx, NC_ERR_NOMEM, "hipMalloc(%zu) failed: %s", n * sizeof(T), hipGetErrorString(e));
        p.push_back(q);
        *out = (T *)q;
        return NC_OK;
    }
};

static inline int hp_check_sites(nc_ctx *ctx, int32_t n_sites, const int32_t *pos)
{
    for (int32_t s = 1; s < n_sites; s++)
        if (pos[s] <= pos[s - 1]) return nc_fail(ctx, NC_ERR_ARG, "phasing sites must ascend strictly (site %d)", s);
    return NC_OK;
}

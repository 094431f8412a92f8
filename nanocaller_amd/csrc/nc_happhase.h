// What the phaser (nc_happhase.hip), its allele detector by realignment (nc_hprealign.hip) and its quality reader (nc_hpquals.hip) share: the
// phasing handle and its set-up, the prefix kernel that turns per-read counts into offsets and the tail that turns them into the entry arrays,
// the uploads of the CSR and its weights, per-call device scratch.
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

// a handle over the checked sites: ctx, n_reads, n_sites and site_pos filled in, off = n_reads + 1 zeros
static inline int hp_new_handle(nc_ctx *ctx, int32_t n_reads, int32_t n_sites, const int32_t *site_pos, nc_phase **out)
{
    NC_TRY(hp_check_sites(ctx, n_sites, site_pos));
    nc_phase *ph = new nc_phase();
    ph->ctx = ctx;
    ph->n_reads = n_reads;
    ph->n_sites = n_sites;
    ph->site_pos.assign(site_pos, site_pos + n_sites);
    ph->off.assign(n_reads + 1, 0);
    *out = ph;
    return NC_OK;
}

// keeps the first HIP error of a sequence of calls whose later steps ask `rc == NC_OK` before they run
struct HpErr {
    nc_ctx *ctx;
    int rc = NC_OK;
    void operator()(hipError_t e, const char *what)
    {
        if (e != hipSuccess && rc == NC_OK) rc = nc_fail(ctx, NC_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    }
};

// The tail the allele detectors share: the per-read entry counts d_cnt on the device -> ph->d_off and ph->off (k_hp_scan), d_site / d_al
// allocated for the total, filled by the caller's launch fill() (asked for only where there are reads), esite / eal downloaded.
// sync_what: the caller's label of the two synchronisations in an error message.  d_flag (or null): a word the caller's kernels raise on malformed input; it comes down with the offsets, and nonzero fails with flag_msg.
template <class Fill>
static inline int hp_entries_from_counts(nc_phase *ph, HpErr &hip, const int32_t *d_cnt, const char *sync_what, const int32_t *d_flag, const char *flag_msg,
                                         Fill fill)
{
    nc_ctx *ctx = ph->ctx;
    const int32_t n_reads = ph->n_reads;
    int32_t flag = 0;
    if (hip.rc == NC_OK) {
        k_hp_scan<<<1, HP_THREADS, 0, ctx->stream>>>(d_cnt, n_reads, ph->d_off);
        hip(hipGetLastError(), "k_hp_scan");
        hip(hipMemcpyAsync(ph->off.data(), ph->d_off, (n_reads + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream), "offset download");
        if (d_flag) hip(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream), "status download");
        hip(hipStreamSynchronize(ctx->stream), sync_what);
    }
    if (hip.rc == NC_OK && flag) hip.rc = nc_fail(ctx, NC_ERR_ARG, "%s", flag_msg);
    const int64_t ne = hip.rc == NC_OK ? ph->off[n_reads] : 0;
    if (hip.rc == NC_OK) {
        hip(hipMalloc(&ph->d_site, ne * sizeof(int32_t) + 16), "hipMalloc(entries)");
        hip(hipMalloc(&ph->d_al, ne + 16), "hipMalloc(alleles)");
    }
    if (hip.rc == NC_OK && n_reads) fill();
    if (hip.rc == NC_OK) {
        ph->esite.resize(ne);
        ph->eal.resize(ne);
        if (ne) {
            hip(hipMemcpyAsync(ph->esite.data(), ph->d_site, ne * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream), "entry download");
            hip(hipMemcpyAsync(ph->eal.data(), ph->d_al, ne, hipMemcpyDeviceToHost, ctx->stream), "allele download");
        }
        hip(hipStreamSynchronize(ctx->stream), sync_what);
    }
    return hip.rc;
}

static inline int hp_upload_csr(nc_phase *ph)
{
    nc_ctx *ctx = ph->ctx;
    const int64_t ne = ph->off[ph->n_reads];
    NC_HIP(ctx, hipMalloc(&ph->d_off, (ph->n_reads + 1) * sizeof(int64_t)));
    NC_HIP(ctx, hipMalloc(&ph->d_site, ne * sizeof(int32_t) + 16));
    NC_HIP(ctx, hipMalloc(&ph->d_al, ne + 16));
    NC_HIP(ctx, hipMemcpyAsync(ph->d_off, ph->off.data(), (ph->n_reads + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (ne) {
        NC_HIP(ctx, hipMemcpyAsync(ph->d_site, ph->esite.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(ph->d_al, ph->eal.data(), ne, hipMemcpyHostToDevice, ctx->stream));
    }
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

// the weighted model's entry weights beside the CSR in HBM (k_hp_tag<true> reads them)
static inline int hp_upload_weights(nc_phase *ph)
{
    nc_ctx *ctx = ph->ctx;
    if (!ph->d_w) NC_HIP(ctx, hipMalloc(&ph->d_w, ph->ew.size() + 16));
    if (!ph->ew.empty()) NC_HIP(ctx, hipMemcpyAsync(ph->d_w, ph->ew.data(), ph->ew.size(), hipMemcpyHostToDevice, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

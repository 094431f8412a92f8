// Read-based SNP phasing (exact minimum-error-correction DP over at most 15 reads per column, WhatsHap's model) and read
// haplotagging, on the contig's resident read pack.  DESIGN.md "Read-based phasing" states the algorithm; every tie-break below
// is part of it (tests/phase_ref.py restates it in numpy and the GPU tests compare bit for bit).
//
//   k_hp_gather<false>  per read: the number of its alleles at the het sites (code == first / second allele)
//   k_hp_scan           one workgroup: exclusive prefix of those counts (nc_wave_incl_scan) -> read -> entry offsets
//   k_hp_gather<true>   per read: the (site, allele) CSR entries
//   (nc_hprealign.hip)  instead of k_hp_gather, opt-in: the alleles by local realignment of the read against both haplotypes
//   host                read selection (max_cov), blocks, slot assignment, per-column masks, backtrace offsets
//   k_hp_dp<GT, W>      one workgroup per block: the 2^15 partition costs in LDS (uint16, relative to the column minimum),
//                       leaving slots minimised out, backtrace in HBM, traceback by the same workgroup; HpColCost is the column cost of all four forms
//     GT                opt-in (nc_snp_phase_solve_gt): the column cost may also call the site homozygous for either allele, at a price for
//                       leaving the called genotype; the traceback records each column's outcome
//     W                 the weighted model (DESIGN.md "Read-based phasing", step 6c; nc_hpquals.hip sets the weights): an entry's flip costs its
//                       weight instead of 1; the column's signed weight sums come from two tables in LDS
//   k_hp_tag<W>         one thread per read-name group: per-block scores (W: +-weight) -> HP / PS
#include "nc_happhase.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace {

constexpr int HP_SLOTS = 15;
constexpr int HP_STATES = 1 << HP_SLOTS;
constexpr int HP_GT_COST_MAX = 1024;       // (a column's cost stays far inside the DP's 16-bit relative range)
constexpr int HP_WTAB = 256 + 128;         // the weighted column's two tables: subsets of slots 0..7, of slots 8..14

struct HpCol {            // one column of a block: the active slots, those continuing from the previous column, the allele masks
    uint16_t act, keep, m0, m1;
};

// the weighted form's LDS tables (only its instantiations allocate them): T[x] = sum of d over the slots of x, d[s] = +w on the m1 slots,
// -w on the m0 slots; entries 0..255 for the slots 0..7, 256..383 for the slots 8..14
template <bool W>
__device__ __forceinline__ int16_t *hp_wtab()
{
    if constexpr (W) {
        __shared__ int16_t T[HP_WTAB];
        return T;
    } else {
        return nullptr;
    }
}

// The cost of column j, stated once for the four forms.  A subset B of the slots puts its reads on the second haplotype: e0 / e1 = what the
// column's alleles cost when the site's first / second allele lies on the first haplotype, e0 = C(m1 & ~B) + C(m0 & B) and
// e1 = C(m0 & ~B) + C(m1 & B), C = the number of slots or (W) the sum of their weights w[slot].
// GT: the site may also come out homozygous: het(B) = min(e0, e1) + hadd against the column's constants homA = C(m1) and homB = C(m0), each
// with the price G added where it leaves the called class gt (0 het, 1 / 2 homozygous first / second allele).
template <bool GT, bool W>
struct HpColCost {
    uint32_t m0, m1;
    uint32_t c0 = 0, c1 = 0;                                            // C(m0), C(m1)
    uint32_t gt = 0, hadd = 0, homA = 0, homB = 0;
    const uint8_t *w = nullptr;
    int16_t *T;

    __device__ __forceinline__ HpColCost(const HpCol &c, int32_t j, const uint8_t *site_gt, uint32_t G, const uint8_t *colw, int16_t *T_)
        : m0(c.m0), m1(c.m1), T(T_)
    {
        if constexpr (W) {
            w = colw + 16 * (int64_t)j;
            for (int s = 0; s < HP_SLOTS; s++) {
                c0 += (m0 >> s) & 1 ? w[s] : 0;
                c1 += (m1 >> s) & 1 ? w[s] : 0;
            }
        } else {
            c0 = __popc(m0);
            c1 = __popc(m1);
        }
        if constexpr (GT) {
            gt = site_gt[j];
            hadd = gt == 0 ? 0u : G;
            homA = c1 + (gt == 1 ? 0u : G);
            homB = c0 + (gt == 2 ? 0u : G);
        }
    }

    // (W) threads 0 .. HP_WTAB - 1 write the column's tables; a barrier lies between this and the first pair()
    __device__ __forceinline__ void fill_table(int tid) const
    {
        if constexpr (W) {
            if (tid < HP_WTAB) {
                const uint32_t x = tid < 256 ? (uint32_t)tid : (uint32_t)(tid - 256) << 8;
                int32_t t = 0;
                for (int s = 0; s < HP_SLOTS; s++)
                    if ((x >> s) & 1) t += (m1 >> s) & 1 ? (int32_t)w[s] : ((m0 >> s) & 1 ? -(int32_t)w[s] : 0);
                T[tid] = (int16_t)t;
            }
        }
    }

    // (e0, e1) of B on the parallel path: (W) e1 = C(m0) + T(B), e0 = C(m1) - T(B) from the tables of this column
    __device__ __forceinline__ void pair(uint32_t B, uint32_t &e0, uint32_t &e1) const
    {
        if constexpr (W) {
            const int32_t tb = T[B & 255] + T[256 + (B >> 8)];
            e1 = (uint32_t)((int32_t)c0 + tb);
            e0 = (uint32_t)((int32_t)c1 - tb);
        } else {
            e0 = __popc(m1 & ~B) + __popc(m0 & B);
            e1 = __popc(m0 & ~B) + __popc(m1 & B);
        }
    }

    // the same on the traceback's one thread, where the tables hold another column: (W) slot by slot
    __device__ __forceinline__ void pair_by_slots(uint32_t B, uint32_t &e0, uint32_t &e1) const
    {
        if constexpr (W) {
            e0 = e1 = 0;
            for (int s = 0; s < HP_SLOTS; s++) {
                const uint32_t b = 1u << s, v = w[s];
                if (m0 & b) (B & b ? e0 : e1) += v;
                if (m1 & b) (B & b ? e1 : e0) += v;
            }
        } else {
            pair(B, e0, e1);
        }
    }

    __device__ __forceinline__ uint32_t cost(uint32_t B) const
    {
        uint32_t e0, e1;
        pair(B, e0, e1);
        return GT ? min(min(e0, e1) + hadd, min(homA, homB)) : min(e0, e1);
    }

    // the traceback's outcome at B: the site's bit, and (GT) the class of the smallest (cost, pref): pref 0 for the called class, else 1 het,
    // 2 homozygous first, 3 homozygous second
    __device__ __forceinline__ void outcome(uint32_t B, int32_t j, uint8_t *colh, uint8_t *colg) const
    {
        uint32_t e0, e1;
        pair_by_slots(B, e0, e1);
        colh[j] = e0 <= e1 ? 0 : 1;
        if constexpr (GT) {
            const uint32_t cost[3] = {min(e0, e1) + hadd, homA, homB};
            uint32_t best = ~0u;
            for (uint32_t o = 0; o < 3; o++) best = min(best, (cost[o] << 4) | ((o == gt ? 0u : o + 1) << 2) | o);
            colg[j] = (uint8_t)(best & 3);
        }
    }
};

__device__ __forceinline__ uint32_t hp_pdep(uint32_t t, uint32_t mask)
{
    uint32_t r = 0;
    for (uint32_t m = mask; m; m &= m - 1) {
        if (t & 1) r |= m & (0u - m);
        t >>= 1;
    }
    return r;
}

__device__ __forceinline__ uint32_t hp_pext(uint32_t x, uint32_t mask)
{
    uint32_t r = 0;
    int k = 0;
    for (uint32_t m = mask; m; m &= m - 1, k++)
        if (x & m & (0u - m)) r |= 1u << k;
    return r;
}

__device__ __forceinline__ uint32_t hp_wave_min(uint32_t v)
{
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// one thread per kept read; codes of read r at position p: codes[slot_off[r] + (start & 15) + p - start]
template <bool FILL>
__global__ __launch_bounds__(256) void k_hp_gather(const uint8_t *__restrict__ codes, int32_t n_reads, const int32_t *__restrict__ rs,
                                                   const int32_t *__restrict__ re, const int64_t *__restrict__ slot_off, int32_t n_sites,
                                                   const int32_t *__restrict__ spos, const uint8_t *__restrict__ sal, int32_t *__restrict__ cnt,
                                                   const int64_t *__restrict__ off, int32_t *__restrict__ esite, uint8_t *__restrict__ eal)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const int32_t s0 = rs[r], s1 = re[r];
    const int64_t base = slot_off[r] + (s0 & 15);
    int32_t n = 0;
    int64_t o = FILL ? off[r] : 0;
    for (int32_t s = hp_lower_bound(spos, 0, n_sites, s0); s < n_sites && spos[s] < s1; s++) {
        const uint8_t c = codes[base + (spos[s] - s0)];
        const int a = c == sal[2 * s] ? 0 : (c == sal[2 * s + 1] ? 1 : -1);
        if (a < 0) continue;
        if (FILL) {
            esite[o] = s;
            eal[o] = (uint8_t)a;
            o++;
        } else {
            n++;
        }
    }
    if (!FILL) cnt[r] = n;
}

// One workgroup per block [bfirst, blast] of columns (= sites).  D(j, B) for the subsets B of the active slots lives in LDS as
// uint16 relative to the column minimum (the minima are summed into the block's cost); P(b) for the subsets of the continuing
// slots, the backtrace (smallest minimising bits of the leaving slots) per (column, continuing subset) in HBM at bt_off[column].
// GT: the genotype-aware form (site_gt[column] = the called class; gt_cost = the price G of leaving it; colg[column] = the outcome, classed
// as the called class is).  The plain form reads neither argument.
// W: the weighted form (colw[16 * column + slot] = the weight of the slot's allele at the column; unit costs read no weight).
template <bool GT, bool W>
__global__ __launch_bounds__(HP_THREADS) void k_hp_dp(const HpCol *__restrict__ cols, const int32_t *__restrict__ bfirst, const int32_t *__restrict__ blast,
                                                       const int64_t *__restrict__ bt_off, uint16_t *__restrict__ bt, uint16_t *__restrict__ colB,
                                                       uint8_t *__restrict__ colh, int64_t *__restrict__ bcost, int32_t *__restrict__ overflow,
                                                       const uint8_t *__restrict__ site_gt, uint8_t *__restrict__ colg, uint32_t gt_cost,
                                                       const uint8_t *__restrict__ colw)
{
    int16_t *const T = hp_wtab<W>();
    __shared__ uint16_t D[HP_STATES];
    __shared__ uint16_t P[HP_STATES];
    __shared__ uint32_t red[HP_THREADS];
    __shared__ uint32_t smin;
    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t c0 = bfirst[blockIdx.x], c1 = blast[blockIdx.x];
    int64_t total = 0;
    uint32_t prevA = 0;
    for (int32_t j = c0; j <= c1; j++) {
        const HpCol c = cols[j];
        const uint32_t A = c.act, K = c.keep;
        const HpColCost<GT, W> col(c, j, site_gt, gt_cost, colw, T);
        col.fill_table(tid);                                             // (the previous column's readers are behind the loop's last barrier)
        if (j > c0) {
            const uint32_t Lm = prevA & ~K;
            const int nk = __popc(K), nl = __popc(Lm);
            const int32_t NT = 1 << nk, NU = 1 << nl;
            uint16_t *btj = bt + bt_off[j];
            if (NT >= HP_THREADS) {
                for (int32_t t = tid; t < NT; t += HP_THREADS) {
                    const uint32_t b = hp_pdep(t, K);
                    uint32_t best = ~0u;
                    for (int32_t u = 0; u < NU; u++) {
                        const uint32_t x = hp_pdep(u, Lm);
                        best = min(best, ((uint32_t)D[b | x] << 16) | x);
                    }
                    P[b] = (uint16_t)(best >> 16);
                    btj[t] = (uint16_t)(best & 0xFFFF);
                }
            } else {
                // fewer continuing subsets than threads: G = 1024 / NT threads share one subset's leaving-slot loop
                const int32_t t = tid & (NT - 1), g = tid >> nk, G = HP_THREADS >> nk;
                if (tid < NT) red[tid] = ~0u;
                __syncthreads();
                const uint32_t b = hp_pdep(t, K);
                uint32_t best = ~0u;
                for (int32_t u = g; u < NU; u += G) {
                    const uint32_t x = hp_pdep(u, Lm);
                    best = min(best, ((uint32_t)D[b | x] << 16) | x);
                }
                if (best != ~0u) atomicMin(&red[t], best);
                __syncthreads();
                if (tid < NT) {
                    P[hp_pdep(tid, K)] = (uint16_t)(red[tid] >> 16);
                    btj[tid] = (uint16_t)(red[tid] & 0xFFFF);
                }
            }
        }
        if (tid == 0) smin = ~0u;
        __syncthreads();
        const int32_t NA = 1 << __popc(A);
        const bool first = j == c0;
        uint32_t mn = ~0u;
        for (int32_t t = tid; t < NA; t += HP_THREADS) {
            const uint32_t B = hp_pdep(t, A);
            mn = min(mn, (first ? 0u : (uint32_t)P[B & K]) + col.cost(B));
        }
        mn = hp_wave_min(mn);
        if (lane == 0 && mn != ~0u) atomicMin(&smin, mn);
        __syncthreads();
        const uint32_t cmin = smin;
        for (int32_t t = tid; t < NA; t += HP_THREADS) {
            const uint32_t B = hp_pdep(t, A);
            const uint32_t v = (first ? 0u : (uint32_t)P[B & K]) + col.cost(B) - cmin;
            if (v > 0xFFFFu) atomicOr(overflow, 1);
            D[B] = (uint16_t)min(v, 0xFFFFu);
        }
        total += cmin;
        prevA = A;
        __syncthreads();
    }
    // the smallest B among the minima of the last column (its minimum is 0 after the shift)
    if (tid == 0) smin = ~0u;
    __syncthreads();
    {
        const uint32_t A = cols[c1].act;
        const int32_t NA = 1 << __popc(A);
        uint32_t mn = ~0u;
        for (int32_t t = tid; t < NA; t += HP_THREADS) {
            const uint32_t B = hp_pdep(t, A);
            mn = min(mn, ((uint32_t)D[B] << 16) | B);
        }
        mn = hp_wave_min(mn);
        if (lane == 0 && mn != ~0u) atomicMin(&smin, mn);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t B = smin & 0xFFFF;
        for (int32_t j = c1; j >= c0; j--) {
            const HpCol c = cols[j];
            colB[j] = (uint16_t)B;
            HpColCost<GT, W>(c, j, site_gt, gt_cost, colw, T).outcome(B, j, colh, colg);
            if (j > c0) {
                const uint32_t bk = B & c.keep;
                B = bk | bt[bt_off[j] + hp_pext(bk, c.keep)];
            }
        }
        bcost[blockIdx.x] = total;
    }
}

// sblk: block of a PHASED site, -1 otherwise (sites are contiguous per block: a read's entries of one block form one run)
// W: an entry scores its weight ew[e] instead of 1
template <bool W>
__device__ void hp_block_score(int32_t r, int32_t b, const int64_t *off, const int32_t *esite, const uint8_t *eal, const uint8_t *ew, const int32_t *sblk,
                               const uint8_t *sh, const int32_t *bfirst, const int32_t *blast, int32_t &n, int32_t &s)
{
    const int64_t e0 = off[r], e1 = off[r + 1];
    int64_t lo = e0, hi = e1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (esite[mid] < bfirst[b]) lo = mid + 1;
        else hi = mid;
    }
    for (int64_t e = lo; e < e1 && esite[e] <= blast[b]; e++) {
        const int32_t site = esite[e];
        if (sblk[site] != b) continue;
        n++;
        const int32_t v = W ? (int32_t)ew[e] : 1;
        s += eal[e] == sh[site] ? v : -v;
    }
}

template <bool W>
__global__ __launch_bounds__(256) void k_hp_tag(int32_t n_groups, const int32_t *__restrict__ goff, const int32_t *__restrict__ greads,
                                                const int64_t *__restrict__ off, const int32_t *__restrict__ esite, const uint8_t *__restrict__ eal,
                                                const uint8_t *__restrict__ ew, const int32_t *__restrict__ sblk, const uint8_t *__restrict__ sh, const int32_t *__restrict__ bfirst,
                                                const int32_t *__restrict__ blast, const int32_t *__restrict__ bps, uint8_t *__restrict__ ghp,
                                                int32_t *__restrict__ gps)
{
    const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    int32_t best_n = 0, best_s = 0, best_ps = INT_MAX;
    for (int32_t ia = goff[g]; ia < goff[g + 1]; ia++) {
        const int32_t r = greads[ia];
        for (int64_t e = off[r]; e < off[r + 1];) {
            const int32_t b = sblk[esite[e]];
            if (b < 0) {
                e++;
                continue;
            }
            while (e < off[r + 1] && esite[e] <= blast[b]) e++;          // the rest of the read's run in block b
            bool seen = false;                                          // scored already from an earlier alignment of the name
            for (int32_t ib = goff[g]; ib < ia && !seen; ib++) {
                int32_t n = 0, s = 0;
                hp_block_score<W>(greads[ib], b, off, esite, eal, ew, sblk, sh, bfirst, blast, n, s);
                seen = n > 0;
            }
            if (seen) continue;
            int32_t n = 0, s = 0;
            for (int32_t ib = goff[g]; ib < goff[g + 1]; ib++) hp_block_score<W>(greads[ib], b, off, esite, eal, ew, sblk, sh, bfirst, blast, n, s);
            if (n > best_n || (n == best_n && bps[b] < best_ps)) {
                best_n = n;
                best_s = s;
                best_ps = bps[b];
            }
        }
    }
    const uint8_t hp = best_n == 0 || best_s == 0 ? 0 : (best_s > 0 ? 1 : 2);
    ghp[g] = hp;
    gps[g] = hp ? best_ps : 0;
}

}  // namespace

static void hp_free_dev(nc_phase *ph)
{
    if (ph->d_off) (void)hipFree(ph->d_off);
    if (ph->d_site) (void)hipFree(ph->d_site);
    if (ph->d_al) (void)hipFree(ph->d_al);
    if (ph->d_w) (void)hipFree(ph->d_w);
    ph->d_w = nullptr;
    ph->d_off = nullptr;
    ph->d_site = nullptr;
    ph->d_al = nullptr;
}

extern "C" {

int nc_snp_phase_gather(nc_ctx *ctx, const uint8_t *codes, int64_t codes_len, int32_t n_reads, const int32_t *rd_start, const int32_t *rd_end,
                        const int64_t *slot_off, int32_t n_sites, const int32_t *site_pos, const uint8_t *site_alleles, nc_phase **out)
{
    if (!ctx || !out || n_reads < 0 || n_sites < 0 || (n_reads && (!codes || !rd_start || !rd_end || !slot_off)) || (n_sites && (!site_pos || !site_alleles)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_gather: bad argument");
    (void)codes_len;
    *out = nullptr;
    const double t0 = hp_now_ms();
    nc_phase *ph = nullptr;
    NC_TRY(hp_new_handle(ctx, n_reads, n_sites, site_pos, &ph));
    HpErr hip{ctx};
    {
        HpScratch sc;
        int32_t *d_spos = nullptr, *d_cnt = nullptr;
        uint8_t *d_sal = nullptr;
        if ((hip.rc = sc.get(ctx, &d_spos, n_sites + 1)) || (hip.rc = sc.get(ctx, &d_sal, 2 * (size_t)n_sites + 2)) || (hip.rc = sc.get(ctx, &d_cnt, n_reads + 1))) {
            nc_snp_phase_free(ph);
            return hip.rc;
        }
        hip(hipMalloc(&ph->d_off, (n_reads + 1) * sizeof(int64_t)), "hipMalloc(offsets)");
        if (n_sites && hip.rc == NC_OK) {
            hip(hipMemcpyAsync(d_spos, site_pos, n_sites * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "site upload");
            hip(hipMemcpyAsync(d_sal, site_alleles, 2 * (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream), "allele upload");
        }
        const int nb = (n_reads + 255) / 256;
        if (n_reads && hip.rc == NC_OK) {
            k_hp_gather<false><<<nb, 256, 0, ctx->stream>>>(codes, n_reads, rd_start, rd_end, slot_off, n_sites, d_spos, d_sal, d_cnt, nullptr, nullptr, nullptr);
            hip(hipGetLastError(), "k_hp_gather (count)");
        }
        hp_entries_from_counts(ph, hip, d_cnt, "gather sync", nullptr, nullptr, [&] {
            k_hp_gather<true><<<nb, 256, 0, ctx->stream>>>(codes, n_reads, rd_start, rd_end, slot_off, n_sites, d_spos, d_sal, nullptr, ph->d_off, ph->d_site, ph->d_al);
            hip(hipGetLastError(), "k_hp_gather (fill)");
        });
    }
    if (hip.rc != NC_OK) {
        nc_snp_phase_free(ph);
        return hip.rc;
    }
    ph->ms[0] = (float)(hp_now_ms() - t0);
    *out = ph;
    return NC_OK;
}

int nc_snp_phase_load(nc_ctx *ctx, int32_t n_reads, int32_t n_sites, const int32_t *site_pos, const int64_t *entry_off, const int32_t *entry_site,
                      const uint8_t *entry_allele, nc_phase **out)
{
    if (!ctx || !out || n_reads < 0 || n_sites < 0 || !entry_off || (n_sites && !site_pos)) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_load: bad argument");
    *out = nullptr;
    nc_phase *ph = nullptr;
    NC_TRY(hp_new_handle(ctx, n_reads, n_sites, site_pos, &ph));
    int rc = entry_off[0] != 0 ? nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_load: entry_off[0] != 0") : NC_OK;
    for (int32_t r = 0; r < n_reads && rc == NC_OK; r++) {
        if (entry_off[r + 1] < entry_off[r]) rc = nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_load: offsets descend at read %d", r);
        for (int64_t e = entry_off[r]; e < entry_off[r + 1] && rc == NC_OK; e++)
            if (entry_site[e] < 0 || entry_site[e] >= n_sites || entry_allele[e] > 1 || (e > entry_off[r] && entry_site[e] <= entry_site[e - 1]))
                rc = nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_load: read %d: sites must ascend inside [0, n_sites), alleles 0 / 1", r);
    }
    if (rc == NC_OK) {
        ph->off.assign(entry_off, entry_off + n_reads + 1);
        ph->esite.assign(entry_site, entry_site + entry_off[n_reads]);
        ph->eal.assign(entry_allele, entry_allele + entry_off[n_reads]);
        rc = hp_upload_csr(ph);
    }
    if (rc != NC_OK) {
        nc_snp_phase_free(ph);
        return rc;
    }
    *out = ph;
    return NC_OK;
}

}  // extern "C"

// ---- the solve (DESIGN.md "Read-based phasing", steps 2 to 6), one step per function; every order and tie-break below is part of the algorithm
namespace {

using HpDpKernel = decltype(&k_hp_dp<false, false>);
const HpDpKernel hp_dp_kernel[2][2] = {{k_hp_dp<false, false>, k_hp_dp<false, true>}, {k_hp_dp<true, false>, k_hp_dp<true, true>}};      // [gt][weighted]

struct HpSolve {
    nc_ctx *ctx;
    nc_phase *ph;
    const int32_t R, S;
    const std::vector<int64_t> &off;
    const std::vector<int32_t> &es;
    // what the steps hand on
    std::vector<uint8_t> acc;          // per read: accepted by read selection
    std::vector<std::vector<int32_t>> enter, ending;     // per site: the accepted reads whose span starts / ends there, in read-index order
    std::vector<int8_t> slot;          // per accepted read: its slot 0 .. 14
    std::vector<HpCol> cols;           // per site (one spare)
    std::vector<uint8_t> colw;         // weighted: 16 per site, the weight of every slot's allele
    std::vector<int64_t> bt_off;       // per site: where the column's backtrace starts; bt_total entries in all
    int64_t bt_total = 0;
    std::vector<uint16_t> colB;        // the device run's traceback per site: the partition, the site's bit, (genotype-aware) the outcome
    std::vector<uint8_t> colh, colg;

    HpSolve(nc_ctx *c, nc_phase *p) : ctx(c), ph(p), R(p->n_reads), S(p->n_sites), off(p->off), es(p->esite) {}

    // read selection: most informative sites first, then the first site, then the read index
    void select_reads(int32_t max_cov)
    {
        std::vector<int32_t> order;
        for (int32_t r = 0; r < R; r++)                                  // (a read the MAPQ floor refuses is never accepted)
            if (off[r + 1] - off[r] >= 2 && (!ph->weighted || ph->rok[r])) order.push_back(r);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            const int64_t na = off[a + 1] - off[a], nb = off[b + 1] - off[b];
            if (na != nb) return na > nb;
            if (es[off[a]] != es[off[b]]) return es[off[a]] < es[off[b]];
            return a < b;
        });
        std::vector<int32_t> cov(S, 0);
        acc.assign(R, 0);
        for (int32_t r : order) {
            const int32_t a = es[off[r]], b = es[off[r + 1] - 1];
            bool ok = true;
            for (int32_t s = a; s <= b && ok; s++) ok = cov[s] < max_cov;
            if (!ok) continue;
            for (int32_t s = a; s <= b; s++) cov[s]++;
            acc[r] = 1;
        }
    }

    // the handle's result as that of a contig without blocks: nothing phased, no read placed; (genotype-aware) every outcome the call
    void reset_result(const uint8_t *site_gt)
    {
        ph->site_block.assign(S, -1);
        ph->site_h.assign(S, 0);
        ph->site_phased.assign(S, 0);
        ph->site_ps.assign(S, 0);
        ph->site_gt.clear();
        if (site_gt) ph->site_gt.assign(site_gt, site_gt + S);
        ph->side.assign(R, -1);
        ph->block_first.clear();
        ph->block_last.clear();
        ph->block_ps.clear();
    }

    // blocks: consecutive sites share a block when an accepted span covers both
    void cut_blocks()
    {
        std::vector<int32_t> link(S + 1, 0);
        enter.assign(S, {});
        for (int32_t r = 0; r < R; r++) {
            if (!acc[r]) continue;
            const int32_t a = es[off[r]], b = es[off[r + 1] - 1];
            link[a]++;
            link[b]--;                               // link[i] > 0 after the prefix: sites i and i + 1 joined
            enter[a].push_back(r);
        }
        for (int32_t s = 1; s <= S; s++) link[s] += link[s - 1];
        for (int32_t s = 0; s < S;) {
            if (link[s] <= 0) {
                s++;
                continue;
            }
            int32_t e = s;
            while (e < S && link[e] > 0) e++;        // sites s .. e form a block
            ph->block_first.push_back(s);
            ph->block_last.push_back(e);
            s = e + 1;
        }
    }

    // slots: a read entering at a column takes the lowest free slot, in read-index order; the column's act / keep
    int assign_slots()
    {
        ending.assign(S, {});
        cols.assign(S + 1, HpCol{0, 0, 0, 0});
        slot.assign(R, -1);
        for (size_t bi = 0; bi < ph->block_first.size(); bi++) {
            uint32_t freem = (1u << HP_SLOTS) - 1, act = 0;
            for (int32_t c = ph->block_first[bi]; c <= ph->block_last[bi]; c++) {
                ph->site_block[c] = (int32_t)bi;
                if (c > ph->block_first[bi])
                    for (int32_t r : ending[c - 1]) {
                        freem |= 1u << slot[r];
                        act &= ~(1u << slot[r]);
                    }
                uint32_t entering = 0;
                for (int32_t r : enter[c]) {
                    if (!freem) return nc_fail(ctx, NC_ERR_STATE, "nc_snp_phase_solve: more than %d reads active", HP_SLOTS);
                    const int sl = __builtin_ctz(freem);
                    freem &= freem - 1;
                    slot[r] = (int8_t)sl;
                    entering |= 1u << sl;
                    ending[es[off[r + 1] - 1]].push_back(r);
                }
                act |= entering;
                cols[c].act = (uint16_t)act;
                cols[c].keep = (uint16_t)(act & ~entering);
            }
        }
        return NC_OK;
    }

    // a column's allele masks and (weighted) slot weights from the accepted reads' entries; a site with an accepted allele counts as phased
    void fill_masks()
    {
        // plain pointers: through the members, with byte stores in the loop, this step measured 1 ms slower on the 1.8 M entries of a chr20-sized contig
        HpCol *col = cols.data();
        uint8_t *phased = ph->site_phased.data();
        const uint8_t *al = ph->eal.data();
        const int32_t *site = es.data();
        for (int32_t r = 0; r < R; r++) {
            if (!acc[r]) continue;
            const int sl = slot[r];
            for (int64_t e = off[r], e1 = off[r + 1]; e < e1; e++) {
                const int32_t c = site[e];
                (al[e] ? col[c].m1 : col[c].m0) |= (uint16_t)(1u << sl);
                phased[c] = 1;
            }
        }
        if (!ph->weighted) return;
        colw.assign(16 * (size_t)(S + 1), 0);
        uint8_t *cw = colw.data();
        const uint8_t *ew = ph->ew.data();
        for (int32_t r = 0; r < R; r++)
            if (acc[r])
                for (int64_t e = off[r], e1 = off[r + 1]; e < e1; e++) cw[16 * (size_t)site[e] + slot[r]] = ew[e];
    }

    // the backtrace of a block's columns behind its first: one entry per subset of the continuing slots
    void layout_backtrace()
    {
        bt_off.assign(S + 1, 0);
        for (size_t bi = 0; bi < ph->block_first.size(); bi++)
            for (int32_t c = ph->block_first[bi] + 1; c <= ph->block_last[bi]; c++) {
                bt_off[c] = bt_total;
                bt_total += 1ll << __builtin_popcount(cols[c].keep);
            }
    }

    // the device run, one workgroup per block (not launched where no block formed) -> block_cost and the traceback per site
    // site_gt: null for the plain form; else the called class of every site, and gt_cost the price of leaving it
    int run_dp(const uint8_t *site_gt, int32_t gt_cost)
    {
        const int32_t nblk = (int32_t)ph->block_first.size();
        colB.assign(S + 1, 0);
        colh.assign(S + 1, 0);
        colg.assign(S + 1, 0);
        ph->block_cost.assign(nblk, 0);
        if (!nblk) return NC_OK;
        int32_t overflow = 0;
        HpScratch sc;
        HpCol *d_cols = nullptr;
        int32_t *d_bf = nullptr, *d_bl = nullptr, *d_ovf = nullptr;
        int64_t *d_bto = nullptr, *d_cost = nullptr;
        uint16_t *d_bt = nullptr, *d_colB = nullptr;
        uint8_t *d_colh = nullptr, *d_colw = nullptr, *d_gt = nullptr, *d_colg = nullptr;
        NC_TRY(sc.get(ctx, &d_cols, S + 1));
        NC_TRY(sc.get(ctx, &d_bf, nblk));
        NC_TRY(sc.get(ctx, &d_bl, nblk));
        NC_TRY(sc.get(ctx, &d_ovf, 1));
        NC_TRY(sc.get(ctx, &d_bto, S + 1));
        NC_TRY(sc.get(ctx, &d_cost, nblk));
        NC_TRY(sc.get(ctx, &d_bt, bt_total + 1));
        NC_TRY(sc.get(ctx, &d_colB, S + 1));
        NC_TRY(sc.get(ctx, &d_colh, S + 1));
        NC_HIP(ctx, hipMemcpyAsync(d_cols, cols.data(), (S + 1) * sizeof(HpCol), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_bf, ph->block_first.data(), nblk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_bl, ph->block_last.data(), nblk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_bto, bt_off.data(), (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemsetAsync(d_ovf, 0, sizeof(int32_t), ctx->stream));
        if (site_gt) {
            NC_TRY(sc.get(ctx, &d_gt, S + 1));
            NC_TRY(sc.get(ctx, &d_colg, S + 1));
            NC_HIP(ctx, hipMemcpyAsync(d_gt, site_gt, S, hipMemcpyHostToDevice, ctx->stream));
        }
        if (ph->weighted) {
            NC_TRY(sc.get(ctx, &d_colw, colw.size()));
            NC_HIP(ctx, hipMemcpyAsync(d_colw, colw.data(), colw.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        hp_dp_kernel[site_gt != nullptr][ph->weighted]<<<nblk, HP_THREADS, 0, ctx->stream>>>(d_cols, d_bf, d_bl, d_bto, d_bt, d_colB, d_colh, d_cost, d_ovf, d_gt,
                                                                                             d_colg, (uint32_t)gt_cost, d_colw);
        NC_HIP(ctx, hipGetLastError());
        NC_HIP(ctx, hipMemcpyAsync(colB.data(), d_colB, (S + 1) * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(colh.data(), d_colh, S + 1, hipMemcpyDeviceToHost, ctx->stream));
        if (site_gt) NC_HIP(ctx, hipMemcpyAsync(colg.data(), d_colg, S + 1, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(ph->block_cost.data(), d_cost, nblk * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(&overflow, d_ovf, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (overflow) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_snp_phase_solve: a partition cost exceeds 65535 above its column's minimum");
        return NC_OK;
    }

    // the traceback into the handle: site_h, (genotype-aware) the outcomes, site_phased, the phase sets, the reads' sides
    void write_back(const uint8_t *site_gt)
    {
        for (int32_t s = 0; s < S; s++) ph->site_h[s] = ph->site_block[s] >= 0 ? colh[s] : 0;
        if (site_gt)                                                     // a site is phased when it has an accepted allele and comes out het
            for (int32_t s = 0; s < S; s++) {
                if (ph->site_block[s] >= 0) ph->site_gt[s] = colg[s];
                if (ph->site_gt[s] != 0) ph->site_phased[s] = 0;
            }
        for (size_t bi = 0; bi < ph->block_first.size(); bi++) {
            int32_t ps = 0;
            for (int32_t c = ph->block_first[bi]; c <= ph->block_last[bi] && !ps; c++)
                if (ph->site_phased[c]) ps = ph->site_pos[c];
            ph->block_ps.push_back(ps);
            for (int32_t c = ph->block_first[bi]; c <= ph->block_last[bi]; c++)
                if (ph->site_phased[c]) ph->site_ps[c] = ps;
        }
        for (int32_t r = 0; r < R; r++)
            if (acc[r]) ph->side[r] = (int8_t)((colB[es[off[r]]] >> slot[r]) & 1);
    }
};

int hp_solve(nc_ctx *ctx, nc_phase *ph, int32_t max_cov, const uint8_t *site_gt, int32_t gt_cost)
{
    const double t0 = hp_now_ms();
    ph->solved = false;                                                  // a solve that fails leaves the handle unsolved: its earlier result is reset below
    ph->n_groups = 0;                                                    // (the haplotags of an earlier solve go with it)
    ph->group_hp.clear();
    ph->group_ps.clear();
    HpSolve sv(ctx, ph);
    sv.select_reads(max_cov);
    sv.reset_result(site_gt);
    sv.cut_blocks();
    NC_TRY(sv.assign_slots());
    sv.fill_masks();
    sv.layout_backtrace();
    ph->ms[1] = (float)(hp_now_ms() - t0);
    const double t1 = hp_now_ms();
    NC_TRY(sv.run_dp(site_gt, gt_cost));
    sv.write_back(site_gt);
    ph->ms[2] = (float)(hp_now_ms() - t1);
    ph->solved = true;
    return NC_OK;
}

}  // namespace

extern "C" {

int nc_snp_phase_solve(nc_ctx *ctx, nc_phase *ph, int32_t max_cov)
{
    if (!ctx || !ph || max_cov < 1 || max_cov > HP_SLOTS) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_solve: max_cov must lie in [1, %d]", HP_SLOTS);
    return hp_solve(ctx, ph, max_cov, nullptr, 0);
}

int nc_snp_phase_solve_gt(nc_ctx *ctx, nc_phase *ph, int32_t max_cov, const uint8_t *site_gt, int32_t gt_cost)
{
    if (!ctx || !ph || max_cov < 1 || max_cov > HP_SLOTS) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_solve_gt: max_cov must lie in [1, %d]", HP_SLOTS);
    if ((ph->n_sites && !site_gt) || gt_cost < 1 || gt_cost > HP_GT_COST_MAX)
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_solve_gt: site_gt missing or gt_cost outside [1, %d]", HP_GT_COST_MAX);
    for (int32_t s = 0; s < ph->n_sites; s++)
        if (site_gt[s] > 2) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_solve_gt: site %d: class %d is not 0 (het), 1 or 2 (homozygous)", s, site_gt[s]);
    return hp_solve(ctx, ph, max_cov, site_gt, gt_cost);
}

int nc_haplotag_run(nc_ctx *ctx, nc_phase *ph, int32_t n_groups, const int32_t *read_group)
{
    if (!ctx || !ph || n_groups < 0 || (ph->n_reads && !read_group)) return nc_fail(ctx, NC_ERR_ARG, "nc_haplotag_run: bad argument");
    if (!ph->solved) return nc_fail(ctx, NC_ERR_STATE, "nc_haplotag_run before nc_snp_phase_solve");
    const double t0 = hp_now_ms();
    const int32_t R = ph->n_reads, S = ph->n_sites, nblk = (int32_t)ph->block_first.size();
    std::vector<int32_t> goff(n_groups + 2, 0), greads(R + 1, 0);
    for (int32_t r = 0; r < R; r++) {
        if (read_group[r] < 0 || read_group[r] >= n_groups) return nc_fail(ctx, NC_ERR_ARG, "nc_haplotag_run: read %d: group out of range", r);
        goff[read_group[r] + 1]++;
    }
    for (int32_t g = 0; g < n_groups; g++) goff[g + 1] += goff[g];
    {
        std::vector<int32_t> fill(goff.begin(), goff.end() - 1);
        for (int32_t r = 0; r < R; r++) greads[fill[read_group[r]]++] = r;
    }
    std::vector<int32_t> sblk(S + 1, -1);
    for (int32_t s = 0; s < S; s++)
        if (ph->site_phased[s]) sblk[s] = ph->site_block[s];
    ph->n_groups = n_groups;
    ph->group_hp.assign(n_groups, 0);
    ph->group_ps.assign(n_groups, 0);
    if (n_groups && nblk) {
        if (!ph->d_off) NC_TRY(hp_upload_csr(ph));
        if (ph->weighted && !ph->d_w) NC_TRY(hp_upload_weights(ph));
        HpScratch sc;
        int32_t *d_goff = nullptr, *d_gr = nullptr, *d_sblk = nullptr, *d_bf = nullptr, *d_bl = nullptr, *d_bps = nullptr, *d_gps = nullptr;
        uint8_t *d_sh = nullptr, *d_ghp = nullptr;
        NC_TRY(sc.get(ctx, &d_goff, n_groups + 1));
        NC_TRY(sc.get(ctx, &d_gr, R + 1));
        NC_TRY(sc.get(ctx, &d_sblk, S + 1));
        NC_TRY(sc.get(ctx, &d_sh, S + 1));
        NC_TRY(sc.get(ctx, &d_bf, nblk));
        NC_TRY(sc.get(ctx, &d_bl, nblk));
        NC_TRY(sc.get(ctx, &d_bps, nblk));
        NC_TRY(sc.get(ctx, &d_ghp, n_groups));
        NC_TRY(sc.get(ctx, &d_gps, n_groups));
        NC_HIP(ctx, hipMemcpyAsync(d_goff, goff.data(), (n_groups + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_gr, greads.data(), (R + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_sblk, sblk.data(), (S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (S) NC_HIP(ctx, hipMemcpyAsync(d_sh, ph->site_h.data(), S, hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_bf, ph->block_first.data(), nblk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_bl, ph->block_last.data(), nblk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(d_bps, ph->block_ps.data(), nblk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (ph->weighted)
            k_hp_tag<true><<<(n_groups + 255) / 256, 256, 0, ctx->stream>>>(n_groups, d_goff, d_gr, ph->d_off, ph->d_site, ph->d_al, ph->d_w, d_sblk, d_sh, d_bf,
                                                                           d_bl, d_bps, d_ghp, d_gps);
        else
            k_hp_tag<false><<<(n_groups + 255) / 256, 256, 0, ctx->stream>>>(n_groups, d_goff, d_gr, ph->d_off, ph->d_site, ph->d_al, nullptr, d_sblk, d_sh, d_bf,
                                                                            d_bl, d_bps, d_ghp, d_gps);
        NC_HIP(ctx, hipGetLastError());
        NC_HIP(ctx, hipMemcpyAsync(ph->group_hp.data(), d_ghp, n_groups, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(ph->group_ps.data(), d_gps, n_groups * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ph->ms[3] = (float)(hp_now_ms() - t0);
    return NC_OK;
}

int nc_snp_phase_view(const nc_phase *ph, nc_phase_arrays *out)
{
    if (!ph || !out) return NC_ERR_ARG;
    out->n_reads = ph->n_reads;
    out->n_sites = ph->n_sites;
    out->n_blocks = ph->solved ? (int32_t)ph->block_first.size() : 0;
    out->n_groups = ph->n_groups;
    out->n_entries = ph->off.empty() ? 0 : ph->off[ph->n_reads];
    out->entry_off = ph->off.data();
    out->entry_site = ph->esite.data();
    out->entry_allele = ph->eal.data();
    out->read_side = ph->solved ? ph->side.data() : nullptr;
    out->site_block = ph->solved ? ph->site_block.data() : nullptr;
    out->site_h = ph->solved ? ph->site_h.data() : nullptr;
    out->site_phased = ph->solved ? ph->site_phased.data() : nullptr;
    out->site_ps = ph->solved ? ph->site_ps.data() : nullptr;
    out->block_first = ph->solved ? ph->block_first.data() : nullptr;
    out->block_last = ph->solved ? ph->block_last.data() : nullptr;
    out->block_ps = ph->solved ? ph->block_ps.data() : nullptr;
    out->block_cost = ph->solved ? ph->block_cost.data() : nullptr;
    out->group_hp = ph->group_hp.data();
    out->group_ps = ph->group_ps.data();
    for (int k = 0; k < 4; k++) out->ms[k] = ph->ms[k];
    return NC_OK;
}

int nc_snp_phase_genotypes(const nc_phase *ph, const uint8_t **site_gt)
{
    if (!ph || !site_gt) return NC_ERR_ARG;
    *site_gt = ph->solved && !ph->site_gt.empty() ? ph->site_gt.data() : nullptr;
    return NC_OK;
}

int nc_snp_phase_free(nc_phase *ph)
{
    if (!ph) return NC_OK;
    hp_free_dev(ph);
    delete ph;
    return NC_OK;
}

}  // extern "C"

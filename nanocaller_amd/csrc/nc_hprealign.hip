// The phaser's allele detection by local realignment: nc_snp_phase_realign makes the handle nc_snp_phase_gather makes (nc_happhase.hip), with a
// read's allele at a site taken from the edit distance of its own bases around the site to the reference window carrying either allele.
// WhatsHap's realignment mode (its default overhang, unit-cost edit distance) restated: DESIGN.md "Read-based phasing", the allele
// detectors; tests/phase_realign_ref.py restates it in numpy with a plain dynamic-programming Levenshtein.
//
//   k_hr_sites          per site: its reference window (at most 21 columns, 3 bits each, in one word), once for all its reads
//   k_hr_span           per read: its first candidate site and the number of them (the sites inside [rd_start, rd_end))
//   k_hp_scan           read -> pair offsets
//   k_hr_align          one lane per (read, site) pair: the query window from the codes, the read's events and inserted bases; Myers'
//                       bit-vector edit distance (the query in one 64-bit word) against the window with either allele -> 0 / 1 / none
//   k_hr_compact<false> per read: the number of its pairs with an allele;  k_hp_scan: read -> entry offsets
//   k_hr_compact<true>  per read: the (site, allele) CSR entries, sites ascending
#include "nc_happhase.h"

#include <algorithm>

namespace {

constexpr int HR_OVERHANG = 10;
constexpr int HR_QMAX = 64;
constexpr uint8_t HR_NONE = 2;

struct HrSite {
    uint64_t bases;       // code of column lo + i in bits 3 i .. 3 i + 2
    int32_t lo;           // first column of the window (1-based)
    uint8_t n;            // columns; 0: the window holds an N, no read gets an entry here
    uint8_t c;            // index of the site's own column
    uint8_t a0, a1;
};

struct HrReads {
    const uint8_t *codes;
    int64_t codes_len;
    int32_t n_reads;
    const int32_t *rs, *re;
    const int64_t *slot_off;
    const int32_t *ev_off, *ev_pos, *ev_len, *ins_off;
    const uint8_t *ins_bases, *read_flag;
    int64_t n_events, n_ins;
};

__global__ __launch_bounds__(256) void k_hr_sites(int32_t n_sites, const int32_t *__restrict__ spos, const uint8_t *__restrict__ sal,
                                                  const uint8_t *__restrict__ ref, int32_t ref_len, HrSite *__restrict__ out)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_sites) return;
    const int32_t p = spos[s];                                      // (the host checked 1 <= p <= ref_len)
    const int32_t lo = max(1, p - HR_OVERHANG), hi = min(ref_len, p + HR_OVERHANG);
    HrSite st;
    st.bases = 0;
    st.lo = lo;
    st.n = (uint8_t)(hi - lo + 1);
    st.c = (uint8_t)(p - lo);
    st.a0 = sal[2 * s];
    st.a1 = sal[2 * s + 1];
    for (int32_t x = lo; x <= hi; x++) {
        const uint32_t c = ref[x - 1];
        if (c > 3) st.n = 0;
        st.bases |= (uint64_t)(c & 7) << (3 * (x - lo));
    }
    if (st.a0 > 3 || st.a1 > 3) st.n = 0;
    out[s] = st;
}

__global__ __launch_bounds__(256) void k_hr_span(int32_t n_reads, const int32_t *__restrict__ rs, const int32_t *__restrict__ re, int32_t n_sites,
                                                 const int32_t *__restrict__ spos, int32_t *__restrict__ first, int32_t *__restrict__ cnt)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const int32_t a = hp_lower_bound(spos, 0, n_sites, rs[r]);
    first[r] = a;
    cnt[r] = max(0, hp_lower_bound(spos, a, n_sites, re[r]) - a);
}

// one column of Myers' bit-vector edit distance, global form (the row above the matrix counts up by one a column): the query's bases are
// the bits of the word, eq = its positions that hold the column's base, top = the bit of its last base, sc = the matrix's last row
__device__ __forceinline__ void hr_step(uint64_t eq, uint64_t top, uint64_t &pv, uint64_t &mv, int32_t &sc)
{
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    sc += (ph & top) ? 1 : 0;
    sc -= (mh & top) ? 1 : 0;
    ph = (ph << 1) | 1;
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

__global__ __launch_bounds__(256) void k_hr_align(HrReads R, int64_t n_pairs, const int64_t *__restrict__ poff, const int32_t *__restrict__ first,
                                                  const HrSite *__restrict__ sites, uint8_t *__restrict__ pal, int32_t *__restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    int32_t lo_r = 0, hi_r = R.n_reads;                             // the read of pair i: the last r with poff[r] <= i
    while (hi_r - lo_r > 1) {
        const int32_t mid = (lo_r + hi_r) >> 1;
        if (poff[mid] <= i) lo_r = mid;
        else hi_r = mid;
    }
    const int32_t r = lo_r;
    const HrSite st = sites[first[r] + (int32_t)(i - poff[r])];
    const int32_t rs = R.rs[r], re = R.re[r];
    const int32_t lo = st.lo, hi = st.lo + st.n - 1;
    uint8_t res = HR_NONE;
    bool ok = st.n != 0 && rs <= lo && hi < re && !(R.read_flag && (R.read_flag[r] & 1));
    const int64_t cb = R.slot_off[r] - (rs & ~15);                  // the code of position x at codes[cb + x]
    const int32_t e0 = R.ev_off[r], e1 = R.ev_off[r + 1];
    if (ok && (cb + lo < 0 || cb + hi >= R.codes_len || e0 < 0 || e1 < e0 || e1 > R.n_events)) {
        atomicOr(status, 1);
        ok = false;
    }
    if (ok) {
        uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;                    // the query window: positions that hold base 0 .. 3 (a read's N matches nothing)
        int32_t m = 0;
        bool over = false;
        auto push = [&](uint32_t c) {
            if (m >= HR_QMAX) {
                over = true;
                return;
            }
            q0 |= (uint64_t)(c == 0) << m;
            q1 |= (uint64_t)(c == 1) << m;
            q2 |= (uint64_t)(c == 2) << m;
            q3 |= (uint64_t)(c == 3) << m;
            m++;
        };
        int32_t k = hp_lower_bound(R.ev_pos, e0, e1, lo);           // first event on a column >= lo
        int32_t del_until = 0;                                      // last column of the deletion that reaches into the window, if any
        if (k > e0 && R.ev_len[k - 1] < 0) del_until = R.ev_pos[k - 1] - R.ev_len[k - 1];
        for (int32_t x = lo; x <= hi && !over; x++) {
            if (x > del_until) push(R.codes[cb + x]);
            for (; k < e1 && R.ev_pos[k] <= x; k++) {
                if (R.ev_pos[k] != x) continue;                     // (events out of order: skipped, not followed)
                const int32_t el = R.ev_len[k];
                if (el < 0) {
                    del_until = max(del_until, x - el);
                } else if (el > 0 && x < hi) {                      // bases inserted between two columns of the window
                    const int32_t b0 = R.ins_off[k], b1 = R.ins_off[k + 1];
                    if (b0 < 0 || b1 < b0 || b1 > R.n_ins) {
                        atomicOr(status, 1);
                        over = true;
                        break;
                    }
                    if (b1 - b0 > HR_QMAX - m) over = true;
                    for (int32_t b = b0; b < b1 && !over; b++) push(R.ins_bases[b]);
                }
            }
        }
        if (!over && m > 0) {
            const uint64_t top = 1ull << (m - 1);
            auto eq_of = [&](uint32_t c) { return c == 0 ? q0 : c == 1 ? q1 : c == 2 ? q2 : c == 3 ? q3 : 0ull; };
            uint64_t pv = ~0ull, mv = 0;
            int32_t sc = m;
            const int32_t c = st.c, n = st.n;
            for (int32_t j = 0; j < c; j++) hr_step(eq_of((uint32_t)(st.bases >> (3 * j)) & 7), top, pv, mv, sc);      // the columns both windows share
            uint64_t pv1 = pv, mv1 = mv;
            int32_t sc1 = sc;
            hr_step(eq_of(st.a0), top, pv, mv, sc);
            hr_step(eq_of(st.a1), top, pv1, mv1, sc1);
            for (int32_t j = c + 1; j < n; j++) {
                const uint64_t eq = eq_of((uint32_t)(st.bases >> (3 * j)) & 7);
                hr_step(eq, top, pv, mv, sc);
                hr_step(eq, top, pv1, mv1, sc1);
            }
            res = sc < sc1 ? 0 : (sc1 < sc ? 1 : HR_NONE);
        }
    }
    pal[i] = res;
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_hr_compact(int32_t n_reads, const int64_t *__restrict__ poff, const int32_t *__restrict__ first,
                                                    const uint8_t *__restrict__ pal, int32_t *__restrict__ cnt, const int64_t *__restrict__ off,
                                                    int32_t *__restrict__ esite, uint8_t *__restrict__ eal)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const int64_t p0 = poff[r], p1 = poff[r + 1];
    int32_t n = 0;
    int64_t o = FILL ? off[r] : 0;
    for (int64_t i = p0; i < p1; i++) {
        const uint8_t a = pal[i];
        if (a == HR_NONE) continue;
        if (FILL) {
            esite[o] = first[r] + (int32_t)(i - p0);
            eal[o] = a;
            o++;
        } else {
            n++;
        }
    }
    if (!FILL) cnt[r] = n;
}

}  // namespace

extern "C" {

int nc_snp_phase_realign(nc_ctx *ctx, const uint8_t *codes, int64_t codes_len, const nc_indel_reads *reads, int64_t n_events, int64_t n_ins_bases,
                         const uint8_t *ref_code, int32_t ref_len, int32_t n_sites, const int32_t *site_pos, const uint8_t *site_alleles, nc_phase **out)
{
    if (!ctx || !out || !reads || reads->n_reads < 0 || n_sites < 0 || n_events < 0 || n_ins_bases < 0 || ref_len < 0 || codes_len < 0 ||
        (n_sites && (!site_pos || !site_alleles || !ref_code)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_realign: bad argument");
    const int32_t n_reads = reads->n_reads;
    if (n_reads && (!codes || !reads->rd_start || !reads->rd_end || !reads->slot_off || !reads->ev_off || (n_events && (!reads->ev_pos || !reads->ev_len || !reads->ins_off)) ||
                    (n_ins_bases && !reads->ins_bases)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_realign: the read table lacks the events or the inserted bases");
    *out = nullptr;
    const double t0 = hp_now_ms();
    nc_phase *ph = nullptr;
    NC_TRY(hp_new_handle(ctx, n_reads, n_sites, site_pos, &ph));
    if (n_sites && (site_pos[0] < 1 || site_pos[n_sites - 1] > ref_len)) {
        nc_snp_phase_free(ph);
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_realign: a site lies outside [1, %d]", ref_len);
    }
    HpErr hip{ctx};
    {
        HpScratch sc;
        int32_t *d_spos = nullptr, *d_cnt = nullptr, *d_first = nullptr, *d_status = nullptr;
        uint8_t *d_sal = nullptr, *d_pal = nullptr;
        int64_t *d_poff = nullptr;
        HrSite *d_sites = nullptr;
        if ((hip.rc = sc.get(ctx, &d_spos, n_sites + 1)) || (hip.rc = sc.get(ctx, &d_sal, 2 * (size_t)n_sites + 2)) || (hip.rc = sc.get(ctx, &d_cnt, n_reads + 1)) ||
            (hip.rc = sc.get(ctx, &d_first, n_reads + 1)) || (hip.rc = sc.get(ctx, &d_status, 1)) || (hip.rc = sc.get(ctx, &d_poff, n_reads + 1)) ||
            (hip.rc = sc.get(ctx, &d_sites, n_sites + 1))) {
            nc_snp_phase_free(ph);
            return hip.rc;
        }
        hip(hipMalloc(&ph->d_off, (n_reads + 1) * sizeof(int64_t)), "hipMalloc(offsets)");
        hip(hipMemsetAsync(d_status, 0, sizeof(int32_t), ctx->stream), "status reset");
        if (n_sites && hip.rc == NC_OK) {
            hip(hipMemcpyAsync(d_spos, site_pos, n_sites * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "site upload");
            hip(hipMemcpyAsync(d_sal, site_alleles, 2 * (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream), "allele upload");
            if (hip.rc == NC_OK) {
                k_hr_sites<<<(n_sites + 255) / 256, 256, 0, ctx->stream>>>(n_sites, d_spos, d_sal, ref_code, ref_len, d_sites);
                hip(hipGetLastError(), "k_hr_sites");
            }
        }
        const int nb = (n_reads + 255) / 256;
        std::vector<int64_t> poff(n_reads + 1, 0);
        if (n_reads && hip.rc == NC_OK) {
            k_hr_span<<<nb, 256, 0, ctx->stream>>>(n_reads, reads->rd_start, reads->rd_end, n_sites, d_spos, d_first, d_cnt);
            hip(hipGetLastError(), "k_hr_span");
        }
        if (hip.rc == NC_OK) {
            k_hp_scan<<<1, HP_THREADS, 0, ctx->stream>>>(d_cnt, n_reads, d_poff);
            hip(hipGetLastError(), "k_hp_scan (pairs)");
            hip(hipMemcpyAsync(&poff[n_reads], d_poff + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream), "pair count download");
            hip(hipStreamSynchronize(ctx->stream), "span sync");
        }
        const int64_t np = hip.rc == NC_OK ? poff[n_reads] : 0;
        if (hip.rc == NC_OK) hip.rc = sc.get(ctx, &d_pal, (size_t)np + 1);
        if (hip.rc == NC_OK && np) {
            HrReads R;
            R.codes = codes;
            R.codes_len = codes_len;
            R.n_reads = n_reads;
            R.rs = reads->rd_start;
            R.re = reads->rd_end;
            R.slot_off = reads->slot_off;
            R.ev_off = reads->ev_off;
            R.ev_pos = reads->ev_pos;
            R.ev_len = reads->ev_len;
            R.ins_off = reads->ins_off;
            R.ins_bases = reads->ins_bases;
            R.read_flag = reads->read_flag;
            R.n_events = n_events;
            R.n_ins = n_ins_bases;
            k_hr_align<<<(unsigned)((np + 255) / 256), 256, 0, ctx->stream>>>(R, np, d_poff, d_first, d_sites, d_pal, d_status);
            hip(hipGetLastError(), "k_hr_align");
        }
        if (hip.rc == NC_OK && n_reads) {
            k_hr_compact<false><<<nb, 256, 0, ctx->stream>>>(n_reads, d_poff, d_first, d_pal, d_cnt, nullptr, nullptr, nullptr);
            hip(hipGetLastError(), "k_hr_compact (count)");
        }
        hp_entries_from_counts(ph, hip, d_cnt, "realign sync", d_status, "nc_snp_phase_realign: a read's events, inserted bases or codes lie outside their arrays (malformed pack)", [&] {
            k_hr_compact<true><<<nb, 256, 0, ctx->stream>>>(n_reads, d_poff, d_first, d_pal, nullptr, ph->d_off, ph->d_site, ph->d_al);
            hip(hipGetLastError(), "k_hr_compact (fill)");
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

}  // extern "C"

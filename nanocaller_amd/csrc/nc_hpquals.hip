// The phaser's weights (DESIGN.md "Read-based phasing", step 6c): given by the host, or read on the device from the BAM records the contig's
// pack was made from -- the input reader beside nc_hprealign.hip.  The handle and its uploads are nc_happhase.h's.
//
//   k_hp_quals          opt-in (nc_snp_phase_weights_from_bam): one wave per kept read walks its BAM record's CIGAR in the inflated record stream
//                       -> the read's MAPQ and, per CSR entry, the quality of the query base aligned to the site
#include "nc_happhase.h"

#include <vector>

namespace {

constexpr int HP_W_MAX = 93;               // the largest entry weight (a BAM quality is a Phred value 0..93)

// MAPQ and base qualities from the device ingest's inflated record stream (nc_ingest.hip made the pack from the same records)
__device__ __forceinline__ uint32_t hq_ldu32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

constexpr int HQ_WPB = 4;                                               // waves (reads) per workgroup
enum { HQ_BAD_RECORD = 1, HQ_BAD_FIELDS = 4 };                          // status bits: the record leaves the stream / its fields leave block_size (k_meta's bit)

// One wave per kept read r (record at raw + rec[r]; entries off[r] .. off[r + 1] in site order).  The CIGAR -- the record's own, or the CG tag's
// behind the placeholder <l_seq>S<n>N, k_meta's rule -- goes by in chunks of 64 operations, one per lane; prefix sums give every operation its
// reference and query start, and the lane looks up the read's entries whose site lies in its reference run: under M / = / X the aligned query
// base's quality, under D / N the last query base's before the operation.  ew = min(quality, w_max); default_weight where there is no base or no
// quality (0xff), and for an entry outside the alignment.  Everything read is checked against block_size, the stream's length and l_seq.
__global__ __launch_bounds__(64 * HQ_WPB) void k_hp_quals(const uint8_t *__restrict__ raw, int64_t raw_len, int32_t n_reads, const int64_t *__restrict__ rec,
                                                          const int64_t *__restrict__ off, const int32_t *__restrict__ esite, const int32_t *__restrict__ spos,
                                                          int32_t mapq_min, int32_t default_weight, int32_t w_max, uint8_t *__restrict__ ew,
                                                          uint8_t *__restrict__ mapq, uint8_t *__restrict__ rok, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * HQ_WPB + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const int64_t e0 = off[r], e1 = off[r + 1], o = rec[r];
    int bad = (o < 0 || o + 36 > raw_len) ? HQ_BAD_RECORD : 0;
    int64_t bs = 0;
    if (!bad) {
        bs = (int32_t)hq_ldu32(raw + o);
        if (bs < 32 || o + 4 + bs > raw_len) bad = HQ_BAD_RECORD;
    }
    const uint8_t *p = raw + (bad ? 0 : o + 4);                          // the record body: p[0, bs)
    int64_t l_name = 0, n_cig = 0, l_seq = 0, pos = 0;
    int mq = 0;
    if (!bad) {
        pos = (int32_t)hq_ldu32(p + 4);
        l_name = p[8];
        mq = p[9];
        n_cig = p[12] | (p[13] << 8);
        l_seq = (int32_t)hq_ldu32(p + 16);
        if (l_seq < 0 || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs) bad = HQ_BAD_FIELDS;
    }
    if (bad) {
        if (lane == 0) {
            atomicOr(status, bad);
            mapq[r] = 0;
            rok[r] = 0;
        }
        for (int64_t e = e0 + lane; e < e1; e += 64) ew[e] = (uint8_t)default_weight;
        return;
    }
    int64_t cigo = 32 + l_name, nc = n_cig;                              // the CIGAR: p[cigo, cigo + 4 nc)
    const int64_t qualo = cigo + 4 * n_cig + (l_seq + 1) / 2, auxo = qualo + l_seq;
    if (n_cig == 2) {
        const uint32_t c0 = hq_ldu32(p + cigo), c1 = hq_ldu32(p + cigo + 4);
        if ((c0 & 15) == 4 && (int64_t)(c0 >> 4) == l_seq && (c1 & 15) == 3) {
            // the placeholder: the real CIGAR is the CG:B,I tag's (every lane walks the tags alike)
            for (int64_t a = auxo; a + 3 <= bs;) {
                const char t0 = (char)p[a], t1 = (char)p[a + 1], ty = (char)p[a + 2];
                a += 3;
                switch (ty) {
                case 'c': case 'C': case 'A': a += 1; break;
                case 's': case 'S': a += 2; break;
                case 'i': case 'I': case 'f': a += 4; break;
                case 'Z': case 'H':
                    while (a < bs && p[a]) a++;
                    a++;
                    break;
                case 'B': {
                    if (a + 5 > bs) {
                        a = bs;
                        break;
                    }
                    const char st = (char)p[a];
                    const int64_t cnt = hq_ldu32(p + a + 1);
                    const int es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4;
                    if (t0 == 'C' && t1 == 'G' && st == 'I' && a + 5 + cnt * 4 <= bs) {
                        cigo = a + 5;
                        nc = cnt;
                    }
                    a += 5 + cnt * es;
                    break;
                }
                default: a = bs; break;
                }
            }
        }
    }
    const int64_t s1 = pos + 1;                                          // the 1-based position of the alignment's first reference base
    int64_t rp = 0, qp = 0;
#pragma unroll 1
    for (int64_t k0 = 0; k0 < nc; k0 += 64) {
        const int64_t k = k0 + lane;
        const uint32_t c = k < nc ? hq_ldu32(p + cigo + 4 * k) : 15u;
        const int op = c & 15;
        const int32_t len = (int32_t)(c >> 4);
        const bool m = op == 0 || op == 7 || op == 8, gap = op == 2 || op == 3;
        const int32_t radv = (m || gap) ? len : 0, qadv = (m || op == 1 || op == 4) ? len : 0;     // (hard clips and pads consume nothing)
        const int64_t ri = (int64_t)nc_wave_incl_scan(radv & 0xFFFF) + ((int64_t)nc_wave_incl_scan(radv >> 16) << 16);
        const int64_t qi = (int64_t)nc_wave_incl_scan(qadv & 0xFFFF) + ((int64_t)nc_wave_incl_scan(qadv >> 16) << 16);
        if (radv > 0) {
            const int64_t a = s1 + rp + ri - radv, b = a + radv, q0 = qp + qi - qadv;
            int64_t lo = e0, hi = e1;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (spos[esite[mid]] < a) lo = mid + 1;
                else hi = mid;
            }
            for (int64_t e = lo; e < e1; e++) {
                const int64_t sp = spos[esite[e]];
                if (sp >= b) break;
                const int64_t q = m ? q0 + (sp - a) : q0 - 1;
                int32_t w = default_weight;
                if (q >= 0 && q < l_seq) {
                    const int32_t v = p[qualo + q];
                    if (v != 0xff) w = min(v, w_max);
                }
                ew[e] = (uint8_t)w;
            }
        }
        rp += __shfl(ri, 63);
        qp += __shfl(qi, 63);
    }
    for (int64_t e = e0 + lane; e < e1; e += 64) {                       // entries the alignment does not reach
        const int64_t sp = spos[esite[e]];
        if (sp < s1 || sp >= s1 + rp) ew[e] = (uint8_t)default_weight;
    }
    if (lane == 0) {
        mapq[r] = (uint8_t)mq;
        rok[r] = mq >= mapq_min ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int nc_snp_phase_set_weights(nc_ctx *ctx, nc_phase *ph, const uint8_t *entry_weight, const uint8_t *read_ok)
{
    if (!ctx || !ph) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_set_weights: bad argument");
    const int64_t ne = ph->off[ph->n_reads];
    for (int64_t e = 0; entry_weight && e < ne; e++)
        if (entry_weight[e] > HP_W_MAX) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_set_weights: entry %lld: weight %d above %d", (long long)e, entry_weight[e], HP_W_MAX);
    for (int32_t r = 0; read_ok && r < ph->n_reads; r++)
        if (read_ok[r] > 1) return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_set_weights: read %d: read_ok must be 0 or 1", r);
    if (entry_weight) ph->ew.assign(entry_weight, entry_weight + ne);
    else ph->ew.assign(ne, 1);
    if (read_ok) ph->rok.assign(read_ok, read_ok + ph->n_reads);
    else ph->rok.assign(ph->n_reads, 1);
    ph->rmapq.assign(ph->n_reads, 0);
    ph->weighted = true;
    ph->solved = false;
    return hp_upload_weights(ph);
}

int nc_snp_phase_weights_from_bam(nc_ctx *ctx, nc_phase *ph, const uint8_t *d_raw, int64_t raw_len, const int64_t *d_rec_off, int32_t mapq_min,
                                  int32_t default_weight, int32_t w_max)
{
    if (!ctx || !ph || raw_len < 0 || (ph->n_reads && (!d_raw || !d_rec_off)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_weights_from_bam: bad argument");
    if (mapq_min < 0 || mapq_min > 255 || default_weight < 0 || default_weight > HP_W_MAX || w_max < 0 || w_max > HP_W_MAX)
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_weights_from_bam: mapq_min outside [0, 255], or default_weight / w_max outside [0, %d]", HP_W_MAX);
    const int32_t R = ph->n_reads, S = ph->n_sites;
    const int64_t ne = ph->off[R];
    std::vector<uint8_t> ew(ne, 0), mq(R, 0), ok(R, 0);
    int32_t status = 0;
    if (!ph->d_off) NC_TRY(hp_upload_csr(ph));
    if (!ph->d_w) NC_HIP(ctx, hipMalloc(&ph->d_w, ne + 16));
    if (R) {
        HpScratch sc;
        int32_t *d_spos = nullptr, *d_status = nullptr;
        uint8_t *d_mq = nullptr, *d_ok = nullptr;
        NC_TRY(sc.get(ctx, &d_spos, S + 1));
        NC_TRY(sc.get(ctx, &d_status, 1));
        NC_TRY(sc.get(ctx, &d_mq, R));
        NC_TRY(sc.get(ctx, &d_ok, R));
        if (S) NC_HIP(ctx, hipMemcpyAsync(d_spos, ph->site_pos.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        NC_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t), ctx->stream));
        k_hp_quals<<<(R + HQ_WPB - 1) / HQ_WPB, 64 * HQ_WPB, 0, ctx->stream>>>(d_raw, raw_len, R, d_rec_off, ph->d_off, ph->d_site, d_spos, mapq_min, default_weight,
                                                                             w_max, ph->d_w, d_mq, d_ok, d_status);
        NC_HIP(ctx, hipGetLastError());
        if (ne) NC_HIP(ctx, hipMemcpyAsync(ew.data(), ph->d_w, ne, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(mq.data(), d_mq, R, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(ok.data(), d_ok, R, hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipMemcpyAsync(&status, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (status) {
        ph->weighted = false;
        return nc_fail(ctx, NC_ERR_ARG, "nc_snp_phase_weights_from_bam: records that %s (status %d)",
                       status & HQ_BAD_RECORD ? "leave the record stream" : "do not hold the fields their header claims", status);
    }
    ph->ew.swap(ew);
    ph->rmapq.swap(mq);
    ph->rok.swap(ok);
    ph->weighted = true;
    ph->solved = false;
    return NC_OK;
}

int nc_snp_phase_weights(const nc_phase *ph, const uint8_t **entry_weight, const uint8_t **read_mapq, const uint8_t **read_ok)
{
    if (!ph) return NC_ERR_ARG;
    if (entry_weight) *entry_weight = ph->weighted ? ph->ew.data() : nullptr;
    if (read_mapq) *read_mapq = ph->weighted ? ph->rmapq.data() : nullptr;
    if (read_ok) *read_ok = ph->weighted ? ph->rok.data() : nullptr;
    return NC_OK;
}

}  // extern "C"

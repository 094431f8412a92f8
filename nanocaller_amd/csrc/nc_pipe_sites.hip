// Device indel pipeline, from alignments to the CNN input and the alleles' strings.
//   k_site_tensor     one workgroup per site: per read set the longest insertion per slot -> columns, the per-column symbol histogram
//                     straight from the tracebacks (no row matrix in HBM), msa()'s frequencies / consensus / tensor (:57-71)
//   k_allele_classes  band class of every consensus' global alignment against its window (allele_prediction)
//   k_alt_copy        the ALT prefixes, back to back in the pool
#include "nc_pipe.h"

namespace {
// HT: the histogram's counter type -- a read set holds at most maxcov reads, so bytes do for maxcov <= 255 (the reference's default is 160)
// and the kernel's LDS drops from 31 to 19 KB: eight workgroups per CU instead of five (3.1 -> 2.x ms; the kernel waits on memory)
template <class HT>
__global__ __launch_bounds__(256) void k_site_tensor(TensorArgs p)
{
    // the three read sets of a site share its alignments (member bits): ONE sweep over the packed entries for the insertion widths and
    // one for the histograms serve all sets (a sweep per set and pass read the site's entries six times: 4.5 GB per chr20-sized contig)
    __shared__ int32_t colv[3][288];
    __shared__ int16_t mxv[3][288];
    __shared__ HT hist[3][CNS_CAP * 4];
    __shared__ uint8_t refrow[CNS_CAP];
    __shared__ uint8_t cnsv[CNS_CAP];
    constexpr int TQ_CAP = 1024;
    __shared__ uint2 qitems[TQ_CAP];                               // insertions of the site's reads: alignment | slot | member bits, length | first base
    __shared__ int32_t s_nq;
    __shared__ int32_t s_ncols[3], s_run;
    // one more read with symbol `sym` in column c of set t: an atomic add on the 32-bit word that holds the counter (no carry: a counter stays <= maxcov)
    auto hist_add = [&](int t, int c, int sym) {
        if (sizeof(HT) == 1) atomicAdd(reinterpret_cast<uint32_t *>(&hist[t][0]) + c, 1u << (8 * sym));
        else atomicAdd(reinterpret_cast<uint32_t *>(&hist[t][0]) + 2 * c + (sym >> 1), 1u << (16 * (sym & 1)));
    };
    __shared__ int32_t wcnt[4], wcntr[4], s_runr, s_dmin, s_dmax;
    const int kl = blockIdx.x, site = p.site0 + kl;
    const int tid = threadIdx.x;
    const int n2 = p.site_n2[site];
    const int S = p.S;
    const int64_t a0 = p.site_al0[site] - p.A0, a1 = p.site_al0[site + 1] - p.A0;
    const uint8_t *mem = p.al_member + p.A0;
    const uint8_t *s2 = p.ref_code + (p.site_pos[site] - p.ref_pos0);
    // ---- ONE sweep over the site's packed entries (round 4 made two: the longest insertion per slot, then the histograms -- the entries are the
    // kernel's traffic, 0.69 GB a sweep per chr20-sized pass): per slot j (thread j; a second turn for the slots past 255 of the 260-base windows) the
    // longest insertion of every set (slot j = before reference position j; slot n2 = after the last), the four base counters of the position's own
    // column in registers, and the insertions onto the block's list.  Neither needs the columns, which come from the insertion widths afterwards.
    // Eight alignments a step, loads first: a load behind a test of the one before it costs a full memory latency each
    if (tid == 0) s_nq = 0;
    __syncthreads();
    uint64_t cntr[2][3] = {{0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int turn = 0; turn < 2; turn++) {
        const int j = tid + 256 * turn;
        if (j > n2) continue;
        int m[3] = {0, 0, 0};
        uint64_t cnt[3] = {0, 0, 0};
        for (int64_t ab = a0; ab < a1; ab += 8) {
            uint32_t en8[8];
            int sym8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) en8[u] = p.ent[min(ab + u, a1 - 1) * p.EW + j];
            // the eight member bytes as two unaligned words, with the other loads, not one by one inside the loop below (the array ends in a pad)
            typedef uint32_t __attribute__((aligned(1))) u32_u;
            const uint32_t mlo = *reinterpret_cast<const u32_u *>(mem + ab), mhi = *reinterpret_cast<const u32_u *>(mem + ab + 4);
#pragma unroll
            for (int u = 0; u < 8; u++) {                             // the base aligned to position j (index clamped: unused when there is none)
                const int qi = (int)(en8[u] & 0x3ffu) - 1;
                sym8[u] = p.win[min(ab + u, a1 - 1) * p.WS + max(qi, 0)];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int64_t a = ab + u;
                if (a >= a1) continue;
                const int mb = (int)(((u < 4 ? mlo : mhi) >> (8 * (u & 3))) & 0xffu);
                const uint32_t en = en8[u];
                if (j < n2 && (en & 0x3ffu) != 0 && sym8[u] < 4) {    // anything else (a read base N) counts as a gap at its column
                    const uint64_t one = 1ull << (16 * sym8[u]);
#pragma unroll
                    for (int t = 0; t < 3; t++)
                        if (mb & (1 << t)) cnt[t] += one;
                }
                // an insertion goes on the block's list: walked here, the whole wave waited for one lane's loads at nearly every alignment
                // (some lane always has one) -- 2/3 of the kernel; from the list every thread takes one insertion
                const int L = (int)((en >> 10) & 0x3ffu);
                if (L > 0) {
#pragma unroll
                    for (int t = 0; t < 3; t++)
                        if (mb & (1 << t)) m[t] = max(m[t], L);        // haploid: one set, member bit 0
                    const int slot = atomicAdd(&s_nq, 1);
                    if (slot < TQ_CAP) qitems[slot] = make_uint2((uint32_t)(a - a0) | ((uint32_t)j << 16) | ((uint32_t)mb << 25), en >> 10);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 3; t++) { mxv[t][j] = (int16_t)m[t]; cntr[turn][t] = cnt[t]; }
    }
    __syncthreads();
    // ---- column of every slot's position = running sum of the insertion widths + j: scan over the block (2 slots per thread: n2 + 1 <= 288)
    for (int t = 0; t < S; t++) {
        const int j0 = 2 * tid, v0 = j0 <= n2 ? mxv[t][j0] : 0, v1 = j0 + 1 <= n2 ? mxv[t][j0 + 1] : 0;
        int inc = v0 + v1;
        inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
        if ((tid & 63) == 63) wcnt[tid >> 6] = inc;
        __syncthreads();
        int wp = 0;
        for (int w = 0; w < (tid >> 6); w++) wp += wcnt[w];
        const int before = wp + inc - v0 - v1;
        if (j0 <= n2) colv[t][j0] = before + v0 + j0;
        if (j0 + 1 <= n2) colv[t][j0 + 1] = before + v0 + v1 + j0 + 1;
        if (tid == 255) s_ncols[t] = wp + inc + n2;
        __syncthreads();
    }
    bool ok[3];
#pragma unroll
    for (int t = 0; t < 3; t++) ok[t] = t < S && s_ncols[t] <= CNS_CAP;      // a longer set: never with real windows; reported, the caller falls back
    for (int t = 0; t < S; t++)
        if (ok[t])
            for (int c = tid; c < s_ncols[t] * 4; c += 256) hist[t][c] = 0;
    __syncthreads();
    // ---- the position columns' counters go to their places
#pragma unroll
    for (int turn = 0; turn < 2; turn++) {
        const int j = tid + 256 * turn;
        if (j >= n2) continue;
#pragma unroll
        for (int t = 0; t < 3; t++)
            if (t < S && ok[t]) {
                const int cj = colv[t][j];
#pragma unroll
                for (int k = 0; k < 4; k++) hist[t][cj * 4 + k] = (HT)((cntr[turn][t] >> (16 * k)) & 0xffffu);
            }
    }
    // (more insertions than the block's list holds -- > 1024 at one site --: every insertion of the site the round-3 way, straight from the entries)
    if (s_nq > TQ_CAP) {
        for (int j = tid; j <= n2; j += 256) {
            int c0[3];
#pragma unroll
            for (int t = 0; t < 3; t++) c0[t] = t < S ? colv[t][j] - mxv[t][j] : 0;
            for (int64_t a = a0; a < a1; a++) {
                const uint32_t en = p.ent[a * p.EW + j];
                const int L = (int)((en >> 10) & 0x3ffu), mb = mem[a];
                const uint8_t *s1 = p.win + a * p.WS + (int)(en >> 20);
                for (int v = 0; v < L; v++) {
                    const int sym = s1[v];
                    if (sym < 4) {
#pragma unroll
                        for (int t = 0; t < 3; t++)
                            if ((mb & (1 << t)) && ok[t]) hist_add(t, c0[t] + v, sym);
                    }
                }
            }
        }
    }
    __syncthreads();
    // ---- the inserted bases: one insertion per thread (columns c0 .. c0 + L - 1 of its slot, shared by the reads of a set: atomic adds)
    {
        const int nq = s_nq > TQ_CAP ? 0 : s_nq;
        for (int i = tid; i < nq; i += 256) {
            const uint2 it = qitems[i];
            const int a = (int)(it.x & 0xffffu), j = (int)((it.x >> 16) & 0x1ffu), mb = (int)(it.x >> 25), L = (int)(it.y & 0x3ffu), q0 = (int)(it.y >> 10);
            const uint8_t *s1 = p.win + (a0 + a) * p.WS + q0;
            int c0[3];
#pragma unroll
            for (int t = 0; t < 3; t++) c0[t] = t < S ? colv[t][j] - mxv[t][j] : 0;
            for (int v = 0; v < L; v++) {
                const int sym = s1[v];
                if (sym < 4) {
#pragma unroll
                    for (int t = 0; t < 3; t++)
                        if ((mb & (1 << t)) && ok[t]) hist_add(t, c0[t] + v, sym);
                }
            }
        }
    }
    __syncthreads();
    for (int t = 0; t < S; t++) {
        const int nr = p.site_nr[site * S + t];
        float *X = p.x + ((int64_t)site * S + t) * 5 * 128 * 2;
        const int ncols = s_ncols[t];
        if (!ok[t]) {
            if (tid == 0) { atomicOr(p.err, 2); p.ncns[kl * S + t] = 0; }
            for (int c = tid; c < 128 * 5; c += 256) { X[c * 2] = 0.0f; X[c * 2 + 1] = 0.0f; }
            continue;
        }
        for (int c = tid; c < ncols; c += 256) refrow[c] = 4;
        __syncthreads();
        for (int j = tid; j < n2; j += 256) refrow[colv[t][j]] = s2[j];
        __syncthreads();
        // frequencies, consensus symbol, tensor (:57-71)
        const float tot = (float)nr;
        for (int c = tid; c < max(ncols, 128); c += 256) {
            if (c < ncols) {
                int h[5];
                int sum = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) { h[k] = hist[t][c * 4 + k]; sum += h[k]; }
                h[4] = nr - sum;
                float alt[5], best = -1e30f;
                int arg = 0;
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    alt[k] = (float)h[k] / tot;
                    const float tv = k == 4 ? alt[k] - 0.01f : alt[k];
                    if (tv > best) { best = tv; arg = k; }
                }
                cnsv[c] = (uint8_t)arg;
                if (c < 128) {
                    const int rc = refrow[c];
#pragma unroll
                    for (int k = 0; k < 5; k++) {
                        const float rf = rc == k ? 1.0f : 0.0f;
                        *reinterpret_cast<float2 *>(X + (k * 128 + c) * 2) = make_float2(alt[k] - rf, rf);
                    }
                }
            } else if (c < 128) {
#pragma unroll
                for (int k = 0; k < 5; k++) *reinterpret_cast<float2 *>(X + (k * 128 + c) * 2) = make_float2(0.0f, 0.0f);
            }
        }
        if (tid == 0) { s_run = 0; s_runr = 0; s_dmin = 0; s_dmax = 0; }
        __syncthreads();
        // consensus with the gap symbols removed (:61-64).  On the way: the diagonals (window columns passed) - (consensus bases written) of the
        // consensus against its window, column by column -- the band of its global alignment in allele_prediction (k_allele_classes)
        uint8_t *out = p.cns + ((int64_t)kl * S + t) * CNS_CAP;
        int dlo = 0, dhi = 0;
        for (int base = 0; base < ncols; base += 256) {
            const int c = base + tid;
            const bool f = c < ncols && cnsv[c] != 4, isr = c < ncols && refrow[c] != 4;
            const uint64_t bm = __ballot(f), br = __ballot(isr);
            if ((tid & 63) == 0) { wcnt[tid >> 6] = __popcll(bm); wcntr[tid >> 6] = __popcll(br); }
            __syncthreads();
            int wp = s_run, totw = 0, wr = s_runr, totr = 0;
            for (int w = 0; w < 4; w++) {
                if (w < (tid >> 6)) { wp += wcnt[w]; wr += wcntr[w]; }
                totw += wcnt[w];
                totr += wcntr[w];
            }
            const uint64_t below = (1ull << (tid & 63)) - 1, upto = below | (1ull << (tid & 63));
            if (f) out[wp + __popcll(bm & below)] = cnsv[c];
            if (c < ncols) {
                const int d = (wr + __popcll(br & upto)) - (wp + __popcll(bm & upto));
                dlo = min(dlo, d);
                dhi = max(dhi, d);
            }
            __syncthreads();
            if (tid == 0) { s_run += totw; s_runr += totr; }
            __syncthreads();
        }
        if (p.cband) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { dlo = min(dlo, __shfl_xor(dlo, o)); dhi = max(dhi, __shfl_xor(dhi, o)); }
            if ((tid & 63) == 0) { atomicMin(&s_dmin, dlo); atomicMax(&s_dmax, dhi); }
            __syncthreads();
            if (tid == 0) { p.cband[(kl * S + t) * 2] = (int16_t)s_dmin; p.cband[(kl * S + t) * 2 + 1] = (int16_t)s_dmax; }
        }
        if (tid == 0) p.ncns[kl * S + t] = s_run;
        __syncthreads();
    }
}

// band of a GLOBAL alignment of a consensus (n1 bases) against its window (n2): the consensus is the window with the set's indels applied, and
// k_site_tensor noted the diagonals its columns run on (cband); classes and lists as k_windows makes them for the star alignment
__global__ __launch_bounds__(256) void k_allele_classes(FillArgs p, const int16_t *__restrict__ cband, int32_t margin, int32_t max_sum, int8_t *__restrict__ band_lo, int32_t *__restrict__ list1,
                                                       int32_t *__restrict__ list2, int32_t *__restrict__ listF, int32_t *__restrict__ counts)
{
    const int al = blockIdx.x * 256 + threadIdx.x;
    int cls = -1;
    if (al < p.A) {
        const int n1 = p.n1[al], n2 = p.site_n2[fill_site(p, al)];
        const int dend = n2 - n1, dmin = min(min(0, dend), (int)cband[2 * al]), dmax = max(max(0, dend), (int)cband[2 * al + 1]), w = dmax - dmin;
        cls = (n1 <= 0 || n1 + n2 > max_sum) ? 2 : w + 2 * margin <= 31 ? 0 : w + 2 * margin <= 63 ? 1 : 2;      // (an empty consensus: the full route reports it)
        const int B = cls == 0 ? 32 : 64;
        int lo = dmin - ((B - 1 - w) >> 1);
        lo -= lo & 1;
        band_lo[al] = (int8_t)(cls == 2 ? 0 : lo);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned long long m = __ballot(cls == c);
        if (!m) continue;
        const int lead = __ffsll((long long)m) - 1, ln = threadIdx.x & 63;
        int base = 0;
        if (ln == lead) base = atomicAdd(counts + c, __popcll(m));
        base = __shfl(base, lead);
        int32_t *lst = c == 0 ? list1 : c == 1 ? list2 : listF;
        if (cls == c) lst[base + __popcll(m & ((1ull << ln) - 1ull))] = al;
    }
}

__global__ __launch_bounds__(256) void k_alt_copy(const uint8_t *__restrict__ cns, const int32_t *__restrict__ alt_len, const int64_t *__restrict__ off,
                                                  int32_t n, uint8_t *__restrict__ pool, int64_t pool_cap, int32_t *__restrict__ err)
{
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n) return;
    const int L = alt_len[a];
    if (L <= 0) return;
    const int64_t o = off[a];
    if (o + L > pool_cap) { if (lane == 0) atomicOr(err, 4); return; }
    for (int i = lane; i < L; i += 64) pool[o + i] = cns[(int64_t)a * CNS_CAP + i];
}

}   // namespace

void nc_pipe_launch_site_tensor(hipStream_t st, const TensorArgs &ta, bool wide_counters)
{
    if (!wide_counters) hipLaunchKernelGGL(k_site_tensor<uint8_t>, dim3(ta.n_sites_g), dim3(256), 0, st, ta);
    else hipLaunchKernelGGL(k_site_tensor<uint16_t>, dim3(ta.n_sites_g), dim3(256), 0, st, ta);
}
void nc_pipe_launch_allele_classes(hipStream_t st, const FillArgs &fb, const int16_t *cband, int32_t margin, int32_t max_sum, int8_t *band_lo, int32_t *list1,
                                   int32_t *list2, int32_t *listF, int32_t *counts)
{
    hipLaunchKernelGGL(k_allele_classes, dim3((fb.A + 255) / 256), dim3(256), 0, st, fb, cband, margin, max_sum, band_lo, list1, list2, listF, counts);
}
void nc_pipe_launch_alt_copy(hipStream_t st, const uint8_t *cns, const int32_t *alt_len, const int64_t *off, int32_t n, uint8_t *pool, int64_t pool_cap, int32_t *err)
{
    hipLaunchKernelGGL(k_alt_copy, dim3((n + 3) / 4), dim3(256), 0, st, cns, alt_len, off, n, pool, pool_cap, err);
}

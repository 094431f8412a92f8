// The write half of BAM on the device: a contig's records, re-tagged with HP / PS from a haplotag table, compressed into BGZF members
// (SAMv1 4.1) in HBM.  Replaces `whatshap haplotag | samtools view -b --write-index` of phase_run (nanocaller_src/indelCaller.py:243-246)
// behind the device phaser (bam_write.py).
//
//   k_retag_size   one lane per record: walks the aux data, drops HP / PS / PC, looks the read name's FNV-1a hash up in the sorted table
//                  -> the record's new size; k_scan_excl turns the sizes into output offsets.
//   k_retag_copy   one wave per record: the record with its kept fields and the new HP (C) / PS (smallest integer type) at the end.
//   k_deflate      one workgroup per member (<= 65,280 bytes in LDS): LZ77 with one hash candidate per position (4-byte hash, heads in LDS
//                  updated batch by batch), a greedy parse in 32-byte segments, one per lane, joined by a prefix maximum over the segments'
//                  ends; then ONE dynamic-Huffman block (15-bit codes, 7-bit code-length code, zlib's run-length symbols 16 / 17 / 18),
//                  bit offsets by a block-wide prefix sum, bits OR-ed into LDS.  A stored block when that would be smaller.
//   k_member_crc   CRC-32 of every member's bytes (nc_crc.h, the reader's k_crc32 arithmetic).
//   k_assemble     every member's 18-byte header, payload and 8-byte trailer into one file image at prefix-summed offsets, + the EOF block.
#include "nc_common.h"
#include "nc_crc.h"

namespace {

constexpr int BGZF_MAX = 0xff00;                     // bytes of one member, the most k_deflate takes
constexpr int DF_THREADS = 1024;
constexpr int SEG = 32;                              // positions per parse segment (one lane's)
constexpr int HALF = DF_THREADS * SEG;               // positions whose candidates are in LDS at once
constexpr int N_SEG = 2 * DF_THREADS;
constexpr int HASH_BITS = 12, N_HEAD = 1 << HASH_BITS;
constexpr int MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr int TOK_MATCH = (int)0x80000000;

// LDS of k_deflate, in bytes
constexpr int L_IN = 0;                              // the member: 65,536
constexpr int L_CAND = L_IN + 65536;                 // distance of every position's candidate (uint16, one half of the member); then the output bits
constexpr int L_HEAD = L_CAND + 65536;               // hash heads: position + 1 (uint32); then the code builders' work arrays
constexpr int L_END = L_HEAD + 4 * N_HEAD;           // end of every segment's parse, then the entry of every segment (int32)
constexpr int L_CNT = L_END + 4 * N_SEG;             // tokens per segment (uint8)
constexpr int L_FLL = L_CNT + N_SEG;                 // frequencies: literal / length [288], distance [32], code length [20] (uint32)
constexpr int L_FD = L_FLL + 4 * 288;
constexpr int L_FC = L_FD + 4 * 32;
constexpr int L_LEN = L_FC + 4 * 20;                 // code lengths: literal / length [288], distance [32], code length [20] (uint8)
constexpr int L_CODE = L_LEN + 340;                  // reversed codes, same order (uint16)
constexpr int L_MISC = L_CODE + 2 * 340;             // 32 int32: counters, header size, wave totals
constexpr int L_TOTAL = L_MISC + 4 * 64;
static_assert(L_TOTAL <= 160 * 1024, "k_deflate's LDS");
// inside the L_HEAD region once the parse is done
constexpr int W_SORT = 0;                            // symbols by frequency (uint16 [320 + 20])
constexpr int W_A = 1024;                            // Moffat-Katajainen work arrays (uint32 [288], [32], [20])
constexpr int W_NUM = W_A + 4 * 340;                 // codes per length (int32 [3][33])
constexpr int W_RLE = W_NUM + 4 * 3 * 33;            // the run-length coded code lengths (uint16 [320])
static_assert(W_RLE + 2 * 320 <= 4 * N_HEAD, "work arrays");

// RFC 1951 3.2.5
__device__ __forceinline__ int len_code(int len)          // 3..258 -> 0..28 (symbol 257 + code)
{
    if (len <= 10) return len - 3;
    if (len == 258) return 28;
    const int x = len - 3, m = 31 - __clz(x);
    return 4 * (m - 1) + ((x >> (m - 2)) & 3);
}
__device__ __forceinline__ int len_extra(int c) { return (c < 8 || c == 28) ? 0 : (c >> 2) - 1; }
__device__ __forceinline__ int len_base(int c) { return c < 8 ? c + 3 : c == 28 ? 258 : ((4 | (c & 3)) << ((c >> 2) - 1)) + 3; }
__device__ __forceinline__ int dist_code(int d)           // 1..32768 -> 0..29
{
    if (d <= 4) return d - 1;
    const int x = d - 1, m = 31 - __clz(x);
    return 2 * m + ((x >> (m - 1)) & 1);
}
__device__ __forceinline__ int dist_extra(int c) { return c < 4 ? 0 : (c >> 1) - 1; }
__device__ __forceinline__ int dist_base(int c) { return c < 4 ? c + 1 : ((2 | (c & 1)) << ((c >> 1) - 1)) + 1; }

// bits, least significant first, OR-ed into 32-bit words of LDS from bit offset `off` on
struct BitW {
    uint32_t *buf;
    int w, nb;
    uint64_t acc;
    __device__ BitW(uint32_t *b, int off) : buf(b), w(off >> 5), nb(off & 31), acc(0) {}
    __device__ __forceinline__ void put(uint32_t v, int len)       // len <= 16
    {
        acc |= (uint64_t)v << nb;
        nb += len;
        if (nb >= 32) {
            atomicOr(&buf[w++], (uint32_t)acc);
            acc >>= 32;
            nb -= 32;
        }
    }
    __device__ __forceinline__ void flush() { if (nb > 0) atomicOr(&buf[w], (uint32_t)acc); }
};

// Code lengths of `n` used symbols, `sorted` = their indices by ascending frequency (ties by index): Moffat and Katajainen's in-place
// minimum-redundancy construction, then limited to `maxbits` (the counts per length are moved up until Kraft's sum is one, as miniz does),
// the longest codes to the least frequent symbols.  One thread.
__device__ void build_lengths(const uint32_t *freq, const uint16_t *sorted, int n, uint32_t *A, int *num, uint8_t *lens, int maxbits)
{
    if (n == 0) return;
    if (n == 1) { lens[sorted[0]] = 1; return; }
    for (int i = 0; i < n; i++) A[i] = freq[sorted[i]];
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; next++) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
        while (avbl > used) { A[next--] = dpth; avbl--; }
        avbl = 2 * used;
        dpth++;
        used = 0;
    }
    for (int l = 0; l <= 32; l++) num[l] = 0;
    for (int i = 0; i < n; i++) num[min((int)A[i], 32)]++;
    for (int l = maxbits + 1; l <= 32; l++) num[maxbits] += num[l];
    uint32_t total = 0;
    for (int l = maxbits; l > 0; l--) total += (uint32_t)num[l] << (maxbits - l);
    while (total != (1u << maxbits)) {
        num[maxbits]--;
        for (int l = maxbits - 1; l > 0; l--)
            if (num[l]) { num[l]--; num[l + 1] += 2; break; }
        total--;
    }
    int i = 0;
    for (int l = maxbits; l > 0; l--)
        for (int k = num[l]; k > 0; k--) lens[sorted[i++]] = (uint8_t)l;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the least-significant-first writer.  One thread.
__device__ void canon_codes(const uint8_t *lens, int n, uint16_t *codes)
{
    int cnt[16], nxt[16];
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int i = 0; i < n; i++) cnt[lens[i]]++;
    cnt[0] = 0;
    int code = 0;
    for (int l = 1; l < 16; l++) { code = (code + cnt[l - 1]) << 1; nxt[l] = code; }
    for (int i = 0; i < n; i++) {
        const int l = lens[i];
        codes[i] = l ? (uint16_t)(__brev((uint32_t)nxt[l]++) >> (32 - l)) : 0;
    }
}

// symbols with non-zero frequency by ascending (frequency, index): thread `t` ranks symbol t of `n`; *cnt += 1 per used symbol
__device__ __forceinline__ void rank_symbol(const uint32_t *freq, int n, int t, uint16_t *sorted, int *cnt)
{
    const uint32_t f = freq[t];
    if (!f) return;
    int r = 0;
    for (int j = 0; j < n; j++) {
        const uint32_t g = freq[j];
        r += (g && (g < f || (g == f && j < t))) ? 1 : 0;
    }
    sorted[r] = (uint16_t)t;
    atomicAdd(cnt, 1);
}

// block-wide exclusive prefix sum of one int per thread (1024 threads); *total = the sum
__device__ __forceinline__ int block_excl_sum(int v, int *wave_tot, int *total)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int inc = nc_wave_incl_scan(v);
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < DF_THREADS / 64; k++) {
        const int t = wave_tot[k];
        before += k < wv ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// block-wide exclusive prefix maximum (values >= 0; the first thread gets 0)
__device__ __forceinline__ int block_excl_max(int v, int *wave_tot)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(inc, s);
        if (lane >= s) inc = max(inc, o);
    }
    if (lane == 63) wave_tot[wv] = inc;
    const int ex_w = __shfl_up(inc, 1);
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wv; k++) before = max(before, wave_tot[k]);
    __syncthreads();
    return max(before, lane ? ex_w : 0);
}

__device__ __forceinline__ int match_len(const uint8_t *in, int p, int d, int maxl)
{
    const uint8_t *a = in + p, *b = in + p - d;
    int l = 0;
    while (l < maxl && a[l] == b[l]) l++;
    return l;
}

// one member: d_in + d_ioff[b], d_ilen[b] bytes -> raw-deflate payload at d_out + d_ooff[b] (room for 65,536 bytes), d_clen[b] bytes.
// d_tok: gridDim.x x 65,536 token slots.  Persistent: workgroup g takes members g, g + gridDim.x, ...
__global__ __launch_bounds__(DF_THREADS) void k_deflate(int32_t n, const uint8_t *__restrict__ d_in, const int64_t *__restrict__ d_ioff,
                                                        const int32_t *__restrict__ d_ilen, uint8_t *__restrict__ d_out, const int64_t *__restrict__ d_ooff,
                                                        int32_t *__restrict__ d_clen, int32_t *__restrict__ d_status, uint32_t *__restrict__ d_tok)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t *s_in = lds + L_IN;
    uint16_t *s_cand = reinterpret_cast<uint16_t *>(lds + L_CAND);
    uint32_t *s_out = reinterpret_cast<uint32_t *>(lds + L_CAND);
    uint32_t *s_head = reinterpret_cast<uint32_t *>(lds + L_HEAD);
    int32_t *s_end = reinterpret_cast<int32_t *>(lds + L_END);
    uint8_t *s_cnt = lds + L_CNT;
    uint32_t *s_fll = reinterpret_cast<uint32_t *>(lds + L_FLL), *s_fd = reinterpret_cast<uint32_t *>(lds + L_FD), *s_fc = reinterpret_cast<uint32_t *>(lds + L_FC);
    uint8_t *s_lll = lds + L_LEN, *s_ld = s_lll + 288, *s_lc = s_lll + 320;
    uint16_t *s_cll = reinterpret_cast<uint16_t *>(lds + L_CODE), *s_cd = s_cll + 288, *s_cc = s_cll + 320;
    int32_t *s_misc = reinterpret_cast<int32_t *>(lds + L_MISC);
    uint8_t *wk = lds + L_HEAD;
    uint16_t *w_sort = reinterpret_cast<uint16_t *>(wk + W_SORT);
    uint32_t *w_A = reinterpret_cast<uint32_t *>(wk + W_A);
    int32_t *w_num = reinterpret_cast<int32_t *>(wk + W_NUM);
    uint16_t *w_rle = reinterpret_cast<uint16_t *>(wk + W_RLE);
    const int tid = threadIdx.x;
    uint32_t *tok = d_tok + (int64_t)blockIdx.x * (N_SEG * SEG);

    for (int b = blockIdx.x; b < n; b += gridDim.x) {
        const int len = d_ilen[b];
        const uint8_t *src = d_in + d_ioff[b];
        uint8_t *dst = d_out + d_ooff[b];
        if (len < 0 || len > BGZF_MAX) {
            if (tid == 0) { d_status[b] = 1; d_clen[b] = 0; }
            continue;
        }
        if (len == 0) {                                                   // an empty fixed-Huffman block, as zlib writes it
            if (tid == 0) { dst[0] = 3; dst[1] = 0; d_clen[b] = 2; d_status[b] = 0; }
            continue;
        }
        for (int i = tid; i < len; i += DF_THREADS) s_in[i] = src[i];
        if (tid < 8) s_in[len + tid] = 0;
        for (int i = tid; i < N_HEAD; i += DF_THREADS) s_head[i] = 0;
        for (int i = tid; i < 288 + 32 + 20; i += DF_THREADS) s_fll[i] = 0;     // (s_fll, s_fd, s_fc are consecutive)
        for (int i = tid; i < 340; i += DF_THREADS) s_lll[i] = 0;
        if (tid < 64) s_misc[tid] = 0;
        __syncthreads();

        // ---- LZ77: candidates, then the segments' greedy parse, one half of the member at a time
        for (int h = 0; h < 2; h++) {
            const int base = h * HALF, hend = min(len, base + HALF);
            for (int bat = base; bat < hend; bat += DF_THREADS) {
                const int p = bat + tid;
                uint32_t hv = 0, c = 0;
                const bool hashed = p + 4 <= len;
                if (hashed) {
                    const uint32_t v = (uint32_t)s_in[p] | (uint32_t)s_in[p + 1] << 8 | (uint32_t)s_in[p + 2] << 16 | (uint32_t)s_in[p + 3] << 24;
                    hv = (v * 2654435761u) >> (32 - HASH_BITS);
                    c = s_head[hv];
                }
                if (p < hend) s_cand[p - base] = (uint16_t)((c && p - (int)(c - 1) <= MAX_DIST) ? p - (int)(c - 1) : 0);
                __syncthreads();
                if (hashed) atomicMax(&s_head[hv], (uint32_t)(p + 1));
                __syncthreads();
            }
            const int k = h * DF_THREADS + tid, s = k * SEG, e = min(s + SEG, len);
            int p = s, cnt = 0;
            uint32_t *tk = tok + k * SEG;
            while (p < e) {
                const int d = p < hend ? s_cand[p - base] : 0;
                const int l = d ? match_len(s_in, p, d, min(MAX_MATCH, len - p)) : 0;
                if (l >= MIN_MATCH) { tk[cnt++] = (uint32_t)TOK_MATCH | (uint32_t)l << 16 | (uint32_t)(d & 0xffff); p += l; }
                else { tk[cnt++] = s_in[p]; p++; }
            }
            s_end[k] = s < len ? p : 0;
            s_cnt[k] = (uint8_t)cnt;
            __syncthreads();
        }

        // ---- join the segments: segment k starts where the parse of segments 0 .. k-1 ended (a prefix maximum of their ends); the token
        //      that straddles that point is cut (a match keeps its distance; fewer than 3 bytes left become literals).  Histograms.
        {
            const int k0 = 2 * tid;
            const int e0 = s_end[k0], e1 = s_end[k0 + 1];
            const int entry0 = block_excl_max(max(e0, e1), s_misc + 32);
            const int entry1 = max(entry0, e0);
            for (int j = 0; j < 2; j++) {
                const int k = k0 + j, entry = j ? entry1 : entry0;
                uint32_t *tk = tok + k * SEG;
                const int n_in = s_cnt[k];
                int p = k * SEG, c = 0;
                uint32_t nxt = n_in ? tk[0] : 0;
                for (int i = 0; i < n_in; i++) {
                    const uint32_t t = nxt;
                    nxt = i + 1 < n_in ? tk[i + 1] : 0;                   // (read before the write below may reach slot i + 1)
                    const bool m = (int)t < 0;
                    const int tl = m ? (int)((t >> 16) & 0x1ff) : 1, te = p + tl;
                    if (te > entry) {
                        if (p >= entry) {
                            tk[c++] = t;
                            if (m) { atomicAdd(&s_fll[257 + len_code(tl)], 1u); atomicAdd(&s_fd[dist_code(t & 0xffff)], 1u); }
                            else atomicAdd(&s_fll[t], 1u);
                        } else if (te - entry >= 3) {
                            const int r = te - entry;
                            tk[c++] = (uint32_t)TOK_MATCH | (uint32_t)r << 16 | (t & 0xffff);
                            atomicAdd(&s_fll[257 + len_code(r)], 1u);
                            atomicAdd(&s_fd[dist_code(t & 0xffff)], 1u);
                        } else {
                            for (int q = entry; q < te; q++) { tk[c++] = s_in[q]; atomicAdd(&s_fll[s_in[q]], 1u); }
                        }
                    }
                    p = te;
                }
                s_cnt[k] = (uint8_t)c;
            }
        }
        __syncthreads();

        // ---- the two codes: every symbol ranked by one thread, then one thread per code builds lengths and codes
        if (tid == 0) {
            s_fll[256] = 1;                                               // end of block
            int used = 0;
            for (int i = 0; i < 286; i++) used += s_fll[i] ? 1 : 0;
            if (used < 2) s_fll[0] = 1;
            used = 0;
            for (int i = 0; i < 30; i++) used += s_fd[i] ? 1 : 0;
            if (used < 2) { if (!s_fd[0]) s_fd[0] = 1; else s_fd[1] = 1; }
            if (used == 0) s_fd[1] = 1;
        }
        __syncthreads();
        if (tid < 286) rank_symbol(s_fll, 286, tid, w_sort, &s_misc[0]);
        else if (tid >= 320 && tid < 350) rank_symbol(s_fd, 30, tid - 320, w_sort + 288, &s_misc[1]);
        __syncthreads();
        if (tid == 0) {
            build_lengths(s_fll, w_sort, s_misc[0], w_A, w_num, s_lll, 15);
            canon_codes(s_lll, 286, s_cll);
        } else if (tid == 64) {
            build_lengths(s_fd, w_sort + 288, s_misc[1], w_A + 288, w_num + 33, s_ld, 15);
            canon_codes(s_ld, 30, s_cd);
        }
        __syncthreads();
        // ---- the code lengths, run-length coded (symbols 16 / 17 / 18), and their own code (7 bits)
        if (tid == 0) {
            int hlit = 286, hdist = 30;
            while (hlit > 257 && !s_lll[hlit - 1]) hlit--;
            while (hdist > 1 && !s_ld[hdist - 1]) hdist--;
            const int total = hlit + hdist;
            int nr = 0, i = 0;
            while (i < total) {
                const int cur = i < hlit ? s_lll[i] : s_ld[i - hlit];
                int run = 1;
                while (i + run < total && (i + run < hlit ? s_lll[i + run] : s_ld[i + run - hlit]) == cur) run++;
                i += run;
                if (cur == 0) {
                    while (run >= 11) { const int r = min(run, 138); w_rle[nr++] = (uint16_t)(18 | (r - 11) << 8); run -= r; }
                    if (run >= 3) { w_rle[nr++] = (uint16_t)(17 | (run - 3) << 8); run = 0; }
                } else {
                    w_rle[nr++] = (uint16_t)cur;
                    run--;
                    while (run >= 3) { const int r = min(run, 6); w_rle[nr++] = (uint16_t)(16 | (r - 3) << 8); run -= r; }
                }
                while (run > 0) { w_rle[nr++] = (uint16_t)cur; run--; }
            }
            for (int r = 0; r < nr; r++) s_fc[w_rle[r] & 31]++;
            int used = 0;
            for (int s = 0; s < 19; s++) used += s_fc[s] ? 1 : 0;
            if (used < 2) { if (!s_fc[0]) s_fc[0] = 1; else s_fc[1] = 1; }
            int nc = 0;
            uint16_t *srt = w_sort + 320;
            for (int s = 0; s < 19; s++) {
                const uint32_t f = s_fc[s];
                if (!f) continue;
                int r = 0;
                for (int j = 0; j < 19; j++) r += (s_fc[j] && (s_fc[j] < f || (s_fc[j] == f && j < s))) ? 1 : 0;
                srt[r] = (uint16_t)s;
                nc++;
            }
            build_lengths(s_fc, srt, nc, w_A + 320, w_num + 66, s_lc, 7);
            canon_codes(s_lc, 19, s_cc);
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            int hclen = 19;
            while (hclen > 4 && !s_lc[order[hclen - 1]]) hclen--;
            int bits = 3 + 5 + 5 + 4 + 3 * hclen;
            for (int r = 0; r < nr; r++) {
                const int s = w_rle[r] & 31;
                bits += s_lc[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
            }
            s_misc[2] = bits;
            s_misc[3] = hlit;
            s_misc[4] = hdist;
            s_misc[5] = hclen;
            s_misc[6] = nr;
        }
        __syncthreads();

        // ---- bit offsets of every lane's tokens (its two segments)
        int mybits = 0;
        for (int j = 0; j < 2; j++) {
            const int k = 2 * tid + j;
            const uint32_t *tk = tok + k * SEG;
            for (int i = 0, nk = s_cnt[k]; i < nk; i++) {
                const uint32_t t = tk[i];
                if ((int)t < 0) {
                    const int lc = len_code((t >> 16) & 0x1ff), dc = dist_code(t & 0xffff);
                    mybits += s_lll[257 + lc] + len_extra(lc) + s_ld[dc] + dist_extra(dc);
                } else mybits += s_lll[t];
            }
        }
        int sum_bits;
        const int off = block_excl_sum(mybits, s_misc + 32, &sum_bits);
        const int head_bits = s_misc[2];
        const int total_bits = head_bits + sum_bits + s_lll[256];
        const int nbytes = (total_bits + 7) >> 3;
        if (nbytes >= len + 5) {                                          // stored block: BFINAL 1, BTYPE 00, LEN, NLEN, the bytes
            if (tid == 0) {
                dst[0] = 1;
                dst[1] = (uint8_t)len; dst[2] = (uint8_t)(len >> 8);
                dst[3] = (uint8_t)~len; dst[4] = (uint8_t)(~len >> 8);
                d_clen[b] = len + 5;
                d_status[b] = 0;
            }
            for (int i = tid; i < len; i += DF_THREADS) dst[5 + i] = s_in[i];
            __syncthreads();
            continue;
        }
        for (int i = tid; i < (nbytes >> 2) + 1; i += DF_THREADS) s_out[i] = 0;
        __syncthreads();
        if (tid == 0) {                                                   // block header + end of block
            BitW bw(s_out, 0);
            const int hlit = s_misc[3], hdist = s_misc[4], hclen = s_misc[5], nr = s_misc[6];
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            bw.put(1 | 2 << 1, 3);
            bw.put(hlit - 257, 5);
            bw.put(hdist - 1, 5);
            bw.put(hclen - 4, 4);
            for (int i = 0; i < hclen; i++) bw.put(s_lc[order[i]], 3);
            for (int r = 0; r < nr; r++) {
                const int s = w_rle[r] & 31, x = w_rle[r] >> 8;
                bw.put(s_cc[s], s_lc[s]);
                if (s == 16) bw.put(x, 2);
                else if (s == 17) bw.put(x, 3);
                else if (s == 18) bw.put(x, 7);
            }
            bw.flush();
            BitW eob(s_out, head_bits + sum_bits);
            eob.put(s_cll[256], s_lll[256]);
            eob.flush();
        }
        {
            BitW bw(s_out, head_bits + off);
            for (int j = 0; j < 2; j++) {
                const int k = 2 * tid + j;
                const uint32_t *tk = tok + k * SEG;
                for (int i = 0, nk = s_cnt[k]; i < nk; i++) {
                    const uint32_t t = tk[i];
                    if ((int)t < 0) {
                        const int l = (t >> 16) & 0x1ff, d = t & 0xffff;
                        const int lc = len_code(l), dc = dist_code(d);
                        bw.put(s_cll[257 + lc], s_lll[257 + lc]);
                        if (len_extra(lc)) bw.put(l - len_base(lc), len_extra(lc));
                        bw.put(s_cd[dc], s_ld[dc]);
                        if (dist_extra(dc)) bw.put(d - dist_base(dc), dist_extra(dc));
                    } else bw.put(s_cll[t], s_lll[t]);
                }
            }
            bw.flush();
        }
        __syncthreads();
        const uint8_t *ob = reinterpret_cast<const uint8_t *>(s_out);
        for (int i = tid; i < nbytes; i += DF_THREADS) dst[i] = ob[i];
        if (tid == 0) { d_clen[b] = nbytes; d_status[b] = 0; }
        __syncthreads();
    }
}

// CRC-32 of every member's bytes, one wave per member
__global__ __launch_bounds__(256) void k_member_crc(int32_t n, const uint8_t *__restrict__ d_in, const int64_t *__restrict__ d_ioff,
                                                    const int32_t *__restrict__ d_ilen, uint32_t *__restrict__ d_crc, nc_crc::CrcOps ops)
{
    __shared__ uint32_t T[4][256];
    const int tid = threadIdx.x, lane = tid & 63;
    nc_crc::crc_tables(T, tid);
    const int b = blockIdx.x * 4 + (tid >> 6);
    if (b >= n) return;
    const uint32_t c = nc_crc::crc_wave(d_in + d_ioff[b], min(max(d_ilen[b], 0), 65536), lane, T, ops);
    if (lane == 0) d_crc[b] = c;
}

// out[i] = sum of (v[j] + add) over j < i, out[n] = the total.  One workgroup.
__global__ __launch_bounds__(1024) void k_scan_excl(int64_t n, const int32_t *__restrict__ v, int32_t add, int64_t *__restrict__ out)
{
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, a = min(n, tid * per), z = min(n, a + per);
    int64_t s = 0;
    for (int64_t i = a; i < z; i++) s += (int64_t)v[i] + add;
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int k = 0; k < 1024; k++) { const int64_t x = part[k]; part[k] = run; run += x; }
        out[n] = run;
    }
    __syncthreads();
    s = part[tid];
    for (int64_t i = a; i < z; i++) { out[i] = s; s += (int64_t)v[i] + add; }
}

// one workgroup per member: gzip header with the BC extra field (SAMv1 4.1), payload, CRC-32, ISIZE; workgroup 0 also the EOF block
__global__ __launch_bounds__(256) void k_assemble(int32_t n, const uint8_t *__restrict__ pay, const int64_t *__restrict__ poff,
                                                  const int32_t *__restrict__ clen, const uint32_t *__restrict__ crc, const int32_t *__restrict__ isize,
                                                  const int64_t *__restrict__ foff, uint8_t *__restrict__ file)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == n) {
        const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (tid < 28) file[foff[n] + tid] = eof[tid];
        return;
    }
    uint8_t *o = file + foff[b];
    const int c = clen[b];
    const int bsize = c + 25;
    if (tid < 18) {
        const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
        o[tid] = hdr[tid];
    } else if (tid < 26) {
        const int k = tid - 18;
        const uint32_t w = k < 4 ? crc[b] : (uint32_t)isize[b];
        o[18 + c + k] = (uint8_t)(w >> (8 * (k & 3)));
    }
    const uint8_t *p = pay + poff[b];
    for (int i = tid; i < c; i += 256) o[18 + i] = p[i];
}

// ---- re-tagging
struct RecHead {
    int32_t end;      // bytes of the record with its block_size field
    int32_t aux;      // where its aux data starts (same origin)
    int32_t l_name;
};
__device__ __forceinline__ uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

__device__ __forceinline__ bool rec_head(const uint8_t *r, RecHead &h)
{
    const int64_t bs = (int32_t)rd32(r);
    if (bs < 32) return false;
    const int l_name = r[12];
    const int n_cig = r[16] | r[17] << 8;
    const int64_t l_seq = (int32_t)rd32(r + 20);
    if (l_seq < 0) return false;
    const int64_t aux = 36 + l_name + 4 * (int64_t)n_cig + (l_seq + 1) / 2 + l_seq;
    if (aux > 4 + bs || bs > (1 << 30)) return false;
    h.end = (int32_t)(4 + bs);
    h.aux = (int32_t)aux;
    h.l_name = l_name;
    return true;
}

// size of the aux field at r[p] (its tag and type included), 0 when it runs past `end` or has an unknown type
__device__ __forceinline__ int aux_field(const uint8_t *r, int p, int end)
{
    if (p + 3 > end) return 0;
    const char ty = (char)r[p + 2];
    int64_t sz;
    switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': {
            int q = p + 3;
            while (q < end && r[q]) q++;
            if (q >= end) return 0;
            sz = q + 1 - (p + 3);
            break;
        }
        case 'B': {
            if (p + 8 > end) return 0;
            const char st = (char)r[p + 3];
            const int64_t cnt = rd32(r + p + 4);
            const int es = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : (st == 'i' || st == 'I' || st == 'f') ? 4 : 0;
            if (!es) return 0;
            sz = 5 + cnt * es;
            break;
        }
        default: return 0;
    }
    if (p + 3 + sz > end) return 0;
    return (int)(3 + sz);
}
__device__ __forceinline__ bool dropped_tag(const uint8_t *f) { return (f[0] == 'H' && f[1] == 'P') || (f[0] == 'P' && (f[1] == 'S' || f[1] == 'C')); }

// PS as pysam's set_tag types an integer: the smallest of C / S / I (c / s / i below zero) that holds it.  -> bytes of the value
__device__ __forceinline__ int ps_type(int32_t v, char &ty)
{
    if (v >= 0) { ty = v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I'; }
    else { ty = v >= -128 ? 'c' : v >= -32768 ? 's' : 'i'; }
    return (ty == 'C' || ty == 'c') ? 1 : (ty == 'S' || ty == 's') ? 2 : 4;
}

__global__ __launch_bounds__(256) void k_retag_size(int32_t n, const uint8_t *__restrict__ raw, const int64_t *__restrict__ rec_off,
                                                    const uint64_t *__restrict__ thash, const int32_t *__restrict__ tps, int32_t n_tags,
                                                    int32_t *__restrict__ new_size, int32_t *__restrict__ tag_idx, int32_t *__restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *r = raw + rec_off[i];
    RecHead h;
    if (!rec_head(r, h)) { atomicOr(status, 1); new_size[i] = 0; tag_idx[i] = -1; return; }
    int drop = 0;
    for (int p = h.aux; p < h.end;) {
        const int f = aux_field(r, p, h.end);
        if (!f) { atomicOr(status, 2); new_size[i] = 0; tag_idx[i] = -1; return; }
        if (dropped_tag(r + p)) drop += f;
        p += f;
    }
    uint64_t hv = 1469598103934665603ull;                                // FNV-1a of the name with its NUL (nc_ingest.hip's M_HASH)
    for (int k = 0; k < h.l_name; k++) hv = (hv ^ r[36 + k]) * 1099511628211ull;
    int lo = 0, hi = n_tags;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thash[mid] < hv) lo = mid + 1; else hi = mid;
    }
    const int t = (lo < n_tags && thash[lo] == hv) ? lo : -1;
    int add = 0;
    if (t >= 0) {
        char ty;
        add = 4 + 3 + ps_type(tps[t], ty);
    }
    new_size[i] = h.end - drop + add;
    tag_idx[i] = t;
}

// dst[0, len) = src[0, len) by the 64 lanes of a wave: dwords to aligned destinations, each put together from the two aligned source
// dwords it straddles
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, int len, int lane)
{
    const int head = min(len, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    if (lane < head) dst[lane] = src[lane];
    dst += head; src += head; len -= head;
    const int nd = len >> 2;
    const int sh = (int)((uintptr_t)src & 3);
    const uint32_t *sa = reinterpret_cast<const uint32_t *>(src - sh);
    uint32_t *da = reinterpret_cast<uint32_t *>(dst);
    if (sh == 0) {
        for (int k = lane; k < nd; k += 64) da[k] = sa[k];
    } else {
        for (int k = lane; k < nd; k += 64) {
            const uint64_t w = (uint64_t)sa[k] | (uint64_t)sa[k + 1] << 32;
            da[k] = (uint32_t)(w >> (8 * sh));
        }
    }
    const int tail = len & 3;
    if (lane < tail) dst[4 * nd + lane] = src[4 * nd + lane];
}

__global__ __launch_bounds__(256) void k_retag_copy(int32_t n, const uint8_t *__restrict__ raw, const int64_t *__restrict__ rec_off,
                                                    const uint8_t *__restrict__ thp, const int32_t *__restrict__ tps, const int32_t *__restrict__ tag_idx,
                                                    const int64_t *__restrict__ out_off, uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const uint8_t *r = raw + rec_off[i];
    uint8_t *o = out + out_off[i];
    const int new_len = (int)(out_off[i + 1] - out_off[i]);
    RecHead h;
    if (!rec_head(r, h)) return;                                        // (k_retag_size reported it)
    if (lane < 4) o[lane] = (uint8_t)((uint32_t)(new_len - 4) >> (8 * lane));
    wave_copy(o + 4, r + 4, h.aux - 4, lane);
    int q = h.aux;
    for (int p = h.aux; p < h.end;) {
        const int f = aux_field(r, p, h.end);
        if (!f) return;
        if (!dropped_tag(r + p)) {
            wave_copy(o + q, r + p, f, lane);
            q += f;
        }
        p += f;
    }
    const int t = tag_idx[i];
    if (t >= 0 && lane == 0) {
        o[q] = 'H'; o[q + 1] = 'P'; o[q + 2] = 'C'; o[q + 3] = thp[t];
        char ty;
        const int32_t v = tps[t];
        const int nb = ps_type(v, ty);
        o[q + 4] = 'P'; o[q + 5] = 'S'; o[q + 6] = (uint8_t)ty;
        for (int k = 0; k < nb; k++) o[q + 7 + k] = (uint8_t)((uint32_t)v >> (8 * k));
    }
}

}   // namespace

extern "C" int nc_bam_retag_sizes(nc_ctx *ctx, const uint8_t *d_raw, int32_t n_rec, const int64_t *d_rec_off, const uint64_t *d_hash, const int32_t *d_ps,
                                  int32_t n_tags, int32_t *d_new_size, int32_t *d_tag_idx, int64_t *d_out_off, int32_t *d_status)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_rec < 0 || n_tags < 0 || (n_tags && (!d_hash || !d_ps)) || (n_rec && (!d_raw || !d_rec_off || !d_new_size || !d_tag_idx)) || !d_out_off || !d_status)
        return nc_fail(ctx, NC_ERR_ARG, "nc_bam_retag_sizes: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    if (n_rec) {
        hipLaunchKernelGGL(k_retag_size, dim3((n_rec + 255) / 256), dim3(256), 0, ctx->stream, n_rec, d_raw, d_rec_off, d_hash, d_ps, n_tags,
                           d_new_size, d_tag_idx, d_status);
        NC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, ctx->stream, (int64_t)n_rec, (const int32_t *)d_new_size, 0, d_out_off);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

extern "C" int nc_bam_retag(nc_ctx *ctx, const uint8_t *d_raw, int32_t n_rec, const int64_t *d_rec_off, const uint8_t *d_hp, const int32_t *d_ps,
                            const int32_t *d_tag_idx, const int64_t *d_out_off, uint8_t *d_out)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_rec < 0 || (n_rec && (!d_raw || !d_rec_off || !d_tag_idx || !d_out_off || !d_out)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_bam_retag: bad argument");
    if (n_rec == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_retag_copy, dim3((n_rec + 3) / 4), dim3(256), 0, ctx->stream, n_rec, d_raw, d_rec_off, d_hp, d_ps, d_tag_idx, d_out_off, d_out);
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

extern "C" int nc_bgzf_deflate_device(nc_ctx *ctx, int32_t n, const uint8_t *d_in, const int64_t *d_ioff, const int32_t *d_ilen, uint8_t *d_out,
                                      const int64_t *d_ooff, int32_t *d_clen, uint32_t *d_crc, int32_t *d_status)
{
    if (!ctx) return NC_ERR_ARG;
    if (n < 0 || (n && (!d_in || !d_ioff || !d_ilen || !d_out || !d_ooff || !d_clen || !d_status)))
        return nc_fail(ctx, NC_ERR_ARG, "nc_bgzf_deflate_device: bad argument");
    if (n == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    int cus = 0;
    NC_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const int grid = min(n, max(1, cus));                               // one workgroup per CU (LDS): persistent over the members
    NC_TRY(nc_ensure(ctx, ctx->deflate_tok, (size_t)grid * N_SEG * SEG * sizeof(uint32_t)));
    if (!ctx->deflate_lds_set) {
        NC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_deflate), hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL));
        ctx->deflate_lds_set = true;
    }
    hipLaunchKernelGGL(k_deflate, dim3(grid), dim3(DF_THREADS), L_TOTAL, ctx->stream, n, d_in, d_ioff, d_ilen, d_out, d_ooff, d_clen, d_status,
                       (uint32_t *)ctx->deflate_tok.p);
    NC_HIP(ctx, hipGetLastError());
    if (d_crc) {
        hipLaunchKernelGGL(k_member_crc, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, n, d_in, d_ioff, d_ilen, d_crc, nc_crc::crc_ops());
        NC_HIP(ctx, hipGetLastError());
    }
    return NC_OK;
}

extern "C" int nc_bgzf_crc32_device(nc_ctx *ctx, int32_t n, const uint8_t *d_in, const int64_t *d_ioff, const int32_t *d_ilen, uint32_t *d_crc)
{
    if (!ctx) return NC_ERR_ARG;
    if (n < 0 || (n && (!d_in || !d_ioff || !d_ilen || !d_crc))) return nc_fail(ctx, NC_ERR_ARG, "nc_bgzf_crc32_device: bad argument");
    if (n == 0) return NC_OK;
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_member_crc, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, n, d_in, d_ioff, d_ilen, d_crc, nc_crc::crc_ops());
    NC_HIP(ctx, hipGetLastError());
    return NC_OK;
}

extern "C" int nc_bgzf_assemble_device(nc_ctx *ctx, int32_t n, const uint8_t *d_pay, const int64_t *d_poff, const int32_t *d_clen, const uint32_t *d_crc,
                                       const int32_t *d_isize, int64_t *d_foff, uint8_t *d_file)
{
    if (!ctx) return NC_ERR_ARG;
    if (n < 0 || !d_foff || (n && (!d_clen || (d_file && (!d_pay || !d_poff || !d_crc || !d_isize)))))
        return nc_fail(ctx, NC_ERR_ARG, "nc_bgzf_assemble_device: bad argument");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_scan_excl, dim3(1), dim3(1024), 0, ctx->stream, (int64_t)n, d_clen, 26, d_foff);
    NC_HIP(ctx, hipGetLastError());
    if (d_file) {
        hipLaunchKernelGGL(k_assemble, dim3(n + 1), dim3(256), 0, ctx->stream, n, d_pay, d_poff, d_clen, d_crc, d_isize, (const int64_t *)d_foff, d_file);
        NC_HIP(ctx, hipGetLastError());
    }
    return NC_OK;
}

// The reference FASTA on the device: a contig's lines, as they stand in the (inflated) file image in HBM, to the three forms the callers
// read -- the letters (bam.read_fasta_bytes), the scan's reference codes on the tile grid (DeviceBam._ref_lut's rule: upper-case AGTC only,
// quirk E4) and the case-blind codes of the phaser (phase._ref_codes).  Position p (1-based) of a contig the .fai describes by (offset,
// linebases lb, linewidth lw) is the byte at first + ((p-1)/lb)*lw + (p-1)%lb.
//   k_fasta_decode   256 lanes x 16 positions per workgroup.  The workgroup's source span (4,096 positions, their line terminators, up to
//                    15 positions before them for the scan grid and one behind them for the last terminator: <= 3 bytes per position at
//                    lb = 1 with \r\n) goes through LDS with coalesced aligned dword loads.  A lane divides ONCE (its first position by
//                    lb) and steps from there, a byte of LDS per position and one table look-up for both codes.  Letters and blind codes lie on the grid of (p-1)/16; the scan codes on the grid of
//                    (p - scan_pos0)/16, which is the same grid shifted by d = (scan_pos0 - 1) mod 16: the lane also decodes the 16 - d
//                    positions before its own and cuts its scan vector out of the 32-byte window.  Every output is one aligned 16-byte
//                    store; vectors that hang over an array's end are stored bytewise.
// The file is checked as it is read: every terminator slot of a full line that another line of the contig follows holds \n (lw - lb == 1)
// or \r\n (lw - lb == 2), no base byte lies outside 0x21..0x7e, and the contig's span lies inside the image; nothing outside
// [0, raw_len) is read whatever the .fai claims.
#include "nc_common.h"

namespace {

constexpr int FA_LANES = 256;                                          // lanes per workgroup
constexpr int FA_GROUP = 16;                                           // positions per lane
constexpr int FA_BLOCK = FA_LANES * FA_GROUP;                          // positions per workgroup
constexpr int FA_LDS = ((FA_BLOCK + FA_GROUP + 1) * 3 + 3 + 15) & ~15; // staged bytes at most: 3 per position + the base's misalignment

enum { FA_BAD_TERMINATOR = 1, FA_BAD_BASE = 2, FA_BAD_SPAN = 4 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A0 G1 T2 C3 for an upper-case letter, else 4
__device__ __forceinline__ uint32_t code_upper(uint32_t c) { return c == 'A' ? 0u : c == 'G' ? 1u : c == 'T' ? 2u : c == 'C' ? 3u : 4u; }

__device__ __forceinline__ void store16(uint8_t *dst, int64_t i, int64_t n, const uint32_t (&w)[4])
{
    if (i + 16 <= n) {
        *(u32x4 *)(dst + i) = u32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (i + k < n) dst[i + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

struct FaWalk {
    const uint8_t *src, *tab;                                          // the staged bytes; per byte value: upper-case code | case-blind code << 4
    int32_t j_first, q0, qf, length;
    uint32_t lb, eol;
    int32_t ga;
    uint32_t g_span;                                                   // gb - ga
};

// One lane's walk over its window: entry j is position q0 - 16 + j (j < 16: the positions before its own, which only its scan vector takes;
// j < j_first, the same in every lane of the launch, are not needed).  EDGE: the window hangs over an end of the contig and every position is
// tested (those outside give code 4); else none is.  A lane steps byte by byte and takes the branch only where it crosses a line's end.
template <bool EDGE>
__device__ __forceinline__ void walk_window(const FaWalk &w, uint32_t col, int32_t off, uint32_t (&wl)[4], uint32_t (&wb)[4], uint32_t (&ws)[9], int32_t &bad)
{
    uint32_t mn = 'A', mx = 'A';
#pragma unroll
    for (int j = 0; j < 2 * FA_GROUP; j++) {
        if (j < FA_GROUP && j < w.j_first) continue;
        const int32_t q = w.q0 - FA_GROUP + j;
        const int sh = 8 * (j & 3);
        if (EDGE && (q < w.qf || q >= w.length)) {
            ws[j >> 2] |= 4u << sh;
            continue;
        }
        const uint32_t c = w.src[off];
        mn = min(mn, c);
        mx = max(mx, c);
        const uint32_t t = w.tab[c];
        ws[j >> 2] |= ((uint32_t)(q + 1 - w.ga) <= w.g_span ? t & 15u : 4u) << sh;
        if (j >= FA_GROUP) {
            wl[(j >> 2) & 3] |= c << sh;
            wb[(j >> 2) & 3] |= (t >> 4) << sh;
        }
        off++;
        if (++col == w.lb) {
            col = 0;
            if (q + 1 < w.length) {                                    // another line of the contig follows: its terminator is staged
                if (w.eol == 1 ? w.src[off] != '\n' : (w.src[off] != '\r' || w.src[off + 1] != '\n')) bad |= FA_BAD_TERMINATOR;
                off += w.eol;
            }
        }
    }
    if (mn < 0x21 || mx > 0x7e) bad |= FA_BAD_BASE;
}

__global__ __launch_bounds__(FA_LANES) void k_fasta_decode(const uint8_t *__restrict__ raw, int64_t raw_len, int64_t first, int64_t span, int32_t length,
                                                           uint32_t lb, uint32_t lw, uint8_t *__restrict__ letters, uint8_t *__restrict__ scan,
                                                           int64_t scan_pos0, int64_t scan_len, int32_t ga, int32_t gb, int32_t d,
                                                           uint8_t *__restrict__ blind, int32_t *status)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[FA_LDS + 256];   // the staged bytes, then the code table
    if (first < 0 || span < 0 || first > raw_len - span) {            // (the host refuses this before the launch)
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, FA_BAD_SPAN);
        return;
    }
    const uint32_t eol = lw - lb;                                      // 1 or 2
    const int32_t back = scan && d ? FA_GROUP - d : 0;                 // positions before a lane's own that its scan vector takes
    // zero-based positions: the workgroup decodes [qa, qe), and stages qe's byte too when there is one (the terminator before it)
    const int64_t b0 = (int64_t)blockIdx.x * FA_BLOCK;
    const int32_t qa = (int32_t)(b0 - back > 0 ? b0 - back : 0);
    const bool have = qa < length;                                     // (false: the grid's spare group alone, nothing of the contig left to read)
    const int32_t qe = (int32_t)(b0 + FA_BLOCK < length ? b0 + FA_BLOCK : length);
    const int32_t ql = qe < length ? qe : length - 1;                  // last staged position
    const int64_t src_a = first + (int64_t)((uint32_t)qa / lb) * lw + (uint32_t)qa % lb;
    const int64_t src_e = first + (int64_t)((uint32_t)ql / lb) * lw + (uint32_t)ql % lb + 1;
    // staging: aligned dwords of the image from the dword that holds src_a; a dword that hangs over either end of the image goes bytewise
    const int64_t stage0 = src_a - (int64_t)((uintptr_t)(raw + src_a) & 3);
    const int32_t n_dw = have ? (int32_t)((src_e - stage0 + 3) >> 2) : 0;   // <= FA_LDS / 4 (lw <= lb + 2)
    for (int32_t i = threadIdx.x; i < n_dw; i += FA_LANES) {
        const int64_t o = stage0 + 4 * (int64_t)i;
        uint32_t w = 0;
        if (o >= 0 && o + 4 <= raw_len) {
            w = *(const uint32_t *)(raw + o);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (o + k >= 0 && o + k < raw_len) w |= (uint32_t)raw[o + k] << (8 * k);
        }
        ((uint32_t *)lds)[i] = w;
    }
    lds[FA_LDS + threadIdx.x] = (uint8_t)(code_upper(threadIdx.x) | code_upper(threadIdx.x & 0xdfu) << 4);   // (FA_LANES == 256 entries)
    __syncthreads();

    const int64_t q0 = b0 + (int64_t)threadIdx.x * FA_GROUP;           // the lane's own positions: [q0, q0 + 16)
    const int64_t qf64 = q0 - back > 0 ? q0 - back : 0;
    const bool walk = qf64 < length;                                   // (else: only a scan vector of 4s, behind the contig's end)
    const int32_t qf = walk ? (int32_t)qf64 : 0;                       // the first position the lane reads
    const uint32_t line = (uint32_t)qf / lb;                           // the lane's one division
    const uint32_t col = (uint32_t)qf - line * lb;
    const int32_t off = (int32_t)(first + (int64_t)line * lw + col - stage0);
    uint32_t wl[4] = {0, 0, 0, 0}, wb[4] = {0, 0, 0, 0}, ws[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int32_t bad = 0;
    const FaWalk w = {lds, lds + FA_LDS, FA_GROUP - back, (int32_t)q0, qf, length, lb, eol, ga, (uint32_t)(gb - ga)};
    if (walk && q0 - back >= 0 && q0 + FA_GROUP <= length)
        walk_window<false>(w, col, off, wl, wb, ws, bad);              // inside the contig: no position is tested
    else if (walk)
        walk_window<true>(w, col, off, wl, wb, ws, bad);
    else
        ws[0] = ws[1] = ws[2] = ws[3] = ws[4] = ws[5] = ws[6] = ws[7] = 0x04040404u;
    if (bad) atomicOr(status, bad);
    if (q0 < length) {
        if (letters) store16(letters, q0, length, wl);
        if (blind) store16(blind, q0, length, wb);
    }
    if (scan) {
        // the lane's scan vector: bytes [vb, vb + 16) of the window, scan entries [s0, s0 + 16)
        const int32_t vb = d ? d : FA_GROUP;
        const int64_t s0 = q0 - FA_GROUP + vb + 1 - scan_pos0;
        if (s0 + 16 > 0 && s0 < scan_len) {
            const int32_t dd = vb >> 2, sh = 8 * (vb & 3);
            uint32_t v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int t = 0; t < 5; t++)                            // (dd is the same in every lane: no register is indexed at run time)
                    if (dd == t) lo = ws[t + i], hi = ws[t + i + 1];
                v[i] = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
            }
            if (s0 >= 0) {
                store16(scan, s0, scan_len, v);
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (s0 + k >= 0 && s0 + k < scan_len) scan[s0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

}   // namespace

extern "C" {

// See the header.  Runs on the context's stream and waits for it (the status word decides the return value).
int nc_fasta_decode(nc_ctx *ctx, const uint8_t *d_raw, int64_t raw_len, int64_t first, int64_t length, int64_t linebases, int64_t linewidth,
                    uint8_t *d_letters, uint8_t *d_scan, int64_t scan_pos0, int64_t scan_len, int64_t ga, int64_t gb, uint8_t *d_blind,
                    int32_t *d_status)
{
    if (!ctx) return NC_ERR_ARG;
    if (!d_raw || !d_status || raw_len < 0 || first < 0 || length < 1 || length > INT32_MAX - 2 * FA_BLOCK)
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: bad argument");
    if (linebases < 1 || linebases > INT32_MAX)
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: linebases %lld is not a line length", (long long)linebases);
    if (linewidth - linebases != 1 && linewidth - linebases != 2)
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: linewidth %lld - linebases %lld is neither 1 (\\n) nor 2 (\\r\\n)", (long long)linewidth,
                       (long long)linebases);
    if (((uintptr_t)d_letters | (uintptr_t)d_scan | (uintptr_t)d_blind) & 15)
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: the outputs must be 16-byte aligned");
    if (d_scan && (scan_len < 0 || scan_pos0 < -(int64_t)INT32_MAX || scan_pos0 > INT32_MAX))
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: bad scan grid");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    NC_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    const int64_t span = ((length - 1) / linebases) * linewidth + (length - 1) % linebases + 1;
    int32_t bad = 0;
    if (first > raw_len - span) {                                      // the .fai points past the end of the image: no launch
        bad = FA_BAD_SPAN;
        NC_HIP(ctx, hipMemcpyAsync(d_status, &bad, sizeof bad, hipMemcpyHostToDevice, st));
        NC_HIP(ctx, hipStreamSynchronize(st));
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: the .fai does not describe this file (the contig ends %lld bytes behind it)",
                       (long long)(first + span - raw_len));
    }
    if (ga < 1) ga = 1;
    if (gb > length) gb = length;
    bool scan_on = d_scan && scan_len > 0;
    int32_t d = 0;
    if (scan_on && gb < ga) {                                          // no position of the contig on the grid: every entry is 4
        NC_HIP(ctx, hipMemsetAsync(d_scan, 4, (size_t)scan_len, st));
        scan_on = false;
    }
    const int64_t n_groups = (length + FA_GROUP - 1) / FA_GROUP + 1;   // one spare: the scan vector that starts inside the last group
    if (scan_on) {
        d = (int32_t)((((scan_pos0 - 1) % FA_GROUP) + FA_GROUP) % FA_GROUP);
        // the entries no lane's vector covers, in front of the first and behind the last
        const int64_t s_lo = (d ? d - FA_GROUP : 0) + 1 - scan_pos0, s_hi = s_lo + n_groups * FA_GROUP;
        const int64_t head = s_lo < 0 ? 0 : s_lo < scan_len ? s_lo : scan_len;
        const int64_t tail = s_hi < 0 ? 0 : s_hi < scan_len ? s_hi : scan_len;
        if (head > 0) NC_HIP(ctx, hipMemsetAsync(d_scan, 4, (size_t)head, st));
        if (tail < scan_len) NC_HIP(ctx, hipMemsetAsync(d_scan + tail, 4, (size_t)(scan_len - tail), st));
    }
    if (d_letters || d_blind || scan_on) {
        const unsigned grid = (unsigned)((n_groups * FA_GROUP + FA_BLOCK - 1) / FA_BLOCK);
        hipLaunchKernelGGL(k_fasta_decode, dim3(grid), dim3(FA_LANES), 0, st, d_raw, raw_len, first, span, (int32_t)length, (uint32_t)linebases,
                           (uint32_t)linewidth, d_letters, scan_on ? d_scan : (uint8_t *)nullptr, scan_pos0, scan_len, (int32_t)ga, (int32_t)gb, d,
                           d_blind, d_status);
        NC_HIP(ctx, hipGetLastError());
    }
    NC_HIP(ctx, hipMemcpyAsync(&bad, d_status, sizeof bad, hipMemcpyDeviceToHost, st));
    NC_HIP(ctx, hipStreamSynchronize(st));
    if (bad)
        return nc_fail(ctx, NC_ERR_ARG, "nc_fasta_decode: the .fai does not describe this file (status %d:%s%s%s)", bad,
                       bad & FA_BAD_TERMINATOR ? " a line does not end where linebases says" : "", bad & FA_BAD_BASE ? " a control byte among the bases" : "",
                       bad & FA_BAD_SPAN ? " the contig ends behind the file" : "");
    return NC_OK;
}

}   // extern "C"

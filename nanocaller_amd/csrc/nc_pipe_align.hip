// Device indel pipeline, the alignment fill: Gotoh DP of a read window (star alignment, free tail) or a consensus (allele_prediction, global)
// against the site's reference window.  The kernels write traceback codes, nc_pipe_trace.hip walks them.
//   k_fill_band<C>  32 C diagonals around the path the CIGAR (or the consensus' columns) predicts, swept by anti-diagonals: the product route
//   k_fill16q<CPL>  the full matrix: band off, windows too wide for a band, paths that touched their band's edge, uncertified allele bands
// Both keep two alignments in the halves of every register (packed 16-bit arithmetic) and share recurrences and tie rules with nc_msa.hip's
// k_nw_fill16, the independent route the tests compare against.
#include <type_traits>

#include "nc_pipe.h"

namespace {
template <int NWP>
__device__ __forceinline__ void tw_stage(uint32_t *lds, int k, int t, int lane, const uint32_t *wd)
{
    uint32_t *ls = lds + ((k * TWB + (t & (TWB - 1))) * 64 + lane) * NWP;
    if (NWP == 1) ls[0] = wd[0];
    else if (NWP == 2) *reinterpret_cast<uint2 *>(ls) = make_uint2(wd[0], wd[1]);
    else *reinterpret_cast<uint4 *>(ls) = make_uint4(wd[0], wd[1], wd[2], 0u);
}
// the 8 steps of block t >> 3 of this lane, LDS (NWP words a step) -> its run in HBM (CPL words)
template <int CPL, int NWP>
__device__ __forceinline__ void tw_flush(const uint32_t *lds, int k, int t, int lane, int q, uint32_t *Tw, int64_t first_block)
{
    constexpr int F = CPL / 8, R = CPL % 8;
    uint32_t *dst = Tw + tw_run(first_block, t, q, CPL);
    uint32_t out[CPL];
#pragma unroll
    for (int w = 0; w < CPL; w++) out[w] = 0;
#pragma unroll
    for (int ts = 0; ts < TWB; ts++) {
        const uint32_t *ls = lds + ((k * TWB + ts) * 64 + lane) * NWP;
#pragma unroll
        for (int w = 0; w < F; w++) out[ts * F + w] = ls[w];
        if (R > 0) {
            const uint32_t part = ls[F] & ((1u << (4 * R)) - 1u);     // the step's last R codes (a step the lane never staged holds anything)
            const int pos = 4 * R * ts, dw = 8 * F + (pos >> 5), sh = pos & 31;
            out[dw] |= part << sh;
            if (sh + 4 * R > 32) out[dw + 1] |= part >> (32 - sh);
        }
    }
#pragma unroll
    for (int x = 0; x + 4 <= CPL; x += 4) *reinterpret_cast<U4 *>(dst + x) = U4{out[x], out[x + 1], out[x + 2], out[x + 3]};
#pragma unroll
    for (int x = CPL & ~3; x < CPL; x++) dst[x] = out[x];
}

// ---- Gotoh DP on the full matrix, 16 lanes per alignment, rows in registers (nc_msa.hip's k_nw_fill16: same recurrences and tie rules: an
// extension wins a tie against an opening, the diagonal against E, the better of them against F), CPL cells of a row per lane; lane q works on read
// row t - q at step t.  TWO alignments per 16-lane group: every score is an exact small integer (|H| < 5,500 + 1,300 for windows of
// <= 272 bases, consensus rows <= 1,024), so a lane keeps alignment A in the low and alignment B in the high 16 bits of each
// register and every recurrence is ONE packed 16-bit instruction for both (v_pk_sub_i16, v_pk_max_i16, ...).  The kernel is bound
// by vector issue (one alignment per group in 32-bit registers: 23.5 VALU per cell, ~70 % of the issue rate): packing halves the instructions per cell.
// Traceback bits (decoded by TbLine::code): bit 0 = E beats the diagonal, bit 1 = F beats both, bit 2 = E opened, bit 3 = F opened
// -- the raw sign bits of four differences, gathered by 32-bit and-ors.  22.6 vector
// instructions per cell pair: the registers hold H - open (what E's and F's openings need; the diagonal's `open` is folded into the score),
// the score is match + (mismatch - match) * min(base xor base, 1).
constexpr int NEG16 = -20000;              // "minus infinity": never selected, and NEG16 - extend - (any score) stays inside int16

// packed 16-bit VALU (two alignments per register).  Inline assembly: written as vector C the compiler turns the sign-mask
// arithmetic back into per-half compares and selects (measured: no fewer instructions than the 32-bit kernel).
#define NC_PK2(name, op)                                                                                     \
    __device__ __forceinline__ uint32_t name(uint32_t a, uint32_t b)                                         \
    {                                                                                                        \
        uint32_t r;                                                                                          \
        asm(op " %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));                                                    \
        return r;                                                                                            \
    }
NC_PK2(pk_sub, "v_pk_sub_i16")
NC_PK2(pk_add, "v_pk_add_i16")
NC_PK2(pk_max, "v_pk_max_i16")
NC_PK2(pk_min_u, "v_pk_min_u16")
#undef NC_PK2
__device__ __forceinline__ uint32_t pk_mad(uint32_t a, uint32_t b, uint32_t c)     // a * b + c per half (low 16 bits)
{
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// full-rate 32-bit ops on the packed pair (the traceback bits are gathered with these: the packed 16-bit forms issue at half rate)
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t b, uint32_t c)      // (a & b) | c
{
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t splat16(int v) { return ((uint32_t)v & 0xffffu) * 0x10001u; }
__device__ __forceinline__ uint32_t dpp_shr1_u(uint32_t old, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x111, 0xf, 0xf, false);
}
__device__ __forceinline__ int32_t half_of(uint32_t v, int k) { return k == 0 ? (int32_t)(int16_t)(v & 0xffffu) : (int32_t)(int16_t)(v >> 16); }

template <int CPL>
__global__ __launch_bounds__(64) void k_fill16q(FillArgs p)
{
    constexpr int NWD = (CPL + 7) / 8, NWP = NWD <= 1 ? 1 : NWD == 2 ? 2 : 4;
    constexpr int NH = (CPL + 3) / 4;                          // packed registers of 4 cells x 4 bits per alignment
    const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
    const int pair = blockIdx.x * 4 + g;
    const int A_live = p.count ? min(*p.count, p.A) : p.A;
    if ((int)blockIdx.x * 8 >= A_live) return;
    int al[2], n1[2], n2[2];                                          // al: the slot in Tw / Hlast / hcol (the alignment itself outside list mode)
    bool live[2];
    const uint8_t *s2[2];
    uint32_t s1o[2];                                                  // the read's bases at p.s1 + s1o (32-bit offsets and block indices: a register fewer each than 64-bit values)
    uint32_t arow[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int a = pair * 2 + k;
        live[k] = a < A_live;
        al[k] = live[k] ? a : 0;
        n1[k] = 0; n2[k] = 0;
        s1o[k] = 0; s2[k] = p.ref_code;
        arow[k] = 0;
        if (live[k]) {
            const int ain = p.list ? p.list[a] : a;
            arow[k] = p.arow ? (uint32_t)p.arow[ain] : (uint32_t)a * (uint32_t)tw_blocks(p.N1);      // (a row table is per alignment, a uniform pitch per slot)
            s1o[k] = (uint32_t)ain * (uint32_t)p.s1_stride;
            n1[k] = p.n1[ain];
            const int site = fill_site(p, ain);
            s2[k] = p.ref_code + (p.site_pos[site] - p.ref_pos0);
            n2[k] = p.site_n2[site];
        }
    }
    uint32_t H[CPL], F[CPL], rb[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        const int j = q * CPL + c + 1;
        H[c] = splat16(-2 * p.open - (j - 1) * p.extend);     // row 0.  H[] holds H - open throughout: that is what both the cell to the
        F[c] = splat16(NEG16);                                 // right (E's opening) and the cell below (F's) need; the diagonal adds `open` back inside the score
        const uint32_t r0 = j <= n2[0] ? (uint32_t)s2[0][j - 1] : 8u, r1 = j <= n2[1] ? (uint32_t)s2[1][j - 1] : 8u;     // 8: no read base equals it
        rb[c] = r0 | (r1 << 16);
    }
    int nmax = max(n1[0], n1[1]);
    nmax = max(nmax, __shfl_xor(nmax, 16));
    nmax = max(nmax, __shfl_xor(nmax, 32));
    __shared__ uint32_t tw_lds[2 * TWB * 64 * NWP];
    const uint32_t k_open = splat16(p.open), k_ext = splat16(p.extend), k_match = splat16(p.match + p.open), k_dmis = splat16(p.mismatch - p.match);
    const uint32_t k_one = splat16(1);
    uint32_t h_out = 0, e_out = splat16(NEG16);
    uint32_t h_in_prev = splat16(q == 0 ? -p.open : -2 * p.open - (q * CPL - 1) * p.extend);     // H[0][q*CPL] - open
    int jn_lane[2], jn_c[2];
#pragma unroll
    for (int k = 0; k < 2; k++) { jn_lane[k] = (n2[k] - 1) / CPL; jn_c[k] = (n2[k] - 1) % CPL; }
    const int n2_first = __builtin_amdgcn_readfirstlane(n2[0]);
    const int jc_uni = __all(n2[0] == n2_first && n2[1] == n2_first && n2_first > 0) ? (n2_first - 1) % CPL : -1;      // wave-uniform (scalar)
    // read bases of both alignments (packed): lane q of a group holds base 16*blk + q; lane 0 takes base t-1 from lane (t-1) & 15, the others get
    // theirs from the lane to their left one step later (by DPP instead of a byte load per step)
    auto load_chunk = [&](int idx) {
        const uint32_t b0 = idx < n1[0] ? (uint32_t)p.s1[s1o[0] + (uint32_t)idx] : 4u, b1 = idx < n1[1] ? (uint32_t)p.s1[s1o[1] + (uint32_t)idx] : 4u;
        return b0 | (b1 << 16);
    };
    uint32_t chunk = load_chunk(q), chunk_nxt = load_chunk(16 + q), c1 = splat16(4);
    for (int t = 1; t <= nmax + 15; t++) {
        const int i = t - q;
        if (t > 1 && ((t - 1) & 15) == 0) {
            chunk = chunk_nxt;
            chunk_nxt = load_chunk(t - 1 + 16 + q);
        }
        const uint32_t c_new = (uint32_t)__shfl((int)chunk, (lane & 48) | ((t - 1) & 15));
        c1 = dpp_shr1_u(splat16(4), c1);
        if (q == 0) c1 = c_new;
        uint32_t nh = dpp_shr1_u(0u, h_out), ne = dpp_shr1_u(splat16(NEG16), e_out);
        if (q == 0) {
            nh = splat16(-2 * p.open - (i - 1) * p.extend);   // H[i][0] - open
            ne = splat16(NEG16);
        }
        if (i >= 1) {                                          // rows beyond a read's end compute values nothing reads
            uint32_t hdiag = h_in_prev, hleft = nh, e = ne;
            uint32_t words[NH + 1];
#pragma unroll
            for (int k = 0; k <= NH; k++) words[k] = 0;
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                const uint32_t hup = H[c], fup = F[c];
                const uint32_t e_ext = pk_sub(e, k_ext);                             // (E's opening = hleft, F's = hup: both already H - open)
                const uint32_t d_e = pk_sub(e_ext, hleft);                           // < 0: E opened
                e = pk_max(hleft, e_ext);
                const uint32_t f_ext = pk_sub(fup, k_ext);
                const uint32_t d_f = pk_sub(f_ext, hup);                             // < 0: F opened
                const uint32_t f = pk_max(hup, f_ext);
                const uint32_t ne_b = pk_min_u(c1 ^ rb[c], k_one);                   // 1: the bases differ
                const uint32_t d = pk_add(hdiag, pk_mad(ne_b, k_dmis, k_match));     // (H - open of the diagonal) + score + open
                const uint32_t h1 = pk_max(d, e);
                const uint32_t d_1 = pk_sub(d, e);                                   // < 0: E beats the diagonal
                const uint32_t hh = pk_max(h1, f);
                const uint32_t d_2 = pk_sub(h1, f);                                  // < 0: F beats both
                const uint32_t h = pk_sub(hh, k_open);
                H[c] = h;
                F[c] = f;
                // the four sign bits of each half -> its 4-bit code (d_1 bit 0, d_2 bit 1, d_e bit 2, d_f bit 3), with 32-bit shifts and
                // and-ors (full rate; the bits of the two halves never meet), then into the row's words
                uint32_t acc = d_1 & 0x80008000u;                                    // (the first one in ends lowest)
                acc = and_or(d_2, 0x80008000u, acc >> 1);
                acc = and_or(d_e, 0x80008000u, acc >> 1);
                acc = and_or(d_f, 0x80008000u, acc >> 1);
                words[c >> 2] |= (acc >> 12) << ((c & 3) * 4);
                hdiag = hup;
                hleft = h;
            }
            h_out = hleft;
            e_out = e;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (!(live[k] && i <= n1[k] && q * CPL < n2[k])) continue;
                uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < NWD; j++) {
                    const uint32_t lo = words[2 * j], hi = words[2 * j + 1 <= NH ? 2 * j + 1 : NH];
                    wd[j] = __builtin_amdgcn_perm(hi, lo, k == 0 ? 0x05040100u : 0x07060302u);      // this alignment's halves of the two registers: one v_perm_b32
                }
                tw_stage<NWP>(tw_lds, k, t, lane, wd);
                if (p.hcol && q == jn_lane[k]) {
                    uint32_t hv = H[0];
                    if (jc_uni >= 0) {                               // every window of the wave has the same length: the cell is picked by a scalar branch
                        switch (jc_uni) {
#define NC_HV(C) case C: hv = H[C < CPL ? C : 0]; break;
                            NC_HV(1) NC_HV(2) NC_HV(3) NC_HV(4) NC_HV(5) NC_HV(6) NC_HV(7) NC_HV(8) NC_HV(9) NC_HV(10) NC_HV(11) NC_HV(12) NC_HV(13)
                            NC_HV(14) NC_HV(15) NC_HV(16)
#undef NC_HV
                        default: break;
                        }
                    } else {
#pragma unroll
                        for (int c = 1; c < CPL; c++) hv = c == jn_c[k] ? H[c] : hv;
                    }
                    p.hcol[(int64_t)al[k] * hcol_pitch(p.N1) + i] = half_of(hv, k) + p.open;
                }
                if (p.Hlast && i == n1[k]) {
#pragma unroll
                    for (int c = 0; c < CPL; c++)
                        if (q * CPL + c + 1 <= n2[k]) p.Hlast[(int64_t)al[k] * hlast_pitch(p.W) + q * CPL + c + 1] = half_of(H[c], k) + p.open;
                }
            }
            h_in_prev = nh;
        }
        if ((t & (TWB - 1)) == TWB - 1 || t == nmax + 15) {
#pragma unroll
            for (int k = 0; k < 2; k++)
                if (live[k] && (t >> TWB_LOG) < tw_blocks(n1[k])) tw_flush<CPL, NWP>(tw_lds, k, t, lane, q, p.Tw, arow[k]);
        }
    }
}

// ---- the banded form.  Every read window was rebuilt from the reference and the read's own CIGAR events (k_windows), so the diagonals
// d = j - i the optimal path can visit are known up front: the range the CIGAR's path covers inside the window plus a margin.  The band
// of B = 32 C diagonals [lo, lo + B) (lo even) is swept by ANTI-DIAGONALS a = i + j: on an even a the band's even diagonals hold a cell,
// on an odd a the odd ones, B / 2 cells either way -- one (C = 1) or two (C = 2) per lane of a 16-lane group, all independent:
//     lane q, cell c, x = q C + c:   a even: d = lo + 2 x        a odd: d = lo + 2 x + 1          i = (a - d) / 2, j = (a + d) / 2
//     left (i, j-1) = diagonal d - 1 of a - 1:   a odd: the same lane cell     a even: lane cell x - 1 (row_shr:1 across lanes)
//     up   (i-1, j) = diagonal d + 1 of a - 1:   a odd: lane cell x + 1 (row_shl:1)     a even: the same lane cell
//     diag (i-1, j-1) = diagonal d of a - 2:     the same lane cell
// so a lane cell walks a staircase down its pair of diagonals: j grows on odd steps (the reference bases move one lane cell down, a new one
// enters at the top lane), i on even steps (the read bases move one lane cell up, a new one enters at lane 0).  321 steps of one or two
// cells replace 175 steps of 11 (k_fill16q), and 4 bits per cell and step leave as ONE word per lane and 8 steps: 2.6 KB of traceback
// codes per alignment instead of 19 KB.  Cells outside the rectangle compute bounded garbage nothing reads: H(0,0) = 0 is planted in the
// registers of step 0, everything around it starts at "minus infinity", and the recurrence itself then produces row 0 and column 0
// (E / F chains from the origin).  Cells outside the band read as minus infinity (what a DPP shift hands the lanes at a row's end).  Two alignments per
// group in the halves of every register, arithmetic and tie rules exactly those of k_fill16q; a path that touches an edge diagonal of the
// band is re-run on the full matrix (k_trace_band -> listF).
__device__ __forceinline__ uint32_t dpp_shl1_u(uint32_t old, uint32_t v)          // lane q <- lane q + 1; the row's last lane keeps `old`
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x101, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t dpp_shl1_z(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true); }   // ... gets 0
__device__ __forceinline__ uint32_t dpp_shr1_z(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t dpp_ror_u(uint32_t v, int n)                   // lane q <- lane (q - n) mod 16
{
    return n == 1 ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, true)        // (a rotation has a source for every lane: with bound_ctrl
                  : (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x12f, 0xf, 0xf, true);       // the `old` operand need not be initialised)
}

template <int C>
__global__ __launch_bounds__(64) void k_fill_band(BandArgs p)
{
    constexpr int B = 32 * C;
    __shared__ __attribute__((aligned(16))) uint32_t tws[2][64][4 * C];
    const int cnt = *p.count;
    if ((int)blockIdx.x * 8 >= cnt) return;
    const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
    const int pair = blockIdx.x * 4 + g;
    const FillArgs &f = p.f;
    int al[2], n1[2], n2[2], l0[2];
    bool live[2];
    const uint8_t *s1[2], *s2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int a = pair * 2 + k;
        live[k] = a < cnt;
        al[k] = p.list[live[k] ? a : 0];
        s1[k] = f.s1 + (int64_t)al[k] * f.s1_stride;
        const int site = fill_site(f, al[k]);
        s2[k] = f.ref_code + (f.site_pos[site] - f.ref_pos0);
        n1[k] = live[k] ? f.n1[al[k]] : 0;
        n2[k] = live[k] ? f.site_n2[site] : 0;
        l0[k] = -(int)p.band_lo[al[k]] / 2;
    }
    // scores carry the bias -NEG16 (H' = H + 20000, likewise E and F): minus infinity is 0, which is what a DPP shift with bound_ctrl hands
    // the lanes at a row's end -- no `old` operand to load; every recurrence is linear in the bias
    constexpr int BIAS = -NEG16;
    const uint32_t k_open = splat16(f.open), k_ext = splat16(f.extend), k_match = splat16(f.match + f.open), k_dmis = splat16(f.mismatch - f.match);
    const uint32_t k_one = splat16(1);
    auto rd_base = [&](int k, int idx) -> uint32_t { return idx >= 0 && idx < n1[k] ? (uint32_t)s1[k][idx] : 4u; };      // string index -> code; 4 / 8 never match
    auto rf_base = [&](int k, int idx) -> uint32_t { return idx >= 0 && idx < n2[k] ? (uint32_t)s2[k][idx] : 8u; };
    // state of anti-diagonal 0 (H holds H - open, as in k_fill16q)
    uint32_t Hp1[C], Hp2[C], Ep1[C], Fp1[C], rd[C], rf[C];
    int di[2][C];                                                       // row of this lane cell at a = 0 (its column is the negative)
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int x = q * C + c;
        di[0][c] = l0[0] - x;
        di[1][c] = l0[1] - x;
        const uint32_t h0 = (uint32_t)(x == l0[0] ? BIAS - f.open : 0) & 0xffffu, h1 = (uint32_t)(x == l0[1] ? BIAS - f.open : 0) & 0xffffu;
        Hp1[c] = h0 | (h1 << 16);
        Hp2[c] = 0; Ep1[c] = 0; Fp1[c] = 0;
        rd[c] = rd_base(0, di[0][c] - 1) | (rd_base(1, di[1][c] - 1) << 16);
        rf[c] = rf_base(0, -di[0][c] - 1) | (rf_base(1, -di[1][c] - 1) << 16);
    }
    // the streams of bases that enter: read element e = string index l0 + e at lane 0 (lane q of a chunk holds element 16 blk + q, the chunk
    // rotates left after every entry); reference element e = string index 16 C - 1 - l0 + e at lane 15 (lane q holds 16 blk + 15 - q, rotates right)
    auto rd_chunk = [&](int blk) -> uint32_t { return rd_base(0, l0[0] + 16 * blk + q) | (rd_base(1, l0[1] + 16 * blk + q) << 16); };
    auto rf_chunk = [&](int blk) -> uint32_t {
        return rf_base(0, 16 * C - 1 - l0[0] + 16 * blk + 15 - q) | (rf_base(1, 16 * C - 1 - l0[1] + 16 * blk + 15 - q) << 16);
    };
    uint32_t ch_rd = rd_chunk(0), ch_rf = rf_chunk(0), ch_rd_n = rd_chunk(1), ch_rf_n = rf_chunk(1);
    int nb[2], nbw = 0, a_tail = 1 << 20;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        nb[k] = live[k] ? (n1[k] + n2[k] + 7) >> 3 : 0;
        nbw = max(nbw, nb[k]);
        if (live[k]) a_tail = min(a_tail, min(2 * n1[k] - 2 * l0[k], 2 * n2[k] + 2 * l0[k] - B + 1));      // first step with a cell in the last row / column
    }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
        nbw = max(nbw, __shfl_xor(nbw, o));
        a_tail = min(a_tail, __shfl_xor(a_tail, o));
    }
    nbw = __builtin_amdgcn_readfirstlane(nbw);
    const int b_tail = p.hrow ? __builtin_amdgcn_readfirstlane(max(0, (a_tail - 1) >> 3)) : nbw;      // (a global alignment ends at the corner: no last row / column to keep)
    uint32_t P[4] = {0, 0, 0, 0};
    // one step.  ODD: the reference base moves (j grows); even: the read base (i grows).  TAIL: the cells of the last row / last column leave
    auto step = [&](auto odd_tag, auto tail_tag, int a, int s) {
        constexpr bool ODD = decltype(odd_tag)::value, TAIL = decltype(tail_tag)::value;
        uint32_t hl[C], el[C], hu[C], fu[C];
        if (ODD) {
            const uint32_t rot = dpp_ror_u(ch_rf, 1);                   // (rotated first: the entry below then overwrites the chunk register in place, no copy)
            const uint32_t top = dpp_shl1_u(ch_rf, rf[0]);
#pragma unroll
            for (int c = 0; c + 1 < C; c++) rf[c] = rf[c + 1];
            rf[C - 1] = top;
            ch_rf = rot;
            const uint32_t hn = dpp_shl1_z(Hp1[0]), fn = dpp_shl1_z(Fp1[0]);
#pragma unroll
            for (int c = 0; c < C; c++) {
                hl[c] = Hp1[c]; el[c] = Ep1[c];
                hu[c] = c + 1 < C ? Hp1[c + 1 < C ? c + 1 : 0] : hn;
                fu[c] = c + 1 < C ? Fp1[c + 1 < C ? c + 1 : 0] : fn;
            }
        } else {
            const uint32_t rot = dpp_ror_u(ch_rd, 15);
            const uint32_t bot = dpp_shr1_u(ch_rd, rd[C - 1]);
#pragma unroll
            for (int c = C - 1; c > 0; c--) rd[c] = rd[c - 1];
            rd[0] = bot;
            ch_rd = rot;
            const uint32_t hn = dpp_shr1_z(Hp1[C - 1]), en = dpp_shr1_z(Ep1[C - 1]);
#pragma unroll
            for (int c = 0; c < C; c++) {
                hu[c] = Hp1[c]; fu[c] = Fp1[c];
                hl[c] = c > 0 ? Hp1[c > 0 ? c - 1 : 0] : hn;
                el[c] = c > 0 ? Ep1[c > 0 ? c - 1 : 0] : en;
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            const uint32_t e_ext = pk_sub(el[c], k_ext);
            const uint32_t d_e = pk_sub(e_ext, hl[c]);                           // < 0: E opened
            const uint32_t e = pk_max(hl[c], e_ext);
            const uint32_t f_ext = pk_sub(fu[c], k_ext);
            const uint32_t d_f = pk_sub(f_ext, hu[c]);                           // < 0: F opened
            const uint32_t ff = pk_max(hu[c], f_ext);
            const uint32_t ne_b = pk_min_u(rd[c] ^ rf[c], k_one);
            const uint32_t d = pk_add(Hp2[c], pk_mad(ne_b, k_dmis, k_match));
            const uint32_t h1 = pk_max(d, e);
            const uint32_t d_1 = pk_sub(d, e);                                   // < 0: E beats the diagonal
            const uint32_t hh = pk_max(h1, ff);
            const uint32_t d_2 = pk_sub(h1, ff);                                 // < 0: F beats both
            const uint32_t h = pk_sub(hh, k_open);
            // the cell's four sign bits join the register of its group of four cells (16 bits a half: the first cell in ends lowest)
            const int cell = s * C + c;                                          // cell of the block: 8 C of them, four to a register
            uint32_t &Pr = P[cell >> 2];
            Pr = (cell & 3) == 0 ? (d_1 & 0x80008000u) : and_or(d_1, 0x80008000u, Pr >> 1);
            Pr = and_or(d_2, 0x80008000u, Pr >> 1);
            Pr = and_or(d_e, 0x80008000u, Pr >> 1);
            Pr = and_or(d_f, 0x80008000u, Pr >> 1);
            Hp2[c] = Hp1[c];
            Hp1[c] = h; Ep1[c] = e; Fp1[c] = ff;
        }
        if (TAIL) {
#pragma unroll
            for (int c = 0; c < C; c++)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int i = (a >> 1) + di[k][c], j = ((a + 1) >> 1) - di[k][c];
                    const int kk = 2 * (q * C + c) + (ODD ? 1 : 0);
                    const int32_t hv = half_of(Hp1[c], k) - BIAS + f.open;
                    if (live[k] && i == n1[k] && j >= 0 && j <= n2[k]) p.hrow[(int64_t)al[k] * 64 + kk] = (int16_t)hv;
                    if (live[k] && j == n2[k] && i >= 0 && i < n1[k]) p.hcolb[(int64_t)al[k] * 64 + kk] = (int16_t)hv;
                }
        }
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    for (int b = 0; b < nbw; b++) {
        if ((b & 3) == 0 && b > 0) {                                       // 16 bases of either stream are used up every four blocks
            ch_rd = ch_rd_n; ch_rf = ch_rf_n;
            ch_rd_n = rd_chunk((b >> 2) + 1); ch_rf_n = rf_chunk((b >> 2) + 1);
        }
        const int a0 = 8 * b + 1;
        if (b < b_tail) {
#pragma unroll
            for (int s = 0; s < 8; s += 2) { step(T_{}, F_{}, a0 + s, s); step(F_{}, F_{}, a0 + s + 1, s + 1); }
        } else {
#pragma unroll
            for (int s = 0; s < 8; s += 2) { step(T_{}, T_{}, a0 + s, s); step(F_{}, T_{}, a0 + s + 1, s + 1); }
        }
        // the block's codes wait in LDS (a lane reads back only what it wrote) until four blocks -- 32 anti-diagonals -- are together: they leave as
        // 16 C bytes per lane, so that a 64-byte line holds 8 diagonals x 32 steps (the traceback stays on a line for ~32 steps instead of 8)
        const int bb = b & 3;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint32_t sel = k == 0 ? 0x05040100u : 0x07060302u;
            uint32_t *ls = &tws[k][lane][bb * C];
            if (C == 1) ls[0] = __builtin_amdgcn_perm(P[1], P[0], sel);
            else *reinterpret_cast<uint2 *>(ls) = make_uint2(__builtin_amdgcn_perm(P[1], P[0], sel), __builtin_amdgcn_perm(P[3], P[2], sel));
        }
        if (bb == 3 || b == nbw - 1) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (!(live[k] && (b & ~3) < nb[k])) continue;
                uint4 *dst = reinterpret_cast<uint4 *>(p.Twb + (int64_t)al[k] * p.NBLK * TWB_PITCH + ((b >> 2) * (16 * C + 4) + q * C + 2) * 4);
                const uint4 *src = reinterpret_cast<const uint4 *>(&tws[k][lane][0]);
#pragma unroll
                for (int u = 0; u < C; u++) dst[u] = src[u];
            }
        }
    }
}

}   // namespace

void nc_pipe_launch_fill(hipStream_t st, int CPL, const FillArgs &fa)
{
    const dim3 gq((unsigned)((fa.A + 7) / 8));
    if (CPL == 4) hipLaunchKernelGGL(k_fill16q<4>, gq, dim3(64), 0, st, fa);
    else if (CPL == 8) hipLaunchKernelGGL(k_fill16q<8>, gq, dim3(64), 0, st, fa);
    else if (CPL == 11) hipLaunchKernelGGL(k_fill16q<11>, gq, dim3(64), 0, st, fa);
    else hipLaunchKernelGGL(k_fill16q<17>, gq, dim3(64), 0, st, fa);
}
// every alignment of the group or set list on its band: the classes' sizes are known on the device only, so both grids cover f.A alignments and the
// blocks beyond a class's count leave at once
void nc_pipe_launch_fill_band(hipStream_t st, const BandArgs &b1, const BandArgs &b2)
{
    hipLaunchKernelGGL(k_fill_band<1>, dim3((b1.f.A + 7) / 8), dim3(64), 0, st, b1);
    hipLaunchKernelGGL(k_fill_band<2>, dim3((b2.f.A + 7) / 8), dim3(64), 0, st, b2);
}

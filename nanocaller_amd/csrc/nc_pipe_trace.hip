// Device indel pipeline, the tracebacks: the walks over the codes nc_pipe_align.hip's kernels wrote.
//   k_trace_band12      star alignment on its band -> alignment in reference coordinates; a path on an edge diagonal joins the redo list
//   k_end_cells         free-tail end point of the full-matrix alignments (the redo list, or all of them with the band off)
//   k_trace16p          their traceback
//   k_allele_trace_b12  allele_prediction (:77-127) on a banded global alignment that certifies itself, else onto the redo list
//   k_allele_trace16p   ... on the full matrix
//   k_band_stats        the group's class counts into the run's totals
#include "nc_pipe.h"

namespace {
enum : uint32_t { T_DIAG = 0, T_DEL = 1, T_INS = 2, T_EEXT = 4, T_FEXT = 8 };

// The line cache of a banded traceback (TbLine's role).  k_fill_band stores the codes of four blocks of 8 anti-diagonals -- a superblock of 32 -- as
// 4 C words per lane: the words of cell x = q C + c of superblock sb at ((sb * (16 C + 4) + x + 2) * 4), block bb = 0 .. 3 of the superblock at + bb
// (C = 2: a lane's two cells share their words: + bb * 2 + h, steps 0-3 and 4-7 of both).  A 64-byte line is therefore 4 cells = 8 diagonals x 32
// steps: the walk changes lines every ~32 steps (every 8 when a line was one block of all 32 diagonals: 41 lines per alignment instead of ~13, 4.3 GB
// read per pass for 0.2 GB of path codes).  The two empty cell slots in front shift the lines by half a line: the middle of the band -- where
// k_windows put the CIGAR's own diagonals -- is the middle of a line, not the border between two.
// One line per walking lane in LDS, re-fetched in epochs.
template <int C>
struct TbBand {
    static constexpr int B = 32 * C;
    uint32_t *slot;                                                    // this lane's 16 words in LDS (odd pitch)
    const uint32_t *tw;                                                // the alignment's codes
    int lo, ckey, edge;
    bool touched;
    U4 pre[4];                                                         // the line one superblock further down the path (same group of diagonals), in flight or arrived
    int pkey;
    __device__ __forceinline__ int key(int i, int j) const { return ((i + j - 1) >> 5) * 16 + ((((j - i - lo) >> 1) + 2) >> 2); }      // (superblock, line)
    __device__ __forceinline__ bool has(int i, int j) const { return key(i, j) == ckey; }
    // the same from the walk's running coordinates: a = i + j - 1 (anti-diagonal), kd = j - i - lo (diagonal of the band)
    __device__ __forceinline__ int key_akd(int a, int kd) const { return (a >> 5) * 16 + (((kd >> 1) + 2) >> 2); }
    __device__ __forceinline__ uint32_t raw(int a, int kd) const          // the cell's four sign bits (any a, kd: the index stays inside the slot)
    {
        const int s = a & 7, bb = (a >> 3) & 3, xx = kd >> 1;
        if (C == 1) return (slot[((xx + 2) & 3) * 4 + bb] >> (4 * s)) & 15u;
        return (slot[(((xx >> 1) + 1) & 1) * 8 + bb * 2 + (s >> 2)] >> (4 * ((s & 3) * 2 + (xx & 1)))) & 15u;
    }
    __device__ __forceinline__ const U4 *line(int k) const { return reinterpret_cast<const U4 *>(tw + (k >> 4) * (64 * C + 16) + (k & 15) * 16); }
    __device__ __forceinline__ void to_slot(const U4 *v)
    {
#pragma unroll
        for (int u = 0; u < 4; u++) { slot[4 * u] = v[u].x; slot[4 * u + 1] = v[u].y; slot[4 * u + 2] = v[u].z; slot[4 * u + 3] = v[u].w; }
    }
    __device__ __forceinline__ void prefetch(int k)
    {
        pkey = k >= 0 ? k : -1;
        if (k >= 0) {
            const U4 *src = line(k);
#pragma unroll
            for (int u = 0; u < 4; u++) pre[u] = src[u];
        }
    }
    // demand load of the line of (i, j) (the wave waits for it), and the request for the one the path most likely enters next
    __device__ __forceinline__ void load(int i, int j)
    {
        ckey = key(i, j);
        const U4 *src = line(ckey);
        U4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = src[u];
        prefetch(ckey - 16);
        to_slot(v);
    }
    // the line of (i, j) into the slot at an epoch's start: from the prefetch registers when the guess was right (no memory wait), else from memory.
    // (Taking a prefetched line inside the walk, lane by lane as each one leaves its line, was tried: the wave then runs the 40-instruction hand-over
    // ~800 times instead of 13 epochs -- 0.96 -> 1.99 ms.)
    __device__ __forceinline__ void fetch(int i, int j)
    {
        const int k = key(i, j);
        if (k == pkey) {
            to_slot(pre);
            ckey = k;
            prefetch(k - 16);
        } else load(i, j);
    }
    // cell (i, j), i, j > 0, of the cached line as a T_* code; notes a cell on (or within `edge` of) an edge diagonal of the band
    __device__ __forceinline__ uint32_t code(int i, int j)
    {
        const int k = j - i - lo, a = i + j - 1, s = a & 7, bb = (a >> 3) & 3, xx = k >> 1;
        touched |= k <= edge || k >= B - 1 - edge;
        uint32_t tc;
        if (C == 1) tc = (slot[((xx + 2) & 3) * 4 + bb] >> (4 * s)) & 15u;
        else tc = (slot[(((xx >> 1) + 1) & 1) * 8 + bb * 2 + (s >> 2)] >> (4 * ((s & 3) * 2 + (xx & 1)))) & 15u;
        return ((tc & 2u) ? (uint32_t)T_INS : (tc & 1u) ? (uint32_t)T_DEL : (uint32_t)T_DIAG) | ((tc & 4u) ? 0u : (uint32_t)T_EEXT) | ((tc & 8u) ? 0u : (uint32_t)T_FEXT);
    }
};
constexpr int TBB_PITCH = 17;

// traceback of a banded alignment: k_trace16p's walk and entries.  The end point (best cell of the last row, ties to the larger column, or a strictly
// better cell of the last column, ties to the larger row) comes from the band's 2 x B last-row / last-column values.
template <int C>
__device__ __forceinline__ void trace_band_body(const BandArgs &p, uint32_t *__restrict__ ent_all, int32_t EW, uint32_t *stage, uint32_t *tbl)
{
    constexpr int B = 32 * C;
    const int cnt = *p.count;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= cnt) return;
    const int lane = threadIdx.x;
    const FillArgs &f = p.f;
    const int al = p.list[idx];
    const int n1 = f.n1[al], n2 = f.site_n2[fill_site(f, al)], lo = p.band_lo[al];
    TbBand<C> tb;
    tb.slot = tbl + lane * TBB_PITCH; tb.tw = p.Twb + (int64_t)al * p.NBLK * TWB_PITCH; tb.lo = lo; tb.ckey = -1; tb.edge = p.edge; tb.touched = false; tb.pkey = -1;
    uint32_t *ent = ent_all + (int64_t)al * EW;
    int i = n1, j = n2;
    if (n1 > 0 && n2 > 0) {
        int32_t rv = INT32_MIN, cv = INT32_MIN;
        int rj = 0, ci = 0;
        const int16_t *hr = p.hrow + (int64_t)al * 64, *hc = p.hcolb + (int64_t)al * 64;
        for (int k0 = 0; k0 < B; k0 += 8) {
            const uint4 gr = *reinterpret_cast<const uint4 *>(hr + k0), gc = *reinterpret_cast<const uint4 *>(hc + k0);
            const uint32_t wr[4] = {gr.x, gr.y, gr.z, gr.w}, wc[4] = {gc.x, gc.y, gc.z, gc.w};
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int k = k0 + u;
                const int32_t vr = (int16_t)(wr[u >> 1] >> ((u & 1) * 16)), vc = (int16_t)(wc[u >> 1] >> ((u & 1) * 16));
                const int jr = n1 + lo + k, ic = n2 - lo - k;
                if (jr >= 0 && jr <= n2 && vr >= rv) { rv = vr; rj = jr; }
                if (ic >= 0 && ic < n1 && vc > cv) { cv = vc; ci = ic; }
            }
        }
        if (cv > rv) { i = ci; j = n2; } else { i = n1; j = rj; }
    }
    uint32_t cur = 0;
    if (i < n1) cur = ((uint32_t)(n1 - i) << 10) | ((uint32_t)i << 20);       // the rest of the read: insertion after the window
    int x = n2;
    auto put = [&](uint32_t e) {
        stage[(x & 15) * 64 + lane] = e;
        if ((x & 15) == 0) {
#pragma unroll
            for (int u = 0; u < 4; u++)
                reinterpret_cast<uint4 *>(ent + (x & ~15))[u] = make_uint4(stage[(4 * u) * 64 + lane], stage[(4 * u + 1) * 64 + lane],
                                                                           stage[(4 * u + 2) * 64 + lane], stage[(4 * u + 3) * 64 + lane]);
        }
        x--;
    };
    while (x > j) put(0u);
    int state = -1;
    int a = i + j - 1, kd = j - i - lo;                                // running coordinates of the cell (anti-diagonal, diagonal of the band)
    // one step of the walk without branches but the one around put(): the round-4 form (a chain of if / else per state and border) ran ~200
    // instructions per step once the lanes of a wave sat in different states -- this kernel's time
    auto step = [&]() {
        const bool bi = i == 0, bj = j == 0;
        const uint32_t tc = tb.raw(a, kd);
        int w = (tc & 2u) ? 2 : (int)(tc & 1u);                        // 0 diagonal, 1 deletion (E), 2 insertion (F)
        bool eext = !(tc & 4u), fext = !(tc & 8u);
        w = bi ? 1 : bj ? 2 : w;                                       // row 0 / column 0: a gap to the origin
        eext = bi ? j > 1 : eext;
        fext = bj && !bi ? i > 1 : fext;
        tb.touched |= !bi && !bj && (kd <= tb.edge || kd >= B - 1 - tb.edge);
        const int wm = state < 0 ? w : state;
        const bool mv_d = wm == 0, mv_e = wm == 1;
        if (mv_d || mv_e) put(cur);
        const uint32_t cur_ins = (cur & 0x3ffu) | ((((cur >> 10) & 0x3ffu) + 1u) << 10) | ((uint32_t)(i - 1) << 20);
        cur = mv_d ? (uint32_t)i : mv_e ? 0u : cur_ins;
        const bool ext = mv_e ? eext : fext;
        state = (mv_d || !ext) ? -1 : wm;
        i -= mv_e ? 0 : 1;
        j -= (mv_d || mv_e) ? 1 : 0;
        a -= mv_d ? 2 : 1;
        kd += mv_d ? 0 : mv_e ? -1 : 1;
    };
    while (__any(i > 0 || j > 0)) {                                    // epochs: the lanes that left their line load the next one together
        if (i > 0 && j > 0 && tb.key_akd(a, kd) != tb.ckey) tb.fetch(i, j);
        for (;;) {
            const bool can = (i > 0 || j > 0) && (i == 0 || j == 0 || tb.key_akd(a, kd) == tb.ckey);
            if (!__any(can)) break;
            if (can) step();
        }
    }
    put(cur);
    if (tb.touched) p.redo_list[atomicAdd(p.redo_count, 1)] = al;
}
// both band widths in one launch (blockIdx.y): the 64-diagonal class is a fifteenth of the alignments, on its own a launch of one wave per SIMD
// whose time is the latency of a single traceback
__global__ __launch_bounds__(64) void k_trace_band12(BandArgs p1, BandArgs p2, uint32_t *__restrict__ ent_all, int32_t EW)
{
    __shared__ uint32_t stage[16 * 64];
    __shared__ uint32_t tbl[64 * TBB_PITCH];
    if (blockIdx.y == 0) trace_band_body<1>(p1, ent_all, EW, stage, tbl);
    else trace_band_body<2>(p2, ent_all, EW, stage, tbl);
}

// free-tail end point of every alignment: the best cell of the last row (ties: the larger column) or a cell of the last column that is
// strictly better (ties: the larger row) -- the order k_nw_trace16 scans them in.  16 lanes per alignment over Hlast / hcol (one lane per
// alignment inside the traceback kernel read its ~360 values one after the other: 2.4 of that kernel's 4.5 ms)
__global__ __launch_bounds__(256) void k_end_cells(FillArgs p)
{
    const int al = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    const int A_live = p.count ? min(*p.count, p.A) : p.A;
    const bool live = al < A_live;
    const int a = live ? al : 0;                                       // slot
    const int ain = p.list ? p.list[a] : a;
    const int n1 = p.n1[ain], n2 = p.site_n2[fill_site(p, ain)];
    int32_t rv = INT32_MIN, rj = 0, cv = INT32_MIN, ci = 0;
    if (live && n1 > 0 && n2 > 0) {
        // four values a load (both rows are 16-byte aligned: hlast_pitch and hcol_pitch are multiples of four words); any split of the
        // indices over the lanes will do, the reduction below orders (value, index) pairs
        const int32_t *hl = p.Hlast + (int64_t)a * hlast_pitch(p.W), *hc = p.hcol + (int64_t)a * hcol_pitch(p.N1);
        for (int j0 = 4 * l; j0 <= n2; j0 += 64) {
            const int4 g = *reinterpret_cast<const int4 *>(hl + j0);
            const int32_t gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + u;
                const int32_t v = j > 0 ? gv[u] : -p.open - (n1 - 1) * p.extend;
                if (j <= n2 && v >= rv) { rv = v; rj = j; }
            }
        }
        for (int i0 = 4 * l; i0 < n1; i0 += 64) {
            const int4 g = *reinterpret_cast<const int4 *>(hc + i0);
            const int32_t gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u;
                const int32_t v = i > 0 ? gv[u] : -p.open - (n2 - 1) * p.extend;
                if (i < n1 && v >= cv) { cv = v; ci = i; }
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const int32_t ov = __shfl_xor(rv, o), oj = __shfl_xor(rj, o), pv = __shfl_xor(cv, o), pi = __shfl_xor(ci, o);
        if (ov > rv || (ov == rv && oj > rj)) { rv = ov; rj = oj; }
        if (pv > cv || (pv == cv && pi > ci)) { cv = pv; ci = pi; }
    }
    if (live && l == 0) p.endcell[al] = (n1 <= 0 || n2 <= 0) ? make_int2(n1, n2) : cv > rv ? make_int2(ci, n2) : make_int2(n1, rj);
}

// The walk of a lane reads one 4-bit code a step, each the end of a chain of dependent loads; the codes of the eight steps a lane q of
// the fill spent on one block are 8 * NWP consecutive words, and a path stays in such a line for several steps (i-- and j-- both lower
// t = i + q).  A lane therefore keeps the line it is in in LDS (odd pitch: no bank conflicts between lanes) and goes to HBM only when it leaves
// it -- in EPOCHS: the lanes that need a new line load it together, then every lane walks on inside its line until none can (a lane that
// fetched on its own whenever it left a line made the whole wave wait at nearly every step: some lane always does).
struct TbLine {
    uint32_t *slot;                                                    // this lane's run of CPL words in LDS (odd pitch)
    int cblk, cq;                                                      // block and fill lane of the cached line (-1: none)
    int q, c;                                                          // fill lane and cell-in-lane of column j, kept in step with j (no division per step)
    __device__ __forceinline__ void set_j(int j, int CPL) { q = j > 0 ? (j - 1) / CPL : 0; c = j > 0 ? (j - 1) % CPL : 0; }
    __device__ __forceinline__ void dec_j(int CPL) { if (--c < 0) { c = CPL - 1; q--; } }
    __device__ __forceinline__ bool has(int i) const { return ((i + q) >> TWB_LOG) == cblk && q == cq; }
    __device__ __forceinline__ void load(const uint32_t *__restrict__ Tw, int64_t arow, int i, int CPL)
    {
        cblk = (i + q) >> TWB_LOG;
        cq = q;
        const uint32_t *src = Tw + tw_run(arow, i + q, q, CPL);
        U4 v[5];                                                         // (whole dwordx4s: up to three words of the next run come along; the buffers end in a pad)
#pragma unroll
        for (int u = 0; u < 5; u++)                                      // CPL <= 17: at most five, all on their way before the first is used (left as an open
            if (4 * u < CPL) v[u] = *reinterpret_cast<const U4 *>(src + 4 * u);     // loop the compiler unrolled it sixteen times: 114 VGPRs instead of 42)
#pragma unroll
        for (int u = 0; u < 5; u++)
            if (4 * u < CPL) { slot[4 * u] = v[u].x; slot[4 * u + 1] = v[u].y; slot[4 * u + 2] = v[u].z; slot[4 * u + 3] = v[u].w; }
    }
    // cell (i, j) of the cached line as a T_* code (the caller checked has(i))
    __device__ __forceinline__ uint32_t code(int i, int CPL) const
    {
        const int F = CPL >> 3, R = CPL & 7, st = (i + q) & (TWB - 1);
        int word = st * F + (c >> 3), sh = (c & 7) * 4;
        if (c >= 8 * F) {                                                // one of the step's last R codes
            const int bit = 4 * (R * st + c - 8 * F);
            word = 8 * F + (bit >> 5);
            sh = bit & 31;
        }
        const uint32_t tc = (slot[word] >> sh) & 15u;
        return ((tc & 2u) ? (uint32_t)T_INS : (tc & 1u) ? (uint32_t)T_DEL : (uint32_t)T_DIAG) | ((tc & 4u) ? 0u : (uint32_t)T_EEXT) | ((tc & 8u) ? 0u : (uint32_t)T_FEXT);
    }
};
constexpr int TBL_PITCH = 33;                                          // words per lane (a run is CPL <= 32 words; odd pitch)

// traceback of a free-tail alignment into reference coordinates (nc_msa.hip k_nw_trace16): one lane per alignment.  Entry x of an
// alignment packs, for reference position x (0-based) and the slot BEFORE it (slot n2 = after the last position):
//     bits 0-9  read index aligned to position x, plus 1 (0 = gap)     bits 10-19  length of the insertion in slot x
//     bits 20-29 read index of the insertion's first base
// The walk visits the slots from n2 down to 0 and an entry is final when the walk leaves its slot, so every entry is written once
// (no initialisation pass, no read-modify-write); a lane collects 16 entries in LDS and writes 64-byte runs.
__global__ __launch_bounds__(64) void k_trace16p(FillArgs p, int32_t CPL, uint32_t *__restrict__ ent_all, int32_t EW)
{
    __shared__ uint32_t stage[16 * 64];
    __shared__ uint32_t tbl[64 * TBL_PITCH];
    const int al = blockIdx.x * 64 + threadIdx.x;                     // slot (the alignment itself outside list mode)
    if (al >= (p.count ? min(*p.count, p.A) : p.A)) return;
    const int lane = threadIdx.x;
    TbLine tb = {tbl + lane * TBL_PITCH, -1, -1, 0, 0};
    const int ain = p.list ? p.list[al] : al;
    const int n1 = p.n1[ain];
    const int n2 = p.site_n2[fill_site(p, ain)];
    const int64_t arow = (int64_t)al * tw_blocks(p.N1), hrow = (int64_t)al * hcol_pitch(p.N1);
    uint32_t *ent = ent_all + (int64_t)ain * EW;                      // EW: a multiple of 16 entries >= n2 + 1
    int i = n1, j = n2;
    uint32_t cur = 0;                                                  // the entry of slot j being built (position j's read index comes last)
    if (p.endcell) {
        const int2 ec = p.endcell[al];
        i = ec.x;
        j = ec.y;
        if (i < n1) cur = ((uint32_t)(n1 - i) << 10) | ((uint32_t)i << 20);
    } else if (n1 > 0 && n2 > 0) {                                    // free tail: best cell of the last row / last column
        int32_t best = p.Hlast[(int64_t)al * hlast_pitch(p.W) + n2];
        for (int jj = n2 - 1; jj >= 0; jj--) {
            const int32_t v = jj > 0 ? p.Hlast[(int64_t)al * hlast_pitch(p.W) + jj] : -p.open - (n1 - 1) * p.extend;
            if (v > best) { best = v; i = n1; j = jj; }
        }
        for (int ii = n1 - 1; ii >= 0; ii--) {
            const int32_t v = ii > 0 ? p.hcol[hrow + ii] : -p.open - (n2 - 1) * p.extend;
            if (v > best) { best = v; i = ii; j = n2; }
        }
        if (i < n1) cur = ((uint32_t)(n1 - i) << 10) | ((uint32_t)i << 20);       // the rest of the read: insertion after the window
    }
    // slots above the end point (free tail in the reference: j < n2) are empty
    int x = n2;                                                        // slot whose entry is being built
    auto put = [&](uint32_t e) {                                       // entry x is final
        stage[(x & 15) * 64 + lane] = e;
        if ((x & 15) == 0) {
            // entries x .. min(x | 15, n2) of this lane, 64 bytes
#pragma unroll
            for (int u = 0; u < 4; u++)
                reinterpret_cast<uint4 *>(ent + (x & ~15))[u] = make_uint4(stage[(4 * u) * 64 + lane], stage[(4 * u + 1) * 64 + lane],
                                                                           stage[(4 * u + 2) * 64 + lane], stage[(4 * u + 3) * 64 + lane]);
        }
        x--;
    };
    while (x > j) put(0u);                                            // (end point in the last ROW: i == n1, so cur is 0 and stays the entry of slot j)
    int state = -1;
    auto step = [&]() {
        uint32_t t;
        if (i == 0) t = T_DEL | (j > 1 ? T_EEXT : 0);
        else if (j == 0) t = T_INS | (i > 1 ? T_FEXT : 0);
        else t = tb.code(i, CPL);
        if (state < 0) {
            const int w = t & 3;
            if (w == T_DIAG) {                                        // position j-1 takes read base i-1; slot j is complete
                put(cur);
                cur = (uint32_t)i;                                    // (i - 1) + 1: the read index of position j - 1, entry j - 1
                i--; j--;
                tb.dec_j(CPL);
                return;
            }
            state = w == T_DEL ? 1 : 2;
        }
        if (state == 1) {
            const bool ext = (t & T_EEXT) != 0;
            put(cur);                                                  // reference position j-1 stays a gap
            cur = 0;
            j--;
            tb.dec_j(CPL);
            if (!ext) state = -1;
        } else {
            const bool ext = (t & T_FEXT) != 0;
            cur = (cur & 0x3ffu) | ((((cur >> 10) & 0x3ffu) + 1u) << 10) | ((uint32_t)(i - 1) << 20);     // il[j]++, iq[j] = i - 1
            i--;
            if (!ext) state = -1;
        }
    };
    tb.set_j(j, CPL);
    while (__any(i > 0 || j > 0)) {                                    // epochs
        if (i > 0 && j > 0 && !tb.has(i)) tb.load(p.Tw, arow, i, CPL);
        for (;;) {                                                     // every lane walks on inside its line
            const bool can = (i > 0 || j > 0) && (i == 0 || j == 0 || tb.has(i));
            if (!__any(can)) break;
            if (can) step();
        }
    }
    put(cur);                                                          // slot 0
}

// allele_prediction on the packed traceback of a GLOBAL alignment of the consensus (s1) against the window (nc_msa.hip k_allele_trace16).
// C = 0: the full-matrix codes of k_fill16q (all alignments, or bp.f.list's); C = 1 / 2: the banded codes of k_fill_band<C> over bp.list --
// an alignment whose path touches an edge diagonal of its band joins bp.redo_list (the caller runs those on the full matrix) and writes nothing
template <int C>
__device__ __forceinline__ void allele_trace_body(const BandArgs &bp, int32_t CPL, const int32_t *__restrict__ site_type, int32_t win_size,
                                                  int16_t *__restrict__ runs, int32_t *__restrict__ ref_len, int32_t *__restrict__ alt_len, uint32_t *tbl)
{
    const FillArgs &p = bp.f;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= (C ? *bp.count : p.count ? min(*p.count, p.A) : p.A)) return;
    const int al = C ? bp.list[idx] : p.list ? p.list[idx] : idx;
    TbLine tb = {tbl + threadIdx.x * TBL_PITCH, -1, -1, 0, 0};
    TbBand<(C ? C : 1)> tbb;
    tbb.slot = tbl + threadIdx.x * TBB_PITCH; tbb.tw = C ? bp.Twb + (int64_t)al * bp.NBLK * TWB_PITCH : nullptr; tbb.lo = C ? (int)bp.band_lo[al] : 0;
    tbb.ckey = -1; tbb.edge = bp.edge; tbb.touched = false; tbb.pkey = -1;
    const int site = fill_site(p, al);
    const uint8_t *s1 = p.s1 + (int64_t)al * p.s1_stride;
    const int n1 = p.n1[al];
    const uint8_t *s2 = p.ref_code + (p.site_pos[site] - p.ref_pos0);
    const int n2 = p.site_n2[site];
    if (n1 <= 0) {                                                   // (an empty consensus cannot happen: every column of a set has a symbol or a gap)
        ref_len[al] = -1;
        alt_len[al] = -1;
        return;
    }
    const int64_t arow = p.arow[al];
    const int run_cap = n1 + n2 + 2;
    int16_t *rop = runs + 2 * (TWB * arow + (int64_t)al * (p.W + 1)), *rcn = rop + run_cap;  // runs in REVERSE alignment order (TWB * blocks >= n1 + 1)
    int nr = 0, last_op = -1, last_cnt = 0;                            // the open run lives in registers: one store pair per run, no read-modify-write
    auto push = [&](int op) {
        if (op == last_op) last_cnt++;
        else {
            if (last_op >= 0 && nr < run_cap) { rop[nr] = (int16_t)last_op; rcn[nr] = (int16_t)last_cnt; nr++; }
            last_op = op;
            last_cnt = 1;
        }
    };
    int i = n1, j = n2, state = -1;
    int32_t path_score = 0;                                            // (banded route) the score of the path walked: the certificate below compares it with what any path outside the band can reach
    auto step = [&]() {
        uint32_t t;
        if (i == 0) t = T_DEL | (j > 1 ? T_EEXT : 0);
        else if (j == 0) t = T_INS | (i > 1 ? T_FEXT : 0);
        else t = C ? tbb.code(i, j) : tb.code(i, CPL);
        if (state < 0) {
            const int w = t & 3;
            if (w == T_DIAG) {
                const bool eq = s1[i - 1] == s2[j - 1];
                push(eq ? 7 : 8);
                path_score += eq ? p.match : p.mismatch;
                i--; j--; tb.dec_j(CPL);
                return;
            }
            state = w == T_DEL ? 1 : 2;
        }
        if (state == 1) {
            push(2);
            const bool ext = (t & T_EEXT) != 0;
            j--;
            tb.dec_j(CPL);
            path_score -= ext ? p.extend : p.open;                     // (walked backwards: the step that is not an extension is the gap's first base)
            if (!ext) state = -1;
        } else {
            push(1);
            const bool ext = (t & T_FEXT) != 0;
            i--;
            path_score -= ext ? p.extend : p.open;
            if (!ext) state = -1;
        }
    };
    tb.set_j(j, CPL);
    while (__any(i > 0 || j > 0)) {                                    // epochs: see TbLine
        if (C) { if (i > 0 && j > 0 && !tbb.has(i, j)) tbb.fetch(i, j); }
        else if (i > 0 && j > 0 && !tb.has(i)) tb.load(p.Tw, arow, i, CPL);
        for (;;) {
            const bool can = (i > 0 || j > 0) && (i == 0 || j == 0 || (C ? tbb.has(i, j) : tb.has(i)));
            if (!__any(can)) break;
            if (can) step();
        }
    }
    if (C) {
        // Is the banded optimum THE optimum?  A path that leaves the band [lo, lo + B) reaches diagonal d_out = lo - 1 or lo + B.  From diagonal 0 to d_out and
        // on to the corner's diagonal D = n2 - n1 it spends at least |d_out| gap bases on one string and |d_out - D| on the other -- two gap runs, and that
        // many bases of either string that pair with nothing -- so it scores at most
        //     match x min(n1 - gi, n2 - gj) - (open + (gj - 1) ext) - (open + (gi - 1) ext),     gj / gi = the gap bases in the window / the consensus.
        // A banded path that scores MORE is optimal over the full matrix, ties included (a co-optimal path through cells outside the band would be a
        // path that leaves the band and reaches the optimum).  A consensus is its window with a few indels applied: the bound holds for all but a few per
        // ten thousand sets; the rest, and the paths that touch an edge diagonal, go to the full matrix.  (For the star alignment of 8 % error reads
        // against the window the same bound proves nothing: that band stays part of the aligner's definition, section 11.4.)
        constexpr int Bw = 32 * (C ? C : 1);
        const int D = n2 - n1, lo = tbb.lo;
        // (0 and D are inside the band: k_allele_classes.)  Above the band: the diagonal rises by d_out window-only bases and falls d_out - D
        // consensus-only ones; below: it falls -d_out and rises D - d_out.
        auto ub = [&](int d_out) -> int32_t {
            const int rise = d_out > 0 ? d_out : D - d_out, fall = d_out > 0 ? d_out - D : -d_out;
            const int pairs = min(n1 - fall, n2 - rise);
            if (pairs < 0) return INT32_MIN;                               // no path gets there
            return p.match * pairs - (p.open + (rise - 1) * p.extend) - (p.open + (fall - 1) * p.extend);
        };
        const bool certified = path_score > ub(lo - 1) && path_score > ub(lo + Bw);
        if (tbb.touched || !certified) {
            bp.redo_list[atomicAdd(bp.redo_count, 1)] = al;
            return;
        }
    }
    if (last_op >= 0 && nr < run_cap) { rop[nr] = (int16_t)last_op; rcn[nr] = (int16_t)last_cnt; nr++; }
    bool indel = false, mm_before = false;
    int32_t rc7 = 0, rc8 = 0, rc2 = 0, ac7 = 0, ac8 = 0, ac1 = 0, mm_after = 0;
    const int32_t mr = site_type[site] == 0 ? max(10, win_size) : 10;       // max_range {0: max(10, win_size), 1: 10}
    auto clampi = [](int32_t v, int32_t n) { return v < 0 ? (v + n < 0 ? 0 : v + n) : (v > n ? n : v); };       // Python slice s[:v]
    int op = 0, cnt = 0;
    bool done = false;
    int32_t out_r = 0, out_a = 0;
    for (int k = nr - 1; k >= 0 && !done; k--) {
        op = rop[k];
        cnt = rcn[k];
        if (op == 8 || op == 7) {
            if (op == 7) { rc7 += cnt; ac7 += cnt; } else { rc8 += cnt; ac8 += cnt; }
            if (indel) mm_after += cnt;
            else mm_before = true;
        }
        if (op == 1) { ac1 += cnt; mm_after = 0; indel = true; }
        if (op == 2) { rc2 += cnt; mm_after = 0; indel = true; }
        const int32_t rsum = rc7 + rc8 + rc2;
        if (!indel && rsum >= mr + 10) {
            if (rc8) {
                const int32_t ol = op == 8 ? rsum : rsum - cnt;
                out_r = clampi(ol, n2);
                out_a = clampi(ol, n1);
            } else {
                out_r = -1;
                out_a = -1;
            }
            done = true;
            break;
        }
        if (indel && mm_after > 20) break;
    }
    if (!done) {
        const int32_t rsum = rc7 + rc8 + rc2, asum = ac7 + ac8 + ac1;
        int32_t ro = op == 8 ? rsum : rsum - cnt, ao = op == 8 ? asum : asum - cnt;
        if (!mm_before) { ro += 1; ao += 1; }
        out_r = clampi(ro, n2);
        out_a = clampi(ao, n1);
    }
    ref_len[al] = out_r;
    alt_len[al] = out_a;
}
template <int C>
__global__ __launch_bounds__(64) void k_allele_trace16p(BandArgs bp, int32_t CPL, const int32_t *__restrict__ site_type, int32_t win_size,
                                                        int16_t *__restrict__ runs, int32_t *__restrict__ ref_len, int32_t *__restrict__ alt_len)
{
    __shared__ uint32_t tbl[64 * TBL_PITCH];
    allele_trace_body<C>(bp, CPL, site_type, win_size, runs, ref_len, alt_len, tbl);
}
__global__ __launch_bounds__(64) void k_allele_trace_b12(BandArgs b1, BandArgs b2, int32_t CPL, const int32_t *__restrict__ site_type, int32_t win_size,
                                                         int16_t *__restrict__ runs, int32_t *__restrict__ ref_len, int32_t *__restrict__ alt_len)
{
    __shared__ uint32_t tbl[64 * TBL_PITCH];
    if (blockIdx.y == 0) allele_trace_body<1>(b1, CPL, site_type, win_size, runs, ref_len, alt_len, tbl);
    else allele_trace_body<2>(b2, CPL, site_type, win_size, runs, ref_len, alt_len, tbl);
}

}   // namespace

__global__ void k_band_stats(const int32_t *__restrict__ counts, long long *__restrict__ acc)
{
    acc[0] += counts[0]; acc[1] += counts[1]; acc[2] += counts[3]; acc[3] += counts[2] - counts[3];
}

void nc_pipe_launch_trace_band(hipStream_t st, const BandArgs &b1, const BandArgs &b2, uint32_t *ent, int32_t EW)
{
    hipLaunchKernelGGL(k_trace_band12, dim3((b1.f.A + 63) / 64, 2), dim3(64), 0, st, b1, b2, ent, EW);
}
void nc_pipe_launch_trace(hipStream_t st, const FillArgs &fa, int CPL, uint32_t *ent, int32_t EW)
{
    hipLaunchKernelGGL(k_end_cells, dim3((fa.A + 15) / 16), dim3(256), 0, st, fa);
    hipLaunchKernelGGL(k_trace16p, dim3((fa.A + 63) / 64), dim3(64), 0, st, fa, CPL, ent, EW);
}
void nc_pipe_launch_band_stats(hipStream_t st, const int32_t *counts, long long *acc) { hipLaunchKernelGGL(k_band_stats, dim3(1), dim3(1), 0, st, counts, acc); }
void nc_pipe_launch_allele_trace_band(hipStream_t st, const BandArgs &b1, const BandArgs &b2, int CPL, const int32_t *site_type, int32_t win_size, int16_t *runs, int32_t *ref_len, int32_t *alt_len)
{
    hipLaunchKernelGGL(k_allele_trace_b12, dim3((b1.f.A + 63) / 64, 2), dim3(64), 0, st, b1, b2, CPL, site_type, win_size, runs, ref_len, alt_len);
}
void nc_pipe_launch_allele_trace(hipStream_t st, const BandArgs &bb, int CPL, const int32_t *site_type, int32_t win_size, int16_t *runs, int32_t *ref_len, int32_t *alt_len)
{
    hipLaunchKernelGGL(k_allele_trace16p<0>, dim3((bb.f.A + 63) / 64), dim3(64), 0, st, bb, CPL, site_type, win_size, runs, ref_len, alt_len);
}

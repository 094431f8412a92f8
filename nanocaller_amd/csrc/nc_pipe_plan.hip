// Device indel pipeline, the plan (nc_indel_sites_plan): from K7's column types (nc_indel.hip and its units; col_type stays in HBM) to the sites and their read sets.
//   k_impute_flags  dct['impute_indel_phase']: every col_type-2 column -> 3 (an anchor by the read grouping) or -1
//   k_pick          one wave per chunk: the order-dependent anchor selection `if v_pos <= prev: continue` (:249,266-275) with the
//                   dict semantics of `variants[anchor] = type`, then the pass-2 range test (:306)
//   k_flatten       the chunks' anchor segments, back to back
//   k_sets          one wave per anchor: reference window test (:325-327), the pileup at the anchor from the read pack's tile
//                   index, the hap0 / hap1 / all read sets with the first-maxcov policy and the mincov tests (:333-348)
// and the exclusive scans of the plan and of the run stages (k_scan_part + k_scan_apply).
#include <algorithm>

#include "nc_pipe.h"
#include "nc_sample.h"

namespace {
// dct['impute_indel_phase'] on the device pipeline (generate_indel_pileups.py:278-304; round 6).  K7 marks the columns that meet the rule's column-level
// predicate (:278-284) with col_type 2; the rule then groups the column's reads by their pileup STRING (base letter + '+n<inserted bases>' /
// '-nN..', upper-cased: :279,287-289), takes the largest group against the runner-up (or against everybody else; or, when one string holds more
// than 80 % of the reads, its first half against its second: :291-297) and makes the column an anchor 10 bp upstream when both sides hold mincov
// reads (:298-303); pass 2 uses those two read-name sets instead of the haplotype tags (:310-312).  Here: k_impute_flags runs the grouping for
// every col_type-2 column and rewrites it to 3 (anchor) or -1; k_pick treats 3 as the small-window rule and notes the source column in the
// anchor's type byte (bit 1 = imputed, bits 2-5 = column - anchor: 10 unless the anchor was clipped to 1); k_sets<.., true> repeats the grouping
// at the source column of an imputed anchor and reads the members' sides where it read the HP tags.  A read's string is keyed by a 64-bit hash
// of (letter, event length, inserted bases); columns deeper than IMP_CAP reads raise the capacity bit (host-assembled route).
struct ImpLds {                        // one wave's scratch
    uint64_t key[IMP_CAP];
    int64_t slot[IMP_CAP];             // the read's slot offset: what identifies it in any tile's entries
    uint16_t first[IMP_CAP], cnt[IMP_CAP];
    uint8_t side[IMP_CAP];             // 0: in neither set, 1: read_names_0, 2: read_names_1
};
// One wave.  -> n = reads in the column's pileup (file order; -1: more than IMP_CAP), L.slot / L.side filled; pass = both sets hold mincov reads
__device__ __forceinline__ int impute_group(const ImpArgs &p, int32_t v, ImpLds &L, bool &pass)
{
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (1ull << lane) - 1;
    pass = false;
    const int t = (v - p.tile_pos0) / p.tile_size;
    if (v < p.tile_pos0 || t >= p.n_tiles) return 0;
    const int e0 = p.tile_off[t], e1 = p.tile_off[t + 1];
    int n = 0;
    for (int eb = e0; eb < e1; eb += 64) {
        const int e = eb + lane;
        nc_tile_entry ent;
        ent.start = 0; ent.end = 0; ent.base_flag = 0;
        if (e < e1) ent = p.tile_ent[e];
        const bool cov = e < e1 && ent.start <= v && v < ent.end;
        const uint64_t m = __ballot(cov);
        const int idx = n + __popcll(m & lt);
        if (cov && idx < IMP_CAP) {
            const int64_t so = (ent.base_flag & ~int64_t(15)) + (ent.start & ~15);
            int r;
            if (p.ent_read) r = p.ent_read[e];
            else {
                int lo = 0, hi = p.n_reads;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.slot_off[mid] < so) lo = mid + 1; else hi = mid; }
                r = lo;
            }
            const int f0 = p.ev_off[r], f1 = p.ev_off[r + 1];
            int lo = f0, hi = f1;                                            // first event on a column >= v
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.ev_pos[mid] < v) lo = mid + 1; else hi = mid; }
            const int k = lo;
            bool deleted = false;
            if (k > f0) { const int32_t el = p.ev_len[k - 1]; deleted = el < 0 && p.ev_pos[k - 1] - el >= v; }
            const int code = p.codes[(ent.base_flag & ~int64_t(15)) + v];
            const uint32_t letter = deleted ? 5u : (code < 4 ? (uint32_t)code : 4u);       // A G T C, N (any other base), '*'
            int32_t len = 0;
            if (k < f1 && p.ev_pos[k] == v) len = p.ev_len[k];
            uint64_t h = 1469598103934665603ull;                                             // FNV-1a over letter, length, inserted bases
            h = (h ^ letter) * 1099511628211ull;
            h = (h ^ (uint64_t)(uint32_t)len) * 1099511628211ull;
            if (len > 0)
                for (int i = p.ins_off[k]; i < p.ins_off[k + 1]; i++) h = (h ^ p.ins_bases[i]) * 1099511628211ull;
            L.key[idx] = h;
            L.slot[idx] = so;
        }
        n += __popcll(m);
    }
    if (n > IMP_CAP) return -1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // groups: first member and size of every read's string
    for (int i = lane; i < n; i += 64) {
        const uint64_t ki = L.key[i];
        int first = -1, c = 0;
        for (int j = 0; j < n; j++)
            if (L.key[j] == ki) { if (first < 0) first = j; c++; }
        L.first[i] = (uint16_t)first;
        L.cnt[i] = (uint16_t)c;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // sorted(groups, key = size, reverse = True) is stable: the largest, ties to the string seen first; then the runner-up
    auto top = [&](int skip) -> uint32_t {
        uint32_t best = 0;
        for (int i = lane; i < n; i += 64)
            if (L.first[i] == i && i != skip) best = max(best, ((uint32_t)L.cnt[i] << 16) | (uint32_t)(0xffff - i));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o));
        return best;
    };
    if (n == 0) return 0;
    const uint32_t b0 = top(-1);
    const int g0 = 0xffff - (int)(b0 & 0xffffu), c0 = (int)(b0 >> 16);
    int n0 = 0, n1 = 0;
    if ((double)c0 <= 0.8 * (double)n) {                                                     // :291
        const uint32_t b1 = top(g0);
        const int g1 = 0xffff - (int)(b1 & 0xffffu), c1 = (int)(b1 >> 16);
        const bool second = c1 >= p.mincov;                                                  // :293: the runner-up, else everybody else
        for (int i = lane; i < n; i += 64) L.side[i] = L.first[i] == g0 ? 1 : ((second ? L.first[i] == g1 : true) ? 2 : 0);
        n0 = c0;
        n1 = second ? c1 : n - c0;
    } else {                                                                                 // :295-296: the string's first half against its second
        const int half = c0 / 2;
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool in = i < n && L.first[i] == g0;
            const uint64_t m = __ballot(in);
            const int rank = base + __popcll(m & lt);
            if (i < n) L.side[i] = in ? (rank < half ? 1 : 2) : 0;
            base += __popcll(m);
        }
        n0 = half;
        n1 = c0 - half;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    pass = n0 >= p.mincov && n1 >= p.mincov;                                                 // :298
    return n;
}

// every col_type-2 column of the chunks -> 3 (the grouping yields two sets of mincov reads: an anchor, :298-303) or -1.  One block per chunk and
// slab of 4096 columns, a wave per 1024 of them.
__global__ __launch_bounds__(256) void k_impute_flags(const PipeChunk *__restrict__ pc, int8_t *__restrict__ ctype, ImpArgs p, int32_t *__restrict__ err)
{
    __shared__ ImpLds lds[4];
    const PipeChunk c = pc[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int8_t *ct = ctype + c.coloff;
    const int col_lo = (int)blockIdx.y * 4096 + wv * 1024;
    for (int b = col_lo; b < min(col_lo + 1024, c.ncol); b += 64) {
        const int col = b + lane;
        uint64_t m = __ballot(col < c.ncol && ct[col] == 2);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            bool pass;
            const int n = impute_group(p, c.lo + b + l, lds[wv], pass);
            if (n < 0 && lane == 0) atomicOr(err, 16);
            if (lane == 0) ct[b + l] = pass ? 3 : -1;
        }
    }
}

// LISTED (a list of columns is set, nc_indel_set_sites): col_type also holds 4 / 5, a listed column forced as a long- / small-window candidate
// (k_listed); such a column acts as a 0 / 1 and the anchor it writes or overwrites remembers it (seg_src; a later natural column that overwrites
// the anchor's type leaves it, as extra_variants stays).  Without a list the kernel is the one it was: the plain form has no seg_src argument.
// The source costs no LDS (a second array took k_pick from three workgroups a CU to two: two rounds for a chr20-sized contig's 645 chunks): it is
// anchor + win or anchor + 10 by the forced column's class, so the anchor's word carries two more bits (6: a forced column wrote it, 7: of the long
// class; stripped from seg_type) -- except where the anchor was clipped to 1, and a chunk has one such anchor: its source is a register (src1).
template <bool LISTED>
__device__ __forceinline__ void pick_body(const PipeChunk *__restrict__ pc, const int8_t *__restrict__ ctype, int32_t win,
                                          int32_t *__restrict__ seg_pos, int8_t *__restrict__ seg_type, int32_t *__restrict__ seg_src,
                                          int32_t *__restrict__ cnt, int32_t *__restrict__ err)
{
    __shared__ uint32_t anc[PICK_CAP];                               // (anchor - aoff) << 8 | type: 4 bytes an anchor (5 in two arrays held two waves per CU)
    int32_t src1 = 0;                                                // (LISTED) the forced column that last wrote anchor 1
    const PipeChunk c = pc[blockIdx.x];
    const int32_t aoff = c.lo - win - 16;                            // an anchor is >= max(1, column - win)
    auto apos = [&](int i) { return (int32_t)(anc[i] >> 8) + aoff; };
    auto apack = [&](int32_t an, int tb) { return ((uint32_t)(an - aoff) << 8) | (uint32_t)(tb & 0xff); };
    const int lane = threadIdx.x;
    const int8_t *ct = ctype + c.coloff;
    int n = 0;
    int base = 0;
    bool over = false;
    // 4096 columns a round: four steps of 1024 columns (16 per lane, one 16-byte load each), loaded together -- the walk is a chain of dependent
    // loads (a step of 64 columns was 0.95 ms per chr20-sized contig for ~1 % flagged columns, a step of 1024 columns 0.21 ms);
    // m16 = this lane's flagged columns of the step still to be visited
    while (base < c.ncol) {
        uint32_t W[4][4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int col0 = base + 1024 * b + 16 * lane;
            W[b][0] = W[b][1] = W[b][2] = W[b][3] = 0xffffffffu;
            if (col0 + 16 <= c.ncol) __builtin_memcpy(W[b], ct + col0, 16);
            else
                for (int k = 0; k < 16 && col0 + k < c.ncol; k++) reinterpret_cast<int8_t *>(W[b])[k] = ct[col0 + k];
        }
        int64_t skip_to = 0;                                          // columns before it are skipped (carried from step to step)
        int next_base = base + 4096;
        bool jump = false;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int bb = base + 1024 * b, col0 = bb + 16 * lane;
            if (jump || bb >= c.ncol) continue;
            const uint32_t (&w)[4] = W[b];
            uint32_t m16 = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t t = (w[k >> 2] >> ((k & 3) * 8)) & 0xffu;
                m16 |= ((t <= 1u || t == 3u || (LISTED && (t == 4u || t == 5u))) ? 1u : 0u) << k;      // (3: an imputed column, k_impute_flags; 4, 5: k_listed)
            }
            {
                const int64_t sh = skip_to - col0;                    // (a skip that reaches into this step)
                if (sh >= 16) m16 = 0;
                else if (sh > 0) m16 &= ~((1u << (int)sh) - 1u);
            }
            for (;;) {
                const uint64_t lm = __ballot(m16 != 0);
                if (!lm) break;
                const int l = __ffsll((long long)lm) - 1;
                const uint32_t mm = (uint32_t)__shfl((int)m16, l);
                const int bq = __ffs((int)mm) - 1;
                const int32_t v = c.lo + bb + 16 * l + bq;
                const int tc0 = (int)((__shfl((int)w[0], l) * (bq < 4) + __shfl((int)w[1], l) * (bq >= 4 && bq < 8) + __shfl((int)w[2], l) * (bq >= 8 && bq < 12) +
                                       __shfl((int)w[3], l) * (bq >= 12)) >> ((bq & 3) * 8)) & 0xff;
                const bool forced = LISTED && tc0 >= 4;
                const int tc = forced ? tc0 - 4 : tc0;
                const int32_t prev = tc == 0 ? v + win : v + 10;                     // :267, :273, :301
                const int32_t an = tc == 0 ? max(1, v - win) : max(1, v - 10);       // :268, :274, :302
                const int tb = tc == 3 ? (1 | 2 | ((v - an) << 2)) : tc;             // imputed: the small-window type + where its read sets come from
                // variants[an] = tb: the anchors stay sorted; an equal key is overwritten (dict), a smaller one (a small-window
                // anchor followed by a long-window one less than 30 columns later) goes a few places back
                int i = n;
                while (i > 0 && apos(i - 1) > an) i--;
                if (i > 0 && apos(i - 1) == an) {
                    // variants[an] is overwritten; extra_variants[an] (an imputed column's read sets) stays unless an imputed column writes it again
                    if (lane == 0) {
                        const int oldw = (int)(anc[i - 1] & 0xffu), old = LISTED ? (oldw & 0x3f) : oldw;
                        const int nt = ((tb & 2) || !(old & 2)) ? tb : ((old & ~1) | tb);
                        anc[i - 1] = apack(an, LISTED ? (nt | (forced ? (0x40 | (tc0 == 4 ? 0x80 : 0)) : (oldw & 0xc0))) : nt);
                    }
                } else if (n >= PICK_CAP) {
                    over = true;
                } else {
                    if (lane == 0) {
                        for (int k = n; k > i; k--) anc[k] = anc[k - 1];
                        anc[i] = apack(an, forced ? (tb | 0x40 | (tc0 == 4 ? 0x80 : 0)) : tb);
                    }
                    n++;
                }
                if (forced && an == 1) src1 = v;
                __syncthreads();
                // every column up to `prev` is skipped by `if v_pos <= prev: continue` (:249)
                skip_to = (int64_t)prev - c.lo + 1;
                if (skip_to >= base + 4096) {
                    next_base = (int)min((int64_t)c.ncol, skip_to);
                    jump = true;
                    break;
                }
                if (skip_to >= bb + 1024) break;                     // the rest of this step is skipped; the next one takes the mask
                const int sh = (int)(skip_to - col0);                              // this lane's columns before skip_to are done
                if (sh >= 16) m16 = 0;
                else if (sh > 0) m16 &= ~((1u << sh) - 1u);
            }
        }
        base = next_base;
    }
    if (over && lane == 0) atomicOr(err, 1);
    // pass-2 range (:306) and the copy to the chunk's segment, in order
    int m = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool ok = k < n && apos(k) > c.a_lo && apos(k) <= c.hi;
        const uint64_t bm = __ballot(ok);
        if (ok) {
            const int w = m + __popcll(bm & ((1ull << lane) - 1));
            seg_pos[c.seg0 + w] = apos(k);
            const uint32_t tw = anc[k] & 0xffu;
            seg_type[c.seg0 + w] = (int8_t)(LISTED ? (tw & 0x3fu) : tw);
            if (LISTED) seg_src[c.seg0 + w] = !(tw & 0x40u) ? 0 : apos(k) == 1 ? src1 : apos(k) + ((tw & 0x80u) ? win : 10);
        }
        m += __popcll(bm);
    }
    if (lane == 0) cnt[c.id] = m;
}

__global__ __launch_bounds__(64) void k_pick(const PipeChunk *__restrict__ pc, const int8_t *__restrict__ ctype, int32_t win,
                                             int32_t *__restrict__ seg_pos, int8_t *__restrict__ seg_type, int32_t *__restrict__ cnt,
                                             int32_t *__restrict__ err)
{
    pick_body<false>(pc, ctype, win, seg_pos, seg_type, nullptr, cnt, err);
}
__global__ __launch_bounds__(64) void k_pick_listed(const PipeChunk *__restrict__ pc, const int8_t *__restrict__ ctype, int32_t win,
                                                    int32_t *__restrict__ seg_pos, int8_t *__restrict__ seg_type, int32_t *__restrict__ seg_src,
                                                    int32_t *__restrict__ cnt, int32_t *__restrict__ err)
{
    pick_body<true>(pc, ctype, win, seg_pos, seg_type, seg_src, cnt, err);
}

__device__ __forceinline__ int block_scan(int v, int *wsum, int &tot)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
    inc = (decltype(inc))nc_wave_incl_scan((int32_t)inc);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int wp = 0;
    tot = 0;
    for (int w = 0; w < nw; w++) {
        const int s = wsum[w];
        if (w < wv) wp += s;
        tot += s;
    }
    return wp + inc;
}

// ---- exclusive scans in two launches of many workgroups.  (One workgroup walking the whole array, every thread a contiguous chunk, is a chain of
// uncoalesced loads on one CU: 0.21 ms for the 120 k consensus lengths of a chr20-sized pass, 0.19 for its ALT lengths, 3 x 0.04 in the plan.)
// k_scan_part: sum of every tile of 4096 inputs; k_scan_apply: a tile's offset = the sum of the tiles before it (a block reduction over <= a few
// hundred partial sums), then the scan of its own 4096 inputs, four consecutive ones per thread.
enum { SC_PLAIN = 0, SC_TWB = 1, SC_POS = 2 };
template <int F>
__device__ __forceinline__ int sc_val(int x) { return F == SC_TWB ? tw_blocks(x) : F == SC_POS ? max(x, 0) : x; }
constexpr int SC_TILE = 4096;

template <int F>
__global__ __launch_bounds__(1024) void k_scan_part(const int32_t *__restrict__ in, int32_t n, int32_t add, long long *__restrict__ part,
                                                    const long long *__restrict__ base_in)
{
    __shared__ long long wsum[16];
    const int i0 = blockIdx.x * SC_TILE + threadIdx.x * 4;
    long long local = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) if (i0 + u < n) local += sc_val<F>(in[i0 + u]) + add;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < 16; w++) t += wsum[w];
        part[blockIdx.x] = t;
        if (blockIdx.x == 0) part[gridDim.x] = base_in ? base_in[0] : 0;       // snapshot of the running base (k_scan_apply's last block advances it)
    }
}

// out[i] = base + exclusive prefix; OUT = int32_t or int64_t.  total_out (nullable): the grand total as {low 31 bits, 0} (the row mailbox's format) when
// mbox_fmt, else a plain OUT at out[n].  base_io (nullable): advanced by the total.
template <int F, class OUT>
__global__ __launch_bounds__(1024) void k_scan_apply(const int32_t *__restrict__ in, int32_t n, int32_t add, const long long *__restrict__ part,
                                                     OUT *__restrict__ out, int32_t write_total, int32_t *__restrict__ total_mbox, long long *__restrict__ base_io)
{
    __shared__ long long wsum2[16];
    __shared__ int wsum[16];
    __shared__ long long s_off;
    const int nb = gridDim.x;
    long long before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 1024) before += part[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if ((threadIdx.x & 63) == 0) wsum2[threadIdx.x >> 6] = before;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = part[nb];
        for (int w = 0; w < 16; w++) t += wsum2[w];
        s_off = t;
    }
    __syncthreads();
    const int i0 = blockIdx.x * SC_TILE + threadIdx.x * 4;
    int v[4], local = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) { v[u] = i0 + u < n ? sc_val<F>(in[i0 + u]) + add : 0; local += v[u]; }
    int tot;
    const int inc = block_scan(local, wsum, tot);
    long long run = s_off + inc - local;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (i0 + u < n) out[i0 + u] = (OUT)run;
        run += v[u];
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) {
        const long long total = s_off + tot;
        if (write_total) out[n] = (OUT)total;
        if (total_mbox) { total_mbox[0] = (int32_t)((total - part[nb]) & 0x7fffffff); total_mbox[1] = (int32_t)((total - part[nb]) >> 31); }
        if (base_io) base_io[0] = total;
    }
}

template <int F, class OUT>
int scan_launch(nc_ctx *ctx, hipStream_t st, DevBuf &partbuf, const int32_t *in, int32_t n, int32_t add, OUT *out, bool write_total, int32_t *total_mbox,
                       long long *base_io)
{
    const int nb = std::max(1, (n + SC_TILE - 1) / SC_TILE);
    // the partial-sum buffers are sized ONCE per pass (nc_indel_sites_plan: SC_PARTS entries): launches queued on another stream may still read
    // them, so a scan never re-allocates -- an array too long for them is refused
    if (((size_t)nb + 2) * 8 > partbuf.cap)
        return nc_fail(ctx, NC_ERR_CAPACITY, "scan of %d elements needs %d partial sums, the pass holds %zu", n, nb + 2, partbuf.cap / 8);
    long long *part = (long long *)partbuf.p;
    hipLaunchKernelGGL((k_scan_part<F>), dim3(nb), dim3(1024), 0, st, in, n, add, part, (const long long *)base_io);
    hipLaunchKernelGGL((k_scan_apply<F, OUT>), dim3(nb), dim3(1024), 0, st, in, n, add, (const long long *)part, out, write_total ? 1 : 0, total_mbox, base_io);
    return NC_OK;
}

__global__ __launch_bounds__(256) void k_flatten(const PipeChunk *__restrict__ pc, const int32_t *__restrict__ seg_pos, const int8_t *__restrict__ seg_type,
                                                 const int32_t *__restrict__ cnt, const int32_t *__restrict__ off, int32_t *__restrict__ anc_pos,
                                                 int8_t *__restrict__ anc_type, int32_t *__restrict__ anc_chunk)
{
    const PipeChunk c = pc[blockIdx.x];
    const int n = cnt[c.id], o = off[c.id];
    for (int k = threadIdx.x; k < n; k += 256) {
        anc_pos[o + k] = seg_pos[c.seg0 + k];
        anc_type[o + k] = seg_type[c.seg0 + k];
        anc_chunk[o + k] = c.id;
    }
}

// MATES: the pack holds alignments that share read names (entries with bit 3 of base_flag; SetArgs::mt).  Pass 2's dicts are keyed by name
// (:322-338): where several alignments of a name cover the anchor, the name is one entry at the rank of the first of them (a dict keeps the order of
// first insertion) with the window of the last (`d_tot[qname] = dt` overwrites); its haplotype is the name's (hap0 when records of the name carry
// HP 1 and HP 2: `if ... elif`), and the site's phase is phase_dict[name].  Every other entry takes the code of the plain form.
// SAMPLED (nc_set_downsample, mode 1; never with IMP or MATES: the plan refuses those): a set deeper than maxcov holds the seeded uniform sample of
// nc_sample.h instead of its first maxcov entries.  Membership needs the sets' sizes, so where the tile holds more than maxcov entries at all a counting
// pass comes first, in the count launch and in the fill launch alike (the two must agree entry by entry).
template <bool FILL, bool IMP, bool MATES, bool SAMPLED>
__global__ __launch_bounds__(256) void k_sets(SetArgs p)
{
    __shared__ ImpLds imp_lds[IMP ? 4 : 1];
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= p.n_anchor) return;
    if (FILL && !p.kept[a]) return;
    const int32_t v = p.anc_pos[a];
    // reference window [v, min(chrom_len, v + window_after + 1)): upper-case AGTC only (:325-327)
    const int64_t b = min(p.chrom_len, (int64_t)v + p.window_after + 1);
    bool ok = b > v && v >= 1;
    if (!FILL) {
        bool mine = true;
        for (int64_t x = v + lane; x < b; x += 64) {
            const int64_t i = x - p.ref_pos0;
            mine = mine && i >= 0 && i < p.ref_len && p.ref_code[i] < 4;
        }
        ok = ok && __all(mine);
    }
    int n_all = 0, n_1 = 0, n_2 = 0, n_u = 0, first0 = -1;
    int32_t first_ps = 0;                                            // (MATES) phase_dict of set 0's first name
    // an imputed anchor (impute_indel_phase): the two read sets of its source column stand where the HP tags stand otherwise (:310-312)
    int n_imp = -1;
    if constexpr (IMP) {
        const int tb = (int)(uint8_t)p.anc_type[a];
        if (tb & 2) {
            bool pass_unused;
            n_imp = impute_group(p.imp, v + (tb >> 2), imp_lds[threadIdx.x >> 6], pass_unused);
            if (n_imp < 0) { if (lane == 0) atomicOr(p.err, 16); n_imp = 0; }
        }
    }
    const int t = (v - p.tile_pos0) / p.tile_size;
    const int site = FILL ? p.site_of[a] : 0;
    const int al0 = FILL ? p.al_of[a] : 0;
    if (ok && v >= p.tile_pos0 && t < p.n_tiles) {
        const int e0 = p.tile_off[t], e1 = p.tile_off[t + 1];
        const uint64_t lt = (1ull << lane) - 1;
        uint32_t sb_all = 0, sb_1 = 0, sb_2 = 0, st_all = 0, st_1 = 0, st_2 = 0;
        bool deep_all = false, deep_1 = false, deep_2 = false;                   // (SAMPLED) the set is deeper than maxcov: an entry is a member when its key <= st_*
        if constexpr (SAMPLED) {
            if (e1 - e0 > p.maxcov) {
                int c_all = 0, c_1 = 0, c_2 = 0;
                for (int eb = e0; eb < e1; eb += 64) {
                    nc_tile_entry ent;
                    ent.start = 0; ent.end = 0; ent.base_flag = 0;
                    if (eb + lane < e1) ent = p.tile_ent[eb + lane];
                    const bool cov = eb + lane < e1 && ent.start <= v && v < ent.end;
                    const int hp = (int)((ent.base_flag >> 1) & 3);
                    c_all += __popcll(__ballot(cov));
                    c_1 += __popcll(__ballot(cov && hp == 1));
                    c_2 += __popcll(__ballot(cov && hp == 2));
                }
                if (c_all > p.maxcov) { deep_all = true; sb_all = nc_sample_base(v, p.seed, 0); st_all = nc_sample_threshold(sb_all, c_all, p.maxcov); }
                if (!p.haploid && c_1 > p.maxcov) { deep_1 = true; sb_1 = nc_sample_base(v, p.seed, 1); st_1 = nc_sample_threshold(sb_1, c_1, p.maxcov); }
                if (!p.haploid && c_2 > p.maxcov) { deep_2 = true; sb_2 = nc_sample_base(v, p.seed, 2); st_2 = nc_sample_threshold(sb_2, c_2, p.maxcov); }
            }
        }
        for (int eb = e0; eb < e1; eb += 64) {
            const int e = eb + lane;
            nc_tile_entry ent;
            ent.start = 0; ent.end = 0; ent.base_flag = 0;
            if (e < e1) ent = p.tile_ent[e];
            bool cov = e < e1 && ent.start <= v && v < ent.end;                  // the pileup at the anchor, in pack (= file) order
            int hp = (int)((ent.base_flag >> 1) & 3);
            int r_name = -1;                                                     // (MATES) the read whose window stands for the name
            int32_t ps_name = 0;
            if constexpr (MATES) {
                if (cov && (ent.base_flag & 8)) {
                    const int self = imate_find(p.mt, (ent.base_flag & ~int64_t(15)) + (ent.start & ~15));
                    if (self >= 0) {
                        const IndelMate me = imate_get(p.mt, self);
                        int first = self, last = self, j = me.next;
                        r_name = me.read;
                        for (int guard = 0; guard < 64 && j != self && j >= 0 && j < p.mt.n; guard++) {     // (a damaged ring must not hang the wave)
                            const IndelMate o = imate_get(p.mt, j);
                            if (o.start <= v && v < o.end) {
                                first = min(first, j);
                                if (j > last) { last = j; r_name = o.read; }
                            }
                            j = o.next;
                        }
                        if (first != self) cov = false;
                        hp = (me.hap & 1) ? 1 : (me.hap & 2) ? 2 : 0;
                        ps_name = me.ps;
                    }
                }
            }
            if constexpr (IMP) {
                if (n_imp >= 0) {
                    hp = 0;
                    if (cov) {
                        const ImpLds &L = imp_lds[threadIdx.x >> 6];
                        const int64_t so = (ent.base_flag & ~int64_t(15)) + (ent.start & ~15);
                        for (int j = 0; j < n_imp; j++)
                            if (L.slot[j] == so) { hp = L.side[j]; break; }
                    }
                }
            }
            const uint64_t m_all = __ballot(cov), m_1 = __ballot(cov && hp == 1), m_2 = __ballot(cov && hp == 2);
            const int my_all = n_all + __popcll(m_all & lt), my_1 = n_1 + __popcll(m_1 & lt), my_2 = n_2 + __popcll(m_2 & lt);
            int member = 0;
            if constexpr (SAMPLED) {
                if (cov) {
                    const bool in_all = deep_all ? mix32(my_all, sb_all) <= st_all : true;
                    if (p.haploid) member = in_all ? 1 : 0;
                    else member = ((hp == 1 && (deep_1 ? mix32(my_1, sb_1) <= st_1 : true)) ? 1 : 0) | ((hp == 2 && (deep_2 ? mix32(my_2, sb_2) <= st_2 : true)) ? 2 : 0) |
                                  (in_all ? 4 : 0);
                }
            } else
            if (cov) {
                if (p.haploid) member = my_all < p.maxcov ? 1 : 0;
                else member = ((hp == 1 && my_1 < p.maxcov) ? 1 : 0) | ((hp == 2 && my_2 < p.maxcov) ? 2 : 0) | (my_all < p.maxcov ? 4 : 0);
            }
            const uint64_t m_u = __ballot(member != 0);
            if (FILL) {
                // the entry's read: its slot offset is unique
                int r = -1;
                if (member != 0 || (cov && hp == 1 && first0 < 0)) {
                    if (p.ent_read) r = p.ent_read[e];
                    else {
                        const int64_t so = (ent.base_flag & ~int64_t(15)) + (ent.start & ~15);
                        int lo = 0, hi = p.n_reads;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (p.slot_off[mid] < so) lo = mid + 1; else hi = mid;
                        }
                        r = lo;
                    }
                }
                int32_t my_ps = 0;
                if constexpr (MATES) {
                    if (!p.haploid && cov && hp == 1 && first0 < 0) my_ps = r_name >= 0 ? ps_name : p.read_ps[r];
                    if (r_name >= 0) r = r_name;
                }
                if (member != 0) {
                    const int w = al0 + n_u + __popcll(m_u & lt);
                    p.al_read[w] = r;
                    p.al_site[w] = site;
                    p.al_member[w] = (uint8_t)member;
                    if (p.al_ev) {
                        // the read's events around the anchor: [first event at or after the anchor's 1024-column block less 64 columns, first one at or
                        // after the block after next less 64) -- the first event on a column >= v lies in that stretch or is its end
                        const int h = (v - (p.tile_pos0 + t * p.tile_size)) >> 10;
                        const int32_t *cur = p.ent_cur + (int64_t)e * NC_ENT_CUR_PITCH(p.spt);
                        p.al_ev[w] = make_int2(cur[h], h + 2 <= p.spt ? cur[h + 2] : p.ev_off[r + 1]);
                        if constexpr (MATES) { if (r_name >= 0) p.al_ev[w] = make_int2(p.ev_off[r], p.ev_off[r + 1]); }      // (the cursors are the entry's own read's)
                    }
                }
                if (first0 < 0) {
                    const uint64_t mf = p.haploid ? m_all : m_1;
                    if (mf) first0 = __shfl(r, __ffsll((long long)mf) - 1);
                    if constexpr (MATES) { if (mf) first_ps = __shfl(my_ps, __ffsll((long long)mf) - 1); }
                }
            }
            n_all += __popcll(m_all);
            n_1 += __popcll(m_1);
            n_2 += __popcll(m_2);
            n_u += __popcll(m_u);
        }
    }
    const int s_all = min(n_all, p.maxcov), s_1 = min(n_1, p.maxcov), s_2 = min(n_2, p.maxcov);
    const bool pass = ok && (p.haploid ? s_all >= p.mincov : (s_1 >= 2 && s_2 >= 2 && s_all >= p.mincov));     // :48, :345
    if (!FILL) {
        if (lane == 0) {
            p.kept[a] = pass ? 1 : 0;
            p.nuniq[a] = pass ? n_u : 0;
        }
    } else if (lane == 0) {
        p.site_pos[site] = v;
        p.site_chunk[site] = p.anc_chunk[a];
        p.site_type[site] = p.anc_type[a] & 1;                                          // (the window rule; bits 1-5: an imputed anchor's source)
        if constexpr (MATES) p.site_phase[site] = (!p.haploid && first0 >= 0) ? first_ps : 0;
        else
        p.site_phase[site] = (!p.haploid && first0 >= 0) ? p.read_ps[first0] : 0;       // :349 (set 0 holds HP-tagged reads only)
        p.site_al0[site] = al0;
        p.site_n2[site] = (int32_t)(b - v);
        if (p.haploid) p.site_nr[site] = s_all;
        else { p.site_nr[site * 3] = s_1; p.site_nr[site * 3 + 1] = s_2; p.site_nr[site * 3 + 2] = s_all; }
    }
}

}   // namespace

void nc_pipe_launch_impute_flags(hipStream_t st, int n_chunks, int maxcol, const PipeChunk *pc, int8_t *ctype, const ImpArgs &imp, int32_t *err)
{
    hipLaunchKernelGGL(k_impute_flags, dim3((unsigned)n_chunks, (unsigned)((maxcol + 4095) / 4096)), dim3(256), 0, st, pc, ctype, imp, err);
}
void nc_pipe_launch_pick(hipStream_t st, int n_chunks, const PipeChunk *pc, const int8_t *ctype, int32_t win, int32_t *seg_pos, int8_t *seg_type, int32_t *cnt, int32_t *err)
{
    hipLaunchKernelGGL(k_pick, dim3(n_chunks), dim3(64), 0, st, pc, ctype, win, seg_pos, seg_type, cnt, err);
}
void nc_pipe_launch_pick_listed(hipStream_t st, int n_chunks, const PipeChunk *pc, const int8_t *ctype, int32_t win, int32_t *seg_pos, int8_t *seg_type,
                                int32_t *seg_src, int32_t *cnt, int32_t *err)
{
    hipLaunchKernelGGL(k_pick_listed, dim3(n_chunks), dim3(64), 0, st, pc, ctype, win, seg_pos, seg_type, seg_src, cnt, err);
}
void nc_pipe_launch_flatten(hipStream_t st, int n_chunks, const PipeChunk *pc, const int32_t *seg_pos, const int8_t *seg_type, const int32_t *cnt,
                            const int32_t *off, int32_t *anc_pos, int8_t *anc_type, int32_t *anc_chunk)
{
    hipLaunchKernelGGL(k_flatten, dim3(n_chunks), dim3(256), 0, st, pc, seg_pos, seg_type, cnt, off, anc_pos, anc_type, anc_chunk);
}
void nc_pipe_launch_sets(hipStream_t st, const SetArgs &sa, bool fill, bool impute, bool sampled)
{
    const dim3 grid((sa.n_anchor + 3) / 4);
    if (sampled) {                                                    // (with shared names or impute_indel_phase: refused by the plan)
        if (fill) hipLaunchKernelGGL((k_sets<true, false, false, true>), grid, dim3(256), 0, st, sa);
        else hipLaunchKernelGGL((k_sets<false, false, false, true>), grid, dim3(256), 0, st, sa);
    } else if (sa.mt.n > 0 && !impute) {                              // (shared names with impute_indel_phase: refused by the plan)
        if (fill) hipLaunchKernelGGL((k_sets<true, false, true, false>), grid, dim3(256), 0, st, sa);
        else hipLaunchKernelGGL((k_sets<false, false, true, false>), grid, dim3(256), 0, st, sa);
    } else if (fill && impute) hipLaunchKernelGGL((k_sets<true, true, false, false>), grid, dim3(256), 0, st, sa);
    else if (fill) hipLaunchKernelGGL((k_sets<true, false, false, false>), grid, dim3(256), 0, st, sa);
    else if (impute) hipLaunchKernelGGL((k_sets<false, true, false, false>), grid, dim3(256), 0, st, sa);
    else hipLaunchKernelGGL((k_sets<false, false, false, false>), grid, dim3(256), 0, st, sa);
}
int nc_pipe_scan_i32(nc_ctx *ctx, hipStream_t st, DevBuf &part, const int32_t *in, int32_t n, int32_t *out)
{
    return scan_launch<SC_PLAIN, int32_t>(ctx, st, part, in, n, 0, out, true, nullptr, nullptr);
}
int nc_pipe_scan_twb(nc_ctx *ctx, hipStream_t st, DevBuf &part, const int32_t *in, int32_t n, int64_t *out, int32_t *total_mbox)
{
    return scan_launch<SC_TWB, int64_t>(ctx, st, part, in, n, 0, out, true, total_mbox, nullptr);
}
int nc_pipe_scan_pos(nc_ctx *ctx, hipStream_t st, DevBuf &part, const int32_t *in, int32_t n, int64_t *out, long long *base_io)
{
    return scan_launch<SC_POS, int64_t>(ctx, st, part, in, n, 0, out, false, nullptr, base_io);
}

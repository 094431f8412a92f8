// Device indel pipeline, listed columns (nc_indel_set_sites): a given list of indel columns reaches K7's decision bytes.
//   k_listed      one wave per listed column: the chunks that contain it (a bisection over the ascending chunk ends; a column on a shared chunk
//                 end belongs to both chunks), the column's depths from the read pack's tile index as k_hap_depth_b counts them, the exclusion
//                 byte, and the rewrite of that one col_type byte per chunk: -1 -> 4 (forced, long window) / 5 (forced, small window), or 2 (the
//                 column predicate of impute_indel_phase reads `... or v_pos in S`); a byte K7 decided (0, 1, 2) stays
//   k_src_sites   the forced column behind every site (k_pick<true> leaves it per anchor of a chunk's segment)
// The rule (generate_indel_pileups.py:252-304 with `elif v_pos in S`): a yielded column (reads present, not excluded) whose two haplotype depths
// reach mincov (haploid: all reads) and where neither window rule fired becomes a candidate of its class; with impute_indel_phase a column that
// fails the haplotype depths and holds 2 * mincov reads goes to the read grouping whatever its event frequencies.
#include "nc_pipe.h"

namespace {

// the col_type byte at `i` of a chunk's slice becomes f(byte), by compare-and-swap on its word: columns of one word are rewritten by different
// waves, and a column listed twice (once per class) ends as the long class whichever wave comes first
__device__ __forceinline__ void listed_rewrite(int8_t *ctype, int64_t i, int code)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(ctype) + (i >> 2);        // (col_type starts on a 16-byte boundary of K7's workspace and is padded to one)
    const int sh = (int)(i & 3) * 8;
    uint32_t old = *w;
    for (;;) {
        const int b = (int)(int8_t)((old >> sh) & 0xffu);
        int nb = b;
        if (b == -1) nb = code;
        else if (b == 5 && code == 4) nb = 4;
        if (nb == b) return;
        const uint32_t want = (old & ~(0xffu << sh)) | ((uint32_t)(nb & 0xff) << sh);
        const uint32_t seen = atomicCAS(w, old, want);
        if (seen == old) return;
        old = seen;
    }
}

template <bool MATES>
__global__ __launch_bounds__(256) void k_listed(ListedArgs p)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= p.n_sites) return;
    const int32_t v = p.pos[s];
    // off the pack's tile grid (position 0, negative, past the contig) or off every chunk: dropped, nothing is written
    if (v < 1 || v < p.tile_pos0) return;
    const int64_t g = (int64_t)v - p.tile_pos0;
    const int t = (int)(g / p.tile_size);
    if (t >= p.n_tiles) return;
    int k0;
    {
        int lo = 0, hi = p.n_chunks;                                     // first chunk that ends at or behind the column (the ends ascend)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.pc[mid].hi < v) lo = mid + 1; else hi = mid; }
        k0 = lo;
    }
    if (k0 >= p.n_chunks || p.pc[k0].lo > v) return;
    // depths at the column: an alignment is present where its code is a base or a deletion (0 .. 4), by haplotype tag -- or, for alignments that
    // share a read name, once per name (not where an earlier alignment of the name is present) on the planes of the name's haplotype mask
    int n0 = 0, n1 = 0, nu = 0;
    const int e0 = p.tile_off[t], e1 = p.tile_off[t + 1];
    for (int eb = e0; eb < e1; eb += 64) {
        const int e = eb + lane;
        bool pres = false;
        int plane = 2;
        int both = 0;
        if (e < e1) {
            const nc_tile_entry ent = p.tile_ent[e];
            const int32_t slo = ent.start & ~15, shi = (ent.end + 15) & ~15;
            if (v >= slo && v < shi) pres = p.codes[(ent.base_flag & ~int64_t(15)) + v] <= 4;
            const int hp = (int)((ent.base_flag >> 1) & 3);
            plane = p.haploid ? 0 : hp == 1 ? 0 : hp == 2 ? 1 : 2;
            if constexpr (MATES) {
                if (pres && (ent.base_flag & 8) && !p.haploid) {
                    const int self = imate_find(p.mt, (ent.base_flag & ~int64_t(15)) + slo);
                    if (self >= 0) {
                        const IndelMate me = imate_get(p.mt, self);
                        int j = me.next;
                        for (int guard = 0; guard < 64 && j != self && j >= 0 && j < p.mt.n; guard++) {      // (a damaged ring must not hang the wave)
                            const IndelMate o = imate_get(p.mt, j);
                            if (j < self && v >= (o.start & ~15) && v < ((o.end + 15) & ~15) && p.codes[(p.mt.key[j] - (o.start & ~15)) + v] <= 4) pres = false;
                            j = o.next;
                        }
                        const int nm = me.hap & 3;
                        plane = nm == 1 ? 0 : nm == 2 ? 1 : 2;
                        both = nm == 3;
                    }
                }
            }
        }
        n0 += __popcll(__ballot(pres && (plane == 0 || both)));
        n1 += __popcll(__ballot(pres && (plane == 1 || both)));
        nu += __popcll(__ballot(pres && plane == 2 && !both));
    }
    if (n0 + n1 + nu == 0) return;                                       // no pileup column: never yielded
    if (p.excl && p.excl[g]) return;                                     // excluded: never yielded
    int code = -1;
    if (p.haploid ? n0 >= p.mincov : (n0 >= p.mincov && n1 >= p.mincov)) code = (p.is_long && p.is_long[s]) ? 4 : 5;
    else if (p.impute && !p.haploid && n0 + n1 + nu >= 2 * p.mincov) code = 2;
    if (code < 0 || lane != 0) return;
    for (int k = k0; k < p.n_chunks; k++) {
        const PipeChunk c = p.pc[k];
        if (c.lo > v) break;                                             // (the starts ascend)
        if (v > c.hi) continue;
        listed_rewrite(p.ctype, c.coloff + (v - c.lo), code);
    }
}

__global__ __launch_bounds__(256) void k_src_sites(const PipeChunk *__restrict__ pc, const int32_t *__restrict__ seg_src, const int32_t *__restrict__ cnt,
                                                   const int32_t *__restrict__ off, const int32_t *__restrict__ kept, const int32_t *__restrict__ site_of,
                                                   int32_t *__restrict__ site_src)
{
    const PipeChunk c = pc[blockIdx.x];
    const int n = cnt[c.id], o = off[c.id];
    for (int k = threadIdx.x; k < n; k += 256)
        if (kept[o + k]) site_src[site_of[o + k]] = seg_src[c.seg0 + k];
}

}   // namespace

void nc_pipe_launch_listed(hipStream_t st, const ListedArgs &la)
{
    if (la.n_sites <= 0 || la.n_chunks <= 0) return;
    const dim3 grid((la.n_sites + 3) / 4);
    if (la.mt.n > 0) hipLaunchKernelGGL(k_listed<true>, grid, dim3(256), 0, st, la);
    else hipLaunchKernelGGL(k_listed<false>, grid, dim3(256), 0, st, la);
}
void nc_pipe_launch_src_sites(hipStream_t st, int n_chunks, const PipeChunk *pc, const int32_t *seg_src, const int32_t *cnt, const int32_t *off,
                              const int32_t *kept, const int32_t *site_of, int32_t *site_src)
{
    hipLaunchKernelGGL(k_src_sites, dim3(n_chunks), dim3(256), 0, st, pc, seg_src, cnt, off, kept, site_of, site_src);
}

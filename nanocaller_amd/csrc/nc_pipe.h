// Device-resident indel featuriser (gfx950): what its translation units share.  get_indel_testing_candidates (reference
// generate_indel_pileups.py:129-371; haploid generate_indel_pileups_haploid.py:118-277) for all chunks of a contig with no host code between the
// column decisions and the CNN input.  The kernels live in anonymous namespaces of their units; the driver (nc_pipe.hip) fills the argument
// structs below and reaches the kernels through the nc_pipe_launch_* / nc_pipe_scan_* functions at the end of this file.
//
//   nc_pipe_plan.hip     plan: k_impute_flags, k_pick, k_flatten, k_sets (anchors, read sets) and the two-launch scans
//   nc_pipe_listed.hip   plan: k_listed, k_src_sites -- a given list of indel columns (nc_indel_set_sites) written into K7's col_type
//   nc_pipe_windows.hip  run:  k_windows16 + k_window_lists (k_windows: the one-lane form) -- query windows and their band classes
//   nc_pipe_align.hip          k_fill_band<1|2> (banded), k_fill16q (full matrix) -- the Gotoh DP; writes the traceback codes
//   nc_pipe_trace.hip          k_trace_band12, k_end_cells, k_trace16p, k_allele_trace_b12, k_allele_trace16p -- reads them
//   nc_pipe_sites.hip          k_site_tensor, k_allele_classes, k_alt_copy -- tensors, consensus, ALT strings
//   nc_pipe.hip          nc_pipe_state, the nc_indel_sites_* entry points, the group driver
#pragma once
#include "nc_common.h"
#include "nc_indel.h"

constexpr int PICK_CAP = 12288;        // anchors of one chunk held in LDS by k_pick (a 100 kb chunk has at most 9,092), one packed word each: 48 KB, three waves per CU
constexpr int IMP_CAP = 512;           // reads of one column that impute_group can group (a deeper column raises the capacity bit)
constexpr int TWB_PITCH = 36;        // words of banded traceback codes per block of 8 anti-diagonals and alignment (C = 2: 32 cells + 4 empty slots a superblock)
constexpr int BAND_NBLK4 = 44;       // ... stored in whole superblocks of four blocks
constexpr int BAND_NBLK = 41;        // blocks of 8 anti-diagonals of a banded ALLELE alignment: n1 + n2 <= 328 (the star alignments size theirs by the window: stage_a)
constexpr int CNS_CAP = 1024;          // alignment columns of one read set (window + the longest insertion of every slot)
constexpr int SC_PARTS = 65536;        // partial sums a scan's buffer holds (tiles of 4096 inputs)
constexpr int TWB_LOG = 3, TWB = 1 << TWB_LOG;                  // steps per block of full-matrix traceback codes
__host__ __device__ __forceinline__ int tw_blocks(int n1) { return ((n1 + 15) >> TWB_LOG) + 1; }
__host__ __device__ __forceinline__ int hcol_pitch(int N1) { return (N1 + 1 + 3) & ~3; }
__host__ __device__ __forceinline__ int hlast_pitch(int W) { return (W + 3) & ~3; }      // row pitch of Hlast (FillArgs::W columns)
// cells per lane of the full-matrix fill for windows of n2 bases (0: longer than the kernels cover)
inline int cpl_for(int n2) { return n2 <= 64 ? 4 : n2 <= 128 ? 8 : n2 <= 176 ? 11 : n2 <= 272 ? 17 : 0; }

struct PipeChunk {
    int32_t lo, hi, ncol;      // columns lo .. hi (lo = max(1, start))
    int32_t a_lo;              // anchors with a_lo < v <= hi go to pass 2 (:306)
    int64_t coloff;            // offset of the chunk's col_type
    int32_t seg0;              // offset of the chunk's anchor segment
    int32_t id;                // index in the caller's chunk list
};

struct ImpArgs {
    const int32_t *tile_off;
    const nc_tile_entry *tile_ent;
    int32_t tile_pos0, tile_size, n_tiles;
    const uint8_t *codes;
    const int64_t *slot_off;
    int32_t n_reads;
    const int32_t *ev_off, *ev_pos, *ev_len, *ins_off;
    const uint8_t *ins_bases;
    const int32_t *ent_read;           // the read of every tile entry (K7's table), or NULL: by search on the slot offsets
    int32_t mincov;
};

struct SetArgs {
    const int32_t *tile_off;
    const nc_tile_entry *tile_ent;
    int32_t tile_pos0, tile_size, n_tiles;
    const uint8_t *ref_code;
    int32_t ref_pos0, ref_len;
    int64_t chrom_len;
    int32_t window_after, maxcov, mincov, haploid;
    const int64_t *slot_off;
    const int32_t *read_ps;
    int32_t n_reads;
    int32_t n_anchor;
    const int32_t *anc_pos, *anc_chunk;
    const int8_t *anc_type;
    // count pass out
    int32_t *kept, *nuniq;
    // fill pass in / out
    const int32_t *site_of, *al_of;
    int32_t *site_pos, *site_chunk, *site_type, *site_phase, *site_al0, *site_nr, *site_n2;
    int32_t *al_read, *al_site;
    uint8_t *al_member;
    // K7's per-entry tables (k_read_cursors + k_entry_rows; NULL when pass 1 ran without them): the read of every tile entry, and its first event at or after every
    // 1024-column block of the tile (less 64 columns) -> the read without a search, and for k_windows the short stretch of the read's events around the anchor
    const int32_t *ent_read, *ent_cur, *ev_off;
    int32_t spt;
    int2 *al_ev;
    ImpArgs imp;                       // (k_sets<.., true, ..>) the grouping of an imputed anchor's source column
    int32_t *err;
    IndelMates mt;                     // (k_sets<.., true>) alignments that share read names (nc_indel_set_mates); n = 0: none
    uint32_t seed;                     // (k_sets<.., SAMPLED>) nc_set_downsample's seed
};

// a given list of indel columns (nc_indel_set_sites) against one group of chunks and its col_type (k_listed)
struct ListedArgs {
    const int32_t *pos;                // [n_sites] 1-based columns, any order, duplicates allowed
    const uint8_t *is_long;            // [n_sites] 1 = the long-window class, or NULL: all small
    int32_t n_sites;
    const PipeChunk *pc;               // the group's chunks (starts and ends ascend; coloff into ctype)
    int32_t n_chunks;
    int8_t *ctype;
    const int32_t *tile_off;
    const nc_tile_entry *tile_ent;
    int32_t tile_pos0, tile_size, n_tiles;
    const uint8_t *codes;
    const uint8_t *excl;               // on the pack's grid, or NULL
    int32_t mincov, haploid, impute;
    IndelMates mt;                     // alignments that share read names; n = 0: none
};

struct WinArgs {
    const uint8_t *codes;
    const int64_t *slot_off;
    const int32_t *rd_start, *rd_end;
    const int32_t *ev_off, *ev_pos, *ev_len, *ins_off, *tail_off;
    const uint8_t *ins_bases, *tail_bases, *read_flag;
    const int32_t *al_read, *al_site, *site_pos, *site_n2;    // al_* offset to the group's first alignment
    const int2 *al_ev;          // (k_sets) the stretch of the read's events that holds the first one at or after the anchor, or NULL: search them all
    int32_t A, W, WS;
    uint8_t *win;           // [A][WS]
    int32_t *n1;            // [A]
    unsigned long long *cells;       // [0] += n1 x n2 of every alignment (the full matrices), [1] += the cells the banded route computes
    // banded alignment (k_fill_band): the diagonals j - i the read's own CIGAR visits inside the window bound the band
    int8_t *band_lo;        // [A] lowest diagonal of the alignment's band (even, <= 0), or NULL: no banding
    int32_t *list1, *list2, *listF;   // alignments whose band fits 32 / 64 diagonals; the rest (full matrix)
    int32_t *counts;        // [0] list1, [1] list2, [2] listF (k_trace_band appends the paths that touch a band edge), [3] class F by width alone
    int32_t band_margin;    // diagonals kept free on either side of the CIGAR's range
    int8_t *wcls;           // [A] (k_windows16) band class of the window, for k_window_lists
};

struct FillArgs {
    const uint8_t *s1;           // read a = s1 + a * s1_stride, n1[a] bases (codes 0..4)
    int32_t s1_stride;
    const int32_t *n1;
    const uint8_t *ref_code;     // reference window of alignment a: ref_code + site_pos[site] - ref_pos0, site_n2[site] bases
    int32_t ref_pos0;
    const int32_t *site_pos, *site_n2;
    const int32_t *al_site;      // site of alignment a, or (NULL) site0 + a / site_div
    int32_t site0, site_div;
    int32_t A, W;                // alignments; row pitch of Hlast
    int32_t open, extend, match, mismatch;
    const int64_t *arow;         // first traceback BLOCK (8 steps) of alignment a, or (NULL) a * tw_blocks(N1)
    int32_t N1;                  // longest read of the launch (row pitch of hcol: hcol_pitch(N1), a multiple of four words)
    uint32_t *Tw;
    int32_t *Hlast, *hcol;       // free-tail end point inputs (NULL for a global alignment, and when `endcell` is set)
    int2 *endcell;               // free-tail end point (i, j) of alignment a (k_end_cells), read by k_trace16p instead of Hlast / hcol
    // list mode (the banded route's fallback): entry x < min(*count, A) of `list` is the alignment, x its slot in Tw / Hlast / hcol / endcell
    const int32_t *list, *count;
};
__device__ __forceinline__ int fill_site(const FillArgs &p, int al) { return p.al_site ? p.al_site[al] : p.site0 + al / p.site_div; }

// Traceback storage of the full matrix.  The DP runs as a wavefront: at step t lane q of a 16-lane group works on read row t - q and produces CPL
// 4-bit codes.  The codes of the 8 steps lane q spends on block t >> 3 of its alignment are ONE contiguous run of CPL words:
//     run = ((first_block + (t >> 3)) * 16 + q) * CPL            [words]
//     words 0 .. 8 F - 1      the F = CPL / 8 full words (8 codes each) of step s = t & 7 at s * F + w
//     words 8 F .. CPL - 1    the R = CPL % 8 remaining codes of every step, 4 R bits a step, step s at bit 4 R s (8 steps = R words)
// so a traceback that climbs a diagonal (row - 1, column - 1: same lane, step - 1) stays inside one 44-byte run (CPL = 11) for 8 steps.
// [Rows stored one after the other made the fill write 16 partial lines per instruction (33 ms, 2.6x the arithmetic); steps stored one
// after the other fixed the writes (15 ms) but left the traceback one 64-byte sector per step (11 GB per chr20-sized contig); whole words
// per step (2 for 11 codes, 4 for 17) wrote 28.5 GB per pass for 15.3 GB of codes.]  The fill kernel collects 8 steps per lane in LDS (a
// lane reads back only what it wrote itself) and writes whole runs.
// A code: bit 0 = E beats the diagonal, bit 1 = F beats both, bit 2 = E opened, bit 3 = F opened (the banded codes are the same four bits).
__device__ __forceinline__ int64_t tw_run(int64_t first_block, int t, int q, int CPL) { return ((first_block + (t >> TWB_LOG)) * 16 + q) * (int64_t)CPL; }
struct __attribute__((packed, aligned(4))) U4 { uint32_t x, y, z, w; };      // four words at a 4-byte aligned address (one dwordx4 access)

struct BandArgs {
    FillArgs f;                  // windows, reference, scoring (Tw / Hlast / hcol / endcell unused)
    const int32_t *list;         // the alignments of this class (indices into the group), *count of them
    const int32_t *count;
    const int8_t *band_lo;       // [A] lowest diagonal (even, -B < lo <= 0)
    uint32_t *Twb;               // [A][NBLK * TWB_PITCH] words: see TbBand (nc_pipe_trace.hip)
    int16_t *hrow, *hcolb;       // [A][64] H of the band's cells in the last row / the last column, by diagonal index d - lo
    int32_t NBLK;                // blocks of 8 anti-diagonals per alignment
    int32_t *redo_list, *redo_count;      // the banded tracebacks: alignments whose path touched an edge of the band
    int32_t edge;                // ... = came within `edge` diagonals of it.  Always 0 (the edge diagonals themselves); the field stays because the
                                 // constant folded into k_allele_trace_b12 costs it 57 instructions and two VGPRs
};

struct TensorArgs {
    int32_t site0, n_sites_g, S, haploid, W, WS;
    int64_t A0;                                 // first alignment of the group
    const int32_t *site_al0, *site_nr, *site_pos, *site_n2;
    const uint8_t *al_member;                   // global
    const uint8_t *win;                         // group-local [A][WS]
    const uint32_t *ent;                        // group-local [A][EW] packed alignment entries (k_trace16p)
    int32_t EW;
    const uint8_t *ref_code;
    int32_t ref_pos0;
    float *x;                                   // global [n_sites][S*5][128][2]
    uint8_t *cns;                               // group-local [n_sites_g * S][CNS_CAP], gap-free consensus
    int32_t *ncns;                              // group-local [n_sites_g * S]
    int16_t *cband;                             // group-local [n_sites_g * S][2]: lowest / highest diagonal of the consensus against the window (or NULL)
    int32_t *err;
};

// ---- launches (enqueue only; the caller checks hipGetLastError where it did before)
// nc_pipe_plan.hip
void nc_pipe_launch_impute_flags(hipStream_t st, int n_chunks, int maxcol, const PipeChunk *pc, int8_t *ctype, const ImpArgs &imp, int32_t *err);
void nc_pipe_launch_pick(hipStream_t st, int n_chunks, const PipeChunk *pc, const int8_t *ctype, int32_t win, int32_t *seg_pos, int8_t *seg_type, int32_t *cnt, int32_t *err);
// k_pick<true>: col_type may hold the forced codes 4 / 5 (k_listed); seg_src = the forced column behind an anchor, 0 for a natural one
void nc_pipe_launch_pick_listed(hipStream_t st, int n_chunks, const PipeChunk *pc, const int8_t *ctype, int32_t win, int32_t *seg_pos, int8_t *seg_type,
                                int32_t *seg_src, int32_t *cnt, int32_t *err);
void nc_pipe_launch_flatten(hipStream_t st, int n_chunks, const PipeChunk *pc, const int32_t *seg_pos, const int8_t *seg_type, const int32_t *cnt,
                            const int32_t *off, int32_t *anc_pos, int8_t *anc_type, int32_t *anc_chunk);
void nc_pipe_launch_sets(hipStream_t st, const SetArgs &sa, bool fill, bool impute, bool sampled);   // k_sets<fill, impute, sa.mt.n > 0, sampled>
// exclusive scans in two launches; `part` holds the partial sums (SC_PARTS of them: a longer array is refused).  out[n] = the total, except _pos
int nc_pipe_scan_i32(nc_ctx *ctx, hipStream_t st, DevBuf &part, const int32_t *in, int32_t n, int32_t *out);
int nc_pipe_scan_twb(nc_ctx *ctx, hipStream_t st, DevBuf &part, const int32_t *in, int32_t n, int64_t *out, int32_t *total_mbox);      // of tw_blocks(in[i]); the total also as a row mailbox
int nc_pipe_scan_pos(nc_ctx *ctx, hipStream_t st, DevBuf &part, const int32_t *in, int32_t n, int64_t *out, long long *base_io);      // of max(in[i], 0), from *base_io, which it advances
// nc_pipe_listed.hip
void nc_pipe_launch_listed(hipStream_t st, const ListedArgs &la);
void nc_pipe_launch_src_sites(hipStream_t st, int n_chunks, const PipeChunk *pc, const int32_t *seg_src, const int32_t *cnt, const int32_t *off,
                              const int32_t *kept, const int32_t *site_of, int32_t *site_src);
// nc_pipe_windows.hip
enum { NC_WIN_16 = 0, NC_WIN_FORCE16 = 1, NC_WIN_SERIAL = 2 };      // the 16-lane kernel; ... with every window on its serial route; one lane per window
void nc_pipe_launch_windows(hipStream_t st, const WinArgs &wa, int mode);
// nc_pipe_align.hip
void nc_pipe_launch_fill(hipStream_t st, int CPL, const FillArgs &fa);                         // k_fill16q<CPL>
void nc_pipe_launch_fill_band(hipStream_t st, const BandArgs &b1, const BandArgs &b2);         // k_fill_band<1>(b1), k_fill_band<2>(b2)
// nc_pipe_trace.hip
void nc_pipe_launch_trace_band(hipStream_t st, const BandArgs &b1, const BandArgs &b2, uint32_t *ent, int32_t EW);
void nc_pipe_launch_trace(hipStream_t st, const FillArgs &fa, int CPL, uint32_t *ent, int32_t EW);      // k_end_cells, k_trace16p
void nc_pipe_launch_band_stats(hipStream_t st, const int32_t *counts, long long *acc);
void nc_pipe_launch_allele_trace_band(hipStream_t st, const BandArgs &b1, const BandArgs &b2, int CPL, const int32_t *site_type, int32_t win_size, int16_t *runs, int32_t *ref_len, int32_t *alt_len);
void nc_pipe_launch_allele_trace(hipStream_t st, const BandArgs &bb, int CPL, const int32_t *site_type, int32_t win_size, int16_t *runs, int32_t *ref_len, int32_t *alt_len);
// nc_pipe_sites.hip
void nc_pipe_launch_site_tensor(hipStream_t st, const TensorArgs &ta, bool wide_counters);
void nc_pipe_launch_allele_classes(hipStream_t st, const FillArgs &fb, const int16_t *cband, int32_t margin, int32_t max_sum, int8_t *band_lo, int32_t *list1,
                                   int32_t *list2, int32_t *listF, int32_t *counts);
void nc_pipe_launch_alt_copy(hipStream_t st, const uint8_t *cns, const int32_t *alt_len, const int64_t *off, int32_t n, uint8_t *pool, int64_t pool_cap, int32_t *err);

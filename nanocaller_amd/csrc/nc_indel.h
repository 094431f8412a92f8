// K7, the indel candidate window scan (pass 1 of get_indel_testing_candidates, reference generate_indel_pileups.py:197-276): what its units
// (nc_indel.hip, nc_indel_tiles.hip, nc_indel_accum.hip) and the device-resident pipeline (nc_pipe.h) share.
#pragma once
#include <vector>

#include "nc_common.h"

// All chunks of a call run in the same launches (chunk = a grid dimension), each chunk with its own workspace slice and
// the reference's per-chunk semantics (window deques start empty at the chunk's first column)
struct IndelChunk {
    int32_t lo, hi, ncol, nd;
    int64_t ws;          // byte offset of depth[3][ncol] | rank[ncol+1] | diff[8][nd] | (impute) cnt[3][ncol] in the workspace
    int64_t coloff;      // offset of this chunk's col_type in the concatenated output
    int32_t tile0, blk0; // first tile of the chunk on the pack's grid, first k_hap_depth_b block of the chunk
};
__device__ __forceinline__ int32_t *ck_depth(char *ws, const IndelChunk &c) { return (int32_t *)(ws + c.ws); }
__device__ __forceinline__ int32_t *ck_rank(char *ws, const IndelChunk &c) { return (int32_t *)(ws + c.ws) + (int64_t)3 * c.ncol; }
__device__ __forceinline__ int32_t *ck_diff(char *ws, const IndelChunk &c) { return (int32_t *)(ws + c.ws) + (int64_t)3 * c.ncol + c.ncol + 1; }
// impute_indel_phase only: per column, over ALL kept reads: [0] reads deleted here ('*'), [1] insertions / [2] deletions that follow this column
__device__ __forceinline__ int32_t *ck_cnt(char *ws, const IndelChunk &c) { return ck_diff(ws, c) + (int64_t)8 * c.nd; }

// columns per workgroup of the tiled form (k_event_tiles), and per block of its cursor tables
constexpr int EV_SUB = 1024;
// words per tile entry of the cursor table (k_read_cursors + k_entry_rows, nc_indel_tiles.hip) for spt EV_SUB-column blocks per tile
#define NC_ENT_CUR_PITCH(spt) (2 * (spt) + 3)

// Alignments that share a read name, for the indel kernels (nc_indel_set_mates; the <.., MATES = true> forms of k_hap_depth_b, k_event_tiles, k_sets).
// The reference keys its hap sets, phase_dict, the per-column event sets and pass 2's read dicts by NAME (generate_indel_pileups.py:180-188,218-235,
// 310-338).  key [n] = byte offset of the alignment's slot in the pack's codes, ascending (= file order); rec [n][8] int32 = start, end, table index of
// the name's next alignment (a ring in file order), the alignment's index among the kept reads | the name's haplotype mask (bit 0: a record of the
// name has HP 1, bit 1: HP 2), phase_dict[name] (PS of the name's last record, 0 when that record has no HP), 0, 0.
struct IndelMates {
    const int64_t *key;
    const int32_t *rec;
    int32_t n;
};
struct IndelMate { int32_t start, end, next, read, hap, ps; };
__device__ __forceinline__ IndelMate imate_get(const IndelMates &m, int i)
{
    const int4 a = reinterpret_cast<const int4 *>(m.rec)[2 * i];
    const int2 b = reinterpret_cast<const int2 *>(m.rec)[4 * i + 2];
    return IndelMate{a.x, a.y, a.z, a.w, b.x, b.y};
}
// the table index of the alignment whose slot starts at byte `key`; -1: none (an entry flagged without a row: a table of another pack)
__device__ __forceinline__ int imate_find(const IndelMates &m, int64_t key)
{
    int lo = 0, hi = m.n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (m.key[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < m.n && m.key[lo] == key ? lo : -1;
}

// per-column decision of :252-275 (float64 divide-and-compare, as in the reference) from the depths n0 / n1 of the two haplotypes (haploid:
// n0 = all reads) and the window counts U(class, haplotype) at the column's rank
template <class UF>
__device__ __forceinline__ int8_t indel_decide(int k, int n0, int n1, UF U, int32_t mincov, double ins_t, double del_t, int32_t haploid)
{
    if (haploid) {
        if (k >= 0 && n0 >= mincov && n0 > 0) {
            double f[4];
#pragma unroll
            for (int cls = 0; cls < 4; cls++) f[cls] = (double)U(cls, 0) / (double)n0;
            if (f[0] >= del_t || f[1] >= ins_t) return 0;
            if (f[2] >= del_t || f[3] >= ins_t || (f[2] + f[3]) >= 0.9) return 1;
        }
    } else if (k >= 0 && n0 >= mincov && n1 >= mincov) {
        double f[4][2];
#pragma unroll
        for (int cls = 0; cls < 4; cls++) {
            f[cls][0] = n0 > 0 ? (double)U(cls, 0) / (double)n0 : 0.0;
            f[cls][1] = n1 > 0 ? (double)U(cls, 1) / (double)n1 : 0.0;
        }
        if (fmax(f[0][0], f[0][1]) >= del_t || fmax(f[1][0], f[1][1]) >= ins_t) return 0;
        if (fmax(f[2][0], f[2][1]) >= del_t || fmax(f[3][0], f[3][1]) >= ins_t || (f[2][0] + f[3][0]) >= 0.9 || (f[2][1] + f[3][1]) >= 0.9) return 1;
    }
    return -1;
}

// ---- one group of chunks, laid out in the workspace and ready to launch (nc_indel.hip fills it; the two forms' launch functions read it)
struct IndelGroup {
    const nc_readpack *pack;
    const nc_indel_events *ev;
    const nc_indel_scan_params *prm;
    const uint8_t *excl;               // device, on the pack's grid, or NULL
    int32_t impute;                    // prm->impute && !prm->haploid
    const std::vector<IndelChunk> *ck; // the descriptors on the host ...
    IndelChunk *ck_dev;                // ... and their place in the workspace
    int32_t ng, nblk;                  // chunks; tile-blocks (k_hap_depth_b's grid)
    char *ws;                          // the workspace: [0, zero_bytes) the chunks' slices
    size_t zero_bytes;
    int8_t *ctype;                     // the chunks' col_type, back to back
    int32_t *blk;                      // [3][nblk]: blk_chunk, blk_yield, blk_base
};
// What the device pipeline's plan (nc_indel_sites_plan) hands K7 beside the scan's own arguments.  With it the scan may take the tiled form
// (nc_indel.hip says when); without it the call is the stand-alone scan.  All pointers on the device.
struct IndelPipeIn {
    const int64_t *slot_off;           // slot offset of every read of the events: the map tile entry -> read
    const int32_t *rd_start, *rd_end;
    int32_t *err_bits;
    bool reuse_tables;                 // a later group of chunks of the SAME pack and events: the cursor tables of the first group stand
    IndelMates mates;                  // alignments that share read names (n = 0: none)
};
struct IndelGroupOut {
    int32_t consumed = 0;              // chunks of the list the group took
    std::vector<IndelChunk> ck;        // their descriptors
    const IndelChunk *ck_dev = nullptr;
    const int8_t *ctype = nullptr;     // the per-column decisions, on the device, chunk k at ck[k].coloff
};

// nc_indel.hip: the two entry points the pipeline's plan calls (K7 for a group of chunks enqueued, col_type left on the device; the argument
// checks of the scan), and what both forms launch first: the descriptors' upload, k_blk_chunks, k_hap_depth_b.  blk_yield: where k_hap_depth_b
// leaves the tile-blocks' counts of yielded columns -- then it writes 16-bit depth rows and block-local ranks, as the tiled form reads them -- or NULL
int nc_indel_scan_group_launch(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const uint8_t *excl_dev, int32_t n_chunks,
                               const int32_t *starts, const int32_t *ends, const nc_indel_scan_params *prm, const IndelPipeIn *pipe, IndelGroupOut *out);
int nc_indel_check(nc_ctx *ctx, const nc_readpack *pack, const nc_indel_events *ev, const nc_indel_scan_params *prm, const char *who);
int nc_indel_launch_depths(nc_ctx *ctx, const IndelGroup &g, int32_t *blk_yield, const IndelMates &mt);
// nc_indel_tiles.hip / nc_indel_accum.hip: the rest of the group's launches in either form (enqueue only)
int nc_indel_launch_tiles(nc_ctx *ctx, const IndelGroup &g, const IndelPipeIn &pipe);
int nc_indel_launch_accum(nc_ctx *ctx, const IndelGroup &g);

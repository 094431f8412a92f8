// Device-resident indel featuriser, the host side: nc_pipe_state and the nc_indel_sites_* entry points (the kernels and what the units share: nc_pipe.h).
//   plan   K7 (nc_indel.hip) -> anchors (k_impute_flags, k_pick, k_flatten) -> sites, read sets and their alignments (k_sets, twice: count, fill);
//          with a list of columns to genotype (nc_indel_set_sites): k_listed behind K7, k_pick_listed for k_pick, k_src_sites behind the fill
//   run    per group of sites (bounded by the traceback workspace), two groups in flight (PipeRun):
//          stage_a   stream A: k_windows16 + k_window_lists, then k_fill_band<1|2> (band off: k_fill16q)
//          stage_b1  stream B: k_trace_band12, the redo list on the full matrix (k_fill16q, k_end_cells, k_trace16p), k_site_tensor, the scan of the
//                    consensus lengths -- the host waits for its total
//          stage_b2  stream B: allele_prediction (:77-127): k_allele_classes, k_fill_band<1|2>, k_allele_trace_b12, the rest on the full matrix
//                    (k_fill16q, k_allele_trace16p), the ALT prefixes (scan + k_alt_copy)
// Results equal nc_indel_pass2_sets -> nc_star_msa_tensor_dup -> nc_allele_prediction_device (tests/test_indel_pipeline.py).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "nc_pipe.h"

struct nc_pipe_state {
    bool planned = false, ran = false;
    nc_readpack pack;
    nc_indel_reads rd;
    const uint8_t *ref_code = nullptr;
    int32_t ref_pos0 = 0, ref_len = 0;
    int64_t chrom_len = 0;
    int32_t window_after = 0, maxcov = 0, mincov = 0, win_size = 0, haploid = 0, S = 3;
    int32_t n_chunks = 0, n_anchor = 0, n_sites = 0;
    int64_t n_al = 0;
    int32_t *al0_pin = nullptr;             // page-locked: first alignment of every site (+ total), read by the host to cut the groups
    int64_t tw_budget = 0;                  // bytes of traceback codes per group (set at the first run from the free device memory)
    size_t al0_cap = 0;
    DevBuf pc, seg_pos, seg_type, cnt, off, anc_pos, anc_type, anc_chunk, kept, nuniq, site_of, al_of;
    DevBuf site_pos, site_chunk, site_type, site_phase, site_al0, site_nr, site_n2, al_read, al_site, al_member, al_ev;
    DevBuf seg_src, site_src;               // (a list of columns was set: nc_indel_set_sites) the forced column behind every anchor / site
    bool listed = false;                    // the last plan ran with a list
    bool have_al_ev = false;
    struct GroupBufs {
        DevBuf win, n1, tw, hlast, hcol, endc, trace, cns, ncns, arow, alt_off;
        DevBuf band_lo, lists, counts, twb, hrow, hcolb, cband;                // banded star alignment: per-alignment band, class lists, codes, last row / column
    } gb[2];                                // two sets: group g+1 is aligned while g is reduced
    int32_t band_mode = -1, band_margin_v = 0;   // nc_indel_sites_band: -1 = the environment's setting
    int64_t band_stats[6] = {0, 0, 0, 0, 0, 0};   // of the last run: alignments on 32 / 64 diagonals, on the full matrix by width, re-run after an edge touch
    DevBuf tw2, runs, rlen, alen, alt_pool, misc;
    DevBuf part_a, part_b;                   // partial sums of the two-launch scans (plan / stream A; stream B)
    DevBuf ab_lo, ab_lists, ab_counts, ab_twb;             // banded allele alignments (PipeRun::stage_b2; one group at a time on stream B)
    hipStream_t sB = nullptr;                // second stream: traceback / tensors / alleles of group g beside the alignment fill of g + 1
    hipEvent_t evA[2] = {nullptr, nullptr}, evB[2] = {nullptr, nullptr}, ev_join = nullptr;
    int64_t alt_pool_cap = 0;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t scoring[4] = {25, 1, 20, -10};         // star alignment: gap open, gap extend, match, mismatch (nc_indel_sites_scoring)
    float stage_ms[6] = {0, 0, 0, 0, 0, 0};
    int64_t cells[2] = {0, 0};
};

void nc_pipe_destroy(nc_ctx *ctx)
{
    nc_pipe_state *s = ctx->pipe;
    if (!s) return;
    for (auto &e : s->ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : s->evA) if (e) (void)hipEventDestroy(e);
    for (auto &e : s->evB) if (e) (void)hipEventDestroy(e);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->sB) (void)hipStreamDestroy(s->sB);
    if (s->al0_pin) (void)hipHostFree(s->al0_pin);
    delete s;                                                      // (its DevBufs free themselves)
    ctx->pipe = nullptr;
}

// banded star alignment (k_fill_band): on unless NC_PIPE_BAND=0; NC_PIPE_BAND_MARGIN = diagonals kept free on either side of the range the read's
// CIGAR covers (default 6).  Read at every run: tests switch them
static bool band_on() { const char *e = getenv("NC_PIPE_BAND"); return !(e && atoi(e) == 0); }
static int band_margin() { const char *e = getenv("NC_PIPE_BAND_MARGIN"); return e ? std::max(1, std::min(15, atoi(e))) : 6; }

extern "C" int nc_indel_sites_plan(nc_ctx *ctx, const nc_readpack *pack, const uint8_t *ref_code_dev, int32_t ref_pos0, int32_t ref_len,
                                   int64_t chrom_len, const nc_indel_reads *reads, const uint8_t *excl_dev, int32_t n_chunks,
                                   const int32_t *starts, const int32_t *ends, const nc_indel_scan_params *prm, int32_t window_after,
                                   int32_t maxcov, int32_t *n_sites, int64_t *n_alignments)
{
    if (!ctx) return NC_ERR_ARG;
    if (!pack || !ref_code_dev || !reads || !prm || !n_sites || !n_alignments || n_chunks < 0 || (n_chunks && (!starts || !ends)) || window_after < 1 ||
        maxcov < 1 || chrom_len < 1)
        return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_plan: bad argument");
    const bool impute = prm->impute && !prm->haploid;                 // (generate_indel_pileups.py:278: the diploid function only)
    if (impute && (!reads->ins_off || !reads->ins_bases)) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_plan: impute_indel_phase needs the inserted bases");
    if (cpl_for(window_after + 1) == 0) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites_plan: windows longer than 271 bases");
    // alignments that share read names (nc_indel_set_mates): K7 and k_sets key them by name; the read grouping of impute_indel_phase does not
    const IndelMates mates = {ctx->imate_key, ctx->imate_rec, ctx->n_imates};
    if (mates.n > 0 && impute)
        return nc_fail(ctx, NC_ERR_UNSUPPORTED, "nc_indel_sites_plan: impute_indel_phase on a contig whose kept alignments share read names");
    // the uniform sample above maxcov (nc_set_downsample): k_sets has it in its plain form only; never served by the first-maxcov cut instead
    const bool sampled = ctx->downsample == 1;
    if (sampled && mates.n > 0)
        return nc_fail(ctx, NC_ERR_UNSUPPORTED, "nc_indel_sites_plan: the uniform sample above maxcov (nc_set_downsample) on a contig whose kept alignments share read names");
    if (sampled && impute)
        return nc_fail(ctx, NC_ERR_UNSUPPORTED, "nc_indel_sites_plan: the uniform sample above maxcov (nc_set_downsample) with impute_indel_phase");
    nc_indel_events ev;
    ev.n_reads = reads->n_reads; ev.ev_off = reads->ev_off; ev.ev_pos = reads->ev_pos; ev.ev_len = reads->ev_len; ev.read_hap = reads->read_hap;
    NC_TRY(nc_indel_check(ctx, pack, &ev, prm, "nc_indel_sites_plan"));
    NC_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->pipe) ctx->pipe = new (std::nothrow) nc_pipe_state();
    nc_pipe_state *s = ctx->pipe;
    if (!s) return NC_ERR_NOMEM;
    s->planned = s->ran = false;
    s->pack = *pack; s->rd = *reads; s->ref_code = ref_code_dev; s->ref_pos0 = ref_pos0; s->ref_len = ref_len; s->chrom_len = chrom_len;
    s->window_after = window_after; s->maxcov = maxcov; s->mincov = prm->mincov; s->win_size = prm->win_size; s->haploid = prm->haploid ? 1 : 0;
    s->S = prm->haploid ? 1 : 3;
    s->n_chunks = n_chunks; s->n_sites = 0; s->n_al = 0; s->n_anchor = 0;
    // a list of columns to genotype (nc_indel_set_sites): k_listed between K7 and k_impute_flags, k_pick in its listed form.  Without one every
    // launch below is the one it was
    const bool listed = ctx->n_isites > 0 || ctx->isites_only;
    s->listed = listed;
    *n_sites = 0;
    *n_alignments = 0;
    for (auto &m : s->stage_ms) m = 0;
    s->cells[0] = s->cells[1] = 0;
    if (n_chunks == 0) { s->planned = true; return NC_OK; }
    for (int32_t c = 0; c < n_chunks; c++) {
        if (ends[c] < starts[c]) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_plan: chunk %d has end < start", c);
        if (c && (starts[c] < starts[c - 1] || ends[c] < ends[c - 1])) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_plan: chunks must ascend");
    }
    const bool timing = ctx->timing == 1;
    if (timing)
        for (auto &e : s->ev) if (!e) NC_HIP(ctx, hipEventCreate(&e));
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[0], ctx->stream));
    // ---- anchors of every chunk
    std::vector<PipeChunk> pcs((size_t)n_chunks);
    int64_t seg_total = 0;
    for (int32_t c = 0; c < n_chunks; c++) {
        PipeChunk &k = pcs[(size_t)c];
        k.lo = starts[c] < 1 ? 1 : starts[c];
        k.hi = ends[c];
        k.ncol = k.hi - k.lo + 1;
        k.a_lo = std::max(0, starts[c] - 10 - prm->win_size);
        k.coloff = 0;
        k.seg0 = (int32_t)seg_total;
        k.id = c;
        const int64_t cap = k.ncol / 11 + 2;
        if (cap > PICK_CAP) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites_plan: chunk %d is longer than the anchor buffer covers", c);
        seg_total += cap;
        if (seg_total > INT32_MAX / 2) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites_plan: too many columns in one call");
    }
    NC_TRY(nc_ensure(ctx, s->pc, (size_t)n_chunks * sizeof(PipeChunk)));
    NC_TRY(nc_ensure(ctx, s->seg_pos, (size_t)seg_total * 4));
    NC_TRY(nc_ensure(ctx, s->seg_type, (size_t)seg_total));
    if (listed) NC_TRY(nc_ensure(ctx, s->seg_src, (size_t)seg_total * 4));
    NC_TRY(nc_ensure(ctx, s->cnt, ((size_t)n_chunks + 1) * 4));
    NC_TRY(nc_ensure(ctx, s->off, ((size_t)n_chunks + 2) * 4));
    NC_TRY(nc_ensure(ctx, s->misc, 256));
    int32_t *err = (int32_t *)s->misc.p;                              // [0] error bits, [2..3] row total mailbox, [4..5] cells, [6..7] banded cells, [8..9] alt pool bytes, [16..23] band classes
    NC_HIP(ctx, hipMemsetAsync(s->misc.p, 0, 256, ctx->stream));
    ImpArgs imp;
    memset(&imp, 0, sizeof imp);
    imp.tile_off = pack->tile_off; imp.tile_ent = pack->tile_ent; imp.tile_pos0 = pack->tile_pos0; imp.tile_size = pack->tile_size; imp.n_tiles = pack->n_tiles;
    imp.codes = pack->codes; imp.slot_off = reads->slot_off; imp.n_reads = reads->n_reads;
    imp.ev_off = reads->ev_off; imp.ev_pos = reads->ev_pos; imp.ev_len = reads->ev_len; imp.ins_off = reads->ins_off; imp.ins_bases = reads->ins_bases;
    imp.mincov = prm->mincov;
    int32_t c0 = 0;
    IndelGroupOut k7;
    while (c0 < n_chunks) {
        const IndelPipeIn k7in = {reads->slot_off, reads->rd_start, reads->rd_end, err, c0 > 0, mates};
        NC_TRY(nc_indel_scan_group_launch(ctx, pack, &ev, excl_dev, n_chunks - c0, starts + c0, ends + c0, prm, &k7in, &k7));
        const int32_t used = k7.consumed;
        const int8_t *ctype = k7.ctype;
        for (int32_t k = 0; k < used; k++) pcs[(size_t)(c0 + k)].coloff = k7.ck[(size_t)k].coloff;
        NC_TRY(nc_h2d_pieces(ctx, (PipeChunk *)s->pc.p + c0, pcs.data() + c0, (size_t)used * sizeof(PipeChunk), ctx->stream));
        if (listed) {
            // only mode: K7 ran for its per-entry tables (k_sets reads them), its verdicts are reset: the list is the only source of candidates
            if (ctx->isites_only && used > 0) {
                const PipeChunk &last = pcs[(size_t)(c0 + used - 1)];
                NC_HIP(ctx, hipMemsetAsync(const_cast<int8_t *>(ctype), 0xff, (size_t)(last.coloff + last.ncol), ctx->stream));
            }
            ListedArgs la;
            memset(&la, 0, sizeof la);
            la.pos = ctx->isite_pos; la.is_long = ctx->isite_long; la.n_sites = ctx->n_isites;
            la.pc = (const PipeChunk *)s->pc.p + c0; la.n_chunks = used; la.ctype = const_cast<int8_t *>(ctype);
            la.tile_off = pack->tile_off; la.tile_ent = pack->tile_ent; la.tile_pos0 = pack->tile_pos0; la.tile_size = pack->tile_size; la.n_tiles = pack->n_tiles;
            la.codes = pack->codes; la.excl = excl_dev; la.mincov = prm->mincov; la.haploid = prm->haploid ? 1 : 0; la.impute = impute ? 1 : 0;
            la.mt = mates;
            nc_pipe_launch_listed(ctx->stream, la);
            // NC_PIPE_DUMP (debugging aid): <dump>.col_type = the group's col_type behind k_listed with up to 64 bytes of K7's workspace on
            // either side (what lies around the bytes the kernel may write), groups appended
            if (const char *dump = getenv("NC_PIPE_DUMP")) {
                const PipeChunk &last = pcs[(size_t)(c0 + used - 1)];
                const char *base = (const char *)ctx->k7.ws.p, *ct = (const char *)ctype;
                const char *a = std::max(base, ct - 64), *b = std::min(base + ctx->k7.ws.cap, ct + last.coloff + last.ncol + 64);
                std::vector<char> h((size_t)(b - a));
                NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
                NC_HIP(ctx, hipMemcpy(h.data(), a, h.size(), hipMemcpyDeviceToHost));
                char path[512];
                snprintf(path, sizeof path, "%s.col_type", dump);
                if (FILE *fp = fopen(path, c0 == 0 ? "wb" : "ab")) { fwrite(h.data(), 1, h.size(), fp); fclose(fp); }
            }
        }
        if (impute) {                                                 // the read grouping of every col_type-2 column: 3 (an anchor) or -1
            int32_t maxcol = 1;
            for (int32_t k = 0; k < used; k++) maxcol = std::max(maxcol, pcs[(size_t)(c0 + k)].ncol);
            nc_pipe_launch_impute_flags(ctx->stream, used, maxcol, (const PipeChunk *)s->pc.p + c0, const_cast<int8_t *>(ctype), imp, err);
        }
        if (listed)
            nc_pipe_launch_pick_listed(ctx->stream, used, (const PipeChunk *)s->pc.p + c0, ctype, prm->win_size, (int32_t *)s->seg_pos.p,
                                       (int8_t *)s->seg_type.p, (int32_t *)s->seg_src.p, (int32_t *)s->cnt.p, err);
        else
        nc_pipe_launch_pick(ctx->stream, used, (const PipeChunk *)s->pc.p + c0, ctype, prm->win_size, (int32_t *)s->seg_pos.p, (int8_t *)s->seg_type.p,
                            (int32_t *)s->cnt.p, err);
        NC_HIP(ctx, hipGetLastError());
        c0 += used;                                                   // (the next group's K7 reuses the workspace in stream order)
    }
    NC_TRY(nc_ensure(ctx, s->part_a, 8 * SC_PARTS));                  // (sized once: the scans never re-allocate between launches of a pass; SC_PARTS x SC_TILE
    NC_TRY(nc_ensure(ctx, s->part_b, 8 * SC_PARTS));                  // = 268 M elements per scan, beyond any array of a pass)
    NC_TRY(nc_pipe_scan_i32(ctx, ctx->stream, s->part_a, (const int32_t *)s->cnt.p, n_chunks, (int32_t *)s->off.p));
    // counts the host waits for travel by copy kernel into the context's page-locked mailbox (a hipMemcpyAsync of either direction
    // queues behind a contig's upload in flight on this platform: DESIGN.md section 2)
    volatile int32_t *mb = ctx->mbox + 32;
    NC_TRY(nc_d2h(ctx, ctx->mbox + 32, (int32_t *)s->off.p + n_chunks, 4, ctx->stream));
    NC_TRY(nc_d2h(ctx, ctx->mbox + 33, err, 4, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t na = mb[0], errh = mb[1];
    if (errh & 1) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites_plan: anchor buffer of a chunk overflowed");
    if (errh & 8) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites_plan: more than 16,000 alignments over one tile of the index");
    if (errh & 16) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites_plan: impute_indel_phase on a column deeper than %d reads", IMP_CAP);
    s->n_anchor = na;
    s->planned = true;
    if (na == 0) {
        if (timing) { NC_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream)); }
        return NC_OK;
    }
    NC_TRY(nc_ensure(ctx, s->anc_pos, (size_t)na * 4));
    NC_TRY(nc_ensure(ctx, s->anc_type, (size_t)na));
    NC_TRY(nc_ensure(ctx, s->anc_chunk, (size_t)na * 4));
    NC_TRY(nc_ensure(ctx, s->kept, ((size_t)na + 1) * 4));
    NC_TRY(nc_ensure(ctx, s->nuniq, ((size_t)na + 1) * 4));
    NC_TRY(nc_ensure(ctx, s->site_of, ((size_t)na + 1) * 4));
    NC_TRY(nc_ensure(ctx, s->al_of, ((size_t)na + 1) * 4));
    nc_pipe_launch_flatten(ctx->stream, n_chunks, (const PipeChunk *)s->pc.p, (const int32_t *)s->seg_pos.p, (const int8_t *)s->seg_type.p,
                           (const int32_t *)s->cnt.p, (const int32_t *)s->off.p, (int32_t *)s->anc_pos.p, (int8_t *)s->anc_type.p, (int32_t *)s->anc_chunk.p);
    SetArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.tile_off = pack->tile_off; sa.tile_ent = pack->tile_ent; sa.tile_pos0 = pack->tile_pos0; sa.tile_size = pack->tile_size; sa.n_tiles = pack->n_tiles;
    sa.ref_code = ref_code_dev; sa.ref_pos0 = ref_pos0; sa.ref_len = ref_len; sa.chrom_len = chrom_len;
    sa.window_after = window_after; sa.maxcov = maxcov; sa.mincov = prm->mincov; sa.haploid = s->haploid;
    sa.slot_off = reads->slot_off; sa.read_ps = reads->read_ps; sa.n_reads = reads->n_reads;
    const bool have_ent = ctx->k7.ent_of == (const void *)pack->tile_ent && ctx->k7.ent_read.p;
    if (have_ent) {
        sa.ent_read = (const int32_t *)ctx->k7.ent_read.p; sa.ent_cur = sa.ent_read + pack->n_entries; sa.ev_off = reads->ev_off; sa.spt = ctx->k7.ent_spt;
    }
    sa.n_anchor = na; sa.anc_pos = (const int32_t *)s->anc_pos.p; sa.anc_chunk = (const int32_t *)s->anc_chunk.p; sa.anc_type = (const int8_t *)s->anc_type.p;
    sa.kept = (int32_t *)s->kept.p; sa.nuniq = (int32_t *)s->nuniq.p;
    sa.imp = imp; sa.imp.ent_read = sa.ent_read; sa.err = err;
    sa.mt = mates;
    sa.seed = ctx->downsample_seed;
    nc_pipe_launch_sets(ctx->stream, sa, false, impute, sampled);
    NC_TRY(nc_pipe_scan_i32(ctx, ctx->stream, s->part_a, (const int32_t *)s->kept.p, na, (int32_t *)s->site_of.p));
    NC_TRY(nc_pipe_scan_i32(ctx, ctx->stream, s->part_a, (const int32_t *)s->nuniq.p, na, (int32_t *)s->al_of.p));
    NC_HIP(ctx, hipGetLastError());
    NC_TRY(nc_d2h(ctx, ctx->mbox + 34, (int32_t *)s->site_of.p + na, 4, ctx->stream));
    NC_TRY(nc_d2h(ctx, ctx->mbox + 35, (int32_t *)s->al_of.p + na, 4, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t ns = mb[2], nal = mb[3];
    s->n_sites = ns;
    s->n_al = nal;
    *n_sites = ns;
    *n_alignments = nal;
    if (ns == 0) {
        if (timing) { NC_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream)); }
        return NC_OK;
    }
    const size_t NS = (size_t)ns;
    NC_TRY(nc_ensure(ctx, s->site_pos, NS * 4));
    NC_TRY(nc_ensure(ctx, s->site_chunk, NS * 4));
    NC_TRY(nc_ensure(ctx, s->site_type, NS * 4));
    NC_TRY(nc_ensure(ctx, s->site_phase, NS * 4));
    NC_TRY(nc_ensure(ctx, s->site_al0, (NS + 1) * 4));
    NC_TRY(nc_ensure(ctx, s->site_nr, NS * 3 * 4));
    NC_TRY(nc_ensure(ctx, s->site_n2, NS * 4));
    NC_TRY(nc_ensure(ctx, s->al_read, (size_t)std::max(nal, 1) * 4));
    NC_TRY(nc_ensure(ctx, s->al_site, (size_t)std::max(nal, 1) * 4));
    NC_TRY(nc_ensure(ctx, s->al_member, (size_t)std::max(nal, 1) + 16));
    sa.site_of = (const int32_t *)s->site_of.p; sa.al_of = (const int32_t *)s->al_of.p;
    sa.site_pos = (int32_t *)s->site_pos.p; sa.site_chunk = (int32_t *)s->site_chunk.p; sa.site_type = (int32_t *)s->site_type.p;
    sa.site_phase = (int32_t *)s->site_phase.p; sa.site_al0 = (int32_t *)s->site_al0.p; sa.site_nr = (int32_t *)s->site_nr.p;
    sa.site_n2 = (int32_t *)s->site_n2.p; sa.al_read = (int32_t *)s->al_read.p; sa.al_site = (int32_t *)s->al_site.p; sa.al_member = (uint8_t *)s->al_member.p;
    s->have_al_ev = have_ent;
    if (have_ent) {
        NC_TRY(nc_ensure(ctx, s->al_ev, (size_t)std::max(nal, 1) * 8));
        sa.al_ev = (int2 *)s->al_ev.p;
    }
    nc_pipe_launch_sets(ctx->stream, sa, true, impute, sampled);
    if (listed) {
        NC_TRY(nc_ensure(ctx, s->site_src, NS * 4));
        nc_pipe_launch_src_sites(ctx->stream, n_chunks, (const PipeChunk *)s->pc.p, (const int32_t *)s->seg_src.p, (const int32_t *)s->cnt.p,
                                 (const int32_t *)s->off.p, (const int32_t *)s->kept.p, (const int32_t *)s->site_of.p, (int32_t *)s->site_src.p);
    }
    NC_HIP(ctx, hipGetLastError());
    NC_TRY(nc_h2d_small(ctx, (int32_t *)s->site_al0.p + ns, &nal, 4, ctx->stream));
    if (s->al0_cap < NS + 1) {
        if (s->al0_pin) (void)hipHostFree(s->al0_pin);
        s->al0_pin = nullptr;
        s->al0_cap = 0;
        NC_HIP(ctx, hipHostMalloc((void **)&s->al0_pin, (NS + 1 + NS / 4) * 4, hipHostMallocDefault));
        s->al0_cap = NS + 1 + NS / 4;
    }
    NC_TRY(nc_d2h_pieces(ctx, s->al0_pin, s->site_al0.p, NS * 4, ctx->stream));
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[1], ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->al0_pin[NS] = nal;
    if (timing) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, s->ev[0], s->ev[1]);
        s->stage_ms[0] = ms;
    }
    return NC_OK;
}

extern "C" int nc_indel_set_mates(nc_ctx *ctx, int32_t n_mates, const int64_t *d_mate_key, const int32_t *d_mate_rec)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_mates < 0 || (n_mates > 0 && (!d_mate_key || !d_mate_rec || ((uintptr_t)d_mate_rec & 15))))
        return nc_fail(ctx, NC_ERR_ARG, "nc_indel_set_mates: bad argument");
    ctx->n_imates = n_mates;
    ctx->imate_key = n_mates ? d_mate_key : nullptr;
    ctx->imate_rec = n_mates ? d_mate_rec : nullptr;
    return NC_OK;
}

extern "C" int nc_indel_set_sites(nc_ctx *ctx, int32_t n_sites, const int32_t *d_pos, const uint8_t *d_long, int32_t only)
{
    if (!ctx) return NC_ERR_ARG;
    if (n_sites < 0 || (n_sites > 0 && !d_pos)) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_set_sites: bad argument");
    ctx->n_isites = n_sites;
    ctx->isite_pos = n_sites ? d_pos : nullptr;
    ctx->isite_long = n_sites ? d_long : nullptr;
    ctx->isites_only = only != 0;                                     // (n_sites = 0 with only: a list that names nothing here -- no candidates)
    return NC_OK;
}

extern "C" int nc_indel_sites_fetch_src(nc_ctx *ctx, int32_t *src_col)
{
    if (!ctx) return NC_ERR_ARG;
    nc_pipe_state *s = ctx->pipe;
    if (!s || !s->planned) return nc_fail(ctx, NC_ERR_STATE, "nc_indel_sites_fetch_src: nc_indel_sites_plan first");
    if (s->n_sites == 0) return NC_OK;
    if (!src_col) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_fetch_src: null buffer");
    if (!s->listed) {                                                 // a plan without a list: every anchor is a natural one
        for (int32_t k = 0; k < s->n_sites; k++) src_col[k] = 0;
        return NC_OK;
    }
    NC_HIP(ctx, hipMemcpyAsync(src_col, s->site_src.p, (size_t)s->n_sites * 4, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

extern "C" int nc_indel_sites_scoring(nc_ctx *ctx, int32_t open, int32_t extend, int32_t match, int32_t mismatch)
{
    if (!ctx) return NC_ERR_ARG;
    // The packed 16-bit fills keep every value, and every difference whose sign bit becomes a traceback bit, inside int16.  The binding one is
    // k_fill_band: its registers carry the bias 20,000 (minus infinity = 0), and the largest value it forms is the diagonal candidate
    // H[i-1][j-1] + match + 20,000 <= match * min(n1, n2) + 20,000 with min(n1, n2) <= 272 (the longest window the plan takes; cells outside the
    // rectangle never match).  It must stay <= 32,767 - extend, so that the difference against a fresh minus infinity on the band's border,
    // (0 - extend) - H', is above -2^15: match * 273 <= 12,767, match <= 46.  (match = 100, accepted until now, wraps on the band after 128
    // matching bases.)  The lower side has room: inside a band a path reaches any cell by gaps of at most 15, so H >= -(272 / 15) * 2 *
    // (open + 14 extend) - open > -9,000 at the limits below, and the chains of -extend outside the rectangle stay above -20,000 - 600 extend.
    // k_fill16q has no bias: |H - open| <= 46 * 272, and its minus infinity (-20,000 - extend) only meets column 0 and row 0, which are <= 0.
    if (open < 0 || extend < 0 || open > 100 || extend > 10 || match < 0 || match > 46 || mismatch > 0 || mismatch < -100)
        return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_scoring: scores out of the range the 16-bit aligner covers");
    if (!ctx->pipe) ctx->pipe = new (std::nothrow) nc_pipe_state();
    if (!ctx->pipe) return NC_ERR_NOMEM;
    ctx->pipe->scoring[0] = open; ctx->pipe->scoring[1] = extend; ctx->pipe->scoring[2] = match; ctx->pipe->scoring[3] = mismatch;
    return NC_OK;
}

// ---- the run.  One group of whole sites in flight on buffer set g & 1: written by stage_a, read by the stages behind it
struct PipeGroup {
    int g, k0, k1;               // group number; its sites k0 .. k1 - 1
    int64_t A0;                  // first alignment
    int32_t Ag;                  // alignments
    FillArgs fa;                 // the star alignment
    BandArgs ba;                 // ... on its band (list / count: band_class)
    int32_t *lists, *counts;     // class lists, max(Ag, 1) entries each (32 diagonals, 64, full matrix), and counts [0..3]
};
static BandArgs band_class(const PipeGroup &q, int c)
{
    BandArgs b = q.ba;
    b.list = q.lists + (size_t)c * std::max(q.Ag, 1);
    b.count = q.counts + c;
    return b;
}

struct PipeRun {
    nc_ctx *ctx;
    nc_pipe_state *s;
    float *x_dev;
    const int32_t *al0h;         // first alignment of every site (+ total), page-locked
    const char *dump;            // NC_PIPE_DUMP
    bool timing, two, band, band_alleles;
    int S, ns, W, EW, WS, N1, CPL, G, nblk, margin, win_mode;
    int64_t tw_per_al, GROUP_AL, GROUP_SITES;
    size_t Acap;
    hipStream_t sA, sB;
    PipeGroup grp[2];
    int32_t *err() const { return (int32_t *)s->misc.p; }
    int stage_a(int g, int k0, int k1);
    int stage_b1(const PipeGroup &q);
    int stage_b2(const PipeGroup &q, int64_t rows);
    void dump_wr(int g, const char *name, const void *src, size_t bytes, bool on_host) const;
    void dump_classes(int g, const char *name, int32_t n, const void *lists, size_t pitch, const void *counts, bool banded) const;
    void dump_b1(const PipeGroup &q) const;
    void dump_b2(const PipeGroup &q) const;
};

// stream A: query windows, alignment fill
int PipeRun::stage_a(int g, int k0, int k1)
{
    const int b = g & 1;
    nc_pipe_state::GroupBufs &B = s->gb[b];
    PipeGroup &q = grp[b];
    const int ng = k1 - k0;
    const int64_t A0 = al0h[k0];
    const int32_t Ag = al0h[k1] - al0h[k0];
    const size_t Agz = (size_t)std::max(Ag, 1);
    const size_t Asz = std::max(Agz, Acap);                          // what the buffers are sized for (the layout inside them goes by Agz)
    NC_TRY(nc_ensure(ctx, B.win, Asz * WS + 64));
    NC_TRY(nc_ensure(ctx, B.n1, Asz * 4));
    NC_TRY(nc_ensure(ctx, B.tw, Asz * (size_t)tw_per_al + 64));
    NC_TRY(nc_ensure(ctx, B.hlast, Asz * hlast_pitch(W) * 4 + 64));
    NC_TRY(nc_ensure(ctx, B.hcol, Asz * hcol_pitch(N1) * 4 + 64));
    NC_TRY(nc_ensure(ctx, B.endc, Asz * sizeof(int2)));
    NC_TRY(nc_ensure(ctx, B.trace, Asz * EW * 4 + 64));
    NC_TRY(nc_ensure(ctx, B.cns, (size_t)ng * S * CNS_CAP));
    NC_TRY(nc_ensure(ctx, B.ncns, (size_t)ng * S * 4));
    NC_TRY(nc_ensure(ctx, B.cband, (size_t)ng * S * 4));
    NC_TRY(nc_ensure(ctx, B.arow, ((size_t)ng * S + 1) * 8));
    NC_TRY(nc_ensure(ctx, B.alt_off, (size_t)ng * S * 8));
    if (band) {
        NC_TRY(nc_ensure(ctx, B.band_lo, 2 * Asz + 128));            // + the windows' classes (k_windows16 -> k_window_lists)
        NC_TRY(nc_ensure(ctx, B.lists, Asz * 3 * 4 + 64));
        NC_TRY(nc_ensure(ctx, B.counts, 64));
        NC_TRY(nc_ensure(ctx, B.twb, Asz * (size_t)nblk * (4 * TWB_PITCH) + 256));
        NC_TRY(nc_ensure(ctx, B.hrow, Asz * 128 + 64));
        NC_TRY(nc_ensure(ctx, B.hcolb, Asz * 128 + 64));
    }
    q.g = g; q.k0 = k0; q.k1 = k1; q.A0 = A0; q.Ag = Ag;
    q.lists = (int32_t *)B.lists.p; q.counts = (int32_t *)B.counts.p;
    if (two && g >= 2) NC_HIP(ctx, hipStreamWaitEvent(sA, s->evB[b], 0));     // stream B is done with this buffer set (group g - 2)
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[0], sA));
    if (band) NC_HIP(ctx, hipMemsetAsync(B.counts.p, 0, 64, sA));
    // ---- query windows
    WinArgs wa;
    wa.codes = s->pack.codes; wa.slot_off = s->rd.slot_off; wa.rd_start = s->rd.rd_start; wa.rd_end = s->rd.rd_end;
    wa.ev_off = s->rd.ev_off; wa.ev_pos = s->rd.ev_pos; wa.ev_len = s->rd.ev_len; wa.ins_off = s->rd.ins_off; wa.tail_off = s->rd.tail_off;
    wa.ins_bases = s->rd.ins_bases; wa.tail_bases = s->rd.tail_bases; wa.read_flag = s->rd.read_flag;
    wa.al_read = (const int32_t *)s->al_read.p + A0; wa.al_site = (const int32_t *)s->al_site.p + A0;
    wa.site_pos = (const int32_t *)s->site_pos.p; wa.site_n2 = (const int32_t *)s->site_n2.p;
    wa.al_ev = s->have_al_ev ? (const int2 *)s->al_ev.p + A0 : nullptr;
    wa.A = Ag; wa.W = s->window_after; wa.WS = WS; wa.win = (uint8_t *)B.win.p; wa.n1 = (int32_t *)B.n1.p;
    wa.cells = (unsigned long long *)(err() + 4);
    wa.band_lo = band ? (int8_t *)B.band_lo.p : nullptr;
    wa.wcls = band ? (int8_t *)B.band_lo.p + Agz + 64 : nullptr;
    wa.list1 = q.lists; wa.list2 = wa.list1 + Agz; wa.listF = wa.list2 + Agz;
    wa.counts = q.counts; wa.band_margin = margin;
    if (Ag > 0) nc_pipe_launch_windows(sA, wa, win_mode);
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[1], sA));
    // ---- star alignment: every read window against its site's reference window (free tail)
    FillArgs &fa = q.fa;
    fa.s1 = (const uint8_t *)B.win.p; fa.s1_stride = WS; fa.n1 = (const int32_t *)B.n1.p;
    fa.ref_code = s->ref_code; fa.ref_pos0 = s->ref_pos0; fa.site_pos = (const int32_t *)s->site_pos.p; fa.site_n2 = (const int32_t *)s->site_n2.p;
    fa.al_site = (const int32_t *)s->al_site.p + A0; fa.site0 = 0; fa.site_div = 1;
    fa.A = Ag; fa.W = W;
    fa.open = s->scoring[0]; fa.extend = s->scoring[1]; fa.match = s->scoring[2]; fa.mismatch = s->scoring[3];
    fa.arow = nullptr; fa.N1 = N1;
    fa.Tw = (uint32_t *)B.tw.p;
    fa.Hlast = (int32_t *)B.hlast.p; fa.hcol = (int32_t *)B.hcol.p; fa.endcell = (int2 *)B.endc.p;
    fa.list = nullptr; fa.count = nullptr;
    if (band && Ag > 0) {
        // every alignment on its band; the full matrix runs behind the banded traceback, over the third list (stage_b1)
        BandArgs &ba = q.ba;
        ba.f = fa;
        ba.list = nullptr; ba.count = nullptr;
        ba.band_lo = (const int8_t *)B.band_lo.p; ba.Twb = (uint32_t *)B.twb.p; ba.hrow = (int16_t *)B.hrow.p; ba.hcolb = (int16_t *)B.hcolb.p;
        ba.NBLK = nblk; ba.redo_list = wa.listF; ba.redo_count = wa.counts + 2; ba.edge = 0;
        nc_pipe_launch_fill_band(sA, band_class(q, 0), band_class(q, 1));
    } else if (Ag > 0) nc_pipe_launch_fill(sA, CPL, fa);
    NC_HIP(ctx, hipGetLastError());
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[2], sA));
    if (two) NC_HIP(ctx, hipEventRecord(s->evA[b], sA));
    return NC_OK;
}

// stream B: traceback + tensors + the row count of the allele alignments (left in the mailbox)
int PipeRun::stage_b1(const PipeGroup &q)
{
    const int b = q.g & 1, ng = q.k1 - q.k0;
    nc_pipe_state::GroupBufs &B = s->gb[b];
    if (two) NC_HIP(ctx, hipStreamWaitEvent(sB, s->evA[b], 0));
    if (band && q.Ag > 0) {
        nc_pipe_launch_trace_band(sB, band_class(q, 0), band_class(q, 1), (uint32_t *)B.trace.p, EW);
        // the rest on the full matrix: too wide for a band, or a path that touched the edge of its band
        FillArgs fl = q.fa;
        fl.list = q.ba.redo_list; fl.count = q.ba.redo_count;
        nc_pipe_launch_fill(sB, CPL, fl);
        nc_pipe_launch_trace(sB, fl, CPL, (uint32_t *)B.trace.p, EW);
        nc_pipe_launch_band_stats(sB, q.counts, (long long *)(err() + 16));
    } else if (q.Ag > 0) nc_pipe_launch_trace(sB, q.fa, CPL, (uint32_t *)B.trace.p, EW);
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[3], sB));
    // ---- columns, histogram, tensor, consensus
    TensorArgs ta;
    ta.site0 = q.k0; ta.n_sites_g = ng; ta.S = S; ta.haploid = s->haploid; ta.W = W; ta.WS = WS; ta.A0 = q.A0;
    ta.site_al0 = (const int32_t *)s->site_al0.p; ta.site_nr = (const int32_t *)s->site_nr.p; ta.site_pos = (const int32_t *)s->site_pos.p;
    ta.site_n2 = (const int32_t *)s->site_n2.p; ta.al_member = (const uint8_t *)s->al_member.p; ta.win = (const uint8_t *)B.win.p;
    ta.ent = (const uint32_t *)B.trace.p; ta.EW = EW; ta.ref_code = s->ref_code; ta.ref_pos0 = s->ref_pos0; ta.x = x_dev;
    ta.cns = (uint8_t *)B.cns.p; ta.ncns = (int32_t *)B.ncns.p; ta.cband = (int16_t *)B.cband.p; ta.err = err();
    nc_pipe_launch_site_tensor(sB, ta, s->maxcov > 255);
    if (timing) NC_HIP(ctx, hipEventRecord(s->ev[4], sB));
    int32_t *mbox = err() + 2;
    NC_TRY(nc_pipe_scan_twb(ctx, sB, s->part_b, (const int32_t *)B.ncns.p, ng * S, (int64_t *)B.arow.p, mbox));
    NC_HIP(ctx, hipGetLastError());
    NC_TRY(nc_d2h(ctx, ctx->mbox + 36, mbox, 8, sB));
    return NC_OK;
}

// stream B: allele_prediction, the global alignment of every consensus against its window (parasail scoring 9 / 1 / 20 / -10, :79)
int PipeRun::stage_b2(const PipeGroup &q, int64_t rows)
{
    nc_pipe_state::GroupBufs &B = s->gb[q.g & 1];
    const int nset = (q.k1 - q.k0) * S;
    // (a run of several groups sizes these for the largest group its bounds allow, like stage_a's buffers: no growth in the middle of a genome)
    const int64_t nset_cap = G > 1 ? std::max<int64_t>(nset, std::min<int64_t>(GROUP_SITES, ns) * S) : nset;
    const int64_t rows_cap = nset > 0 ? (rows * nset_cap + nset - 1) / nset : rows;
    NC_TRY(nc_ensure(ctx, s->tw2, (size_t)(rows_cap + 1) * 64 * CPL + 64));                 // `rows` counts blocks of TWB steps
    NC_TRY(nc_ensure(ctx, s->runs, (size_t)(TWB * rows_cap + nset_cap * (W + 1) + 2) * 4 + 64));
    FillArgs fb = q.fa;
    fb.s1 = (const uint8_t *)B.cns.p; fb.s1_stride = CNS_CAP; fb.n1 = (const int32_t *)B.ncns.p;
    fb.al_site = nullptr; fb.site0 = q.k0; fb.site_div = S;
    fb.A = nset;
    fb.open = 9; fb.extend = 1; fb.match = 20; fb.mismatch = -10;
    fb.arow = (const int64_t *)B.arow.p; fb.N1 = 0;
    fb.Tw = (uint32_t *)s->tw2.p; fb.Hlast = nullptr; fb.hcol = nullptr; fb.endcell = nullptr;
    fb.list = nullptr; fb.count = nullptr;
    const int32_t *site_type = (const int32_t *)s->site_type.p;
    int16_t *runs = (int16_t *)s->runs.p;
    int32_t *rl = (int32_t *)s->rlen.p + (size_t)q.k0 * S, *al = (int32_t *)s->alen.p + (size_t)q.k0 * S;
    BandArgs bb;
    memset(&bb, 0, sizeof bb);
    bb.f = fb;
    // allele_prediction is an exact global alignment in the reference (parasail nw_trace, generate_indel_pileups.py:79), and REF / ALT strings are row
    // a13's bit-exact output.  The banded form is therefore kept only where it PROVES itself: k_allele_trace_b12 compares the score of the path it
    // walked with the most any path outside the band can reach (allele_trace_body's certificate) and sends every set it cannot certify -- and every
    // path that touches an edge diagonal -- to the full matrix.  NC_PIPE_BAND_ALLELES=0: every consensus on the full matrix (+1.0 ms per chr20 pass).
    if (band && band_alleles) {
        // the consensus against its window on a band around the diagonals 0 .. n2 - n1; too long / too wide / edge-touching ones on the full matrix
        const size_t nz = (size_t)std::max(nset, 1), nzc = (size_t)std::max<int64_t>(nset_cap, 1);
        NC_TRY(nc_ensure(ctx, s->ab_lo, nzc + 64));
        NC_TRY(nc_ensure(ctx, s->ab_lists, nzc * 3 * 4 + 64));
        NC_TRY(nc_ensure(ctx, s->ab_counts, 64));
        NC_TRY(nc_ensure(ctx, s->ab_twb, nzc * (size_t)BAND_NBLK4 * (4 * TWB_PITCH) + 256));
        NC_HIP(ctx, hipMemsetAsync(s->ab_counts.p, 0, 64, sB));
        int32_t *l1 = (int32_t *)s->ab_lists.p, *l2 = l1 + nz, *lF = l2 + nz, *cn = (int32_t *)s->ab_counts.p;
        nc_pipe_launch_allele_classes(sB, fb, (const int16_t *)B.cband.p, margin, 8 * BAND_NBLK, (int8_t *)s->ab_lo.p, l1, l2, lF, cn);
        bb.band_lo = (const int8_t *)s->ab_lo.p; bb.Twb = (uint32_t *)s->ab_twb.p; bb.hrow = nullptr; bb.hcolb = nullptr; bb.NBLK = BAND_NBLK4;
        bb.redo_list = lF; bb.redo_count = cn + 2; bb.edge = 0;
        bb.list = l1; bb.count = cn;
        BandArgs bb2 = bb;
        bb2.list = l2; bb2.count = cn + 1;
        nc_pipe_launch_fill_band(sB, bb, bb2);
        nc_pipe_launch_allele_trace_band(sB, bb, bb2, CPL, site_type, s->win_size, runs, rl, al);
        fb.list = lF; fb.count = cn + 2;
        bb.f = fb;
    }
    nc_pipe_launch_fill(sB, CPL, fb);
    nc_pipe_launch_allele_trace(sB, bb, CPL, site_type, s->win_size, runs, rl, al);
    NC_TRY(nc_pipe_scan_pos(ctx, sB, s->part_b, (const int32_t *)al, nset, (int64_t *)B.alt_off.p, (long long *)(err() + 8)));
    nc_pipe_launch_alt_copy(sB, (const uint8_t *)B.cns.p, (const int32_t *)al, (const int64_t *)B.alt_off.p, nset, (uint8_t *)s->alt_pool.p, s->alt_pool_cap, err());
    NC_HIP(ctx, hipGetLastError());
    if (two) NC_HIP(ctx, hipEventRecord(s->evB[q.g & 1], sB));
    if (timing) {
        NC_HIP(ctx, hipEventRecord(s->ev[5], sB));
        NC_HIP(ctx, hipEventSynchronize(s->ev[5]));
        for (int st = 0; st < 5; st++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, s->ev[st], s->ev[st + 1]);
            s->stage_ms[st + 1] += ms;
        }
        s->cells[1] += TWB * rows * (int64_t)(s->window_after + 1);               // (upper estimate: whole blocks)
    }
    return NC_OK;
}

// NC_PIPE_DUMP (debugging aid): the run's arrays as files <dump>.<name> -- the per-site ones once, the per-alignment and per-set ones of every
// group appended in group order (a run's files cover all its alignments and sets).  Class bytes: 0 = 32 diagonals, 1 = 64, 2 = full matrix by
// width, 3 = full matrix after a banded try (an edge touch; for the allele alignments also a band without its certificate), -1 = band off
void PipeRun::dump_wr(int g, const char *name, const void *src, size_t bytes, bool on_host) const
{
    if (!src || !bytes) return;
    std::vector<char> h;
    if (!on_host) {
        h.resize(bytes);
        if (hipMemcpy(h.data(), src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return;
        src = h.data();
    }
    char path[512];
    snprintf(path, sizeof path, "%s.%s", dump, name);
    if (FILE *fp = fopen(path, g == 0 ? "wb" : "ab")) { fwrite(src, 1, bytes, fp); fclose(fp); }
}
// the class of every item from the three lists: a banded try that failed is listed in its band's list AND in the full matrix's
void PipeRun::dump_classes(int g, const char *name, int32_t n, const void *lists, size_t pitch, const void *counts, bool banded) const
{
    std::vector<int8_t> cls((size_t)std::max(n, 0), -1);
    if (banded && n > 0) {
        std::vector<int32_t> l(pitch * 3), c(4);
        if (hipMemcpy(l.data(), lists, pitch * 3 * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
        if (hipMemcpy(c.data(), counts, 16, hipMemcpyDeviceToHost) != hipSuccess) return;
        for (int k = 0; k < 3; k++)
            for (int32_t i = 0; i < std::min<int32_t>(c[k], (int32_t)pitch); i++) {
                const int32_t a = l[(size_t)k * pitch + i];
                if (a < 0 || a >= n) continue;
                int8_t &v = cls[(size_t)a];
                v = k < 2 ? (int8_t)k : v < 0 ? 2 : 3;
            }
    }
    dump_wr(g, name, cls.data(), cls.size(), true);
}
// behind stage_b1 (stream B drained): the group's alignments
void PipeRun::dump_b1(const PipeGroup &q) const
{
    const int g = q.g;
    const nc_pipe_state::GroupBufs &B = s->gb[g & 1];
    dump_wr(g, "trace", B.trace.p, (size_t)q.Ag * EW * 4, false);
    dump_wr(g, "win", B.win.p, (size_t)q.Ag * WS, false);
    dump_wr(g, "n1", B.n1.p, (size_t)q.Ag * 4, false);
    dump_wr(g, "al_site", (const int32_t *)s->al_site.p + q.A0, (size_t)q.Ag * 4, false);
    dump_wr(g, "al_read", (const int32_t *)s->al_read.p + q.A0, (size_t)q.Ag * 4, false);
    if (g == 0) {
        dump_wr(g, "site_pos", s->site_pos.p, (size_t)ns * 4, false);
        dump_wr(g, "site_n2", s->site_n2.p, (size_t)ns * 4, false);
    }
    if (band) dump_wr(g, "band_lo", B.band_lo.p, (size_t)q.Ag, false);
    dump_classes(g, "cls", q.Ag, B.lists.p, (size_t)std::max(q.Ag, 1), B.counts.p, band);
}
// behind stage_b2 (stream B drained): the allele stage's arrays of the group
void PipeRun::dump_b2(const PipeGroup &q) const
{
    const int g = q.g, nset = (q.k1 - q.k0) * S;
    const nc_pipe_state::GroupBufs &B = s->gb[g & 1];
    const bool ab = band && band_alleles;
    dump_wr(g, "cns", B.cns.p, (size_t)nset * CNS_CAP, false);
    dump_wr(g, "ncns", B.ncns.p, (size_t)nset * 4, false);
    dump_wr(g, "rlen", (const int32_t *)s->rlen.p + (size_t)q.k0 * S, (size_t)nset * 4, false);
    dump_wr(g, "alen", (const int32_t *)s->alen.p + (size_t)q.k0 * S, (size_t)nset * 4, false);
    if (ab) {
        dump_wr(g, "ab_lo", s->ab_lo.p, (size_t)nset, false);
        dump_wr(g, "ab_counts", s->ab_counts.p, 16, false);
    }
    dump_classes(g, "ab_cls", nset, s->ab_lists.p, (size_t)std::max(nset, 1), s->ab_counts.p, ab);
}

extern "C" int nc_indel_sites_run(nc_ctx *ctx, float *x_dev)
{
    if (!ctx) return NC_ERR_ARG;
    nc_pipe_state *s = ctx->pipe;
    if (!s || !s->planned) return nc_fail(ctx, NC_ERR_STATE, "nc_indel_sites_run: nc_indel_sites_plan first");
    s->ran = true;
    if (s->n_sites == 0) return NC_OK;
    if (!x_dev) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_run: x_dev");
    NC_HIP(ctx, hipSetDevice(ctx->device));
    PipeRun r;
    r.ctx = ctx; r.s = s; r.x_dev = x_dev;
    r.timing = ctx->timing == 1;
    const int S = r.S = s->S, ns = r.ns = s->n_sites;
    r.W = s->window_after + 2;                                     // n2 <= window_after + 1; row pitch n2 + 1
    r.EW = (r.W + 15) & ~15;
    r.WS = (s->window_after + 15) & ~15;
    r.N1 = r.WS;
    r.CPL = cpl_for(s->window_after + 1);
    // the environment's switches, read once per run (tests switch them between runs)
    r.dump = getenv("NC_PIPE_DUMP");
    const char *bae = getenv("NC_PIPE_BAND_ALLELES"), *wm = getenv("NC_PIPE_WINDOWS");
    r.band_alleles = !(bae && atoi(bae) == 0);
    // NC_PIPE_WINDOWS = serial: one lane per window (k_windows); force16: the 16-lane kernel with every window on its serial route
    r.win_mode = wm && !strcmp(wm, "serial") ? NC_WIN_SERIAL : wm && !strcmp(wm, "force16") ? NC_WIN_FORCE16 : NC_WIN_16;
    r.margin = s->band_margin_v > 0 ? s->band_margin_v : band_margin();
    r.nblk = (((r.N1 + r.W + 7) / 8) + 3) & ~3;                      // blocks of 8 anti-diagonals of a banded alignment: n1 + n2 <= N1 + W (41 for the 160-base windows, 66 for the 260-base ones)
    r.band = (s->band_mode < 0 ? band_on() : s->band_mode != 0) && r.nblk <= 80;
    // groups of whole sites, two in flight: the traceback codes of a group's alignments (16 KB each for 160-base windows) take a twelfth of
    // the device memory that is free when the context first runs, at most 24 GiB (a chr20-sized contig's 1.07 M alignments are then ONE group:
    // 24.4 -> 23.7 ms per pass against three groups of 6 GiB -- fewer launches and host waits, no allele stage with stream A idle); at least 1 GiB
    r.tw_per_al = (int64_t)tw_blocks(r.N1) * 64 * r.CPL;          // bytes: blocks of 8 steps x 16 lanes x CPL words
    if (s->tw_budget == 0) {
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) mfree = (size_t)72 << 30;
        s->tw_budget = std::min<int64_t>((int64_t)24 << 30, std::max<int64_t>((int64_t)1 << 30, (int64_t)(mfree / 12)));
    }
    int64_t GROUP_AL = std::max<int64_t>(4096, s->tw_budget / r.tw_per_al);
    if (const char *g = getenv("NC_PIPE_GROUP_AL")) GROUP_AL = std::max<int64_t>(64, atoll(g));
    const int64_t GROUP_SITES = 65536;
    r.GROUP_AL = GROUP_AL; r.GROUP_SITES = GROUP_SITES;
    // ALT pool: generous (most ALT alleles are a few dozen bases); an overflow is reported, not silent
    s->alt_pool_cap = std::max<int64_t>((int64_t)1 << 20, (int64_t)ns * S * 160);
    NC_TRY(nc_ensure(ctx, s->alt_pool, (size_t)s->alt_pool_cap));
    NC_TRY(nc_ensure(ctx, s->rlen, (size_t)ns * S * 4));
    NC_TRY(nc_ensure(ctx, s->alen, (size_t)ns * S * 4));
    const int32_t *al0h = r.al0h = s->al0_pin;
    std::vector<std::pair<int, int>> groups;
    {
        // as many groups as the bounds need, of about the same number of alignments each (filled greedily the last one is a remainder)
        const int64_t total_al = al0h[ns];
        const int64_t ng = std::max<int64_t>(std::max<int64_t>(1, (total_al + GROUP_AL - 1) / GROUP_AL), (ns + GROUP_SITES - 1) / GROUP_SITES);
        const int64_t target = std::min<int64_t>(GROUP_AL, (total_al + ng - 1) / ng + 64);
        for (int k0 = 0; k0 < ns;) {
            int k1 = k0 + 1;
            while (k1 < ns && k1 - k0 < GROUP_SITES && (int64_t)al0h[k1 + 1] - al0h[k0] <= target) k1++;
            groups.emplace_back(k0, k1);
            k0 = k1;
        }
    }
    const int G = r.G = (int)groups.size();
    // A contig with more alignments than one group holds is cut into groups of about the same size, each smaller than GROUP_AL; a later, slightly
    // shorter contig may then arrive as ONE group of nearly GROUP_AL alignments -- larger than any group before it.  Sized by their own group, the
    // per-alignment buffers then grew in the middle of a whole-genome pass (hipFree + hipMalloc of ~9 GB: a second of idle GPU at chr18 after
    // chr1 .. chr17).  A run of several groups therefore sizes them for GROUP_AL at once; a run of one group takes what it needs.
    r.Acap = G > 1 ? (size_t)std::min<int64_t>(GROUP_AL, al0h[ns]) + 64 : 0;
    // Stream A (the context's): query windows + alignment fill (bound by vector issue).  Stream B: traceback, tensors, allele_prediction
    // (bound by memory latency) of the previous group, beside it on the same CUs.  Stage timers (timing mode) need the stages one
    // after the other: one stream then.
    const bool timing = r.timing, two = r.two = !timing && G > 1;
    if (two && !s->sB) {
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        // high priority: its latency-bound kernels take the wave slots the issue-bound fill leaves free as soon as they open
        NC_HIP(ctx, hipStreamCreateWithPriority(&s->sB, hipStreamNonBlocking, prio_hi));
        for (auto &e : s->evA) NC_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : s->evB) NC_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        NC_HIP(ctx, hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
    }
    const hipStream_t sA = r.sA = ctx->stream, sB = r.sB = two ? s->sB : ctx->stream;
    if (two) {                                                         // B starts behind the plan's kernels
        NC_HIP(ctx, hipEventRecord(s->ev_join, sA));
        NC_HIP(ctx, hipStreamWaitEvent(sB, s->ev_join, 0));
    }
    auto stage_a = [&](int g) { return r.stage_a(g, groups[(size_t)g].first, groups[(size_t)g].second); };
    NC_TRY(stage_a(0));
    for (int g = 0; g < G; g++) {
        if (!timing && g + 1 < G) NC_TRY(stage_a(g + 1));            // the next group's alignments are enqueued before the host waits for this one's row count
        const PipeGroup &q = r.grp[g & 1];
        NC_TRY(r.stage_b1(q));
        volatile int32_t *mb = ctx->mbox + 36;
        NC_HIP(ctx, hipStreamSynchronize(sB));
        if (r.dump) r.dump_b1(q);
        const int64_t rows = ((int64_t)mb[1] << 31) | (int64_t)(mb[0] & 0x7fffffff);
        NC_TRY(r.stage_b2(q, rows));
        if (r.dump) {
            NC_HIP(ctx, hipStreamSynchronize(sB));
            r.dump_b2(q);
        }
        if (timing && g + 1 < G) NC_TRY(stage_a(g + 1));
    }
    if (two) {                                                         // the caller's stream continues behind stream B
        NC_HIP(ctx, hipEventRecord(s->ev_join, sB));
        NC_HIP(ctx, hipStreamWaitEvent(sA, s->ev_join, 0));
    }
    return NC_OK;
}

extern "C" int nc_indel_sites_fetch(nc_ctx *ctx, int32_t *pos, int32_t *chunk, int32_t *var_type, int32_t *phase, int32_t *ref_len,
                                    int32_t *alt_len, int64_t *n_alt_bytes)
{
    if (!ctx) return NC_ERR_ARG;
    nc_pipe_state *s = ctx->pipe;
    if (!s || !s->planned) return nc_fail(ctx, NC_ERR_STATE, "nc_indel_sites_fetch: nc_indel_sites_plan first");
    if (n_alt_bytes) *n_alt_bytes = 0;
    if (s->n_sites == 0) return NC_OK;
    const size_t NS = (size_t)s->n_sites;
    auto cp = [&](void *dst, const DevBuf &b, size_t bytes) -> int {
        if (dst) NC_HIP(ctx, hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return NC_OK;
    };
    NC_TRY(cp(pos, s->site_pos, NS * 4));
    NC_TRY(cp(chunk, s->site_chunk, NS * 4));
    NC_TRY(cp(var_type, s->site_type, NS * 4));
    NC_TRY(cp(phase, s->site_phase, NS * 4));
    int32_t misc[32] = {0};
    if (s->ran) {
        NC_TRY(cp(ref_len, s->rlen, NS * s->S * 4));
        NC_TRY(cp(alt_len, s->alen, NS * s->S * 4));
    }
    NC_HIP(ctx, hipMemcpyAsync(misc, s->misc.p, sizeof misc, hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (misc[0] & 2) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites: a read set needs more than %d alignment columns", CNS_CAP);
    if (misc[0] & 4) return nc_fail(ctx, NC_ERR_CAPACITY, "nc_indel_sites: ALT allele pool overflow");
    long long cells = 0, pool = 0;
    memcpy(&cells, misc + 4, 8);
    memcpy(&pool, misc + 8, 8);
    memcpy(s->band_stats, misc + 16, 32);
    memcpy(s->band_stats + 4, misc + 6, 8);
    s->cells[0] = cells;
    if (n_alt_bytes) *n_alt_bytes = pool;
    return NC_OK;
}

extern "C" int nc_indel_sites_fetch_alt(nc_ctx *ctx, uint8_t *alt_bases, int64_t cap)
{
    if (!ctx) return NC_ERR_ARG;
    nc_pipe_state *s = ctx->pipe;
    if (!s || !s->ran) return nc_fail(ctx, NC_ERR_STATE, "nc_indel_sites_fetch_alt: nc_indel_sites_run first");
    if (cap <= 0 || s->n_sites == 0) return NC_OK;
    if (!alt_bases) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_fetch_alt: null buffer");
    NC_HIP(ctx, hipMemcpyAsync(alt_bases, s->alt_pool.p, (size_t)std::min<int64_t>(cap, s->alt_pool_cap), hipMemcpyDeviceToHost, ctx->stream));
    NC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NC_OK;
}

extern "C" int nc_indel_sites_band(nc_ctx *ctx, int32_t mode, int32_t margin)
{
    if (!ctx || mode < -1 || mode > 1 || margin < 0 || margin > 15) return nc_fail(ctx, NC_ERR_ARG, "nc_indel_sites_band: mode -1 / 0 / 1, margin 0 (default) .. 15");
    if (!ctx->pipe) ctx->pipe = new (std::nothrow) nc_pipe_state();
    if (!ctx->pipe) return NC_ERR_NOMEM;
    ctx->pipe->band_mode = mode;
    ctx->pipe->band_margin_v = margin;
    return NC_OK;
}

extern "C" int nc_indel_sites_band_stats(nc_ctx *ctx, int64_t *stats6)
{
    if (!ctx || !ctx->pipe || !stats6) return NC_ERR_ARG;
    for (int k = 0; k < 6; k++) stats6[k] = ctx->pipe->band_stats[k];
    return NC_OK;
}

extern "C" int nc_indel_sites_stage_ms(nc_ctx *ctx, float *ms6, int64_t *cells2)
{
    if (!ctx || !ctx->pipe) return NC_ERR_ARG;
    if (ms6) for (int k = 0; k < 6; k++) ms6[k] = ctx->pipe->stage_ms[k];
    if (cells2) { cells2[0] = ctx->pipe->cells[0]; cells2[1] = ctx->pipe->cells[1]; }
    return NC_OK;
}

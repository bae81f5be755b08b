// decode.hip — host side of the decoder: the workspace layout, the stage sequence of a
// decode (decode_heads) and the pp_decode_* entry points.  The kernels and their
// launchers are in seed_loop.hip, seed_loop_ext.hip, complete.hip and nms.hip.
#include "grow_args.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <mutex>

// ---------------------------------------------------------------------------------------
// host: workspace layout + pp_decode_batch
// ---------------------------------------------------------------------------------------
namespace pp {

int launch_seeds(const Heads &h, const HrMap &hr, int n_img, int K, const pp_config *cfg,
                 pp_seed *seeds, int cap, int *counts, void *scratch, hipStream_t s,
                 bool emitted, const int32_t *ext);
size_t seeds_scratch_size(int n_img, int cap);
int launch_caf_bucketed(const Heads &h, const HrMap &hr, int n_img, int K, int C,
                        const int32_t *skeleton, const pp_config *cfg, float th, float *cols,
                        int *offs, const int *gate, bool index_only, hipStream_t s,
                        const int32_t *ext);
void caf_bucket_grid(int H, int W, int stride, int *bw, int *bh, int *nb, float *inv_e);

// the decoder's kernels, each launched from the file that defines it (seed_loop.hip,
// seed_loop_ext.hip, complete.hip, nms.hip)
// (ext: NULL, or a ragged batch's extent table, hr_dims)
int launch_seed_loop(const GrowArgs &g, int n_img, hipStream_t s, const int32_t *ext);
int launch_seed_loop_ext(const GrowArgs &g, int n_img, hipStream_t s, const int32_t *ext);
int launch_complete(const GrowArgs &g, int n_img, int ways, hipStream_t s, const int32_t *ext);
int launch_nms(const GrowArgs &g, int n_img, bool wide, bool bitmap, hipStream_t s);

struct DecodeLayout {
    int hh, ww;
    int64_t pitch, hw;
    int seed_cap, ann_cap, ann_np, log_cap;
    int bw, bh, nb;
    float inv_e;
    int64_t occ_cap;
    size_t off_cifhr, off_hr_aux, off_hr_masks, off_cifhr_ws, off_seeds, off_seed_counts, off_seed_ws, off_cols[2],
        off_offs[2], off_n_work, off_need, off_occ, off_wq, off_log, off_work, off_spec, off_xext, off_xrec, off_nms_score,
        off_nms_idx, off_nms_f, off_nms_box, total;
    size_t cifhr_ws_bytes;
};

// CifHr map from head 0 (cif_hr.py:46-51); column sets and seeds over the cells of all heads
static DecodeLayout make_layout(int n_img, int K, int C, const Heads &h, const pp_config *cfg,
                                int ann_cap) {
    DecodeLayout d{};
    d.hh = h.hr_hh;
    d.ww = h.hr_ww;
    d.pitch = pp_cifhr_pitch(d.ww);
    d.hw = h.caf_cells();
    d.seed_cap = (int)(K * h.cif_cells());  // every cell of every field: no seed overflow
    d.ann_cap = ann_cap;
    d.ann_np = 1;
    while (d.ann_np < ann_cap) d.ann_np <<= 1;
    d.log_cap = K * ann_cap;
    const int64_t oh = (int64_t)((double)d.hh / cfg->occupancy_reduction);
    const int64_t ow = (int64_t)((double)d.ww / cfg->occupancy_reduction);
    d.occ_cap = (int64_t)align_up((size_t)(K * (oh + kOccMargin) * ((ow + kOccMargin + 15) & ~15)));
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes);
        return at;
    };
    const size_t n = (size_t)n_img;
    // scratch CifHr, block-sparse (HrMap with masks): 64x64 tiles of 8x8 blocks
    const HrMap geo = dense_hr(nullptr, d.hh, d.ww);
    d.off_cifhr = take(n * K * (size_t)geo.tiles * kHrTile * kHrTile * sizeof(float));
    d.off_hr_aux = take(h.n_groups > 1 ? n * K * (size_t)geo.tiles * kHrTile * kHrTile * sizeof(float) : 0);
    d.off_hr_masks = take(n * K * (size_t)geo.tiles * sizeof(uint64_t));
    d.cifhr_ws_bytes = std::max(cifhr_heads_workspace_size(h, n_img, K),
                                cifhr_sparse_workspace_size(h, n_img, K));
    d.off_cifhr_ws = take(d.cifhr_ws_bytes);
    d.off_seeds = take(n * d.seed_cap * sizeof(pp_seed));
    d.off_seed_counts = take(n * sizeof(int));
    d.off_seed_ws = take(seeds_scratch_size(n_img, d.seed_cap));
    caf_bucket_grid(h.cH[0], h.cW[0], h.cstride[0], &d.bw, &d.bh, &d.nb, &d.inv_e);
    for (int t = 0; t < 2; t++) {
        const bool used = t == 0 || cfg->force_complete;
        d.off_cols[t] = take(used ? n * C * 2 * (t ? 1 : kColRows) * d.hw * sizeof(float) : 0);
        d.off_offs[t] = take(used ? n * C * 2 * (d.nb + 1) * sizeof(int) : 0);
    }
    d.off_n_work = take(n * sizeof(int));
    d.off_need = take(n * sizeof(int));
    d.off_occ = take(n * d.occ_cap);  // zero region from here (pp_decode_workspace_zero_offset)
    d.off_wq = take(n * sizeof(int));
    d.off_log = take(n * d.log_cap * sizeof(OccLog));
    d.off_work = take(n * ann_cap * sizeof(pp_ann));
    d.off_spec = take(n * kSpecCache * sizeof(pp_ann));
    d.off_xext = take(n * sizeof(SeedExt));
    d.off_xrec = take(n * kExtCache * sizeof(pp_ann));
    d.off_nms_score = take(n * 2 * ann_cap * sizeof(double));
    d.off_nms_idx = take(n * (4 * ann_cap + d.ann_np) * sizeof(int));
    d.off_nms_f = take(n * 2 * ann_cap * sizeof(float));
    d.off_nms_box = take(n * kNmsBoxLists * ann_cap * sizeof(int2));
    d.total = o;
    return d;
}

}  // namespace pp

using namespace pp;

extern "C" {

// The layout behind the six size / offset entry points, all zero for arguments outside the
// envelope.  min_img: 0 for the sizes (an empty batch has an empty workspace), 1 for the
// offsets (which return 0 for it).
static DecodeLayout layout_single(int min_img, int32_t n_img, int32_t K, int32_t C, int32_t H,
                                  int32_t W, const pp_config *cfg, int32_t ann_capacity) {
    if (!cfg || n_img < min_img || K <= 0 || C <= 0 || H <= 0 || W <= 0 || ann_capacity <= 0 ||
        cfg->stride <= 0)
        return DecodeLayout{};
    return make_layout(n_img, K, C, single_head(nullptr, nullptr, H, W, cfg->stride), cfg,
                       ann_capacity);
}

static DecodeLayout layout_multi(const char *who, int min_img, const pp_scale *scales,
                                 int32_t n_scales, int32_t cif_pairs, int32_t n_img, int32_t K,
                                 int32_t C, const pp_config *cfg, int32_t ann_capacity) {
    Heads h;
    if (!cfg || make_heads(scales, n_scales, cif_pairs, 3, &h, who) || n_img < min_img || K <= 0 ||
        C <= 0 || ann_capacity <= 0)
        return DecodeLayout{};
    return make_layout(n_img, K, C, h, cfg, ann_capacity);
}

size_t pp_decode_workspace_size(int32_t n_img, int32_t K, int32_t C, int32_t H, int32_t W,
                                const pp_config *cfg, int32_t ann_capacity) {
    return layout_single(0, n_img, K, C, H, W, cfg, ann_capacity).total;
}

size_t pp_decode_workspace_zero_offset(int32_t n_img, int32_t K, int32_t C, int32_t H, int32_t W,
                                       const pp_config *cfg, int32_t ann_capacity) {
    return layout_single(1, n_img, K, C, H, W, cfg, ann_capacity).off_occ;
}

size_t pp_decode_work_offset(int32_t n_img, int32_t K, int32_t C, int32_t H, int32_t W,
                             const pp_config *cfg, int32_t ann_capacity) {
    return layout_single(1, n_img, K, C, H, W, cfg, ann_capacity).off_work;
}

size_t pp_decode_multi_work_offset(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                                   int32_t n_img, int32_t K, int32_t C, const pp_config *cfg,
                                   int32_t ann_capacity) {
    return layout_multi("pp_decode_multi_work_offset", 1, scales, n_scales, cif_pairs, n_img, K,
                        C, cfg, ann_capacity).off_work;
}

size_t pp_decode_multi_workspace_size(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                                      int32_t n_img, int32_t K, int32_t C, const pp_config *cfg,
                                      int32_t ann_capacity) {
    return layout_multi("pp_decode_multi_workspace_size", 0, scales, n_scales, cif_pairs, n_img,
                        K, C, cfg, ann_capacity).total;
}

size_t pp_decode_multi_workspace_zero_offset(const pp_scale *scales, int32_t n_scales,
                                             int32_t cif_pairs, int32_t n_img, int32_t K,
                                             int32_t C, const pp_config *cfg,
                                             int32_t ann_capacity) {
    return layout_multi("pp_decode_multi_workspace_zero_offset", 1, scales, n_scales, cif_pairs,
                        n_img, K, C, cfg, ann_capacity).off_occ;
}

}  // extern "C"

namespace pp {

// One non-blocking side stream (+ fork / join events) per device, created on first use;
// the mutex keeps concurrent host threads' fork / join pairs from interleaving.
struct SideStream {
    hipStream_t stream;
    hipEvent_t fork, join;
    mutable std::mutex mu;
};

static const SideStream *side_stream() {
    static std::mutex create_mu;
    static SideStream *per_dev[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(create_mu);
    if (!per_dev[dev]) {
        SideStream *ss = new SideStream();
        if (hipStreamCreateWithFlags(&ss->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ss->fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ss->join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            delete ss;
            return nullptr;
        }
        per_dev[dev] = ss;
    }
    return per_dev[dev];
}

// External helper workgroups per image for the seed loop: enough to give every CU a seed
// loop workgroup when the batch has fewer images than CUs (at most kExtWgMax).
static int seed_ext_per_image(int n_img) {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (cus[dev] <= 0 &&
        hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        (void)hipGetLastError();
        cus[dev] = 0;
    }
    if (n_img <= 0 || cus[dev] <= 0) return 0;
    return std::max(0, std::min(kExtWgMax, cus[dev] / n_img - 1));
}

// Force-complete workgroups per image.  The workgroups pull annotations from a per-image
// counter, so any count gives the same result; 8 or 16 for sparse batches measured no
// better than 64 (round 5).
static int complete_ways(uint32_t) { return kCompleteWays; }


// optional inputs of pp_decode_initial
struct DecodeInit {
    const pp_ann *anns = nullptr;
    const int32_t *counts = nullptr;
    int32_t cap = 0;
    int32_t *out_index = nullptr;
    // pp_decode_ragged: the images' own field sizes, device (n_img, 2) (hr_dims)
    const int32_t *extents = nullptr;
};

static int decode_heads(const Heads &h, int32_t n_img, int32_t K, int32_t C,
                        const int32_t *skeleton, const pp_config *cfg, float *d_cifhr,
                        pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                        int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                        uint32_t stages, void *stream, const DecodeInit &init = DecodeInit{}) {
    if (!skeleton || !cfg || !d_anns || !d_counts || !d_status || !d_workspace)
        return fail(PP_EINVAL, "pp_decode_batch: NULL argument");
    for (int m = 0; m < h.n_cif; m++)
        if (!h.cif[m]) return fail(PP_EINVAL, "pp_decode_batch: NULL CIF field");
    for (int m = 0; m < h.n_caf; m++)
        if (!h.caf[m]) return fail(PP_EINVAL, "pp_decode_batch: NULL CAF field");
    if (n_img < 0 || K <= 0 || K > PP_MAX_KP || C <= 0 || C > PP_MAX_EDGES ||
        ann_capacity <= 0 || cfg->occupancy_reduction <= 0)
        return fail(PP_ESHAPE, "pp_decode_batch: shape outside the supported envelope "
                               "(K <= PP_MAX_KP, C <= PP_MAX_EDGES)");
    if (cfg->connection_method != 0 && cfg->connection_method != 1)
        return fail(PP_EINVAL, "connection method not known");
    for (int i = 0; i < 2 * C; i++)
        if (skeleton[i] < 1 || skeleton[i] > K)
            return fail(PP_EINVAL, "pp_decode_batch: skeleton joint index out of 1..K");
    if ((int64_t)K * h.cif_cells() > INT32_MAX || h.caf_cells() > INT32_MAX)
        return fail(PP_ESHAPE, "pp_decode_batch: fields too large");
    if (n_img == 0) return PP_OK;
    const DecodeLayout d = make_layout(n_img, K, C, h, cfg, ann_capacity);
    if (workspace_bytes < d.total) return fail(PP_ENOMEM, "pp_decode_batch: workspace too small");
    if ((int64_t)d.hh >= kMaxHrSide || (int64_t)d.ww >= kMaxHrSide)
        return fail(PP_ESHAPE, "pp_decode_batch: field too large (CifHr map of 32768 px or "
                               "more per side)");
    char *ws = (char *)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    const int32_t *ext = init.extents;
    // the caller's d_cifhr gets the dense map; otherwise the decoder keeps the block-sparse
    // scratch map, written only where splat boxes land
    float *hr_base = d_cifhr ? d_cifhr : (float *)(ws + d.off_cifhr);
    uint64_t *hr_masks = d_cifhr ? nullptr : (uint64_t *)(ws + d.off_hr_masks);
    HrMap hr = dense_hr(hr_base, d.hh, d.ww);
    hr.masks = hr_masks;
    pp_seed *seeds = (pp_seed *)(ws + d.off_seeds);
    int *seed_counts = (int *)(ws + d.off_seed_counts);
    float *cols[2] = {(float *)(ws + d.off_cols[0]), (float *)(ws + d.off_cols[1])};
    int *offs[2] = {(int *)(ws + d.off_offs[0]), (int *)(ws + d.off_offs[1])};
    int rc = PP_OK;
    // PP_STAGE_COMPLETE_SETS_EARLY with stage 1 (and without 8): the force-complete sets read
    // only the CAF fields, so they start on the side stream before the CifHr map, and a later
    // call's side-stream join (stages 2 | 4) covers them
    const bool b_first = (stages & PP_STAGE_COMPLETE_SETS_EARLY) && (stages & 1u) &&
                         !(stages & 8u) && cfg->force_complete;
    if (b_first) {
        const SideStream *side = side_stream();
        if (!side) return fail(PP_EHIP, "pp_decode_stages: no side stream for stage 16");
        std::lock_guard<std::mutex> lock(side->mu);
        if (hipEventRecord(side->fork, s) != hipSuccess ||
            hipStreamWaitEvent(side->stream, side->fork, 0) != hipSuccess)
            return fail(PP_EHIP, "pp_decode_batch: side-stream fork failed");
        rc = launch_caf_bucketed(h, hr, n_img, K, C, skeleton, cfg, cfg->complete_caf_threshold,
                                 cols[1], offs[1], nullptr, true, side->stream, ext);
        if (rc) {
            (void)hipEventRecord(side->join, side->stream);
            (void)hipStreamWaitEvent(s, side->join, 0);
            return rc;
        }
    }
    // the block-sparse map's kernel emits the seeds too when it can (stage 1 then writes
    // what seeds_emit_kernel would; stage 2 sorts them): the same test in both stages
    const bool fused_seeds = !d_cifhr && cifhr_fuses_seeds(h, n_img, K, cfg);
    if (stages & 1u) {
        if (d_cifhr) {
            rc = cifhr_heads_launch<false>(h, n_img, K, cfg, d_cifhr, ws + d.off_cifhr_ws,
                                           d.cifhr_ws_bytes, s, "pp_decode_batch(cifhr)");
        } else {
            const SeedSink sink = seed_sink(n_img, K, cfg, d.seed_cap, ws + d.off_seed_ws);
            rc = cifhr_sparse_launch(h, n_img, K, cfg, hr_base, (float *)(ws + d.off_hr_aux),
                                     hr_masks, ws + d.off_cifhr_ws, d.cifhr_ws_bytes, s,
                                     "pp_decode_batch(cifhr)", fused_seeds ? &sink : nullptr, ext);
        }
        if (rc) return rc;
    }
    // CifSeeds and CafScored both read only the fields and the CifHr map: with both stages
    // requested, CafScored runs on a side stream beside the seeds (fork / join events)
    // PP_STAGE_COMPLETE_SETS_EARLY: the force-complete sets (every field and direction) with
    // CafScored instead of gated after the seed loop
    const bool early_b = (stages & PP_STAGE_COMPLETE_SETS_EARLY) && (stages & 4u) &&
                         !(stages & 1u) && cfg->force_complete;
    const SideStream *side = (stages & 6u) == 6u ? side_stream() : nullptr;
    if (side) {
        std::lock_guard<std::mutex> lock(side->mu);
        if (hipEventRecord(side->fork, s) != hipSuccess ||
            hipStreamWaitEvent(side->stream, side->fork, 0) != hipSuccess)
            return fail(PP_EHIP, "pp_decode_batch: side-stream fork failed");
        rc = launch_caf_bucketed(h, hr, n_img, K, C, skeleton, cfg, cfg->caf_threshold, cols[0],
                                 offs[0], nullptr, false, side->stream, ext);
        if (!rc && early_b)
            rc = launch_caf_bucketed(h, hr, n_img, K, C, skeleton, cfg,
                                     cfg->complete_caf_threshold, cols[1], offs[1], nullptr, true,
                                     side->stream, ext);
        if (!rc)
            rc = launch_seeds(h, hr, n_img, K, cfg, seeds, d.seed_cap, seed_counts,
                              ws + d.off_seed_ws, s, fused_seeds, ext);
        // join even after a failed launch, so the caller's stream never runs ahead
        if (hipEventRecord(side->join, side->stream) != hipSuccess ||
            hipStreamWaitEvent(s, side->join, 0) != hipSuccess)
            return fail(PP_EHIP, "pp_decode_batch: side-stream join failed");
        if (rc) return rc;
    } else {
        if (stages & 2u) {
            rc = launch_seeds(h, hr, n_img, K, cfg, seeds, d.seed_cap, seed_counts,
                              ws + d.off_seed_ws, s, fused_seeds, ext);
            if (rc) return rc;
        }
        if (stages & 4u) {  // CafScored at caf_threshold; the force-complete set is lazy
            rc = launch_caf_bucketed(h, hr, n_img, K, C, skeleton, cfg, cfg->caf_threshold,
                                     cols[0], offs[0], nullptr, false, s, ext);
            if (!rc && early_b)
                rc = launch_caf_bucketed(h, hr, n_img, K, C, skeleton, cfg,
                                         cfg->complete_caf_threshold, cols[1], offs[1], nullptr,
                                         true, s, ext);
            if (rc) return rc;
        }
    }
    if (stages & 8u) {
        GrowArgs g{};
        g.seeds = seeds;
        g.seed_counts = seed_counts;
        g.seed_cap = d.seed_cap;
        g.cols[0] = cols[0];
        g.cols[1] = cols[1];
        g.offs[0] = offs[0];
        g.offs[1] = offs[1];
        g.bw = d.bw;
        g.bh = d.bh;
        g.nb = d.nb;
        g.inv_e = d.inv_e;
        g.K = K;
        g.C = C;
        g.hh = d.hh;
        g.ww = d.ww;
        g.col_cap = d.hw;
        g.cfg = *cfg;
        g.nms_it = (double)cfg->nms_instance_threshold;
        g.heads = h;
        g.hr = hr;
        g.cif_floor = cfg->cif_floor;
        g.one_minus_floor = (float)(1.0 - (double)cfg->cif_floor);  // (1.0 - self.cif_floor)
        g.th_b = cfg->complete_caf_threshold;
        for (int ci = 0; ci < C; ci++) {
            g.caf_j1[ci] = (uint8_t)(skeleton[2 * ci] - 1);
            g.caf_j2[ci] = (uint8_t)(skeleton[2 * ci + 1] - 1);
        }
        // by_source (cifcaf.py:62-65): dict insertion order, later duplicate keys
        // overwrite the value in place; flattened into directed-edge slots per start joint
        {
            int nbs[kKP] = {0};
            int bk[kKP][kKP], bc[kKP][kKP], bf[kKP][kKP];
            for (int ci = 0; ci < C; ci++) {
                const int j1 = skeleton[2 * ci] - 1, j2 = skeleton[2 * ci + 1] - 1;
                const int ins[2][3] = {{j1, j2, 1}, {j2, j1, 0}};
                for (int t = 0; t < 2; t++) {
                    const int st = ins[t][0];
                    int pos = -1;
                    for (int e = 0; e < nbs[st]; e++)
                        if (bk[st][e] == ins[t][1]) pos = e;
                    if (pos < 0) pos = nbs[st]++;
                    bk[st][pos] = ins[t][1];
                    bc[st][pos] = ci;
                    bf[st][pos] = ins[t][2];
                }
            }
            int d = 0;
            for (int j = 0; j < K; j++) {
                g.j_off[j] = (uint8_t)d;
                for (int e = 0; e < nbs[j]; e++, d++) {
                    g.d_j[d] = (uint8_t)j;
                    g.d_k[d] = (uint8_t)bk[j][e];
                    g.d_caf[d] = (uint8_t)bc[j][e];
                    g.d_fwd[d] = (uint8_t)bf[j][e];
                }
            }
            g.j_off[K] = (uint8_t)d;
            g.nd = d;
            g.has_cs = cfg->confidence_scales != nullptr;
            for (int e = 0; e < kSlots; e++)
                g.slot_cs[e] = (g.has_cs && e < d) ? cfg->confidence_scales[g.d_caf[e]] : 1.0f;
        }
        g.occ = (uint8_t *)(ws + d.off_occ);
        g.occ_cap = d.occ_cap;
        g.log = (OccLog *)(ws + d.off_log);
        g.log_cap = d.log_cap;
        g.work = (pp_ann *)(ws + d.off_work);
        g.spec = (pp_ann *)(ws + d.off_spec);
        g.spec_far = kSpecFar;
        g.n_ext = seed_ext_per_image(n_img);
        g.xext = (SeedExt *)(ws + d.off_xext);
        g.xrec = (pp_ann *)(ws + d.off_xrec);
        g.nms_score = (double *)(ws + d.off_nms_score);
        g.nms_idx = (int *)(ws + d.off_nms_idx);
        g.nms_f = (float *)(ws + d.off_nms_f);
        g.nms_box = (int2 *)(ws + d.off_nms_box);
        g.ann_np = d.ann_np;
        g.ann_cap = ann_capacity;
        g.stamps = nullptr;
#ifdef PP_STAMPS
        hipMalloc((void **)&g.stamps, (size_t)n_img * 3 * kStampSlots * sizeof(uint64_t));
        hipMemsetAsync(g.stamps, 0, (size_t)n_img * 3 * kStampSlots * sizeof(uint64_t), s);
        uint64_t *gcs = nullptr;
        hipMalloc((void **)&gcs, (size_t)n_img * 4 * sizeof(uint64_t));
        hipMemsetAsync(gcs, 0, (size_t)n_img * 4 * sizeof(uint64_t), s);
        g.gc_stamps = gcs;
#endif
        g.n_work = (int *)(ws + d.off_n_work);
        g.need_complete = (int *)(ws + d.off_need);
        g.complete_next = (int *)(ws + d.off_wq);
        g.init = init.anns;
        g.init_counts = init.counts;
        g.init_cap = init.cap;
        g.out_idx = init.out_index;
        g.out = d_anns;
        g.counts = d_counts;
        g.status = d_status;
        // PP_STAGE_SEED_LOOP_ONLY / PP_STAGE_AFTER_SEED_LOOP split stage 8 in two calls
        const bool run_rest = !(stages & PP_STAGE_SEED_LOOP_ONLY);
        if (!(stages & PP_STAGE_AFTER_SEED_LOOP)) {
            // external helper workgroups (images fewer than CUs) have a kernel of their own
            rc = g.n_ext > 0 ? launch_seed_loop_ext(g, n_img, s, ext) : launch_seed_loop(g, n_img, s, ext);
            if (rc) return rc;
        }
        // PP_STAGE_COMPLETE_ONLY / PP_STAGE_NMS_ONLY split the rest once more
        const bool run_complete = run_rest && !(stages & PP_STAGE_NMS_ONLY);
        const bool run_nms = run_rest && !(stages & PP_STAGE_COMPLETE_ONLY);
        if (run_complete && cfg->force_complete && !(stages & PP_STAGE_COMPLETE_SETS_EARLY)) {
            // complete_annotations' CafScored(score_th=0.0001) only where phase 1 left work
            rc = launch_caf_bucketed(h, hr, n_img, K, C, skeleton, cfg, cfg->complete_caf_threshold,
                                     cols[1], offs[1], g.need_complete, true, s, ext);
            if (rc) return rc;
        }
        if (run_complete && cfg->force_complete) {
            rc = launch_complete(g, n_img, complete_ways(stages), s, ext);
            if (rc) return rc;
        }
        if (run_nms)
            rc = launch_nms(g, n_img, (stages & PP_STAGE_NMS_WIDE) && g.n_ext == 0,
                            (stages & PP_STAGE_NMS_BITMAP) != 0, s);
#ifdef PP_STAMPS
        hipStreamSynchronize(s);
        const size_t nst = (size_t)n_img * 3 * kStampSlots;
        uint64_t *h = (uint64_t *)malloc(nst * sizeof(uint64_t));
        hipMemcpy(h, g.stamps, nst * sizeof(uint64_t), hipMemcpyDeviceToHost);
        const char *path = getenv("PP_STAMPS_OUT");
        FILE *fo = fopen(path ? path : "pp_stamps.bin", "ab");
        if (fo) {
            fwrite(h, sizeof(uint64_t), nst, fo);
            fclose(fo);
        }
        free(h);
        hipFree(g.stamps);
        uint64_t *hg = (uint64_t *)malloc((size_t)n_img * 4 * sizeof(uint64_t));
        hipMemcpy(hg, gcs, (size_t)n_img * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost);
        double a0 = 0, a1 = 0, a2 = 0;
        for (int i = 0; i < n_img; i++) {
            a0 += hg[4 * i];
            a1 += hg[4 * i + 1];
            a2 += hg[4 * i + 2];
        }
        fprintf(stderr, "grow_connection sections per image: offsets+scan-setup %.0f  columns %.0f  merge %.0f\n",
                a0 / n_img, a1 / n_img, a2 / n_img);
        free(hg);
        hipFree(gcs);
#endif
    }
    return rc;
}

}  // namespace pp

extern "C" {

int pp_decode_stages(const float *d_cif, const float *d_caf, int32_t n_img, int32_t K, int32_t C,
                     int32_t H, int32_t W, const int32_t *skeleton, const pp_config *cfg,
                     float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                     int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                     uint32_t stages, void *stream) {
    if (!d_cif || !d_caf || !cfg) return fail(PP_EINVAL, "pp_decode_batch: NULL argument");
    if (H <= 0 || W <= 0 || cfg->stride <= 0) return fail(PP_ESHAPE, "pp_decode_batch: bad shape");
    return decode_heads(single_head(d_cif, d_caf, H, W, cfg->stride), n_img, K, C, skeleton, cfg,
                        d_cifhr, d_anns, ann_capacity, d_counts, d_status, d_workspace,
                        workspace_bytes, stages, stream);
}

int pp_decode_ragged(const float *d_cif, const float *d_caf, int32_t n_img, int32_t K, int32_t C,
                     int32_t H, int32_t W, const int32_t *d_extents, const int32_t *extents,
                     const int32_t *skeleton, const pp_config *cfg, float *d_cifhr, pp_ann *d_anns,
                     int32_t ann_capacity, int32_t *d_counts, int32_t *d_status, void *d_workspace,
                     size_t workspace_bytes, uint32_t stages, void *stream) {
    if (!d_cif || !d_caf || !cfg || !d_extents || !extents)
        return fail(PP_EINVAL, "pp_decode_ragged: NULL argument");
    if (d_cifhr)
        return fail(PP_EINVAL, "pp_decode_ragged: the dense CifHr map of a ragged batch has no "
                               "layout (d_cifhr must be NULL)");
    if (H <= 0 || W <= 0 || cfg->stride <= 0) return fail(PP_ESHAPE, "pp_decode_ragged: bad shape");
    // cells outside an extent hold confidence 0 and every threshold compare is c > th: they
    // are candidates of nothing as long as no threshold is negative
    if (cfg->cif_threshold < 0.0f || cfg->seed_threshold < 0.0f || cfg->caf_threshold < 0.0f ||
        cfg->complete_caf_threshold < 0.0f)
        return fail(PP_EINVAL, "pp_decode_ragged: a ragged batch needs thresholds >= 0");
    for (int i = 0; i < n_img; i++)
        if (extents[2 * i] <= 0 || extents[2 * i] > H || extents[2 * i + 1] <= 0 ||
            extents[2 * i + 1] > W)
            return fail(PP_ESHAPE, "pp_decode_ragged: extent outside the container");
    DecodeInit init;
    init.extents = d_extents;
    return decode_heads(single_head(d_cif, d_caf, H, W, cfg->stride), n_img, K, C, skeleton, cfg,
                        nullptr, d_anns, ann_capacity, d_counts, d_status, d_workspace,
                        workspace_bytes, stages, stream, init);
}

int pp_decode_multi(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs, int32_t n_img,
                    int32_t K, int32_t C, const int32_t *skeleton, const pp_config *cfg,
                    float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                    int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                    uint32_t stages, void *stream) {
    Heads h;
    const int rc = make_heads(scales, n_scales, cif_pairs, 3, &h, "pp_decode_multi");
    if (rc) return rc;
    return decode_heads(h, n_img, K, C, skeleton, cfg, d_cifhr, d_anns, ann_capacity, d_counts,
                        d_status, d_workspace, workspace_bytes, stages, stream);
}

int pp_decode_initial(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs, int32_t n_img,
                      int32_t K, int32_t C, const int32_t *skeleton, const pp_config *cfg,
                      float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                      int32_t *d_status, const pp_ann *d_initial, const int32_t *d_initial_counts,
                      int32_t initial_capacity, int32_t *d_out_index, void *d_workspace,
                      size_t workspace_bytes, uint32_t stages, void *stream) {
    Heads h;
    const int rc = make_heads(scales, n_scales, cif_pairs, 3, &h, "pp_decode_initial");
    if (rc) return rc;
    if ((d_initial == nullptr) != (d_initial_counts == nullptr))
        return fail(PP_EINVAL, "pp_decode_initial: d_initial and d_initial_counts go together");
    if (d_initial && initial_capacity <= 0)
        return fail(PP_ESHAPE, "pp_decode_initial: bad initial_capacity");
    DecodeInit init;
    init.anns = d_initial;
    init.counts = d_initial_counts;
    init.cap = d_initial ? initial_capacity : 0;
    init.out_index = d_out_index;
    return decode_heads(h, n_img, K, C, skeleton, cfg, d_cifhr, d_anns, ann_capacity, d_counts,
                        d_status, d_workspace, workspace_bytes, stages, stream, init);
}

int pp_decode_batch(const float *d_cif, const float *d_caf, int32_t n_img, int32_t K, int32_t C,
                    int32_t H, int32_t W, const int32_t *skeleton, const pp_config *cfg,
                    float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                    int32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream) {
    return pp_decode_stages(d_cif, d_caf, n_img, K, C, H, W, skeleton, cfg, d_cifhr, d_anns,
                            ann_capacity, d_counts, d_status, d_workspace, workspace_bytes, 15u,
                            stream);
}

}  // extern "C"

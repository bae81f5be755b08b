// decode.hip — host side of the decoder.  The kernels and their launchers are in
// seed_loop.hip, seed_loop_ext.hip, complete.hip and nms.hip.  In the order of the file:
//   DecodeLayout / make_layout and the six size / offset exports: the workspace layout;
//   SideStream / SideFork: the library's side stream and one fork / join of it;
//   check_decode: every refusal of a decode, before anything touches HIP;
//   DecodeRegions / decode_regions: the workspace regions as typed pointers;
//   grow_args: the GrowArgs of stage 8 (the skeleton through by_source.hpp's BySource);
//   stamps_begin / stamps_end: the diagnostic build's buffers and their dump;
//   decode_heads: the stage sequence, behind all six pp_decode_* entry points.
#include "by_source.hpp"
#include "grow_args.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <mutex>

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

// One fork of the side stream off the caller's stream s: the side stream's lock, held from
// here to the end of the scope, and the fork events (the side stream waits for what s holds
// now).  join() makes s wait for what the side stream holds then.
struct SideFork {
    const SideStream *side;
    hipStream_t s;
    std::lock_guard<std::mutex> lock;
    bool forked;

    SideFork(const SideStream *ss, hipStream_t caller)
        : side(ss), s(caller), lock(ss->mu),
          forked(hipEventRecord(ss->fork, caller) == hipSuccess &&
                 hipStreamWaitEvent(ss->stream, ss->fork, 0) == hipSuccess) {}
    bool join() const {
        return hipEventRecord(side->join, side->stream) == hipSuccess &&
               hipStreamWaitEvent(s, side->join, 0) == hipSuccess;
    }
};

// the stage bits that include/pifpaf_amd.h gives as numbers (pp_decode_stages)
constexpr uint32_t kStageCifHr = 1u, kStageSeeds = 2u, kStageCafScored = 4u;
constexpr uint32_t kStageGrow = 8u;  // seed loop, force-complete and NMS
constexpr uint32_t kStageSeedsAndCaf = kStageSeeds | kStageCafScored;
constexpr uint32_t kStageAll = kStageCifHr | kStageSeedsAndCaf | kStageGrow;

// optional inputs of pp_decode_initial
struct DecodeInit {
    const pp_ann *anns = nullptr;
    const int32_t *counts = nullptr;
    int32_t cap = 0;
    int32_t *out_index = nullptr;
    // pp_decode_ragged / pp_decode_multi_ragged: the images' own field sizes (of CIF head 0),
    // device (n_img, 2) (hr_dims)
    const int32_t *extents = nullptr;
};

// Every refusal of a decode, in this order and before anything touches HIP; the messages
// name pp_decode_batch whichever entry point was called.  An empty batch is PP_OK with *d
// left alone: the caller returns on `rc || n_img == 0`.
static int check_decode(const Heads &h, int32_t n_img, int32_t K, int32_t C,
                        const int32_t *skeleton, const pp_config *cfg, const pp_ann *d_anns,
                        int32_t ann_capacity, const int32_t *d_counts, const int32_t *d_status,
                        const void *d_workspace, size_t workspace_bytes, DecodeLayout *d) {
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
    *d = make_layout(n_img, K, C, h, cfg, ann_capacity);
    if (workspace_bytes < d->total) return fail(PP_ENOMEM, "pp_decode_batch: workspace too small");
    if ((int64_t)d->hh >= kMaxHrSide || (int64_t)d->ww >= kMaxHrSide)
        return fail(PP_ESHAPE, "pp_decode_batch: field too large (CifHr map of 32768 px or "
                               "more per side)");
    return PP_OK;
}

// The workspace regions of a decode as typed pointers.
struct DecodeRegions {
    // the caller's d_cifhr gets the dense map; otherwise the decoder keeps the block-sparse
    // scratch map (hr_masks, and hr_aux with more than one CifHr group), written only where
    // splat boxes land
    float *hr_base, *hr_aux;
    uint64_t *hr_masks;
    HrMap hr;
    char *cifhr_ws, *seed_ws;
    pp_seed *seeds;
    int *seed_counts;
    float *cols[2];
    int *offs[2];
    // what only stage 8 reads, in the GrowArgs it reads them through: the regions and the
    // five above that its kernels read too, every other field zero (grow_args sets those)
    GrowArgs grow;
};

static DecodeRegions decode_regions(const DecodeLayout &d, void *d_workspace, float *d_cifhr) {
    char *ws = (char *)d_workspace;
    DecodeRegions p{};
    p.hr_base = d_cifhr ? d_cifhr : (float *)(ws + d.off_cifhr);
    p.hr_aux = (float *)(ws + d.off_hr_aux);
    p.hr_masks = d_cifhr ? nullptr : (uint64_t *)(ws + d.off_hr_masks);
    p.hr = dense_hr(p.hr_base, d.hh, d.ww);
    p.hr.masks = p.hr_masks;
    p.cifhr_ws = ws + d.off_cifhr_ws;
    p.seed_ws = ws + d.off_seed_ws;
    p.seeds = (pp_seed *)(ws + d.off_seeds);
    p.seed_counts = (int *)(ws + d.off_seed_counts);
    GrowArgs &g = p.grow;
    g.hr = p.hr;
    g.seeds = p.seeds;
    g.seed_counts = p.seed_counts;
    for (int t = 0; t < 2; t++) {
        g.cols[t] = p.cols[t] = (float *)(ws + d.off_cols[t]);
        g.offs[t] = p.offs[t] = (int *)(ws + d.off_offs[t]);
    }
    g.n_work = (int *)(ws + d.off_n_work);
    g.need_complete = (int *)(ws + d.off_need);
    g.complete_next = (int *)(ws + d.off_wq);
    g.occ = (uint8_t *)(ws + d.off_occ);
    g.log = (OccLog *)(ws + d.off_log);
    g.work = (pp_ann *)(ws + d.off_work);
    g.spec = (pp_ann *)(ws + d.off_spec);
    g.xext = (SeedExt *)(ws + d.off_xext);
    g.xrec = (pp_ann *)(ws + d.off_xrec);
    g.nms_score = (double *)(ws + d.off_nms_score);
    g.nms_idx = (int *)(ws + d.off_nms_idx);
    g.nms_f = (float *)(ws + d.off_nms_f);
    g.nms_box = (int2 *)(ws + d.off_nms_box);
    return p;
}

// GrowArgs of stage 8: the workspace regions, then the decode's shapes and options, the
// skeleton as directed-edge slots, the optional initial annotations and the outputs.
static GrowArgs grow_args(const Heads &h, int32_t n_img, int32_t K, int32_t C,
                          const int32_t *skeleton, const pp_config *cfg, const DecodeLayout &d,
                          const DecodeRegions &p, const DecodeInit &init, pp_ann *d_anns,
                          int32_t ann_capacity, int32_t *d_counts, int32_t *d_status) {
    GrowArgs g = p.grow;
    g.seed_cap = d.seed_cap;
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
    g.cif_floor = cfg->cif_floor;
    g.one_minus_floor = (float)(1.0 - (double)cfg->cif_floor);  // (1.0 - self.cif_floor)
    g.th_b = cfg->complete_caf_threshold;
    for (int ci = 0; ci < C; ci++) {
        g.caf_j1[ci] = (uint8_t)(skeleton[2 * ci] - 1);
        g.caf_j2[ci] = (uint8_t)(skeleton[2 * ci + 1] - 1);
    }
    // by_source flattened into directed-edge slots per start joint
    const BySource bs(skeleton, C);
    int nd = 0;
    for (int j = 0; j < K; j++) {
        g.j_off[j] = (uint8_t)nd;
        for (int e = 0; e < bs.n[j]; e++, nd++) {
            g.d_j[nd] = (uint8_t)j;
            g.d_k[nd] = (uint8_t)bs.end[j][e];
            g.d_caf[nd] = (uint8_t)bs.caf[j][e];
            g.d_fwd[nd] = (uint8_t)bs.fwd[j][e];
        }
    }
    g.j_off[K] = (uint8_t)nd;
    g.nd = nd;
    g.has_cs = cfg->confidence_scales != nullptr;
    for (int e = 0; e < kSlots; e++)
        g.slot_cs[e] = (g.has_cs && e < nd) ? cfg->confidence_scales[g.d_caf[e]] : 1.0f;
    g.occ_cap = d.occ_cap;
    g.log_cap = d.log_cap;
    g.spec_far = kSpecFar;
    g.n_ext = seed_ext_per_image(n_img);
    g.ann_np = d.ann_np;
    g.ann_cap = ann_capacity;
    g.init = init.anns;
    g.init_counts = init.counts;
    g.init_cap = init.cap;
    g.out_idx = init.out_index;
    g.out = d_anns;
    g.counts = d_counts;
    g.status = d_status;
    return g;
}

// The diagnostic build's cycle sums (grow_args.hpp): stamps_begin allocates and zeroes them
// before stage 8's first launch, stamps_end waits for the stream after its last, appends the
// kernels' sums to $PP_STAMPS_OUT and prints grow_connection's.
#ifdef PP_STAMPS
static void stamps_begin(GrowArgs &g, int n_img, hipStream_t s) {
    hipMalloc((void **)&g.stamps, (size_t)n_img * 3 * kStampSlots * sizeof(uint64_t));
    hipMemsetAsync(g.stamps, 0, (size_t)n_img * 3 * kStampSlots * sizeof(uint64_t), s);
    hipMalloc((void **)&g.gc_stamps, (size_t)n_img * 4 * sizeof(uint64_t));
    hipMemsetAsync(g.gc_stamps, 0, (size_t)n_img * 4 * sizeof(uint64_t), s);
}

static void stamps_end(const GrowArgs &g, int n_img, hipStream_t s) {
    hipStreamSynchronize(s);
    const size_t nst = (size_t)n_img * 3 * kStampSlots;
    uint64_t *hs = (uint64_t *)malloc(nst * sizeof(uint64_t));
    hipMemcpy(hs, g.stamps, nst * sizeof(uint64_t), hipMemcpyDeviceToHost);
    const char *path = getenv("PP_STAMPS_OUT");
    FILE *fo = fopen(path ? path : "pp_stamps.bin", "ab");
    if (fo) {
        fwrite(hs, sizeof(uint64_t), nst, fo);
        fclose(fo);
    }
    free(hs);
    hipFree(g.stamps);
    uint64_t *hg = (uint64_t *)malloc((size_t)n_img * 4 * sizeof(uint64_t));
    hipMemcpy(hg, g.gc_stamps, (size_t)n_img * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost);
    double a0 = 0, a1 = 0, a2 = 0;
    for (int i = 0; i < n_img; i++) {
        a0 += hg[4 * i];
        a1 += hg[4 * i + 1];
        a2 += hg[4 * i + 2];
    }
    fprintf(stderr, "grow_connection sections per image: offsets+scan-setup %.0f  columns %.0f  merge %.0f\n",
            a0 / n_img, a1 / n_img, a2 / n_img);
    free(hg);
    hipFree(g.gc_stamps);
}
#else
static void stamps_begin(GrowArgs &, int, hipStream_t) {}
static void stamps_end(const GrowArgs &, int, hipStream_t) {}
#endif

// The stage sequence of a decode, behind all six entry points.
static int decode_heads(const Heads &h, int32_t n_img, int32_t K, int32_t C,
                        const int32_t *skeleton, const pp_config *cfg, float *d_cifhr,
                        pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                        int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                        uint32_t stages, void *stream, const DecodeInit &init = DecodeInit{}) {
    DecodeLayout d;
    int rc = check_decode(h, n_img, K, C, skeleton, cfg, d_anns, ann_capacity, d_counts, d_status,
                          d_workspace, workspace_bytes, &d);
    if (rc || n_img == 0) return rc;
    const DecodeRegions p = decode_regions(d, d_workspace, d_cifhr);
    hipStream_t s = (hipStream_t)stream;
    const int32_t *ext = init.extents;
    // CafScored on stream `on`: set A at caf_threshold; set B, the force-complete set at
    // complete_caf_threshold (cell indices only), for the images `gate` marks (NULL: all)
    auto caf_a = [&](hipStream_t on) {
        return launch_caf_bucketed(h, p.hr, n_img, K, C, skeleton, cfg, cfg->caf_threshold,
                                   p.cols[0], p.offs[0], nullptr, false, on, ext);
    };
    auto caf_b = [&](hipStream_t on, const int *gate) {
        return launch_caf_bucketed(h, p.hr, n_img, K, C, skeleton, cfg,
                                   cfg->complete_caf_threshold, p.cols[1], p.offs[1], gate, true,
                                   on, ext);
    };
    // PP_STAGE_COMPLETE_SETS_EARLY with stage 1 (and without 8): the force-complete sets read
    // only the CAF fields, so they start on the side stream before the CifHr map, and a later
    // call's side-stream join (stages 2 | 4) covers them
    const bool sets_early = (stages & PP_STAGE_COMPLETE_SETS_EARLY) && cfg->force_complete;
    if (sets_early && (stages & kStageCifHr) && !(stages & kStageGrow)) {
        const SideStream *side = side_stream();
        if (!side) return fail(PP_EHIP, "pp_decode_stages: no side stream for stage 16");
        const SideFork fork(side, s);
        if (!fork.forked) return fail(PP_EHIP, "pp_decode_batch: side-stream fork failed");
        rc = caf_b(side->stream, nullptr);
        if (rc) {
            (void)fork.join();
            return rc;
        }
    }
    // the block-sparse map's kernel emits the seeds too when it can (stage 1 then writes
    // what seeds_emit_kernel would; stage 2 sorts them): the same test in both stages
    const bool fused_seeds = !d_cifhr && cifhr_fuses_seeds(h, n_img, K, cfg);
    auto seeds = [&]() {
        return launch_seeds(h, p.hr, n_img, K, cfg, p.seeds, d.seed_cap, p.seed_counts, p.seed_ws,
                            s, fused_seeds, ext);
    };
    if (stages & kStageCifHr) {
        if (d_cifhr) {
            rc = cifhr_heads_launch<false>(h, n_img, K, cfg, d_cifhr, p.cifhr_ws,
                                           d.cifhr_ws_bytes, s, "pp_decode_batch(cifhr)");
        } else {
            const SeedSink sink = seed_sink(n_img, K, cfg, d.seed_cap, p.seed_ws);
            rc = cifhr_sparse_launch(h, n_img, K, cfg, p.hr_base, p.hr_aux, p.hr_masks,
                                     p.cifhr_ws, d.cifhr_ws_bytes, s, "pp_decode_batch(cifhr)",
                                     fused_seeds ? &sink : nullptr, ext);
        }
        if (rc) return rc;
    }
    // CifSeeds and CafScored both read only the fields and the CifHr map: with both stages
    // requested, CafScored runs on a side stream beside the seeds (fork / join events)
    // PP_STAGE_COMPLETE_SETS_EARLY: the force-complete sets (every field and direction) with
    // CafScored instead of gated after the seed loop
    const bool early_b = sets_early && (stages & kStageCafScored) && !(stages & kStageCifHr);
    const SideStream *side =
        (stages & kStageSeedsAndCaf) == kStageSeedsAndCaf ? side_stream() : nullptr;
    if (side) {
        const SideFork fork(side, s);
        if (!fork.forked) return fail(PP_EHIP, "pp_decode_batch: side-stream fork failed");
        rc = caf_a(side->stream);
        if (!rc && early_b) rc = caf_b(side->stream, nullptr);
        if (!rc) rc = seeds();
        // join even after a failed launch, so the caller's stream never runs ahead
        if (!fork.join()) return fail(PP_EHIP, "pp_decode_batch: side-stream join failed");
        if (rc) return rc;
    } else {
        if (stages & kStageSeeds) {
            rc = seeds();
            if (rc) return rc;
        }
        if (stages & kStageCafScored) {  // the force-complete set is lazy unless early_b
            rc = caf_a(s);
            if (!rc && early_b) rc = caf_b(s, nullptr);
            if (rc) return rc;
        }
    }
    if (stages & kStageGrow) {
        GrowArgs g = grow_args(h, n_img, K, C, skeleton, cfg, d, p, init, d_anns, ann_capacity,
                               d_counts, d_status);
        stamps_begin(g, n_img, s);
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
            rc = caf_b(s, g.need_complete);
            if (rc) return rc;
        }
        if (run_complete && cfg->force_complete) {
            // kCompleteWays workgroups per image.  They pull annotations from a per-image
            // counter, so any count gives the same result; 8 or 16 for sparse batches measured
            // no better than 64 (round 5).
            rc = launch_complete(g, n_img, kCompleteWays, s, ext);
            if (rc) return rc;
        }
        if (run_nms)
            rc = launch_nms(g, n_img, (stages & PP_STAGE_NMS_WIDE) && g.n_ext == 0,
                            (stages & PP_STAGE_NMS_BITMAP) != 0, s);
        stamps_end(g, n_img, s);
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

int pp_decode_multi_ragged(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                           int32_t n_img, int32_t K, int32_t C, const int32_t *d_extents,
                           const int32_t *extents, const int32_t *skeleton, const pp_config *cfg,
                           float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity,
                           int32_t *d_counts, int32_t *d_status, void *d_workspace,
                           size_t workspace_bytes, uint32_t stages, void *stream) {
    if (!cfg || !d_extents || !extents)
        return fail(PP_EINVAL, "pp_decode_multi_ragged: NULL argument");
    if (d_cifhr)
        return fail(PP_EINVAL, "pp_decode_multi_ragged: the dense CifHr map of a ragged batch has "
                               "no layout (d_cifhr must be NULL)");
    Heads h;
    const int rc = make_heads(scales, n_scales, cif_pairs, 3, &h, "pp_decode_multi_ragged");
    if (rc) return rc;
    // the map is CIF head 0's: the kernels take every image's own map size from that head's
    // sub-table (hr_dims), first = the entry that is CIF head 0
    int first = -1;
    for (int e = 0; e < n_scales; e++) {
        if (scales[e].role == PP_ROLE_HRMAP)
            return fail(PP_EINVAL, "pp_decode_multi_ragged: a ragged batch takes no PP_ROLE_HRMAP "
                                   "entry (the map is CIF head 0's)");
        if (first < 0 && (scales[e].role == 0 || (scales[e].role & PP_ROLE_CIF))) first = e;
    }
    // cells outside an extent hold confidence 0 and every threshold compare is c > th: they
    // are candidates of nothing as long as no threshold is negative
    if (cfg->cif_threshold < 0.0f || cfg->seed_threshold < 0.0f || cfg->caf_threshold < 0.0f ||
        cfg->complete_caf_threshold < 0.0f)
        return fail(PP_EINVAL, "pp_decode_multi_ragged: a ragged batch needs thresholds >= 0");
    for (int e = 0; e < n_scales; e++)
        for (int i = 0; i < n_img; i++) {
            const int32_t *x = extents + 2 * ((int64_t)e * n_img + i);
            if (x[0] <= 0 || x[0] > scales[e].H || x[1] <= 0 || x[1] > scales[e].W)
                return fail(PP_ESHAPE, "pp_decode_multi_ragged: extent outside the container");
        }
    DecodeInit init;
    init.extents = d_extents + 2 * (int64_t)first * std::max(n_img, 0);
    return decode_heads(h, n_img, K, C, skeleton, cfg, nullptr, d_anns, ann_capacity, d_counts,
                        d_status, d_workspace, workspace_bytes, stages, stream, init);
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
                            ann_capacity, d_counts, d_status, d_workspace, workspace_bytes,
                            kStageAll, stream);
}

}  // extern "C"

// grow_args.hpp — what the CifCaf decoder's kernels (grow.hpp has the overview) and
// its host side (decode.hip) share.  Constants, workspace records, GrowArgs, the
// per-wave LDS record and the diagnostic build's stamp macros.
#pragma once

#include "pp_common.hpp"

// Diagnostic build only (-DPP_STAMPS, libpifpaf_amd_stamps.so): per-section shader-cycle
// sums of the decode kernel, dumped to $PP_STAMPS_OUT.  The product build compiles these
// to nothing.
#ifdef PP_STAMPS
#define STAMP_DECL                                                                          \
    uint64_t st_acc[kStampSlots] = {};                                                     \
    uint64_t st_t = __builtin_amdgcn_s_memtime();
#define STAMP(i)                                                                            \
    do {                                                                                    \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                                   \
        st_acc[i] += t_ - st_t;                                                             \
        st_t = t_;                                                                          \
    } while (0)
#define STAMP_FLUSH(ph)                                                                     \
    if (lane == 0 && g.stamps) {                                                            \
        st_acc[9] = L.fst[0];                                                               \
        st_acc[10] = L.fst[1];                                                              \
        st_acc[11] = L.fst[2];                                                              \
        st_acc[8] = L.fst[3];                                                               \
        st_acc[12] = L.fst[6];                                                              \
        st_acc[13] = L.fst[7];                                                              \
        for (int q_ = 0; q_ < kStampSlots; q_++)                                            \
            atomicAdd((unsigned long long *)&g.stamps[((int64_t)img * 3 + (ph)-1) * kStampSlots + q_], \
                      (unsigned long long)st_acc[q_]);                                      \
    }
#define FSTAMP_BEGIN const uint64_t fst_t0 = __builtin_amdgcn_s_memtime();
// eval_ahead's sections on wave 0 (fst[6]: from the column loads to their data, fst[7]: the
// forward query), with a vmcnt / lgkmcnt drain after the loads so the wait is attributed
#define ESTAMP(L, i, t)                                                                     \
    do {                                                                                    \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                                   \
        if ((threadIdx.x & 63) == 0) (L).fst[i] += t_ - (t);                                \
        (t) = t_;                                                                           \
    } while (0)
#define FSTAMP_END(L, i)                                                                    \
    if ((threadIdx.x & 63) == 0) (L).fst[i] += __builtin_amdgcn_s_memtime() - fst_t0;
// a section with a clock of its own: STAMP_T0(t) declares t and starts it, STAMP_SINCE(t) is
// the cycles since (t keeps running); STAMP_DO(...) is a statement of the diagnostic build
// only (a counter, `if (lane == 0) L.fst[8] += STAMP_SINCE(t)`, ...)
#define STAMP_T0(t) uint64_t t = __builtin_amdgcn_s_memtime()
#define STAMP_SINCE(t) (__builtin_amdgcn_s_memtime() - (t))
#define STAMP_DO(...) __VA_ARGS__
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH(ph)
#define FSTAMP_BEGIN
#define FSTAMP_END(L, i)
#define ESTAMP(L, i, t)
#define STAMP_T0(t)
#define STAMP_SINCE(t) 0
#define STAMP_DO(...)
#endif
constexpr int kStampSlots = 16;  // per (image, phase) in the diagnostic build

namespace pp {

constexpr int kKP = PP_MAX_KP;
constexpr int kSlots = 2 * PP_MAX_EDGES;   // directed edges (two lanes' worth of slots)
// flood-fill heap capacity: every joint is expanded at most once, pushing its by_source
// entries, so a fill pushes at most 2C <= 2 * PP_MAX_EDGES entries
constexpr int kHeap = 2 * PP_MAX_EDGES + 8;
constexpr int kOccMargin = 64;              // NMS occupancy slack beyond the main grid
constexpr int kCompleteWays = 64;           // force-complete workgroups per image
// the seed loop's workgroup, caches and external helpers (seed_loop.hpp has the design)
// 8 waves; 16 (cache 32, scan 256): 1.79 vs 1.28 ms per cfg3 step; 4 / 6: no better
constexpr int kSeedWaves = 8;
constexpr int kSpecCache = 16;     // speculative annotations of this CU's helpers
// distance (joint scales) a helper's seed keeps from the committed one and from the
// round's other picks; cached annotations are excluded by their exact occupancy boxes.
// Throughput is flat for 0-4 (both generators) and drops beyond 8.
constexpr float kSpecFar = 4.0f;
constexpr int kExtWgMax = 3;
constexpr int kExtHelpers = kExtWgMax * kSeedWaves;
constexpr int kExtCache = 32;
constexpr int kCacheSlots = kSpecCache + kExtCache;  // one lane per slot
static_assert(kCacheSlots <= 64 && kSeedWaves + kExtHelpers <= 64, "one lane per slot / helper");
// box-list scratch per image: one list per wave of nms_kernel, or per plane of
// nms_planes_kernel's fallback
constexpr int kNmsBoxLists = PP_MAX_KP;

struct FFEntry {  // _flood_fill frontier entry (-v, end_i, start_xyv, s)
    float neg;
    int end;
    float sxyv[3];
    float s;
};

struct OccLog {
    int f;
    int16_t x0, x1, y0, y1;
};

struct SeedExt {  // per image; zero at every launch (workspace zero region; the launch's
                  // last workgroup out re-zeroes it, ext_exit)
    unsigned long long task[kExtHelpers];  // 0 absent, 1 idle, 3 left; assigned: 2 |
                                           // slot << 8 | seed << 32
    unsigned int tag[kExtCache];           // seed + 1 of the record published in the slot
    unsigned int fin;                      // wave 0 is done
    unsigned int heavy;                    // wave 0 switched to the heavy regime
    unsigned int exited;                   // workgroups of the image done with these words
    unsigned int pad;
};
static_assert(sizeof(SeedExt) % 16 == 0, "memset block of whole 16-byte units");

struct GrowArgs {
    const pp_seed *seeds;
    const int *seed_counts;
    int seed_cap;
    const float *cols[2];     // bucketed column sets (n_img, C, 2, kColRows, col_cap): set A
                              // at caf_threshold, set B at complete_caf_threshold
    const int *offs[2];       // bucket boundaries (n_img, C, 2, nb + 1)
    int64_t col_cap;          // columns per set: the cells of all heads
    // set B (force-complete, complete_caf_threshold) holds only concatenated cell indices
    // (n_img, C, 2, col_cap); its queries read the heads' raw CAF and rescore with CifHr
    // (consider_raw)
    Heads heads;
    HrMap hr;                 // CifHr (dense, or the tile-major scratch layout)
    float cif_floor, one_minus_floor, th_b;
    uint8_t caf_j1[PP_MAX_EDGES], caf_j2[PP_MAX_EDGES];  // 0-based joints of each CAF
    int bw, bh, nb;           // bucket grid (see caf_bucketed_kernel)
    float inv_e;
    int K, C, hh, ww;
    pp_config cfg;
    // directed edges ("slots") in by_source order (cifcaf.py:62-65): joint j's entries
    // are slots j_off[j] .. j_off[j+1]-1 in dict insertion order
    int nd;
    uint8_t j_off[kKP + 1];
    uint8_t d_j[kSlots], d_k[kSlots], d_caf[kSlots], d_fwd[kSlots];
    // CifCaf(confidence_scales=...) (cifcaf.py:259-260, 282-284): the slot's CAF weight on
    // its frontier priorities when has_cs (pp_config.confidence_scales), else unused
    int has_cs;
    float slot_cs[kSlots];
    // workspace (per image regions)
    uint8_t *occ;
    int64_t occ_cap;          // bytes per image
    OccLog *log;
    int log_cap;              // entries per image
    pp_ann *work;             // working annotations
    pp_ann *spec;             // (n_img, kSpecCache) speculatively grown annotations
    float spec_far;           // seed-loop speculation distance, in joint scales
    int n_ext;                // external helper workgroups per image (seed loop)
    SeedExt *xext;            // (n_img) their hand-off words (zero at launch; the loop's last
                              // workgroup out re-zeroes them, ext_exit)
    pp_ann *xrec;             // (n_img, kExtCache) their published annotations
    double *nms_score;        // (n_img, 2 * ann_cap)
    // standalone NMS over caller annotations (pp_nms_keypoints_scored), else NULL: per
    // (image, record) -2 fixed_score, -1 none, j >= 0 suppress_score_index; the record's
    // score_weights (K each) and fixed scores (annotation.py:60-71)
    const int32_t *nms_spec;
    const double *nms_sw;
    const double *nms_fixed;
    double nms_it;            // nms.Keypoints.instance_threshold as the float64 it compares in
    int *nms_idx;             // (n_img, 4 * ann_cap + ann_np)
    float *nms_f;             // (n_img, 2 * ann_cap) per-annotation max x, max y
    int2 *nms_box;            // (n_img, kNmsBoxLists, ann_cap) plane box lists beyond registers
    int ann_np;               // next pow2 >= ann_cap
    int ann_cap;
    uint64_t *stamps;         // diagnostic build: (n_img, 3, kStampSlots) cycle sums, else NULL
    int *n_work;              // (n_img) annotations after the seed loop (phase 1 -> 2)
    int *complete_next;       // (n_img) force-complete work counters (zero region; the NMS
                              // kernel, ordered after completion, resets them)
    int *need_complete;       // (n_img) bitmask of joints left unset by the seed loop in any
                              // annotation (force-complete has work iff != 0; gates the B sets)
    // initial annotations (cifcaf.py:95-98), optional: (n_img, init_cap) records, the
    // first init_counts[img] of an image grown and committed before its seed loop
    const pp_ann *init;
    const int *init_counts;
    int init_cap;
    // outputs
    int *out_idx;             // optional (n_img, ann_cap): input index of each output record
    pp_ann *out;
    int *counts;
    int *status;
#ifdef PP_STAMPS
    // diagnostic build only, and last, so that no other field moves: (n_img, 4) section sums
    // of grow_connection (GSTAMP), or NULL
    uint64_t *gc_stamps;
#endif
};

// per-wave LDS of the grow kernels; HEAP: the flood-fill heap (force-complete only)
template <bool HEAP>
struct GrowLDST {
    pp_ann a;                     // record being built (lists; data synced from registers)
    FFEntry ff[HEAP ? kHeap : 1];
    int mark_pre[kKP + 1];        // occupancy boxes of one annotation: area prefix
    int mark_box[kKP][4];
    int ff_n;
    int log_n;
    int status;
#ifdef PP_STAMPS
    uint64_t fst[10];  // inside-grow section sums (diagnostic build); [8], [9]: seed loop
#endif
};
using GrowLDS = GrowLDST<true>;
using SeedLDS = GrowLDST<false>;  // the seed loop's waves (no flood fill)

// workspace regions start on 256-byte boundaries
static inline size_t align_up(size_t a) { return (a + 255) / 256 * 256; }

}  // namespace pp

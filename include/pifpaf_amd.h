/*
 * pifpaf_amd.h — C ABI of libpifpaf_amd.so, the MI355X (gfx950) CIF/CAF pose decoder.
 *
 * Drop-in boundary for openpifpaf v0.11.6's decoder hot path.  The reference exposes
 * this path as the Cython extension module `openpifpaf.functional`
 * (openpifpaf/functional.pyx) plus the pure-Python decoder classes in
 * openpifpaf/decoder/ (cif_hr.py, cif_seeds.py, caf_scored.py, generator/cifcaf.py,
 * nms.py, occupancy.py).  Every entry point below names the reference interface it
 * replaces (file:line).  The Python mirror of those interfaces is the package
 * openpifpaf_amd (ctypes over this header).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no C++/torch types; arrays are C-contiguous float32 unless
 *     a pitch/stride argument says otherwise.  Element strides, not byte strides.
 *   - every pointer named d_* is DEVICE memory (hipMalloc / torch device tensors).
 *     The caller owns all buffers; the library never allocates or frees them.
 *   - calls are asynchronous on `stream` (a hipStream_t; NULL = legacy default stream).
 *     No host synchronisation inside (graph-capturable).
 *   - return 0 on success or a negative pp_status; pp_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - the library has no global mutable state; calls on distinct streams are thread-safe.
 */
#ifndef PIFPAF_AMD_H
#define PIFPAF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ABI_VERSION 4

/* capacities of one annotation record (COCO person: 17 keypoints, 19 or 44 edges) */
#define PP_MAX_KP 24
#define PP_MAX_EDGES 64
#define PP_MAX_FRONTIER (4 * PP_MAX_EDGES)
#define PP_MAX_SCALES 16   /* CIF / CAF heads of one multi-scale decode */

typedef enum pp_status {
    PP_OK = 0,
    PP_EINVAL = -1,     /* bad argument (NULL pointer, negative size, bad enum) */
    PP_ESHAPE = -2,     /* shape outside the supported envelope                 */
    PP_EOVERFLOW = -3,  /* a capacity was exceeded; see the per-image status     */
    PP_EHIP = -4,       /* HIP runtime error (launch / device)                   */
    PP_ENOMEM = -5      /* workspace too small                                   */
} pp_status;

/*
 * Decoder configuration.  The reference keeps these as CLASS ATTRIBUTES written by
 * decoder/factory.py:configure (factory.py:64-98); pp_default_config() fills the
 * reference defaults (eval_coco: force_complete=1, seed_threshold=0.2).
 */
typedef struct pp_config {
    float cif_threshold;          /* CifHr.v_threshold                cif_hr.py:16          */
    float seed_threshold;         /* CifSeeds.threshold               cif_seeds.py:14       */
    float seed_score_scale;       /* CifSeeds.score_scale             cif_seeds.py:15       */
    float caf_threshold;          /* CafScored.default_score_th       caf_scored.py:14      */
    float complete_caf_threshold; /* score_th of the force-complete CafScored cifcaf.py:337 */
    float cif_floor;              /* CafScored(cif_floor=0.1)         caf_scored.py:16      */
    float keypoint_threshold;     /* CifCaf.keypoint_threshold        cifcaf.py:33          */
    float nms_keypoint_threshold; /* nms.Keypoints.keypoint_threshold nms.py:14             */
    float nms_instance_threshold; /* nms.Keypoints.instance_threshold nms.py:13             */
    float nms_suppression;        /* nms.Keypoints.suppression        nms.py:12             */
    int32_t stride;               /* FieldConfig.cif_strides[0] == caf_strides[0]  field_config.py:9-10 */
    int32_t cif_neighbors;        /* CifHr.neighbors                  cif_hr.py:15          */
    int32_t force_complete;       /* CifCaf.force_complete            cifcaf.py:31          */
    int32_t greedy;               /* CifCaf.greedy                    cifcaf.py:32          */
    int32_t connection_method;    /* CifCaf.connection_method: 0 'blend', 1 'max'  cifcaf.py:29 */
    int32_t apply_nms;            /* CifCaf(nms=True) -> nms.Keypoints()  cifcaf.py:43-44   */
    int32_t occupancy_reduction;  /* Occupancy(shape, 2, min_scale=4)  cifcaf.py:84         */
    int32_t occupancy_min_scale;
    uint32_t seed_skip_mask;      /* bit f set: field f emits no seeds, FieldConfig.seed_mask[f]
                                     falsy (cif_seeds.py:28-29); 0 = every field seeds       */
    int32_t exp_mode;             /* np.exp of the CAF scores (cifcaf.py:139): 0 = NumPy's
                                     float32 SIMD exp (the FMA3 / AVX512F routine NumPy runs on
                                     any x86-64 since 2013; bit-exact over every float32 in
                                     [-104, 0], tests/test_np_exp.py), 1 = correctly rounded
                                     (NumPy's scalar loop on CPUs without FMA3)              */
    const float *confidence_scales; /* HOST array (C): CifCaf(confidence_scales=...)
                                     (cifcaf.py:39,52), each CAF's weight on the frontier
                                     priorities of _grow (cifcaf.py:259-260, 282-284), f32
                                     products as NumPy forms them from a list of Python
                                     floats; NULL = none (the default)                       */
} pp_config;

/*
 * One output annotation (openpifpaf/annotation.py:9-28).  data/joint_scales are the
 * reference's float32 arrays; score is Annotation.score() (float64, annotation.py:60-71).
 * decoding_order entries (jsi, jti, xyv_jsi, xyv_jti) and frontier_order pairs as
 * appended by CifCaf._grow (cifcaf.py:263,305-306), 0-based joint indices.
 */
typedef struct pp_ann {
    float data[PP_MAX_KP][3];
    float joint_scales[PP_MAX_KP];
    double score;
    int32_t n_keypoints;
    int32_t n_decoding;
    int32_t n_frontier;
    int32_t image;
    uint8_t decoding_pairs[PP_MAX_KP][2];
    float decoding_xyv[PP_MAX_KP][6];
    uint8_t frontier_pairs[PP_MAX_FRONTIER][2];
} pp_ann;

/* one seed (cif_seeds.py:47 tuple (v, field, x, y, s)) */
typedef struct pp_seed {
    float v;
    int32_t field;
    float x;
    float y;
    float s;
} pp_seed;

/* One detection: AnnotationDet (annotation.py:122-137) with its image */
typedef struct pp_det {
    int32_t field;       /* category index (field_i)                                     */
    float score;
    float bbox[4];       /* x, y, w, h                                                   */
    int32_t image;
    int32_t pad_;
} pp_det;

/* nms.Detection class attributes (nms.py:60-65) */
typedef struct pp_det_nms {
    float suppression;        /* 0.1 */
    float suppression_soft;   /* 0.3 */
    float instance_threshold; /* 0.1 */
    float iou_threshold;      /* 0.7 */
    float iou_threshold_soft; /* 0.5 */
    int32_t apply;            /* 1 */
} pp_det_nms;

/* The meta of one image that Preprocess.annotations_inverse reads
 * (transforms/annotations.py:39-44): offset and scale float64, width_height[0], hflip,
 * rotation angle / width / height */
typedef struct pp_inverse_meta {
    double offset[2];
    double scale[2];
    double rotation_angle;
    double rotation_width;
    double rotation_height;
    double width;
    int32_t hflip;
    int32_t pad_;
} pp_inverse_meta;

/* One head of a multi-scale decode: FieldConfig entries (field_config.py:7-13,
 * factory.py:153-180).  The entries with the PP_ROLE_CIF bit form the CIF head list
 * (cif_indices order), those with PP_ROLE_CAF the CAF head list (caf_indices order); role 0
 * means both (one stride shared by a CIF and a CAF head).  0 for a min scale / distance
 * means unused (the reference tests them for truthiness). */
#define PP_ROLE_CIF 1
#define PP_ROLE_CAF 2
/* An entry that only names the CifHr map's geometry, (H-1)*stride+1 x (W-1)*stride+1,
 * instead of CIF head 0's (no field is read): the stage entry points then read or write a
 * map made at another head's size (CifSeeds.fill_cif / CafScored.fill_caf at any stride,
 * CifHr.fill_multiple into an existing map, cif_hr.py:42-57). */
#define PP_ROLE_HRMAP 4
typedef struct pp_scale {
    const float *cif;        /* (n_img, K, 5, H, W) when a CIF head */
    const float *caf;        /* (n_img, C, 9, H, W) when a CAF head */
    int32_t H, W, stride;
    float cif_min_scale;     /* cif_min_scales[i] */
    float caf_min_distance;  /* caf_min_distances[i] */
    float caf_max_distance;  /* caf_max_distances[i] (None -> 0) */
    int32_t role;            /* PP_ROLE_* bits, 0 = both */
} pp_scale;

/* per-image status bits written by pp_decode_batch (d_status) */
#define PP_ST_ANN_OVERFLOW 1   /* more annotations than ann_capacity               */
#define PP_ST_NMS_OVERFLOW 2   /* NMS occupancy larger than the occupancy workspace */
#define PP_ST_SEED_OVERFLOW 4  /* more seeds than the seed workspace               */
#define PP_ST_DEC_OVERFLOW 8   /* decoding/frontier order longer than the record   */

int pp_version(void);
const char *pp_last_error(void);
void pp_default_config(pp_config *cfg);

/* ---------------------------------------------------------------------------------
 * Decoder stages.  Batched: n_img images, fields (n_img, K, 5, H, W) and
 * (n_img, C, 9, H, W) resident in device memory.  The high-resolution CIF map is laid
 * out (n_img, K, H', pitch) with H' = (H-1)*stride+1, W' = (W-1)*stride+1 and
 * pitch = pp_cifhr_pitch(W') (a multiple of 32 floats, so each row starts on a 128-B line).
 * --------------------------------------------------------------------------------- */
int64_t pp_cifhr_pitch(int64_t w_hr);

/* bytes of scratch pp_decode_batch needs (pass the same arguments) */
size_t pp_decode_workspace_size(int32_t n_img, int32_t K, int32_t C, int32_t H, int32_t W,
                                const pp_config *cfg, int32_t ann_capacity);

/*
 * CifHr (cif_hr.py:14-81): zero-init + accumulate every CIF cell with c > cif_threshold
 * as a truncate=1 Gaussian splat (functional.pyx:105-141) into d_cifhr.  Bit-exact.
 * d_workspace >= pp_cifhr_workspace_size(n_img, K, H, W).
 */
size_t pp_cifhr_workspace_size(int32_t n_img, int32_t K, int32_t H, int32_t W);
int pp_cifhr(const float *d_cif, int32_t n_img, int32_t K, int32_t H, int32_t W,
             const pp_config *cfg, float *d_cifhr, void *d_workspace, size_t workspace_bytes,
             void *stream);

/*
 * The same CifHr as the block-sparse map the decoder keeps (cif_hr.py:14-81, values bit-equal
 * to pp_cifhr): the (H', pitch) plane is cut into T = pp_cifhr_sparse_tiles(H, W, stride)
 * 64x64 tiles (row-major, ceil(pitch/64) per row) of 64 8x8 blocks.  d_map
 * (n_img, K, T, 64 blocks, 64 px): block b = 8*by + bx of a tile holds its 8 rows of 8
 * pixels back to back; d_masks (n_img, K, T) u64 with bit b set iff block b was written.
 * Only blocks some splat box touches are written; every other pixel is 0.
 * d_workspace >= pp_cifhr_sparse_workspace_size(n_img, K, H, W).
 */
int32_t pp_cifhr_sparse_tiles(int32_t H, int32_t W, int32_t stride);
size_t pp_cifhr_sparse_workspace_size(int32_t n_img, int32_t K, int32_t H, int32_t W);
int pp_cifhr_sparse(const float *d_cif, int32_t n_img, int32_t K, int32_t H, int32_t W,
                    const pp_config *cfg, float *d_map, uint64_t *d_masks, void *d_workspace,
                    size_t workspace_bytes, void *stream);

/*
 * CifSeeds (cif_seeds.py:23-64): per image, the seeds sorted as
 * sorted(seeds, reverse=True) (cif_seeds.py:54).  d_seeds (n_img, seed_capacity) with
 * seed_capacity >= K*H*W (every cell can seed, so no overflow is possible);
 * d_counts (n_img) = number of seeds.
 */
int pp_seeds(const float *d_cif, const float *d_cifhr, int32_t n_img, int32_t K, int32_t H,
             int32_t W, const pp_config *cfg, pp_seed *d_seeds, int32_t seed_capacity,
             int32_t *d_counts, void *stream);

/*
 * CafScored (caf_scored.py:32-98) for one score threshold: per image and CAF field, the
 * backward and forward (9, N) column sets.  Layout d_cols (n_img, C, 2, 9, H*W) with
 * direction 0 = backward, 1 = forward; d_counts (n_img, C, 2).
 */
int pp_caf_scored(const float *d_caf, const float *d_cifhr, int32_t n_img, int32_t K,
                  int32_t C, int32_t H, int32_t W, const int32_t *skeleton, float score_th,
                  const pp_config *cfg, float *d_cols, int32_t *d_counts, void *stream);

/*
 * Full decode, CifCaf.__call__ (cifcaf.py:67-122) for a batch: CifHr -> CifSeeds ->
 * CafScored -> seed loop / _grow -> complete_annotations -> nms.Keypoints.
 *   skeleton      HOST array (C, 2) of 1-based joint pairs (cifcaf.py:50)
 *   d_anns        (n_img, ann_capacity) records, image-major, in the reference's final order
 *   d_counts      (n_img) number of annotations per image (true count)
 *   d_status      (n_img) PP_ST_* bits; a non-zero bit means "re-run with more capacity"
 *   d_cifhr       optional (n_img, K, H', pitch) output of the CifHr stage (NULL: scratch)
 */
int pp_decode_batch(const float *d_cif, const float *d_caf, int32_t n_img, int32_t K,
                    int32_t C, int32_t H, int32_t W, const int32_t *skeleton,
                    const pp_config *cfg, float *d_cifhr, pp_ann *d_anns,
                    int32_t ann_capacity, int32_t *d_counts, int32_t *d_status,
                    void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Multi-scale decode: the same stages over a FieldConfig of CIF and CAF heads
 * (field_config.py:7-13; the heads' scale / min-distance lists of factory.py:153-180) given
 * as n_scales pp_scale entries (see PP_ROLE_*), device arrays of each head's own size.
 * cif_pairs groups the CIF heads for CifHr (fill_multiple, cif_hr.py:42-57): 0 = one group
 * per head; 1 = the reference's 10-head hflip layout (cif_hr.py:63-68), heads g and g + n/2
 * accumulated into one map at head g's stride and min scale (the reference pairs exactly
 * when len(cif_indices) == 10); m >= 2 = groups of m heads, head g + i * (n / m) being
 * member i of group g, each splat weighted v / neighbors / m.  The groups' maps are combined
 * by np.maximum.  The CifHr map has CIF head 0's size, (n_img, K, H', pitch) with
 * H' = (H_0 - 1) * stride_0 + 1, unless a PP_ROLE_HRMAP entry names another.  cfg->stride
 * is unused.
 *   pp_cifhr_multi       CifHr.fill (cif_hr.py:59-73), maps combined by np.maximum
 *   pp_seeds_multi       CifSeeds.fill over every CIF head (cif_seeds.py:56-64), sorted;
 *                        seed_capacity >= K * (sum of the CIF heads' H * W)
 *   pp_caf_scored_multi  CafScored.fill over every CAF head (caf_scored.py:88-98): per field
 *                        the heads' columns concatenated; d_cols (n_img, C, 2, 9,
 *                        col_capacity) with col_capacity >= the CAF heads' cells,
 *                        d_counts (n_img, C, 2); the list must hold the CIF heads too
 *                        (CIF head 0 gives the CifHr geometry; CIF fields are not read)
 *   pp_decode_multi      CifCaf.__call__ (cifcaf.py:67-122) over the heads, `stages` as
 *                        pp_decode_stages (15 = the full decode); outputs and status as
 *                        pp_decode_batch, workspace contract as pp_decode_stages (zero
 *                        region from pp_decode_multi_workspace_zero_offset).
 */
size_t pp_cifhr_multi_workspace_size(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                                     int32_t n_img, int32_t K);
int pp_cifhr_multi(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs, int32_t n_img,
                   int32_t K, const pp_config *cfg, float *d_cifhr, void *d_workspace,
                   size_t workspace_bytes, void *stream);
int pp_seeds_multi(const pp_scale *scales, int32_t n_scales, const float *d_cifhr, int32_t n_img,
                   int32_t K, const pp_config *cfg, pp_seed *d_seeds, int32_t seed_capacity,
                   int32_t *d_counts, void *stream);
int pp_caf_scored_multi(const pp_scale *scales, int32_t n_scales, const float *d_cifhr,
                        int32_t n_img, int32_t K, int32_t C, const int32_t *skeleton,
                        float score_th, const pp_config *cfg, float *d_cols,
                        int64_t col_capacity, int32_t *d_counts, void *stream);
size_t pp_decode_multi_workspace_size(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                                      int32_t n_img, int32_t K, int32_t C, const pp_config *cfg,
                                      int32_t ann_capacity);
size_t pp_decode_multi_workspace_zero_offset(const pp_scale *scales, int32_t n_scales,
                                             int32_t cif_pairs, int32_t n_img, int32_t K,
                                             int32_t C, const pp_config *cfg,
                                             int32_t ann_capacity);
int pp_decode_multi(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs, int32_t n_img,
                    int32_t K, int32_t C, const int32_t *skeleton, const pp_config *cfg,
                    float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                    int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                    uint32_t stages, void *stream);

/*
 * CifCaf.__call__(fields, initial_annotations) (cifcaf.py:67-71, 95-98): pp_decode_multi
 * where each image first grows its initial annotations d_initial[img * initial_capacity + i],
 * i < d_initial_counts[img] (set A, reverse matching, from every joint with v != 0; the
 * records' decoding / frontier orders are kept and appended to), appends them to its
 * annotation list in that order and marks them occupied, then runs the seed loop; force-
 * complete and NMS see them like any other annotation.  A record needs data,
 * joint_scales, n_decoding, decoding_pairs / decoding_xyv, n_frontier and frontier_pairs;
 * image and n_keypoints are set by the decoder.  d_initial / d_initial_counts may be NULL
 * (then this is pp_decode_multi).  d_out_index (optional, (n_img, ann_capacity) int32):
 * for each output record its position in the image's annotation list before NMS, so
 * positions < d_initial_counts[img] are the initial annotations (the reference returns those
 * objects, mutated).  Workspace as pp_decode_multi (pp_decode_multi_workspace_size).
 * Reference interface: openpifpaf.decoder.CifCaf.__call__ (cifcaf.py:67).
 */
/*
 * Byte offset, inside a decode workspace of that shape, of the (n_img, ann_capacity) pp_ann
 * working records: after a decode with the grow stage, image img's annotation list before
 * NMS (positions as d_out_index reports them), in the state NMS left every one of them in,
 * including those it dropped (nms.py:20-53 edits the Annotation objects in place before it
 * filters them).  Valid until the next decode into the workspace.  pp_decode_work_offset
 * for pp_decode_batch / pp_decode_stages workspaces, pp_decode_multi_work_offset for
 * pp_decode_multi / pp_decode_initial ones; 0 on a bad shape.
 * Reference interface: the initial_annotations objects CifCaf.__call__ mutates
 * (cifcaf.py:67-71, 95-98, 117-118).
 */
size_t pp_decode_work_offset(int32_t n_img, int32_t K, int32_t C, int32_t H, int32_t W,
                             const pp_config *cfg, int32_t ann_capacity);
size_t pp_decode_multi_work_offset(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                                   int32_t n_img, int32_t K, int32_t C, const pp_config *cfg,
                                   int32_t ann_capacity);

int pp_decode_initial(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs, int32_t n_img,
                      int32_t K, int32_t C, const int32_t *skeleton, const pp_config *cfg,
                      float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                      int32_t *d_status, const pp_ann *d_initial, const int32_t *d_initial_counts,
                      int32_t initial_capacity, int32_t *d_out_index, void *d_workspace,
                      size_t workspace_bytes, uint32_t stages, void *stream);

/*
 * CifDet detection decoder (decoder/generator/cifdet.py:27-52), batched:
 *   d_det     (n_img, K, 7, H, W) CifDet fields [c, x, y, b, w, h, b2] (heads.py:127-144)
 *   d_cifhr   optional (n_img, K, H', pitch) output of CifDetHr (NULL: scratch)
 *   d_out     (n_img, det_capacity) pp_det, d_counts (n_img), d_status (n_img) PP_ST_* bits
 * Uses cfg's cif_threshold (CifHr.v_threshold), seed_threshold (>= 0), seed_score_scale,
 * stride and cif_neighbors; the occupancy is the reference's fixed Occupancy(cifhr.shape,
 * 2, min_scale=2.0); nms.Detection runs with *nms (pp_default_det_nms) when nms->apply.
 * pp_cifdet_hr is the CifDetHr stage alone (cif_hr.py:84-100), workspace as pp_cifhr.
 */
void pp_default_det_nms(pp_det_nms *nms);
int pp_cifdet_hr(const float *d_det, int32_t n_img, int32_t K, int32_t H, int32_t W,
                 const pp_config *cfg, float *d_cifhr, void *d_workspace, size_t workspace_bytes,
                 void *stream);
/* CifDetHr.fill over several detection heads (cif_hr.py:67-80 as CifDetHr inherits it: each
 * head its own map at its stride, min-scale masks p[4] and p[5] > cif_min_scale / stride
 * (cif_hr.py:84-90), combined by np.maximum; cif_pairs as pp_cifhr_multi for the 10-head
 * layout).  scales: PP_ROLE_CIF entries whose `cif` points at (n_img, K, 7, H, W) detection
 * fields; d_cifhr has head 0's size (or a PP_ROLE_HRMAP entry's); workspace
 * pp_cifhr_multi_workspace_size of the same list. */
int pp_cifdet_hr_multi(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs, int32_t n_img,
                       int32_t K, const pp_config *cfg, float *d_cifhr, void *d_workspace,
                       size_t workspace_bytes, void *stream);
/* nms.Detection.annotations (nms.py:79-102) over caller records: n_img groups, d_in
 * (n_img, capacity) with d_counts[i] records (field, score, bbox) in list order.  Output
 * as pp_cifdet_decode; d_out_index (optional) = input index of each output record;
 * d_scores_out (optional, (n_img, capacity)) = every input record's score after the
 * reference's in-place edits (soft suppression; nms.py:90-99), in input order. */
size_t pp_nms_detection_workspace_size(int32_t n_img, int32_t capacity);
int pp_nms_detection(const pp_det *d_in, const int32_t *d_counts, int32_t n_img, int32_t capacity,
                     const pp_det_nms *nms, pp_det *d_out, int32_t *d_out_counts,
                     int32_t *d_out_index, float *d_scores_out, void *d_workspace,
                     size_t workspace_bytes, void *stream);
/* CifDetSeeds.fill_cif (cif_seeds.py:67-90) per (image, field), in cell order:
 * d_seg (n_img, K, 5, H*W) = v, x, y, w, h of the first d_seg_counts[i, f] entries;
 * d_cifhr (n_img, K, H', pitch).  get() = sorted((v, f, x, y, w, h), reverse=True). */
int pp_cifdet_seeds(const float *d_det, const float *d_cifhr, int32_t n_img, int32_t K, int32_t H,
                    int32_t W, const pp_config *cfg, float *d_seg, int32_t *d_seg_counts,
                    void *stream);
/* CifDetSeeds.fill over several detection heads (cif_seeds.py:56-64, 67-90: each head's
 * cells, min-scale masks on p[4] and p[5], x / y / w / h at the head's stride, v from the
 * one d_cifhr map), each field's seeds appended head after head: d_seg (n_img, K, 5, cells)
 * with cells = the heads' H * W summed. */
int pp_cifdet_seeds_multi(const pp_scale *scales, int32_t n_scales, const float *d_cifhr,
                          int32_t n_img, int32_t K, const pp_config *cfg, float *d_seg,
                          int32_t *d_seg_counts, void *stream);
size_t pp_cifdet_workspace_size(int32_t n_img, int32_t K, int32_t H, int32_t W,
                                const pp_config *cfg, int32_t det_capacity);
int pp_cifdet_decode(const float *d_det, int32_t n_img, int32_t K, int32_t H, int32_t W,
                     const pp_config *cfg, const pp_det_nms *nms, float *d_cifhr, pp_det *d_out,
                     int32_t det_capacity, int32_t *d_counts, int32_t *d_status,
                     void *d_workspace, size_t workspace_bytes, void *stream);
/* CifDet.__call__ (generator/cifdet.py:27-52) over a FieldConfig of several detection heads
 * and / or min scales: CifDetHr as pp_cifdet_hr_multi, CifDetSeeds as pp_cifdet_seeds_multi,
 * then the occupancy loop and nms.Detection as pp_cifdet_decode. */
size_t pp_cifdet_multi_workspace_size(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                                      int32_t n_img, int32_t K, int32_t det_capacity);
int pp_cifdet_decode_multi(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                           int32_t n_img, int32_t K, const pp_config *cfg, const pp_det_nms *nms,
                           float *d_cifhr, pp_det *d_out, int32_t det_capacity, int32_t *d_counts,
                           int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                           void *stream);

/*
 * Preprocess.annotations_inverse (transforms/preprocess.py:35-95) on device records, one
 * meta per image (d_metas (n_img) device array):
 *   pp_annotations_inverse  poses: rotation, offset, scale (data, joint_scales,
 *                           decoding_order), hflip with the optional horizontal swap
 *                           d_hswap (K) = target row of each source row (hflip.py:17-29);
 *                           d_nan_flags[i] |= 1 where the reference's NaN assert fires
 *   pp_dets_inverse         boxes: rotate_box (transforms/utils.py:5-28), offset, scale
 */
int pp_annotations_inverse(pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                           int32_t capacity, int32_t K, const pp_inverse_meta *d_metas,
                           const int32_t *d_hswap, int32_t *d_nan_flags, void *stream);
int pp_dets_inverse(pp_det *d_dets, const int32_t *d_counts, int32_t n_img, int32_t capacity,
                    const pp_inverse_meta *d_metas, void *stream);

/*
 * COCO prediction records, EvalCoco.from_predictions (eval_coco.py:108-158) for a whole
 * batch: from a decode's records (NOT modified) and one meta per image to the records an
 * evaluation writes to json, packed image after image.  Per image, in the reference's order:
 *   1. Preprocess.annotations_inverse on every record (eval_coco.py:113; the arithmetic of
 *      pp_annotations_inverse / pp_dets_inverse; d_hswap as there).  A NaN in x, y or v of
 *      any record sets PP_COCO_NAN in the image's flag word (preprocess.py:67 asserts).
 *   2. poses only, when small_threshold != 0: keep a record when
 *      Annotation.scale(v_th=0.01) >= small_threshold (eval_coco.py:115-117,
 *      annotation.py:73-80; float32 scale against the threshold rounded to float32, the
 *      Python float 0.0 against the threshold in float64 when no joint has v > 0.01).
 *   3. the first max_per_image survivors, in record order (eval_coco.py:118-120).
 *   4. json_data() (annotation.py:82-119 / 138-145) with image_id (eval_coco.py:122-131):
 *      keypoints with v of visible joints raised to 0.01, every value rounded to 2
 *      decimals as a double; bbox_from_keypoints in float32, rounded to 2 decimals; score
 *      max(0.001, round(score, 3)) of the record's score; a detection's category_id is
 *      field + 1.  The doubles are the Python floats the reference dumps.
 *   5. an image without a kept record gets one dummy record (eval_coco.py:133-141):
 *      keypoints zero, bbox [0, 0, 1, 1], score 0.001, category_id 1; PP_COCO_EMPTY is set
 *      in its flag word.
 * Pose records have pp_coco_record_size(K) = 56 + 24 K bytes: the pp_coco_det head with
 * n_keypoints (= K) in place of pad_, then double keypoints[K][3].
 *   d_anns / d_dets  (n_img, capacity) records, d_counts (n_img); a count above capacity
 *                    reads as capacity
 *   d_image_ids      (n_img) int64
 *   out              out_capacity records, 8-byte aligned; out_counts (n_img) = records of
 *                    each image, the dummy included; out_flags (n_img) PP_COCO_* bits.  Each
 *                    may be device memory or pinned host memory, as for pp_pack_compact.
 *                    Records whose packed index is >= out_capacity are not written;
 *                    out_counts is always complete, so the caller can size a second call.
 *   d_workspace      pp_coco_workspace_size(n_img) bytes of device memory
 * Two launches on `stream` (counts, then records).  Checked before any launch: NULL
 * pointers (d_hswap may be NULL) and a misaligned `out` -> PP_EINVAL; K outside
 * [1, PP_MAX_KP], max_per_image < 1, negative sizes or capacity < 1 -> PP_ESHAPE.
 * pp_coco_keypoints_cpu / pp_coco_dets_cpu: the same on HOST pointers, on the calling
 * thread, byte for byte (no workspace, no stream).
 */
#define PP_COCO_NAN 1
#define PP_COCO_EMPTY 2
typedef struct pp_coco_params {
    double small_threshold;   /* EvalCoco.small_threshold   eval_coco.py:33 (0 = no filter) */
    int32_t max_per_image;    /* EvalCoco.max_per_image     eval_coco.py:32 (20)            */
    int32_t category_id;      /* Annotation.category_id     annotation.py:13 (1); poses     */
} pp_coco_params;
typedef struct pp_coco_det {
    int64_t image_id;
    double score;
    double bbox[4];
    int32_t category_id;
    int32_t pad_;
} pp_coco_det;
int64_t pp_coco_record_size(int32_t K);
size_t pp_coco_workspace_size(int32_t n_img);
int pp_coco_keypoints(const pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                      int32_t capacity, int32_t K, const pp_inverse_meta *d_metas,
                      const int64_t *d_image_ids, const int32_t *d_hswap,
                      const pp_coco_params *params, void *out, int64_t out_capacity,
                      int32_t *out_counts, int32_t *out_flags, void *d_workspace, void *stream);
int pp_coco_dets(const pp_det *d_dets, const int32_t *d_counts, int32_t n_img, int32_t capacity,
                 const pp_inverse_meta *d_metas, const int64_t *d_image_ids,
                 const pp_coco_params *params, pp_coco_det *out, int64_t out_capacity,
                 int32_t *out_counts, int32_t *out_flags, void *d_workspace, void *stream);
int pp_coco_keypoints_cpu(const pp_ann *anns, const int32_t *counts, int32_t n_img,
                          int32_t capacity, int32_t K, const pp_inverse_meta *metas,
                          const int64_t *image_ids, const int32_t *hswap,
                          const pp_coco_params *params, void *out, int64_t out_capacity,
                          int32_t *out_counts, int32_t *out_flags);
int pp_coco_dets_cpu(const pp_det *dets, const int32_t *counts, int32_t n_img, int32_t capacity,
                     const pp_inverse_meta *metas, const int64_t *image_ids,
                     const pp_coco_params *params, pp_coco_det *out, int64_t out_capacity,
                     int32_t *out_counts, int32_t *out_flags);

/*
 * Field ingestion: the raw output of a CompositeFieldFused head's conv (network/heads.py:
 * 406-455, eval mode) -> the decoder's field layout, as CifCafCollector /
 * CifdetCollector.forward (heads.py:65-88, 127-144) produce it: `quad` PixelShuffle(2)
 * dequads with the last row / column cropped, sigmoid on confidences, exp on scales, the
 * index grid added to the vector components and the channel reorder, in one pass.
 *   d_conv  (n_img, F * 4^quad, h, w) with F = n_fields * (5 | 9 | 7) for layout
 *           0 CIF (IntensityMeta), 1 CAF (AssociationMeta), 2 CifDet (DetectionMeta)
 *   d_out   (n_img, n_fields, 5 | 9 | 7, H, W) with H = pp_fields_dim(h, quad)
 * Floats: sigmoid / exp are evaluated in f64 and rounded (within 1 ulp of torch's).
 */
int64_t pp_fields_dim(int64_t n, int32_t quad);
int pp_fields_from_conv(const float *d_conv, int32_t n_img, int32_t n_fields, int32_t layout,
                        int32_t h, int32_t w, int32_t quad, float *d_out, void *stream);

/*
 * pp_fields_from_conv with the conv output's type, the un-flip of a horizontally mirrored
 * pass and a field range of the output, still one read of the conv output.  With
 * conv_dtype PP_DTYPE_F32, mirror 0, no tables, out_fields = n_fields and out_field0 = 0 it
 * is pp_fields_from_conv (which calls it that way).
 *   conv_dtype  PP_DTYPE_F32 / F16 / BF16: the element type of d_conv.  A half value is
 *               converted exactly to float32 first, so the result equals the float32
 *               ingest of the up-converted tensor.  (Under autocast the reference would
 *               round its sigmoid / exp to half; the fields written here are float32 and
 *               are not rounded to half.)
 *   mirror      1: output column X reads source column W-1-X, and the x component of every
 *               vector the index grid is added to is negated before X is added (CIF: its
 *               vector; CAF: both; CifDet: the first vector only, not (w, h))
 *   src_field   host (n_fields) or NULL: output field f reads conv field src_field[f]
 *               (PifHFlip / PafHFlip's flip_indices, heads.py:149-152, 184-190)
 *   swap_ends   host (n_fields) or NULL, CAF only: 1 = output (x1, y1) takes conv vector
 *               2 and (x2, y2) conv vector 1 (PafHFlip's reverse_direction).  Regressions
 *               only: confidence, logb1 / logb2 and scale1 / scale2 stay in place, as the
 *               reference exchanges only the regressions (heads.py:209-212).
 *   d_out       (n_img, out_fields, 5 | 9 | 7, H, W); fields out_field0 .. out_field0 +
 *               n_fields - 1 of every image are written, the others are left alone
 * src_field and swap_ends are copied into the kernel arguments (at most 64 fields); they
 * need not outlive the call.  Checked before any launch: unknown dtype or layout,
 * src_field[i] outside [0, n_fields), swap_ends with a non-CAF layout -> PP_EINVAL; tables
 * with n_fields > 64, out_field0 < 0 or out_field0 + n_fields > out_fields -> PP_ESHAPE.
 */
#define PP_DTYPE_F32 0
#define PP_DTYPE_F16 1
#define PP_DTYPE_BF16 2
int pp_fields_from_conv_ex(const void *d_conv, int32_t conv_dtype, int32_t n_img,
                           int32_t n_fields, int32_t layout, int32_t h, int32_t w, int32_t quad,
                           int32_t mirror, const int32_t *src_field, const uint8_t *swap_ends,
                           float *d_out, int32_t out_fields, int32_t out_field0, void *stream);

/*
 * pp_fields_from_conv_ex on a view of a larger or differently ordered tensor, read in place:
 * the result is, bit for bit, that of pp_fields_from_conv_ex on the dense
 * (n_img, channels, h, w) copy of the same values, with channels = n_fields * (5 | 9 | 7) *
 * 4^quad.
 *   d_conv        element (0, 0, 0, 0) of the view; aligned to its element size, no more
 *   conv_strides  host (4): the image, channel, row and column strides in elements.  The
 *                 stride of a dimension of extent 1 is ignored.
 * The view must be one of
 *   planar       column stride 1, any image / channel / row strides: a dense NCHW tensor
 *                and its channel, batch and spatial slices (one thread per output pixel,
 *                as pp_fields_from_conv_ex)
 *   interleaved  channel stride 1, any image / row / column strides: a channels-last (NHWC)
 *                tensor and its slices (a workgroup reads the channel runs of 16 conv
 *                pixels with 16-byte loads and transposes them in LDS)
 * A view that is both (one column, or one channel) is read either way.  Checked before any
 * launch, after the checks of pp_fields_from_conv_ex: a negative stride, or neither the
 * channel nor the column stride equal to 1 -> PP_EINVAL.  Offsets are 64-bit.
 */
int pp_fields_from_conv_strided(const void *d_conv, int32_t conv_dtype,
                                const int64_t *conv_strides, int32_t n_img, int32_t n_fields,
                                int32_t layout, int32_t h, int32_t w, int32_t quad,
                                int32_t mirror, const int32_t *src_field,
                                const uint8_t *swap_ends, float *d_out, int32_t out_fields,
                                int32_t out_field0, void *stream);

/*
 * pp_fields_from_conv_ex for n_img images of different sizes, straight into the container of
 * a ragged batch (see "Ragged batches" below) in one pass: inside image i's own field,
 * [0, H_i) x [0, W_i) with (H_i, W_i) = (pp_fields_dim(h_i, quad), pp_fields_dim(w_i, quad)),
 * every value is, bit for bit, what pp_fields_from_conv_ex gives for the dense
 * (1, channels, h_i, w_i) copy of that image alone with the same conv_dtype, mirror, src_field
 * and swap_ends (the mirror is about the image's own W_i); outside it the value is +0.  Every
 * element of the written fields is stored exactly once: the container needs no memset, and
 * its bytes are those of pp_fields_pack_ragged over the per-image ingests.
 *   convs         HOST (n_img): device pointers to element (0, 0, 0) of each image's
 *                 (channels, h_i, w_i) conv view; aligned to the element size, no more
 *   conv_extents  HOST (n_img, 2): the conv sizes (h_i, w_i)
 *   conv_strides  HOST (n_img, 2) or NULL: each image's channel and row strides in elements;
 *                 NULL = every image dense.  The column stride is 1 (the planar class of
 *                 pp_fields_from_conv_strided).  The row stride of an image with h_i = 1 is
 *                 ignored.  Pointers and strides together describe a list of per-image
 *                 tensors as well as a padded (n_img, channels, hmax, wmax) batch, or a
 *                 channel slice of a fused one, with per-image valid extents.
 *   d_container   (n_img, out_fields, 5 | 9 | 7, H, W) float32, 4-byte aligned; fields
 *                 out_field0 .. out_field0 + n_fields - 1 of every image are written in full,
 *                 the others are left alone
 *   d_tables      pp_ragged_conv_tables_size(n_img) bytes, 8-byte aligned.  The three host
 *                 tables are copied into it on the stream, the 8-byte entries first; pageable
 *                 host tables are consumed before the call returns, pinned ones when the
 *                 stream reaches the copy.  The kernel also writes the (n_img, 2) int32 FIELD
 *                 extent table (H_i, W_i) that pp_decode_ragged takes, at d_tables +
 *                 pp_ragged_conv_extents_offset(n_img) (the last 8 n_img bytes).
 * Checked before any copy or launch: everything pp_fields_from_conv_ex checks; a NULL or
 * misaligned conv pointer, a negative stride -> PP_EINVAL; a conv extent <= 0, a field extent
 * larger than (H, W), H * W or n_img * out_fields * channels beyond int32, more than 65535
 * images or fields (the launch grid) -> PP_ESHAPE; then, for n_img > 0, a table buffer too
 * small -> PP_ENOMEM, d_tables not 8-byte or d_container not 4-byte aligned -> PP_EINVAL.
 * n_img = 0 returns PP_OK after the checks.  Offsets are 64-bit.
 */
size_t pp_ragged_conv_tables_size(int32_t n_img);
size_t pp_ragged_conv_extents_offset(int32_t n_img);
int pp_fields_from_conv_ragged(const void *const *convs, int32_t conv_dtype,
                               const int32_t *conv_extents, const int64_t *conv_strides,
                               int32_t n_img, int32_t n_fields, int32_t layout, int32_t quad,
                               int32_t mirror, const int32_t *src_field, const uint8_t *swap_ends,
                               int32_t H, int32_t W, float *d_container, int32_t out_fields,
                               int32_t out_field0, void *d_tables, size_t tables_bytes,
                               void *stream);

/*
 * pp_fields_from_conv_ragged for channels-last (NHWC) conv outputs and their slices, read where
 * they lie: the interleaved class of pp_fields_from_conv_strided, per image.  Inside image i's
 * own field every value is, bit for bit, what pp_fields_from_conv_ex gives for the dense
 * (1, channels, h_i, w_i) copy of that image alone with the same conv_dtype, mirror, src_field
 * and swap_ends (the mirror is about the image's own W_i); outside it the value is +0; every
 * element of the written fields is stored exactly once.  The container's bytes are those of
 * pp_fields_from_conv_ragged on the NCHW copies of the same values.  The arguments are those
 * of pp_fields_from_conv_ragged but for
 *   conv_strides  HOST (n_img, 2) or NULL: each image's ROW and COLUMN strides in elements;
 *                 the channel stride is 1.  NULL = every image dense channels-last (column
 *                 stride channels, row stride w_i * channels).  The stride of a dimension of
 *                 extent 1 is ignored.  A channel slice of a wider channels-last tensor is
 *                 such a view; its channel runs may start at any element offset.
 * d_tables has the size and layout of pp_fields_from_conv_ragged's (pp_ragged_conv_tables_size,
 * the field extent table at pp_ragged_conv_extents_offset) and is staged in the same way:
 * pageable host tables are consumed before the call returns, pinned ones when the stream
 * reaches the copy.  A workgroup reads the channel runs of 16 conv pixels of one row with
 * 16-byte loads and transposes them in LDS; the tiles cover the container.  The checks, their
 * codes and their order are those of pp_fields_from_conv_ragged, with more than 65535 channel
 * chunks (channels / 512 at quad <= 1) -> PP_ESHAPE beside the other grid limits; n_img = 0
 * returns PP_OK after the checks.  No device memory is allocated.  Offsets are 64-bit.
 */
int pp_fields_from_conv_ragged_interleaved(const void *const *convs, int32_t conv_dtype,
        const int32_t *conv_extents, const int64_t *conv_strides, int32_t n_img, int32_t n_fields,
        int32_t layout, int32_t quad, int32_t mirror, const int32_t *src_field,
        const uint8_t *swap_ends, int32_t H, int32_t W, float *d_container, int32_t out_fields,
        int32_t out_field0, void *d_tables, size_t tables_bytes, void *stream);

/*
 * pp_fields_from_conv_ragged for every head of a multi-scale FieldConfig in ONE launch: the
 * conv outputs of n_entries heads of n_img images go straight into the containers of a ragged
 * head set (pp_decode_multi_ragged), with no per-image fields, no pack and no memset.  An
 * entry (pp_conv_head) is one conv head and the field range of one container it writes;
 * several entries may write side by side into one container (CAF and dense CAF).  For every
 * entry the bytes of its field range are those of pp_fields_from_conv_ragged called for that
 * entry alone: inside image i's own field bit for bit pp_fields_from_conv_ex of the image
 * alone, mirrored about its own width, +0 outside it, every element stored exactly once, the
 * container's other fields untouched.
 *   heads         HOST (n_entries), 1 <= n_entries <= 3 * PP_MAX_SCALES.  layout 0 CIF or
 *                 1 CAF; d_container (n_img, out_fields, 5 | 9, H, W) float32, 4-byte aligned;
 *                 ext_row = the row of the field extent table the entry writes, or -1: every
 *                 row 0 .. n_rows - 1 is named by exactly one entry.  mirror, has_src,
 *                 src_field and swap_mask are pp_fields_from_conv_ex's mirror, src_field and
 *                 swap_ends; pp_conv_head_set_flip fills them from that call's arguments
 *                 (n_fields and layout set beforehand) with that call's checks.
 *   convs, conv_extents, conv_strides
 *                 HOST, entry-major (n_entries, n_img), (n_entries, n_img, 2) and
 *                 (n_entries, n_img, 2) or NULL, per (entry, image) what
 *                 pp_fields_from_conv_ragged takes per image (the planar class: column
 *                 stride 1).  The entries of one container have the same conv extents.
 *   conv_dtype, quad   of every conv output
 *   d_tables      pp_ragged_conv_heads_tables_size(n_img, n_entries) bytes, 8-byte aligned:
 *                 the pointers (8 n_entries n_img bytes), the strides (16 ...), the entries
 *                 (sizeof(pp_conv_head) n_entries), the conv extents (8 ...), then, at
 *                 pp_ragged_conv_heads_extents_offset(n_img, n_entries), the (n_rows, n_img, 2)
 *                 int32 FIELD extent table the kernel writes, row r = the (H_i, W_i) of the
 *                 entry that names r: the layout pp_decode_multi_ragged takes.  The host
 *                 tables go there in one copy on the stream when they lie in one host block in
 *                 this order (conv_strides given), else in one copy per table.  Pageable host
 *                 tables are consumed before the call returns, pinned ones when the stream
 *                 reaches the copy.  No device memory is allocated.
 * Workgroups of entry 0 come first on the x grid, then entry 1's (a prefix table of workgroup
 * counts in the kernel arguments); the image is the y grid.  Checked before any copy or launch,
 * in this order: a NULL table -> PP_EINVAL; n_img < 0, n_entries outside 1 .. 3 *
 * PP_MAX_SCALES, n_rows outside 1 .. n_entries, quad outside 0 .. 4 -> PP_ESHAPE; an unknown
 * dtype -> PP_EINVAL; per entry a NULL container -> PP_EINVAL, n_fields, H or W <= 0 ->
 * PP_ESHAPE, a layout other than 0 or 1 -> PP_EINVAL, and the checks of pp_fields_from_conv_ex
 * on the flip tables and the field range with its codes, H * W or n_img * out_fields * channels
 * beyond int32 -> PP_ESHAPE, a misaligned container -> PP_EINVAL; more than 65535 images or
 * 2^31 - 1 workgroups -> PP_ESHAPE; an ext_row outside -1 .. n_rows - 1, a row named by no
 * entry or by two -> PP_EINVAL; two entries whose container ranges overlap, or that share a
 * container but not its (layout, H, W, out_fields) -> PP_EINVAL; per (entry, image) the
 * pointer, extent and stride checks of pp_fields_from_conv_ragged with its codes; entries of
 * one container with different conv extents for some image -> PP_ESHAPE; then, for n_img > 0,
 * a table buffer too small -> PP_ENOMEM and d_tables not 8-byte aligned -> PP_EINVAL.
 * n_img = 0 returns PP_OK after the checks.  Offsets are 64-bit.
 */
typedef struct pp_conv_head {
    float *d_container;
    int32_t layout, n_fields;
    int32_t H, W;                     /* the container's */
    int32_t out_fields, out_field0;
    int32_t ext_row;
    int32_t mirror, has_src;
    int32_t reserved;                 /* 0 */
    uint64_t swap_mask;               /* bit f: swap_ends[f] */
    uint8_t src_field[64];
} pp_conv_head;
int pp_conv_head_set_flip(pp_conv_head *head, int32_t mirror, const int32_t *src_field,
                          const uint8_t *swap_ends);
size_t pp_ragged_conv_heads_tables_size(int32_t n_img, int32_t n_entries);
size_t pp_ragged_conv_heads_extents_offset(int32_t n_img, int32_t n_entries);
int pp_fields_from_conv_ragged_heads(const pp_conv_head *heads, int32_t n_entries,
                                     int32_t n_rows, const void *const *convs,
                                     const int32_t *conv_extents, const int64_t *conv_strides,
                                     int32_t n_img, int32_t conv_dtype, int32_t quad,
                                     void *d_tables, size_t tables_bytes, void *stream);

/*
 * nms.Keypoints.annotations (nms.py:17-57) over caller records, n_img independent groups:
 * d_anns (n_img, ann_capacity) with d_counts[i] records in group i (modified in place as
 * the reference modifies its Annotation objects: joints below keypoint_threshold zeroed,
 * suppressed joints' v scaled by nms_suppression).  Survivors sorted by -score go to
 * d_out (n_img, ann_capacity) with their score set, d_out_counts (n_img), and optionally
 * d_out_index (n_img, ann_capacity) = the input index of each survivor.  Uses cfg's
 * nms_* thresholds and occupancy_reduction / occupancy_min_scale.  Scores are the
 * default Annotation.score() (annotation.py:60-71 without fixed_score or
 * suppress_score_index).
 */
size_t pp_nms_workspace_size(int32_t n_img, int32_t ann_capacity);
int pp_nms_keypoints(pp_ann *d_anns, const int32_t *d_counts, int32_t n_img, int32_t K,
                     int32_t ann_capacity, const pp_config *cfg, pp_ann *d_out,
                     int32_t *d_out_counts, int32_t *d_out_index, void *d_workspace,
                     size_t workspace_bytes, void *stream);

/*
 * pp_nms_keypoints with each record's own Annotation.score() (annotation.py:60-71), for
 * annotations carrying fixed_score, suppress_score_index or non-default score_weights
 * (nms.py:21, 33, 53-54 sort and filter by it).  Per (image, record), laid out like d_anns:
 * d_score_spec -2 = fixed_score (d_fixed_score holds it), -1 = none, j in [0, K) =
 * suppress_score_index (v[j] reads as 0, negative Python indices normalised by the
 * caller); d_score_weights (n_img, ann_capacity, K) float64 = the record's score_weights;
 * d_fixed_score (n_img, ann_capacity) float64.  instance_threshold replaces cfg's float32
 * nms_instance_threshold: the reference compares score() >= it in float64 (a fixed_score
 * equal to the threshold is kept).  NULL d_score_spec = the default score().
 */
int pp_nms_keypoints_scored(pp_ann *d_anns, const int32_t *d_counts, int32_t n_img, int32_t K,
                            int32_t ann_capacity, const pp_config *cfg,
                            double instance_threshold, const int32_t *d_score_spec, const double *d_score_weights,
                            const double *d_fixed_score, pp_ann *d_out, int32_t *d_out_counts,
                            int32_t *d_out_index, void *d_workspace, size_t workspace_bytes,
                            void *stream);

/*
 * Packs a decode's records (d_anns (n_img, ann_capacity), d_counts[i] valid in slot row i)
 * image after image into `out` and copies the counts to out_counts: the flattened
 * per-image Annotation lists that Generator.batch returns (generator.py:96-97), in one
 * launch.  `out` / `out_counts` may be device memory or pinned host memory
 * (hipHostMalloc / hipHostRegister; written zero-copy through its mapped device address,
 * so one stream synchronisation hands the caller every record).  Records whose packed
 * index is >= out_capacity are not written; out_counts is always complete, so the caller
 * can size a retry.
 */
int pp_pack_records(const pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                    int32_t ann_capacity, pp_ann *out, int64_t out_capacity, int32_t *out_counts,
                    void *stream);

/*
 * The same hand-over for the detection decoder: d_dets (n_img, det_capacity) pp_det with
 * d_counts[i] valid records in row i, as every pp_cifdet_decode* entry point writes them,
 * packed image after image into `out`, the counts copied to out_counts and, when d_status
 * and out_status are given (together, or both NULL: PP_EINVAL otherwise), the decode's
 * PP_ST_* status words to out_status -- all in one launch, so one stream synchronisation
 * hands the caller the records and what it needs to judge them (an overflow bit means a
 * decode at a larger capacity).  `out`, `out_counts` and `out_status` may be device memory
 * or pinned host memory, as for pp_pack_records.  d_dets and `out` are 16-byte aligned
 * (PP_EINVAL otherwise, also for an empty batch): a pp_det is copied as two 16-byte chunks.
 * Records whose packed index is >= out_capacity are not written; out_counts is always
 * complete.  No more than det_capacity records of a row are read, whatever its count.
 * n_img == 0 is PP_OK without a launch.  Reference consumer: Generator.batch's per-image
 * lists (generator.py:96-97) of the CifDet generator (generator/cifdet.py:27-52).
 */
int pp_pack_det_records(const pp_det *d_dets, const int32_t *d_counts, const int32_t *d_status,
                        int32_t n_img, int32_t det_capacity, pp_det *out, int64_t out_capacity,
                        int32_t *out_counts, int32_t *out_status, void *stream);

/*
 * The same hand-over with COMPACT records (the wire format of the host fetch and the
 * multi-GPU gather): a pp_ann cut to K keypoints, pp_packed_record_size(K, C, flags) bytes
 * (a multiple of 16), little-endian:
 *   0   f64 score                       Annotation.score()        annotation.py:60-71
 *   8   i32 image
 *   12  u16 n_decoding | PP_PACK_REFETCH (bit 15), 14 u16 n_frontier
 *   16  f32 data[K][3], f32 joint_scales[K]                       annotation.py:17-18
 *   PP_PACK_DECODING: u8 decoding_pairs[K][2] (padded to 4 B), f32 decoding_v[K][2],
 *       f32 decoding_xy[K][2]: the (jsi, jti) pairs of decoding_order (cifcaf.py:305-306),
 *       v of xyv_jsi / xyv_jti, and per joint the x / y it had when it entered the order:
 *       xyv_jsi = (decoding_xy[jsi], v[0]), xyv_jti = (decoding_xy[jti], v[1]) (checked on
 *       the device for every entry)
 *   PP_PACK_FRONTIER: u8 frontier_pairs[F][2] (padded to 4 B), F = min(PP_MAX_FRONTIER, 4*C)
 * A record whose decoding entries disagree with the per-joint x / y, or whose orders exceed
 * K / F entries, carries PP_PACK_REFETCH: fetch that decode's full pp_ann records instead.
 * `out_flags` (optional, NULL to skip; device or pinned host memory, n_img int32): set to 1
 * for an image with at least one flagged record, else 0 -- so a caller whose records stay in
 * device memory (the multi-GPU gather) learns of a refetch without reading them.
 * `out` (16-byte aligned) holds out_capacity records; device or pinned host memory as for
 * pp_pack_records.  Reference consumer: Generator.batch's per-image lists
 * (generator.py:96-97).
 */
#define PP_PACK_DECODING 1u
#define PP_PACK_FRONTIER 2u
#define PP_PACK_REFETCH 0x8000u
int64_t pp_packed_record_size(int32_t K, int32_t C, uint32_t flags);
int pp_pack_compact(const pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                    int32_t ann_capacity, int32_t K, int32_t C, uint32_t flags, void *out,
                    int64_t out_capacity, int32_t *out_counts, int32_t *out_flags,
                    void *stream);

/*
 * The same decode split into stages for measurement: bit 1 CifHr, 2 CifSeeds,
 * 4 CafScored at caf_threshold, 8 seed loop + grow + complete + NMS (stage 8 also builds
 * the complete_caf_threshold column sets, only where force-complete needs them).  Stage buffers live
 * in the workspace, so calling the stages in order with the same workspace equals one
 * pp_decode_batch call.  pp_decode_batch == pp_decode_stages(..., 15, stream).
 * Bit 16 (PP_STAGE_COMPLETE_SETS_EARLY) moves the complete_caf_threshold column sets into
 * stage 4, built for every (field, direction) (stage 8 then reads them): the same result,
 * for callers that overlap one batch's stages 1-4 with the previous batch's stage 8.  In a
 * call with stage 1 (and without 8) they start on the library's side stream before the
 * CifHr map instead (they read only the CAF fields); a later call with stages 2 | 4 joins
 * that stream.
 * With bit 16, stage 8 may run in two calls on the same workspace and outputs: first with
 * PP_STAGE_SEED_LOOP_ONLY (32), then with PP_STAGE_AFTER_SEED_LOOP (64: force-complete and
 * NMS), so the second part can run on another stream beside the next batch's seed loop.
 * The second part may itself run as two calls: PP_STAGE_AFTER_SEED_LOOP | PP_STAGE_COMPLETE_ONLY
 * (128: force-complete), then PP_STAGE_AFTER_SEED_LOOP | PP_STAGE_NMS_ONLY (256).  NMS reads
 * only the annotation records and NMS scratch, none of which stages 1-4 write, so the
 * workspace's next stages 1-4 need wait only for the force-complete call.
 * PP_STAGE_NMS_WIDE (512, a hint for dense batches): NMS in workgroups of 8 waves instead of
 * 4 when the batch runs the one-CU seed loop (at least about CUs / 2 images).  The 4-wave
 * form fits on a CU beside a seed-loop workgroup, so an overlapped caller's NMS runs beside
 * the next batch's seed loop; the 8-wave form is faster per image on dense input
 * (hundreds of annotations per image).  With force-complete it also selects the number of
 * force-complete workgroups per image (more for dense batches).  Same results either way.
 * PP_STAGE_NMS_BITMAP (1024): NMS as three launches whose middle one decides each (image,
 * joint plane) with the plane's occupancy as a bitmap in LDS (one wave each) instead of
 * one launch walking box lists.  Same results; faster one step at a time, slower beside
 * another batch's seed loop (the many one-wave workgroups), hence opt-in.
 *
 * Workspace contract: bytes [pp_decode_workspace_zero_offset(), end) must be zero before
 * the first call (e.g. hipMemset once at allocation); every call leaves them zero again.
 */
#define PP_STAGE_COMPLETE_SETS_EARLY 16u
#define PP_STAGE_SEED_LOOP_ONLY 32u
#define PP_STAGE_AFTER_SEED_LOOP 64u
#define PP_STAGE_COMPLETE_ONLY 128u
#define PP_STAGE_NMS_ONLY 256u
#define PP_STAGE_NMS_WIDE 512u
#define PP_STAGE_NMS_BITMAP 1024u
int pp_decode_stages(const float *d_cif, const float *d_caf, int32_t n_img, int32_t K,
                     int32_t C, int32_t H, int32_t W, const int32_t *skeleton,
                     const pp_config *cfg, float *d_cifhr, pp_ann *d_anns,
                     int32_t ann_capacity, int32_t *d_counts, int32_t *d_status,
                     void *d_workspace, size_t workspace_bytes, uint32_t stages, void *stream);
size_t pp_decode_workspace_zero_offset(int32_t n_img, int32_t K, int32_t C, int32_t H,
                                       int32_t W, const pp_config *cfg, int32_t ann_capacity);

/* ---------------------------------------------------------------------------------
 * Ragged batches: images of different field sizes decoded in one batch.
 *
 * The images share a container: fields (n_img, K, 5, H, W) and (n_img, C, 9, H, W) with
 * (H, W) at least every image's own (h_i, w_i), image i in the top-left h_i x w_i corner
 * of its planes, and an (n_img, 2) int32 table of the (h_i, w_i).  The result is defined
 * as that of decoding every image alone at its own size (pp_decode_ragged_cpu is that
 * definition); zero-padding to a common size and pp_decode_batch give other annotations,
 * because the reference's scalar_values bounds, its splat box clip and its occupancy grid
 * follow the image's own CifHr size.  Everything else (workspace, capacities, outputs,
 * status bits, stage mask) is pp_decode_stages' at the container's (H, W).
 * pp_cifdet_decode_ragged (below) is the detection decoder over the same kind of batch, a
 * container (n_img, K, 7, H, W) with the same extent table.
 *
 * pp_fields_pack_ragged builds one container: `fields` is a HOST array of n_img device
 * pointers, image i's contiguous float32 (n_fields, channels, h_i, w_i), and `extents` the
 * HOST (n_img, 2) table.  Both are copied into d_tables (pp_ragged_tables_size(n_img)
 * bytes, 8-byte aligned) on the stream, pointers first; afterwards the device extent table
 * pp_decode_ragged takes is at d_tables + pp_ragged_extents_offset(n_img).  Pageable host
 * tables are consumed before the call returns, pinned ones when the stream reaches the copy.
 * Every element of d_container (n_img, n_fields, channels, H, W) is written once: the
 * image's value inside its extent, 0 outside, in 16-byte stores over each plane's 16-byte
 * aligned interior (d_container needs 4-byte alignment only).  PP_ESHAPE: an extent <= 0 or
 * larger than the container.
 *
 * pp_decode_ragged: single-scale.  d_extents is the device table, `extents` the same
 * table on the host (argument checks only, read before the call returns).  Precondition:
 * the confidence channel (channel 0) of every cell outside its image's extent is 0, as the
 * packer leaves it.  PP_ESHAPE: an extent <= 0 or larger than the container.  PP_EINVAL: a
 * negative cif_threshold, seed_threshold, caf_threshold or complete_caf_threshold (cells
 * outside an extent must pass no `c > threshold`), or d_cifhr != NULL (a dense map of a
 * ragged batch has no defined layout yet; the argument is kept for the signature's sake).
 * --------------------------------------------------------------------------------- */
size_t pp_ragged_tables_size(int32_t n_img);
size_t pp_ragged_extents_offset(int32_t n_img);
int pp_fields_pack_ragged(const float *const *fields, const int32_t *extents, int32_t n_img,
                          int32_t n_fields, int32_t channels, int32_t H, int32_t W,
                          float *d_container, void *d_tables, size_t tables_bytes, void *stream);
int pp_decode_ragged(const float *d_cif, const float *d_caf, int32_t n_img, int32_t K,
                     int32_t C, int32_t H, int32_t W, const int32_t *d_extents,
                     const int32_t *extents, const int32_t *skeleton, const pp_config *cfg,
                     float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity, int32_t *d_counts,
                     int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                     uint32_t stages, void *stream);
/*
 * Ragged multi-scale batches: pp_decode_multi over images of different field sizes.
 *
 * Every pp_scale entry is a container (n_img, n_fields, channels, H, W) of its own (H, W),
 * image i in the top-left corner of its planes at that head's own size.  The extent tables
 * hold one (h, w) per entry and image, entry-major: (n_scales, n_img, 2) int32, so the
 * sub-table of entry e starts at 2 * e * n_img.  d_extents is the device table, `extents` the
 * same on the host (argument checks only, read before the call returns).
 *
 * pp_decode_multi_ragged: image i's records are, record for record and bit for bit, those of
 * pp_decode_multi over that image alone with every head cropped to its own extent; pp_ann.image
 * is its position in the batch.  In the reference the CifHr map takes its size from the first
 * head filled (cif_hr.py:45-51), and the bounds of scalar_values (cif_seeds.py:37,
 * caf_scored.py:63,74), the splat box clip and the occupancy grid (occupancy.py:11-26) follow
 * the map: so image i's map is (h - 1) * stride + 1 of CIF head 0's extent, the sub-table of
 * the entry that is CIF head 0, and the other heads' extents only say which container cells
 * are real.  Precondition: the confidence channel (channel 0) of every cell outside its
 * image's extent is 0 in every head, as the packers leave it.  Outputs, status bits, `stages`
 * and the workspace contract are pp_decode_multi's at the containers' sizes
 * (pp_decode_multi_workspace_size / _zero_offset / _work_offset).  With one CIF and one CAF
 * entry of one (H, W) and stride it is pp_decode_ragged, byte for byte.
 * Refused before anything touches HIP: PP_EINVAL for a NULL table, d_cifhr != NULL (no layout,
 * as pp_decode_ragged), a negative cif_threshold, seed_threshold, caf_threshold or
 * complete_caf_threshold, or a PP_ROLE_HRMAP entry (the map is CIF head 0's); PP_ESHAPE for an
 * extent <= 0 or beyond its entry's (H, W).  n_img == 0 is PP_OK.  pp_decode_initial has no
 * ragged form.
 * Reference interface: openpifpaf.decoder.CifCaf.__call__ (cifcaf.py:67-122) per image.
 *
 * pp_fields_pack_ragged_heads fills the containers of all n_heads heads (at most
 * 2 * PP_MAX_SCALES, in pp_scale entry order) in one launch.  HOST arguments: `fields`
 * (n_heads, n_img) device pointers, head m's image i a contiguous float32
 * (planes[m], h, w); `extents` (n_heads, n_img, 2); `planes` (n_heads) = n_fields * channels;
 * `sizes` (n_heads, 2) the containers' (H, W); `d_containers` (n_heads) device pointers, each
 * 4-byte aligned.  The two tables are copied into d_tables
 * (pp_ragged_heads_tables_size(n_img, n_heads) bytes, 8-byte aligned) on the stream, pointers
 * first, in ONE copy when `extents` lies right behind `fields` in host memory (at byte
 * pp_ragged_heads_extents_offset(n_img, n_heads) of one block), else in two; afterwards the
 * device extent table pp_decode_multi_ragged takes is at d_tables + that offset.  Host
 * tables as for pp_fields_pack_ragged (pageable: consumed before the call returns; pinned:
 * when the stream reaches the copy).  Every container element is written exactly once, as
 * pp_fields_pack_ragged writes it, so no container needs a memset.  PP_ESHAPE: n_heads out of
 * range, an extent <= 0 or larger than its head's container.  Both size functions return 0
 * for n_img <= 0 or n_heads outside 1 .. 2 * PP_MAX_SCALES.
 */
size_t pp_ragged_heads_tables_size(int32_t n_img, int32_t n_heads);
size_t pp_ragged_heads_extents_offset(int32_t n_img, int32_t n_heads);
int pp_fields_pack_ragged_heads(const float *const *fields, const int32_t *extents, int32_t n_img,
                                int32_t n_heads, const int32_t *planes, const int32_t *sizes,
                                float *const *d_containers, void *d_tables, size_t tables_bytes,
                                void *stream);
int pp_decode_multi_ragged(const pp_scale *scales, int32_t n_scales, int32_t cif_pairs,
                           int32_t n_img, int32_t K, int32_t C, const int32_t *d_extents,
                           const int32_t *extents, const int32_t *skeleton, const pp_config *cfg,
                           float *d_cifhr, pp_ann *d_anns, int32_t ann_capacity,
                           int32_t *d_counts, int32_t *d_status, void *d_workspace,
                           size_t workspace_bytes, uint32_t stages, void *stream);
/*
 * pp_cifdet_decode_ragged: pp_cifdet_decode over a ragged batch, one detection head without a
 * min scale.  d_det is the container (n_img, K, 7, H, W) (pp_fields_pack_ragged with channels
 * 7, or pp_fields_from_conv_ragged with layout 2, CifDet), d_extents / extents the device and
 * host tables as pp_decode_ragged takes them.  Image i's records are, bit for bit, those of
 * pp_cifdet_decode of the image alone at its own size; pp_det.image is its position in the
 * batch.  The image's own CifHr size decides the splat box clip of CifDetHr.accumulate
 * (cif_hr.py:84-100), the bounds of scalar_values in CifDetSeeds.fill_cif
 * (cif_seeds.py:67-90) and Occupancy(cifhr.shape, 2, min_scale=2.0) (cifdet.py:38-45);
 * workspace (pp_cifdet_ragged_workspace_size), capacities, outputs and status bits are
 * pp_cifdet_decode's at the container's (H, W).
 * d_cifhr (optional) receives the dense map (n_img, K, (H - 1) * stride + 1, pitch) at the
 * container's size: image i's own map in the top-left H'_i x W'_i of its planes, +0.0f in
 * every other element.
 * PP_ESHAPE: an extent <= 0 or larger than the container.  PP_EINVAL: a negative
 * cif_threshold or seed_threshold (cells outside an extent must pass no `c > threshold`).
 * Every argument error is returned before any launch.
 */
size_t pp_cifdet_ragged_workspace_size(int32_t n_img, int32_t K, int32_t H, int32_t W,
                                       const pp_config *cfg, int32_t det_capacity);
int pp_cifdet_decode_ragged(const float *d_det, int32_t n_img, int32_t K, int32_t H, int32_t W,
                            const int32_t *d_extents, const int32_t *extents,
                            const pp_config *cfg, const pp_det_nms *nms, float *d_cifhr,
                            pp_det *d_out, int32_t det_capacity, int32_t *d_counts,
                            int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                            void *stream);

/* ---------------------------------------------------------------------------------
 * openpifpaf.functional primitives (functional.pyx).  `field` arguments are
 * (h, w) float32 with row pitch `pitch` (elements).  Point lists are length-n device
 * arrays.  All are bit-exact restatements run as HIP kernels.
 * --------------------------------------------------------------------------------- */

/* functional.pyx:105-141 */
int pp_scalar_square_add_gauss_with_max(float *d_field, int64_t h, int64_t w, int64_t pitch,
                                        const float *d_x, const float *d_y,
                                        const float *d_sigma, const float *d_v, int64_t n,
                                        float truncate, float max_value, void *stream);
/* functional.pyx:71-102 */
int pp_scalar_square_add_gauss(float *d_field, int64_t h, int64_t w, int64_t pitch,
                               const float *d_x, const float *d_y, const float *d_sigma,
                               const float *d_v, int64_t n, float truncate, void *stream);
/* functional.pyx:7-26 */
int pp_scalar_square_add_constant(float *d_field, int64_t h, int64_t w, int64_t pitch,
                                  const float *d_x, const float *d_y, const float *d_width,
                                  const float *d_v, int64_t n, void *stream);
/* functional.pyx:144-169 */
int pp_scalar_square_max_gauss(float *d_field, int64_t h, int64_t w, int64_t pitch,
                               const float *d_x, const float *d_y, const float *d_sigma,
                               const float *d_v, int64_t n, float truncate, void *stream);
/* functional.pyx:29-54 */
int pp_cumulative_average(float *d_cuma, float *d_cumw, int64_t h, int64_t w, int64_t pitch,
                          const float *d_x, const float *d_y, const float *d_width,
                          const float *d_v, const float *d_w, int64_t n, void *stream);
/* functional.pyx:172-211: x (n, d) row pitch x_pitch, y (>=2) updated in place,
 * d_denom (n) out; d_out_steps (1 int32) = iterations run */
int pp_weiszfeld_nd(const float *d_x, int64_t n, int64_t d, int64_t x_pitch, float *d_y,
                    const float *d_weights, float epsilon, int64_t max_steps, float *d_denom,
                    void *stream);
/* functional.pyx:231-244 */
int pp_scalar_values(const float *d_field, int64_t h, int64_t w, int64_t pitch,
                     const float *d_x, const float *d_y, int64_t n, float default_value,
                     float *d_out, void *stream);
/*
 * Single-point lookups, batched (functional.pyx:247-286).  mode:
 *   0 scalar_value(default)  1 scalar_value_clipped  (float field, float out)
 *   2 scalar_nonzero(default) 3 scalar_nonzero_clipped 4 ..._with_reduction(r)  (u8 field)
 */
int pp_scalar_lookup(const void *d_field, int64_t h, int64_t w, int64_t pitch, int32_t mode,
                     const float *d_x, const float *d_y, int64_t n, float default_value,
                     float reduction, void *d_out, void *stream);
/*
 * Occupancy.set (decoder/occupancy.py:36-44) with scalar_square_add_single
 * (decoder/utils.py:61-66) for n marks, in order: plane d_f[i] of d_occ (n_planes, h, w) u8
 * with row pitch `pitch` gets += 1 (wrapping) on the box of half-width
 * round(max(min_scale_reduced, sigma / reduction)) around (round(x / reduction),
 * round(y / reduction)); f32 division, round half to even, NumPy slice clipping.  Marks
 * with d_f[i] outside [0, n_planes) are skipped, as the reference's early return; marks
 * with non-finite coordinates are skipped (the reference's round() raises).  Occupancy.get
 * is pp_scalar_lookup mode 4.
 */
int pp_occupancy_set(uint8_t *d_occ, int32_t n_planes, int64_t h, int64_t w, int64_t pitch,
                     const int32_t *d_f, const float *d_x, const float *d_y, const float *d_sigma,
                     int64_t n, float reduction, float min_scale_reduced, void *stream);

/*
 * Column filters over a (rows, n) field with row pitch `pitch` (functional.pyx:214-228,
 * 289-359), order preserving.  mode: 0 caf_center_s, 1 paf_center, 2 paf_center_b,
 * 3 paf_mask_center (d_out = u8 mask (n)).  Modes 0-2 write the kept columns to
 * d_out (rows, out_pitch) and the kept count to d_count (1 int32).
 */
int pp_center_filter(const float *d_field, int64_t rows, int64_t n, int64_t pitch, int32_t mode,
                     float x, float y, float sigma, void *d_out, int64_t out_pitch,
                     int32_t *d_count, void *stream);

/*
 * CifCaf._grow_connection + _target_with_blend / _target_with_maxscore
 * (cifcaf.py:124-192; the north star's "grow_connection_blend") for one query point on a
 * (9, n) column set with row pitch `pitch`.  method bit 0: 0 blend, 1 max; bit 1: the
 * scores' np.exp correctly rounded (pp_config.exp_mode 1) instead of NumPy's SIMD exp.
 * d_out = 4 floats (x, y, scale, score); all zero when no column lies in the 2*xy_scale box.
 */
int pp_grow_connection(const float *d_cols, int64_t n, int64_t pitch, float x, float y,
                       float xy_scale, int32_t method, float *d_out, void *stream);

/*
 * np.exp of float32 values as the decoder's CAF scores take it (cifcaf.py:139, the
 * score's exp): d_y[i] = exp(d_x[i]) with pp_config.exp_mode's rounding (0 NumPy's SIMD
 * float32 routine, 1 correctly rounded).  The device form of the decoder's own function
 * (caf_exp, pp_common.hpp), for checking it against np.exp.
 */
int pp_np_exp(const float *d_x, float *d_y, int64_t n, int32_t exp_mode, void *stream);

/*
 * d_y[i] = d_x[i] ** 2 as NumPy computes it for a float32 SCALAR (cifcaf.py:139 `sigma**2`):
 * the C library's powf(x, 2.0f), glibc 2.35's FMA build, which differs from x * x in about
 * 0.07 % of inputs.  The device form of the decoder's own function (np_pow2_f32).
 */
int pp_np_square(const float *d_x, float *d_y, int64_t n, void *stream);

/*
 * One query of pp_connection_values / pp_p2p_values: the source joint (x, y, v, s) = an
 * annotation's data[start_i] and joint_scales[start_i]; for pp_p2p_values the target joint
 * (tx, ty, ts) = target_xysv[:3]; `set` = the column set the query reads.
 */
typedef struct pp_edge_query {
    float x, y, v, s;
    float tx, ty, ts; /* unused by pp_connection_values */
    int32_t set;
} pp_edge_query;

/*
 * CifCaf.connection_value (cifcaf.py:194-217) for n_q queries in one launch, one wave per
 * query, no host synchronisation.  Column sets: set i is a (9, d_counts[i]) array at
 * d_cols + i * set_stride with row pitch `pitch` (set_stride >= 9 * pitch), i in
 * [0, n_sets).  The (n_caf, 2, 9, cap) / (n_caf, 2) output of pp_caf_scored or
 * pp_caf_scored_multi for one or many images is this layout without a copy: set_stride =
 * 9 * cap, pitch = cap, set = ((image * n_caf) + caf_i) * 2 + direction, direction 1 =
 * forward.  A query grows from (x, y) with scale max(0, s) over its set (caf_f,
 * cifcaf.py:124-192 as pp_grow_connection), applies keypoint_threshold to sqrt(score * v)
 * and the zero-score exit, and with reverse_match grows back from the new point over the
 * opposite direction's set, set ^ 1 (caf_b; n_sets must then be even), testing the
 * reverse result's SCALE against 0 as cifcaf.py:212 does, then the L1 distance against
 * the source scale.  method as pp_grow_connection.  d_out = (n_q, 4) floats (x, y, scale,
 * score), all zero where the reference returns its zero tuple.  A set index outside
 * [0, n_sets) reads as an empty set and a count is held to [0, pitch] (the device entry
 * cannot refuse what lies in device memory; the host twin returns PP_EINVAL for such an
 * index).  n_q == 0 returns PP_OK without a launch.
 */
int pp_connection_values(const float *d_cols, int64_t set_stride, int64_t pitch,
                         const int32_t *d_counts, int32_t n_sets, const pp_edge_query *d_queries,
                         int64_t n_q, int32_t method, float keypoint_threshold,
                         int32_t reverse_match, float *d_out, void *stream);

/*
 * CifCaf.p2p_value (cifcaf.py:219-245) for n_q queries in one launch; sets and queries as
 * pp_connection_values (only method bit 1, the exp mode, matters).  Per column of the
 * query's set inside the caf_center_s box of 2 * max(0, s) around (x, y): exp(-0.5 d_s^2
 * / sigma_s^2) * exp(-0.5 d_t^2 / sigma_t^2) * v, sigma = 0.5 * max(0, scale); d_out[q] =
 * sqrt(v * max(scores)), 0.0 when no column is kept.  max is Python's max() over the kept
 * columns in column order (cifcaf.py:245): it keeps its first element unless a later one
 * compares greater, so the result is NaN exactly when the first kept column's score is
 * NaN, and a NaN score of any later column is ignored.  d_out = (n_q) floats.
 */
int pp_p2p_values(const float *d_cols, int64_t set_stride, int64_t pitch, const int32_t *d_counts,
                  int32_t n_sets, const pp_edge_query *d_queries, int64_t n_q, int32_t method,
                  float *d_out, void *stream);

/* ---------------------------------------------------------------------------------
 * Host twins of the functional.pyx primitives above (SURVEY.md §8(b) `_cpu` variants):
 * the same arguments as the device entry points minus the stream, HOST pointers, run
 * sequentially on the calling thread in the reference's loop order (functional.pyx is
 * CPU-only Cython), bit-exact with it and with the kernels.  Explicit entry points only:
 * nothing in the library or its Python API falls back to them.
 * --------------------------------------------------------------------------------- */
int pp_scalar_square_add_gauss_with_max_cpu(float *field, int64_t h, int64_t w, int64_t pitch,
                                            const float *x, const float *y, const float *sigma,
                                            const float *v, int64_t n, float truncate,
                                            float max_value);
int pp_scalar_square_add_gauss_cpu(float *field, int64_t h, int64_t w, int64_t pitch,
                                   const float *x, const float *y, const float *sigma,
                                   const float *v, int64_t n, float truncate);
int pp_scalar_square_max_gauss_cpu(float *field, int64_t h, int64_t w, int64_t pitch,
                                   const float *x, const float *y, const float *sigma,
                                   const float *v, int64_t n, float truncate);
int pp_scalar_square_add_constant_cpu(float *field, int64_t h, int64_t w, int64_t pitch,
                                      const float *x, const float *y, const float *width,
                                      const float *v, int64_t n);
int pp_cumulative_average_cpu(float *cuma, float *cumw, int64_t h, int64_t w, int64_t pitch,
                              const float *x, const float *y, const float *width,
                              const float *v, const float *w_, int64_t n);
/* pp_np_exp / pp_np_square on host pointers */
int pp_np_exp_cpu(const float *x, float *y, int64_t n, int32_t exp_mode);
int pp_np_square_cpu(const float *x, float *y, int64_t n);
/* out_steps (optional, 1 int64) = iterations run */
int pp_weiszfeld_nd_cpu(const float *x, int64_t n, int64_t d, int64_t x_pitch, float *y,
                        const float *weights, float epsilon, int64_t max_steps, float *denom,
                        int64_t *out_steps);
int pp_scalar_values_cpu(const float *field, int64_t h, int64_t w, int64_t pitch, const float *x,
                         const float *y, int64_t n, float default_value, float *out);
int pp_scalar_lookup_cpu(const void *field, int64_t h, int64_t w, int64_t pitch, int32_t mode,
                         const float *x, const float *y, int64_t n, float default_value,
                         float reduction, void *out);
int pp_occupancy_set_cpu(uint8_t *occ, int32_t n_planes, int64_t h, int64_t w, int64_t pitch,
                         const int32_t *f, const float *x, const float *y, const float *sigma,
                         int64_t n, float reduction, float min_scale_reduced);
int pp_center_filter_cpu(const float *field, int64_t rows, int64_t n, int64_t pitch, int32_t mode,
                         float x, float y, float sigma, void *out, int64_t out_pitch,
                         int32_t *count);
/* pp_connection_values / pp_p2p_values (cifcaf.py:194-245) on host pointers, byte-identical
 * with the kernels; a query whose set index lies outside [0, n_sets) is PP_EINVAL */
int pp_connection_values_cpu(const float *cols, int64_t set_stride, int64_t pitch,
                             const int32_t *counts, int32_t n_sets, const pp_edge_query *queries,
                             int64_t n_q, int32_t method, float keypoint_threshold,
                             int32_t reverse_match, float *out);
int pp_p2p_values_cpu(const float *cols, int64_t set_stride, int64_t pitch, const int32_t *counts,
                      int32_t n_sets, const pp_edge_query *queries, int64_t n_q, int32_t method,
                      float *out);

/* ---------------------------------------------------------------------------------
 * Host twins of the front stages (csrc/stages_cpu.hip): pp_cifhr / pp_seeds /
 * pp_caf_scored for one CIF and one CAF head with the same layouts, HOST pointers, run on
 * the calling thread in the reference's order (the stage classes are CPU-only NumPy code).
 * Explicit entry points only, as the primitives' twins above.
 *   pp_cifhr_cpu       CifHr.fill / fill_cif (cif_hr.py:23-81): cifhr (n_img, K, H', pitch),
 *                      pitch = pp_cifhr_pitch(W'), zeroed then accumulated
 *   pp_seeds_cpu       CifSeeds.fill + get (cif_seeds.py:23-64): seeds (n_img, seed_capacity)
 *                      sorted as sorted(seeds, reverse=True), counts (n_img); PP_ESHAPE when
 *                      an image has more than seed_capacity seeds
 *   pp_caf_scored_cpu  CafScored.fill (caf_scored.py:32-98) at score_th: cols
 *                      (n_img, C, 2, 9, H*W), dir 0 backward, 1 forward; counts (n_img, C, 2)
 * --------------------------------------------------------------------------------- */
int pp_cifhr_cpu(const float *cif, int32_t n_img, int32_t K, int32_t H, int32_t W,
                 const pp_config *cfg, float *cifhr);
int pp_seeds_cpu(const float *cif, const float *cifhr, int32_t n_img, int32_t K, int32_t H,
                 int32_t W, const pp_config *cfg, pp_seed *seeds, int32_t seed_capacity,
                 int32_t *counts);
int pp_caf_scored_cpu(const float *caf, const float *cifhr, int32_t n_img, int32_t K, int32_t C,
                      int32_t H, int32_t W, const int32_t *skeleton, float score_th,
                      const pp_config *cfg, float *cols, int32_t *counts);
/* nms.Keypoints.annotations (nms.py:17-57) as pp_nms_keypoints, on host records (no workspace):
 * anns edited in place, survivors sorted by -score in out with their score, out_counts,
 * out_index (optional) = each survivor's input index. */
int pp_nms_keypoints_cpu(pp_ann *anns, const int32_t *counts, int32_t n_img, int32_t K,
                         int32_t ann_capacity, const pp_config *cfg, pp_ann *out,
                         int32_t *out_counts, int32_t *out_index);
/* pp_nms_keypoints_scored on host records (each record's own Annotation.score()). */
int pp_nms_keypoints_scored_cpu(pp_ann *anns, const int32_t *counts, int32_t n_img, int32_t K,
                                int32_t ann_capacity, const pp_config *cfg,
                                double instance_threshold, const int32_t *score_spec,
                                const double *score_weights, const double *fixed_score,
                                pp_ann *out, int32_t *out_counts, int32_t *out_index);

/*
 * Host twin of pp_decode_batch (CifCaf.__call__, cifcaf.py:67-122, for a batch of one-head
 * fields; no initial annotations): CifHr, seeds and both CafScored sets through the front
 * stages' twins, the seed loop with its occupancy, _grow, complete_annotations with
 * _flood_fill (force_complete) and nms.Keypoints (apply_nms), on HOST pointers, one image
 * per task on n_threads host threads (0: one per hardware thread).  Outputs as
 * pp_decode_batch: per image ann_capacity records (counts[i] of them used, sorted by
 * nms.Keypoints) and status flags (PP_ST_*; PP_ST_ANN_OVERFLOW: more annotations than
 * ann_capacity, retry with a larger one).  Bit-exact with the device decode and with the
 * reference's fixtures (tests/test_decode_cpu.py).
 */
int pp_decode_batch_cpu(const float *cif, const float *caf, int32_t n_img, int32_t K, int32_t C,
                        int32_t H, int32_t W, const int32_t *skeleton, const pp_config *cfg,
                        pp_ann *anns, int32_t ann_capacity, int32_t *counts, int32_t *status,
                        int32_t n_threads);

/*
 * Host twin of pp_decode_ragged and the definition of a ragged decode: image i is the
 * extents[i] = (h_i, w_i) top-left crop of its container planes, decoded by
 * pp_decode_batch_cpu's per-image decode at that size.  Same argument checks as
 * pp_decode_ragged (extents on the host).
 */
int pp_decode_ragged_cpu(const float *cif, const float *caf, int32_t n_img, int32_t K, int32_t C,
                         int32_t H, int32_t W, const int32_t *extents, const int32_t *skeleton,
                         const pp_config *cfg, pp_ann *anns, int32_t ann_capacity,
                         int32_t *counts, int32_t *status, int32_t n_threads);

/*
 * Eval preprocessing (eval_coco.py:350-389 preprocess_factory without its options:
 * RescaleAbsolute scale.py:113-134, CenterPad / CenterPadTight pad.py:12-111, EVAL_TRANSFORM
 * transforms/__init__.py:20-27) of a batch of uint8 RGB images of different sizes in one launch.
 *
 * d_src holds the packed source images, each (h, w, 3) interleaved as PIL / np.asarray give
 * them.  descs is a HOST table of n_img descriptors: it is checked on the host, extended by
 * the zoom factors and the per-image first workgroup (a prefix sum) and staged into d_tables
 * (pp_preprocess_tables_size(n_img) bytes, 8-byte aligned) beside the value table below, so
 * the kernel reads its descriptors from the device.  Image i is resized to (th, tw) exactly
 * as scipy.ndimage.zoom(im, (th / h, tw / w, 1), order=1) resizes uint8 (float64, every
 * operation in scipy's order, no contraction; where the last coordinate rounds above h - 1
 * or w - 1 the last row or column is 0, scipy's constant mode), pasted at (top, left) into an
 * (H, W) output filled with `fill`, and every pixel mapped through
 * ((float)u8 / 255.0f - mean[c]) / std[c], each one IEEE float32 operation, looked up in a
 * 3 x 256 table the host computes (the device divides nothing).
 *   dtype  PP_PRE_F32 / PP_PRE_F16 / PP_PRE_BF16: the float32 value, or its round-to-nearest-
 *          even float16 / bfloat16; PP_PRE_U8: the padded uint8 image itself, always (H, W, 3)
 *          (the image the reference holds before ToTensor; mean and std unused but checked)
 *   layout PP_PRE_PLANAR (3, H, W) or PP_PRE_CHANNELS_LAST (H, W, 3) at out_offset
 * src_offset counts bytes, out_offset and out_elems elements of the output type.
 * PP_ESHAPE: n_img < 0, a source or target edge < 2, a source image beyond 2^31 - 1 bytes,
 * H or W <= 0 (or H * W beyond 2^29), a
 * target that does not fit its output with the given pad, a source image or an output region
 * beyond its buffer.  PP_EINVAL: an unknown dtype or layout, a NULL pointer with n_img > 0, a
 * std entry that is 0 or not finite, an output pointer not aligned to its type, a misaligned
 * d_tables.  PP_ENOMEM: tables_bytes too small.  n_img == 0 succeeds and launches nothing.
 * pp_preprocess_images_cpu is the host twin on host pointers (same checks, same per-pixel
 * code: bit-identical outputs).
 */
enum { PP_PRE_F32 = 0, PP_PRE_F16 = 1, PP_PRE_BF16 = 2, PP_PRE_U8 = 3 };
enum { PP_PRE_PLANAR = 0, PP_PRE_CHANNELS_LAST = 1 };
typedef struct pp_image_desc {
    int64_t src_offset;   /* first byte of the source image in the source buffer     */
    int64_t out_offset;   /* first element of the image's output region              */
    int32_t h, w;         /* source size                                              */
    int32_t th, tw;       /* size after the rescale (th == h, tw == w: no rescale)    */
    int32_t left, top;    /* pad before the rescaled image                            */
    int32_t H, W;         /* output size                                              */
} pp_image_desc;
size_t pp_preprocess_tables_size(int32_t n_img);
int pp_preprocess_images(const uint8_t *d_src, int64_t src_bytes, const pp_image_desc *descs,
                         int32_t n_img, void *d_out, int64_t out_elems, int32_t dtype,
                         int32_t layout, const float *mean, const float *std,
                         const uint8_t *fill, void *d_tables, size_t tables_bytes, void *stream);
int pp_preprocess_images_cpu(const uint8_t *src, int64_t src_bytes, const pp_image_desc *descs,
                             int32_t n_img, void *out, int64_t out_elems, int32_t dtype,
                             int32_t layout, const float *mean, const float *std,
                             const uint8_t *fill);

/*
 * Eval preprocessing with the options of eval_coco.preprocess_factory and the input pyramid
 * of a multi-scale model, in one launch: the chain of pp_preprocess_images, then
 *   * a turn of the square padded image by rot * 90 degrees (eval_coco.py:376-384
 *     --orientation-invariant, transforms/rotate.py:42-52 RotateBy90's swapaxes and flips):
 *     with N = H = W and `canvas` the padded image,
 *       rot 1: T[y][x] = canvas[x][N-1-y]; rot 2: canvas[N-1-y][N-1-x]; rot 3: canvas[N-1-x][y];
 *   * the reduced inputs of network/nets.py:111-131 ShellMultiScale.forward: `reductions` is
 *     a mask of PP_VIEW_R1 (every pixel), PP_VIEW_R1_5 (rows and columns with i % 3 != 2, at
 *     i - i / 3), PP_VIEW_R2, PP_VIEW_R3, PP_VIEW_R5 (i % r == 0, at i / r); with `mirror`
 *     each is followed by its torch.flip(dims=[3]) (column sx at n - 1 - sx, channels not
 *     swapped).  The views are ordered as nets.py:115-116 orders them: the selected reductions
 *     ascending, then (mirror) the same mirrored: n_views = popcount(reductions) * (mirror ?
 *     2 : 1).  PP_VIEW_R1 alone without mirror is the plain turned image.
 * --extended-scale (eval_coco.py:359-366) needs nothing here: every image carries its own
 * rescaled size (th, tw) and pad.
 * images is a HOST table (pp_view_image: pp_image_desc without out_offset, with rot);
 * view_offsets a HOST (n_img, n_views) table: the first element of image i's region in view
 * v inside d_out, a region being (3, n_r, n_c) or (n_r, n_c, 3) elements with n = ceil(N / r),
 * or N - N / 3 for reduction 1.5.  Both are checked on the host and staged into d_tables
 * (pp_preprocess_views_tables_size(n_img, n_views) bytes, 8-byte aligned) with the value
 * table.  dtype, layout, mean, std, fill, src_offset and out_elems as pp_preprocess_images.
 * Each padded pixel is computed once and stored into every view that keeps it.
 * PP_ESHAPE: everything pp_preprocess_images refuses with it, rot != 0 with H != W, more
 * than PP_VIEW_R1 alone (or mirror) with H != W, a view region beyond the output buffer.
 * PP_EINVAL: an empty or unknown reduction mask, rot outside 0..3, an unknown dtype or layout, a
 * NULL pointer with n_img > 0, a std entry that is 0 or not finite, a misaligned output or
 * d_tables.  PP_ENOMEM: tables_bytes too small.  n_img == 0 succeeds and launches nothing.
 */
enum { PP_VIEW_R1 = 1, PP_VIEW_R1_5 = 2, PP_VIEW_R2 = 4, PP_VIEW_R3 = 8, PP_VIEW_R5 = 16 };
typedef struct pp_view_image {
    int64_t src_offset;   /* first byte of the source image in the source buffer     */
    int32_t h, w;         /* source size                                              */
    int32_t th, tw;       /* size after the rescale (th == h, tw == w: no rescale)    */
    int32_t left, top;    /* pad before the rescaled image                            */
    int32_t H, W;         /* padded size                                              */
    int32_t rot;          /* 0, 1, 2, 3: turned by 0, 90, 180, 270 degrees            */
    int32_t reserved;     /* 0                                                        */
} pp_view_image;
/* bytes of d_tables for n_img images and n_views views (0 when either is <= 0) */
size_t pp_preprocess_views_tables_size(int32_t n_img, int32_t n_views);
/* eval_coco.py:359-384 and nets.py:111-131 on the device, one launch on `stream` */
int pp_preprocess_views(const uint8_t *d_src, int64_t src_bytes, const pp_view_image *images,
                        const int64_t *view_offsets, int32_t n_img, int32_t reductions,
                        int32_t mirror, void *d_out, int64_t out_elems, int32_t dtype,
                        int32_t layout, const float *mean, const float *std, const uint8_t *fill,
                        void *d_tables, size_t tables_bytes, void *stream);
/* the host twin of pp_preprocess_views on host pointers: the same checks and the same
 * per-pixel code (eval_coco.py:359-384, nets.py:111-131), bit-identical outputs */
int pp_preprocess_views_cpu(const uint8_t *src, int64_t src_bytes, const pp_view_image *images,
                            const int64_t *view_offsets, int32_t n_img, int32_t reductions,
                            int32_t mirror, void *out, int64_t out_elems, int32_t dtype,
                            int32_t layout, const float *mean, const float *std,
                            const uint8_t *fill);

/*
 * CIF and CAF target encoders (openpifpaf/encoder/cif.py, caf.py, annrescaler.py and
 * utils.py:6-37 create_sink, mask_valid_area) for a batch of images in one launch per
 * encoder.  The tensors are bit for bit the reference's (NumPy 2 promotion rules, NaN as
 * 0x7FC00000).
 *
 * All inputs are HOST tables.  The call checks them, restates the per-annotation scalars
 * of the reference on the host (annrescaler.py:39-47 keypoint_sets /= stride, 49-75 bg_mask
 * boxes, 77-109 scale; cif.py:87-101 max_r by quadrant, 113-114 joint_scale, 119-126 the
 * patch's place and offset; caf.py:100-114 shortest_sparse, 124-144 the dense-to-sparse and
 * field-of-view tests, 164-177 offset, num, fmargin and the linspace), stages the resulting
 * job lists into d_tables on `stream` (pp_encode_*_tables_size bytes are always enough;
 * 8-byte aligned) and launches one kernel, asynchronously.  The rasterisation
 * (cif.py:129-145, caf.py:180-222) and fields() (cif.py:147-162, caf.py:224-246: the crop
 * of the padding, the bg_mask NaN, mask_valid_area) are the kernel: every output element is
 * stored exactly once, nothing is cleared first.
 *
 *   images     n_img records: pixel size, the field size (h, w) = ((height - 1) / stride + 1,
 *              (width - 1) / stride + 1), meta['valid_area'] in pixels (x, y, w, h) when
 *              has_valid_area, the image's annotations anns[ann0 .. ann0 + n_ann) and the
 *              first element of each of its output tensors in d_out:
 *                CIF  (K, h, w), (K, 6, h, w), (K, h, w)                       out_offset[0..2]
 *                CAF  (C, h, w), (C, 6, h, w), (C, 6, h, w), (C, h, w), (C, h, w)   [0..4]
 *              all float32.  Images of one size whose regions are adjacent per tensor stack
 *              to (B, ...).
 *   anns       per annotation: bbox (x, y, w, h) float32 in pixels, iscrowd, and flags
 *              PP_ENC_HAS_KEYPOINTS / PP_ENC_HAS_BBOX ('keypoints' in ann, 'bbox' in ann)
 *   keypoints  (n_ann, K, 3) float32 (x, y, v) in pixels; rows of annotations without
 *              keypoints are not read
 *   enc        the encoder: pose and pose_45 (K, 2) doubles (annrescaler.py:18-26; the
 *              total areas are derived here), sigmas (K doubles, used as Python floats, or
 *              NULL), v_threshold, side (Cif.side_length / Caf.min_size, 1..8), padding
 *              (0..64), stride; for CAF the 1-based skeleton (C, 2), the sparse skeleton
 *              (n_sparse, 2) or NULL, dense_to_sparse_radius, only_in_field_of_view,
 *              fixed_size and aspect_ratio.
 *
 * Refused before any launch.  PP_EINVAL: a NULL argument, a misaligned or NULL table block,
 * aspect_ratio != 0 ("aspect_ratio": the patch side would grow with the limb; not built), a
 * non-finite coordinate of a joint with v > v_threshold, an annotation that the reference
 * would need a key from that it lacks, a joint scale <= 0 that reaches the reference's
 * `assert scale > 0.0` (cif.py:144, caf.py:219-221).  PP_ESHAPE: K outside [1, PP_MAX_KP],
 * C outside [1, PP_MAX_EDGES], a skeleton index outside 1..K, side outside 1..8, padding
 * outside 0..64, stride < 1, a field size that is not the pixel size's or beyond 16384, an
 * annotation range outside [0, n_ann), an output region outside d_out.  PP_ENOMEM:
 * tables_bytes too small.  n_img == 0 succeeds and launches nothing.
 *
 * pp_encode_cif_cpu / pp_encode_caf_cpu are the host twins on host pointers: the same plan
 * and the same per-cell code, one image per task on n_threads host threads (< 1: one).
 */
enum { PP_ENC_HAS_KEYPOINTS = 1, PP_ENC_HAS_BBOX = 2 };
typedef struct pp_enc_image {
    int64_t out_offset[5];  /* first element of each output tensor of this image         */
    double valid_area[4];   /* meta['valid_area'] (x, y, w, h) in pixels                 */
    int32_t has_valid_area; /* 'valid_area' in meta                                      */
    int32_t height, width;  /* pixels                                                    */
    int32_t h, w;           /* field size                                                */
    int32_t ann0, n_ann;    /* this image's annotations                                  */
    int32_t reserved;       /* 0                                                         */
} pp_enc_image;
typedef struct pp_enc_ann {
    float bbox[4];
    int32_t iscrowd;
    int32_t flags;          /* PP_ENC_HAS_*                                              */
} pp_enc_ann;
typedef struct pp_encoder {
    const double *pose;             /* (K, 2) */
    const double *pose_45;          /* (K, 2) */
    const double *sigmas;           /* (K) or NULL */
    const int32_t *skeleton;        /* CAF: (C, 2), 1-based */
    const int32_t *sparse_skeleton; /* CAF: (n_sparse, 2), 1-based, or NULL */
    double v_threshold;
    double dense_to_sparse_radius;
    double aspect_ratio;            /* must be 0 */
    int32_t stride, K, C, n_sparse;
    int32_t side;                   /* Cif.side_length / Caf.min_size */
    int32_t padding;
    int32_t only_in_field_of_view, fixed_size;
} pp_encoder;
/* bytes of d_tables that are enough for any batch of n_img images and n_ann annotations */
size_t pp_encode_cif_tables_size(int32_t n_img, int32_t n_ann, int32_t K);
size_t pp_encode_caf_tables_size(int32_t n_img, int32_t n_ann, int32_t C);
/* float32 elements of one image's tensors together: 8 K h w and 15 C h w (0: bad shape) */
int64_t pp_encode_cif_output_size(int32_t h, int32_t w, int32_t K);
int64_t pp_encode_caf_output_size(int32_t h, int32_t w, int32_t C);
/* encoder/cif.py:25-162 CifGenerator for a batch, one launch on `stream` */
int pp_encode_cif(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                  const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *d_out,
                  int64_t out_elems, void *d_tables, size_t tables_bytes, void *stream);
/* encoder/caf.py:32-246 CafGenerator for a batch, one launch on `stream` */
int pp_encode_caf(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                  const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *d_out,
                  int64_t out_elems, void *d_tables, size_t tables_bytes, void *stream);
int pp_encode_cif_cpu(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                      const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *out,
                      int64_t out_elems, int32_t n_threads);
int pp_encode_caf_cpu(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                      const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *out,
                      int64_t out_elems, int32_t n_threads);
/* the twins' helpers, for tests against NumPy: np.linalg.norm of n float32 pairs (caf.py:111,
 * 165; cif.py:99) and np.linspace(start, stop, num) for num >= 2 (caf.py:177) */
int pp_encode_norm_cpu(const float *xy, float *out, int64_t n);
int pp_encode_linspace_cpu(double start, double stop, int32_t num, double *out);

#ifdef __cplusplus
}
#endif
#endif /* PIFPAF_AMD_H */

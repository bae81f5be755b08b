// coco.hpp — EvalCoco.from_predictions (eval_coco.py:108-158) per record: the pieces the
// gfx950 kernels (coco.hip) and their host twins (coco_cpu.hip) share, so the two cannot
// drift.  Every function is the reference's arithmetic in its order:
//   - Preprocess.annotations_inverse (preprocess.py:35-95) from inverse.hpp, the statement
//     inverse.hip's in-place kernels use, here per joint and without writing the record
//     back;
//   - Annotation.scale(v_th=0.01) (annotation.py:73-80), json_data (annotation.py:82-119)
//     and AnnotationDet.json_data (annotation.py:138-145).
// Rounding: a double that came from a float32 times 100.0 is exact (24 + 7 bits), so
// np.around(x, 2), round(x, 2) and rint(x * 100.0) / 100.0 are the same double; NumPy's
// scalar round(np.float64, 3) is multiply, rint, divide.
#pragma once

#include "inverse.hpp"

namespace pp {

// np.min / np.max of float32 values as a commutative, associative operation (so a wave
// reduction and a sequential loop give the same bits): NaN propagates, and of two equal
// values of either sign the minimum is the negative zero, the maximum the positive one
PP_HD float coco_min(float a, float b) {
    if (a != a || b != b) return NAN;
    if (a == b) return signbit(a) ? a : b;
    return a < b ? a : b;
}
PP_HD float coco_max(float a, float b) {
    if (a != a || b != b) return NAN;
    if (a == b) return signbit(a) ? b : a;
    return a > b ? a : b;
}

// np.around(float64(x), 2) == round(float(x), 2) of a float32 x.  A NaN comes out as the one
// quiet NaN 0x7ff8000000000000: which sign and payload an operation hands on differs between
// the host's and the device's arithmetic, and json prints every NaN alike.
PP_HD double coco_round2(float x) {
    const double r = rint((double)x * 100.0) / 100.0;
    return r != r ? f64_of(0x7ff8000000000000ull) : r;
}
// max(0.001, round(score, 3)) (annotation.py:93, 143): Python's max keeps its first
// argument unless the second is larger, so NaN gives 0.001
PP_HD double coco_score3(double s) {
    const double r = rint(s * 1000.0) / 1000.0;
    return r > 0.001 ? r : 0.001;
}

// _HorizontalSwap as a gather (hflip.py:17-29 scatters source rows to hswap[source], last
// writer wins, rows nobody writes stay zero): the source row of target row t, or -1
PP_HD int coco_swap_source(const int *hswap, int K, int t) {
    int src = -1;
    for (int sj = 0; sj < K; sj++)
        if (hswap[sj] == t) src = sj;
    return src;
}

// Row j of the record's data after annotations_inverse, with joint j's scale; src_of
// (K, or NULL without a swap) from coco_swap_source
PP_HD void coco_row(const pp_ann &a, const pp_inverse_meta &m, const InverseXf &t,
                    const int *src_of, int j, float &x, float &y, float &v, float &js) {
    const int src = src_of ? src_of[j] : j;
    js = inverse_jscale(m, a.joint_scales[j]);
    if (src < 0) {
        x = y = v = 0.0f;
        return;
    }
    x = a.data[src][0];
    y = a.data[src][1];
    v = a.data[src][2];
    bool nan = false;
    inverse_point(m, t, x, y, v, nan);
}

// Steps 1 and 2 of from_predictions for one record: whether it passes the small-object
// filter (always true with small_threshold == 0), and in `nan` whether the reference's
// NaN assert fires on it.  Annotation.scale(v_th=0.01) in float32 over the rows with
// v > 0.01f, compared with the threshold in float32 (NEP 50); without such a row the scale
// is the Python float 0.0, compared in float64.
PP_HD bool coco_keep(const pp_ann &a, int K, const pp_inverse_meta &m, const InverseXf &t,
                     const int *src_of, double small_threshold, bool &nan) {
    bool any = false;
    float x0 = 0.0f, x1 = 0.0f, y0 = 0.0f, y1 = 0.0f;
    for (int j = 0; j < K; j++) {  // the NaN test reads every source row
        float x = a.data[j][0], y = a.data[j][1];
        inverse_point(m, t, x, y, a.data[j][2], nan);
    }
    if (!(small_threshold != 0.0)) return true;
    for (int j = 0; j < K; j++) {
        float x, y, v, js;
        coco_row(a, m, t, src_of, j, x, y, v, js);
        if (!(v > 0.01f)) continue;
        x0 = any ? coco_min(x0, x) : x;
        x1 = any ? coco_max(x1, x) : x;
        y0 = any ? coco_min(y0, y) : y;
        y1 = any ? coco_max(y1, y) : y;
        any = true;
    }
    if (!any) return 0.0 >= small_threshold;
    const float ex = x1 - x0, ey = y1 - y0;
    const float scale = ey > ex ? ey : ex;  // Python's max(ex, ey)
    return scale >= (float)small_threshold;
}

// keypoints entry of json_data: v of visible joints raised to 0.01f (np.maximum)
PP_HD float coco_v(float v) { return v > 0.0f ? (v < 0.01f ? 0.01f : v) : v; }

PP_HD uint64_t coco_cat_word(int32_t category_id, int32_t second) {
    return (uint64_t)(uint32_t)category_id | ((uint64_t)(uint32_t)second << 32);
}

// The seven 8-byte words ahead of the keypoints (and the whole of a detection record):
// image_id, score, bbox[4], (category_id, n_keypoints | pad_)
constexpr int kCocoHeadWords = 7;
PP_HD int coco_record_words(int K) { return kCocoHeadWords + 3 * K; }

PP_HD void coco_dummy_head(int64_t image_id, int32_t second, uint64_t *w) {
    w[0] = (uint64_t)image_id;
    w[1] = u64_of(0.001);
    w[2] = u64_of(0.0);
    w[3] = u64_of(0.0);
    w[4] = u64_of(1.0);
    w[5] = u64_of(1.0);
    w[6] = coco_cat_word(1, second);
}

// anndet_inverse (inverse_box), then AnnotationDet.json_data (annotation.py:138-145)
PP_HD void coco_det_words(const pp_det &d, const pp_inverse_meta &m, const InverseXf &t,
                          int64_t image_id, uint64_t *w) {
    float b[4] = {d.bbox[0], d.bbox[1], d.bbox[2], d.bbox[3]};
    inverse_box(m, t, b);
    w[0] = (uint64_t)image_id;
    w[1] = u64_of(coco_score3((double)d.score));
    for (int i = 0; i < 4; i++) w[2 + i] = u64_of(coco_round2(b[i]));
    w[6] = coco_cat_word(d.field + 1, 0);
}

// records of one image that are looked at: the count clamped as ann_inverse_kernel clamps it
PP_HD int coco_clamp_count(int count, int cap) { return count < 0 ? 0 : (count < cap ? count : cap); }

// argument checks shared by the device entry points and the host twins (in coco_cpu.hip,
// which holds host code only)
int coco_check_args(const char *who, const void *recs, const void *counts, int32_t n_img,
                    int32_t capacity, int32_t K, const void *metas, const void *image_ids,
                    const pp_coco_params *params, const void *out, int64_t out_capacity,
                    const void *out_counts, const void *out_flags);

}  // namespace pp

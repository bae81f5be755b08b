// coco_cpu.hip — host twins of pp_coco_keypoints / pp_coco_dets (coco.hip): the same
// records, byte for byte, from HOST pointers on the calling thread.  Every value comes from
// coco.hpp's per-record functions, the ones the kernels call; only the control flow around
// them (a loop here, a workgroup there) is restated.  For callers holding host records, for
// instance compact records gathered from several GPUs; no product path falls back to them.
#include <cstring>
#include <string>

#include "coco.hpp"

namespace pp {

int coco_check_args(const char *who, const void *recs, const void *counts, int32_t n_img,
                    int32_t capacity, int32_t K, const void *metas, const void *image_ids,
                    const pp_coco_params *params, const void *out, int64_t out_capacity,
                    const void *out_counts, const void *out_flags) {
    const std::string w(who);
    if (!recs || !counts || !metas || !image_ids || !params || !out || !out_counts || !out_flags)
        return fail(PP_EINVAL, w + ": NULL argument");
    if (n_img < 0 || capacity <= 0 || out_capacity < 0)
        return fail(PP_ESHAPE, w + ": bad shape");
    if (K <= 0 || K > PP_MAX_KP) return fail(PP_ESHAPE, w + ": K outside [1, PP_MAX_KP]");
    if (params->max_per_image < 1) return fail(PP_ESHAPE, w + ": max_per_image < 1");
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_coco_keypoints_cpu(const pp_ann *anns, const int32_t *counts, int32_t n_img,
                          int32_t capacity, int32_t K, const pp_inverse_meta *metas,
                          const int64_t *image_ids, const int32_t *hswap,
                          const pp_coco_params *params, void *out, int64_t out_capacity,
                          int32_t *out_counts, int32_t *out_flags) {
    const int rc = coco_check_args("pp_coco_keypoints_cpu", anns, counts, n_img, capacity, K, metas,
                                   image_ids, params, out, out_capacity, out_counts, out_flags);
    if (rc != PP_OK) return rc;
    const int words = coco_record_words(K);
    int64_t at = 0;  // packed index of the next record
    for (int img = 0; img < n_img; img++) {
        const pp_inverse_meta &m = metas[img];
        const InverseXf t = inverse_xf(m);
        int table[PP_MAX_KP];
        const int *src_of = nullptr;
        if (m.hflip && hswap) {
            for (int j = 0; j < K; j++) table[j] = coco_swap_source(hswap, K, j);
            src_of = table;
        }
        const int n_rec = coco_clamp_count(counts[img], capacity);
        bool nan = false;
        int done = 0;
        for (int r = 0; r < n_rec; r++) {
            const pp_ann &a = anns[(int64_t)img * capacity + r];
            const bool keep = coco_keep(a, K, m, t, src_of, params->small_threshold, nan);
            if (!keep || done >= params->max_per_image) continue;
            uint64_t w[kCocoHeadWords + 3 * PP_MAX_KP];
            bool any = false;
            float bx = INFINITY, by = INFINITY, bxm = -INFINITY, bym = -INFINITY;
            for (int j = 0; j < K; j++) {
                float x, y, v, js;
                coco_row(a, m, t, src_of, j, x, y, v, js);
                w[kCocoHeadWords + 3 * j] = u64_of(coco_round2(x));
                w[kCocoHeadWords + 3 * j + 1] = u64_of(coco_round2(y));
                w[kCocoHeadWords + 3 * j + 2] = u64_of(coco_round2(coco_v(v)));
                if (!(v > 0.0f)) continue;
                any = true;
                bx = coco_min(bx, x - js);
                by = coco_min(by, y - js);
                bxm = coco_max(bxm, x + js);
                bym = coco_max(bym, y + js);
            }
            w[0] = (uint64_t)image_ids[img];
            w[1] = u64_of(coco_score3(a.score));
            w[2] = u64_of(any ? coco_round2(bx) : 0.0);
            w[3] = u64_of(any ? coco_round2(by) : 0.0);
            w[4] = u64_of(any ? coco_round2(bxm - bx) : 0.0);
            w[5] = u64_of(any ? coco_round2(bym - by) : 0.0);
            w[6] = coco_cat_word(params->category_id, K);
            if (at + done < out_capacity)
                std::memcpy((char *)out + (at + done) * 8 * (int64_t)words, w, 8 * (size_t)words);
            done++;
        }
        if (done == 0) {
            uint64_t w[kCocoHeadWords + 3 * PP_MAX_KP];
            coco_dummy_head(image_ids[img], K, w);
            for (int i = kCocoHeadWords; i < words; i++) w[i] = u64_of(0.0);
            if (at < out_capacity)
                std::memcpy((char *)out + at * 8 * (int64_t)words, w, 8 * (size_t)words);
        }
        out_counts[img] = done > 0 ? done : 1;
        out_flags[img] = (nan ? PP_COCO_NAN : 0) | (done > 0 ? 0 : PP_COCO_EMPTY);
        at += out_counts[img];
    }
    return PP_OK;
}

int pp_coco_dets_cpu(const pp_det *dets, const int32_t *counts, int32_t n_img, int32_t capacity,
                     const pp_inverse_meta *metas, const int64_t *image_ids,
                     const pp_coco_params *params, pp_coco_det *out, int64_t out_capacity,
                     int32_t *out_counts, int32_t *out_flags) {
    const int rc = coco_check_args("pp_coco_dets_cpu", dets, counts, n_img, capacity, 1, metas,
                                   image_ids, params, out, out_capacity, out_counts, out_flags);
    if (rc != PP_OK) return rc;
    static_assert(sizeof(pp_coco_det) == 8 * kCocoHeadWords, "a detection record is the head words");
    int64_t at = 0;
    for (int img = 0; img < n_img; img++) {
        const InverseXf t = inverse_xf(metas[img]);
        const int n_rec = coco_clamp_count(counts[img], capacity);
        const int kept = n_rec < params->max_per_image ? n_rec : params->max_per_image;
        for (int r = 0; r < kept; r++) {
            uint64_t w[kCocoHeadWords];
            coco_det_words(dets[(int64_t)img * capacity + r], metas[img], t, image_ids[img], w);
            if (at + r < out_capacity) std::memcpy(&out[at + r], w, sizeof(w));
        }
        if (kept == 0) {
            uint64_t w[kCocoHeadWords];
            coco_dummy_head(image_ids[img], 0, w);
            if (at < out_capacity) std::memcpy(&out[at], w, sizeof(w));
        }
        out_counts[img] = kept > 0 ? kept : 1;
        out_flags[img] = kept > 0 ? 0 : PP_COCO_EMPTY;
        at += out_counts[img];
    }
    return PP_OK;
}

}  // extern "C"

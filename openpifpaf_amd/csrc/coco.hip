// coco.hip — EvalCoco.from_predictions (eval_coco.py:108-158) for whole batches on the
// device: from a decode's records and one meta per image to the rounded COCO prediction
// records, packed image after image into the caller's block (usually mapped pinned host
// memory).  The decode records are only read.
//
// Two launches on one stream, one workgroup per image in each; no workgroup waits for
// another inside a launch:
//   coco_count_kernel  every record's inverse, NaN test and small-object test (coco_keep),
//                      the kept count after the cap by an in-order prefix over the keep
//                      flags (ballot / popcount per wave, then across the waves); the
//                      image's record count (a dummy record when nothing is kept) goes to
//                      the workspace and to out_counts, its flag word to out_flags
//   coco_write_kernel  the image's offset is the sum of the earlier images' counts (read by
//                      the whole workgroup); the keep flags are formed again, 256 records at
//                      a time, and one wave per kept record builds the record's 7 + 3 K
//                      8-byte words in LDS (lane j = joint j, bbox by a wave reduction) and
//                      stores them as contiguous 16-byte pairs
// The per-record arithmetic is coco.hpp's, shared with the host twins (coco_cpu.hip); its
// inverse transform is inverse.hpp's, shared with the in-place kernels (inverse.hip).  The
// packed offset, the 16-byte-pair store and the destination mapping are pack_common.hpp's,
// shared with pack.hip.
#include "coco.hpp"
#include "pack_common.hpp"

namespace pp {

namespace {

struct CocoImage {  // what one workgroup knows about its image (LDS)
    pp_inverse_meta m;
    InverseXf t;
    int src_of[PP_MAX_KP];
    int swap;
};

// meta, rotation constants and the swap's gather table of image `img`; the caller's next
// barrier publishes them
__device__ __forceinline__ void coco_image_setup(CocoImage &I, const pp_inverse_meta *metas,
                                                 const int *hswap, int K, int img) {
    if (threadIdx.x == 0) {
        I.m = metas[img];
        I.t = inverse_xf(I.m);
        I.swap = I.m.hflip && hswap != nullptr;
    }
    if (threadIdx.x < K && hswap) I.src_of[threadIdx.x] = coco_swap_source(hswap, K, threadIdx.x);
}

__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o > 0; o >>= 1) v = coco_min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = coco_max(v, __shfl_xor(v, o));
    return v;
}

}  // namespace

__global__ __launch_bounds__(256) void coco_count_kernel(const pp_ann *__restrict__ anns,
                                                         const int *__restrict__ counts, int cap,
                                                         int K, const pp_inverse_meta *metas,
                                                         const int *hswap, pp_coco_params P,
                                                         int *ws_counts, int *out_counts,
                                                         int *out_flags) {
    __shared__ CocoImage I;
    __shared__ int s_tmp[4], s_nan;
    const int img = blockIdx.x;
    if (threadIdx.x == 0) s_nan = 0;
    coco_image_setup(I, metas, hswap, K, img);
    __syncthreads();
    const int n_rec = coco_clamp_count(counts[img], cap);
    const int *src_of = I.swap ? I.src_of : nullptr;
    int kept = 0;
    bool nan = false;
    for (int base = 0; base < n_rec; base += 256) {  // uniform trip count
        const int r = base + threadIdx.x;
        bool keep = false;
        if (r < n_rec)
            keep = coco_keep(anns[(int64_t)img * cap + r], K, I.m, I.t, src_of, P.small_threshold,
                             nan);
        int total;
        block_compact<4>(keep, s_tmp, total);
        kept += total;
    }
    if (nan) s_nan = 1;  // every writer stores the same value
    __syncthreads();
    if (threadIdx.x == 0) {  // plain stores: the destinations may lie across PCIe
        const int n_out = kept < P.max_per_image ? kept : P.max_per_image;
        ws_counts[img] = n_out > 0 ? n_out : 1;
        out_counts[img] = n_out > 0 ? n_out : 1;
        out_flags[img] = (s_nan ? PP_COCO_NAN : 0) | (n_out > 0 ? 0 : PP_COCO_EMPTY);
    }
}

__global__ __launch_bounds__(256) void coco_write_kernel(const pp_ann *__restrict__ anns,
                                                         const int *__restrict__ counts, int cap,
                                                         int K, const pp_inverse_meta *metas,
                                                         const int64_t *image_ids, const int *hswap,
                                                         pp_coco_params P, const int *ws_counts,
                                                         char *out, int64_t out_cap) {
    __shared__ CocoImage I;
    __shared__ int s_tmp[4], s_off, s_idx[256];
    __shared__ uint64_t s_rec[4][kCocoHeadWords + 3 * PP_MAX_KP];
    const int img = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    coco_image_setup(I, metas, hswap, K, img);
    const int64_t off = packed_offset(ws_counts, img, s_off);
    const int n_rec = coco_clamp_count(counts[img], cap);
    const int *src_of = I.swap ? I.src_of : nullptr;
    const int words = coco_record_words(K);
    const int64_t image_id = image_ids[img];
    uint64_t *w = s_rec[wave];
    int done = 0;  // kept records so far (uniform)
    for (int base = 0; base < n_rec && done < P.max_per_image; base += 256) {
        const int r = base + threadIdx.x;
        bool keep = r < n_rec, nan = false;
        if (keep && P.small_threshold != 0.0)
            keep = coco_keep(anns[(int64_t)img * cap + r], K, I.m, I.t, src_of, P.small_threshold,
                             nan);
        int total;
        const int slot = block_compact<4>(keep, s_tmp, total);
        if (keep) s_idx[slot] = r;  // slot < 256
        __syncthreads();
        const int m = min(total, P.max_per_image - done);
        for (int q = wave; q < m; q += 4) {
            const pp_ann &a = anns[(int64_t)img * cap + s_idx[q]];
            float x = 0.0f, y = 0.0f, v = 0.0f, js = 0.0f;
            if (lane < K) {
                coco_row(a, I.m, I.t, src_of, lane, x, y, v, js);
                w[kCocoHeadWords + 3 * lane] = u64_of(coco_round2(x));
                w[kCocoHeadWords + 3 * lane + 1] = u64_of(coco_round2(y));
                w[kCocoHeadWords + 3 * lane + 2] = u64_of(coco_round2(coco_v(v)));
            }
            // bbox_from_keypoints (annotation.py:108-119) over the joints with v > 0
            const bool vis = lane < K && v > 0.0f;
            const float bx = wave_min(vis ? x - js : INFINITY);
            const float by = wave_min(vis ? y - js : INFINITY);
            const float bxm = wave_max(vis ? x + js : -INFINITY);
            const float bym = wave_max(vis ? y + js : -INFINITY);
            const bool any = __ballot(vis) != 0ull;
            if (lane == 0) {
                w[0] = (uint64_t)image_id;
                w[1] = u64_of(coco_score3(a.score));
                w[2] = u64_of(any ? coco_round2(bx) : 0.0);
                w[3] = u64_of(any ? coco_round2(by) : 0.0);
                w[4] = u64_of(any ? coco_round2(bxm - bx) : 0.0);
                w[5] = u64_of(any ? coco_round2(bym - by) : 0.0);
                w[6] = coco_cat_word(P.category_id, K);
            }
            wave_sync();
            const int64_t at = off + done + q;
            if (at < out_cap)
                store_words(reinterpret_cast<uint64_t *>(out + at * (8 * (int64_t)words)), w, words,
                            lane, 64);
            wave_sync();  // the wave's words are rewritten for its next record
        }
        done += m;
        __syncthreads();  // s_idx is rewritten in the next round
    }
    if (done == 0 && wave == 0) {  // the one dummy record (eval_coco.py:133-141)
        if (lane == 0) coco_dummy_head(image_id, K, w);
        if (lane < K) w[kCocoHeadWords + 3 * lane] = w[kCocoHeadWords + 3 * lane + 1] =
                          w[kCocoHeadWords + 3 * lane + 2] = u64_of(0.0);
        wave_sync();
        if (off < out_cap)
            store_words(reinterpret_cast<uint64_t *>(out + off * (8 * (int64_t)words)), w, words,
                        lane, 64);
    }
}

// Detections (AnnotationDet has no scale: a cap and no filter): the count is known from
// the record count alone
__global__ __launch_bounds__(256) void coco_det_count_kernel(const int *__restrict__ counts, int n,
                                                             int cap, pp_coco_params P,
                                                             int *ws_counts, int *out_counts,
                                                             int *out_flags) {
    const int img = blockIdx.x * 256 + threadIdx.x;
    if (img >= n) return;
    const int kept = min(coco_clamp_count(counts[img], cap), P.max_per_image);
    ws_counts[img] = kept > 0 ? kept : 1;
    out_counts[img] = kept > 0 ? kept : 1;
    out_flags[img] = kept > 0 ? 0 : PP_COCO_EMPTY;
}

// One workgroup per image, one thread per record: the record's seven words go to LDS and
// the workgroup copies them out as 16-byte pairs
__global__ __launch_bounds__(256) void coco_det_write_kernel(const pp_det *__restrict__ dets,
                                                             const int *__restrict__ counts, int cap,
                                                             const pp_inverse_meta *metas,
                                                             const int64_t *image_ids,
                                                             pp_coco_params P, const int *ws_counts,
                                                             uint64_t *out, int64_t out_cap) {
    __shared__ CocoImage I;
    __shared__ int s_off;
    __shared__ uint64_t s_w[256 * kCocoHeadWords];
    const int img = blockIdx.x;
    coco_image_setup(I, metas, nullptr, 0, img);
    const int64_t off = packed_offset(ws_counts, img, s_off);
    const int64_t image_id = image_ids[img];
    const int kept = min(coco_clamp_count(counts[img], cap), P.max_per_image);
    const int n_out = kept > 0 ? kept : 1;
    for (int base = 0; base < n_out; base += 256) {  // uniform trip count
        const int r = base + threadIdx.x;
        if (r < kept)
            coco_det_words(dets[(int64_t)img * cap + r], I.m, I.t, image_id,
                           s_w + kCocoHeadWords * threadIdx.x);
        else if (r == 0)
            coco_dummy_head(image_id, 0, s_w);
        __syncthreads();
        const int64_t first = off + base;
        const int64_t fit = min((int64_t)min(256, n_out - base), max((int64_t)0, out_cap - first));
        store_words(out + first * kCocoHeadWords, s_w, (int)fit * kCocoHeadWords, (int)threadIdx.x,
                    256);
        __syncthreads();  // s_w is rewritten in the next round
    }
}

}  // namespace pp

using namespace pp;

extern "C" {

int64_t pp_coco_record_size(int32_t K) {
    if (K <= 0 || K > PP_MAX_KP) return 0;
    return 8 * (int64_t)coco_record_words(K);
}

size_t pp_coco_workspace_size(int32_t n_img) {
    if (n_img < 0) return 0;
    return ((size_t)n_img * sizeof(int32_t) + 255) / 256 * 256;
}

int pp_coco_keypoints(const pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                      int32_t capacity, int32_t K, const pp_inverse_meta *d_metas,
                      const int64_t *d_image_ids, const int32_t *d_hswap,
                      const pp_coco_params *params, void *out, int64_t out_capacity,
                      int32_t *out_counts, int32_t *out_flags, void *d_workspace, void *stream) {
    const char *who = "pp_coco_keypoints";
    const int rc = coco_check_args(who, d_anns, d_counts, n_img, capacity, K, d_metas, d_image_ids,
                                   params, out, out_capacity, out_counts, out_flags);
    if (rc != PP_OK) return rc;
    if (!d_workspace) return fail(PP_EINVAL, "pp_coco_keypoints: NULL argument");
    if (reinterpret_cast<uintptr_t>(out) & 7)
        return fail(PP_EINVAL, "pp_coco_keypoints: destination not 8-byte aligned");
    if (n_img == 0) return PP_OK;
    void *dst[3] = {out, out_counts, out_flags};
    if (const int rd = map_destinations(who, dst, 3)) return rd;
    if (reinterpret_cast<uintptr_t>(dst[0]) & 7)  // the mapped address
        return fail(PP_EINVAL, std::string(who) + ": destination not 8-byte aligned");
    hipLaunchKernelGGL(coco_count_kernel, dim3((unsigned)n_img), dim3(256), 0, (hipStream_t)stream,
                       d_anns, d_counts, capacity, K, d_metas, d_hswap, *params,
                       (int *)d_workspace, (int *)dst[1], (int *)dst[2]);
    if (const int rl = check_launch(who)) return rl;
    hipLaunchKernelGGL(coco_write_kernel, dim3((unsigned)n_img), dim3(256), 0, (hipStream_t)stream,
                       d_anns, d_counts, capacity, K, d_metas, d_image_ids, d_hswap, *params,
                       (const int *)d_workspace, (char *)dst[0], out_capacity);
    return check_launch(who);
}

int pp_coco_dets(const pp_det *d_dets, const int32_t *d_counts, int32_t n_img, int32_t capacity,
                 const pp_inverse_meta *d_metas, const int64_t *d_image_ids,
                 const pp_coco_params *params, pp_coco_det *out, int64_t out_capacity,
                 int32_t *out_counts, int32_t *out_flags, void *d_workspace, void *stream) {
    const char *who = "pp_coco_dets";
    const int rc = coco_check_args(who, d_dets, d_counts, n_img, capacity, 1, d_metas, d_image_ids,
                                   params, out, out_capacity, out_counts, out_flags);
    if (rc != PP_OK) return rc;
    if (!d_workspace) return fail(PP_EINVAL, "pp_coco_dets: NULL argument");
    if (reinterpret_cast<uintptr_t>(out) & 7)
        return fail(PP_EINVAL, "pp_coco_dets: destination not 8-byte aligned");
    if (n_img == 0) return PP_OK;
    void *dst[3] = {out, out_counts, out_flags};
    if (const int rd = map_destinations(who, dst, 3)) return rd;
    if (reinterpret_cast<uintptr_t>(dst[0]) & 7)  // the mapped address
        return fail(PP_EINVAL, std::string(who) + ": destination not 8-byte aligned");
    hipLaunchKernelGGL(coco_det_count_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d_counts, n_img, capacity, *params,
                       (int *)d_workspace, (int *)dst[1], (int *)dst[2]);
    if (const int rl = check_launch(who)) return rl;
    hipLaunchKernelGGL(coco_det_write_kernel, dim3((unsigned)n_img), dim3(256), 0,
                       (hipStream_t)stream, d_dets, d_counts, capacity, d_metas, d_image_ids,
                       *params, (const int *)d_workspace, (uint64_t *)dst[0], out_capacity);
    return check_launch(who);
}

}  // extern "C"

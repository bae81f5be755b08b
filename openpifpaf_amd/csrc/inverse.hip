// inverse.hip — Preprocess.annotations_inverse (transforms/preprocess.py:35-95) on decoded
// records in place: image-space poses and boxes from network-input coordinates, one thread
// per record, batched over images (each image has its own meta).  The arithmetic is
// inverse.hpp's, which the COCO record kernels (coco.hip) share; the two kernels here and
// their two exports are all this file holds.
#include "inverse.hpp"

namespace pp {

__global__ __launch_bounds__(256) void ann_inverse_kernel(pp_ann *anns, const int *counts, int cap,
                                                          int K, const pp_inverse_meta *metas,
                                                          const int *hswap, int *nan_flags) {
    const int img = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= min(counts[img], cap)) return;
    pp_ann &a = anns[(int64_t)img * cap + r];
    const pp_inverse_meta m = metas[img];
    const InverseXf t = inverse_xf(m);
    bool nan = false;
    for (int j = 0; j < K; j++) {
        float x = a.data[j][0], y = a.data[j][1];
        inverse_point(m, t, x, y, a.data[j][2], nan);
        a.data[j][0] = x;
        a.data[j][1] = y;
        a.joint_scales[j] = inverse_jscale(m, a.joint_scales[j]);
    }
    if (nan) atomicOr(&nan_flags[img], 1);  // the reference asserts here (preprocess.py:67)
    if (m.hflip && hswap) {  // _HorizontalSwap (hflip.py:17-29): target rows, last writer wins
        float s[PP_MAX_KP][3];
        for (int j = 0; j < K; j++) s[j][0] = s[j][1] = s[j][2] = 0.0f;
        for (int sj = 0; sj < K; sj++) {
            const int tj = hswap[sj];
            s[tj][0] = a.data[sj][0];
            s[tj][1] = a.data[sj][1];
            s[tj][2] = a.data[sj][2];
        }
        for (int j = 0; j < K; j++) {
            a.data[j][0] = s[j][0];
            a.data[j][1] = s[j][1];
            a.data[j][2] = s[j][2];
        }
    }
    const int nd = min(a.n_decoding, PP_MAX_KP);
    for (int d = 0; d < nd; d++)  // decoding_order: offset and scale only (preprocess.py:76-81)
        for (int c = 0; c < 2; c++)
            for (int h = 0; h < 2; h++)
                a.decoding_xyv[d][3 * h + c] = inverse_coord(m, c, a.decoding_xyv[d][3 * h + c]);
}

__global__ __launch_bounds__(256) void det_inverse_kernel(pp_det *dets, const int *counts, int cap,
                                                          const pp_inverse_meta *metas) {
    const int img = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= min(counts[img], cap)) return;
    pp_det &d = dets[(int64_t)img * cap + r];
    const pp_inverse_meta m = metas[img];
    float b[4] = {d.bbox[0], d.bbox[1], d.bbox[2], d.bbox[3]};
    inverse_box(m, inverse_xf(m), b);
    for (int i = 0; i < 4; i++) d.bbox[i] = b[i];
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_annotations_inverse(pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                           int32_t capacity, int32_t K, const pp_inverse_meta *d_metas,
                           const int32_t *d_hswap, int32_t *d_nan_flags, void *stream) {
    if (!d_anns || !d_counts || !d_metas || !d_nan_flags)
        return fail(PP_EINVAL, "pp_annotations_inverse: NULL argument");
    if (n_img < 0 || capacity <= 0 || K <= 0 || K > PP_MAX_KP)
        return fail(PP_ESHAPE, "pp_annotations_inverse: bad shape");
    if (n_img == 0) return PP_OK;
    const dim3 grid((unsigned)((capacity + 255) / 256), (unsigned)n_img);
    hipLaunchKernelGGL(ann_inverse_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_anns,
                       d_counts, capacity, K, d_metas, d_hswap, d_nan_flags);
    return check_launch("pp_annotations_inverse");
}

int pp_dets_inverse(pp_det *d_dets, const int32_t *d_counts, int32_t n_img, int32_t capacity,
                    const pp_inverse_meta *d_metas, void *stream) {
    if (!d_dets || !d_counts || !d_metas) return fail(PP_EINVAL, "pp_dets_inverse: NULL argument");
    if (n_img < 0 || capacity <= 0) return fail(PP_ESHAPE, "pp_dets_inverse: bad shape");
    if (n_img == 0) return PP_OK;
    const dim3 grid((unsigned)((capacity + 255) / 256), (unsigned)n_img);
    hipLaunchKernelGGL(det_inverse_kernel, grid, dim3(256), 0, (hipStream_t)stream, d_dets,
                       d_counts, capacity, d_metas);
    return check_launch("pp_dets_inverse");
}

}  // extern "C"

// encode_cpu.hip — host twins of the CIF / CAF target encoders (pp_encode_cif_cpu,
// pp_encode_caf_cpu): the plan of encode_plan.hip and the per-cell functions of encode.hpp,
// cell after cell, one image per task on n_threads host threads.  Also the two helpers the
// tests pin against NumPy (pp_encode_norm_cpu, pp_encode_linspace_cpu).
#pragma clang fp contract(off)
#include "encode.hpp"

#include <atomic>
#include <thread>
#include <vector>

namespace pp {

static void encode_image_cpu(bool is_caf, const pp_encoder *enc, const EncPlan &plan, int i,
                             float *out) {
    const EncImage &m = plan.images[(size_t)i];
    const int cells = m.h * m.w;
    for (int f = 0; f < plan.F; f++)
        for (int cell = 0; cell < cells; cell++) {
            if (is_caf)
                caf_cell(out, m, plan.boxes.data(), plan.fj.data(), plan.caf.data(), enc->side,
                         enc->padding, enc->fixed_size != 0, f, cell);
            else
                cif_cell(out, m, plan.boxes.data(), plan.fj.data(), plan.cif.data(), enc->side, f,
                         cell);
        }
}

static int encode_cpu(const char *who, bool is_caf, const pp_encoder *enc,
                      const pp_enc_image *images, int32_t n_img, const pp_enc_ann *anns,
                      const float *keypoints, int32_t n_ann, float *out, int64_t out_elems,
                      int32_t n_threads) {
    EncPlan plan;
    const int rc = encode_plan(who, is_caf, enc, images, n_img, anns, keypoints, n_ann, out,
                               out_elems, &plan);
    if (rc != PP_OK || n_img == 0) return rc;
    const int nt = n_threads < 1 ? 1 : n_threads > n_img ? n_img : n_threads;
    if (nt == 1) {
        for (int i = 0; i < n_img; i++) encode_image_cpu(is_caf, enc, plan, i, out);
        return PP_OK;
    }
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++)
        pool.emplace_back([&]() {
            for (int i = next++; i < n_img; i = next++) encode_image_cpu(is_caf, enc, plan, i, out);
        });
    for (std::thread &t : pool) t.join();
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_encode_cif_cpu(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                      const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *out,
                      int64_t out_elems, int32_t n_threads) {
    return encode_cpu("pp_encode_cif_cpu", false, enc, images, n_img, anns, keypoints, n_ann, out,
                      out_elems, n_threads);
}

int pp_encode_caf_cpu(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                      const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *out,
                      int64_t out_elems, int32_t n_threads) {
    return encode_cpu("pp_encode_caf_cpu", true, enc, images, n_img, anns, keypoints, n_ann, out,
                      out_elems, n_threads);
}

int pp_encode_norm_cpu(const float *xy, float *out, int64_t n) {
    if (n < 0) return fail(PP_ESHAPE, "pp_encode_norm_cpu: n < 0");
    if (n > 0 && (!xy || !out)) return fail(PP_EINVAL, "pp_encode_norm_cpu: NULL argument");
    for (int64_t i = 0; i < n; i++) out[i] = norm2_f32(xy[2 * i], xy[2 * i + 1]);
    return PP_OK;
}

int pp_encode_linspace_cpu(double start, double stop, int32_t num, double *out) {
    if (num < 2) return fail(PP_ESHAPE, "pp_encode_linspace_cpu: num < 2");
    if (!out) return fail(PP_EINVAL, "pp_encode_linspace_cpu: NULL argument");
    const double step = (stop - start) / (double)(num - 1);
    for (int i = 0; i < num; i++) out[i] = linspace_at(start, step, stop, num, i);
    return PP_OK;
}

}  // extern "C"

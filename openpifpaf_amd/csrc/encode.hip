// encode.hip — the CIF / CAF target encoders on gfx950 (pp_encode_cif, pp_encode_caf): one
// launch per encoder per batch over the job lists the host plans (encode_plan.hip).
//
// Kernel shape.  A cell's result depends on no other cell (encode.hpp), so a lane owns one
// cell of one (image, field) plane from its initial state to its stored elements and keeps
// the fold's state (l, the winner's regressions and job) in registers: no LDS stage, no
// tiles whose edges limbs would cross, no plane too large to hold, and no second pass over
// memory.  A workgroup takes 256 consecutive cells of a plane in row-major order, so a wave
// stores 64 consecutive floats into each of the field's 8 (CIF) or 15 (CAF) output planes;
// the workgroups of image 0 come first, field by field, then image 1's, and a workgroup
// finds its image by bisecting the per-image first-workgroup numbers.  The job records of
// the field are read at wave-uniform addresses.  A CIF cell walks its field's joints (one
// per annotation); a CAF cell walks its field's limbs, skips those whose box it lies
// outside, and for the others evaluates the steps along the limb in float64.
#pragma clang fp contract(off)
#include "encode.hpp"

#include <vector>

namespace pp {

struct EncArgs {
    float *out;
    const EncImage *images;
    const int32_t *fj;
    const EncBox *boxes;
    const void *jobs;
    int n_img, F;
    int side, padding, fixed;
};

template <bool CAF>
__global__ __launch_bounds__(kEncBlock) void encode_kernel(EncArgs a) {
    // the last image whose first workgroup is not after this one
    const int b = (int)blockIdx.x;
    int lo = 0, hi = a.n_img;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.images[mid].block0 <= b)
            lo = mid;
        else
            hi = mid;
    }
    const EncImage m = a.images[lo];
    const int rel = b - m.block0;
    const int f = rel / m.bpp;
    const int cell = (rel - f * m.bpp) * kEncBlock + (int)threadIdx.x;
    if (f >= a.F || cell >= m.h * m.w) return;
    if (CAF)
        caf_cell(a.out, m, a.boxes, a.fj, (const CafJob *)a.jobs, a.side, a.padding, a.fixed != 0,
                 f, cell);
    else
        cif_cell(a.out, m, a.boxes, a.fj, (const CifJob *)a.jobs, a.side, f, cell);
}

static int encode_device(const char *who, bool is_caf, const pp_encoder *enc,
                         const pp_enc_image *images, int32_t n_img, const pp_enc_ann *anns,
                         const float *keypoints, int32_t n_ann, float *d_out, int64_t out_elems,
                         void *d_tables, size_t tables_bytes, void *stream) {
    EncPlan plan;
    const int rc = encode_plan(who, is_caf, enc, images, n_img, anns, keypoints, n_ann, d_out,
                               out_elems, &plan);
    if (rc != PP_OK || n_img == 0) return rc;
    if (!d_tables) return fail(PP_EINVAL, std::string(who) + ": NULL argument");
    if ((uintptr_t)d_tables & 7u) return fail(PP_EINVAL, std::string(who) + ": misaligned buffer");
    if (tables_bytes < plan.bytes)
        return fail(PP_ENOMEM, std::string(who) + ": table buffer too small");
    // one staging copy (a pageable host buffer is consumed before the copy call returns)
    std::vector<char> host(plan.bytes);
    plan.stage(host.data(), is_caf);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(d_tables, host.data(), host.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PP_EHIP, std::string(who) + ": staging the tables failed");
    }
    const char *t = (const char *)d_tables;
    EncArgs a{};
    a.out = d_out;
    a.images = (const EncImage *)t;
    a.fj = (const int32_t *)(t + plan.off_fj);
    a.boxes = (const EncBox *)(t + plan.off_boxes);
    a.jobs = t + plan.off_jobs;
    a.n_img = n_img;
    a.F = plan.F;
    a.side = enc->side;
    a.padding = enc->padding;
    a.fixed = enc->fixed_size != 0;
    if (is_caf)
        hipLaunchKernelGGL(encode_kernel<true>, dim3((unsigned)plan.blocks), dim3(kEncBlock), 0, s, a);
    else
        hipLaunchKernelGGL(encode_kernel<false>, dim3((unsigned)plan.blocks), dim3(kEncBlock), 0, s, a);
    return check_launch(who);
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_encode_cif(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                  const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *d_out,
                  int64_t out_elems, void *d_tables, size_t tables_bytes, void *stream) {
    return encode_device("pp_encode_cif", false, enc, images, n_img, anns, keypoints, n_ann, d_out,
                         out_elems, d_tables, tables_bytes, stream);
}

int pp_encode_caf(const pp_encoder *enc, const pp_enc_image *images, int32_t n_img,
                  const pp_enc_ann *anns, const float *keypoints, int32_t n_ann, float *d_out,
                  int64_t out_elems, void *d_tables, size_t tables_bytes, void *stream) {
    return encode_device("pp_encode_caf", true, enc, images, n_img, anns, keypoints, n_ann, d_out,
                         out_elems, d_tables, tables_bytes, stream);
}

}  // extern "C"

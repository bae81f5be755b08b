// preprocess.hip — eval_coco.preprocess_factory's image chain (RescaleAbsolute,
// CenterPad / CenterPadTight, EVAL_TRANSFORM's ToTensor and Normalize) on a batch of uint8
// RGB images of different sizes in ONE launch (pp_preprocess_images), and its host twin
// (pp_preprocess_images_cpu).  Both run the per-pixel functions below, so they agree bit
// for bit by construction.
//
// Resize: scipy.ndimage.zoom(im, (th / h, tw / w, 1), order=1) on uint8 (transforms/
// scale.py:36-40) restated in float64, operation by operation (DESIGN.md has how the order
// was established): per axis the coordinate y = i * ((h - 1) / (th - 1)), its floor y0 and
// the weights wy0 = 1 - (y - y0), wy1 = 1 - wy0 (not y - y0); per pixel
//     t = ((a wy0) wx0 + (b wy0) wx1) + (c wy1) wx0;  t = t + (d wy1) wx1
// rounded as t > 0 ? (uint8)min(t + 0.5, 255) : 0, and 0 wherever a coordinate compares
// above the last source index (scipy's constant mode: when (th - 1) * zoom rounds above
// h - 1 the whole last row is black, likewise the last column).  No operation may be fused.
#pragma clang fp contract(off)
//
// Pad: pixels outside the rescaled region take `fill`.  ToTensor and Normalize:
// ((float)u8 / 255.0f - mean_c) / std_c has 3 * 256 distinct results, so the host computes
// them once (normalize_table, in the output's number format already: float16 and bfloat16
// are round-to-nearest-even of the float32 value) and the kernel reads them from LDS; the
// device never divides.
//
// Kernel shape: the pass is bound by its stores (12 B per pixel in float32).  An image's
// output is H * W pixels in row-major order; a workgroup takes 1024 consecutive ones, a lane
// four of them 256 apart, each with its three channels (one pixel per lane left the
// workgroup waiting on its own chain of dependent loads: table, descriptor, taps).  A planar
// plane is contiguous in that order, so the lanes of a wave store 64 consecutive elements per
// plane; channels-last lanes store their 3 channels side by side.  The workgroups of image 0 come first, then image 1's: a
// workgroup finds its image by bisecting the per-image first-workgroup numbers (a prefix
// sum, beside the descriptors in the staged table).  The source taps are 12 cached byte
// loads per pixel, issued without a branch (load_taps).
#include "pp_common.hpp"
#include "preprocess_pixel.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace pp {

constexpr int kPreBlock = 256;
constexpr int kPrePixels = 4;  // pixels per lane, kPreBlock apart: their loads overlap
constexpr int kPreTile = kPreBlock * kPrePixels;

constexpr size_t kLutBytes = 768 * sizeof(uint32_t);

struct PreArgs {
    const uint8_t *src;
    void *out;
    const uint32_t *lut;    // (3, 256) results of ToTensor + Normalize as bits of the output type
    const PreImage *images; // (n_img), block0 ascending
    int n_img;
    uint8_t fill[4];
};

// DT: PP_PRE_*; LAYOUT: PP_PRE_PLANAR / PP_PRE_CHANNELS_LAST (PP_PRE_U8 is always HWC)
template <int DT, int LAYOUT>
__global__ __launch_bounds__(kPreBlock) void preprocess_kernel(PreArgs a) {
    __shared__ uint32_t s_lut[768];
    if (DT != PP_PRE_U8) {
        for (int k = threadIdx.x; k < 768; k += kPreBlock) s_lut[k] = a.lut[k];
        __syncthreads();
    }
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
    const PreImage m = a.images[lo];
    // H * W <= 2^29 (checked on the host): 32-bit index arithmetic inside the image
    const int hw = m.H * m.W;
    const int base = (b - m.block0) * kPreTile + (int)threadIdx.x;
    const uint8_t fill[3] = {a.fill[0], a.fill[1], a.fill[2]};
    Taps taps[kPrePixels];
#pragma unroll
    for (int k = 0; k < kPrePixels; k++) {
        const int p = min(base + k * kPreBlock, hw - 1);  // past the end: recomputes the last
        const int y = p / m.W, x = p - y * m.W;
        taps[k] = load_taps(a.src, m, y, x);
    }
    uint8_t px[kPrePixels][3];
#pragma unroll
    for (int k = 0; k < kPrePixels; k++) padded_pixel(taps[k], fill, px[k]);
#pragma unroll
    for (int k = 0; k < kPrePixels; k++) {
        const int p = base + k * kPreBlock;
        if (p >= hw) break;
        if (DT == PP_PRE_U8) {
            uint8_t *o = (uint8_t *)a.out + m.out_offset + 3 * (int64_t)p;
            o[0] = px[k][0];
            o[1] = px[k][1];
            o[2] = px[k][2];
        } else if (DT == PP_PRE_F32) {
            store_pixel<uint32_t, LAYOUT>(a.out, m, p, px[k], s_lut);
        } else {
            store_pixel<uint16_t, LAYOUT>(a.out, m, p, px[k], s_lut);
        }
    }
}

// The argument checks both entries share; fills `images` (zoom factors and first workgroups)
// when they pass.  n_img == 0 returns PP_OK with nothing filled.
static int prepare(const char *who, const void *src, int64_t src_bytes, const pp_image_desc *descs,
                   int32_t n_img, const void *out, int64_t out_elems, int32_t dtype,
                   int32_t layout, const float *mean, const float *stdv, const uint8_t *fill,
                   std::vector<PreImage> *images, int64_t *n_blocks) {
    const std::string w(who);
    if (n_img < 0) return fail(PP_ESHAPE, w + ": n_img < 0");
    if (dtype != PP_PRE_F32 && dtype != PP_PRE_F16 && dtype != PP_PRE_BF16 && dtype != PP_PRE_U8)
        return fail(PP_EINVAL, w + ": unknown dtype");
    if (layout != PP_PRE_PLANAR && layout != PP_PRE_CHANNELS_LAST)
        return fail(PP_EINVAL, w + ": unknown layout");
    if (n_img == 0) return PP_OK;
    if (!src || !descs || !out || !mean || !stdv || !fill)
        return fail(PP_EINVAL, w + ": NULL argument");
    for (int c = 0; c < 3; c++)
        if (!(stdv[c] != 0.0f) || !std::isfinite(stdv[c]))
            return fail(PP_EINVAL, w + ": std must be finite and not 0");
    if ((uintptr_t)out & (elem_size(dtype) - 1)) return fail(PP_EINVAL, w + ": misaligned output");
    if (src_bytes < 0 || out_elems < 0) return fail(PP_ESHAPE, w + ": negative buffer size");
    images->resize((size_t)n_img);
    int64_t blocks = 0;
    for (int i = 0; i < n_img; i++) {
        const pp_image_desc &d = descs[i];
        if (d.h < 2 || d.w < 2 || d.th < 2 || d.tw < 2)
            return fail(PP_ESHAPE, w + ": a source or target edge < 2");
        if ((int64_t)d.h * d.w * 3 > INT32_MAX)
            return fail(PP_ESHAPE, w + ": source image out of range");
        if (d.H <= 0 || d.W <= 0 || (int64_t)d.H * d.W > INT32_MAX / 4)
            return fail(PP_ESHAPE, w + ": output size out of range");
        if (d.left < 0 || d.top < 0 || (int64_t)d.left + d.tw > d.W || (int64_t)d.top + d.th > d.H)
            return fail(PP_ESHAPE, w + ": the target does not fit its output with this pad");
        if (d.src_offset < 0 || d.src_offset > src_bytes ||
            (int64_t)d.h * d.w * 3 > src_bytes - d.src_offset)
            return fail(PP_ESHAPE, w + ": a source image beyond the source buffer");
        if (d.out_offset < 0 || d.out_offset > out_elems ||
            (int64_t)d.H * d.W * 3 > out_elems - d.out_offset)
            return fail(PP_ESHAPE, w + ": an output region beyond the output buffer");
        PreImage &m = (*images)[(size_t)i];
        m.src_offset = d.src_offset;
        m.out_offset = d.out_offset;
        m.h = d.h, m.w = d.w, m.th = d.th, m.tw = d.tw;
        m.left = d.left, m.top = d.top, m.H = d.H, m.W = d.W;
        m.zy = (double)(d.h - 1) / (double)(d.th - 1);
        m.zx = (double)(d.w - 1) / (double)(d.tw - 1);
        m.block0 = (int32_t)blocks;
        m.pad_ = 0;
        blocks += ((int64_t)d.H * d.W + kPreTile - 1) / kPreTile;
        if (blocks > INT32_MAX) return fail(PP_ESHAPE, w + ": too many output pixels for one launch");
    }
    *n_blocks = blocks;
    return PP_OK;
}

template <int LAYOUT>
static void image_cpu(const uint8_t *src, const PreImage &m, void *out, int dtype,
                      const uint8_t *fill, const uint32_t *lut) {
    for (int y = 0; y < m.H; y++)
        for (int x = 0; x < m.W; x++) {
            uint8_t px[3];
            padded_pixel(load_taps(src, m, y, x), fill, px);
            const int64_t p = (int64_t)y * m.W + x;
            if (dtype == PP_PRE_U8) {
                uint8_t *o = (uint8_t *)out + m.out_offset + 3 * p;
                o[0] = px[0], o[1] = px[1], o[2] = px[2];
            } else if (dtype == PP_PRE_F32) {
                store_pixel<uint32_t, LAYOUT>(out, m, p, px, lut);
            } else {
                store_pixel<uint16_t, LAYOUT>(out, m, p, px, lut);
            }
        }
}

template <int DT>
static void launch(int layout, int64_t blocks, hipStream_t s, const PreArgs &a) {
    if (layout == PP_PRE_PLANAR)
        hipLaunchKernelGGL((preprocess_kernel<DT, PP_PRE_PLANAR>), dim3((unsigned)blocks),
                           dim3(kPreBlock), 0, s, a);
    else
        hipLaunchKernelGGL((preprocess_kernel<DT, PP_PRE_CHANNELS_LAST>), dim3((unsigned)blocks),
                           dim3(kPreBlock), 0, s, a);
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_preprocess_tables_size(int32_t n_img) {
    return n_img > 0 ? kLutBytes + (size_t)n_img * sizeof(PreImage) : 0;
}

int pp_preprocess_images(const uint8_t *d_src, int64_t src_bytes, const pp_image_desc *descs,
                         int32_t n_img, void *d_out, int64_t out_elems, int32_t dtype,
                         int32_t layout, const float *mean, const float *stdv,
                         const uint8_t *fill, void *d_tables, size_t tables_bytes, void *stream) {
    const char *who = "pp_preprocess_images";
    std::vector<PreImage> images;
    int64_t blocks = 0;
    const int rc = prepare(who, d_src, src_bytes, descs, n_img, d_out, out_elems, dtype, layout,
                           mean, stdv, fill, &images, &blocks);
    if (rc != PP_OK || n_img == 0) return rc;
    if (!d_tables) return fail(PP_EINVAL, std::string(who) + ": NULL argument");
    if (tables_bytes < pp_preprocess_tables_size(n_img))
        return fail(PP_ENOMEM, std::string(who) + ": table buffer too small");
    if ((uintptr_t)d_tables & 7u) return fail(PP_EINVAL, std::string(who) + ": misaligned buffer");
    // the value table and the image records in one staging copy (a pageable host buffer is
    // consumed before the copy call returns)
    std::vector<char> host(pp_preprocess_tables_size(n_img));
    normalize_table(dtype, mean, stdv, (uint32_t *)host.data());
    memcpy(host.data() + kLutBytes, images.data(), images.size() * sizeof(PreImage));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(d_tables, host.data(), host.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PP_EHIP, std::string(who) + ": staging the tables failed");
    }
    PreArgs a{};
    a.src = d_src;
    a.out = d_out;
    a.lut = (const uint32_t *)d_tables;
    a.images = (const PreImage *)((const char *)d_tables + kLutBytes);
    a.n_img = n_img;
    a.fill[0] = fill[0], a.fill[1] = fill[1], a.fill[2] = fill[2];
    if (dtype == PP_PRE_F32)
        launch<PP_PRE_F32>(layout, blocks, s, a);
    else if (dtype == PP_PRE_F16)
        launch<PP_PRE_F16>(layout, blocks, s, a);
    else if (dtype == PP_PRE_BF16)
        launch<PP_PRE_BF16>(layout, blocks, s, a);
    else
        launch<PP_PRE_U8>(PP_PRE_CHANNELS_LAST, blocks, s, a);
    return check_launch(who);
}

int pp_preprocess_images_cpu(const uint8_t *src, int64_t src_bytes, const pp_image_desc *descs,
                             int32_t n_img, void *out, int64_t out_elems, int32_t dtype,
                             int32_t layout, const float *mean, const float *stdv,
                             const uint8_t *fill) {
    std::vector<PreImage> images;
    int64_t blocks = 0;
    const int rc = prepare("pp_preprocess_images_cpu", src, src_bytes, descs, n_img, out,
                           out_elems, dtype, layout, mean, stdv, fill, &images, &blocks);
    if (rc != PP_OK || n_img == 0) return rc;
    uint32_t lut[768];
    normalize_table(dtype, mean, stdv, lut);
    for (const PreImage &m : images) {
        if (layout == PP_PRE_PLANAR)
            image_cpu<PP_PRE_PLANAR>(src, m, out, dtype, fill, lut);
        else
            image_cpu<PP_PRE_CHANNELS_LAST>(src, m, out, dtype, fill, lut);
    }
    return PP_OK;
}

}  // extern "C"

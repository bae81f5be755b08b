// preprocess.hip — eval_coco.preprocess_factory on a batch of uint8 RGB images of different
// sizes in ONE launch, and the host twins.  Four parts: the per-pixel header
// (preprocess_pixel.hpp), the two kernels with their argument structs, one host layer
// (checks, table staging, dtype dispatch, host twin) and the six C entries.
//   * pp_preprocess_images: the image chain (RescaleAbsolute, CenterPad / CenterPadTight,
//     EVAL_TRANSFORM's ToTensor and Normalize);
//   * pp_preprocess_views: the chain's remaining modes,
//       --extended-scale (eval_coco.py:359-366): nothing new here, every image carries its own
//       rescaled size (th, tw) already;
//       --orientation-invariant (eval_coco.py:376-384, transforms/rotate.py:42-52): the square
//       padded image turned by a quarter, a half or three quarters;
//       --multi-scale / --multi-scale-hflip (network/nets.py:111-131): the normalised input cut
//       into up to five reduced inputs (every pixel, two of every three, every 2nd, 3rd and
//       5th) and their mirror images.
// A kernel and the host twin run the same per-pixel functions, so they agree bit for bit by
// construction.
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
//
// The views kernel has that shape, but a lane owns pixels of the TURNED canvas T
// (H == W == N), so that the stores of a wave stay consecutive in every view:
//     rot 1: T[y'][x'] = canvas[x'][N-1-y']     (swapaxes, then flip axis 0)
//     rot 2: T[y'][x'] = canvas[N-1-y'][N-1-x']
//     rot 3: T[y'][x'] = canvas[N-1-x'][y']     (swapaxes, then flip axis 1)
// and maps (y', x') back through the turn for its taps (with rot 1 or 3 the source reads of a
// wave run down a column: cached byte loads, a third to a twelfth of the store bytes).
// Reduction r in {1, 2, 3, 5} keeps the rows and columns with i % r == 0 at i / r; reduction
// 1.5 keeps i % 3 != 2 at i - i / 3.  A mirrored view stores column sx at n - 1 - sx.  A
// pixel's three bytes are computed once, its three table values looked up once, and stored
// into every selected view that keeps (y', x'): the float64 blend, which bounds the images
// kernel, is done once per canvas pixel and not once per view pixel (3.69 times as many with
// all ten views).
#include "pp_common.hpp"
#include "preprocess_pixel.hpp"

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

namespace pp {

// ---------------------------------------------------------------- the images kernel
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

template <int DT>
static void launch(int layout, int64_t blocks, hipStream_t s, const PreArgs &a) {
    if (layout == PP_PRE_PLANAR)
        hipLaunchKernelGGL((preprocess_kernel<DT, PP_PRE_PLANAR>), dim3((unsigned)blocks),
                           dim3(kPreBlock), 0, s, a);
    else
        hipLaunchKernelGGL((preprocess_kernel<DT, PP_PRE_CHANNELS_LAST>), dim3((unsigned)blocks),
                           dim3(kPreBlock), 0, s, a);
}

// ----------------------------------------------------------------- the views kernel
// the images kernel's geometry: the host layer counts workgroups in kPreTile for both
constexpr int kViewBlock = kPreBlock;
constexpr int kViewPixels = kPrePixels;  // pixels per lane, kViewBlock apart: their loads overlap
constexpr int kViewTile = kViewBlock * kViewPixels;
static_assert(kViewTile == kPreTile, "one workgroup count serves both kernels");
constexpr int kViewReductions = 5;
constexpr uint32_t kViewMaskAll = (1u << kViewReductions) - 1u;

// one image as the views kernel reads it (m.out_offset is not used: the per-view offsets are
// a table of their own)
struct ViewImage {
    PreImage m;
    int32_t rot, pad_;
};
static_assert(sizeof(ViewImage) == 80, "ViewImage layout");

// canvas pixel (y, x) shown at (yt, xt) of the turned canvas (h == w == n when rot != 0)
__host__ __device__ __forceinline__ void turned_source(int rot, int n, int yt, int xt, int &y,
                                                       int &x) {
    y = rot == 0 ? yt : rot == 1 ? xt : rot == 2 ? n - 1 - yt : n - 1 - xt;
    x = rot == 0 ? xt : rot == 1 ? n - 1 - yt : rot == 2 ? n - 1 - xt : yt;
}

// Reduction RI (0..4: 1, 1.5, 2, 3, 5) of an H x W image: the view's size, and whether it
// keeps pixel (y, x) and where.  The divisors are constants.
template <int RI>
__host__ __device__ __forceinline__ void view_size(int H, int W, int &nrows, int &ncols) {
    if (RI == 0) {
        nrows = H, ncols = W;
    } else if (RI == 1) {
        nrows = H - H / 3, ncols = W - W / 3;
    } else {
        constexpr int R = RI == 2 ? 2 : RI == 3 ? 3 : 5;
        nrows = (H + R - 1) / R, ncols = (W + R - 1) / R;
    }
}
template <int RI>
__host__ __device__ __forceinline__ bool view_keeps(int y, int x, int &sy, int &sx) {
    if (RI == 0) {
        sy = y, sx = x;
        return true;
    }
    if (RI == 1) {
        const int qy = y / 3, qx = x / 3;
        sy = y - qy, sx = x - qx;
        return y - 3 * qy != 2 && x - 3 * qx != 2;
    }
    constexpr int R = RI == 2 ? 2 : RI == 3 ? 3 : 5;
    sy = y / R, sx = x / R;
    return sy * R == y && sx * R == x;
}

// the three values of view pixel `pix` into an image's region of npix pixels at o
// (3 * npix <= INT32_MAX is checked on the host: 32-bit arithmetic inside the region)
template <typename T, int LAYOUT>
__host__ __device__ __forceinline__ void store_view(T *o, int npix, int pix,
                                                    const uint32_t val[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[LAYOUT == PP_PRE_PLANAR ? c * npix + pix : 3 * pix + c] = (T)val[c];
}

// turned-canvas pixel (y, x) into reduction RI's view at `off` and its mirrored view at
// `off_m` (elements of T), when the reduction keeps it
template <int RI, typename T, int LAYOUT>
__host__ __device__ __forceinline__ void store_reduced(T *out, int64_t off, int64_t off_m,
                                                       bool mirror, int H, int W, int y, int x,
                                                       const uint32_t val[3]) {
    int sy, sx, nrows, ncols;
    if (!view_keeps<RI>(y, x, sy, sx)) return;
    view_size<RI>(H, W, nrows, ncols);
    const int npix = nrows * ncols;
    store_view<T, LAYOUT>(out + off, npix, sy * ncols + sx, val);
    if (mirror) store_view<T, LAYOUT>(out + off_m, npix, sy * ncols + (ncols - 1 - sx), val);
}

// the values of one pixel as the output holds them: table entries, or the bytes themselves
template <int DT>
__host__ __device__ __forceinline__ void pixel_values(const uint8_t px[3], const uint32_t *lut,
                                                      uint32_t val[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) val[c] = DT == PP_PRE_U8 ? (uint32_t)px[c] : lut[c * 256 + px[c]];
}

struct ViewArgs {
    const uint8_t *src;
    void *out;
    const uint32_t *lut;      // (3, 256) results of ToTensor + Normalize as bits of the output type
    const ViewImage *images;  // (n_img), block0 ascending
    const int64_t *offs;      // (n_img, n_views) first element of the image in each view
    int n_img, n_views, n_red;
    uint32_t mask;            // selected reductions
    int mirror;
    uint8_t fill[4];
};

template <int DT>
struct ViewElem {
    using type = uint16_t;
};
template <>
struct ViewElem<PP_PRE_F32> {
    using type = uint32_t;
};
template <>
struct ViewElem<PP_PRE_U8> {
    using type = uint8_t;
};

// DT: PP_PRE_*; LAYOUT: PP_PRE_PLANAR / PP_PRE_CHANNELS_LAST (PP_PRE_U8 is always HWC)
template <int DT, int LAYOUT>
__global__ __launch_bounds__(kViewBlock) void preprocess_views_kernel(ViewArgs a) {
    using T = typename ViewElem<DT>::type;
    __shared__ uint32_t s_lut[768];
    if (DT != PP_PRE_U8) {
        for (int k = threadIdx.x; k < 768; k += kViewBlock) s_lut[k] = a.lut[k];
        __syncthreads();
    }
    // the last image whose first workgroup is not after this one
    const int b = (int)blockIdx.x;
    int lo = 0, hi = a.n_img;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.images[mid].m.block0 <= b)
            lo = mid;
        else
            hi = mid;
    }
    const ViewImage vi = a.images[lo];
    const PreImage &m = vi.m;
    // H * W <= 2^29 (checked on the host): 32-bit index arithmetic inside the image
    const int hw = m.H * m.W;
    const int base = (b - m.block0) * kViewTile + (int)threadIdx.x;
    const uint8_t fill[3] = {a.fill[0], a.fill[1], a.fill[2]};
    Taps taps[kViewPixels];
    int yt[kViewPixels], xt[kViewPixels];
#pragma unroll
    for (int k = 0; k < kViewPixels; k++) {
        const int p = min(base + k * kViewBlock, hw - 1);  // past the end: recomputes the last
        yt[k] = p / m.W, xt[k] = p - yt[k] * m.W;
        int y, x;
        turned_source(vi.rot, m.H, yt[k], xt[k], y, x);
        taps[k] = load_taps(a.src, m, y, x);
    }
    uint32_t val[kViewPixels][3];
#pragma unroll
    for (int k = 0; k < kViewPixels; k++) {
        uint8_t px[3];
        padded_pixel(taps[k], fill, px);
        pixel_values<DT>(px, s_lut, val[k]);
    }
    T *out = (T *)a.out;
    const int64_t *offs = a.offs + (int64_t)lo * a.n_views;
    const bool mirror = a.mirror != 0;
    int v = 0;  // the view of the next selected reduction (workgroup-uniform)
#define PP_VIEW_REDUCTION(RI)                                                                  \
    if ((a.mask >> RI) & 1u) {                                                                 \
        const int64_t off = offs[v], off_m = mirror ? offs[v + a.n_red] : 0;                   \
        _Pragma("unroll") for (int k = 0; k < kViewPixels; k++) {                             \
            if (base + k * kViewBlock < hw) /* lanes past the end store nothing */             \
                store_reduced<RI, T, LAYOUT>(out, off, off_m, mirror, m.H, m.W, yt[k], xt[k],  \
                                             val[k]);                                          \
        }                                                                                      \
        v++;                                                                                   \
    }
    PP_VIEW_REDUCTION(0)
    PP_VIEW_REDUCTION(1)
    PP_VIEW_REDUCTION(2)
    PP_VIEW_REDUCTION(3)
    PP_VIEW_REDUCTION(4)
#undef PP_VIEW_REDUCTION
}

template <int DT>
static void launch(int layout, int64_t blocks, hipStream_t s, const ViewArgs &a) {
    if (layout == PP_PRE_PLANAR)
        hipLaunchKernelGGL((preprocess_views_kernel<DT, PP_PRE_PLANAR>), dim3((unsigned)blocks),
                           dim3(kViewBlock), 0, s, a);
    else
        hipLaunchKernelGGL((preprocess_views_kernel<DT, PP_PRE_CHANNELS_LAST>),
                           dim3((unsigned)blocks), dim3(kViewBlock), 0, s, a);
}

// ------------------------------------------------------------------- the host layer
static int popcount5(uint32_t mask) {
    int n = 0;
    for (int r = 0; r < kViewReductions; r++) n += (int)((mask >> r) & 1u);
    return n;
}

static void view_size_of(int ri, int H, int W, int &nrows, int &ncols) {
    switch (ri) {
    case 0: view_size<0>(H, W, nrows, ncols); break;
    case 1: view_size<1>(H, W, nrows, ncols); break;
    case 2: view_size<2>(H, W, nrows, ncols); break;
    case 3: view_size<3>(H, W, nrows, ncols); break;
    default: view_size<4>(H, W, nrows, ncols); break;
    }
}

// What every entry passes on as it got it.  `beyond` is the entry's refusal of an image
// region outside the output.
struct Call {
    const char *who, *beyond;
    const uint8_t *src;
    int64_t src_bytes;
    int32_t n_img;
    void *out;
    int64_t out_elems;
    int32_t dtype, layout;
    const float *mean, *stdv;
    const uint8_t *fill;
};

// The argument checks of all four entries; fills `images` (zoom factors and first
// workgroups) and the workgroup count when they pass.  n_img == 0 returns PP_OK with nothing
// filled.
static int prepare(const Call &c, const pp_view_image *descs, const int64_t *view_offsets,
                   int32_t reductions, int32_t mirror, std::vector<ViewImage> *images,
                   int64_t *n_blocks) {
    const std::string w(c.who);
    if (c.n_img < 0) return fail(PP_ESHAPE, w + ": n_img < 0");
    if (c.dtype != PP_PRE_F32 && c.dtype != PP_PRE_F16 && c.dtype != PP_PRE_BF16 &&
        c.dtype != PP_PRE_U8)
        return fail(PP_EINVAL, w + ": unknown dtype");
    if (c.layout != PP_PRE_PLANAR && c.layout != PP_PRE_CHANNELS_LAST)
        return fail(PP_EINVAL, w + ": unknown layout");
    if (reductions <= 0 || ((uint32_t)reductions & ~kViewMaskAll))
        return fail(PP_EINVAL, w + ": empty or unknown reduction mask");
    if (c.n_img == 0) return PP_OK;
    if (!c.src || !descs || !view_offsets || !c.out || !c.mean || !c.stdv || !c.fill)
        return fail(PP_EINVAL, w + ": NULL argument");
    for (int k = 0; k < 3; k++)
        if (!(c.stdv[k] != 0.0f) || !std::isfinite(c.stdv[k]))
            return fail(PP_EINVAL, w + ": std must be finite and not 0");
    if ((uintptr_t)c.out & (elem_size(c.dtype) - 1))
        return fail(PP_EINVAL, w + ": misaligned output");
    if (c.src_bytes < 0 || c.out_elems < 0) return fail(PP_ESHAPE, w + ": negative buffer size");
    const uint32_t mask = (uint32_t)reductions;
    const int n_red = popcount5(mask), n_views = n_red * (mirror ? 2 : 1);
    const bool pyramid = mask != 1u || mirror;
    images->resize((size_t)c.n_img);
    int64_t blocks = 0;
    for (int i = 0; i < c.n_img; i++) {
        const pp_view_image &d = descs[i];
        if (d.h < 2 || d.w < 2 || d.th < 2 || d.tw < 2)
            return fail(PP_ESHAPE, w + ": a source or target edge < 2");
        if ((int64_t)d.h * d.w * 3 > INT32_MAX)
            return fail(PP_ESHAPE, w + ": source image out of range");
        if (d.H <= 0 || d.W <= 0 || (int64_t)d.H * d.W > INT32_MAX / 4)
            return fail(PP_ESHAPE, w + ": output size out of range");
        if (d.left < 0 || d.top < 0 || (int64_t)d.left + d.tw > d.W || (int64_t)d.top + d.th > d.H)
            return fail(PP_ESHAPE, w + ": the target does not fit its output with this pad");
        if (d.src_offset < 0 || d.src_offset > c.src_bytes ||
            (int64_t)d.h * d.w * 3 > c.src_bytes - d.src_offset)
            return fail(PP_ESHAPE, w + ": a source image beyond the source buffer");
        if (d.rot < 0 || d.rot > 3) return fail(PP_EINVAL, w + ": rot must be 0, 1, 2 or 3");
        if (d.rot != 0 && d.H != d.W)
            return fail(PP_ESHAPE, w + ": a turn needs a square output (H == W)");
        if (pyramid && d.H != d.W)
            return fail(PP_ESHAPE, w + ": reduced or mirrored views need a square output (H == W)");
        int v = 0;
        for (int ri = 0; ri < kViewReductions; ri++) {
            if (!((mask >> ri) & 1u)) continue;
            int nrows, ncols;
            view_size_of(ri, d.H, d.W, nrows, ncols);
            const int64_t elems = (int64_t)nrows * ncols * 3;
            for (int side = 0; side < (mirror ? 2 : 1); side++) {
                const int64_t off = view_offsets[(int64_t)i * n_views + v + side * n_red];
                if (off < 0 || off > c.out_elems || elems > c.out_elems - off)
                    return fail(PP_ESHAPE, w + ": " + c.beyond);
            }
            v++;
        }
        ViewImage &vi = (*images)[(size_t)i];
        PreImage &m = vi.m;
        m.src_offset = d.src_offset;
        m.out_offset = 0;
        m.h = d.h, m.w = d.w, m.th = d.th, m.tw = d.tw;
        m.left = d.left, m.top = d.top, m.H = d.H, m.W = d.W;
        m.zy = (double)(d.h - 1) / (double)(d.th - 1);
        m.zx = (double)(d.w - 1) / (double)(d.tw - 1);
        m.block0 = (int32_t)blocks;
        m.pad_ = 0;
        vi.rot = d.rot;
        vi.pad_ = 0;
        blocks += ((int64_t)d.H * d.W + kPreTile - 1) / kPreTile;
        if (blocks > INT32_MAX) return fail(PP_ESHAPE, w + ": too many output pixels for one launch");
    }
    *n_blocks = blocks;
    return PP_OK;
}

// pp_image_desc rows as `prepare` takes them: rot 0, the out_offsets as an (n_img, 1) offset
// table; to go with mask PP_VIEW_R1 and no mirror, for which none of the views-only checks
// can fire.  Without rows (which `prepare` refuses, or returns before reading one) both
// tables are NULL.
struct ImageRows {
    std::vector<pp_view_image> rows;
    std::vector<int64_t> offs;
    ImageRows(const pp_image_desc *descs, int32_t n_img) {
        if (!descs || n_img <= 0) return;
        rows.resize((size_t)n_img);
        offs.resize((size_t)n_img);
        for (int i = 0; i < n_img; i++) {
            const pp_image_desc &d = descs[i];
            rows[(size_t)i] = {d.src_offset, d.h, d.w, d.th, d.tw, d.left, d.top, d.H, d.W, 0, 0};
            offs[(size_t)i] = d.out_offset;
        }
    }
    const pp_view_image *images() const { return rows.empty() ? nullptr : rows.data(); }
    const int64_t *offsets() const { return offs.empty() ? nullptr : offs.data(); }
};

// f(std::integral_constant<int, DT>, layout) for the call's dtype; PP_PRE_U8 is always HWC
template <typename F>
static void with_dtype(int dtype, int layout, F &&f) {
    if (dtype == PP_PRE_F32)
        f(std::integral_constant<int, PP_PRE_F32>(), layout);
    else if (dtype == PP_PRE_F16)
        f(std::integral_constant<int, PP_PRE_F16>(), layout);
    else if (dtype == PP_PRE_BF16)
        f(std::integral_constant<int, PP_PRE_BF16>(), layout);
    else
        f(std::integral_constant<int, PP_PRE_U8>(), (int)PP_PRE_CHANNELS_LAST);
}

// The device entries' tables in d_tables, in one staging copy (a pageable host buffer is
// consumed before the copy call returns): the value table, the image records and (views) the
// offsets.  `*d_recs` is where the records went; the offsets follow them.
static int stage_tables(const Call &c, const void *recs, size_t recs_bytes, const int64_t *offs,
                        size_t offs_bytes, void *d_tables, size_t tables_bytes, hipStream_t s,
                        const char **d_recs) {
    const std::string w(c.who);
    if (!d_tables) return fail(PP_EINVAL, w + ": NULL argument");
    const size_t need = kLutBytes + recs_bytes + offs_bytes;
    if (tables_bytes < need) return fail(PP_ENOMEM, w + ": table buffer too small");
    if ((uintptr_t)d_tables & 7u) return fail(PP_EINVAL, w + ": misaligned buffer");
    std::vector<char> host(need);
    normalize_table(c.dtype, c.mean, c.stdv, (uint32_t *)host.data());
    memcpy(host.data() + kLutBytes, recs, recs_bytes);
    if (offs_bytes) memcpy(host.data() + kLutBytes + recs_bytes, offs, offs_bytes);
    if (hipMemcpyAsync(d_tables, host.data(), host.size(), hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PP_EHIP, w + ": staging the tables failed");
    }
    *d_recs = (const char *)d_tables + kLutBytes;
    return PP_OK;
}

template <int DT, int LAYOUT>
static void image_cpu(const uint8_t *src, const ViewImage &vi, const int64_t *offs, uint32_t mask,
                      bool mirror, int n_red, void *out_, const uint8_t *fill,
                      const uint32_t *lut) {
    using T = typename ViewElem<DT>::type;
    T *out = (T *)out_;
    const PreImage &m = vi.m;
    for (int yt = 0; yt < m.H; yt++)
        for (int xt = 0; xt < m.W; xt++) {
            int y, x;
            turned_source(vi.rot, m.H, yt, xt, y, x);
            uint8_t px[3];
            padded_pixel(load_taps(src, m, y, x), fill, px);
            uint32_t val[3];
            pixel_values<DT>(px, lut, val);
            int v = 0;
#define PP_VIEW_REDUCTION(RI)                                                                  \
    if ((mask >> RI) & 1u) {                                                                   \
        store_reduced<RI, T, LAYOUT>(out, offs[v], mirror ? offs[v + n_red] : 0, mirror, m.H,  \
                                     m.W, yt, xt, val);                                        \
        v++;                                                                                   \
    }
            PP_VIEW_REDUCTION(0)
            PP_VIEW_REDUCTION(1)
            PP_VIEW_REDUCTION(2)
            PP_VIEW_REDUCTION(3)
            PP_VIEW_REDUCTION(4)
#undef PP_VIEW_REDUCTION
        }
}

// the host twin of both kernels: the checks, then every image through image_cpu
static int twin(const Call &c, const pp_view_image *descs, const int64_t *view_offsets,
                int32_t reductions, int32_t mirror) {
    std::vector<ViewImage> recs;
    int64_t blocks = 0;
    const int rc = prepare(c, descs, view_offsets, reductions, mirror, &recs, &blocks);
    if (rc != PP_OK || c.n_img == 0) return rc;
    const uint32_t mask = (uint32_t)reductions;
    const int n_red = popcount5(mask), n_views = n_red * (mirror ? 2 : 1);
    const bool mir = mirror != 0;
    uint32_t lut[768];
    normalize_table(c.dtype, c.mean, c.stdv, lut);
    with_dtype(c.dtype, c.layout, [&](auto dt, int layout) {
        constexpr int DT = decltype(dt)::value;
        for (size_t i = 0; i < recs.size(); i++) {
            const int64_t *o = view_offsets + (int64_t)i * n_views;
            if (layout == PP_PRE_PLANAR)
                image_cpu<DT, PP_PRE_PLANAR>(c.src, recs[i], o, mask, mir, n_red, c.out, c.fill, lut);
            else
                image_cpu<DT, PP_PRE_CHANNELS_LAST>(c.src, recs[i], o, mask, mir, n_red, c.out,
                                                    c.fill, lut);
        }
    });
    return PP_OK;
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
    const Call c{"pp_preprocess_images", "an output region beyond the output buffer", d_src,
                 src_bytes, n_img, d_out, out_elems, dtype, layout, mean, stdv, fill};
    const ImageRows rows(descs, n_img);
    std::vector<ViewImage> recs;
    int64_t blocks = 0;
    const int rc = prepare(c, rows.images(), rows.offsets(), PP_VIEW_R1, 0, &recs, &blocks);
    if (rc != PP_OK || n_img == 0) return rc;
    std::vector<PreImage> images(recs.size());
    for (size_t i = 0; i < recs.size(); i++) {
        images[i] = recs[i].m;
        images[i].out_offset = descs[i].out_offset;
    }
    hipStream_t s = (hipStream_t)stream;
    PreArgs a{};
    const char *d_recs = nullptr;
    const int staged = stage_tables(c, images.data(), images.size() * sizeof(PreImage), nullptr, 0,
                                    d_tables, tables_bytes, s, &d_recs);
    if (staged != PP_OK) return staged;
    a.src = d_src;
    a.out = d_out;
    a.lut = (const uint32_t *)d_tables;
    a.images = (const PreImage *)d_recs;
    a.n_img = n_img;
    a.fill[0] = fill[0], a.fill[1] = fill[1], a.fill[2] = fill[2];
    with_dtype(dtype, layout,
               [&](auto dt, int lay) { launch<decltype(dt)::value>(lay, blocks, s, a); });
    return check_launch(c.who);
}

int pp_preprocess_images_cpu(const uint8_t *src, int64_t src_bytes, const pp_image_desc *descs,
                             int32_t n_img, void *out, int64_t out_elems, int32_t dtype,
                             int32_t layout, const float *mean, const float *stdv,
                             const uint8_t *fill) {
    const Call c{"pp_preprocess_images_cpu", "an output region beyond the output buffer", src,
                 src_bytes, n_img, out, out_elems, dtype, layout, mean, stdv, fill};
    const ImageRows rows(descs, n_img);
    return twin(c, rows.images(), rows.offsets(), PP_VIEW_R1, 0);
}

size_t pp_preprocess_views_tables_size(int32_t n_img, int32_t n_views) {
    if (n_img <= 0 || n_views <= 0) return 0;
    return kLutBytes + (size_t)n_img * sizeof(ViewImage) +
           (size_t)n_img * (size_t)n_views * sizeof(int64_t);
}

int pp_preprocess_views(const uint8_t *d_src, int64_t src_bytes, const pp_view_image *images,
                        const int64_t *view_offsets, int32_t n_img, int32_t reductions,
                        int32_t mirror, void *d_out, int64_t out_elems, int32_t dtype,
                        int32_t layout, const float *mean, const float *stdv, const uint8_t *fill,
                        void *d_tables, size_t tables_bytes, void *stream) {
    const Call c{"pp_preprocess_views", "a view region beyond the output buffer", d_src,
                 src_bytes, n_img, d_out, out_elems, dtype, layout, mean, stdv, fill};
    std::vector<ViewImage> recs;
    int64_t blocks = 0;
    const int rc = prepare(c, images, view_offsets, reductions, mirror, &recs, &blocks);
    if (rc != PP_OK || n_img == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    ViewArgs a{};
    a.mask = (uint32_t)reductions;
    a.n_red = popcount5(a.mask);
    a.n_views = a.n_red * (mirror ? 2 : 1);
    const size_t recs_bytes = recs.size() * sizeof(ViewImage);
    const char *d_recs = nullptr;
    const int staged = stage_tables(c, recs.data(), recs_bytes, view_offsets,
                                    (size_t)n_img * (size_t)a.n_views * sizeof(int64_t), d_tables,
                                    tables_bytes, s, &d_recs);
    if (staged != PP_OK) return staged;
    a.src = d_src;
    a.out = d_out;
    a.lut = (const uint32_t *)d_tables;
    a.images = (const ViewImage *)d_recs;
    a.offs = (const int64_t *)(d_recs + recs_bytes);
    a.n_img = n_img;
    a.mirror = mirror ? 1 : 0;
    a.fill[0] = fill[0], a.fill[1] = fill[1], a.fill[2] = fill[2];
    with_dtype(dtype, layout,
               [&](auto dt, int lay) { launch<decltype(dt)::value>(lay, blocks, s, a); });
    return check_launch(c.who);
}

int pp_preprocess_views_cpu(const uint8_t *src, int64_t src_bytes, const pp_view_image *images,
                            const int64_t *view_offsets, int32_t n_img, int32_t reductions,
                            int32_t mirror, void *out, int64_t out_elems, int32_t dtype,
                            int32_t layout, const float *mean, const float *stdv,
                            const uint8_t *fill) {
    const Call c{"pp_preprocess_views_cpu", "a view region beyond the output buffer", src,
                 src_bytes, n_img, out, out_elems, dtype, layout, mean, stdv, fill};
    return twin(c, images, view_offsets, reductions, mirror);
}

}  // extern "C"

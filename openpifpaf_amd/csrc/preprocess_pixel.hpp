// preprocess_pixel.hpp — the per-pixel code of the eval preprocessing kernels
// (preprocess.hip: pp_preprocess_images and pp_preprocess_views) and of their host twin: the image record, the zoom of one axis, the bilinear blend, the taps of
// one output pixel, the padded pixel, the output index and store, and the host's value table.
// Every function a kernel calls is __host__ __device__, so a kernel and its twin agree bit
// for bit by construction.  preprocess.hip's head comment has the arithmetic and why no
// operation may be fused.
#pragma once
#pragma clang fp contract(off)

#include "pp_common.hpp"

namespace pp {

// one image as the kernel reads it: the caller's descriptor, the two zoom factors (one
// float64 division each, done once on the host) and the image's first workgroup
struct PreImage {
    int64_t src_offset, out_offset;
    int32_t h, w, th, tw, left, top, H, W;
    double zy, zx;
    int32_t block0, pad_;
};
static_assert(sizeof(PreImage) == 72, "PreImage layout");

// one axis of the zoom at output index i: taps i0, i1 with weights w0, w1; out: the
// coordinate lies beyond the last source index n - 1 (floating-point comparison)
struct Axis {
    int i0, i1;
    double w0, w1;
    bool out;
};
__host__ __device__ __forceinline__ Axis zoom_axis(int i, double z, int n) {
    const double y = (double)i * z;
    const double fl = __builtin_floor(y);
    int y0 = (int)fl;
    const double fy = y - fl;
    Axis a;
    a.w0 = 1.0 - fy;
    a.w1 = 1.0 - a.w0;
    a.out = y > (double)(n - 1);
    y0 = y0 < n - 1 ? y0 : n - 1;
    a.i0 = y0;
    a.i1 = y0 + 1 < n - 1 ? y0 + 1 : n - 1;
    return a;
}

__host__ __device__ __forceinline__ uint8_t zoom_blend(double a, double b, double c, double d,
                                                       const Axis &ay, const Axis &ax) {
    double t = ((a * ay.w0) * ax.w0 + (b * ay.w0) * ax.w1) + (c * ay.w1) * ax.w0;
    t = t + (d * ay.w1) * ax.w1;
    if (!(t > 0.0)) return 0;
    t = t + 0.5;
    return (uint8_t)(int)(t < 255.0 ? t : 255.0);
}

// The taps of output pixel (y, x) of image m: the two axes and the 4 x 3 source bytes.  A
// pixel outside the rescaled region [top, top + th) x [left, left + tw) takes the nearest one
// inside (and drops its value later), so the loads are unconditional and those of a lane's
// several pixels can be in flight together.
struct Taps {
    Axis ay, ax;
    uint32_t v[4][3];  // a, b, c, d
    bool inside;
};
__host__ __device__ __forceinline__ Taps load_taps(const uint8_t *__restrict__ src,
                                                   const PreImage &m, int y, int x) {
    Taps t;
    const int i = y - m.top, j = x - m.left;
    t.inside = i >= 0 && i < m.th && j >= 0 && j < m.tw;
    const int ic = i < 0 ? 0 : i < m.th ? i : m.th - 1, jc = j < 0 ? 0 : j < m.tw ? j : m.tw - 1;
    t.ay = zoom_axis(ic, m.zy, m.h);
    t.ax = zoom_axis(jc, m.zx, m.w);
    const uint8_t *s = src + m.src_offset;
    // h * w * 3 <= INT32_MAX (checked on the host): 32-bit offsets inside the image
    const int r0 = t.ay.i0 * m.w, r1 = t.ay.i1 * m.w;
    const uint8_t *p[4] = {s + (r0 + t.ax.i0) * 3, s + (r0 + t.ax.i1) * 3,
                           s + (r1 + t.ax.i0) * 3, s + (r1 + t.ax.i1) * 3};
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int c = 0; c < 3; c++) t.v[q][c] = p[q][c];
    return t;
}

// the three channels of that pixel as the reference holds them before ToTensor: the
// rescaled image inside the region, fill outside
__host__ __device__ __forceinline__ void padded_pixel(const Taps &t, const uint8_t fill[3],
                                                      uint8_t px[3]) {
    const bool black = t.ay.out || t.ax.out;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint8_t v = zoom_blend((double)t.v[0][c], (double)t.v[1][c], (double)t.v[2][c],
                                     (double)t.v[3][c], t.ay, t.ax);
        px[c] = !t.inside ? fill[c] : black ? (uint8_t)0 : v;
    }
}

// element `p` (row-major pixel) channel c of an image's output region
template <int LAYOUT>
__host__ __device__ __forceinline__ int64_t out_index(const PreImage &m, int64_t p, int c) {
    return LAYOUT == PP_PRE_PLANAR ? m.out_offset + (int64_t)c * m.H * m.W + p
                                   : m.out_offset + 3 * p + c;
}

template <typename T, int LAYOUT>
__host__ __device__ __forceinline__ void store_pixel(void *out, const PreImage &m, int64_t p,
                                                     const uint8_t px[3], const uint32_t *lut) {
    T *o = (T *)out;
#pragma unroll
    for (int c = 0; c < 3; c++) o[out_index<LAYOUT>(m, p, c)] = (T)lut[c * 256 + px[c]];
}

// float32 -> float16 bits, round to nearest even (subnormals, overflow to inf, NaN kept)
static uint16_t f16_bits(float f) {
    const uint32_t u = u32_of(f);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t abs = u & 0x7fffffffu;
    if (abs >= 0x7f800000u) return (uint16_t)(sign | (abs > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (abs >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to inf
    if (abs < 0x33000001u) return sign;  // <= 2^-25 rounds to 0 (the tie goes to even)
    const int e = (int)(abs >> 23) - 127;
    uint32_t mant = (abs & 0x7fffffu) | 0x800000u;
    int shift;  // bits of mant dropped
    uint32_t base;
    if (e >= -14) {
        shift = 13;
        base = (uint32_t)(e + 15) << 10;
        mant &= 0x7fffffu;
    } else {
        shift = 13 + (-14 - e);
        base = 0;
    }
    uint32_t q = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (q & 1u))) q++;
    return (uint16_t)(sign | (base + q));  // a carry runs into the exponent as it should
}

// float32 -> bfloat16 bits, round to nearest even (NaN kept quiet)
static uint16_t bf16_bits(float f) {
    const uint32_t u = u32_of(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// EVAL_TRANSFORM per channel and byte value: ToTensor's u8 / 255 and Normalize's
// (v - mean) / std, each one IEEE float32 operation, then the output's format
static void normalize_table(int dtype, const float *mean, const float *stdv, uint32_t *lut) {
    for (int c = 0; c < 3; c++)
        for (int v = 0; v < 256; v++) {
            volatile float t = (float)v / 255.0f;
            volatile float d = t - mean[c];
            const float r = d / stdv[c];
            lut[c * 256 + v] = dtype == PP_PRE_F16    ? f16_bits(r)
                               : dtype == PP_PRE_BF16 ? bf16_bits(r)
                                                      : u32_of(r);
        }
}

static size_t elem_size(int dtype) {
    return dtype == PP_PRE_F32 ? 4 : dtype == PP_PRE_U8 ? 1 : 2;
}

}  // namespace pp

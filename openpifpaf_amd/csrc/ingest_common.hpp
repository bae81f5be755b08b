// ingest_common.hpp — what the ingest kernel families (ingest.hip, ingest_heads.hip) share:
// the kernel arguments of one head, the hflip tables, the conv value as float32, the head's
// and collector's arithmetic, the index logic of the planar kernels as macros, and the host
// checks that derive the arguments from a head's layout.
#pragma once

#include <hip/hip_fp16.h>

#include "pp_common.hpp"

namespace pp {

constexpr int kMaxOutCh = 16;
constexpr int kMaxTableFields = 64;  // src_field / swap_ends travel in the kernel arguments

struct IngestArgs {
    const void *conv;    // (n_img, n_fields * n_per_field * 4^quad, h, w)
    float *out;          // (n_img, out_fields, n_out, H, W)
    int n_img, n_fields, h, w, H, W, quad;
    int n_conf, n_vec, n_scales, n_out;
    int out_fields, out_field0;  // fields per image of `out`, first field written
    int64_t conv_ch;     // channels per image of the conv output
    // per output channel: conv channel group offset and stride per field, component, op
    int grp_off[kMaxOutCh];  // first conv channel of the component's group (pre-dequad units)
    int fld_mul[kMaxOutCh];  // channels per field inside the group
    int comp[kMaxOutCh];     // component inside the field
    int op[kMaxOutCh];       // 0 copy, 1 sigmoid, 2 exp, 3 + x index, 4 + y index
};

// the hflip tables of the kEx kernel (unused by the plain one)
struct IngestFlip {
    int mirror;                          // output column X reads source column W-1-X
    int has_src;                         // src_field[] is set (else field f reads field f)
    uint64_t swap_mask;                  // bit f: CAF field f trades (x1, y1) and (x2, y2)
    uint8_t src_field[kMaxTableFields];  // output field f reads conv field src_field[f]
};

struct Bf16 {
    uint16_t bits;
};

// the conv value as float32, exactly
__device__ __forceinline__ float load_f32(const float *p) { return *p; }
__device__ __forceinline__ float load_f32(const __half *p) { return __half2float(*p); }
__device__ __forceinline__ float load_f32(const Bf16 *p) {
    return __uint_as_float((uint32_t)p->bits << 16);
}

// what the head and its collector do to one conv value (both kernels call this)
__device__ __forceinline__ float ingest_value(int op, float v, bool mirror, int X, int Y) {
    float r;
    switch (op) {
        case 1: r = (float)(1.0 / (1.0 + exp(-(double)v))); break;  // torch.sigmoid
        case 2: r = (float)exp((double)v); break;                  // torch.exp
        case 3: r = (mirror ? -v : v) + (float)X; break;           // + index_field x
        case 4: r = v + (float)Y; break;                           // + index_field y
        default: r = v;
    }
    return r;
}

// The index logic the planar kernels share, for output pixel (X, Y) of output field f
// inside a kernel<T, kEx> with IngestArgs a and IngestFlip t.  It is text, not a function:
// as force-inlined functions the same lines compiled to other code in all twelve existing
// instantiations, and the hflip ones ran 20 to 32 % slower (DESIGN.md §4 "Ragged ingest").
// A file that uses them #undefs both after its last kernel.
//
// PP_INGEST_PIXEL(W_own) declares the conv field fs, mirror / swap (the columns are mirrored
// about W_own, the width of the image's own field; the CAF end points trade places) and the
// conv pixel (y0, x0).  It undoes the dequads: T_q[c, Y, X] = T_{q-1}[4c + 2(Y&1) + (X&1),
// Y>>1, X>>1], so the conv channel is mul * c + sub, mul = 4^quad, with the finest level's
// offset the most significant.
#define PP_INGEST_PIXEL(W_own)                                      \
    int fs = f;                                                     \
    bool mirror = false, swap = false;                              \
    if (kEx) {                                                      \
        mirror = t.mirror != 0;                                     \
        if (t.has_src) fs = t.src_field[f];                         \
        swap = f < kMaxTableFields && ((t.swap_mask >> f) & 1);     \
    }                                                               \
    int sub = 0, y0 = Y, x0 = mirror ? (W_own) - 1 - X : X, mul = 1; \
    for (int q = 0; q < a.quad; q++) {                              \
        sub = 4 * sub + (2 * (y0 & 1) + (x0 & 1));                  \
        mul *= 4;                                                   \
        y0 >>= 1;                                                   \
        x0 >>= 1;                                                   \
    }

// PP_INGEST_CHANNEL(o) declares op and the conv channel ch that output channel o reads.  The
// end points trade places in the regressions only (heads.py:209-212); CAF's four vector
// components are exactly its ops 3 / 4.
#define PP_INGEST_CHANNEL(o)                                \
    const int op = a.op[o];                                 \
    int comp = a.comp[o];                                   \
    if (kEx && swap && (op == 3 || op == 4)) comp ^= 2;     \
    const int64_t ch = (int64_t)(a.grp_off[o] + fs * a.fld_mul[o] + comp) * mul + sub;

// The checks every ingest symbol shares after its NULL and shape checks, and the kernel
// arguments that do not depend on the images' sizes or addresses (n_fields > 0, 0 <= quad <= 4).
int ingest_setup(const std::string &name, int32_t conv_dtype, int32_t n_fields, int32_t layout,
                 int32_t quad, int32_t mirror, const int32_t *src_field,
                 const uint8_t *swap_ends, int32_t out_fields, int32_t out_field0, IngestArgs &a,
                 IngestFlip &t);

}  // namespace pp

// ingest.hip — head conv outputs -> decoder fields, one pass over HBM.
//
// Replaces the eval-mode tail of CompositeFieldFused.forward (network/heads.py:406-455):
// `quad` PixelShuffle(2) dequads with the last row / column cropped, sigmoid on the
// confidences, exp on the scales; and CifCafCollector / CifdetCollector.forward
// (heads.py:65-88, 127-144): per-field concatenation, the index grid added to the vector
// components, the channel reorder.  The result is what the decoder consumes, written
// straight from the conv output (no intermediate tensors, no host copy).
//
// pp_fields_from_conv_ex also undoes the horizontal flip of a mirrored pass in the same
// read, as PifHFlip / PafHFlip do on the unfused head's list (heads.py:145-214): the
// left / right field permutation, the mirrored columns, the negated x offsets and the
// exchanged CAF end points; it reads f32, f16 or bf16 conv outputs and can write into a
// field range of a wider output tensor.
//
// Work unit: one thread per output pixel of one (image, field); it writes every output
// channel of that field.  Reads and writes are coalesced along x (a mirrored wave reads
// the same contiguous segment, back to front).
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

template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_kernel(IngestArgs a, IngestFlip t) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)a.H * a.W;
    const int f = blockIdx.y, img = blockIdx.z;
    if (pix >= HW) return;
    const int Y = (int)(pix / a.W), X = (int)(pix % a.W);
    int fs = f;
    bool mirror = false, swap = false;
    if (kEx) {
        mirror = t.mirror != 0;
        if (t.has_src) fs = t.src_field[f];
        swap = f < kMaxTableFields && ((t.swap_mask >> f) & 1);
    }
    // undo the dequads: T_q[c, Y, X] = T_{q-1}[4c + 2(Y&1) + (X&1), Y>>1, X>>1], so the
    // conv channel is 4^quad * c + sub with the finest level's offset the most significant
    int sub = 0, y0 = Y, x0 = mirror ? a.W - 1 - X : X, mul = 1;
    for (int q = 0; q < a.quad; q++) {
        sub = 4 * sub + (2 * (y0 & 1) + (x0 & 1));
        mul *= 4;
        y0 >>= 1;
        x0 >>= 1;
    }
    const T *src = (const T *)a.conv + (int64_t)img * a.conv_ch * a.h * a.w + (int64_t)y0 * a.w + x0;
    float *dst = a.out + (((int64_t)img * a.out_fields + a.out_field0 + f) * a.n_out) * HW + pix;
    for (int o = 0; o < a.n_out; o++) {
        const int op = a.op[o];
        int comp = a.comp[o];
        // the end points trade places in the regressions only (heads.py:209-212); CAF's
        // four vector components are exactly its ops 3 / 4
        if (kEx && swap && (op == 3 || op == 4)) comp ^= 2;
        const int64_t ch = (int64_t)(a.grp_off[o] + fs * a.fld_mul[o] + comp) * mul + sub;
        const float v = load_f32(src + ch * a.h * a.w);
        float r;
        switch (op) {
            case 1: r = (float)(1.0 / (1.0 + exp(-(double)v))); break;  // torch.sigmoid
            case 2: r = (float)exp((double)v); break;                  // torch.exp
            case 3: r = (mirror ? -v : v) + (float)X; break;           // + index_field x
            case 4: r = v + (float)Y; break;                           // + index_field y
            default: r = v;
        }
        dst[(int64_t)o * HW] = r;
    }
}

template <typename T>
static void launch_ingest(const IngestArgs &a, const IngestFlip &t, bool ex, hipStream_t stream) {
    const int64_t HW = (int64_t)a.H * a.W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)a.n_fields, (unsigned)a.n_img);
    if (ex)
        hipLaunchKernelGGL((ingest_kernel<T, true>), grid, dim3(256), 0, stream, a, t);
    else
        hipLaunchKernelGGL((ingest_kernel<T, false>), grid, dim3(256), 0, stream, a, t);
}

}  // namespace pp

using namespace pp;

extern "C" {

int64_t pp_fields_dim(int64_t n, int32_t quad) {
    for (int q = 0; q < quad; q++) n = 2 * n - 1;  // PixelShuffle(2) then [:-1]
    return n;
}

static int fields_from_conv(const char *who, const void *d_conv, int32_t conv_dtype,
                            int32_t n_img, int32_t n_fields, int32_t layout, int32_t h,
                            int32_t w, int32_t quad, int32_t mirror, const int32_t *src_field,
                            const uint8_t *swap_ends, float *d_out, int32_t out_fields,
                            int32_t out_field0, void *stream) {
    const std::string name(who);
    if (!d_conv || !d_out) return fail(PP_EINVAL, name + ": NULL argument");
    if (n_img < 0 || n_fields <= 0 || h <= 0 || w <= 0 || quad < 0 || quad > 4)
        return fail(PP_ESHAPE, name + ": bad shape");
    IngestArgs a{};
    IngestFlip t{};
    // (n_confidences, n_vectors, n_scales) of IntensityMeta / AssociationMeta /
    // DetectionMeta (heads.py:218-265) and the collector's output channel order
    static const int metas[3][3] = {{1, 1, 1}, {1, 2, 2}, {1, 2, 0}};
    // concatenated per-field channels: conf..., vec0 x, vec0 y, vec1 x, ..., logb..., scale...
    // output channel -> concatenated channel (heads.py:87 for CAF, :142 for CifDet)
    static const int perm[3][9] = {{0, 1, 2, 3, 4, 0, 0, 0, 0},
                                   {0, 1, 2, 5, 7, 3, 4, 6, 8},
                                   {0, 1, 2, 5, 3, 4, 6, 0, 0}};
    static const int n_out[3] = {5, 9, 7};
    if (layout < 0 || layout > 2) return fail(PP_EINVAL, name + ": layout 0 CIF, 1 CAF, 2 CifDet");
    if (conv_dtype < PP_DTYPE_F32 || conv_dtype > PP_DTYPE_BF16)
        return fail(PP_EINVAL, name + ": dtype 0 f32, 1 f16, 2 bf16");
    if ((src_field || swap_ends) && n_fields > kMaxTableFields)
        return fail(PP_ESHAPE, name + ": src_field / swap_ends hold at most 64 fields");
    if (swap_ends && layout != 1)
        return fail(PP_EINVAL, name + ": swap_ends needs the CAF layout");
    if (out_field0 < 0 || (int64_t)out_field0 + n_fields > out_fields)
        return fail(PP_ESHAPE, name + ": fields out_field0.. do not fit in out_fields");
    if (src_field) {
        t.has_src = 1;
        for (int f = 0; f < n_fields; f++) {
            if (src_field[f] < 0 || src_field[f] >= n_fields)
                return fail(PP_EINVAL, name + ": src_field entry outside [0, n_fields)");
            t.src_field[f] = (uint8_t)src_field[f];
        }
    }
    if (swap_ends)
        for (int f = 0; f < n_fields; f++)
            if (swap_ends[f]) t.swap_mask |= (uint64_t)1 << f;
    t.mirror = mirror != 0;
    a.conv = d_conv;
    a.out = d_out;
    a.n_img = n_img;
    a.n_fields = n_fields;
    a.h = h;
    a.w = w;
    a.quad = quad;
    a.H = (int)pp_fields_dim(h, quad);
    a.W = (int)pp_fields_dim(w, quad);
    a.n_conf = metas[layout][0];
    a.n_vec = metas[layout][1];
    a.n_scales = metas[layout][2];
    a.n_out = n_out[layout];
    a.out_fields = out_fields;
    a.out_field0 = out_field0;
    const int F0 = a.n_conf * n_fields, F1 = F0 + 2 * a.n_vec * n_fields,
              F2 = F1 + a.n_vec * n_fields, F3 = F2 + a.n_scales * n_fields;
    a.conv_ch = (int64_t)F3 << (2 * quad);
    const int nc = a.n_conf, nv2 = 2 * a.n_vec, nv = a.n_vec;
    for (int o = 0; o < a.n_out; o++) {
        const int q = perm[layout][o];
        if (q < nc) {  // confidences: sigmoid
            a.grp_off[o] = 0;
            a.fld_mul[o] = nc;
            a.comp[o] = q;
            a.op[o] = 1;
        } else if (q < nc + nv2) {  // vectors: index added to the first (CifDet) or all
            const int c = q - nc;
            a.grp_off[o] = F0;
            a.fld_mul[o] = nv2;
            a.comp[o] = c;
            const bool indexed = layout != 2 || c < 2;
            a.op[o] = indexed ? ((c & 1) ? 4 : 3) : 0;
        } else if (q < nc + nv2 + nv) {  // logb: as is
            a.grp_off[o] = F1;
            a.fld_mul[o] = nv;
            a.comp[o] = q - nc - nv2;
            a.op[o] = 0;
        } else {  // scales: exp
            a.grp_off[o] = F2;
            a.fld_mul[o] = a.n_scales;
            a.comp[o] = q - nc - nv2 - nv;
            a.op[o] = 2;
        }
    }
    if (n_img == 0) return PP_OK;
    // the plain f32 ingest keeps its own instantiation without the table reads
    const bool ex = t.mirror || t.has_src || t.swap_mask;
    if (conv_dtype == PP_DTYPE_F32)
        launch_ingest<float>(a, t, ex, (hipStream_t)stream);
    else if (conv_dtype == PP_DTYPE_F16)
        launch_ingest<__half>(a, t, ex, (hipStream_t)stream);
    else
        launch_ingest<Bf16>(a, t, ex, (hipStream_t)stream);
    return check_launch(who);
}

int pp_fields_from_conv_ex(const void *d_conv, int32_t conv_dtype, int32_t n_img,
                           int32_t n_fields, int32_t layout, int32_t h, int32_t w, int32_t quad,
                           int32_t mirror, const int32_t *src_field, const uint8_t *swap_ends,
                           float *d_out, int32_t out_fields, int32_t out_field0, void *stream) {
    return fields_from_conv("pp_fields_from_conv_ex", d_conv, conv_dtype, n_img, n_fields,
                            layout, h, w, quad, mirror, src_field, swap_ends, d_out, out_fields,
                            out_field0, stream);
}

int pp_fields_from_conv(const float *d_conv, int32_t n_img, int32_t n_fields, int32_t layout,
                        int32_t h, int32_t w, int32_t quad, float *d_out, void *stream) {
    return fields_from_conv("pp_fields_from_conv", d_conv, PP_DTYPE_F32, n_img, n_fields,
                            layout, h, w, quad, 0, nullptr, nullptr, d_out, n_fields, 0, stream);
}

}  // extern "C"

// ingest_heads.hip — pp_fields_from_conv_ragged_heads: the conv outputs of every head of a
// multi-scale FieldConfig, n images of their own sizes each, straight into the containers of
// a ragged head set in one launch (ingest_ragged_heads_kernel).
//
// An entry is one conv head and the field range of one container it writes (pp_conv_head).
// The workgroups of entry 0 come first on the x grid, then entry 1's; a workgroup finds its
// entry from a prefix table of workgroup counts held in the kernel arguments, as
// ragged_pack_heads_kernel does (ragged.hip), and then is ingest_ragged_kernel's work unit
// (ingest.hip) on that entry's container: one thread per container pixel of one (image,
// field), all output channels, the ingested value inside the image's own field and +0
// outside it with no load.  The entry and the image (blockIdx.y) are uniform per workgroup,
// so the entry's descriptor, the pointer, the strides and the extents are scalar loads.
//
// The descriptors are the caller's pp_conv_head rows, copied to the device with the other
// host tables; what ingest_setup derives from a layout alone (the per-channel tables) is the
// same for every entry of that layout but for a factor n_fields and travels in the kernel
// arguments, once per layout.
#include "ingest_common.hpp"

#include <algorithm>
#include <vector>

namespace pp {

constexpr int kMaxConvHeads = 3 * PP_MAX_SCALES;

// ingest_setup's per-channel tables of layouts 0 (CIF) and 1 (CAF) for n_fields = 1: the
// group offset of an entry is grp_off * n_fields
struct HeadChannels {
    int n_out[2];
    int grp_off[2][kMaxOutCh], fld_mul[2][kMaxOutCh], comp[2][kMaxOutCh], op[2][kMaxOutCh];
};

struct IngestHeads {
    const void *const *conv;  // (n_entries, n_img)
    const int64_t *strides;   // (n_entries, n_img, 2) channel, row; or NULL: every view dense
    const int32_t *conv_ext;  // (n_entries, n_img, 2) h_i, w_i
    int32_t *field_ext;       // (n_rows, n_img, 2) H_i, W_i, written here
    int n_img, n_entries, quad;
    int first[kMaxConvHeads + 1];  // first workgroup of entry m on the x grid
};

// what PP_INGEST_PIXEL / PP_INGEST_CHANNEL read of IngestArgs, for one entry
struct HeadView {
    struct Scaled {
        const int *v;
        int k;
        __device__ __forceinline__ int operator[](int o) const { return v[o] * k; }
    };
    int quad;
    Scaled grp_off;
    const int *fld_mul, *comp, *op;
};

template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_ragged_heads_kernel(
    const pp_conv_head *__restrict__ heads, IngestHeads r, HeadChannels c) {
    const int b = (int)blockIdx.x, img = (int)blockIdx.y;
    // the entry: selects over constant indices of the kernel arguments (ragged_pack_heads_kernel)
    int m = 0, first = 0;
#pragma unroll
    for (int e = 1; e < kMaxConvHeads; e++)
        if (e < r.n_entries && b >= r.first[e]) {
            m = e;
            first = r.first[e];
        }
    const pp_conv_head &t = heads[m];
    const int H = t.H, W = t.W, n_fields = t.n_fields, caf = t.layout;
    const int out_fields = t.out_fields, out_field0 = t.out_field0, ext_row = t.ext_row;
    float *const out = t.d_container;
    const int64_t HW = (int64_t)H * W;
    const int per_plane = (int)((HW + 255) / 256);  // workgroups per (image, field) plane
    const int wb = b - first;
    const int f = wb / per_plane, px = wb - f * per_plane;
    const int64_t row = (int64_t)m * r.n_img + img;
    const int h = r.conv_ext[2 * row], w = r.conv_ext[2 * row + 1];
    const int64_t s_ch = r.strides ? r.strides[2 * row] : (int64_t)h * w;
    const int64_t s_row = r.strides ? r.strides[2 * row + 1] : (int64_t)w;
    const T *const conv = (const T *)r.conv[row];
    int Hi = h, Wi = w;
    for (int q = 0; q < r.quad; q++) {  // pp_fields_dim
        Hi = 2 * Hi - 1;
        Wi = 2 * Wi - 1;
    }
    if (wb == 0 && ext_row >= 0 && threadIdx.x == 0) {
        int32_t *ext = r.field_ext + 2 * ((int64_t)ext_row * r.n_img + img);
        ext[0] = Hi;
        ext[1] = Wi;
    }
    const int64_t pix = (int64_t)px * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int n_out = caf ? c.n_out[1] : c.n_out[0];
    const int Y = (int)(pix / W), X = (int)(pix % W);
    // the container pointer comes from memory: say that it is global, as a.out of the
    // single-head kernels is known to be, so that the stores are global and not flat
    typedef __attribute__((address_space(1))) float GlobalFloat;
    GlobalFloat *dst = (GlobalFloat *)(out + (((int64_t)img * out_fields + out_field0 + f) * n_out) * HW + pix);
    if (Y >= Hi || X >= Wi) {
        for (int o = 0; o < n_out; o++) dst[(int64_t)o * HW] = 0.0f;
        return;
    }
    HeadView a;
    a.quad = r.quad;
    a.grp_off = HeadView::Scaled{caf ? c.grp_off[1] : c.grp_off[0], n_fields};
    a.fld_mul = caf ? c.fld_mul[1] : c.fld_mul[0];
    a.comp = caf ? c.comp[1] : c.comp[0];
    a.op = caf ? c.op[1] : c.op[0];
    PP_INGEST_PIXEL(Wi)
    // a stride whose extent is 1 meets index 0 only (h = 1: y0 = 0)
    const T *src = conv + (int64_t)y0 * s_row + x0;
    for (int o = 0; o < n_out; o++) {
        PP_INGEST_CHANNEL(o)
        const float v = load_f32(src + ch * s_ch);
        dst[(int64_t)o * HW] = ingest_value(op, v, mirror, X, Y);
    }
}

#undef PP_INGEST_PIXEL
#undef PP_INGEST_CHANNEL

template <typename T>
static void launch_ingest_heads(const pp_conv_head *d_heads, const IngestHeads &r,
                                const HeadChannels &c, bool ex, hipStream_t stream) {
    const dim3 grid((unsigned)r.first[r.n_entries], (unsigned)r.n_img);
    if (ex)
        hipLaunchKernelGGL((ingest_ragged_heads_kernel<T, true>), grid, dim3(256), 0, stream,
                           d_heads, r, c);
    else
        hipLaunchKernelGGL((ingest_ragged_heads_kernel<T, false>), grid, dim3(256), 0, stream,
                           d_heads, r, c);
}

// byte offsets of the tables inside d_tables (n = n_entries * n_img rows)
struct HeadsLayout {
    size_t strides, heads, conv_ext, field_ext, size;
};
static HeadsLayout heads_layout(int32_t n_img, int32_t n_entries) {
    HeadsLayout l{};
    if (n_img <= 0 || n_entries <= 0 || n_entries > kMaxConvHeads) return l;
    const size_t n = (size_t)n_entries * n_img;
    l.strides = n * sizeof(void *);
    l.heads = l.strides + n * 2 * sizeof(int64_t);
    l.conv_ext = l.heads + (size_t)n_entries * sizeof(pp_conv_head);
    l.field_ext = l.conv_ext + n * 2 * sizeof(int32_t);
    l.size = l.field_ext + n * 2 * sizeof(int32_t);
    return l;
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_conv_head_set_flip(pp_conv_head *head, int32_t mirror, const int32_t *src_field,
                          const uint8_t *swap_ends) {
    const std::string name = "pp_conv_head_set_flip";
    if (!head) return fail(PP_EINVAL, name + ": NULL argument");
    const int n_fields = head->n_fields;
    if (n_fields <= 0) return fail(PP_ESHAPE, name + ": bad shape");
    if ((src_field || swap_ends) && n_fields > kMaxTableFields)
        return fail(PP_ESHAPE, name + ": src_field / swap_ends hold at most 64 fields");
    if (swap_ends && head->layout != 1)
        return fail(PP_EINVAL, name + ": swap_ends needs the CAF layout");
    if (src_field)
        for (int f = 0; f < n_fields; f++)
            if (src_field[f] < 0 || src_field[f] >= n_fields)
                return fail(PP_EINVAL, name + ": src_field entry outside [0, n_fields)");
    head->mirror = mirror != 0;
    head->has_src = src_field != nullptr;
    head->swap_mask = 0;
    for (int f = 0; f < kMaxTableFields; f++)
        head->src_field[f] = (uint8_t)(src_field && f < n_fields ? src_field[f] : 0);
    if (swap_ends)
        for (int f = 0; f < n_fields; f++)
            if (swap_ends[f]) head->swap_mask |= (uint64_t)1 << f;
    return PP_OK;
}

size_t pp_ragged_conv_heads_tables_size(int32_t n_img, int32_t n_entries) {
    return heads_layout(n_img, n_entries).size;
}

size_t pp_ragged_conv_heads_extents_offset(int32_t n_img, int32_t n_entries) {
    return heads_layout(n_img, n_entries).field_ext;
}

int pp_fields_from_conv_ragged_heads(const pp_conv_head *heads, int32_t n_entries,
                                     int32_t n_rows, const void *const *convs,
                                     const int32_t *conv_extents, const int64_t *conv_strides,
                                     int32_t n_img, int32_t conv_dtype, int32_t quad,
                                     void *d_tables, size_t tables_bytes, void *stream) {
    const std::string name = "pp_fields_from_conv_ragged_heads";
    if (!heads || !convs || !conv_extents || !d_tables)
        return fail(PP_EINVAL, name + ": NULL argument");
    if (n_img < 0 || n_entries <= 0 || n_entries > kMaxConvHeads || n_rows <= 0 ||
        n_rows > n_entries || quad < 0 || quad > 4)
        return fail(PP_ESHAPE, name + ": bad shape (1 .. 3 * PP_MAX_SCALES entries, 1 .. "
                    "n_entries extent rows)");
    if (conv_dtype < PP_DTYPE_F32 || conv_dtype > PP_DTYPE_BF16)
        return fail(PP_EINVAL, name + ": dtype 0 f32, 1 f16, 2 bf16");
    // the per-channel tables of the two layouts, from the one statement of them
    HeadChannels c{};
    for (int layout = 0; layout < 2; layout++) {
        IngestArgs a{};
        IngestFlip t{};
        if (const int rc = ingest_setup(name, conv_dtype, 1, layout, quad, 0, nullptr, nullptr, 1,
                                        0, a, t))
            return rc;
        c.n_out[layout] = a.n_out;
        for (int o = 0; o < kMaxOutCh; o++) {
            c.grp_off[layout][o] = a.grp_off[o];
            c.fld_mul[layout][o] = a.fld_mul[o];
            c.comp[layout][o] = a.comp[o];
            c.op[layout][o] = a.op[o];
        }
    }
    IngestHeads r{};
    bool ex = false;
    int64_t total = 0;  // workgroups of one image over all entries
    for (int m = 0; m < n_entries; m++) {
        const pp_conv_head &e = heads[m];
        const std::string at = name + ": entry " + std::to_string(m);
        if (!e.d_container) return fail(PP_EINVAL, at + ": NULL container");
        if (e.n_fields <= 0 || e.H <= 0 || e.W <= 0) return fail(PP_ESHAPE, at + ": bad shape");
        if (e.layout < 0 || e.layout > 1)
            return fail(PP_EINVAL, at + ": layout 0 CIF or 1 CAF (no multi-head CifDet decode)");
        if ((e.has_src || e.swap_mask) && e.n_fields > kMaxTableFields)
            return fail(PP_ESHAPE, at + ": src_field / swap_ends hold at most 64 fields");
        if (e.swap_mask && e.layout != 1)
            return fail(PP_EINVAL, at + ": swap_ends needs the CAF layout");
        if (e.out_field0 < 0 || (int64_t)e.out_field0 + e.n_fields > e.out_fields)
            return fail(PP_ESHAPE, at + ": fields out_field0.. do not fit in out_fields");
        if (e.has_src)
            for (int f = 0; f < e.n_fields; f++)
                if (e.src_field[f] >= e.n_fields)
                    return fail(PP_EINVAL, at + ": src_field entry outside [0, n_fields)");
        const int64_t n_out = c.n_out[e.layout];
        if ((int64_t)e.H * e.W > INT32_MAX || (int64_t)e.out_fields * n_out > INT32_MAX ||
            (int64_t)n_img * e.out_fields * n_out > INT32_MAX)
            return fail(PP_ESHAPE, at + ": bad shape (a product beyond int32)");
        if ((uintptr_t)e.d_container & 3u) return fail(PP_EINVAL, at + ": misaligned buffer");
        ex = ex || e.mirror || e.has_src || e.swap_mask;
        total += (((int64_t)e.H * e.W + 255) / 256) * e.n_fields;
        if (total > INT32_MAX)
            return fail(PP_ESHAPE, name + ": more than 2^31 - 1 workgroups (the launch grid)");
        r.first[m + 1] = (int)total;
    }
    if (n_img > 65535)
        return fail(PP_ESHAPE, name + ": more than 65535 images (the launch grid)");
    // every extent row is named by exactly one entry
    int named[kMaxConvHeads] = {};
    for (int m = 0; m < n_entries; m++) {
        if (heads[m].ext_row < -1 || heads[m].ext_row >= n_rows)
            return fail(PP_EINVAL, name + ": ext_row outside -1 .. n_rows - 1");
        if (heads[m].ext_row >= 0 && named[heads[m].ext_row]++)
            return fail(PP_EINVAL, name + ": an extent row named by two entries");
    }
    for (int row = 0; row < n_rows; row++)
        if (!named[row]) return fail(PP_EINVAL, name + ": an extent row named by no entry");
    // the ranges the entries write are disjoint; entries of one container agree about it
    std::vector<std::pair<int, int>> shared;  // entries m < k of one container
    for (int m = 0; m < n_entries; m++)
        for (int k = m + 1; k < n_entries; k++) {
            const pp_conv_head &p = heads[m], &q = heads[k];
            if (p.d_container == q.d_container) {
                if (p.layout != q.layout || p.H != q.H || p.W != q.W ||
                    p.out_fields != q.out_fields)
                    return fail(PP_EINVAL, name + ": entries of one container differ in its "
                                "layout, size or fields");
                if (p.out_field0 < q.out_field0 + q.n_fields &&
                    q.out_field0 < p.out_field0 + p.n_fields)
                    return fail(PP_EINVAL, name + ": the field ranges of two entries overlap");
                shared.emplace_back(m, k);
                continue;
            }
            const uintptr_t p0 = (uintptr_t)p.d_container, q0 = (uintptr_t)q.d_container;
            // (an empty batch is checked as one image)
            const uint64_t n1 = (uint64_t)std::max(n_img, 1);
            const uint64_t pn = n1 * p.out_fields * c.n_out[p.layout] * p.H * p.W * 4,
                           qn = n1 * q.out_fields * c.n_out[q.layout] * q.H * q.W * 4;
            if (p0 < q0 + qn && q0 < p0 + pn)
                return fail(PP_EINVAL, name + ": the containers of two entries overlap");
        }
    const uintptr_t elem = conv_dtype == PP_DTYPE_F32 ? 4 : 2;
    for (int m = 0; m < n_entries; m++)
        for (int i = 0; i < n_img; i++) {
            const int64_t row = (int64_t)m * n_img + i;
            if (!convs[row]) return fail(PP_EINVAL, name + ": NULL conv pointer");
            if ((uintptr_t)convs[row] & (elem - 1))
                return fail(PP_EINVAL, name + ": misaligned conv pointer");
            const int32_t h = conv_extents[2 * row], w = conv_extents[2 * row + 1];
            if (h <= 0 || w <= 0) return fail(PP_ESHAPE, name + ": conv extent <= 0");
            if (pp_fields_dim(h, quad) > heads[m].H || pp_fields_dim(w, quad) > heads[m].W)
                return fail(PP_ESHAPE, name + ": field extent outside the container");
            // the stride of a dimension of extent 1 says nothing (the channels are never 1)
            if (conv_strides && (conv_strides[2 * row] < 0 || (h > 1 && conv_strides[2 * row + 1] < 0)))
                return fail(PP_EINVAL, name + ": negative conv stride");
        }
    for (const auto &mk : shared)
        for (int i = 0; i < n_img; i++) {
            const int64_t p = (int64_t)mk.first * n_img + i, q = (int64_t)mk.second * n_img + i;
            if (conv_extents[2 * p] != conv_extents[2 * q] ||
                conv_extents[2 * p + 1] != conv_extents[2 * q + 1])
                return fail(PP_ESHAPE, name + ": entries of one container differ in the conv "
                            "extent of an image");
        }
    if (n_img == 0) return PP_OK;
    const HeadsLayout l = heads_layout(n_img, n_entries);
    if (tables_bytes < l.size) return fail(PP_ENOMEM, name + ": table buffer too small");
    if ((uintptr_t)d_tables & 7u) return fail(PP_EINVAL, name + ": misaligned buffer");
    const hipStream_t s = (hipStream_t)stream;
    char *tab = (char *)d_tables;
    // one staging copy when the host tables lie in one block in d_tables' order, one per table
    // otherwise; pageable host tables are consumed before these return (the runtime waits for
    // the copy), pinned ones are read when the stream gets there and must stay valid until then
    const char *base = (const char *)convs;
    const bool joined = conv_strides && (const char *)conv_strides == base + l.strides &&
                        (const char *)heads == base + l.heads &&
                        (const char *)conv_extents == base + l.conv_ext;
    hipError_t err = hipMemcpyAsync(tab, convs, joined ? l.field_ext : l.strides,
                                    hipMemcpyHostToDevice, s);
    if (!joined) {
        if (err == hipSuccess && conv_strides)
            err = hipMemcpyAsync(tab + l.strides, conv_strides, l.heads - l.strides,
                                 hipMemcpyHostToDevice, s);
        if (err == hipSuccess)
            err = hipMemcpyAsync(tab + l.heads, heads, l.conv_ext - l.heads,
                                 hipMemcpyHostToDevice, s);
        if (err == hipSuccess)
            err = hipMemcpyAsync(tab + l.conv_ext, conv_extents, l.field_ext - l.conv_ext,
                                 hipMemcpyHostToDevice, s);
    }
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return fail(PP_EHIP, name + ": staging the tables failed");
    }
    r.conv = (const void *const *)tab;
    r.strides = conv_strides ? (const int64_t *)(tab + l.strides) : nullptr;
    r.conv_ext = (const int32_t *)(tab + l.conv_ext);
    r.field_ext = (int32_t *)(tab + l.field_ext);
    r.n_img = n_img;
    r.n_entries = n_entries;
    r.quad = quad;
    const pp_conv_head *d_heads = (const pp_conv_head *)(tab + l.heads);
    if (conv_dtype == PP_DTYPE_F32)
        launch_ingest_heads<float>(d_heads, r, c, ex, s);
    else if (conv_dtype == PP_DTYPE_F16)
        launch_ingest_heads<__half>(d_heads, r, c, ex, s);
    else
        launch_ingest_heads<Bf16>(d_heads, r, c, ex, s);
    return check_launch(name.c_str());
}

}  // extern "C"

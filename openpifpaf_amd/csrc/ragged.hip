// ragged.hip — the packer of ragged batches (pp_fields_pack_ragged): n images' own
// contiguous float32 fields (n_fields, channels, h_i, w_i), each at its own address, gathered
// into one container (n, n_fields, channels, H, W) that pp_decode_ragged reads beside the
// (n, 2) extent table.
//
// The kernel is a copy: per container element one 4-byte store and, inside the extent, one
// 4-byte load; with S source and D = n * n_fields * channels * H * W container elements it
// moves 4 (S + D) bytes, so at the 6.3 TB/s a float4 copy reaches on this chip a 256-image
// batch of 81x81 containers (D = 430 M for the CIF and CAF heads of the COCO skeleton,
// S about 0.75 D) should take about 0.5 ms.  DESIGN.md §4 has the measured rate.
//
// One workgroup per (image, field, channel) plane: the source pointer and the extent are
// scalar loads.  A container plane is H * W contiguous floats, so the workgroup walks it as
// one row-major run: a head of at most three elements up to the first 16-byte boundary,
// then 16-byte stores (consecutive lanes consecutive quads, whatever W is), then a tail of
// at most three.  Every element is written exactly once, the image's value inside
// [0, h_i) x [0, w_i) and 0 outside, so the container needs no memset.  A quad costs one
// integer division (its first element's row); source rows start at any 4-byte boundary
// (w_i is arbitrary), so loads stay scalar: four per lane, the four instructions together
// reading the wave's 1 KiB run of the source.
//
// pp_fields_pack_ragged_heads packs every head of a multi-scale FieldConfig in one launch
// (ragged_pack_heads_kernel): the workgroups of head 0's planes come first, then head 1's,
// and a workgroup finds its head from a prefix table of workgroup counts held in the kernel
// arguments (at most 2 * PP_MAX_SCALES heads).  Inside a plane it is the same walk
// (pack_plane), so its stores are ragged_pack_kernel's.
#include "pp_common.hpp"

#include <algorithm>

namespace pp {

struct PackArgs {
    const float *const *src;  // (n) device table of the images' field pointers
    const int32_t *ext;       // (n, 2) device table: h_i, w_i
    float *dst;               // (n, planes, H, W)
    int planes;               // n_fields * channels
    int H, W;
};

__global__ __launch_bounds__(256) void ragged_pack_kernel(PackArgs a) {
    const int64_t plane = blockIdx.x;  // image * planes + (field * channels + channel)
    const int img = (int)(plane / a.planes), p = (int)(plane % a.planes);
    const int h = a.ext[2 * img], w = a.ext[2 * img + 1];
    const float *__restrict__ s = a.src[img] + (int64_t)p * h * w;
    const int hw = a.H * a.W;
    float *__restrict__ d = a.dst + plane * hw;
    const int W = a.W;
    auto value = [&](int y, int x) { return (y < h && x < w) ? s[(int64_t)y * w + x] : 0.0f; };
    // elements up to the plane's first 16-byte boundary (d is 4-byte aligned), whole quads
    const int head = min(hw, (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2));
    const int nq = (hw - head) >> 2;
    for (int i = threadIdx.x; i < nq; i += 256) {
        const int e = head + 4 * i;
        int y = e / W, x = e - y * W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = value(y, x);
            if (++x == W) {
                x = 0;
                y++;
            }
        }
        *reinterpret_cast<float4 *>(d + e) = make_float4(v[0], v[1], v[2], v[3]);
    }
    // the head and the tail, one element per lane (at most three each)
    const int tail0 = head + 4 * nq;
    const int t = (int)threadIdx.x;
    const int e = t < head ? t : tail0 + (t - head);
    if (e < hw && (t < head || e >= tail0)) d[e] = value(e / W, e % W);
}

// One container plane d (H * W floats) from the image's plane s (h * w floats), by the 256
// threads of a workgroup.
__device__ __forceinline__ void pack_plane(const float *__restrict__ s, int h, int w,
                                           float *__restrict__ d, int H, int W) {
    const int hw = H * W;
    auto value = [&](int y, int x) { return (y < h && x < w) ? s[(int64_t)y * w + x] : 0.0f; };
    // elements up to the plane's first 16-byte boundary (d is 4-byte aligned), whole quads
    const int head = min(hw, (int)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2));
    const int nq = (hw - head) >> 2;
    for (int i = threadIdx.x; i < nq; i += 256) {
        const int e = head + 4 * i;
        int y = e / W, x = e - y * W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = value(y, x);
            if (++x == W) {
                x = 0;
                y++;
            }
        }
        *reinterpret_cast<float4 *>(d + e) = make_float4(v[0], v[1], v[2], v[3]);
    }
    // the head and the tail, one element per lane (at most three each)
    const int tail0 = head + 4 * nq;
    const int t = (int)threadIdx.x;
    const int e = t < head ? t : tail0 + (t - head);
    if (e < hw && (t < head || e >= tail0)) d[e] = value(e / W, e % W);
}

constexpr int kMaxPackHeads = 2 * PP_MAX_SCALES;

struct PackHeadsArgs {
    const float *const *src;  // (n_heads, n_img) device table of the images' field pointers
    const int32_t *ext;       // (n_heads, n_img, 2) device table: h_i, w_i of each head
    int n_img, n_heads;
    float *dst[kMaxPackHeads];    // head m's container (n_img, planes[m], H[m], W[m])
    int planes[kMaxPackHeads];    // n_fields * channels
    int H[kMaxPackHeads], W[kMaxPackHeads];
    int first[kMaxPackHeads + 1]; // first workgroup of head m: n_img * (planes of the heads before)
};

// One workgroup per (head, image, field, channel) plane, head-major.  The head and its
// entries are picked by selects over constant indices: a dynamic index into the
// kernel-argument struct would make the compiler copy the struct to scratch.
__global__ __launch_bounds__(256) void ragged_pack_heads_kernel(PackHeadsArgs a) {
    const int b = (int)blockIdx.x;
    int m = 0;
#pragma unroll
    for (int c = 1; c < kMaxPackHeads; c++)
        if (c < a.n_heads && b >= a.first[c]) m = c;
    float *dst = a.dst[0];
    int planes = a.planes[0], H = a.H[0], W = a.W[0], first = 0;
#pragma unroll
    for (int c = 1; c < kMaxPackHeads; c++)
        if (c == m) {
            dst = a.dst[c];
            planes = a.planes[c];
            H = a.H[c];
            W = a.W[c];
            first = a.first[c];
        }
    const int plane = b - first;  // image * planes + (field * channels + channel)
    const int img = plane / planes, p = plane % planes;
    const int64_t row = (int64_t)m * a.n_img + img;
    const int h = a.ext[2 * row], w = a.ext[2 * row + 1];
    pack_plane(a.src[row] + (int64_t)p * h * w, h, w, dst + (int64_t)plane * H * W, H, W);
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_ragged_tables_size(int32_t n_img) {
    return n_img > 0 ? (size_t)n_img * (sizeof(void *) + 2 * sizeof(int32_t)) : 0;
}

size_t pp_ragged_extents_offset(int32_t n_img) {
    return n_img > 0 ? (size_t)n_img * sizeof(void *) : 0;
}

int pp_fields_pack_ragged(const float *const *fields, const int32_t *extents, int32_t n_img,
                          int32_t n_fields, int32_t channels, int32_t H, int32_t W,
                          float *d_container, void *d_tables, size_t tables_bytes, void *stream) {
    if (!fields || !extents || !d_container || !d_tables)
        return fail(PP_EINVAL, "pp_fields_pack_ragged: NULL argument");
    if (n_img < 0 || n_fields <= 0 || channels <= 0 || H <= 0 || W <= 0 ||
        (int64_t)n_fields * channels > INT32_MAX || (int64_t)H * W > INT32_MAX ||
        (int64_t)n_img * n_fields * channels > INT32_MAX)
        return fail(PP_ESHAPE, "pp_fields_pack_ragged: bad shape");
    for (int i = 0; i < n_img; i++) {
        if (!fields[i]) return fail(PP_EINVAL, "pp_fields_pack_ragged: NULL field");
        if (extents[2 * i] <= 0 || extents[2 * i] > H || extents[2 * i + 1] <= 0 ||
            extents[2 * i + 1] > W)
            return fail(PP_ESHAPE, "pp_fields_pack_ragged: extent outside the container");
    }
    if (n_img == 0) return PP_OK;
    if (tables_bytes < pp_ragged_tables_size(n_img))
        return fail(PP_ENOMEM, "pp_fields_pack_ragged: table buffer too small");
    if (((uintptr_t)d_tables & 7u) || ((uintptr_t)d_container & 3u))
        return fail(PP_EINVAL, "pp_fields_pack_ragged: misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    char *tab = (char *)d_tables;
    const size_t ext_off = pp_ragged_extents_offset(n_img);
    // pageable host tables are consumed before these return (the runtime waits for the copy);
    // pinned ones are read when the stream gets there and must stay valid until then
    if (hipMemcpyAsync(tab, fields, (size_t)n_img * sizeof(void *), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(tab + ext_off, extents, (size_t)n_img * 2 * sizeof(int32_t),
                       hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PP_EHIP, "pp_fields_pack_ragged: staging the tables failed");
    }
    PackArgs a{};
    a.src = (const float *const *)tab;
    a.ext = (const int32_t *)(tab + ext_off);
    a.dst = d_container;
    a.planes = n_fields * channels;
    a.H = H;
    a.W = W;
    const dim3 grid((unsigned)((int64_t)n_img * a.planes));
    hipLaunchKernelGGL(ragged_pack_kernel, grid, dim3(256), 0, s, a);
    return check_launch("pp_fields_pack_ragged");
}

size_t pp_ragged_heads_tables_size(int32_t n_img, int32_t n_heads) {
    if (n_img <= 0 || n_heads <= 0 || n_heads > kMaxPackHeads) return 0;
    return (size_t)n_heads * n_img * (sizeof(void *) + 2 * sizeof(int32_t));
}

size_t pp_ragged_heads_extents_offset(int32_t n_img, int32_t n_heads) {
    if (n_img <= 0 || n_heads <= 0 || n_heads > kMaxPackHeads) return 0;
    return (size_t)n_heads * n_img * sizeof(void *);
}

int pp_fields_pack_ragged_heads(const float *const *fields, const int32_t *extents, int32_t n_img,
                                int32_t n_heads, const int32_t *planes, const int32_t *sizes,
                                float *const *d_containers, void *d_tables, size_t tables_bytes,
                                void *stream) {
    const char *who = "pp_fields_pack_ragged_heads";
    if (!fields || !extents || !planes || !sizes || !d_containers || !d_tables)
        return fail(PP_EINVAL, std::string(who) + ": NULL argument");
    if (n_img < 0 || n_heads <= 0 || n_heads > kMaxPackHeads)
        return fail(PP_ESHAPE, std::string(who) + ": bad shape (at most 2 * PP_MAX_SCALES heads)");
    PackHeadsArgs a{};
    int64_t total = 0;  // planes of one image over all heads
    for (int m = 0; m < n_heads; m++) {
        const int H = sizes[2 * m], W = sizes[2 * m + 1];
        if (planes[m] <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX)
            return fail(PP_ESHAPE, std::string(who) + ": bad shape");
        if (!d_containers[m]) return fail(PP_EINVAL, std::string(who) + ": NULL container");
        if ((uintptr_t)d_containers[m] & 3u)
            return fail(PP_EINVAL, std::string(who) + ": misaligned buffer");
        a.dst[m] = d_containers[m];
        a.planes[m] = planes[m];
        a.H[m] = H;
        a.W[m] = W;
        total += planes[m];
        if (total * std::max(n_img, 1) > INT32_MAX)
            return fail(PP_ESHAPE, std::string(who) + ": bad shape");
        a.first[m + 1] = (int)(total * n_img);
        for (int i = 0; i < n_img; i++) {
            const int64_t row = (int64_t)m * n_img + i;
            if (!fields[row]) return fail(PP_EINVAL, std::string(who) + ": NULL field");
            if (extents[2 * row] <= 0 || extents[2 * row] > H || extents[2 * row + 1] <= 0 ||
                extents[2 * row + 1] > W)
                return fail(PP_ESHAPE, std::string(who) + ": extent outside the container");
        }
    }
    if (n_img == 0) return PP_OK;
    if (tables_bytes < pp_ragged_heads_tables_size(n_img, n_heads))
        return fail(PP_ENOMEM, std::string(who) + ": table buffer too small");
    if ((uintptr_t)d_tables & 7u) return fail(PP_EINVAL, std::string(who) + ": misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    char *tab = (char *)d_tables;
    const size_t ext_off = pp_ragged_heads_extents_offset(n_img, n_heads);
    const size_t ext_bytes = (size_t)n_heads * n_img * 2 * sizeof(int32_t);
    // one staging copy when the host extent table lies right behind the host pointer table (the
    // layout of d_tables), two otherwise; pageable or pinned as in pp_fields_pack_ragged
    const bool joined = (const char *)extents == (const char *)fields + ext_off;
    hipError_t e = hipMemcpyAsync(tab, fields, joined ? ext_off + ext_bytes : ext_off,
                                  hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !joined)
        e = hipMemcpyAsync(tab + ext_off, extents, ext_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(PP_EHIP, std::string(who) + ": staging the tables failed");
    }
    a.src = (const float *const *)tab;
    a.ext = (const int32_t *)(tab + ext_off);
    a.n_img = n_img;
    a.n_heads = n_heads;
    hipLaunchKernelGGL(ragged_pack_heads_kernel, dim3((unsigned)a.first[n_heads]), dim3(256), 0, s, a);
    return check_launch(who);
}

}  // extern "C"

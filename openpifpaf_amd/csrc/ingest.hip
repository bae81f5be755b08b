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
//
// pp_fields_from_conv_strided reads a view by its strides.  A view whose columns are
// adjacent (NCHW and its slices) keeps that work unit.  A view whose channels are adjacent
// (channels-last and its slices) goes through ingest_interleaved_kernel: a workgroup loads
// the channel runs of 16 conv pixels of one row, lanes along the channels, transposes them
// in LDS and writes with lanes along X, as the planar kernel does.
//
// pp_fields_from_conv_ragged and pp_fields_from_conv_ragged_interleaved write the conv outputs
// of n images of their own sizes into one container, the first from planar views
// (ingest_ragged_kernel), the second from channels-last ones (ingest_ragged_interleaved_kernel).
#include "ingest_common.hpp"

namespace pp {

// element strides of a conv view (pp_fields_from_conv_strided)
struct IngestStrides {
    int64_t img, ch, row, col;
};

template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_kernel(IngestArgs a, IngestFlip t) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)a.H * a.W;
    const int f = blockIdx.y, img = blockIdx.z;
    if (pix >= HW) return;
    const int Y = (int)(pix / a.W), X = (int)(pix % a.W);
    PP_INGEST_PIXEL(a.W)
    const T *src = (const T *)a.conv + (int64_t)img * a.conv_ch * a.h * a.w + (int64_t)y0 * a.w + x0;
    float *dst = a.out + (((int64_t)img * a.out_fields + a.out_field0 + f) * a.n_out) * HW + pix;
    for (int o = 0; o < a.n_out; o++) {
        PP_INGEST_CHANNEL(o)
        const float v = load_f32(src + ch * a.h * a.w);
        dst[(int64_t)o * HW] = ingest_value(op, v, mirror, X, Y);
    }
}

// ingest_kernel on a view with adjacent columns and any image / channel / row strides
template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_strided_kernel(IngestArgs a, IngestFlip t,
                                                             IngestStrides s) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)a.H * a.W;
    const int f = blockIdx.y, img = blockIdx.z;
    if (pix >= HW) return;
    const int Y = (int)(pix / a.W), X = (int)(pix % a.W);
    PP_INGEST_PIXEL(a.W)
    const T *src = (const T *)a.conv + (int64_t)img * s.img + (int64_t)y0 * s.row + x0;
    float *dst = a.out + (((int64_t)img * a.out_fields + a.out_field0 + f) * a.n_out) * HW + pix;
    for (int o = 0; o < a.n_out; o++) {
        PP_INGEST_CHANNEL(o)
        const float v = load_f32(src + ch * s.ch);
        dst[(int64_t)o * HW] = ingest_value(op, v, mirror, X, Y);
    }
}

// ---- n images of their own sizes into one container (pp_fields_from_conv_ragged) ----
//
// The device tables, staged from the caller's host tables: per image the pointer to element
// (0, 0, 0) of its conv view, its channel and row strides (strides NULL: every image dense)
// and its conv extents.  field_ext is written here, the (H_i, W_i) pp_decode_ragged reads.
struct IngestRagged {
    const void *const *conv;  // (n)
    const int64_t *strides;   // (n, 2) channel, row (interleaved kernel: row, column); or NULL
    const int32_t *conv_ext;  // (n, 2) h_i, w_i
    int32_t *field_ext;       // (n, 2) H_i, W_i
};

// ingest_strided_kernel's work unit over the CONTAINER's pixels (a.H, a.W; a.h, a.w and
// a.conv are unused): inside the image's own field the ingested value, mirrored about the
// image's own width, outside it +0, every element of the written fields stored exactly
// once.  The image is blockIdx.z, so its table entries are scalar loads.
template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_ragged_kernel(IngestArgs a, IngestFlip t,
                                                            IngestRagged r) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)a.H * a.W;
    const int f = blockIdx.y, img = blockIdx.z;
    const int h = r.conv_ext[2 * img], w = r.conv_ext[2 * img + 1];
    int Hi = h, Wi = w;
    for (int q = 0; q < a.quad; q++) {  // pp_fields_dim
        Hi = 2 * Hi - 1;
        Wi = 2 * Wi - 1;
    }
    if (blockIdx.x == 0 && f == 0 && threadIdx.x == 0) {
        r.field_ext[2 * img] = Hi;
        r.field_ext[2 * img + 1] = Wi;
    }
    if (pix >= HW) return;
    const int Y = (int)(pix / a.W), X = (int)(pix % a.W);
    float *dst = a.out + (((int64_t)img * a.out_fields + a.out_field0 + f) * a.n_out) * HW + pix;
    if (Y >= Hi || X >= Wi) {
        for (int o = 0; o < a.n_out; o++) dst[(int64_t)o * HW] = 0.0f;
        return;
    }
    const int64_t s_ch = r.strides ? r.strides[2 * img] : (int64_t)h * w;
    const int64_t s_row = r.strides ? r.strides[2 * img + 1] : (int64_t)w;
    PP_INGEST_PIXEL(Wi)
    // a stride whose extent is 1 meets index 0 only (h = 1: y0 = 0)
    const T *src = (const T *)r.conv[img] + (int64_t)y0 * s_row + x0;
    for (int o = 0; o < a.n_out; o++) {
        PP_INGEST_CHANNEL(o)
        const float v = load_f32(src + ch * s_ch);
        dst[(int64_t)o * HW] = ingest_value(op, v, mirror, X, Y);
    }
}

#undef PP_INGEST_PIXEL
#undef PP_INGEST_CHANNEL

// ---- channels adjacent in memory (channels-last and its slices) ----
//
// Tile: kTilePix conv pixels of one conv row of one image, and a chunk of whole pre-dequad
// channels (chunk_base of them = chunk_base * 4^quad conv channels <= kMaxChunkCh).  The
// tile owns the 2^quad output rows and kTilePix * 2^quad output columns of those pixels
// for every (field, output channel) whose conv channels are in the chunk.
//
// LDS image: float32 [pixel][channel of the chunk], pixel pitch `lds_pitch` = 2 (mod 32)
// floats.  On the store side lanes run along X; at quad 1 two adjacent lanes are the two
// channels sub, sub + 1 of one pixel and the next pair is the next pixel, so 32 lanes
// read banks 2k + {0, 1}, k = 0..15: all 32 banks of a ds_read_b32 lane group once.
constexpr int kTilePix = 16;
constexpr int kMaxChunkCh = 512;
constexpr int kLdsFloats = kTilePix * (kMaxChunkCh + 2);  // pitch <= kMaxChunkCh + 2

struct IngestTile {
    int chunk_base;  // pre-dequad channels per chunk (blockIdx.y counts chunks)
    int lds_pitch;   // floats between two pixels of the LDS image
    int tiles_x;     // tiles per conv row (blockIdx.x = row * tiles_x + tile)
};

__device__ __forceinline__ float bits_f32(const float *, uint32_t b) { return __uint_as_float(b); }
__device__ __forceinline__ float bits_f32(const __half *, uint32_t b) {
    return __half2float(__ushort_as_half((unsigned short)b));
}
__device__ __forceinline__ float bits_f32(const Bf16 *, uint32_t b) {
    return __uint_as_float(b << 16);
}

// one 16-byte vector of the run -> its 4 or 8 float32 values in the LDS row
__device__ __forceinline__ void spill_vec(const float *tag, uint4 v, float *row) {
    row[0] = bits_f32(tag, v.x);
    row[1] = bits_f32(tag, v.y);
    row[2] = bits_f32(tag, v.z);
    row[3] = bits_f32(tag, v.w);
}
template <typename T>
__device__ __forceinline__ void spill_vec(const T *tag, uint4 v, float *row) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    for (int j = 0; j < 4; j++) {
        row[2 * j] = bits_f32(tag, w[j] & 0xffffu);
        row[2 * j + 1] = bits_f32(tag, w[j] >> 16);
    }
}

// The load phase of the two interleaved kernels, as text for the reason PP_INGEST_PIXEL is
// (the instances of ingest_interleaved_kernel compile to the code they had with these lines
// written out).  One wave per pixel, lanes along its channel run; 16-byte loads between the
// run's first and last 16-byte boundary, single elements before and after (a slice at an odd
// channel offset is aligned to its element only).  All of a wave's loads are issued before its
// first LDS write, so that they are in flight together: kPix pixels, each at most kIter
// vectors and two elements a lane.  RUN is the address of conv channel 0 of the chunk at
// pixel p of the tile; T, kVec, lane, wave, n (conv channels of the chunk), n_pix (pixels of
// the tile to load: none past it is touched), g and lds are the kernel's.
#define PP_INGEST_TILE_LOAD(RUN)                                                              \
    constexpr int kPix = kTilePix / 4, kIter = kMaxChunkCh / kVec / 64;                       \
    const T *run[kPix];                                                                       \
    int head[kPix], n_vec[kPix];                                                              \
    uint4 vec[kPix][kIter];                                                                   \
    float first[kPix], last[kPix];                                                            \
    _Pragma("unroll") for (int i = 0; i < kPix; i++) {                                        \
        const int p = wave + 4 * i;                                                           \
        n_vec[i] = head[i] = 0;                                                               \
        if (p >= n_pix) continue;                                                             \
        run[i] = RUN;                                                                         \
        const int to_boundary = (int)((16 - ((uintptr_t)run[i] & 15)) & 15) / (int)sizeof(T); \
        head[i] = min(to_boundary, n);                                                        \
        n_vec[i] = (n - head[i]) / kVec;                                                      \
        if (lane < head[i]) first[i] = load_f32(run[i] + lane);                               \
        _Pragma("unroll") for (int j = 0; j < kIter; j++)                                     \
            if (lane + 64 * j < n_vec[i])                                                     \
                vec[i][j] = *reinterpret_cast<const uint4 *>(run[i] + head[i] +               \
                                                             (lane + 64 * j) * kVec);         \
        const int c = head[i] + n_vec[i] * kVec + lane;                                       \
        if (c < n) last[i] = load_f32(run[i] + c);                                            \
    }                                                                                         \
    _Pragma("unroll") for (int i = 0; i < kPix; i++) {                                        \
        const int p = wave + 4 * i;                                                           \
        if (p >= n_pix) continue;                                                             \
        float *row = lds + p * g.lds_pitch;                                                   \
        if (lane < head[i]) row[lane] = first[i];                                             \
        _Pragma("unroll") for (int j = 0; j < kIter; j++)                                     \
            if (lane + 64 * j < n_vec[i])                                                     \
                spill_vec(run[i], vec[i][j], row + head[i] + (lane + 64 * j) * kVec);         \
        const int c = head[i] + n_vec[i] * kVec + lane;                                       \
        if (c < n) row[c] = last[i];                                                          \
    }

template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_interleaved_kernel(IngestArgs a, IngestFlip t,
                                                                 IngestStrides s, IngestTile g) {
    __shared__ float lds[kLdsFloats];
    constexpr int kVec = 16 / (int)sizeof(T);  // elements per 16-byte load
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.z;
    const int y0 = blockIdx.x / g.tiles_x, x0t = (blockIdx.x % g.tiles_x) * kTilePix;
    const int shift = 2 * a.quad;
    const int cb0 = blockIdx.y * g.chunk_base;  // first pre-dequad channel of the chunk
    const int n_base = (int)(a.conv_ch >> shift);
    const int cb1 = min(cb0 + g.chunk_base, n_base);
    const int n = (cb1 - cb0) << shift;  // conv channels of the chunk
    const int n_pix = min(kTilePix, a.w - x0t);

    // load: one wave per pixel, lanes along its channel run (PP_INGEST_TILE_LOAD above)
    PP_INGEST_TILE_LOAD((const T *)a.conv + (int64_t)img * s.img + (int64_t)y0 * s.row +
                        (int64_t)(x0t + p) * s.col + ((int64_t)cb0 << shift))
    __syncthreads();

    // store: lanes along X, then the tile's output rows, then the fields
    const int64_t HW = (int64_t)a.H * a.W;
    const bool mirror = kEx && t.mirror != 0;
    const int x_bits = 4 + a.quad;  // kTilePix << quad output columns
    static_assert(kTilePix == 16, "x_bits assumes 16 pixels per tile");
    const int n_work = a.n_fields << (x_bits + a.quad);
    for (int e = tid; e < n_work; e += 256) {
        const int xl = e & ((1 << x_bits) - 1);
        const int yr = (e >> x_bits) & ((1 << a.quad) - 1);
        const int f = e >> (x_bits + a.quad);
        const int xs = (x0t << a.quad) + xl;  // source column after the dequads
        const int Y = (y0 << a.quad) + yr;
        if (xs >= a.W || Y >= a.H) continue;  // the crop of the last row / column
        const int X = mirror ? a.W - 1 - xs : xs;
        int fs = f;
        bool swap = false;
        if (kEx) {
            if (t.has_src) fs = t.src_field[f];
            swap = f < kMaxTableFields && ((t.swap_mask >> f) & 1);
        }
        int sub = 0, yy = Y, xx = xs;
        for (int q = 0; q < a.quad; q++) {
            sub = 4 * sub + (2 * (yy & 1) + (xx & 1));
            yy >>= 1;
            xx >>= 1;
        }
        const float *src = lds + (xl >> a.quad) * g.lds_pitch + sub;
        float *dst = a.out + (((int64_t)img * a.out_fields + a.out_field0 + f) * a.n_out) * HW +
                     (int64_t)Y * a.W + X;
        for (int o = 0; o < a.n_out; o++) {
            const int op = a.op[o];
            int comp = a.comp[o];
            if (kEx && swap && (op == 3 || op == 4)) comp ^= 2;
            const int cb = a.grp_off[o] + fs * a.fld_mul[o] + comp;
            if (cb < cb0 || cb >= cb1) continue;  // another chunk's workgroup writes it
            dst[(int64_t)o * HW] = ingest_value(op, src[(cb - cb0) << shift], mirror, X, Y);
        }
    }
}

// ingest_interleaved_kernel's tile over the CONTAINER (pp_fields_from_conv_ragged_interleaved):
// blockIdx.x counts (conv row, 16-pixel tile) of ceil(a.H / 2^quad) rows of g.tiles_x tiles,
// which own every container pixel; r.strides holds each image's ROW and COLUMN strides (NULL:
// dense channels-last), the channel stride is 1.  A tile loads the pixels inside the image's
// conv extent only (one wholly outside loads nothing) and stores, for the output channels of
// its chunk, the ingested value inside the image's own field, mirrored about the image's own
// width, and +0 outside it at the unmirrored position: every element of the written fields
// is stored exactly once.  The image is blockIdx.z, so its table entries are scalar loads.
template <typename T, bool kEx>
__global__ __launch_bounds__(256) void ingest_ragged_interleaved_kernel(IngestArgs a, IngestFlip t,
                                                                        IngestRagged r,
                                                                        IngestTile g) {
    __shared__ float lds[kLdsFloats];
    constexpr int kVec = 16 / (int)sizeof(T);  // elements per 16-byte load
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.z;
    const int h = r.conv_ext[2 * img], w = r.conv_ext[2 * img + 1];
    int Hi = h, Wi = w;
    for (int q = 0; q < a.quad; q++) {  // pp_fields_dim
        Hi = 2 * Hi - 1;
        Wi = 2 * Wi - 1;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        r.field_ext[2 * img] = Hi;
        r.field_ext[2 * img + 1] = Wi;
    }
    const int y0 = blockIdx.x / g.tiles_x, x0t = (blockIdx.x % g.tiles_x) * kTilePix;
    const int shift = 2 * a.quad;
    const int cb0 = blockIdx.y * g.chunk_base;  // first pre-dequad channel of the chunk
    const int n_base = (int)(a.conv_ch >> shift);
    const int cb1 = min(cb0 + g.chunk_base, n_base);
    const int n = (cb1 - cb0) << shift;  // conv channels of the chunk
    const int n_pix = y0 < h ? min(kTilePix, w - x0t) : 0;  // <= 0: the tile is outside the image

    // a stride whose extent is 1 meets index 0 only
    const int64_t s_row = h == 1 ? 0 : r.strides ? r.strides[2 * img] : (int64_t)w * a.conv_ch;
    const int64_t s_col = w == 1 ? 0 : r.strides ? r.strides[2 * img + 1] : a.conv_ch;
    const T *row0 = (const T *)r.conv[img] + (int64_t)y0 * s_row + ((int64_t)cb0 << shift);
    PP_INGEST_TILE_LOAD(row0 + (int64_t)(x0t + p) * s_col)
    __syncthreads();

    // store: lanes along X, then the tile's output rows, then the fields
    const int64_t HW = (int64_t)a.H * a.W;
    const bool mirror = kEx && t.mirror != 0;
    const int x_bits = 4 + a.quad;  // kTilePix << quad output columns
    static_assert(kTilePix == 16, "x_bits assumes 16 pixels per tile");
    const int n_work = a.n_fields << (x_bits + a.quad);
    for (int e = tid; e < n_work; e += 256) {
        const int xl = e & ((1 << x_bits) - 1);
        const int yr = (e >> x_bits) & ((1 << a.quad) - 1);
        const int f = e >> (x_bits + a.quad);
        const int xs = (x0t << a.quad) + xl;  // source column after the dequads
        const int Y = (y0 << a.quad) + yr;
        if (xs >= a.W || Y >= a.H) continue;  // outside the container
        // inside the image's own field (the crop is against it) the conv pixel is in the
        // LDS image: xs < Wi = 2^quad (w - 1) + 1 gives xs >> quad < w, and Y likewise
        const bool inside = xs < Wi && Y < Hi;
        const int X = inside && mirror ? Wi - 1 - xs : xs;
        int fs = f;
        bool swap = false;
        if (kEx) {
            if (t.has_src) fs = t.src_field[f];
            swap = f < kMaxTableFields && ((t.swap_mask >> f) & 1);
        }
        int sub = 0, yy = Y, xx = xs;
        for (int q = 0; q < a.quad; q++) {
            sub = 4 * sub + (2 * (yy & 1) + (xx & 1));
            yy >>= 1;
            xx >>= 1;
        }
        const float *src = lds + (xl >> a.quad) * g.lds_pitch + sub;
        float *dst = a.out + (((int64_t)img * a.out_fields + a.out_field0 + f) * a.n_out) * HW +
                     (int64_t)Y * a.W + X;
        for (int o = 0; o < a.n_out; o++) {
            const int op = a.op[o];
            int comp = a.comp[o];
            if (kEx && swap && (op == 3 || op == 4)) comp ^= 2;
            const int cb = a.grp_off[o] + fs * a.fld_mul[o] + comp;
            if (cb < cb0 || cb >= cb1) continue;  // another chunk's workgroup writes it, zeros too
            dst[(int64_t)o * HW] =
                inside ? ingest_value(op, src[(cb - cb0) << shift], mirror, X, Y) : 0.0f;
        }
    }
}

#undef PP_INGEST_TILE_LOAD

enum Route { kDense, kPlanar, kInterleaved };

template <typename T>
static void launch_ingest(Route route, const IngestArgs &a, const IngestFlip &t,
                          const IngestStrides &s, const IngestTile &g, int n_chunks, bool ex,
                          hipStream_t stream) {
    const int64_t HW = (int64_t)a.H * a.W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)a.n_fields, (unsigned)a.n_img);
    const dim3 tiles((unsigned)(a.h * g.tiles_x), (unsigned)n_chunks, (unsigned)a.n_img);
    if (route == kDense && ex)
        hipLaunchKernelGGL((ingest_kernel<T, true>), grid, dim3(256), 0, stream, a, t);
    else if (route == kDense)
        hipLaunchKernelGGL((ingest_kernel<T, false>), grid, dim3(256), 0, stream, a, t);
    else if (route == kPlanar && ex)
        hipLaunchKernelGGL((ingest_strided_kernel<T, true>), grid, dim3(256), 0, stream, a, t, s);
    else if (route == kPlanar)
        hipLaunchKernelGGL((ingest_strided_kernel<T, false>), grid, dim3(256), 0, stream, a, t, s);
    else if (ex)
        hipLaunchKernelGGL((ingest_interleaved_kernel<T, true>), tiles, dim3(256), 0, stream, a,
                           t, s, g);
    else
        hipLaunchKernelGGL((ingest_interleaved_kernel<T, false>), tiles, dim3(256), 0, stream, a,
                           t, s, g);
}

template <typename T>
static void launch_ingest_ragged(const IngestArgs &a, const IngestFlip &t, const IngestRagged &r,
                                 bool ex, hipStream_t stream) {
    const int64_t HW = (int64_t)a.H * a.W;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)a.n_fields, (unsigned)a.n_img);
    if (ex)
        hipLaunchKernelGGL((ingest_ragged_kernel<T, true>), grid, dim3(256), 0, stream, a, t, r);
    else
        hipLaunchKernelGGL((ingest_ragged_kernel<T, false>), grid, dim3(256), 0, stream, a, t, r);
}

template <typename T>
static void launch_ingest_ragged_interleaved(const IngestArgs &a, const IngestFlip &t,
                                             const IngestRagged &r, const IngestTile &g,
                                             int n_chunks, bool ex, hipStream_t stream) {
    const int rows = (a.H + (1 << a.quad) - 1) >> a.quad;
    const dim3 tiles((unsigned)(rows * g.tiles_x), (unsigned)n_chunks, (unsigned)a.n_img);
    if (ex)
        hipLaunchKernelGGL((ingest_ragged_interleaved_kernel<T, true>), tiles, dim3(256), 0,
                           stream, a, t, r, g);
    else
        hipLaunchKernelGGL((ingest_ragged_interleaved_kernel<T, false>), tiles, dim3(256), 0,
                           stream, a, t, r, g);
}

}  // namespace pp

using namespace pp;

extern "C" {

int64_t pp_fields_dim(int64_t n, int32_t quad) {
    for (int q = 0; q < quad; q++) n = 2 * n - 1;  // PixelShuffle(2) then [:-1]
    return n;
}

}  // extern "C"

// ingest_common.hpp
int pp::ingest_setup(const std::string &name, int32_t conv_dtype, int32_t n_fields,
                     int32_t layout, int32_t quad, int32_t mirror, const int32_t *src_field,
                     const uint8_t *swap_ends, int32_t out_fields, int32_t out_field0,
                     IngestArgs &a, IngestFlip &t) {
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
    a.n_fields = n_fields;
    a.quad = quad;
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
    return PP_OK;
}

extern "C" {

// conv_strides NULL: the dense (n_img, channels, h, w) tensor of the two older symbols
static int fields_from_conv(const char *who, const void *d_conv, int32_t conv_dtype,
                            const int64_t *conv_strides, int32_t n_img, int32_t n_fields, int32_t layout, int32_t h,
                            int32_t w, int32_t quad, int32_t mirror, const int32_t *src_field,
                            const uint8_t *swap_ends, float *d_out, int32_t out_fields,
                            int32_t out_field0, void *stream) {
    const std::string name(who);
    if (!d_conv || !d_out) return fail(PP_EINVAL, name + ": NULL argument");
    if (n_img < 0 || n_fields <= 0 || h <= 0 || w <= 0 || quad < 0 || quad > 4)
        return fail(PP_ESHAPE, name + ": bad shape");
    IngestArgs a{};
    IngestFlip t{};
    if (const int rc = ingest_setup(name, conv_dtype, n_fields, layout, quad, mirror, src_field,
                                    swap_ends, out_fields, out_field0, a, t))
        return rc;
    a.conv = d_conv;
    a.out = d_out;
    a.n_img = n_img;
    a.h = h;
    a.w = w;
    a.H = (int)pp_fields_dim(h, quad);
    a.W = (int)pp_fields_dim(w, quad);
    // the plain f32 ingest keeps its own instantiation without the table reads
    const bool ex = t.mirror || t.has_src || t.swap_mask;
    Route route = kDense;
    IngestStrides s{};
    IngestTile g{};
    int n_chunks = 1;
    if (conv_strides) {
        // the stride of a dimension of extent 1 says nothing (torch reports any value)
        const int64_t extent[4] = {n_img, a.conv_ch, h, w};
        int64_t st[4];
        for (int d = 0; d < 4; d++) {
            st[d] = extent[d] > 1 ? conv_strides[d] : 0;
            if (st[d] < 0) return fail(PP_EINVAL, name + ": negative conv stride");
        }
        s = IngestStrides{st[0], st[1], st[2], st[3]};
        if (s.ch == 1) {
            route = kInterleaved;
            // chunks of whole pre-dequad channels, as even as the LDS image allows
            const int n_base = (int)(a.conv_ch >> (2 * quad));
            const int most = kMaxChunkCh >> (2 * quad);  // >= 2: quad <= 4
            n_chunks = (n_base + most - 1) / most;
            g.tiles_x = (w + kTilePix - 1) / kTilePix;
            if (n_chunks > 65535 || (int64_t)h * g.tiles_x > INT32_MAX)
                return fail(PP_ESHAPE, name + ": conv too large for the interleaved grid");
            g.chunk_base = (n_base + n_chunks - 1) / n_chunks;
            const int ch = g.chunk_base << (2 * quad);
            g.lds_pitch = ch + ((2 - ch) & 31);
        } else if (w == 1 || s.col == 1) {
            // a dense NCHW tensor is what ingest_kernel reads without the stride arguments
            const bool dense = (h == 1 || s.row == w) &&
                               s.ch == (a.conv_ch > 1 ? (int64_t)h * w : 0) &&
                               (n_img <= 1 || s.img == a.conv_ch * h * w);
            route = dense ? kDense : kPlanar;
        } else {
            return fail(PP_EINVAL, name + ": neither the channel stride (" + std::to_string(s.ch) +
                        ") nor the column stride (" + std::to_string(s.col) + ") is 1");
        }
    }
    if (n_img == 0) return PP_OK;
    const hipStream_t hs = (hipStream_t)stream;
    if (conv_dtype == PP_DTYPE_F32)
        launch_ingest<float>(route, a, t, s, g, n_chunks, ex, hs);
    else if (conv_dtype == PP_DTYPE_F16)
        launch_ingest<__half>(route, a, t, s, g, n_chunks, ex, hs);
    else
        launch_ingest<Bf16>(route, a, t, s, g, n_chunks, ex, hs);
    return check_launch(who);
}

int pp_fields_from_conv_ex(const void *d_conv, int32_t conv_dtype, int32_t n_img,
                           int32_t n_fields, int32_t layout, int32_t h, int32_t w, int32_t quad,
                           int32_t mirror, const int32_t *src_field, const uint8_t *swap_ends,
                           float *d_out, int32_t out_fields, int32_t out_field0, void *stream) {
    return fields_from_conv("pp_fields_from_conv_ex", d_conv, conv_dtype, nullptr, n_img, n_fields,
                            layout, h, w, quad, mirror, src_field, swap_ends, d_out, out_fields,
                            out_field0, stream);
}

int pp_fields_from_conv_strided(const void *d_conv, int32_t conv_dtype,
                                const int64_t *conv_strides, int32_t n_img, int32_t n_fields,
                                int32_t layout, int32_t h, int32_t w, int32_t quad,
                                int32_t mirror, const int32_t *src_field,
                                const uint8_t *swap_ends, float *d_out, int32_t out_fields,
                                int32_t out_field0, void *stream) {
    if (!conv_strides) return fail(PP_EINVAL, "pp_fields_from_conv_strided: NULL argument");
    return fields_from_conv("pp_fields_from_conv_strided", d_conv, conv_dtype, conv_strides,
                            n_img, n_fields, layout, h, w, quad, mirror, src_field, swap_ends,
                            d_out, out_fields, out_field0, stream);
}

int pp_fields_from_conv(const float *d_conv, int32_t n_img, int32_t n_fields, int32_t layout,
                        int32_t h, int32_t w, int32_t quad, float *d_out, void *stream) {
    return fields_from_conv("pp_fields_from_conv", d_conv, PP_DTYPE_F32, nullptr, n_img, n_fields,
                            layout, h, w, quad, 0, nullptr, nullptr, d_out, n_fields, 0, stream);
}

// d_tables: the pointers (8 n bytes), the strides (16 n), the conv extents (8 n) and the field
// extents (8 n) the kernel writes
size_t pp_ragged_conv_tables_size(int32_t n_img) {
    return n_img > 0 ? (size_t)n_img * (sizeof(void *) + 2 * sizeof(int64_t) + 4 * sizeof(int32_t))
                     : 0;
}

size_t pp_ragged_conv_extents_offset(int32_t n_img) {
    return n_img > 0 ? (size_t)n_img * (sizeof(void *) + 2 * sizeof(int64_t) + 2 * sizeof(int32_t))
                     : 0;
}

// The two ragged symbols: conv_strides holds (channel, row) with column stride 1 for the planar
// one, (row, column) with channel stride 1 for the interleaved one.
static int fields_from_conv_ragged(const char *who, bool interleaved, const void *const *convs,
                                   int32_t conv_dtype, const int32_t *conv_extents,
                                   const int64_t *conv_strides, int32_t n_img, int32_t n_fields,
                                   int32_t layout, int32_t quad, int32_t mirror,
                                   const int32_t *src_field, const uint8_t *swap_ends, int32_t H,
                                   int32_t W, float *d_container, int32_t out_fields,
                                   int32_t out_field0, void *d_tables, size_t tables_bytes,
                                   void *stream) {
    const std::string name(who);
    if (!convs || !conv_extents || !d_container || !d_tables)
        return fail(PP_EINVAL, name + ": NULL argument");
    if (n_img < 0 || n_fields <= 0 || H <= 0 || W <= 0 || quad < 0 || quad > 4)
        return fail(PP_ESHAPE, name + ": bad shape");
    IngestArgs a{};
    IngestFlip t{};
    if (const int rc = ingest_setup(name, conv_dtype, n_fields, layout, quad, mirror, src_field,
                                    swap_ends, out_fields, out_field0, a, t))
        return rc;
    if ((int64_t)H * W > INT32_MAX || (int64_t)out_fields * a.n_out > INT32_MAX ||
        (int64_t)n_img * out_fields * a.n_out > INT32_MAX)
        return fail(PP_ESHAPE, name + ": bad shape (a product beyond int32)");
    if (n_img > 65535 || n_fields > 65535)
        return fail(PP_ESHAPE, name + ": more than 65535 images or fields (the launch grid)");
    IngestTile g{};
    int n_chunks = 1;
    if (interleaved) {
        // chunks of whole pre-dequad channels, as even as the LDS image allows; the tiles
        // cover the container (rows * tiles_x <= H * W, which is inside int32)
        const int n_base = (int)(a.conv_ch >> (2 * quad));
        const int most = kMaxChunkCh >> (2 * quad);  // >= 2: quad <= 4
        n_chunks = (n_base + most - 1) / most;
        if (n_chunks > 65535)
            return fail(PP_ESHAPE, name + ": more than 65535 channel chunks (the launch grid)");
        g.tiles_x = (((W + (1 << quad) - 1) >> quad) + kTilePix - 1) / kTilePix;
        g.chunk_base = (n_base + n_chunks - 1) / n_chunks;
        const int ch = g.chunk_base << (2 * quad);
        g.lds_pitch = ch + ((2 - ch) & 31);
    }
    const uintptr_t elem = conv_dtype == PP_DTYPE_F32 ? 4 : 2;
    for (int i = 0; i < n_img; i++) {
        if (!convs[i]) return fail(PP_EINVAL, name + ": NULL conv pointer");
        if ((uintptr_t)convs[i] & (elem - 1))
            return fail(PP_EINVAL, name + ": misaligned conv pointer");
        const int32_t h = conv_extents[2 * i], w = conv_extents[2 * i + 1];
        if (h <= 0 || w <= 0) return fail(PP_ESHAPE, name + ": conv extent <= 0");
        if (pp_fields_dim(h, quad) > H || pp_fields_dim(w, quad) > W)
            return fail(PP_ESHAPE, name + ": field extent outside the container");
        // the stride of a dimension of extent 1 says nothing (the channels are never 1)
        if (conv_strides && !interleaved &&
            (conv_strides[2 * i] < 0 || (h > 1 && conv_strides[2 * i + 1] < 0)))
            return fail(PP_EINVAL, name + ": negative conv stride");
        if (conv_strides && interleaved &&
            ((h > 1 && conv_strides[2 * i] < 0) || (w > 1 && conv_strides[2 * i + 1] < 0)))
            return fail(PP_EINVAL, name + ": negative conv stride");
    }
    if (n_img == 0) return PP_OK;
    if (tables_bytes < pp_ragged_conv_tables_size(n_img))
        return fail(PP_ENOMEM, name + ": table buffer too small");
    if (((uintptr_t)d_tables & 7u) || ((uintptr_t)d_container & 3u))
        return fail(PP_EINVAL, name + ": misaligned buffer");
    const hipStream_t s = (hipStream_t)stream;
    char *tab = (char *)d_tables;
    const size_t n = (size_t)n_img, str_off = n * sizeof(void *),
                 cext_off = str_off + n * 2 * sizeof(int64_t);
    // straight from the caller's tables: pageable ones are consumed before these return (the
    // runtime waits for the copy); pinned ones are read when the stream gets there and must
    // stay valid until then
    bool ok = hipMemcpyAsync(tab, convs, n * sizeof(void *), hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok && conv_strides)
        ok = hipMemcpyAsync(tab + str_off, conv_strides, n * 2 * sizeof(int64_t),
                            hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(tab + cext_off, conv_extents, n * 2 * sizeof(int32_t),
                              hipMemcpyHostToDevice, s) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return fail(PP_EHIP, name + ": staging the tables failed");
    }
    a.out = d_container;
    a.n_img = n_img;
    a.H = H;
    a.W = W;
    IngestRagged r{};
    r.conv = (const void *const *)tab;
    r.strides = conv_strides ? (const int64_t *)(tab + str_off) : nullptr;
    r.conv_ext = (const int32_t *)(tab + cext_off);
    r.field_ext = (int32_t *)(tab + pp_ragged_conv_extents_offset(n_img));
    const bool ex = t.mirror || t.has_src || t.swap_mask;
    if (interleaved && conv_dtype == PP_DTYPE_F32)
        launch_ingest_ragged_interleaved<float>(a, t, r, g, n_chunks, ex, s);
    else if (interleaved && conv_dtype == PP_DTYPE_F16)
        launch_ingest_ragged_interleaved<__half>(a, t, r, g, n_chunks, ex, s);
    else if (interleaved)
        launch_ingest_ragged_interleaved<Bf16>(a, t, r, g, n_chunks, ex, s);
    else if (conv_dtype == PP_DTYPE_F32)
        launch_ingest_ragged<float>(a, t, r, ex, s);
    else if (conv_dtype == PP_DTYPE_F16)
        launch_ingest_ragged<__half>(a, t, r, ex, s);
    else
        launch_ingest_ragged<Bf16>(a, t, r, ex, s);
    return check_launch(who);
}

int pp_fields_from_conv_ragged(const void *const *convs, int32_t conv_dtype,
                               const int32_t *conv_extents, const int64_t *conv_strides,
                               int32_t n_img, int32_t n_fields, int32_t layout, int32_t quad,
                               int32_t mirror, const int32_t *src_field, const uint8_t *swap_ends,
                               int32_t H, int32_t W, float *d_container, int32_t out_fields,
                               int32_t out_field0, void *d_tables, size_t tables_bytes,
                               void *stream) {
    return fields_from_conv_ragged("pp_fields_from_conv_ragged", false, convs, conv_dtype,
                                   conv_extents, conv_strides, n_img, n_fields, layout, quad,
                                   mirror, src_field, swap_ends, H, W, d_container, out_fields,
                                   out_field0, d_tables, tables_bytes, stream);
}

int pp_fields_from_conv_ragged_interleaved(
    const void *const *convs, int32_t conv_dtype, const int32_t *conv_extents,
    const int64_t *conv_strides, int32_t n_img, int32_t n_fields, int32_t layout, int32_t quad,
    int32_t mirror, const int32_t *src_field, const uint8_t *swap_ends, int32_t H, int32_t W,
    float *d_container, int32_t out_fields, int32_t out_field0, void *d_tables,
    size_t tables_bytes, void *stream) {
    return fields_from_conv_ragged("pp_fields_from_conv_ragged_interleaved", true, convs,
                                   conv_dtype, conv_extents, conv_strides, n_img, n_fields, layout,
                                   quad, mirror, src_field, swap_ends, H, W, d_container,
                                   out_fields, out_field0, d_tables, tables_bytes, stream);
}

}  // extern "C"

// pack.hip — record packing: the per-image record slots of a decode, image after image, into
// one caller buffer (Generator.batch's list of per-image Annotation lists, generator.py:96-97,
// flattened); the destination may be mapped pinned host memory (zero-copy).
//   pack_records_kernel / pp_pack_records   whole pp_ann records
//   pack_det_records_kernel / pp_pack_det_records   whole pp_det records, counts and status
//   pack_compact_kernel / pp_pack_compact   compact records (PackLayout / pack_layout,
//                                           packed_word; pp_packed_record_size gives the size)
// One workgroup per image in all three.
#include "pack_common.hpp"

namespace pp {

// One workgroup per image: the image's offset is the sum of the earlier counts (read by
// the whole workgroup, n is small), then its records are copied as 8-byte words (a record
// is 1544 = 8 * 193 bytes).  Records at packed index >= out_cap are not written.
__global__ __launch_bounds__(256) void pack_records_kernel(const pp_ann *__restrict__ anns,
                                                           const int *__restrict__ counts, int n,
                                                           int cap, pp_ann *out, int64_t out_cap,
                                                           int *out_counts) {
    __shared__ int s_off;
    const int img = blockIdx.x;
    const int64_t off = packed_offset(counts, img, s_off);
    const int cnt = counts[img];
    if (threadIdx.x == 0) out_counts[img] = cnt;
    const int64_t fit = min((int64_t)cnt, max((int64_t)0, out_cap - off));
    constexpr int kWords = sizeof(pp_ann) / 8;
    static_assert(sizeof(pp_ann) % 8 == 0, "pp_ann is copied in 8-byte words");
    const uint64_t *src = reinterpret_cast<const uint64_t *>(anns + (int64_t)img * cap);
    store_words(reinterpret_cast<uint64_t *>(out + off), src, fit * kWords, (int)threadIdx.x, 256);
}

// The same for the detection decoder's records, with the decode's status words beside the
// counts: a pp_det is two 16-byte chunks, thread t copies chunks t, t + 256, ... of the
// image's records (16-byte loads and stores; rows and destination are 16-byte aligned, so
// every chunk is).  Reads stop at the row's capacity whatever the count says.
__global__ __launch_bounds__(256) void pack_det_records_kernel(
    const pp_det *__restrict__ dets, const int *__restrict__ counts,
    const int *__restrict__ status, int n, int cap, pp_det *out, int64_t out_cap, int *out_counts,
    int *out_status) {
    __shared__ int s_off;
    const int img = blockIdx.x;
    const int64_t off = packed_offset(counts, img, s_off);
    const int cnt = counts[img];
    if (threadIdx.x == 0) {
        out_counts[img] = cnt;
        if (out_status) out_status[img] = status[img];
    }
    const int64_t fit = min((int64_t)min(cnt, cap), max((int64_t)0, out_cap - off));
    static_assert(sizeof(pp_det) == 32, "pp_det is copied as two 16-byte chunks");
    const uint4 *src = reinterpret_cast<const uint4 *>(dets + (int64_t)img * cap);
    uint4 *dst = reinterpret_cast<uint4 *>(out + off);
    for (int64_t c = threadIdx.x; c < 2 * fit; c += 256) dst[c] = src[c];
}

// -------------------------------------------------------------------------------------
// compact records (pp_pack_compact): a pp_ann cut to K keypoints and the skeleton's frontier
// bound, for the PCIe hand-over and the multi-GPU gather.  decoding_order keeps the pairs,
// the two v of each entry and, once per joint, the x / y the joint had when it entered the
// order (set once by _grow, cifcaf.py:300-306; nms.Keypoints may zero the data row later,
// nms.py:22, so the data rows cannot stand in for them).  The kernel checks that every
// entry's coordinates equal its joints' recorded x / y bit for bit; a record where that does
// not hold, or whose orders exceed the compact bounds, is flagged PP_PACK_REFETCH for a
// full-record fetch.
// -------------------------------------------------------------------------------------
struct PackLayout {
    int K, F, dec, front;
    int off_data, off_scales, off_pairs, off_decv, off_decxy, off_front, size;
};

__host__ __device__ inline PackLayout pack_layout(int K, int C, uint32_t flags) {
    PackLayout L{};
    L.K = K;
    L.F = min(PP_MAX_FRONTIER, 4 * C);  // frontier_order: <= 2C edges per _grow, grow + complete
    L.dec = (flags & PP_PACK_DECODING) != 0;
    L.front = (flags & PP_PACK_FRONTIER) != 0;
    int o = 16;
    L.off_data = o;
    o += 12 * K;
    L.off_scales = o;
    o += 4 * K;
    L.off_pairs = o;
    if (L.dec) o += (2 * K + 3) / 4 * 4;
    L.off_decv = o;
    if (L.dec) o += 8 * K;
    L.off_decxy = o;
    if (L.dec) o += 8 * K;
    L.off_front = o;
    if (L.front) o += (2 * L.F + 3) / 4 * 4;
    L.size = (o + 15) / 16 * 16;
    return L;
}

// 4-byte word i of the compact record of `a` (w3 = the count word; jxy = the wave's LDS
// copy of the recorded joint coordinates)
__device__ __forceinline__ uint32_t packed_word(const pp_ann &a, const PackLayout &L, int i,
                                                uint32_t w3, const float *jxy) {
    const uint32_t *s = reinterpret_cast<const uint32_t *>(&a);
    const int b = 4 * i;
    if (i < 2) return s[offsetof(pp_ann, score) / 4 + i];
    if (i == 2) return (uint32_t)a.image;
    if (i == 3) return w3;
    if (b < L.off_scales) return s[offsetof(pp_ann, data) / 4 + (b - L.off_data) / 4];
    if (b < L.off_pairs) return s[offsetof(pp_ann, joint_scales) / 4 + (b - L.off_scales) / 4];
    const int nd = min(a.n_decoding, L.K), nf = min(a.n_frontier, L.F);
    if (b < L.off_decv) {  // pairs bytes [q, q + 4) of the first nd entries
        const int q = b - L.off_pairs;
        uint32_t w = s[offsetof(pp_ann, decoding_pairs) / 4 + q / 4];
        const int keep = min(max(2 * nd - q, 0), 4);
        return keep == 4 ? w : (w & ((1u << (8 * keep)) - 1u));
    }
    if (b < L.off_decxy) {  // (v of the source joint, v of the target joint) per entry
        const int t = (b - L.off_decv) / 4, e = t >> 1;
        return e < nd ? __float_as_uint(a.decoding_xyv[e][2 + 3 * (t & 1)]) : 0u;
    }
    if (b < L.off_front) {  // (x, y) per joint as it entered decoding_order
        return __float_as_uint(jxy[(b - L.off_decxy) / 4]);
    }
    if (b < L.off_front + (2 * L.F + 3) / 4 * 4 && L.front) {
        const int q = b - L.off_front;
        uint32_t w = s[offsetof(pp_ann, frontier_pairs) / 4 + q / 4];
        const int keep = min(max(2 * nf - q, 0), 4);
        return keep == 4 ? w : (w & ((1u << (8 * keep)) - 1u));
    }
    return 0u;
}

// One workgroup per image (offset = the sum of the earlier counts), one wave per record,
// lane = one 16-byte chunk of the compact record (16-byte stores; the destination is
// usually mapped host memory across PCIe).
__global__ __launch_bounds__(256) void pack_compact_kernel(const pp_ann *__restrict__ anns,
                                                           const int *__restrict__ counts, int n,
                                                           int cap, PackLayout L, char *out,
                                                           int64_t out_cap, int *out_counts,
                                                           int *out_flags) {
    __shared__ int s_off, s_bad;
    __shared__ float s_jxy[4][2 * PP_MAX_KP];
    const int img = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) s_bad = 0;
    const int64_t off = packed_offset(counts, img, s_off);
    const int cnt = counts[img];
    if (threadIdx.x == 0) out_counts[img] = cnt;
    const int fit = (int)min((int64_t)min(cnt, cap), max((int64_t)0, out_cap - off));
    const int chunks = L.size / 16;
    for (int r = wave; r < fit; r += 4) {
        const pp_ann &a = anns[(int64_t)img * cap + r];
        // compact form: lane j records joint j's x / y at its first appearance in
        // decoding_order; every entry must agree with its joints' records
        const int nd = a.n_decoding, nf = a.n_frontier;
        const int ndc = min(max(nd, 0), L.K);
        bool bad = (L.dec && nd > L.K) || (L.front && nf > L.F) || nd < 0 || nf < 0;
        float jx = 0.0f, jy = 0.0f;
        if (L.dec) {
            bool found = false;
            for (int e = 0; e < ndc; e++) {  // wave-uniform walk, nd <= K entries
                const int js = a.decoding_pairs[e][0], jt = a.decoding_pairs[e][1];
                if (!found && (js == lane || jt == lane)) {
                    const int h = js == lane ? 0 : 3;
                    jx = a.decoding_xyv[e][h];
                    jy = a.decoding_xyv[e][h + 1];
                    found = true;
                }
            }
            int js = 0, jt = 0;
            if (lane < ndc) {
                js = a.decoding_pairs[lane][0];
                jt = a.decoding_pairs[lane][1];
                bad |= js >= L.K || jt >= L.K;
            }
            const float sx = __shfl(jx, js), sy = __shfl(jy, js);
            const float tx = __shfl(jx, jt), ty = __shfl(jy, jt);
            if (lane < ndc) {
                const float *x = a.decoding_xyv[lane];
                bad |= __float_as_uint(x[0]) != __float_as_uint(sx) ||
                       __float_as_uint(x[1]) != __float_as_uint(sy) ||
                       __float_as_uint(x[3]) != __float_as_uint(tx) ||
                       __float_as_uint(x[4]) != __float_as_uint(ty);
            }
        }
        bad = __ballot(bad) != 0ull;
        if (bad && lane == 0) s_bad = 1;
        if (lane < L.K) {
            s_jxy[wave][2 * lane] = jx;
            s_jxy[wave][2 * lane + 1] = jy;
        }
        wave_sync();
        const uint32_t w3 = (uint32_t)(L.dec ? min(nd, L.K) : 0) | (bad ? PP_PACK_REFETCH : 0u) |
                            ((uint32_t)(L.front ? min(nf, L.F) : 0) << 16);
        uint4 *dst = reinterpret_cast<uint4 *>(out + (off + r) * (int64_t)L.size);
        for (int c = lane; c < chunks; c += 64) {
            uint4 v;
            v.x = packed_word(a, L, 4 * c, w3, s_jxy[wave]);
            v.y = packed_word(a, L, 4 * c + 1, w3, s_jxy[wave]);
            v.z = packed_word(a, L, 4 * c + 2, w3, s_jxy[wave]);
            v.w = packed_word(a, L, 4 * c + 3, w3, s_jxy[wave]);
            dst[c] = v;
        }
        wave_sync();  // s_jxy is rewritten for the wave's next record
    }
    if (out_flags) {  // one plain store per image: no atomics across PCIe
        __syncthreads();
        if (threadIdx.x == 0) out_flags[img] = s_bad;
    }
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_pack_records(const pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                    int32_t ann_capacity, pp_ann *out, int64_t out_capacity, int32_t *out_counts,
                    void *stream) {
    if (!d_anns || !d_counts || !out || !out_counts)
        return fail(PP_EINVAL, "pp_pack_records: NULL argument");
    if (n_img < 0 || ann_capacity <= 0 || out_capacity < 0)
        return fail(PP_ESHAPE, "pp_pack_records: bad shape");
    if (n_img == 0) return PP_OK;
    void *dst[2] = {out, out_counts};
    if (const int rd = map_destinations("pp_pack_records", dst, 2)) return rd;
    hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)n_img), dim3(256), 0,
                       (hipStream_t)stream, d_anns, d_counts, n_img, ann_capacity,
                       (pp_ann *)dst[0], out_capacity, (int *)dst[1]);
    return check_launch("pp_pack_records");
}

int pp_pack_det_records(const pp_det *d_dets, const int32_t *d_counts, const int32_t *d_status,
                        int32_t n_img, int32_t det_capacity, pp_det *out, int64_t out_capacity,
                        int32_t *out_counts, int32_t *out_status, void *stream) {
    if (!d_dets || !d_counts || !out || !out_counts)
        return fail(PP_EINVAL, "pp_pack_det_records: NULL argument");
    if (!d_status != !out_status)
        return fail(PP_EINVAL, "pp_pack_det_records: d_status and out_status go together");
    if (n_img < 0 || det_capacity <= 0 || out_capacity < 0)
        return fail(PP_ESHAPE, "pp_pack_det_records: bad shape");
    if (reinterpret_cast<uintptr_t>(d_dets) & 15)
        return fail(PP_EINVAL, "pp_pack_det_records: records not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 15)
        return fail(PP_EINVAL, "pp_pack_det_records: destination not 16-byte aligned");
    if (n_img == 0) return PP_OK;
    void *dst[3] = {out, out_counts, out_status};  // out_status is optional
    if (const int rd = map_destinations("pp_pack_det_records", dst, 3)) return rd;
    if (reinterpret_cast<uintptr_t>(dst[0]) & 15)  // the mapped address, should it differ
        return fail(PP_EINVAL, "pp_pack_det_records: destination not 16-byte aligned");
    hipLaunchKernelGGL(pack_det_records_kernel, dim3((unsigned)n_img), dim3(256), 0,
                       (hipStream_t)stream, d_dets, d_counts, d_status, n_img, det_capacity,
                       (pp_det *)dst[0], out_capacity, (int *)dst[1], (int *)dst[2]);
    return check_launch("pp_pack_det_records");
}

int64_t pp_packed_record_size(int32_t K, int32_t C, uint32_t flags) {
    if (K <= 0 || K > PP_MAX_KP || C <= 0 || C > PP_MAX_EDGES) return 0;
    return pack_layout(K, C, flags).size;
}

int pp_pack_compact(const pp_ann *d_anns, const int32_t *d_counts, int32_t n_img,
                    int32_t ann_capacity, int32_t K, int32_t C, uint32_t flags, void *out,
                    int64_t out_capacity, int32_t *out_counts, int32_t *out_flags,
                    void *stream) {
    if (!d_anns || !d_counts || !out || !out_counts)
        return fail(PP_EINVAL, "pp_pack_compact: NULL argument");
    if (n_img < 0 || ann_capacity <= 0 || out_capacity < 0 || K <= 0 || K > PP_MAX_KP || C <= 0 ||
        C > PP_MAX_EDGES)
        return fail(PP_ESHAPE, "pp_pack_compact: bad shape");
    if (flags & ~(uint32_t)(PP_PACK_DECODING | PP_PACK_FRONTIER))
        return fail(PP_EINVAL, "pp_pack_compact: unknown flag");
    if (n_img == 0) return PP_OK;
    void *dst[3] = {out, out_counts, out_flags};  // out_flags is optional
    if (const int rd = map_destinations("pp_pack_compact", dst, 3)) return rd;
    if (reinterpret_cast<uintptr_t>(dst[0]) & 15)
        return fail(PP_EINVAL, "pp_pack_compact: destination not 16-byte aligned");
    hipLaunchKernelGGL(pack_compact_kernel, dim3((unsigned)n_img), dim3(256), 0,
                       (hipStream_t)stream, d_anns, d_counts, n_img, ann_capacity,
                       pack_layout(K, C, flags), (char *)dst[0], out_capacity, (int *)dst[1],
                       (int *)dst[2]);
    return check_launch("pp_pack_compact");
}

}  // extern "C"

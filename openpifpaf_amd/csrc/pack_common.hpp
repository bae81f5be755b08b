// pack_common.hpp — what the record hand-over kernels (pack.hip, coco.hip) share: records of
// one workgroup per image, packed image after image into a caller block that is usually
// mapped pinned host memory across PCIe.
#pragma once

#include "pp_common.hpp"

namespace pp {

// Host: the n destinations as the device sees them: device memory as is, pinned host memory
// (hipHostMalloc / registered) through its mapped device address.  A NULL entry (an
// optional destination) is skipped.
inline int map_destinations(const char *who, void **dst, int n) {
    for (int i = 0; i < n; i++) {
        if (!dst[i]) continue;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dst[i]) != hipSuccess || !at.devicePointer ||
            (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeHost)) {
            (void)hipGetLastError();
            return fail(PP_EINVAL, std::string(who) + ": destination is neither device memory "
                                                      "nor pinned host memory");
        }
        dst[i] = at.devicePointer;
    }
    return PP_OK;
}

// The packed index of image `img`'s first record: the sum of the earlier images' counts,
// read by the whole workgroup of 256 (n is small).  Two barriers; the first also publishes
// whatever LDS the caller wrote before the call.
__device__ __forceinline__ int64_t packed_offset(const int *counts, int img, int &s_off) {
    if (threadIdx.x == 0) s_off = 0;
    __syncthreads();
    int part = 0;
    for (int j = threadIdx.x; j < img; j += 256) part += counts[j];
    if (part) atomicAdd(&s_off, part);
    __syncthreads();
    return s_off;
}

// `words` 8-byte words from src to dst (8-byte aligned) by the threads first, first + stride,
// ... (0..255 by 256 for a workgroup, the lane by 64 for a wave) as 16-byte stores (the
// destination is usually across PCIe, where wide writes pay): one leading 8-byte word when
// dst is 8 mod 16, then word pairs, each assembled from two 8-byte loads, then a trailing
// word
template <typename I>
__device__ __forceinline__ void store_words(uint64_t *dst, const uint64_t *src, I words, int first,
                                            int stride) {
    const I lead = (reinterpret_cast<uintptr_t>(dst) & 8) ? min(words, (I)1) : 0;
    const I pairs = (words - lead) >> 1;
    if (first == 0 && lead) dst[0] = src[0];
    typedef uint64_t v2u __attribute__((ext_vector_type(2)));
    v2u *dst2 = reinterpret_cast<v2u *>(dst + lead);
    for (I i = first; i < pairs; i += stride) {
        v2u v;
        v.x = src[lead + 2 * i];
        v.y = src[lead + 2 * i + 1];
        dst2[i] = v;
    }
    if (first == 0 && lead + 2 * pairs < words) dst[words - 1] = src[words - 1];
}

}  // namespace pp

// grow_device.hpp — the device helpers that more than one kernel file of the decoder uses
// (the seed loops and force-complete through grow.hpp, nms.hip): readlane and the DPP wave
// reductions, the occupancy grid's geometry, whole-record copies.
#pragma once

#include "grow_args.hpp"

namespace pp {

__device__ __forceinline__ float rl_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int rl_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// Wave reductions on DPP (row-level VALU data movement, no LDS round trip): quad xor 1,
// quad xor 2, row half-mirror, row mirror, then row_bcast15 / row_bcast31 fold the rows
// into lane 63.  Each step pairs lanes holding disjoint lane sets, so any associative,
// commutative merge (sum, min, exact top-2) is correct; lanes outside a step's row mask
// receive `old` (the identity).
constexpr int kDppXor1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;
constexpr int kDppMirror = 0x140;
constexpr int kDppBcast15 = 0x142;
constexpr int kDppBcast31 = 0x143;

template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_i(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWS, 0xF, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_f(float old, float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROWS, 0xF, false));
}

// sum over the wave, uniform result
__device__ __forceinline__ int wave_total(int v) {
    v += dpp_i<kDppXor1, 0xF>(0, v);
    v += dpp_i<kDppXor2, 0xF>(0, v);
    v += dpp_i<kDppHalfMirror, 0xF>(0, v);
    v += dpp_i<kDppMirror, 0xF>(0, v);
    v += dpp_i<kDppBcast15, 0xA>(0, v);
    v += dpp_i<kDppBcast31, 0xC>(0, v);
    return __builtin_amdgcn_readlane(v, 63);
}

// min over the wave (fminf: NaN ignored), uniform result
__device__ __forceinline__ float wave_fmin(float v) {
    v = fminf(v, dpp_f<kDppXor1, 0xF>(INFINITY, v));
    v = fminf(v, dpp_f<kDppXor2, 0xF>(INFINITY, v));
    v = fminf(v, dpp_f<kDppHalfMirror, 0xF>(INFINITY, v));
    v = fminf(v, dpp_f<kDppMirror, 0xF>(INFINITY, v));
    v = fminf(v, dpp_f<kDppBcast15, 0xA>(INFINITY, v));
    v = fminf(v, dpp_f<kDppBcast31, 0xC>(INFINITY, v));
    return rl_f(v, 63);
}

// ---------------------------------------------------------------------------------------
// occupancy (occupancy.py:10-47, decoder/utils.py:61-66)
// ---------------------------------------------------------------------------------------
// u8 planes (f, h, w) stored with a row pitch of round_up(w, 16) bytes, so that no two
// rows (and no two planes) share a 16-byte chunk: marking updates whole chunks.
struct OccGrid {
    uint8_t *p;
    int f, h, w, pitch;
};

__device__ __forceinline__ OccGrid occ_grid(uint8_t *p, int f, int h, int w) {
    return OccGrid{p, f, h, w, (w + 15) & ~15};
}

__device__ __forceinline__ long round_half_even(float x) { return (long)rintf(x); }

// Occupancy.get (occupancy.py:41-47): nonzero at floor((x, y) / reduction), clipped
__device__ __forceinline__ bool occ_get(const OccGrid &o, int f, float x, float y, float red) {
    if (f >= o.f) return true;
    if (o.h <= 0 || o.w <= 0) return false;  // the reference reads out of bounds here
    x = clip_ref(x / red, 0.0f, (float)(o.w - 1));
    y = clip_ref(y / red, 0.0f, (float)(o.h - 1));
    const int xi = (int)x, yi = (int)y;
    return o.p[((int64_t)f * o.h + yi) * o.pitch + xi] != 0;
}

// Occupancy.set box (occupancy.py:31-39 + utils.py:61-66) of joint f; false when empty.
// red = reduction, msr = min_scale / reduction (occ_box below takes them from the config)
__device__ __forceinline__ bool occ_box_r(float red, float msr, const OccGrid &o, int f, float x,
                                          float y, float sigma, int box[4]) {
    if (f >= o.f) return false;
    const long xi = (long)rintf(x / red);  // round(): half to even
    const long yi = (long)rintf(y / red);
    const float sr = sigma / red;
    const long si = (long)rintf((sr > msr) ? sr : msr);  // max(min_scale_reduced, sigma / r)
    const long minx = xi - si > 0 ? xi - si : 0;
    const long miny = yi - si > 0 ? yi - si : 0;
    const long mx = xi + si + 1 < o.w ? xi + si + 1 : o.w;
    const long my = yi + si + 1 < o.h ? yi + si + 1 : o.h;
    long maxx = minx + 1 > mx ? minx + 1 : mx;
    long maxy = miny + 1 > my ? miny + 1 : my;
    if (maxx > o.w) maxx = o.w;  // numpy slice clipping
    if (maxy > o.h) maxy = o.h;
    if (minx >= maxx || miny >= maxy) return false;
    box[0] = (int)minx;
    box[1] = (int)maxx;
    box[2] = (int)miny;
    box[3] = (int)maxy;
    return true;
}

__device__ __forceinline__ float occ_msr(const GrowArgs &g) {
    return (float)((double)g.cfg.occupancy_min_scale / g.cfg.occupancy_reduction);
}

__device__ __forceinline__ bool occ_box(const GrowArgs &g, const OccGrid &o, int f, float x, float y, float sigma,
                        int box[4]) {
    return occ_box_r((float)g.cfg.occupancy_reduction, occ_msr(g), o, f, x, y, sigma, box);
}

// all loads first, then all stores: one round trip (the two records may alias as far as the
// compiler knows, so a plain copy loop waits for every load in turn)
// a record copy in two halves, so that other work overlaps the loads' latency: the loads
// into registers (per lane kAnnWords words), then the stores
constexpr int kAnnWords = (int)((sizeof(pp_ann) / 4 + 63) / 64);
struct AnnRegs {
    uint32_t v[kAnnWords];
};
__device__ __forceinline__ AnnRegs ann_load(const pp_ann *src) {
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
    constexpr int nw = sizeof(pp_ann) / 4;
    const int lane = threadIdx.x & 63;
    AnnRegs r;
#pragma unroll
    for (int u = 0; u < kAnnWords; u++) r.v[u] = (u * 64 + lane < nw) ? s[u * 64 + lane] : 0u;
    return r;
}
__device__ __forceinline__ void ann_store(pp_ann *dst, const AnnRegs &r) {
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    constexpr int nw = sizeof(pp_ann) / 4;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < kAnnWords; u++)
        if (u * 64 + lane < nw) d[u * 64 + lane] = r.v[u];
    wave_sync();
}

__device__ __forceinline__ void copy_ann(pp_ann *dst, const pp_ann *src) {
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    constexpr int nw = sizeof(pp_ann) / 4;
    constexpr int per = (nw + 63) / 64;
    const int lane = threadIdx.x & 63;
    uint32_t v[per];
#pragma unroll
    for (int u = 0; u < per; u++) v[u] = (u * 64 + lane < nw) ? s[u * 64 + lane] : 0u;
#pragma unroll
    for (int u = 0; u < per; u++)
        if (u * 64 + lane < nw) d[u * 64 + lane] = v[u];
    wave_sync();
}

}  // namespace pp

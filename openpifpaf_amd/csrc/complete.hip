// complete.hip — force-complete (complete_annotations, cifcaf.py:309-351): complete_kernel
// with its flood fill, and the functional API's one-connection kernel (pp_grow_connection).
// grow.hpp has the overview.
#include "grow.hpp"

namespace pp {

// _flood_fill's frontier: a binary heap in LDS
__device__ __forceinline__ bool ff_less(const FFEntry &a, const FFEntry &b) {
    if (a.neg != b.neg) return a.neg < b.neg;
    if (a.end != b.end) return a.end < b.end;
    for (int t = 0; t < 3; t++)
        if (a.sxyv[t] != b.sxyv[t]) return a.sxyv[t] < b.sxyv[t];
    return a.s < b.s;
}

__device__ __forceinline__ void ff_push(GrowLDS &L, const FFEntry &x) {
    int i = L.ff_n;
    if (i >= kHeap) {
        L.status |= PP_ST_DEC_OVERFLOW;
        return;
    }
    L.ff_n = i + 1;
    while (i > 0) {
        const int p = (i - 1) >> 1;
        if (!ff_less(x, L.ff[p])) break;
        L.ff[i] = L.ff[p];
        i = p;
    }
    L.ff[i] = x;
}

__device__ __forceinline__ FFEntry ff_pop(GrowLDS &L) {
    const FFEntry top = L.ff[0];
    const int n = L.ff_n - 1;
    L.ff_n = n;
    if (n > 0) {
        const FFEntry x = L.ff[n];
        int i = 0;
        for (;;) {
            const int l = 2 * i + 1, r = l + 1;
            int m = i;
            if (l < n && ff_less(L.ff[l], x)) m = l;
            if (r < n && ff_less(L.ff[r], m == i ? x : L.ff[l])) m = r;
            if (m == i) break;
            L.ff[i] = L.ff[m];
            i = m;
        }
        L.ff[i] = x;
    }
    return top;
}

// cifcaf.py:309-331 (the key is the ENCLOSING xyv, App. D item 5)
__device__ __forceinline__ void flood_fill(const GrowArgs &g, GrowLDS &L) {  // (inlined: a call would copy GrowArgs to scratch)
    L.ff_n = 0;
    auto add = [&](int start_i, float key_v) {
        for (int e = g.j_off[start_i]; e < g.j_off[start_i + 1]; e++) {
            const int end_i = g.d_k[e];
            if (L.a.data[end_i][2] > 0.0f) continue;
            FFEntry x;
            x.neg = -key_v;
            x.end = end_i;
            x.sxyv[0] = L.a.data[start_i][0];
            x.sxyv[1] = L.a.data[start_i][1];
            x.sxyv[2] = L.a.data[start_i][2];
            x.s = L.a.joint_scales[start_i];
            ff_push(L, x);
        }
    };
    for (int j = 0; j < g.K; j++) {
        if (L.a.data[j][2] == 0.0f) continue;
        add(j, L.a.data[j][2]);
    }
    while (L.ff_n > 0) {
        const FFEntry top = ff_pop(L);
        const int end_i = top.end;
        if (L.a.data[end_i][2] > 0.0f) continue;
        L.a.data[end_i][0] = top.sxyv[0];
        L.a.data[end_i][1] = top.sxyv[1];
        L.a.data[end_i][2] = 0.00001f;
        L.a.joint_scales[end_i] = top.s;
        add(end_i, top.sxyv[2]);
    }
}

// ---- complete_annotations (cifcaf.py:333-351) ----
// Each annotation is completed from its own joints and the read-only set-B columns, so the
// annotations of an image are spread over kCompleteWays workgroups.  Ones with every joint
// set are unchanged by it (their frontier is empty) and are skipped, and images the seed
// loop did not flag return at once.
// (5 or 6 waves per SIMD via amdgpu_waves_per_eu: 21 / 46 spills, slower)
// NS: frontier slots per lane (grow_frontier.hpp), 1 when the skeleton has at most 64
// directed edges.
// `ext` (hr_dims): NULL, or the images' own field sizes (complete_ragged_kernel).
template <bool CS, int NS>
__device__ __forceinline__ void complete_body(const GrowArgs &g, const int32_t *ext) {
    __shared__ GrowLDS L;
    const int img = blockIdx.x;
    const int K = g.K;
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
        L.status = 0;
        L.log_n = 0;
        STAMP_DO(for (int q = 0; q < 8; q++) L.fst[q] = 0);
    }
    wave_sync();
    STAMP_DECL
    pp_ann *work = g.work + (int64_t)img * g.ann_cap;
    const int n_anns = g.n_work[img];
    STAMP(0);
    if (!g.need_complete[img]) return;
    // annotations are handed out one at a time (their completion costs differ widely)
    for (;;) {
        int i = 0;
        if (lane == 0) i = atomicAdd(&g.complete_next[img], 1);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= n_anns) break;
        // one vector load for the K visibilities (a short-circuit loop over them would wait
        // for each in turn)
        const float vj = lane < K ? work[i].data[lane][2] : 1.0f;
        if (!__ballot(lane < K && vj == 0.0f)) continue;
        copy_ann(&L.a, &work[i]);
        uint32_t unfilled = 0;
        for (int j = 0; j < K; j++) unfilled |= (L.a.data[j][2] == 0.0f) ? (1u << j) : 0u;
        grow<false, CS, NS, GrowLDS>(g, L, img, 1, false, ColStage{}, nullptr, nullptr, nullptr, ext);
        bool any0 = false;
        for (int j = 0; j < K; j++) {
            float &v = L.a.data[j][2];
            if (((unfilled >> j) & 1u) && v > 0.0f) v = (0.001f < v) ? 0.001f : v;  // np.minimum
            any0 = any0 || v == 0.0f;
        }
        if (any0) flood_fill(g, L);
        wave_sync();
        copy_ann(&work[i], &L.a);
    }
    STAMP(1);
    STAMP_FLUSH(2);
    if (lane == 0 && L.status) atomicOr(&g.status[img], L.status);
}

template <bool CS, int NS>
__global__ __launch_bounds__(64) void complete_kernel(GrowArgs g) {
    complete_body<CS, NS>(g, nullptr);
}

template <bool CS, int NS>
__global__ __launch_bounds__(64) void complete_ragged_kernel(GrowArgs g, const int32_t *ext) {
    complete_body<CS, NS>(g, ext);
}

// ---------------------------------------------------------------------------------------
// host: the kernel's launcher (decode.hip has the rest of the host side)
// ---------------------------------------------------------------------------------------
// force-complete, `ways` workgroups per image (they pull annotations from a per-image counter)
int launch_complete(const GrowArgs &g, int n_img, int ways, hipStream_t s, const int32_t *ext) {
    const dim3 grid(n_img, ways);
    if (ext) {  // a ragged batch: the same instances over the extent table
        if (g.has_cs)
            hipLaunchKernelGGL((complete_ragged_kernel<true, 2>), grid, dim3(64), 0, s, g, ext);
        else if (g.nd <= 64)
            hipLaunchKernelGGL((complete_ragged_kernel<false, 1>), grid, dim3(64), 0, s, g, ext);
        else
            hipLaunchKernelGGL((complete_ragged_kernel<false, 2>), grid, dim3(64), 0, s, g, ext);
        return check_launch("pp_decode_ragged(force complete)");
    }
    if (g.has_cs)  // (two-slot at every skeleton size, as in launch_seed_loop)
        hipLaunchKernelGGL((complete_kernel<true, 2>), grid, dim3(64), 0, s, g);
    else if (g.nd <= 64)
        hipLaunchKernelGGL((complete_kernel<false, 1>), grid, dim3(64), 0, s, g);
    else
        hipLaunchKernelGGL((complete_kernel<false, 2>), grid, dim3(64), 0, s, g);
    return check_launch("pp_decode_batch(force complete)");
}

// ---------------------------------------------------------------------------------------
// one _grow_connection (+ blend / max) on a device column set, for the functional API
// ---------------------------------------------------------------------------------------
// column set in the reference's order, n columns (the functional API entry point)
template <bool MAXM>
__device__ void grow_connection_flat(const float *__restrict__ cf, int n, int64_t hw, float x,
                                     float y, float xy_scale, int exp_mode, float out[4]) {
    const int lane = threadIdx.x & 63;
    const ColQuery q = make_query(x, y, xy_scale, exp_mode);
    Top2 t = top2_empty();
    for (int i = lane; i < n; i += 64) consider<MAXM, false>(cf, hw, q, i, t);
    finish_connection<MAXM>(t, out);
}

template <bool MAXM>
__global__ __launch_bounds__(64) void grow_connection_kernel(const float *cf, int n, int64_t pitch,
                                                             float x, float y, float xy_scale,
                                                             int exp_mode, float *out) {
    float r[4];
    grow_connection_flat<MAXM>(cf, n, pitch, x, y, xy_scale, exp_mode, r);
    if (threadIdx.x < 4) out[threadIdx.x] = r[threadIdx.x];
}

}  // namespace pp

using namespace pp;

extern "C" int pp_grow_connection(const float *d_cols, int64_t n, int64_t pitch, float x, float y,
                                  float xy_scale, int32_t method, float *d_out, void *stream) {
    if (!d_cols || !d_out) return fail(PP_EINVAL, "pp_grow_connection: NULL argument");
    if (n < 0 || pitch < n || n > INT32_MAX) return fail(PP_ESHAPE, "pp_grow_connection: bad shape");
    // bit 0: connection method (0 blend, 1 max); bit 1: pp_config.exp_mode 1 (correctly
    // rounded np.exp instead of NumPy's SIMD one)
    if (method < 0 || method > 3) return fail(PP_EINVAL, "connection method not known");
    hipStream_t s = (hipStream_t)stream;
    const int exp_mode = (method >> 1) & 1;
    if (method & 1)
        hipLaunchKernelGGL(grow_connection_kernel<true>, dim3(1), dim3(64), 0, s, d_cols, (int)n,
                           pitch, x, y, xy_scale, exp_mode, d_out);
    else
        hipLaunchKernelGGL(grow_connection_kernel<false>, dim3(1), dim3(64), 0, s, d_cols, (int)n,
                           pitch, x, y, xy_scale, exp_mode, d_out);
    return check_launch("pp_grow_connection");
}

// edges.hip — batched CifCaf.connection_value and CifCaf.p2p_value (cifcaf.py:194-245) over
// CafScored column sets: pp_connection_values and pp_p2p_values.  One wave per query, four
// waves per workgroup; a query names one flat (9, n) set in the layout pp_caf_scored writes
// ((n_caf, 2, 9, cap) floats and (n_caf, 2) counts, direction 1 forward), so the opposite
// direction's set of query set s is s ^ 1.  Lanes stride the columns, the row loads stay
// coalesced; any number of queries goes in one launch with no read-back.
//
// connection: the forward _grow_connection, the keypoint threshold on the geometric mean,
// the zero-score exit, and with reverse_match a second _grow_connection over set s ^ 1 from
// the new point; as the reference (cifcaf.py:212) and grow_connection.hpp's
// connection_value do, the reverse result is tested for a zero SCALE.
//
// p2p: per column inside the 2 * max(0, source_s) box, exp(-0.5 d_s^2 / sigma_s^2) *
// exp(-0.5 d_t^2 / sigma_t^2) * v in that order, then Python's max() over the kept columns
// in column order: max() keeps its first element unless a later one compares greater, so
// the result is NaN exactly when the FIRST kept column's score is NaN, a NaN in a later
// column never wins, and among equal scores (+0.0 and -0.0) the earliest column stays.
#include "grow_connection.hpp"

namespace pp {

constexpr int kEdgeWaves = 4;  // queries (waves) per workgroup

// the set of a query: NULL columns / 0 for an index outside [0, n_sets); the count is held
// to [0, pitch], whatever the counts array says
struct EdgeSets {
    const float *cols;
    const int32_t *counts;
    int64_t set_stride, pitch;
    int n_sets;
};

__device__ __forceinline__ int edge_set(const EdgeSets &s, int set, const float *&cf) {
    cf = s.cols;
    if (set < 0 || set >= s.n_sets) return 0;
    cf = s.cols + (int64_t)set * s.set_stride;
    const int64_t n = s.counts[set];
    return (int)(n < 0 ? 0 : (n > s.pitch ? s.pitch : n));
}

// _grow_connection on a flat set in the reference's column order (complete.hip's
// grow_connection_flat: make_query, consider, finish_connection)
template <bool MAXM>
__device__ __forceinline__ void grow_flat(const float *__restrict__ cf, int n, int64_t hw, float x,
                                          float y, float xy_scale, int exp_mode, float out[4]) {
    const int lane = threadIdx.x & 63;
    const ColQuery q = make_query(x, y, xy_scale, exp_mode);
    Top2 t = top2_empty();
    for (int i = lane; i < n; i += 64) consider<MAXM, false>(cf, hw, q, i, t);
    finish_connection<MAXM>(t, out);
}

// cifcaf.py:194-217 (every value below is uniform over the wave)
template <bool MAXM>
__device__ __forceinline__ void connection_flat(const EdgeSets &s, const pp_edge_query &e, int exp_mode,
                                                float keypoint_threshold, bool reverse_match,
                                                float out[4]) {
    const float *cf;
    const int n = edge_set(s, e.set, cf);
    const float xy_scale_s = max0(e.s);
    float nx[4];
    grow_flat<MAXM>(cf, n, s.pitch, e.x, e.y, xy_scale_s, exp_mode, nx);
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    const float ks = sqrtf(nx[3] * e.v);  // geometric mean
    if (ks < keypoint_threshold) return;
    if (nx[3] == 0.0f) return;
    if (reverse_match) {
        const float *cb;
        const int nb = edge_set(s, e.set ^ 1, cb);
        float rv[4];
        grow_flat<MAXM>(cb, nb, s.pitch, nx[0], nx[1], max0(nx[2]), exp_mode, rv);
        if (rv[2] == 0.0f) return;  // tests the SCALE (cifcaf.py:212)
        if (fabsf(e.x - rv[0]) + fabsf(e.y - rv[1]) > xy_scale_s) return;
    }
    out[0] = nx[0];
    out[1] = nx[1];
    out[2] = nx[2];
    out[3] = ks;
}

// a float's bits in an order that unsigned comparison follows (-0.0 ranked as +0.0; never
// called with NaN)
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// cifcaf.py:219-245
__device__ __forceinline__ float p2p_flat(const EdgeSets &s, const pp_edge_query &e, int exp_mode) {
    const int lane = threadIdx.x & 63;
    const float *cf;
    const int n = edge_set(s, e.set, cf);
    const int64_t hw = s.pitch;
    const ColQuery q = make_query(e.x, e.y, max0(e.s), exp_mode);
    // the target term's divisor: no box bounds d_target, so score_arg's refined reciprocal
    // has no domain here and the quotient is the IEEE division
    const float sigma_t = 0.5f * max0(e.ts);
    const float sigma_t2 = np_pow2_f32(sigma_t);
    // keys, 0 = none, larger = better; the low word prefers the lower column index.
    // first: this lane's first kept column (bit 0: its score is NaN); best: its largest
    // score that is a number, the earliest of equal ones
    uint64_t first = 0, best = 0;
    float best_score = 0.0f;
    for (int i = lane; i < n; i += 64) {
        const float c1 = cf[hw + i], c2 = cf[2 * hw + i], c0 = cf[i];
        const float t1 = cf[5 * hw + i], t2 = cf[6 * hw + i];
        if (c1 < q.lo_x || c1 > q.hi_x || c2 < q.lo_y || c2 > q.hi_y) continue;  // caf_center_s
        const float dx = q.x - c1, dy = q.y - c2;
        const float ds = sqrtf(dx * dx + dy * dy);  // np.linalg.norm(axis=0)
        const float ex = e.tx - t1, ey = e.ty - t2;
        const float dt = sqrtf(ex * ex + ey * ey);
        const float score = caf_exp(score_arg(q, ds), exp_mode) *
                            caf_exp((-0.5f * (dt * dt)) / sigma_t2, exp_mode) * c0;
        const uint32_t rank = (uint32_t)(0x7FFFFFFF - i);
        const bool nan = score != score;
        const uint64_t fk = ((uint64_t)rank << 1) | (nan ? 1u : 0u);
        first = fk > first ? fk : first;
        const uint64_t bk = nan ? 0 : (((uint64_t)ordered_bits(score) << 32) | rank);
        if (bk > best) {
            best = bk;
            best_score = score;
        }
    }
    const uint64_t f1 = wave_max_u64(first);
    const uint64_t b1 = wave_max_u64(best);
    if (f1 == 0) return 0.0f;  // caf_field.shape[1] == 0
    float mx = __builtin_nanf("");
    if (!(f1 & 1)) {  // the first kept score is a number, so b1 != 0
        const uint64_t m = __ballot(best == b1);
        mx = rl_f(best_score, __ffsll((unsigned long long)m) - 1);
    }
    return sqrtf(e.v * mx);
}

// this wave's query index, uniform (a scalar register), or -1 past the end
__device__ __forceinline__ int64_t edge_query_index(int64_t n_q) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w = (int64_t)blockIdx.x * kEdgeWaves + wave;
    return w < n_q ? w : -1;
}

template <bool MAXM>
__global__ __launch_bounds__(64 * kEdgeWaves) void connection_values_kernel(
    EdgeSets s, const pp_edge_query *__restrict__ queries, int64_t n_q, int exp_mode,
    float keypoint_threshold, int reverse_match, float *__restrict__ out) {
    const int64_t w = edge_query_index(n_q);
    if (w < 0) return;  // the whole wave
    const pp_edge_query e = queries[w];
    float r[4];
    connection_flat<MAXM>(s, e, exp_mode, keypoint_threshold, reverse_match != 0, r);
    const int lane = threadIdx.x & 63;
    if (lane < 4) out[w * 4 + lane] = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3];
}

__global__ __launch_bounds__(64 * kEdgeWaves) void p2p_values_kernel(
    EdgeSets s, const pp_edge_query *__restrict__ queries, int64_t n_q, int exp_mode,
    float *__restrict__ out) {
    const int64_t w = edge_query_index(n_q);
    if (w < 0) return;
    const pp_edge_query e = queries[w];
    const float r = p2p_flat(s, e, exp_mode);
    if ((threadIdx.x & 63) == 0) out[w] = r;
}

// admission checks shared by the two entries; PP_OK with *launch = false for no queries
int edge_admit(const char *who, const float *cols, int64_t set_stride, int64_t pitch,
               const int32_t *counts, int32_t n_sets, const pp_edge_query *queries, int64_t n_q,
               int32_t method, const float *out, bool pairs, bool *launch) {
    *launch = false;
    if (n_q < 0 || n_q > INT32_MAX || n_sets < 0 || pitch < 0 || pitch > INT32_MAX ||
        set_stride < 9 * pitch)
        return fail(PP_ESHAPE, std::string(who) + ": bad shape");
    if (pairs && (n_sets & 1))
        return fail(PP_ESHAPE, std::string(who) + ": reverse_match needs the sets in (backward, "
                                                  "forward) pairs, n_sets is odd");
    // bit 0: connection method (0 blend, 1 max); bit 1: pp_config.exp_mode 1
    if (method < 0 || method > 3) return fail(PP_EINVAL, "connection method not known");
    if (n_q == 0) return PP_OK;
    if (!queries || !out || (n_sets > 0 && (!cols || !counts)))
        return fail(PP_EINVAL, std::string(who) + ": NULL argument");
    *launch = true;
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_connection_values(const float *d_cols, int64_t set_stride, int64_t pitch,
                                    const int32_t *d_counts, int32_t n_sets,
                                    const pp_edge_query *d_queries, int64_t n_q, int32_t method,
                                    float keypoint_threshold, int32_t reverse_match, float *d_out,
                                    void *stream) {
    bool launch;
    const int rc = edge_admit("pp_connection_values", d_cols, set_stride, pitch, d_counts, n_sets,
                              d_queries, n_q, method, d_out, reverse_match != 0, &launch);
    if (rc != PP_OK || !launch) return rc;
    const EdgeSets s{d_cols, d_counts, set_stride, pitch, n_sets};
    const dim3 grid((unsigned)((n_q + kEdgeWaves - 1) / kEdgeWaves)), block(64 * kEdgeWaves);
    hipStream_t st = (hipStream_t)stream;
    const int exp_mode = (method >> 1) & 1;
    if (method & 1)
        hipLaunchKernelGGL(connection_values_kernel<true>, grid, block, 0, st, s, d_queries, n_q,
                           exp_mode, keypoint_threshold, reverse_match, d_out);
    else
        hipLaunchKernelGGL(connection_values_kernel<false>, grid, block, 0, st, s, d_queries, n_q,
                           exp_mode, keypoint_threshold, reverse_match, d_out);
    return check_launch("pp_connection_values");
}

extern "C" int pp_p2p_values(const float *d_cols, int64_t set_stride, int64_t pitch,
                             const int32_t *d_counts, int32_t n_sets,
                             const pp_edge_query *d_queries, int64_t n_q, int32_t method,
                             float *d_out, void *stream) {
    bool launch;
    const int rc = edge_admit("pp_p2p_values", d_cols, set_stride, pitch, d_counts, n_sets,
                              d_queries, n_q, method, d_out, false, &launch);
    if (rc != PP_OK || !launch) return rc;
    const EdgeSets s{d_cols, d_counts, set_stride, pitch, n_sets};
    const dim3 grid((unsigned)((n_q + kEdgeWaves - 1) / kEdgeWaves)), block(64 * kEdgeWaves);
    hipLaunchKernelGGL(p2p_values_kernel, grid, block, 0, (hipStream_t)stream, s, d_queries, n_q,
                       (method >> 1) & 1, d_out);
    return check_launch("pp_p2p_values");
}

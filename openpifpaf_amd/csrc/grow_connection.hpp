// grow_connection.hpp — one connection of the CifCaf decoder scored by a wave:
// _grow_connection and connection_value (cifcaf.py:124-217) over a bucketed column set.
// grow.hpp has the overview.
#pragma once

#include "grow_device.hpp"

namespace pp {

// ---------------------------------------------------------------------------------------
// _grow_connection: caf_center_s + scores + blend / max (cifcaf.py:124-192)
// ---------------------------------------------------------------------------------------
// Candidate columns are ranked by a 64-bit key, larger = better: high word = the score's
// bits (scores are >= 0, so float order == unsigned order; NaN sorts last in np.argsort,
// i.e. largest, and its bits are above every finite score), low word = the column's
// row-major index, so ties follow the reference: blend (stable argsort, last wins) ->
// higher index; max (np.argmax, first wins) -> lower index.  0 = no candidate.
template <bool MAXM>
__device__ __forceinline__ uint64_t cand_key(float score, int o) {
    const uint32_t hi = (score != score) ? 0xFFFFFFFFu : __float_as_uint(score);
    const uint32_t lo = MAXM ? (uint32_t)(0x7FFFFFFF - o) : (uint32_t)(o + 1);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ float key_score(uint64_t k) { return __uint_as_float((uint32_t)(k >> 32)); }

struct Top2 {
    uint64_t k1, k2;   // best and second-best keys of this lane (0 = none)
    float x1, y1, c1;  // target (x2, y2, s2) rows of the best column
    float x2, y2, c2;  // ... and of the second best
};

// branch-free on purpose: values feed DPP reductions, which must not run under a
// partial exec mask
__device__ __forceinline__ void top2_insert(Top2 &t, uint64_t k, float x, float y, float c) {
    const bool b1 = k > t.k1;
    const bool b2 = !b1 & (k > t.k2);
    t.k2 = b1 ? t.k1 : (b2 ? k : t.k2);
    t.x2 = b1 ? t.x1 : (b2 ? x : t.x2);
    t.y2 = b1 ? t.y1 : (b2 ? y : t.y2);
    t.c2 = b1 ? t.c1 : (b2 ? c : t.c2);
    t.k1 = b1 ? k : t.k1;
    t.x1 = b1 ? x : t.x1;
    t.y1 = b1 ? y : t.y1;
    t.c1 = b1 ? c : t.c1;
}

template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
    const uint32_t lo = (uint32_t)dpp_i<CTRL, ROWS>(0, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)dpp_i<CTRL, ROWS>(0, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// max of a 64-bit key over the wave, uniform result
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    uint64_t o;
    o = dpp_u64<kDppXor1, 0xF>(v);
    v = o > v ? o : v;
    o = dpp_u64<kDppXor2, 0xF>(v);
    v = o > v ? o : v;
    o = dpp_u64<kDppHalfMirror, 0xF>(v);
    v = o > v ? o : v;
    o = dpp_u64<kDppMirror, 0xF>(v);
    v = o > v ? o : v;
    o = dpp_u64<kDppBcast15, 0xA>(v);
    v = o > v ? o : v;
    o = dpp_u64<kDppBcast31, 0xC>(v);
    v = o > v ? o : v;
    const uint32_t lo = (uint32_t)rl_i((int)(uint32_t)v, 63);
    const uint32_t hi = (uint32_t)rl_i((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

// exact top-2 over the wave (uniform): the global best K1 by a max reduction, then the
// best key other than K1 (keys are unique per column); targets from the holding lane
struct Best2 {
    uint64_t k1, k2;
    float x1, y1, c1, x2, y2, c2;
};

__device__ __forceinline__ uint64_t rl_u64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)rl_i((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)rl_i((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// at most two lanes hold candidates (the usual case: the 2*scale box passes a handful of
// columns): merge them with scalar reads instead of the two DPP reductions
__device__ __forceinline__ Best2 top2_wave(const Top2 &t) {
    Best2 b;
    const uint64_t cm = __ballot(t.k1 != 0);
    if (__popcll(cm) <= 2) {
        const uint64_t cm2 = cm & (cm - 1);
        const int la = cm ? __ffsll((unsigned long long)cm) - 1 : 0;
        const int lb = cm2 ? __ffsll((unsigned long long)cm2) - 1 : la;
        const uint64_t ka1 = rl_u64(t.k1, la), ka2 = rl_u64(t.k2, la);
        const uint64_t kb1 = cm2 ? rl_u64(t.k1, lb) : 0, kb2 = cm2 ? rl_u64(t.k2, lb) : 0;
        const bool a_first = ka1 > kb1;  // equal only when both are 0
        const int l1 = a_first ? la : lb, lo = a_first ? lb : la;
        const uint64_t own2 = a_first ? ka2 : kb2, oth1 = a_first ? kb1 : ka1;
        const bool own_second = own2 > oth1;  // the best lane's runner-up beats the other's best
        b.k1 = a_first ? ka1 : kb1;
        b.k2 = own_second ? own2 : oth1;
        b.x1 = rl_f(t.x1, l1);
        b.y1 = rl_f(t.y1, l1);
        b.c1 = rl_f(t.c1, l1);
        const int l2 = own_second ? l1 : lo;
        b.x2 = own_second ? rl_f(t.x2, l2) : rl_f(t.x1, l2);
        b.y2 = own_second ? rl_f(t.y2, l2) : rl_f(t.y1, l2);
        b.c2 = own_second ? rl_f(t.c2, l2) : rl_f(t.c1, l2);
        return b;
    }
    b.k1 = wave_max_u64(t.k1);
    b.k2 = wave_max_u64(t.k1 == b.k1 ? t.k2 : t.k1);
    const uint64_t m1 = __ballot(t.k1 == b.k1 && b.k1 != 0);
    const int l1 = m1 ? __ffsll((unsigned long long)m1) - 1 : 0;
    b.x1 = rl_f(t.x1, l1);
    b.y1 = rl_f(t.y1, l1);
    b.c1 = rl_f(t.c1, l1);
    const uint64_t m2a = __ballot(t.k1 == b.k2 && b.k2 != 0);
    const uint64_t m2b = __ballot(t.k2 == b.k2 && b.k2 != 0);
    const int l2a = m2a ? __ffsll((unsigned long long)m2a) - 1 : 0;
    const int l2b = m2b ? __ffsll((unsigned long long)m2b) - 1 : 0;
    b.x2 = m2a ? rl_f(t.x1, l2a) : rl_f(t.x2, l2b);
    b.y2 = m2a ? rl_f(t.y1, l2a) : rl_f(t.y2, l2b);
    b.c2 = m2a ? rl_f(t.c1, l2a) : rl_f(t.c2, l2b);
    return b;
}

struct ColQuery {
    float x, y, lo_x, hi_x, lo_y, hi_y, sigma2;
    int exp_mode;  // pp_config.exp_mode (caf_exp)
    // sigma2's refined reciprocal (div_refined) for every column's -0.5 d^2 / sigma2, when
    // the query is in its domain: sigma2 in [1, 2^90] and finite box bounds (a column that
    // passes the box test then has |-0.5 d^2| <= 16 sigma2 <= 2^94); else IEEE division
    Recip sr;
    bool fast;
};

__device__ __forceinline__ ColQuery make_query(float x, float y, float xy_scale, int exp_mode) {
    ColQuery q;
    q.exp_mode = exp_mode;
    const float sbox = 2.0f * xy_scale;  // caf_center_s(..., sigma=2.0 * xy_scale)
    q.x = x;
    q.y = y;
    q.lo_x = x - sbox;
    q.hi_x = x + sbox;
    q.lo_y = y - sbox;
    q.hi_y = y + sbox;
    const float sigma = 0.5f * xy_scale;
    q.sigma2 = np_pow2_f32(sigma);  // `sigma**2` of a NumPy float32 scalar: libm powf
    q.sr = recip_of(q.sigma2);
    q.fast = q.sigma2 >= 1.0f && q.sigma2 <= 0x1p90f && fabsf(q.lo_x) <= 0x1p100f &&
             fabsf(q.hi_x) <= 0x1p100f && fabsf(q.lo_y) <= 0x1p100f && fabsf(q.hi_y) <= 0x1p100f;
    return q;
}

// -0.5 d^2 / sigma^2 of a column inside the query's box (cifcaf.py:139), IEEE-rounded
__device__ __forceinline__ float score_arg(const ColQuery &q, float dd) {
    const float n = -0.5f * (dd * dd);
    return q.fast ? div_refined(n, q.sr) : n / q.sigma2;
}

// column k (all rows loaded in one round): caf_center_s test, score (cifcaf.py:134-139).
// PACKED: the decoder's kColRows layout (index in row 6); else the reference's 9 rows
// with the column's position k as its index.
template <bool MAXM>
__device__ __forceinline__ void consider_vals(const ColQuery &q, float c0, float c1, float c2, float tx,
                                              float ty, float tc, int o, Top2 &t) {
    if (c1 < q.lo_x || c1 > q.hi_x || c2 < q.lo_y || c2 > q.hi_y) return;
    const float dx = q.x - c1, dy = q.y - c2;
    const float dd = sqrtf(dx * dx + dy * dy);  // np.linalg.norm(axis=0)
    const float score = caf_exp(score_arg(q, dd), q.exp_mode) * c0;  // np.exp
    top2_insert(t, cand_key<MAXM>(score, o), tx, ty, tc);
}

template <bool MAXM, bool PACKED>
__device__ __forceinline__ void consider(const float *__restrict__ cf, int64_t hw, const ColQuery &q,
                                         int k, Top2 &t) {
    const float c1 = cf[hw + k], c2 = cf[2 * hw + k], c0 = cf[k];
    const float tx = cf[(PACKED ? 3 : 5) * hw + k], ty = cf[(PACKED ? 4 : 6) * hw + k];
    const float tc = cf[(PACKED ? 5 : 8) * hw + k];
    const int o = PACKED ? __float_as_int(cf[6 * hw + k]) : k;
    consider_vals<MAXM>(q, c0, c1, c2, tx, ty, tc, o, t);
}

// a set-B column: concatenated cell index -> the head's raw CAF values (caf_scored.py:58-81
// for this one column: rows * stride, CifHr rescoring at the target, the second
// threshold), then as consider
struct RawSet {
    const int *idx;      // bucketed concatenated cell indices (int32), or
    const uint16_t *idx16;  // u16 ones (sets of at most kSetBIdx16Max cells)
    int64_t fld;         // image * C + CAF field
    int64_t hrt;         // CifHr plane of the direction's target joint (rescore), or -1
    int src, tgt, tsc;   // raw rows of source x, target x, target scale (y = x + 1)
    HrDims dm;           // the image's own CifHr size (hr_dims)
};

template <bool MAXM>
__device__ __forceinline__ void consider_raw(const GrowArgs &g, const RawSet &r, const ColQuery &q,
                                             int k, Top2 &t) {
    const int key = r.idx16 ? (int)r.idx16[k] : r.idx[k];
    const Heads &h = g.heads;
    int hm = 0, cell = key;
    if (h.n_caf > 1) {
        hm = h.caf_head_of(key);
        cell = key - (int)h.caf_off[hm];
    }
    const int64_t hw = (int64_t)h.aH[hm] * h.aW[hm];
    const float stride = (float)h.astride[hm];
    const float *caf9 = h.caf[hm] + r.fld * 9 * hw;
    const float c = caf9[cell];
    const float c1 = caf9[r.src * hw + cell] * stride;
    const float c2 = caf9[(r.src + 1) * hw + cell] * stride;
    const float tx = caf9[r.tgt * hw + cell] * stride;
    const float ty = caf9[(r.tgt + 1) * hw + cell] * stride;
    const float tc = caf9[r.tsc * hw + cell] * stride;
    if (c1 < q.lo_x || c1 > q.hi_x || c2 < q.lo_y || c2 > q.hi_y) return;
    float c0 = c;
    if (r.hrt >= 0) c0 = c * (g.cif_floor + g.one_minus_floor * g.hr.at(r.hrt, tx, ty, 0.0f, r.dm.hh, r.dm.ww));
    if (!(c0 > g.th_b)) return;
    const float dx = q.x - c1, dy = q.y - c2;
    const float dd = sqrtf(dx * dx + dy * dy);
    const float score = caf_exp(score_arg(q, dd), q.exp_mode) * c0;
    top2_insert(t, cand_key<MAXM>(score, key), tx, ty, tc);
}

// _target_with_blend / _target_with_maxscore (cifcaf.py:147-192) on the merged top-2
template <bool MAXM>
__device__ __forceinline__ void finish_connection(const Top2 &t, float out[4]) {
    const Best2 b = top2_wave(t);
    if (b.k1 == 0) {  // no candidate (every candidate's key is nonzero)
        out[0] = out[1] = out[2] = out[3] = 0.0f;
        return;
    }
    const float s1 = key_score(b.k1), s2 = key_score(b.k2);
    if (MAXM) {
        out[0] = b.x1;
        out[1] = b.y1;
        out[2] = b.c1;
        out[3] = s1;
        return;
    }
    // one candidate (len(scores) == 1): k2 = 0, s2 = 0.0 takes this branch with the same
    // result
    if (s2 < 0.01f || s2 < 0.5f * s1) {
        out[0] = b.x1;
        out[1] = b.y1;
        out[2] = b.c1;
        out[3] = s1 * 0.5f;
        return;
    }
    const float ex = b.x1 - b.x2, ey = b.y1 - b.y2;
    const float dist = sqrtf(ex * ex + ey * ey);
    if (dist > b.c1 / 2.0f) {
        out[0] = b.x1;
        out[1] = b.y1;
        out[2] = b.c1;
        out[3] = s1 * 0.5f;
        return;
    }
    const float ssum = s1 + s2;
    out[0] = (s1 * b.x1 + s2 * b.x2) / ssum;
    out[1] = (s1 * b.y1 + s2 * b.y2) / ssum;
    out[2] = (s1 * b.c1 + s2 * b.c2) / ssum;
    out[3] = 0.5f * (s1 + s2);
}

__device__ __forceinline__ Top2 top2_empty() {
    Top2 t;
    t.k1 = t.k2 = 0;
    t.x1 = t.y1 = t.c1 = t.x2 = t.y2 = t.c2 = 0.0f;
    return t;
}

// diagnostic build: grow_connection's section sums into g.gc_stamps[img][4]
#ifdef PP_STAMPS
#define GSTAMP(i)                                                                           \
    do {                                                                                    \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                                   \
        if (lane == 0 && g.gc_stamps) atomicAdd((unsigned long long *)&g.gc_stamps[blockIdx.x * 4 + (i)], (unsigned long long)(t_ - gs_t));        \
        gs_t = t_;                                                                          \
    } while (0)
#else
#define GSTAMP(i)
#endif

// bucketed column set (caf_bucketed_kernel): visit only the buckets the 2*scale box
// overlaps (+ the NaN-source bucket); segments flattened over the 64 lanes
template <bool MAXM, bool RAW>
__device__ __forceinline__ void grow_connection(const GrowArgs &g, const float *__restrict__ cf, const RawSet &raw,
                                const int *__restrict__ off, float x, float y, float xy_scale,
                                float out[4]) {
    const int lane = threadIdx.x & 63;
    STAMP_T0(gs_t);
    const int64_t hw = g.col_cap;
    const ColQuery q = make_query(x, y, xy_scale, g.cfg.exp_mode);
    Top2 t = top2_empty();
    int bx0, bx1, by0, by1;
    if (q.lo_x != q.lo_x || q.hi_x != q.hi_x || q.lo_y != q.lo_y || q.hi_y != q.hi_y) {
        bx0 = 0;  // NaN bounds pass every column (every comparison is false): scan all
        bx1 = g.bw - 1;
        by0 = 0;
        by1 = g.bh - 1;
    } else {
        bx0 = (int)fminf(fmaxf(floorf(q.lo_x * g.inv_e), 0.0f), (float)(g.bw - 1));
        bx1 = (int)fminf(fmaxf(floorf(q.hi_x * g.inv_e), 0.0f), (float)(g.bw - 1));
        by0 = (int)fminf(fmaxf(floorf(q.lo_y * g.inv_e), 0.0f), (float)(g.bh - 1));
        by1 = (int)fminf(fmaxf(floorf(q.hi_y * g.inv_e), 0.0f), (float)(g.bh - 1));
    }
    const int nseg = (by1 - by0 + 1) + 1;  // bucket rows + the NaN bucket
    for (int sb = 0; sb < nseg; sb += 64) {
        const int r = sb + lane;
        int st = 0, len = 0;
        if (r < nseg) {
            int lo, hi;
            if (r == nseg - 1) {
                lo = g.nb - 1;
                hi = g.nb;
            } else {
                const int row = by0 + r;
                lo = row * g.bw + bx0;
                hi = row * g.bw + bx1 + 1;
            }
            st = off[lo];
            len = off[hi] - st;
        }
        const int ng = min(64, nseg - sb);
        int total = 0;
        for (int rr = 0; rr < ng; rr++) total += rl_i(len, rr);  // scalar
        GSTAMP(0);
        for (int base = 0; base < total; base += 64) {
            const int tt = base + lane;
            int k = -1, run = 0;
            for (int rr = 0; rr < ng; rr++) {  // the segment holding tt (uniform loop)
                const int l = rl_i(len, rr);
                if (tt >= run && tt < run + l) k = rl_i(st, rr) + (tt - run);
                run += l;
            }
            if (k >= 0) {
                if (RAW)
                    consider_raw<MAXM>(g, raw, q, k, t);
                else
                    consider<MAXM, true>(cf, hw, q, k, t);
            }
        }
        GSTAMP(1);
    }
    finish_connection<MAXM>(t, out);
    GSTAMP(2);
}

__device__ __forceinline__ float max0(float v) { return (v > 0.0f) ? v : 0.0f; }

__device__ __forceinline__ const float *col_set(const GrowArgs &g, int set, int img, int caf_i,
                                                int dir) {
    return g.cols[set] + (((int64_t)img * g.C + caf_i) * 2 + dir) * (set ? 1 : kColRows) * g.col_cap;
}

// set B of (image, CAF, direction): dir 1 forward (x1, y1) -> (x2, y2, s2), rescored at
// joint j2; dir 0 backward (x2, y2) -> (x1, y1, s1), rescored at j1 (caf_scored.py:58-81)
__device__ __forceinline__ RawSet raw_set(const GrowArgs &g, int img, int caf_i, int dir,
                                          const int32_t *ext) {
    RawSet r;
    r.dm = hr_dims(ext, img, g.heads.cstride[0], g.hr.hh, g.hr.ww);
    const float *cs = col_set(g, 1, img, caf_i, dir);
    const bool i16 = g.col_cap <= kSetBIdx16Max;  // caf_bucketed_kernel<true, true>
    r.idx = i16 ? nullptr : reinterpret_cast<const int *>(cs);
    r.idx16 = i16 ? reinterpret_cast<const uint16_t *>(cs) : nullptr;
    r.fld = (int64_t)img * g.C + caf_i;
    const int tj = dir ? g.caf_j2[caf_i] : g.caf_j1[caf_i];
    r.hrt = (g.cif_floor < 1.0f && tj < g.K) ? (int64_t)img * g.K + tj : -1;
    r.src = dir ? 1 : 5;
    r.tgt = dir ? 5 : 1;
    r.tsc = dir ? 8 : 4;
    return r;
}

__device__ __forceinline__ const int *col_offs(const GrowArgs &g, int set, int img, int caf_i,
                                               int dir) {
    return g.offs[set] + (((int64_t)img * g.C + caf_i) * 2 + dir) * (int64_t)(g.nb + 1);
}

// cifcaf.py:194-217 for start joint (jx, jy, jv, js) along CAF caf_i in direction fwd
__device__ __forceinline__ void connection_value(const GrowArgs &g, int img, int set, int caf_i, int fwd,
                                 float jx, float jy, float jv, float js, bool reverse_match,
                                 float out[4], const int32_t *ext = nullptr) {
    const int df = fwd ? 1 : 0, db = fwd ? 0 : 1;
    const float xy_scale_s = max0(js);
    const bool maxm = g.cfg.connection_method == 1;
    // one query along direction `dir` from (qx, qy, qs)
    auto query = [&](int dir, float qx, float qy, float qs, float r[4]) {
        const float *cf = col_set(g, set, img, caf_i, dir);
        const int *off = col_offs(g, set, img, caf_i, dir);
        if (set) {
            const RawSet raw = raw_set(g, img, caf_i, dir, ext);
            if (maxm)
                grow_connection<true, true>(g, cf, raw, off, qx, qy, qs, r);
            else
                grow_connection<false, true>(g, cf, raw, off, qx, qy, qs, r);
        } else {
            const RawSet none{};
            if (maxm)
                grow_connection<true, false>(g, cf, none, off, qx, qy, qs, r);
            else
                grow_connection<false, false>(g, cf, none, off, qx, qy, qs, r);
        }
    };
    float nx[4];
    query(df, jx, jy, xy_scale_s, nx);

    out[0] = out[1] = out[2] = out[3] = 0.0f;
    const float ks = sqrtf(nx[3] * jv);  // geometric mean
    if (ks < g.cfg.keypoint_threshold) return;
    if (nx[3] == 0.0f) return;
    const float xy_scale_t = max0(nx[2]);
    if (reverse_match) {
        float rv[4];
        query(db, nx[0], nx[1], xy_scale_t, rv);
        if (rv[2] == 0.0f) return;  // tests the SCALE (cifcaf.py:212)
        if (fabsf(jx - rv[0]) + fabsf(jy - rv[1]) > xy_scale_s) return;
    }
    out[0] = nx[0];
    out[1] = nx[1];
    out[2] = nx[2];
    out[3] = ks;
}

}  // namespace pp

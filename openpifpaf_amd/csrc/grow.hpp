// grow.hpp — the CifCaf greedy decoder (generator/cifcaf.py) on gfx950: `grow` and the
// occupancy grid's marks.
//
// The seed loop is sequential by construction (each annotation's occupancy marks decide
// whether later seeds start annotations, cifcaf.py:100-108), so an image is one workgroup
// and a batch fills the chip with one workgroup per image.  Inside it, wave 0 commits in
// the reference order while seven helper waves grow seeds it is likely to reach (a grow is
// a pure function of the seed and the CAF columns); each wave's serial state lives in
// REGISTERS, not memory:
//
//   * the annotation being grown: lane j holds joint j's (x, y, v, scale);
//   * the frontier (cifcaf.py:248 PriorityQueue): at most one entry per directed skeleton
//     edge is ever live (in_frontier admits (j, k) once; its evaluated re-push replaces
//     the popped unevaluated entry), so lane d holds the entry of directed edge d (by_source
//     order, cifcaf.py:62-65) and pop-min is a wave reduction with the reference's tuple
//     order (-score, None|xysv, j, k);
//   * caf_center_s + scoring (functional.pyx:338-359, cifcaf.py:124-145): the lanes scan
//     the CAF columns (the image's small set-A sets from LDS, else the buckets the 2*scale
//     box overlaps, caf_bucketed_kernel) and merge the argsort top-2 _target_with_blend
//     (cifcaf.py:157-192) needs, targets included;
//   * occupancy grids (occupancy.py, u8 += 1 with wrap) live in a per-image workspace that
//     every launch leaves zeroed: each box a launch marks is logged and cleared again.
//
// Force-complete (cifcaf.py:333-351) spreads an image's annotations over 64 workgroups;
// NMS (nms.py:17-57) is one 8-wave workgroup per image.  Float arithmetic is f32
// op-for-op as NumPy evaluates it (NEP 50); np.exp is computed correctly rounded through
// f64.
//
// grow_connection.hpp scores one connection, grow_frontier.hpp holds the frontier,
// grow_columns.hpp reads the small column sets flat; seed_loop.hpp and seed_loop.hip /
// seed_loop_ext.hip are the seed loops, complete.hip is force-complete, nms.hip the NMS.
#pragma once

#include "grow_columns.hpp"

namespace pp {

// _grow (cifcaf.py:247-307) on the record in L.a (joint data mirrored into registers).
// AHEAD (seed loop: set A, reverse_match): new entries' connections via eval_ahead from
// the image's set-A column counts and LDS-staged sets.  Force-complete (set B, no reverse
// matching) evaluates each entry when it is popped: evaluating set-B connections ahead, a
// few edges per memory round trip, needed 224 VGPRs (2 waves per SIMD instead of 4) and
// measured slower (planted cfg3 323k vs 331k, uniform 12.4k vs 15.1k-15.7k images/s, round 4).
// `abort` (a seed-loop helper's speculative grow): stop at the next pop once *abort is set
// (wave 0 is done: the result would never be read)
// NS: the frontier's slots per lane (grow_frontier.hpp): 1 when g.nd <= 64, else 2; the
// launchers pick the kernel instance.
template <bool AHEAD, bool CS, int NS, typename LDS>
__device__ __forceinline__ void grow(const GrowArgs &g, LDS &L, int img, int set, bool reverse_match,
                                     const ColStage &cs = ColStage{}, int *abort = nullptr,
                                     float4 *pub = nullptr, uint32_t *pub_mask = nullptr,
                                     const int32_t *ext = nullptr) {
    const int lane = threadIdx.x & 63;
    const int K = g.K;
    float ax = 0.0f, ay = 0.0f, av = 0.0f, as = 0.0f;
    if (lane < K) {
        ax = L.a.data[lane][0];
        ay = L.a.data[lane][1];
        av = L.a.data[lane][2];
        as = L.a.joint_scales[lane];
    }
    int nfr = L.a.n_frontier, ndec = L.a.n_decoding;
    Frontier<NS> F;
#pragma unroll
    for (int r = 0; r < NS; r++) {
        const int d = lane + 64 * r;
        const bool ok = d < g.nd;
        F.st[r] = 0;
        F.added[r] = 0;
        F.neg[r] = 0.0f;
        F.x[r] = F.y[r] = F.s[r] = F.v[r] = 0.0f;
        F.sj[r] = ok ? g.d_j[d] : 0;
        F.sk[r] = ok ? g.d_k[d] : 0;
        F.scaf[r] = ok ? g.d_caf[d] : 0;
        F.sfwd[r] = ok ? g.d_fwd[d] : 0;
        F.pc[r] = 0;
        F.px[r] = F.py[r] = F.ps[r] = F.pv[r] = 0.0f;
    }
    const bool maxm = g.cfg.connection_method == 1;
    SlotSets<NS> ss{};
    if (AHEAD) ss = slot_sets<NS>(g, cs);
    auto ahead = [&](const uint64_t (&added)[NS]) {
        const uint64_t a1 = NS == 2 ? added[NS - 1] : 0ull;
        if (!AHEAD || !(added[0] | a1)) return;
        FSTAMP_BEGIN
        if (maxm)
            eval_ahead<true>(g, F, img, cs, ss, added[0], a1, ax, ay, av, as, L);
        else
            eval_ahead<false>(g, F, img, cs, ss, added[0], a1, ax, ay, av, as, L);
        FSTAMP_END(L, 1)
    };
    // `pub` (the seed loop): every joint the annotation holds, as (x, y, v, scale) in LDS as
    // soon as it is set, and its bit in *pub_mask -- a grow in flight shows the helpers'
    // plans which seeds its person's occupancy will cover (joints never change once set)
    if (pub) {
        if (lane < K && av > 0.0f) pub[lane] = make_float4(ax, ay, av, as);
        const uint32_t m0 = (uint32_t)__ballot(lane < K && av > 0.0f);
        if (lane == 0) __hip_atomic_store(pub_mask, m0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    for (int j = 0; j < K; j++) {  // seeding the frontier (cifcaf.py:288-291)
        const float vj = rl_f(av, j);
        if (vj == 0.0f) continue;
        uint64_t added[NS];
        add_to_frontier<CS>(g, L, F, av, j, vj, nfr, added);
        ahead(added);
    }
    for (;;) {
        if (abort && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
            break;
        // frontier_get (cifcaf.py:265-285)
        Entry got;
        bool have = false;
        Entry e;
        for (;;) {
            bool popped;
            {
                FSTAMP_BEGIN
                popped = frontier_pop(F, e);
                FSTAMP_END(L, 0)
            }
            if (!popped) break;
            if (e.eval) {
                got = e;
                have = true;
                break;
            }
            if (rl_f(av, e.k) > 0.0f) continue;
            float nx[4];
            if (AHEAD && e.pc) {  // computed ahead when joint e.j entered
                nx[0] = e.px;
                nx[1] = e.py;
                nx[2] = e.ps;
                nx[3] = e.pv;
            } else {
                STAMP_DO(if (lane == 0) L.fst[3] += 1);
                FSTAMP_BEGIN
                connection_value(g, img, set, e.caf, e.fwd, rl_f(ax, e.j), rl_f(ay, e.j),
                                 rl_f(av, e.j), rl_f(as, e.j), reverse_match, nx, ext);
                FSTAMP_END(L, 1)
            }
            if (nx[3] == 0.0f) continue;
            e.eval = 1;
            // score *= confidence_scales[caf_i] (cifcaf.py:282-284; not on the greedy return)
            e.neg = CS ? -(nx[3] * g.slot_cs[e.slot]) : -nx[3];
            e.x = nx[0];
            e.y = nx[1];
            e.s = nx[2];
            e.v = nx[3];
            if (g.cfg.greedy) {
                got = e;
                have = true;
                break;
            }
            const int sl = e.slot & 63, sr = e.slot >> 6;  // re-push into the edge's slot
            if (lane == sl) {
#pragma unroll
                for (int r = 0; r < NS; r++) {
                    if (r != sr) continue;
                    F.st[r] = 2;
                    F.neg[r] = e.neg;
                    F.x[r] = e.x;
                    F.y[r] = e.y;
                    F.s[r] = e.s;
                    F.v[r] = e.v;
                }
            }
        }
        if (!have) break;
        const int jsi = got.j, jti = got.k;
        if (rl_f(av, jti) > 0.0f) continue;
        if (lane == jti) {  // ann.data[jti] = (x, y, score); joint_scales[jti] = s
            ax = got.x;
            ay = got.y;
            av = got.v;
            as = got.s;
            if (pub) pub[jti] = make_float4(got.x, got.y, got.v, got.s);
        }
        if (pub && lane == 0)
            __hip_atomic_fetch_or(pub_mask, 1u << jti, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (lane == 0) {
            if (ndec < kKP) {
                L.a.decoding_pairs[ndec][0] = (uint8_t)jsi;
                L.a.decoding_pairs[ndec][1] = (uint8_t)jti;
                L.a.decoding_xyv[ndec][0] = rl_f(ax, jsi);
                L.a.decoding_xyv[ndec][1] = rl_f(ay, jsi);
                L.a.decoding_xyv[ndec][2] = rl_f(av, jsi);
                L.a.decoding_xyv[ndec][3] = got.x;
                L.a.decoding_xyv[ndec][4] = got.y;
                L.a.decoding_xyv[ndec][5] = got.v;
            } else {
                L.status |= PP_ST_DEC_OVERFLOW;
            }
        }
        ndec++;
        uint64_t added[NS];
        {
            FSTAMP_BEGIN
            add_to_frontier<CS>(g, L, F, av, jti, got.v, nfr, added);
            FSTAMP_END(L, 2)
        }
        ahead(added);
    }
    if (nfr > PP_MAX_FRONTIER && lane == 0) L.status |= PP_ST_DEC_OVERFLOW;
    if (lane < K) {
        L.a.data[lane][0] = ax;
        L.a.data[lane][1] = ay;
        L.a.data[lane][2] = av;
        L.a.joint_scales[lane] = as;
    }
    if (lane == 0) {
        L.a.n_frontier = nfr;
        L.a.n_decoding = ndec;
    }
    wave_sync();
}

// Mark the boxes of every joint j with mark(j) in one pass: joints live on different
// occupancy planes, so the per-joint `+= 1` boxes are independent and spread over the 64
// lanes.  Each marked box is logged for occ_clear.  Collective (all 64 lanes).
// lane j < K holds joint j: (jx, jy), scale js, `on` = mark it
template <typename LDS>
__device__ __forceinline__ void occ_mark(const GrowArgs &g, LDS &L, OccLog *log, const OccGrid &o,
                                         float jx, float jy, float js, bool on, int K) {
    const int lane = threadIdx.x & 63;
    int box[4] = {0, 0, 0, 0};
    bool has = false;
    if (lane < K && on) has = occ_box(g, o, lane, jx, jy, js, box);
    // work items: (row, 16-byte chunk) pairs of the box
    const int area = has ? (box[3] - box[2]) * (((box[1] - 1) >> 4) - (box[0] >> 4) + 1) : 0;
    int pre = 0, total = 0;
    for (int i = 0; i < K; i++) {  // exclusive prefix of the box areas (uniform loop)
        const int ai = rl_i(area, i);
        pre += (i < lane) ? ai : 0;
        total += ai;
    }
    const uint64_t hm = __ballot(has);
    if (lane < K) {
        L.mark_pre[lane] = pre;
        L.mark_box[lane][0] = box[0];
        L.mark_box[lane][1] = box[1];
        L.mark_box[lane][2] = box[2];
        L.mark_box[lane][3] = box[3];
        if (has) {
            const int li = L.log_n + lane_prefix(hm);
            if (li < g.log_cap) {
                OccLog e;
                e.f = lane;
                e.x0 = (int16_t)box[0];
                e.x1 = (int16_t)box[1];
                e.y0 = (int16_t)box[2];
                e.y1 = (int16_t)box[3];
                log[li] = e;
            }
        }
    }
    wave_sync();
    // Within one call every chunk is updated by one lane only (one box per joint plane,
    // rows padded to whole chunks), so a batch of chunks is loaded before any is stored.
    // u8 += 1 with wrap on the bytes inside the box: ((v & 0x7f..) + inc) ^ (v & 0x80..).
    constexpr int kB = 4;
    for (int t0 = 0; t0 < total; t0 += 64 * kB) {
        uint4 *cell[kB];
        uint4 inc[kB], val[kB];
#pragma unroll
        for (int u = 0; u < kB; u++) {
            const int t = t0 + u * 64 + lane;
            cell[u] = nullptr;
            inc[u] = make_uint4(0, 0, 0, 0);
            if (t < total) {
                int lo = 0, hi = K - 1;  // largest joint whose item prefix <= t
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (L.mark_pre[mid] <= t)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                const int r = t - L.mark_pre[lo];
                const int x0 = L.mark_box[lo][0], x1 = L.mark_box[lo][1];
                const int c0 = x0 >> 4, nch = ((x1 - 1) >> 4) - c0 + 1;
                const int yy = L.mark_box[lo][2] + r / nch, cx = (c0 + r % nch) << 4;
                cell[u] = reinterpret_cast<uint4 *>(&o.p[((int64_t)lo * o.h + yy) * o.pitch + cx]);
                uint32_t w4[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    uint32_t m = 0;
#pragma unroll
                    for (int bq = 0; bq < 4; bq++) {
                        const int x = cx + 4 * q + bq;
                        m |= (x >= x0 && x < x1) ? (1u << (8 * bq)) : 0u;
                    }
                    w4[q] = m;
                }
                inc[u] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
            }
        }
#pragma unroll
        for (int u = 0; u < kB; u++) val[u] = cell[u] ? *cell[u] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < kB; u++) {
            if (!cell[u]) continue;
            const uint4 v = val[u], m = inc[u];
            *cell[u] = make_uint4(((v.x & 0x7F7F7F7Fu) + m.x) ^ (v.x & 0x80808080u),
                                  ((v.y & 0x7F7F7F7Fu) + m.y) ^ (v.y & 0x80808080u),
                                  ((v.z & 0x7F7F7F7Fu) + m.z) ^ (v.z & 0x80808080u),
                                  ((v.w & 0x7F7F7F7Fu) + m.w) ^ (v.w & 0x80808080u));
        }
    }
    const int nm = __popcll(hm);
    if (L.log_n + nm > g.log_cap) L.status |= PP_ST_NMS_OVERFLOW;
    wave_sync();
    L.log_n = L.log_n + nm;
    wave_sync();
}

// zero every box the launch marked, so the next launch starts from a clean grid
template <typename LDS>
__device__ __forceinline__ void occ_clear(const GrowArgs &g, LDS &L, OccLog *log, const OccGrid &o) {
    wave_sync();
    const int n = L.log_n < g.log_cap ? L.log_n : g.log_cap;
    const int lane = threadIdx.x & 63;
    for (int e0 = 0; e0 < n; e0 += 64) {  // 64 boxes per round, one per lane
        const int e = e0 + lane;
        OccLog l{0, 0, 0, 0, 0};
        if (e < n) l = log[e];
        // bytes outside the marked boxes are zero already: clear whole chunks
        const int c0 = l.x0 >> 4, nch = (e < n) ? ((l.x1 - 1) >> 4) - c0 + 1 : 0;
        const int items = (e < n) ? nch * (l.y1 - l.y0) : 0;
        for (int t = 0; t < items; t++) {
            uint8_t *c = &o.p[((int64_t)l.f * o.h + l.y0 + t / nch) * o.pitch + ((c0 + t % nch) << 4)];
            *reinterpret_cast<uint4 *>(c) = make_uint4(0, 0, 0, 0);
        }
    }
    L.log_n = 0;
    wave_sync();
}

}  // namespace pp

// grow_columns.hpp — small set-A column sets read flat (from global memory or the seed
// loop's LDS stage) and the connections of a joint's new frontier entries evaluated ahead
// of their pops from them.  grow.hpp has the overview.
#pragma once

#include "grow_connection.hpp"
#include "grow_frontier.hpp"

namespace pp {

// ---------------------------------------------------------------------------------------
// connection_value ahead of the pop, several edges per memory round trip (seed loop)
// ---------------------------------------------------------------------------------------
// An unevaluated frontier entry (j, k) is evaluated when popped (cifcaf.py:275-279), but
// its connection_value depends only on the CAF columns and on joint j, which never changes
// once set.  So when joint j enters the frontier, the connections of all its new entries
// are computed at once: up to kAhead edges, the column rows of both directions of all of
// them loaded in ONE round trip (flat scan of small set-A column sets, <= kFlatCols
// columns, count from LDS), instead of two dependent round trips (bucket offsets, then
// columns) per edge and direction.  The pop then takes the stored result; the frontier order, the
// evaluation results and everything the reference observes are unchanged.  Edges whose
// sets are larger stay lazy (grow_connection over the buckets).
// edges per batch: 1 since the sets come from LDS (2 batched the HBM round trips; with
// LDS the extra registers only added spills: 1.006 -> 0.979 ms per overlapped step)
constexpr int kAhead = 1;
constexpr int kFlatPer = 2;
constexpr int kFlatCols = 64 * kFlatPer;

__device__ __forceinline__ void flat_load(const float *__restrict__ cf, int64_t hw, int n,
                                          float v[kFlatPer][kColRows]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int p = 0; p < kFlatPer; p++) {
        const int k = p * 64 + lane;
#pragma unroll
        for (int r = 0; r < kColRows; r++) v[p][r] = (k < n) ? cf[r * hw + k] : 0.0f;
    }
}

// Set-A column sets staged in LDS by the seed loop: every small set (<= kFlatCols columns)
// that fits the kernel's stage (kColLds / kColLdsExt floats), in (CAF, direction) order, column-major (kColPad floats per
// column: two 16-byte reads).  cofs[q] = its offset, -1 = global.
constexpr int kColPad = 8;
struct ColStage {
    const int *ncol;   // set-A column counts per (CAF, direction)
    const int *cofs;
    const float *lds;
};

// the same from the LDS copy of the set (offset `lo`, -1 = not staged)
__device__ __forceinline__ void flat_load_set(const float *__restrict__ cf, int64_t hw, int n,
                                              const float *lds, int lo,
                                              float v[kFlatPer][kColRows]) {
    if (lo < 0) {
        flat_load(cf, hw, n, v);
        return;
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int p = 0; p < kFlatPer; p++) {
        const int k = p * 64 + lane;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (k < n) {
            const float4 *c = reinterpret_cast<const float4 *>(lds + lo + k * kColPad);
            a = c[0];
            b = c[1];
        }
        v[p][0] = a.x;
        v[p][1] = a.y;
        v[p][2] = a.z;
        v[p][3] = a.w;
        v[p][4] = b.x;
        v[p][5] = b.y;
        v[p][6] = b.z;
    }
}

// per directed-edge slot (one per lane and half, like the Frontier): both directions' set
// sizes and LDS offsets packed as (count << 16) | (offset + 1), and whether both are small
template <int NS>
struct SlotSets {
    int f[NS], b[NS];
    uint64_t small[NS];
};

template <int NS>
__device__ __forceinline__ SlotSets<NS> slot_sets(const GrowArgs &g, const ColStage &cs) {
    const int lane = threadIdx.x & 63;
    SlotSets<NS> t;
#pragma unroll
    for (int r = 0; r < NS; r++) {
        const int d = lane + 64 * r;
        int f = 0, b = 0;
        bool small = false;
        if (d < g.nd) {
            const int caf = g.d_caf[d], df = g.d_fwd[d] ? 1 : 0;
            const int qf = caf * 2 + df, qb = caf * 2 + 1 - df;
            const int nf = cs.ncol[qf], nb = cs.ncol[qb];
            small = nf <= kFlatCols && nb <= kFlatCols;
            f = (nf << 16) | (cs.cofs[qf] + 1);
            b = (nb << 16) | (cs.cofs[qb] + 1);
        }
        t.f[r] = f;
        t.b[r] = b;
        t.small[r] = __ballot(small);
    }
    return t;
}

// grow_connection over every column of a flat-loaded set (same columns pass caf_center_s
// as through the buckets; the merge is independent of visiting order: unique keys)
template <bool MAXM>
__device__ __forceinline__ void flat_query(const float v[kFlatPer][kColRows], int n, float x, float y,
                                           float xy_scale, int exp_mode, float out[4]) {
    const int lane = threadIdx.x & 63;
    const ColQuery q = make_query(x, y, xy_scale, exp_mode);
    Top2 t = top2_empty();
#pragma unroll
    for (int p = 0; p < kFlatPer; p++)
        if (p * 64 + lane < n)
            consider_vals<MAXM>(q, v[p][0], v[p][1], v[p][2], v[p][3], v[p][4], v[p][5],
                                __float_as_int(v[p][6]), t);
    finish_connection<MAXM>(t, out);
}

// the new entries `added` (slot masks, add_to_frontier) of a start joint: connection_value
// with reverse_match (cifcaf.py:194-217) for those whose two column sets are small
// (r1: the slots from 64 on, always 0 with one slot per lane)
template <bool MAXM, int NS, typename LDS>
__device__ __forceinline__ void eval_ahead(const GrowArgs &g, Frontier<NS> &F, int img,
                                           const ColStage &cs, const SlotSets<NS> &ss, uint64_t r0,
                                           uint64_t r1, float ax, float ay, float av, float as,
                                           LDS &L) {
    const int lane = threadIdx.x & 63;
    const int64_t hw = g.col_cap;
    r0 &= ss.small[0];  // the others stay lazy
    if constexpr (NS == 2)
        r1 &= ss.small[1];
    else
        r1 = 0;
    while (r0 | r1) {
        STAMP_T0(et);
        int sl[kAhead];
#pragma unroll
        for (int b = 0; b < kAhead; b++) {  // the next kAhead slots
            sl[b] = -1;
            if (r0) {
                sl[b] = __ffsll((unsigned long long)r0) - 1;
                r0 &= r0 - 1;
            } else if (r1) {
                sl[b] = 64 + __ffsll((unsigned long long)r1) - 1;
                r1 &= r1 - 1;
            }
        }
        // both directions' columns of every edge at once: the reverse query's set is known
        // before the forward result (only its start point is not)
        float vf[kAhead][kFlatPer][kColRows], vb[kAhead][kFlatPer][kColRows];
        int nf[kAhead], nb[kAhead], jj[kAhead];
#pragma unroll
        for (int b = 0; b < kAhead; b++) {
            if (sl[b] < 0) continue;
            const int d = sl[b], l = d & 63;
            const bool h = NS == 2 && d >= 64;
            const int pf = rl_i(PP_SLOT(ss.f, h), l), pb = rl_i(PP_SLOT(ss.b, h), l);
            const int caf = rl_i(PP_SLOT(F.scaf, h), l);
            const int df = rl_i(PP_SLOT(F.sfwd, h), l) ? 1 : 0;
            jj[b] = rl_i(PP_SLOT(F.sj, h), l);
            nf[b] = pf >> 16;
            nb[b] = pb >> 16;
            flat_load_set(col_set(g, 0, img, caf, df), hw, nf[b], cs.lds, (pf & 0xFFFF) - 1, vf[b]);
            flat_load_set(col_set(g, 0, img, caf, 1 - df), hw, nb[b], cs.lds, (pb & 0xFFFF) - 1,
                          vb[b]);
        }
        STAMP_DO(asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"));
        ESTAMP(L, 6, et);
#pragma unroll
        for (int b = 0; b < kAhead; b++) {
            if (sl[b] < 0) continue;
            const int d = sl[b], j = jj[b];
            const float jx = rl_f(ax, j), jy = rl_f(ay, j), jv = rl_f(av, j), js = rl_f(as, j);
            float nx[4];
            flat_query<MAXM>(vf[b], nf[b], jx, jy, max0(js), g.cfg.exp_mode, nx);
            ESTAMP(L, 7, et);
            float res[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const float ks = sqrtf(nx[3] * jv);
            if (!(ks < g.cfg.keypoint_threshold) && nx[3] != 0.0f) {
                // reverse query from the new point (cifcaf.py:210-214)
                float rv[4];
                flat_query<MAXM>(vb[b], nb[b], nx[0], nx[1], max0(nx[2]), g.cfg.exp_mode, rv);
                if (rv[2] != 0.0f && !(fabsf(jx - rv[0]) + fabsf(jy - rv[1]) > max0(js))) {
                    res[0] = nx[0];
                    res[1] = nx[1];
                    res[2] = nx[2];
                    res[3] = ks;
                }
            }
            if (lane == (d & 63)) {
                if (NS == 1 || d < 64) {
                    F.pc[0] = 1;
                    F.px[0] = res[0];
                    F.py[0] = res[1];
                    F.ps[0] = res[2];
                    F.pv[0] = res[3];
                } else if constexpr (NS == 2) {
                    F.pc[1] = 1;
                    F.px[1] = res[0];
                    F.py[1] = res[1];
                    F.ps[1] = res[2];
                    F.pv[1] = res[3];
                }
            }
        }
    }
}

}  // namespace pp

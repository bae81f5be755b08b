// grow_frontier.hpp — the frontier of a grow (cifcaf.py:248 PriorityQueue) in a wave's
// registers.  grow.hpp has the overview.
#pragma once

#include "grow_device.hpp"

namespace pp {

// ---------------------------------------------------------------------------------------
// the frontier in registers: lane l holds directed-edge slots l and, with NS == 2, l + 64
// ---------------------------------------------------------------------------------------
// NS slots per lane: 1 for a skeleton of at most 64 directed edges (COCO has 38), where the
// second slot would always stay empty, else 2 (up to 128 directed edges).  The one-slot form
// is the two-slot form with every `r == 1` term folded away: the same pops in the same
// order, without slot 1's selects, its second ds_bpermute and ballot per add_to_frontier and
// its 17 live registers.
template <int NS>
struct Frontier {
    int st[NS];         // 0 empty, 1 (-max_possible, None, j, k), 2 (-score, xysv, j, k)
    float neg[NS];
    float x[NS], y[NS], s[NS], v[NS];
    int added[NS];      // in_frontier (cifcaf.py:249)
    int sj[NS], sk[NS], scaf[NS], sfwd[NS];  // slot constants
    // connection_value of an unevaluated entry computed ahead of its pop (eval_ahead)
    int pc[NS];
    float px[NS], py[NS], ps[NS], pv[NS];
};

// slot `w ? 1 : 0` of a per-slot array, as a select (not a[w]: a dynamic index sends the
// frontier to scratch); with one slot there is nothing to select.  (A macro: through an
// inlined function the two-slot kernels came out with 11 more VGPRs.)
#define PP_SLOT(a, w) (NS == 2 ? ((w) ? (a)[NS - 1] : (a)[0]) : (a)[0])

struct Entry {
    int slot, eval, j, k, caf, fwd, pc;
    float neg, x, y, s, v;
    float px, py, ps, pv;
};

// tuple order of (neg, None | (x, y, s, v), j, k); a None/tuple tie would raise TypeError
// in the reference (never happens in a successful run): unevaluated first here
__device__ __forceinline__ bool entry_less(float na, int ea, float xa, float ya, float sa,
                                           float va, int ja, int ka, float nb, int eb, float xb,
                                           float yb, float sb, float vb, int jb, int kb) {
    if (na != nb) return na < nb;
    if (ea != eb) return ea < eb;
    if (ea) {
        if (xa != xb) return xa < xb;
        if (ya != yb) return ya < yb;
        if (sa != sb) return sa < sb;
        if (va != vb) return va < vb;
    }
    if (ja != jb) return ja < jb;
    return ka < kb;
}

template <int NS>
__device__ __forceinline__ bool slot_less(const Frontier<NS> &F, int a, int b) {
    return entry_less(F.neg[a], F.st[a] == 2, F.x[a], F.y[a], F.s[a], F.v[a], F.sj[a], F.sk[a],
                      F.neg[b], F.st[b] == 2, F.x[b], F.y[b], F.s[b], F.v[b], F.sj[b], F.sk[b]);
}

// PriorityQueue.get(): remove and return the smallest live entry (false when empty)
template <int NS>
__device__ __forceinline__ bool frontier_pop(Frontier<NS> &F, Entry &e) {
    const int lane = threadIdx.x & 63;
    int lb = -1;
    if (F.st[0]) lb = 0;
    if constexpr (NS == 2)
        if (F.st[1] && (lb < 0 || slot_less(F, 1, 0))) lb = 1;
    const uint64_t live = __ballot(lb >= 0);
    if (live == 0) return false;
    const bool w1 = lb == 1;
    const float myneg = lb >= 0 ? PP_SLOT(F.neg, w1) : INFINITY;
    const float mn = wave_fmin(myneg);
    uint64_t cand = __ballot(lb >= 0 && myneg == mn);
    if (cand == 0) cand = live;  // only NaN scores left
    int win = __ffsll((unsigned long long)cand) - 1;
    const float my_x = PP_SLOT(F.x, w1), my_y = PP_SLOT(F.y, w1);
    const float my_s = PP_SLOT(F.s, w1), my_v = PP_SLOT(F.v, w1);
    const int my_e = PP_SLOT(F.st, w1) == 2, my_j = PP_SLOT(F.sj, w1);
    const int my_k = PP_SLOT(F.sk, w1);
    if (__popcll(cand) > 1) {  // exact score tie: full tuple comparison (rare)
        uint64_t rest = cand & (cand - 1);
        while (rest) {
            const int c = __ffsll((unsigned long long)rest) - 1;
            rest &= rest - 1;
            if (entry_less(rl_f(myneg, c), rl_i(my_e, c), rl_f(my_x, c), rl_f(my_y, c),
                           rl_f(my_s, c), rl_f(my_v, c), rl_i(my_j, c), rl_i(my_k, c),
                           rl_f(myneg, win), rl_i(my_e, win), rl_f(my_x, win), rl_f(my_y, win),
                           rl_f(my_s, win), rl_f(my_v, win), rl_i(my_j, win), rl_i(my_k, win)))
                win = c;
        }
    }
    const int wr = NS == 2 ? rl_i(w1 ? 1 : 0, win) : 0;
    e.slot = win + 64 * wr;
    e.neg = rl_f(myneg, win);
    e.eval = rl_i(my_e, win);
    e.x = rl_f(my_x, win);
    e.y = rl_f(my_y, win);
    e.s = rl_f(my_s, win);
    e.v = rl_f(my_v, win);
    e.j = rl_i(my_j, win);
    e.k = rl_i(my_k, win);
    e.caf = rl_i(PP_SLOT(F.scaf, wr), win);
    e.fwd = rl_i(PP_SLOT(F.sfwd, wr), win);
    e.pc = rl_i(PP_SLOT(F.pc, wr), win);
    e.px = rl_f(PP_SLOT(F.px, wr), win);
    e.py = rl_f(PP_SLOT(F.py, wr), win);
    e.ps = rl_f(PP_SLOT(F.ps, wr), win);
    e.pv = rl_f(PP_SLOT(F.pv, wr), win);
    if (lane == win) {
        if constexpr (NS == 2) {
            if (wr)
                F.st[1] = 0;
            else
                F.st[0] = 0;
        } else {
            F.st[0] = 0;
        }
    }
    return true;
}

// add_to_frontier (cifcaf.py:251-263): the start joint's slots in dict order, one pass
template <bool CS, int NS, typename LDS>
__device__ __forceinline__ void add_to_frontier(const GrowArgs &g, LDS &L, Frontier<NS> &F, float av,
                                                int start, float start_v, int &nfr,
                                                uint64_t (&added)[NS]) {
    const int lane = threadIdx.x & 63;
    const int lo = g.j_off[start], hi = g.j_off[start + 1];
    const float neg = -sqrtf(start_v);
#pragma unroll
    for (int r = 0; r < NS; r++) {
        const int d = lane + 64 * r;
        const float tv = __shfl(av, F.sk[r]);  // target joint's v (all lanes shuffle)
        const bool elig = d >= lo && d < hi && !(tv > 0.0f) && !F.added[r];
        const uint64_t m = __ballot(elig);
        if (elig) {
            F.st[r] = 1;
            // max_possible_score *= confidence_scales[caf_i] (cifcaf.py:258-261)
            F.neg[r] = CS ? -(sqrtf(start_v) * g.slot_cs[d]) : neg;
            F.added[r] = 1;
            const int t = nfr + lane_prefix(m);
            if (t < PP_MAX_FRONTIER) {
                L.a.frontier_pairs[t][0] = (uint8_t)start;
                L.a.frontier_pairs[t][1] = (uint8_t)F.sk[r];
            }
        }
        nfr += __popcll(m);
        added[r] = m;
    }
}

}  // namespace pp

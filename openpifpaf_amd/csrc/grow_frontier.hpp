// grow_frontier.hpp — the frontier of a grow (cifcaf.py:248 PriorityQueue) in a wave's
// registers.  grow.hpp has the overview.
#pragma once

#include "grow_device.hpp"

namespace pp {

// ---------------------------------------------------------------------------------------
// the frontier in registers: lane l holds directed-edge slots l and l + 64
// ---------------------------------------------------------------------------------------
struct Frontier {
    int st[2];         // 0 empty, 1 (-max_possible, None, j, k), 2 (-score, xysv, j, k)
    float neg[2];
    float x[2], y[2], s[2], v[2];
    int added[2];      // in_frontier (cifcaf.py:249)
    int sj[2], sk[2], scaf[2], sfwd[2];  // slot constants
    // connection_value of an unevaluated entry computed ahead of its pop (eval_ahead)
    int pc[2];
    float px[2], py[2], ps[2], pv[2];
};

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

__device__ __forceinline__ bool slot_less(const Frontier &F, int a, int b) {
    return entry_less(F.neg[a], F.st[a] == 2, F.x[a], F.y[a], F.s[a], F.v[a], F.sj[a], F.sk[a],
                      F.neg[b], F.st[b] == 2, F.x[b], F.y[b], F.s[b], F.v[b], F.sj[b], F.sk[b]);
}

// PriorityQueue.get(): remove and return the smallest live entry (false when empty)
__device__ __forceinline__ bool frontier_pop(Frontier &F, Entry &e) {
    const int lane = threadIdx.x & 63;
    int lb = -1;
    if (F.st[0]) lb = 0;
    if (F.st[1] && (lb < 0 || slot_less(F, 1, 0))) lb = 1;
    const uint64_t live = __ballot(lb >= 0);
    if (live == 0) return false;
    const bool w1 = lb == 1;  // selects, not F.x[w]: a dynamic index sends F to scratch
    const float myneg = lb >= 0 ? (w1 ? F.neg[1] : F.neg[0]) : INFINITY;
    const float mn = wave_fmin(myneg);
    uint64_t cand = __ballot(lb >= 0 && myneg == mn);
    if (cand == 0) cand = live;  // only NaN scores left
    int win = __ffsll((unsigned long long)cand) - 1;
    const float my_x = w1 ? F.x[1] : F.x[0], my_y = w1 ? F.y[1] : F.y[0];
    const float my_s = w1 ? F.s[1] : F.s[0], my_v = w1 ? F.v[1] : F.v[0];
    const int my_e = (w1 ? F.st[1] : F.st[0]) == 2, my_j = w1 ? F.sj[1] : F.sj[0];
    const int my_k = w1 ? F.sk[1] : F.sk[0];
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
    const int wr = rl_i(w1 ? 1 : 0, win);
    e.slot = win + 64 * wr;
    e.neg = rl_f(myneg, win);
    e.eval = rl_i(my_e, win);
    e.x = rl_f(my_x, win);
    e.y = rl_f(my_y, win);
    e.s = rl_f(my_s, win);
    e.v = rl_f(my_v, win);
    e.j = rl_i(my_j, win);
    e.k = rl_i(my_k, win);
    e.caf = rl_i(wr ? F.scaf[1] : F.scaf[0], win);
    e.fwd = rl_i(wr ? F.sfwd[1] : F.sfwd[0], win);
    e.pc = rl_i(wr ? F.pc[1] : F.pc[0], win);
    e.px = rl_f(wr ? F.px[1] : F.px[0], win);
    e.py = rl_f(wr ? F.py[1] : F.py[0], win);
    e.ps = rl_f(wr ? F.ps[1] : F.ps[0], win);
    e.pv = rl_f(wr ? F.pv[1] : F.pv[0], win);
    if (lane == win) {
        if (wr)
            F.st[1] = 0;
        else
            F.st[0] = 0;
    }
    return true;
}

// add_to_frontier (cifcaf.py:251-263): the start joint's slots in dict order, one pass
template <bool CS, typename LDS>
__device__ __forceinline__ void add_to_frontier(const GrowArgs &g, LDS &L, Frontier &F, float av, int start,
                                float start_v, int &nfr, uint64_t added[2]) {
    const int lane = threadIdx.x & 63;
    const int lo = g.j_off[start], hi = g.j_off[start + 1];
    const float neg = -sqrtf(start_v);
#pragma unroll
    for (int r = 0; r < 2; r++) {
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

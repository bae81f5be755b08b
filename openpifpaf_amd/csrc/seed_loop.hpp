// seed_loop.hpp — what both seed-loop kernels use (seed_loop.hip: an image per workgroup;
// seed_loop_ext.hip: with helper workgroups on other CUs): the design, the per-seed
// occupancy counters, the workgroup's shared state and its handshake, and the pieces of the
// loop that are the same in both.
#pragma once

#include "grow.hpp"

namespace pp {

// ---------------------------------------------------------------------------------------
// seed loop (cifcaf.py:84-108): one workgroup of kSeedWaves waves per image
// ---------------------------------------------------------------------------------------
// The loop is sequential: whether a seed starts an annotation depends on the occupancy
// marks of every annotation before it.  But _grow from a seed is a pure function of the
// seed and the CAF columns, so helper waves grow seeds the loop is LIKELY to reach next
// while wave 0 grows the one it needs now; wave 0 then commits strictly in the reference
// order (the next free seed, cifcaf.py:100-104) and takes a seed's annotation from the
// cache when a helper grew it already.  Speculation only changes WHEN an annotation is
// computed, never which seeds start one or what they contain.
//
// Helpers pick free seeds after the committed one that lie far (kSpecFar joint scales,
// Chebyshev) from it, from each other and from the cached ones, since seeds near an
// annotation's joints are the ones its occupancy marks will cover.
//
// Nothing waits for the slowest wave: wave 0 hands a seed to each IDLE helper when it has
// to grow one itself, and a helper publishes its annotation (cache slot state 2) whenever
// it finishes.  Wave 0 waits on a helper only for the seed it needs next, if that helper
// is still growing it.  The handshake is LDS flags with workgroup-scope acquire/release.
//
// Both plans (spec_plan in seed_loop.hip, plan_round in seed_loop_ext.hip) exclude a seed
// only for annotations that come BEFORE it in seed order: near a
// seed in flight, inside the occupancy boxes of a grown annotation or of the joints an
// in-flight grow has set so far, when that annotation's seed precedes it (wave 0 commits it
// first, and its boxes then cover the seed).  An annotation whose seed comes after cannot
// cover it at its turn, so excluding it there only made wave 0 grow it itself (cfg5 planted
// 39.4k-40.2k -> 42.9k-43.7k, planted cfg3 406k-413k -> 415k-416k; round 6).
// Who plans the idle helpers when wave 0 has to grow a seed itself: an idle helper, so that
// wave 0 starts its grow at once and the plan (a scan of kSpecScan seeds against the cache,
// about 50k cycles, stamps) is off the committer's path (wave 0 planning before its grow
// measured no faster, round 5).  Wave 0 publishes its seed without the plan lock: a plan
// that misses it only grows a seed twice, which never changes a result.  A helper that
// finishes plans its own next grow (the external helpers of seed_loop_ext_kernel do not:
// cfg5 uniform 725 vs 1080 images/s with it, round 4), and a helper whose plan found
// nothing plans again once wave 0 has committed or passed a seed (idle_dec): a wave 0 that
// only takes cached annotations never misses, so never requests a plan.  Uniform cfg3
// (round 6, A/B on one box): the slot-register plan alone 15.2-15.3k images/s, with the
// re-plan 16.3-16.5k, the round-5 plan 15.7-15.9k.
// Grows in flight publish their joints as they are set (grow's `pub`), and the plans keep
// seeds their occupancy boxes will cover away from the helpers.  Planted cfg3 (stamps,
// serial): at kernel start about 4 of the 7 first picks are seeds the loop commits
// (tools/spec_sim.py).  (Helper waves at issue priority 2 measured no faster, round 5.)

// ---- the seed loop's occupancy as per-seed counters in LDS ----
// The seed loop reads its occupancy grid only at seed positions (cifcaf.py:100-102: the
// free-seed test; the helpers' plans), so for an image with at most kOccSeeds seeds the
// grid is replaced by one u8 counter per seed: a mark adds 1 (wrapping, as the grid's
// `+= 1`, utils.py:66) to every seed of the joint's field whose grid cell lies in the
// joint's box, and a seed is occupied iff its counter is nonzero -- exactly the grid's
// cell value there.  Marks and tests stay in LDS: no global read-modify-write, no clearing.
constexpr int kOccSeeds = 2560;
// Counters, cells and fields are stored by the seeds' position p in field-grouped order (pos:
// seed index -> p), so that a mark reads one seed's cell, field and counter in one LDS round
// trip, four seeds per lane at once, over all the marked joints' fields in one sweep.
struct SeedOcc {
    uint8_t cnt[kOccSeeds];     // counter per position
    uint8_t fld[kOccSeeds];     // field per position
    uint32_t cell[kOccSeeds];   // grid cell (yi << 16 | xi) per position
    uint16_t pos[kOccSeeds];    // position of each seed index
    int foff[kKP + 1];          // field f's positions: foff[f] .. foff[f + 1]
    int fcur[kKP];
    int n;
};

__device__ __forceinline__ bool seed_occupied(const SeedOcc &O, int idx) { return O.cnt[O.pos[idx]] != 0; }

// collective over the workgroup (ends with a barrier): the counters and field groups of
// the image's n <= kOccSeeds seeds
__device__ __forceinline__ void seed_occ_init(SeedOcc &O, const pp_seed *seeds, int n, int K,
                                              const OccGrid &o, float red) {
    if (threadIdx.x < kKP) O.fcur[threadIdx.x] = 0;
    if (threadIdx.x == 0) O.n = n;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&O.fcur[seeds[i].field], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int f = 0; f < K; f++) {
            O.foff[f] = a;
            a += O.fcur[f];
            O.fcur[f] = 0;
        }
        O.foff[K] = a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const pp_seed c = seeds[i];
        const int xi = (int)clip_ref(c.x / red, 0.0f, (float)(o.w - 1));  // occ_get's cell
        const int yi = (int)clip_ref(c.y / red, 0.0f, (float)(o.h - 1));
        const int p = O.foff[c.field] + atomicAdd(&O.fcur[c.field], 1);
        O.pos[i] = (uint16_t)p;
        O.cell[p] = ((uint32_t)yi << 16) | (uint32_t)xi;
        O.fld[p] = (uint8_t)c.field;
        O.cnt[p] = 0;
    }
    __syncthreads();
}

// occ_mark on the counters (one wave): lane j < K holds joint j (x, y, scale, `on`).  Each
// position is one seed of one field, so a sweep touches every counter at most once (no
// races between lanes); a seed whose field's joint is marked gets +1 if its cell is in the
// joint's box (the box from lane `field`, ds_bpermute).
__device__ __forceinline__ void seed_occ_mark(const GrowArgs &g, SeedOcc &O, const OccGrid &o,
                                              float jx, float jy, float js, bool on, int K) {
    const int lane = threadIdx.x & 63;
    int box[4] = {0, 0, 0, 0};
    const bool has = lane < K && on && occ_box(g, o, lane, jx, jy, js, box);
    const uint64_t hm = __ballot(has);
    if (hm) {
        const int n = O.n;
        constexpr int kU = 4;
        for (int p0 = 0; p0 < n; p0 += 64 * kU) {
            uint32_t c[kU];
            int f[kU], v[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int p = p0 + u * 64 + lane;
                const bool in = p < n;
                c[u] = in ? O.cell[p] : 0u;
                f[u] = in ? (int)O.fld[p] : 0;
                v[u] = in ? (int)O.cnt[p] : 0;
            }
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const int p = p0 + u * 64 + lane;
                const int x0 = __shfl(box[0], f[u]), x1 = __shfl(box[1], f[u]);
                const int y0 = __shfl(box[2], f[u]), y1 = __shfl(box[3], f[u]);
                const int xi = (int)(c[u] & 0xFFFFu), yi = (int)(c[u] >> 16);
                if (p < n && ((hm >> f[u]) & 1ull) && xi >= x0 && xi < x1 && yi >= y0 && yi < y1)
                    O.cnt[p] = (uint8_t)(v[u] + 1);
            }
        }
    }
    wave_sync();
}

template <int NSLOT>
struct SeedLoopSharedT {
    int task[kSeedWaves];          // seed a helper is to grow (-1 idle), set by wave 0
    int task_slot[kSeedWaves];     // cache slot its annotation goes to
    int cache_seed[NSLOT];         // seed index held by a cache slot (< current: dead)
    float cache_x[NSLOT], cache_y[NSLOT], cache_s[NSLOT];  // seed position
    // 0 free, 1 being grown, 2 grown (joints below valid), 4 zombie (external slot whose
    // seed wave 0 grew itself; free once its tag arrives); external slots' 1 -> 2 and
    // 4 -> 0 are wave 0's, on seeing the slot's tag
    int cache_state[NSLOT];
    float4 cache_j[kSpecCache][kKP];  // its joints (x, y, v, scale); the external slots'
                                      // after the column stage in dynamic LDS (cache_joints)
    // seed_loop_kernel: joints of a slot still being grown that are set already (bit j:
    // cache_j[q][j] holds joint j; grow's `pub`), and the same for wave 0's own grow
    uint32_t cache_pm[kSpecCache];
    float4 own_j[kKP];
    uint32_t own_pm;
    int done;
    // seed_loop_kernel's helper self-planning (spec_plan): the plan lock, the first seed not
    // yet decided by wave 0 (seeds before it were committed or skipped), and the seed wave 0
    // grows itself now (own_on)
    int plan_lock, decided, own_on;
    float own_x, own_y, own_s;
    // seed_loop_kernel: wave 0 started a grow of its own; an idle helper plans the others
    int plan_req;
};

// The occupancy box joint j of field f will mark once its annotation is committed
// (occ_box_r), packed x0 | x1 << 16, y0 | y1 << 16 (an empty box is 0, 0), for the plans'
// test of a seed's grid cell against a cache slot
__device__ __forceinline__ uint2 plan_box(float red, float msr, const OccGrid &o, int f, float4 j) {
    int box[4];
    if (j.z == 0.0f || !occ_box_r(red, msr, o, f, j.x, j.y, j.w, box)) return make_uint2(0u, 0u);
    return make_uint2((uint32_t)box[0] | ((uint32_t)box[1] << 16),
                      (uint32_t)box[2] | ((uint32_t)box[3] << 16));
}
__device__ __forceinline__ bool in_plan_box(uint2 b, int cx, int cy) {
    return cx >= (int)(b.x & 0xFFFFu) && cx < (int)(b.x >> 16) && cy >= (int)(b.y & 0xFFFFu) &&
           cy < (int)(b.y >> 16);
}

__device__ __forceinline__ int lds_acquire(int *p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_release(int *p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t lds_acquire_u(uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ bool spec_far(float far, float xa, float ya, float sa, float xb,
                                         float yb, float sb) {
    const float r = far * fmaxf(fmaxf(sa, sb), 1.0f);
    return fabsf(xa - xb) > r || fabsf(ya - yb) > r;
}

// Annotation(keypoints, out_skeleton).add(f, (x, y, v)); joint_scales[f] = s
template <typename LDS>
__device__ __forceinline__ void ann_from_seed(LDS &L, const pp_seed &sd, int K, int img) {
    const int lane = threadIdx.x & 63;
    uint32_t *z = reinterpret_cast<uint32_t *>(&L.a);
    for (int t = lane; t < (int)(sizeof(pp_ann) / 4); t += 64) z[t] = 0u;
    wave_sync();
    if (lane == 0) {
        L.a.n_keypoints = K;
        L.a.image = img;
        L.a.data[sd.field][0] = sd.x;
        L.a.data[sd.field][1] = sd.y;
        L.a.data[sd.field][2] = sd.v;
        L.a.joint_scales[sd.field] = sd.s;
    }
    wave_sync();
}

template <int NS>
__device__ __forceinline__ void plan_lock(SeedLoopSharedT<NS> &S) {
    if ((threadIdx.x & 63) == 0) {
        int expect = 0;
        while (!__hip_atomic_compare_exchange_strong(&S.plan_lock, &expect, 1, __ATOMIC_ACQUIRE,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
            expect = 0;
            __builtin_amdgcn_s_sleep(1);
        }
    }
    wave_sync();
}

template <int NS>
__device__ __forceinline__ void plan_unlock(SeedLoopSharedT<NS> &S) {
    wave_sync();
    if ((threadIdx.x & 63) == 0) lds_release(&S.plan_lock, 0);
}

// ---- pieces both seed-loop kernels share (force-inlined: each takes GrowArgs by
// reference, which a real call would copy to scratch) ----

// The image's small set-A column sets (<= kFlatCols columns, in (CAF, direction) order
// while they fit kColLds floats) into LDS, column-major, kColPad floats per column: their
// counts into s_ncol, LDS offsets into s_cofs (-1: read from global memory).  Every wave of
// the workgroup takes part; no barrier after the copy (the caller's init barrier follows).
__device__ __forceinline__ ColStage stage_small_sets(const GrowArgs &g, int img, int *s_ncol,
                                                     int *s_cofs, float *s_cols, int cap) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = threadIdx.x; q < 2 * g.C; q += blockDim.x) s_ncol[q] = col_offs(g, 0, img, q >> 1, q & 1)[g.nb];
    __syncthreads();
    if (threadIdx.x == 0) {  // LDS placement of the small sets, in order while they fit
        int o = 0;
        for (int q = 0; q < 2 * g.C; q++) {
            const int sz = kColPad * s_ncol[q];
            const bool fit = s_ncol[q] <= kFlatCols && o + sz <= cap;
            s_cofs[q] = fit ? o : -1;
            o += fit ? sz : 0;
        }
    }
    __syncthreads();
    for (int q = wave; q < 2 * g.C; q += kSeedWaves) {  // one set per wave
        const int n = s_ncol[q];
        if (s_cofs[q] < 0 || n == 0) continue;
        const float *cf = col_set(g, 0, img, q >> 1, q & 1);
        float *dst = s_cols + s_cofs[q];
        for (int k = lane; k < n; k += 64) {
            float c[kColRows];
#pragma unroll
            for (int r = 0; r < kColRows; r++) c[r] = cf[r * g.col_cap + k];
            float4 *o = reinterpret_cast<float4 *>(dst + k * kColPad);
            o[0] = make_float4(c[0], c[1], c[2], c[3]);
            o[1] = make_float4(c[4], c[5], c[6], 0.0f);
        }
    }
    return ColStage{s_ncol, s_cofs, s_cols};
}

// The next free seed from index s on (cifcaf.py:100-104), 64 occupancy tests per step (the
// per-seed LDS counters `socc`, or the global grid); -1 when none is left.  s advances past
// the all-occupied steps.  Wave 0.
__device__ __forceinline__ int next_free_seed(int &s, int n_seeds, const SeedOcc *socc,
                                              const pp_seed *seeds, const OccGrid &occ,
                                              float red) {
    const int lane = threadIdx.x & 63;
    while (s < n_seeds) {
        const int idx = s + lane;
        bool is_free = false;
        if (idx < n_seeds) {
            if (socc) {
                is_free = !seed_occupied(*socc, idx);
            } else {
                const pp_seed c = seeds[idx];
                is_free = !occ_get(occ, c.field, c.x, c.y, red);
            }
        }
        const uint64_t m = __ballot(is_free);
        if (m) return s + __ffsll((unsigned long long)m) - 1;
        s += 64;
    }
    return -1;
}

// Initial annotations (cifcaf.py:95-98): each is grown with set A and reverse matching from
// all its set joints (its decoding / frontier orders are appended to), then committed
// (appended and marked occupied, `commit(record)`), in order, before any seed is looked
// at.  Wave 0.
template <bool CS, int NS, typename Commit>
__device__ __forceinline__ void grow_initial(const GrowArgs &g, SeedLDS &L, int img,
                                             const ColStage &cstage, const int &n_anns,
                                             Commit commit) {
    const int lane = threadIdx.x & 63;
    const int n_init = g.init ? min(g.init_counts[img], g.init_cap) : 0;
    for (int i = 0; i < n_init; i++) {
        if (n_anns >= g.ann_cap) {
            if (lane == 0) L.status |= PP_ST_ANN_OVERFLOW;
            break;
        }
        copy_ann(&L.a, &g.init[(int64_t)img * g.init_cap + i]);
        if (lane == 0) {
            L.a.image = img;
            L.a.n_keypoints = g.K;
        }
        wave_sync();
        grow<true, CS, NS>(g, L, img, 0, true, cstage);
        commit(&L.a);
    }
}

// A helper wave's finished grow into this CU's cache slot q: the record (global memory),
// its joints (LDS), then the slot's state 2 (grown).  The record's global stores complete
// before the flag (the workgroup-scope release alone does not wait for them).
template <int NS>
__device__ __forceinline__ void publish_cached(SeedLoopSharedT<NS> &S, pp_ann *cache, int q,
                                               const SeedLDS &L) {
    const int lane = threadIdx.x & 63;
    copy_ann(&cache[q], &L.a);
    if (lane < kKP)
        S.cache_j[q][lane] = make_float4(L.a.data[lane][0], L.a.data[lane][1],
                                         L.a.data[lane][2], L.a.joint_scales[lane]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    if (lane == 0) lds_release(&S.cache_state[q], 2);
    wave_sync();
}

// The end of a seed loop (wave 0, after the barrier that drains the helpers): the image's
// occupancy marks cleared (the grid stays zero between launches), then its annotation
// count, the joints force-complete must fill, and the waves' status bits.
__device__ __forceinline__ void seed_loop_outputs(const GrowArgs &g, const SeedLDS *Ls, int img,
                                                  int n_anns, uint32_t unset_mask) {
    if ((threadIdx.x & 63) == 0) {
        int st = 0;
        for (int w = 0; w < kSeedWaves; w++) st |= Ls[w].status;
        g.n_work[img] = n_anns;
        g.need_complete[img] = g.cfg.force_complete ? (int)unset_mask : 0;
        g.status[img] = st;
    }
}

}  // namespace pp

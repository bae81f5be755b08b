// seed_loop_ext.hip — the seed loop of a batch of fewer images than CUs: each image's
// workgroup gets helper workgroups on other CUs (seed_loop_ext_kernel, its hand-off through
// global memory, its launcher).  seed_loop.hpp has the design both loops share.
#include "seed_loop.hpp"

namespace pp {

// seeds after the committed one that wave 0 of seed_loop_ext_kernel examines per plan round
// (cfg5 planted 42.9k-43.7k -> 45.8k-47.0k images/s with 512 instead of 128, round 6)
constexpr int kExtScan = 512;
// the external-helper plan's speculation distance (joint scales): 1 instead of kSpecFar's 4
// (cfg5 planted 45.5k-46.9k -> 50.3k-50.4k images/s, uniform 1513-1517 vs 1518-1527; with 1
// for the one-CU kernel too, planted cfg3 was 415k vs 415k-420k and uniform 16.1k-16.3k vs
// 16.0k; round 6, r06z_ab_spec_far.txt)
constexpr float kExtSpecFar = 1.0f;
// Wave 0 of seed_loop_ext_kernel plans the idle helpers when it has to grow a seed itself (a
// miss), and, on images of kExtRefillAnns annotations or more, also after a cached commit that
// leaves fewer than kExtRefill speculated seeds ahead: a dense image otherwise ran its helpers
// dry between misses (~77 of ~1370 seeds per cfg5 uniform image grown by wave 0 itself, each a
// whole grow on the critical path, r06h stamps).  cfg5 uniform 1510-1545 -> 1562-1737 images/s
// with 12 (8: 1616-1661, 16: no gain, 20: 1558-1576; planted unchanged from 32 annotations on,
// -2 % when refilling on every image; r06z_ab_refill.txt).
constexpr int kExtRefillAnns = 32;
constexpr int kExtRefill = 12;

// External helpers.  A batch of fewer images than CUs leaves CUs without a seed loop, so
// each image may get n_ext (<= kExtWgMax) more workgroups whose waves are all helpers.
// They take seeds from wave 0 through per-image global words (SeedExt) and publish into
// kExtCache more cache slots, whose records live in global memory, across CUs and XCDs
// with the agent-scope publish / consume form of cdna_hip_programming.md Guideline 16: the
// record is stored write-through (sc1) and drained (s_waitcnt vmcnt(0)) before one lane
// stores the slot's tag (seed + 1); wave 0 polls tags relaxed and reads records and joints
// with sc1 loads.  A helper announces itself (task word 1 = idle) before wave 0 may hand
// it a seed (CAS 1 -> assigned), so a workgroup that is not resident never holds one; an
// idle helper leaves when wave 0 finishes (fin) or after kExtIdleTicks without work (CAS
// 1 -> 3; losing that CAS to an assignment means: grow it).  The image's workgroups count
// themselves out (SeedExt.exited) after their last access to these words, and the last one
// out zeroes them, so every launch finds them zero whatever runs between two seed loops.
// Policy (s_memrealtime ticks, 100 MHz).  Wave 0 waits for an external slot it needs next
// only if that grow is at least half done by the running mean of external grows (at most
// 2 s: a helper always finishes); otherwise it grows the seed itself and the slot is a
// zombie (state 4) until its tag arrives.  An idle helper leaves after 300 us, so that on
// images with few annotations its CU goes back to the other stages' kernels; once an image
// has kExtHeavyAnns annotations wave 0 flags it heavy (SeedExt.heavy) and helpers stay up
// to 1 s idle.  cfg5 (64 images, 160x160; 16 / 1370 annotations per image), images/s,
// planted / uniform: no helpers 26.4k / 795; this 27.7k / 969; helpers that stay 1 ms idle
// 22.7k / 1024; wave 0 always waiting 22.5k / 1027; also handing out seeds after every 4th
// cached commit 21.7k / 986; a 100 us light idle and no wait before 32 annotations 27.0k / 907.
constexpr int kExtHeavyAnns = 8;
constexpr uint64_t kExtIdleLight = 30000ull, kExtIdleHeavy = 100000000ull;
constexpr uint64_t kExtWaitMax = 200000000ull;
// (Wave 0 planning the idle helpers while it waits for one, once per wait, when that grow is
// expected to run 40 us longer on images of 32+ annotations: cfg5 uniform 1445-1724 vs
// 1670 images/s without, planted 39.8-41.2k vs 40.4-43.5k, round 6.)

typedef __attribute__((address_space(1))) unsigned int gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;
__device__ __forceinline__ unsigned int ld_agent(const unsigned int *p) {
    return __hip_atomic_load((gu32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) {
    return __hip_atomic_load((gu64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned int *p, unsigned int v) {
    __hip_atomic_store((gu32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store((gu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool cas_agent(unsigned long long *p, unsigned long long expect,
                                          unsigned long long v) {
    return __hip_atomic_compare_exchange_strong((gu64 *)p, &expect, v, __ATOMIC_RELAXED,
                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// lane 0's CAS, its result on every lane
__device__ __forceinline__ bool cas_agent_wave(unsigned long long *p, unsigned long long expect,
                                               unsigned long long v) {
    int ok = 0;
    if ((threadIdx.x & 63) == 0) ok = cas_agent(p, expect, v) ? 1 : 0;
    return __builtin_amdgcn_readfirstlane(ok) != 0;
}

// One of an image's 1 + n_ext workgroups is done with its SeedExt words (called by every
// thread after a __syncthreads that follows the workgroup's last access to them): it counts
// itself out, and the last one out zeroes the words for the workspace's next seed loop.
// Every workgroup of the image runs (a helper that was not resident before wave 0 finished
// starts later, sees fin and leaves), so exactly one sees the count reach n_ext, after
// every other workgroup's last access.  The workspace contract (zero at each launch) then
// holds after any stage split (PP_STAGE_SEED_LOOP_ONLY with or without the NMS call).
__device__ __forceinline__ void ext_exit(SeedExt *X, int n_ext) {
    if (!X || threadIdx.x != 0) return;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    const unsigned int before = __hip_atomic_fetch_add((gu32 *)&X->exited, 1u, __ATOMIC_ACQ_REL,
                                                       __HIP_MEMORY_SCOPE_AGENT);
    if (before != (unsigned int)n_ext) return;
    unsigned int *w = reinterpret_cast<unsigned int *>(X);
    for (int t = 0; t < (int)(sizeof(SeedExt) / 4); t++) st_agent(w + t, 0u);
}

// an LDS record to global memory, write-through (sc1), drained
__device__ __forceinline__ void publish_ann(pp_ann *dst, const pp_ann *src) {
    const unsigned long long *s = reinterpret_cast<const unsigned long long *>(src);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
    constexpr int nw = sizeof(pp_ann) / 8;
    for (int t = threadIdx.x & 63; t < nw; t += 64) st_agent(d + t, s[t]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// copy_ann from another CU's published record (sc1 loads)
__device__ __forceinline__ void copy_ann_agent(pp_ann *dst, const pp_ann *src) {
    const unsigned long long *s = reinterpret_cast<const unsigned long long *>(src);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
    constexpr int nw = sizeof(pp_ann) / 8;
    constexpr int per = (nw + 63) / 64;
    const int lane = threadIdx.x & 63;
    unsigned long long v[per];
#pragma unroll
    for (int u = 0; u < per; u++) v[u] = (u * 64 + lane < nw) ? ld_agent(s + u * 64 + lane) : 0ull;
#pragma unroll
    for (int u = 0; u < per; u++)
        if (u * 64 + lane < nw) d[u * 64 + lane] = v[u];
    wave_sync();
}

// floats of the column stage (stage_small_sets) in dynamic LDS.  This kernel (images with
// helpers on other CUs, e.g. cfg5) stages 48 KB: the LDS it leaves lets the other batch's
// kernels share its CUs (cfg5 uniform 1452-1473 -> 1583-1585 images/s, planted 41.3k ->
// 43.1k-43.7k; 80 KB for the one-CU kernel, where 48 / 64 KB measured 1 % slower, A/B on
// one box)
constexpr int kColLdsExt = 12288;

struct SeedLoopSharedX : SeedLoopSharedT<kCacheSlots> {
    uint32_t cache_t[kCacheSlots];  // external slots: s_memrealtime (low bits) at hand-over
    uint32_t ext_ticks;             // running mean of hand-over -> tag seen (0: none yet)
};

// joints of cache slot q (LDS): this CU's slots in SeedLoopShared, the external ones in the
// dynamic LDS after the kColLdsExt column floats (launched only when n_ext > 0)
__device__ __forceinline__ float4 *cache_joints(SeedLoopSharedX &S, float *s_cols, int q) {
    return q < kSpecCache ? S.cache_j[q]
                          : reinterpret_cast<float4 *>(s_cols + kColLdsExt) + (q - kSpecCache) * kKP;
}
// The occupancy boxes a grown slot's joints will mark once committed (occ_box_r), for the
// plan of seed_loop_ext_kernel: written with the joints, before the slot's state 2, so a
// plan tests a seed against a slot with one LDS read.  Packed x0 | x1 << 16, y0 | y1 << 16;
// an empty box is 0, 0.  (An occupancy grid of 2^16 cells or more per side, reduction < 1,
// garbles them: that only changes which seeds the helpers grow ahead, never a result.)
// After the external joints in the dynamic LDS, one row of kKP per slot (all kCacheSlots).
constexpr size_t kExtDynLds = kColLdsExt * sizeof(float) + (size_t)kExtCache * kKP * sizeof(float4) +
                              (size_t)kCacheSlots * kKP * sizeof(uint2);
__device__ __forceinline__ uint2 *cache_boxes(float *s_cols, int q) {
    return reinterpret_cast<uint2 *>(reinterpret_cast<float4 *>(s_cols + kColLdsExt) + kExtCache * kKP) +
           q * kKP;
}

// wave 0: external slots being grown whose tag has arrived become grown (joints into LDS);
// `only` >= 0 restricts the check to that slot
__device__ __forceinline__ void ext_refresh(SeedLoopSharedX &S, float *s_cols, const SeedExt *X,
                                            const pp_ann *xrec, int only, float red, float msr,
                                            const OccGrid &occ) {
    const int lane = threadIdx.x & 63;
    const int q = kSpecCache + lane;
    bool ready = false;
    const int st = lane < kExtCache ? S.cache_state[q] : 0;
    if (lane < kExtCache && (only < 0 || only == q) && (st == 1 || st == 4))
        ready = ld_agent(&X->tag[lane]) == (unsigned int)S.cache_seed[q] + 1u;
    if (ready && st == 4) {  // the zombie's helper is done: free
        S.cache_state[q] = 0;
        ready = false;
    }
    wave_sync();
    const uint64_t rm = __ballot(ready);
    if (rm) {
        const uint32_t now = (uint32_t)__builtin_amdgcn_s_memrealtime();
        const uint32_t dur = ready ? now - S.cache_t[q] : 0u;
        uint32_t mt = S.ext_ticks;
        for (uint64_t b = rm; b; b &= b - 1) {
            const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)dur, __ffsll((unsigned long long)b) - 1);
            mt = mt ? 3u * (mt >> 2) + (d >> 2) : d;
        }
        wave_sync();
        if (lane == 0) S.ext_ticks = mt;
    }
    for (uint64_t m = rm; m; m &= m - 1) {
        const int e = __ffsll((unsigned long long)m) - 1;
        const pp_ann *r = xrec + e;
        if (lane < kKP) {
            const unsigned int *d = reinterpret_cast<const unsigned int *>(&r->data[lane][0]);
            const float4 j = make_float4(
                __uint_as_float(ld_agent(d)), __uint_as_float(ld_agent(d + 1)),
                __uint_as_float(ld_agent(d + 2)),
                __uint_as_float(ld_agent(reinterpret_cast<const unsigned int *>(&r->joint_scales[lane]))));
            cache_joints(S, s_cols, kSpecCache + e)[lane] = j;
            cache_boxes(s_cols, kSpecCache + e)[lane] = plan_box(red, msr, occ, lane, j);
        }
        wave_sync();
        if (lane == 0) S.cache_state[kSpecCache + e] = 2;
        wave_sync();
    }
}

// seed_loop_kernel's loop with external helpers (n_ext > 0).  A separate kernel: the
// big-batch one (seed_loop.hip) carries none of the hand-off state, whose registers cost it
// 4% per planted cfg3 step when merged into it (spills inside the grow).
// FS: frontier slots per lane (grow_frontier.hpp), 1 when the skeleton has at most 64
// directed edges.
// `ext` (hr_dims): NULL, or the images' own field sizes (seed_loop_ext_ragged_kernel).
template <bool CS, int FS>
__device__ __forceinline__ void seed_loop_ext_body(const GrowArgs &g, const int32_t *ext) {
    constexpr int NS = kCacheSlots;
    __shared__ SeedLDS Ls[kSeedWaves];
    __shared__ SeedLoopSharedX S;
    __shared__ int s_ncol[2 * PP_MAX_EDGES];  // set-A column counts per (CAF, direction)
    __shared__ int s_cofs[2 * PP_MAX_EDGES];  // their LDS offsets in s_cols (-1: global)
    __shared__ SeedOcc s_occ;  // per-seed occupancy (the image's own workgroup)
    // kColLdsExt floats (dynamic: the launch sizes it), then the external slots' joints
    // (cache_joints)
    extern __shared__ float s_cols[];
    const int n_img = (int)gridDim.x / (1 + g.n_ext);
    const bool external = (int)blockIdx.x >= n_img;
    const int img = (int)blockIdx.x % n_img;
    const int K = g.K;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    SeedLDS &L = Ls[wave];
    const ColStage cstage = stage_small_sets(g, img, s_ncol, s_cofs, s_cols, kColLdsExt);
    if (lane == 0) {
        L.status = 0;
        L.log_n = 0;
        STAMP_DO(for (int q = 0; q < 10; q++) L.fst[q] = 0);
    }
    if (threadIdx.x < NS) {
        S.cache_seed[threadIdx.x] = -1;
        S.cache_state[threadIdx.x] = 0;
    }
    if (threadIdx.x < kSeedWaves) S.task[threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        S.done = 0;
        S.ext_ticks = 0u;
        S.plan_lock = 0;
        S.decided = 0;
        S.own_on = 0;
    }
    __syncthreads();

    const int n_seeds = min(g.seed_counts[img], g.seed_cap);
    bool heavy = false;  // wave 0's regime (see kExtHeavyAnns)
    const pp_seed *seeds = g.seeds + (int64_t)img * g.seed_cap;
    SeedExt *X = g.xext + img;
    pp_ann *xrec = g.xrec + (int64_t)img * kExtCache;

    STAMP_DECL
    uint8_t *occ_base = g.occ + (int64_t)img * g.occ_cap;
    OccLog *log = g.log + (int64_t)img * g.log_cap;
    pp_ann *work = g.work + (int64_t)img * g.ann_cap;
    pp_ann *cache = g.spec + (int64_t)img * kSpecCache;
    const float red = (float)g.cfg.occupancy_reduction;
    const float msr = occ_msr(g);
    const HrDims dm = hr_dims(ext, img, g.heads.cstride[0], g.hh, g.ww);
    const OccGrid occ = occ_grid(occ_base, K, (int)((double)dm.hh / g.cfg.occupancy_reduction),
                                 (int)((double)dm.ww / g.cfg.occupancy_reduction));
    const int n_help = kSeedWaves + (X ? g.n_ext * kSeedWaves : 0);  // helper lanes 1 .. n_help-1
    // the occupancy at the seeds in LDS (seed_occ_*), or the global grid for more seeds
    const bool socc_on = !external && n_seeds <= kOccSeeds;  // block-uniform
    if (socc_on) seed_occ_init(s_occ, seeds, n_seeds, K, occ, red);

    // committer state (wave 0)
    int n_anns = 0, s = 0;
    uint32_t unset_mask = 0;
    STAMP_DO(int n_rounds = 0, n_hits = 0);

    // append one finished annotation and mark_occupied (cifcaf.py:87-93): wave 0 only
    // (lane j < K holds joint j of the record: x, y, v, scale, from LDS)
    auto commit = [&](const pp_ann *src, bool other_cu, float jx, float jy, float jv, float js) {
        if (other_cu)
            copy_ann_agent(&work[n_anns], src);
        else
            copy_ann(&work[n_anns], src);
        n_anns++;
        const uint32_t set = (uint32_t)__ballot(lane < K && jv > 0.0f);
        unset_mask |= ~set & (K >= 32 ? 0xFFFFFFFFu : ((1u << K) - 1u));
        if (socc_on)
            seed_occ_mark(g, s_occ, occ, jx, jy, js, jv != 0.0f, K);
        else
            occ_mark(g, L, log, occ, jx, jy, js, jv != 0.0f, K);
    };

    if (external || wave > 0) {
        // helper: grow the seeds wave 0 hands over until it is done.  This CU's helpers
        // take them from LDS words and publish into LDS-flagged slots; external ones poll
        // their global word and publish write-through (see SeedExt)
        unsigned long long *tw =
            external ? &X->task[((int)blockIdx.x / n_img - 1) * kSeedWaves + wave] : nullptr;
        if (external && lane == 0) st_agent(tw, 1ull);
        uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            int my = -1, q = 0;
            if (!external) {
                for (;;) {
                    my = lds_acquire(&S.task[wave]);
                    if (my >= 0 || lds_acquire(&S.done)) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (my < 0) break;
                q = S.task_slot[wave];
            } else {
                const unsigned long long v = ld_agent(tw);
                if ((v & 0xFFull) != 2ull) {
                    const bool quit = ld_agent(&X->fin) != 0u ||
                                      __builtin_amdgcn_s_memrealtime() - t0 >
                                          (ld_agent(&X->heavy) ? kExtIdleHeavy : kExtIdleLight);
                    if (quit && cas_agent_wave(tw, 1ull, 3ull)) break;
                    __builtin_amdgcn_s_sleep(2);
                    continue;
                }
                q = (int)((v >> 8) & 0xFFFFull);
                my = (int)(v >> 32);
            }
            ann_from_seed(L, seeds[my], K, img);
            grow<true, CS, FS>(g, L, img, 0, true, cstage, external ? nullptr : &S.done);
            if (!external && lds_acquire(&S.done)) break;  // nobody reads the cache any more
            if (external) {
                publish_ann(&xrec[q], &L.a);
                if (lane == 0) {
                    st_agent(&X->tag[q], (unsigned int)my + 1u);
                    st_agent(tw, 1ull);
                }
                wave_sync();
                t0 = __builtin_amdgcn_s_memrealtime();
                continue;
            }
            if (lane < kKP)
                cache_boxes(s_cols, q)[lane] = plan_box(
                    red, msr, occ, lane,
                    make_float4(L.a.data[lane][0], L.a.data[lane][1], L.a.data[lane][2], L.a.joint_scales[lane]));
            publish_cached(S, cache, q, L);  // (its release orders the boxes too)
            // idle again: wave 0 plans this CU's helpers (no self-planning here, seed_loop.hpp)
            plan_lock(S);
            if (lane == 0) lds_release(&S.task[wave], -1);
            plan_unlock(S);
        }
        if (external) {  // every wave of an external workgroup is a helper
            __syncthreads();
            ext_exit(X, g.n_ext);
            return;
        }
    } else {
        __builtin_amdgcn_s_setprio(3);  // the committer is the critical path: issue first
        grow_initial<CS, FS>(g, L, img, cstage, n_anns, [&](const pp_ann *a) {
            commit(a, false, lane < K ? a->data[lane][0] : 0.0f,
                   lane < K ? a->data[lane][1] : 0.0f, lane < K ? a->data[lane][2] : 0.0f,
                   lane < K ? a->joint_scales[lane] : 0.0f);
        });
        // Hand far-away free seeds after t to the idle helpers (this CU's and the external
        // ones), with S.plan_lock held; `own`: wave 0 grows seed st itself next (the picks
        // keep kSpecFar from it too)
        auto plan_round = [&](const int t, const bool own, const pp_seed &st) {
            STAMP_T0(xr0);
            ext_refresh(S, s_cols, X, xrec, -1, red, msr, occ);
            STAMP_DO(st_acc[14] += STAMP_SINCE(xr0));  // plan: the external slots' refresh
            int tk = 0;
            if (lane > 0 && lane < kSeedWaves)
                tk = lds_acquire(&S.task[lane]) < 0 ? 1 : 0;
            else if (lane >= kSeedWaves && lane < n_help)
                tk = ld_agent(&X->task[lane - kSeedWaves]) == 1ull ? 1 : 0;
            uint64_t idle = __ballot(tk != 0);
            // The slots, one lane each: a snapshot (only wave 0 claims slots; a helper turning
            // 1 into 2 meanwhile at most keeps this plan from reusing or testing that slot),
            // kept current for this plan's own picks.
            const bool sl = lane < NS;
            int r_st = sl ? lds_acquire(&S.cache_state[lane]) : 0;
            int r_seed = sl ? S.cache_seed[lane] : -1;
            float r_x = sl ? S.cache_x[lane] : 0.0f, r_y = sl ? S.cache_y[lane] : 0.0f,
                  r_s = sl ? S.cache_s[lane] : 0.0f;
            // the seeds in flight: later picks keep kSpecFar from them
            uint64_t fly = __ballot(sl && r_st == 1);
            const int scan_end = min(n_seeds, t + 1 + kExtScan);
            STAMP_T0(pf0);
            for (int base = t + 1; base < scan_end && idle; base += 64) {
                const int idx = base + lane;
                bool ok = idx < scan_end;
                pp_seed c{};
                if (ok) {
                    c = seeds[idx];
                    ok = (!own || spec_far(kExtSpecFar, c.x, c.y, c.s, st.x, st.y, st.s)) &&
                         !(socc_on ? seed_occupied(s_occ, idx) : occ_get(occ, c.field, c.x, c.y, red));
                }
                // the slots holding seeds after t (the others are free or passed): skip the
                // seeds they hold, seeds near one still being grown, and seeds that a grown
                // annotation's occupancy boxes will cover once committed
                const uint64_t ahead = __ballot(sl && r_seed > t);
                const uint64_t held = __ballot(sl && r_seed >= base && r_seed < base + 64) & ahead;
                for (uint64_t hq = held; hq; hq &= hq - 1)
                    if (idx == __builtin_amdgcn_readlane(r_seed, __ffsll((unsigned long long)hq) - 1)) ok = false;
                for (uint64_t fq = ahead & fly; fq; fq &= fq - 1) {
                    const int q = __ffsll((unsigned long long)fq) - 1;
                    ok = ok && (__builtin_amdgcn_readlane(r_seed, q) > idx ||
                                 spec_far(kExtSpecFar, c.x, c.y, c.s, rl_f(r_x, q), rl_f(r_y, q), rl_f(r_s, q)));
                }
                const int cxi = (int)clip_ref(c.x / red, 0.0f, (float)(occ.w - 1));
                const int cyi = (int)clip_ref(c.y / red, 0.0f, (float)(occ.h - 1));
                const int cf = ok ? c.field : 0;
                uint64_t gq = ahead & __ballot(sl && r_st == 2);
                while (gq) {  // four slots' boxes per LDS round trip
                    int qs[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        qs[u] = gq ? __ffsll((unsigned long long)gq) - 1 : -1;
                        gq &= gq ? gq - 1 : 0ull;
                    }
                    uint2 b[4];
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        b[u] = qs[u] >= 0 ? cache_boxes(s_cols, qs[u])[cf] : make_uint2(0u, 0u);
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (qs[u] >= 0 && __builtin_amdgcn_readlane(r_seed, qs[u]) < idx &&
                            in_plan_box(b[u], cxi, cyi))
                            ok = false;
                }
                uint64_t m = __ballot(ok);
                ESTAMP(L, 6, pf0);  // plan: the seed filter
                while (m && idle) {
                    const int l = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    const float cx = rl_f(c.x, l), cy = rl_f(c.y, l), csc = rl_f(c.s, l);
                    // far from every seed in flight, this plan's earlier picks included (a
                    // lane per slot)
                    if (__ballot(((fly >> lane) & 1ull) && r_seed < base + l &&
                                 !spec_far(kExtSpecFar, cx, cy, csc, r_x, r_y, r_s)))
                        continue;
                    // a free slot of the helper's kind (this CU's: 0 .. kSpecCache-1; the
                    // external ones after): never grown into, or grown for a seed passed
                    const uint64_t freeq = __ballot(sl && (r_st == 0 || (r_st == 2 && r_seed < t)));
                    const uint64_t free_l = freeq & ((1ull << kSpecCache) - 1ull);
                    const uint64_t free_x = freeq & ~((1ull << kSpecCache) - 1ull);
                    const uint64_t idle_l = idle & ((1ull << kSeedWaves) - 1ull);
                    const uint64_t idle_x = idle & ~((1ull << kSeedWaves) - 1ull);
                    const bool use_l = idle_l && free_l;
                    if (!use_l && !(idle_x && free_x)) {
                        m = 0;
                        idle = 0;
                        break;
                    }
                    const int q = __ffsll((unsigned long long)(use_l ? free_l : free_x)) - 1;
                    const int w = __ffsll((unsigned long long)(use_l ? idle_l : idle_x)) - 1;
                    idle &= ~(1ull << w);
                    const int sd = base + l;
                    if (!use_l) {  // the helper may have just left: then skip it
                        const unsigned long long job = 2ull | ((unsigned long long)(q - kSpecCache) << 8) |
                                                       ((unsigned long long)sd << 32);
                        STAMP_T0(xc0);
                        const bool got = cas_agent_wave(&X->task[w - kSeedWaves], 1ull, job);
                        STAMP_DO(st_acc[15] += STAMP_SINCE(xc0));  // plan: hand-off CAS
                        if (!got) {
                            m |= 1ull << l;  // the seed is still unassigned
                            continue;
                        }
                    }
                    fly |= 1ull << q;
                    if (lane == q) {
                        r_st = 1;
                        r_seed = sd;
                        r_x = cx;
                        r_y = cy;
                        r_s = csc;
                    }
                    if (lane == 0) {
                        S.cache_x[q] = cx;
                        S.cache_y[q] = cy;
                        S.cache_s[q] = csc;
                        lds_release(&S.cache_state[q], 1);  // state first (spec_plan)
                        lds_release(&S.cache_seed[q], sd);
                        S.cache_t[q] = (uint32_t)__builtin_amdgcn_s_memrealtime();
                        if (use_l) {
                            S.task_slot[w] = q;
                            lds_release(&S.task[w], sd);
                        }
                    }
                    wave_sync();
                }
                ESTAMP(L, 6, pf0);  // plan: the picks
            }
        };
        for (;;) {
            const int t = next_free_seed(s, n_seeds, socc_on ? &s_occ : nullptr, seeds, occ, red);
            STAMP(0);
            if (t < 0 || n_anns >= g.ann_cap) {
                if (lane == 0 && t >= 0) L.status |= PP_ST_ANN_OVERFLOW;
                break;
            }
            if (!heavy && n_anns >= kExtHeavyAnns) {  // helpers stay (kExtIdleHeavy)
                heavy = true;
                if (lane == 0) st_agent(&X->heavy, 1u);
            }
            const int cs = lane < NS ? S.cache_seed[lane] : -1;
            const int cst0 = lane < NS ? S.cache_state[lane] : 0;
            const uint64_t hit = __ballot(lane < NS && cs == t && cst0 != 4);
            bool taken = false;
            int hslot = -1;
            if (hit) {  // a helper grew it, or is growing it
                const int slot = __ffsll((unsigned long long)hit) - 1;
                STAMP_T0(hw0);
                if (slot < kSpecCache) {
                    while (lds_acquire(&S.cache_state[slot]) != 2) __builtin_amdgcn_s_sleep(1);
                } else {
                    // another CU's: wait for its tag (bounded; a helper always finishes), or
                    // on a light image grow the seed here and leave the slot a zombie
                    const uint64_t w0 = __builtin_amdgcn_s_memrealtime();
                    const uint32_t el = (uint32_t)w0 - S.cache_t[slot];
                    const uint64_t limit =
                        (S.ext_ticks == 0u || el >= S.ext_ticks / 2u) ? kExtWaitMax : 0ull;
                    for (;;) {
                        ext_refresh(S, s_cols, X, xrec, slot, red, msr, occ);
                        if (S.cache_state[slot] == 2) break;
                        if (__builtin_amdgcn_s_memrealtime() - w0 >= limit) {
                            if (lane == 0) S.cache_state[slot] = 4;  // grow it here instead
                            wave_sync();
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                }
                taken = S.cache_state[slot] == 2;
                hslot = slot;
                ESTAMP(L, 7, hw0);  // a hit: waiting for the helper
            }
            if (taken) {
                const float4 jq = lane < kKP ? cache_joints(S, s_cols, hslot)[lane]
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
                if (hslot < kSpecCache)
                    commit(&cache[hslot], false, jq.x, jq.y, jq.z, jq.w);
                else
                    commit(&xrec[hslot - kSpecCache], true, jq.x, jq.y, jq.z, jq.w);
                s = t + 1;
                if (lane == 0) lds_release(&S.decided, s);  // the slot is free again
                STAMP_DO(n_hits++);
                if (n_anns >= kExtRefillAnns) {
                    // few speculated seeds left ahead: plan a round now, not at the next miss
                    const uint64_t aq = __ballot(lane < NS && S.cache_seed[lane] > t &&
                                                 (S.cache_state[lane] == 1 || S.cache_state[lane] == 2));
                    if (__popcll(aq) < kExtRefill) {
                        plan_lock(S);
                        plan_round(t, false, seeds[t]);
                        plan_unlock(S);
                    }
                }
                STAMP(4);
                continue;
            }
            // a miss: hand far-away free seeds to the idle helpers, then grow t here
            const pp_seed st = seeds[t];
            plan_lock(S);  // wave 0 plans every idle helper, this CU's and the external ones
            if (lane == 0) {
                S.own_x = st.x;
                S.own_y = st.y;
                S.own_s = st.s;
                lds_release(&S.own_on, 1);
                lds_release(&S.decided, t);
            }
            wave_sync();
            // (own = false: picks need not keep kExtSpecFar from seed t, which wave 0 grows
            // itself: cfg5 uniform 1517-1798 -> 1742-1787 images/s, planted unchanged;
            // r06z_ab_refill.txt)
            plan_round(t, false, st);
            plan_unlock(S);
            STAMP_DO(n_rounds++);
            STAMP(1);
            ann_from_seed(L, st, K, img);
            grow<true, CS, FS>(g, L, img, 0, true, cstage);
            STAMP(2);
            commit(&L.a, false, lane < K ? L.a.data[lane][0] : 0.0f,
                   lane < K ? L.a.data[lane][1] : 0.0f, lane < K ? L.a.data[lane][2] : 0.0f,
                   lane < K ? L.a.joint_scales[lane] : 0.0f);
            s = t + 1;
            if (lane == 0) {
                lds_release(&S.own_on, 0);
                lds_release(&S.decided, s);
            }
            STAMP(3);
        }
        if (lane == 0) {
            lds_release(&S.done, 1);
            if (X) st_agent(&X->fin, 1u);
        }
    }
    __syncthreads();  // helpers drained: no wave of this CU is still growing into the cache
    ext_exit(X, g.n_ext);
    if (wave == 0) {
        occ_clear(g, L, log, occ);
        STAMP(5);
        STAMP_DO(st_acc[6] = n_rounds; st_acc[7] = n_hits);
        STAMP_FLUSH(1);
        seed_loop_outputs(g, Ls, img, n_anns, unset_mask);
    }
}

template <bool CS, int FS>
__global__ __launch_bounds__(64 * kSeedWaves) __attribute__((amdgpu_waves_per_eu(3)))
void seed_loop_ext_kernel(GrowArgs g) {
    seed_loop_ext_body<CS, FS>(g, nullptr);
}

template <bool CS, int FS>
__global__ __launch_bounds__(64 * kSeedWaves) __attribute__((amdgpu_waves_per_eu(3)))
void seed_loop_ext_ragged_kernel(GrowArgs g, const int32_t *ext) {
    seed_loop_ext_body<CS, FS>(g, ext);
}

// ---------------------------------------------------------------------------------------
// host: the kernel's launcher (decode.hip has the rest of the host side)
// ---------------------------------------------------------------------------------------
// The seed loop of a decode whose images get external helper workgroups (g.n_ext > 0).
int launch_seed_loop_ext(const GrowArgs &g, int n_img, hipStream_t s, const int32_t *ext) {
    // g.xext is zero: the workspace's zero region, which every external-helper seed
    // loop leaves zero (ext_exit)
    const dim3 grid(n_img * (1 + g.n_ext)), blk(64 * kSeedWaves);
    if (ext) {  // a ragged batch: the same instances over the extent table
        if (g.has_cs)
            hipLaunchKernelGGL((seed_loop_ext_ragged_kernel<true, 2>), grid, blk, kExtDynLds, s, g, ext);
        else if (g.nd <= 64)
            hipLaunchKernelGGL((seed_loop_ext_ragged_kernel<false, 1>), grid, blk, kExtDynLds, s, g, ext);
        else
            hipLaunchKernelGGL((seed_loop_ext_ragged_kernel<false, 2>), grid, blk, kExtDynLds, s, g, ext);
        return check_launch("pp_decode_ragged(seed loop)");
    }
    if (g.has_cs)  // (two-slot at every skeleton size, as in launch_seed_loop)
        hipLaunchKernelGGL((seed_loop_ext_kernel<true, 2>), grid, blk, kExtDynLds, s, g);
    else if (g.nd <= 64)
        hipLaunchKernelGGL((seed_loop_ext_kernel<false, 1>), grid, blk, kExtDynLds, s, g);
    else
        hipLaunchKernelGGL((seed_loop_ext_kernel<false, 2>), grid, blk, kExtDynLds, s, g);
    return check_launch("pp_decode_batch(seed loop)");
}

}  // namespace pp

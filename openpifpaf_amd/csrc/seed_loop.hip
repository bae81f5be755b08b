// seed_loop.hip — the seed loop of a batch that fills the chip (one workgroup per image, no
// external helpers): seed_loop_kernel, its helpers' plan (spec_plan) and its launcher.
// seed_loop.hpp has the design.
#include "seed_loop.hpp"

namespace pp {

constexpr int kSpecScan = 128;     // seeds after the committed one examined per round
constexpr int kSelfScan = 256;     // seeds after the decided ones a finished helper examines

// floats of the column stage (stage_small_sets) in dynamic LDS:
// 74.5 KB (64 KB: 1-2% slower per planted cfg3 step).  With the seed loop's static LDS this
// leaves 39 KB of the CU's 160 KB for the next batch's kernels (DecodePipeline): CafScored
// (caf_bucketed_kernel, 37 KB) must fit beside it (3 KB less: uniform cfg3 4% slower).
constexpr int kColLds = 19072;
struct SeedLoopShared : SeedLoopSharedT<kSpecCache> {
    uint2 cache_box[kSpecCache][kKP];  // the grown slots' occupancy boxes (plan_box)
};
// (kColLds above keeps the one-CU seed loop's LDS at 124,608 bytes with these and SeedOcc)

// Speculation plan of seed_loop_kernel, collective over one wave, with S.plan_lock held:
// free seeds in [decided, decided + scan) that the committed occupancy and the cached
// annotations' occupancy boxes do not cover (the grown ones' boxes, S.cache_box, and the
// joints set so far of those in flight, cache_pm / own_pm), kSpecFar joint scales from
// every seed in flight (and from wave 0's own seed when S.own_on), each into a free cache
// slot (never used, or holding a seed before `decided`), for the helper waves in `idle`
// (bit w = wave w), which get their seeds through S.task.  Returns the helpers left idle.
// A slot is claimed state first, seed second (both released): wave 0 reads the seed without
// the lock and, seeing its seed there, waits for state 2.
// The slots are read once, a lane each (only the plan, under the lock, claims slots; a
// helper turning 1 into 2 meanwhile at most keeps this plan from reusing that slot), and
// kept current for the plan's own picks; per seed the slots are tested with SGPR operands
// (readlane), the grown ones' boxes four per LDS round trip.
// Not inlined: it runs outside the grow and takes no GrowArgs (a non-inlined reference to
// the kernarg struct makes the compiler copy it to scratch), so the kernel's registers stay
// the grow's.
__device__ __noinline__ uint64_t spec_plan(SeedLoopShared &S, const pp_seed *seeds, int n_seeds,
                                           int decided, int scan, OccGrid occ, float red,
                                           float msr, float far_k, uint64_t idle,
                                           const SeedOcc *socc) {
    constexpr int NS = kSpecCache;
    const int lane = threadIdx.x & 63;
    const bool sl = lane < NS;
    int r_st = sl ? lds_acquire(&S.cache_state[lane]) : 0;
    int r_seed = sl ? S.cache_seed[lane] : -1;
    float r_x = sl ? S.cache_x[lane] : 0.0f, r_y = sl ? S.cache_y[lane] : 0.0f,
          r_s = sl ? S.cache_s[lane] : 0.0f;
    uint64_t fly = __ballot(sl && r_st == 1);
    const bool own = lds_acquire(&S.own_on) != 0;
    const float ox = S.own_x, oy = S.own_y, osc = S.own_s;
    const int scan_end = min(n_seeds, decided + scan);
    for (int base = decided; base < scan_end && idle; base += 64) {
        const int idx = base + lane;
        bool ok = idx < scan_end;
        pp_seed c{};
        if (ok) {
            c = seeds[idx];
            ok = (!own || spec_far(far_k, c.x, c.y, c.s, ox, oy, osc)) &&
                 !(socc ? seed_occupied(*socc, idx) : occ_get(occ, c.field, c.x, c.y, red));
        }
        const int cxi = (int)clip_ref(c.x / red, 0.0f, (float)(occ.w - 1));
        const int cyi = (int)clip_ref(c.y / red, 0.0f, (float)(occ.h - 1));
        const int cf = c.field;
        // inside the occupancy box joint jq of an annotation will mark (occupancy.py:31-39)
        auto covered = [&](const float4 &jq) {
            int box[4];
            return jq.z != 0.0f && occ_box_r(red, msr, occ, cf, jq.x, jq.y, jq.w, box) &&
                   cxi >= box[0] && cxi < box[1] && cyi >= box[2] && cyi < box[3];
        };
        if (ok && own && ((lds_acquire_u(&S.own_pm) >> cf) & 1u) && covered(S.own_j[cf]))
            ok = false;  // wave 0's own annotation in flight covers it
        // the slots holding a seed from `decided` on, not zombies (the others are free)
        const uint64_t live = __ballot(sl && r_seed >= decided && r_st != 0 && r_st != 4);
        // skip the seeds they hold
        for (uint64_t hq = live & __ballot(sl && r_seed >= base && r_seed < base + 64); hq; hq &= hq - 1)
            if (idx == __builtin_amdgcn_readlane(r_seed, __ffsll((unsigned long long)hq) - 1)) ok = false;
        // seeds near one still being grown, or covered by the joints its grow has set so far
        const uint32_t r_pm = sl ? lds_acquire_u(&S.cache_pm[lane]) : 0u;
        for (uint64_t fq = live & fly; fq; fq &= fq - 1) {
            const int q = __ffsll((unsigned long long)fq) - 1;
            ok = ok && (__builtin_amdgcn_readlane(r_seed, q) > idx ||
                         spec_far(far_k, c.x, c.y, c.s, rl_f(r_x, q), rl_f(r_y, q), rl_f(r_s, q)));
            const uint32_t pm = (uint32_t)__builtin_amdgcn_readlane((int)r_pm, q);
            if (ok && ((pm >> cf) & 1u) && __builtin_amdgcn_readlane(r_seed, q) < idx &&
                covered(S.cache_j[q][cf]))
                ok = false;
        }
        // seeds a grown annotation's occupancy boxes will cover once committed
        const int bf = ok ? cf : 0;
        uint64_t gq = live & ~fly & __ballot(sl && r_st == 2);
        while (gq) {  // four slots' boxes per LDS round trip
            int qs[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                qs[u] = gq ? __ffsll((unsigned long long)gq) - 1 : -1;
                gq &= gq ? gq - 1 : 0ull;
            }
            uint2 bx[4];
#pragma unroll
            for (int u = 0; u < 4; u++) bx[u] = qs[u] >= 0 ? S.cache_box[qs[u]][bf] : make_uint2(0u, 0u);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (qs[u] >= 0 && __builtin_amdgcn_readlane(r_seed, qs[u]) < idx &&
                    in_plan_box(bx[u], cxi, cyi))
                    ok = false;
        }
        uint64_t m = __ballot(ok);
        while (m && idle) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const float cx = rl_f(c.x, l), cy = rl_f(c.y, l), csc = rl_f(c.s, l);
            // far from this plan's earlier picks and every other seed in flight (a lane per slot)
            if (__ballot(((fly >> lane) & 1ull) && r_seed < base + l &&
                         !spec_far(far_k, cx, cy, csc, r_x, r_y, r_s)))
                continue;
            // a free slot: never grown into, or grown for a seed already decided
            const uint64_t freeq = __ballot(sl && (r_st == 0 || (r_st == 2 && r_seed < decided)));
            if (!freeq) return idle;  // no slot: nobody else can be planned either
            const int q = __ffsll((unsigned long long)freeq) - 1;
            const int w = __ffsll((unsigned long long)idle) - 1;
            idle &= idle - 1;
            fly |= 1ull << q;
            if (lane == q) {
                r_st = 1;
                r_seed = base + l;
                r_x = cx;
                r_y = cy;
                r_s = csc;
            }
            if (lane == 0) {
                S.cache_x[q] = cx;
                S.cache_y[q] = cy;
                S.cache_s[q] = csc;
                S.cache_pm[q] = 0u;  // no joints of the new grow yet
                lds_release(&S.cache_state[q], 1);
                lds_release(&S.cache_seed[q], base + l);
                S.task_slot[w] = q;
                lds_release(&S.task[w], base + l);
            }
            wave_sync();
        }
    }
    return idle;
}

// <= 168 VGPRs (3 waves per SIMD; a few spills) and the column stage in dynamic LDS: the
// image's workgroup leaves room on its CU for the next batch's CifHr / seeds / CafScored
// workgroups (DecodePipeline).  Planted 1.031 -> 1.013 ms, uniform 21.7 -> 20.4 ms per
// overlapped step; 4 waves per SIMD (128 VGPRs, 532 spills): 1.37 ms.
// Grid: n_img image workgroups, then n_ext * n_img external helper workgroups (helper
// workgroup x of image i is block n_img * (1 + x) + i, on image i's XCD when n_img % 8 == 0).
// NS: frontier slots per lane (grow_frontier.hpp), 1 when the skeleton has at most 64
// directed edges: seed_loop_kernel<false, 1> needs 154 VGPRs and no spills where the two-slot
// instance sits at the 168 cap with 28 (tools/resource_usage.py).
// `ext` (hr_dims): NULL, or the images' own field sizes (seed_loop_ragged_kernel).
template <bool CS, int NS>
__device__ __forceinline__ void seed_loop_body(const GrowArgs &g, const int32_t *ext) {
    __shared__ SeedLDS Ls[kSeedWaves];
    __shared__ SeedLoopShared S;
    __shared__ int s_ncol[2 * PP_MAX_EDGES];  // set-A column counts per (CAF, direction)
    __shared__ int s_cofs[2 * PP_MAX_EDGES];  // their LDS offsets in s_cols (-1: global)
    __shared__ SeedOcc s_occ;  // per-seed occupancy (images of at most kOccSeeds seeds)
    extern __shared__ float s_cols[];  // kColLds floats (dynamic: the launch sizes it)
    const int img = blockIdx.x;
    const int K = g.K;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    SeedLDS &L = Ls[wave];
    const ColStage cstage = stage_small_sets(g, img, s_ncol, s_cofs, s_cols, kColLds);
    if (lane == 0) {
        L.status = 0;
        L.log_n = 0;
        STAMP_DO(for (int q = 0; q < 10; q++) L.fst[q] = 0);
    }
    if (threadIdx.x < kSpecCache) {
        S.cache_seed[threadIdx.x] = -1;
        S.cache_state[threadIdx.x] = 0;
        S.cache_pm[threadIdx.x] = 0u;
    }
    if (threadIdx.x < kSeedWaves) S.task[threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        S.done = 0;
        S.plan_lock = 0;
        S.decided = 0;
        S.own_on = 0;
        S.plan_req = 0;
        S.own_pm = 0u;
    }
    __syncthreads();

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
    const int n_seeds = min(g.seed_counts[img], g.seed_cap);
    const pp_seed *seeds = g.seeds + (int64_t)img * g.seed_cap;
    // the occupancy at the seeds in LDS (seed_occ_*), or the global grid for more seeds
    const bool socc_on = n_seeds <= kOccSeeds;
    if (socc_on) seed_occ_init(s_occ, seeds, n_seeds, K, occ, red);
    const SeedOcc *socc = socc_on ? &s_occ : nullptr;
    // the plans' speculation distance: kSpecFar, but none on images with more seeds than
    // kOccSeeds (dense fields, where nearly every seed lies near one in flight): uniform
    // cfg3 15.6k-16.1k -> 16.1k-16.2k images/s, planted unchanged (r06z_ab_dense_far.txt)
    const float far_img = socc_on ? g.spec_far : 0.0f;

    // committer state (wave 0)
    int n_anns = 0, s = 0;
    uint32_t unset_mask = 0;
    STAMP_DO(int n_rounds = 0, n_hits = 0);

    // append one finished annotation and mark_occupied (cifcaf.py:87-93): wave 0 only
    // (lane j < K holds joint j of the record: x, y, v, scale, from LDS)
    // (the record's loads are issued first and stored after the marks: the marks hide
    // their latency)
    auto commit = [&](const pp_ann *src, float jx, float jy, float jv, float js) {
        STAMP_T0(ct0);
        const AnnRegs rec = ann_load(src);
        const uint32_t set = (uint32_t)__ballot(lane < K && jv > 0.0f);
        unset_mask |= ~set & (K >= 32 ? 0xFFFFFFFFu : ((1u << K) - 1u));
        if (socc_on)
            seed_occ_mark(g, s_occ, occ, jx, jy, js, jv != 0.0f, K);
        else
            occ_mark(g, L, log, occ, jx, jy, js, jv != 0.0f, K);
        ESTAMP(L, 5, ct0);  // (wave 0) the occupancy marks
        ann_store(&work[n_anns], rec);
        n_anns++;
        ESTAMP(L, 4, ct0);  // (wave 0) the record's stores (after the marks)
    };

    if (wave > 0) {  // helper: grow the seeds wave 0 hands over until it is done
        // `decided` when this helper's last plan found it nothing to grow (-1: none): once
        // wave 0 has moved on (commits free slots, passes seeds), an idle helper plans itself
        // again instead of waiting for wave 0's next miss (which a wave 0 that only takes
        // cached annotations never has)
        int idle_dec = -1;
        for (;;) {
            int my;
            for (;;) {
                my = lds_acquire(&S.task[wave]);
                if (my >= 0 || lds_acquire(&S.done)) break;
                if (idle_dec >= 0 && lds_acquire(&S.decided) != idle_dec) {
                    STAMP_T0(hp2);
                    plan_lock(S);
                    uint64_t left = 1ull << wave;
                    const int dec = lds_acquire(&S.decided);
                    if (!lds_acquire(&S.done) && lds_acquire(&S.task[wave]) < 0)
                        left = spec_plan(S, seeds, n_seeds, dec, kSelfScan, occ, red, msr, far_img,
                                         left, socc);
                    plan_unlock(S);
                    idle_dec = left ? dec : -1;
                    STAMP_DO(if (lane == 0) L.fst[8] += STAMP_SINCE(hp2));
                    continue;
                }
                if (lds_acquire(&S.plan_req)) {
                    // wave 0 is growing a seed of its own: plan every idle helper (this one
                    // included) around it
                    STAMP_T0(hp0);
                    plan_lock(S);
                    if (lds_acquire(&S.plan_req) && !lds_acquire(&S.done)) {
                        if (lane == 0) lds_release(&S.plan_req, 0);
                        const int tk = lane > 0 && lane < kSeedWaves ? lds_acquire(&S.task[lane]) : 0;
                        const uint64_t idle = __ballot(lane > 0 && lane < kSeedWaves && tk < 0);
                        const int dec = lds_acquire(&S.decided);
                        if (idle)
                            spec_plan(S, seeds, n_seeds, dec, kSpecScan, occ, red, msr, far_img,
                                      idle, socc);
                    }
                    plan_unlock(S);
                    if (lds_acquire(&S.task[wave]) < 0) idle_dec = lds_acquire(&S.decided);
                    STAMP_DO(if (lane == 0) L.fst[8] += STAMP_SINCE(hp0));
                    continue;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (my < 0) break;
            const int q = S.task_slot[wave];
            STAMP_T0(hg0);
            ann_from_seed(L, seeds[my], K, img);
            grow<true, CS, NS>(g, L, img, 0, true, cstage, &S.done, S.cache_j[q], &S.cache_pm[q]);
            STAMP_DO(if (lane == 0) {  // helper grows and their cycles (phase-1 slots 8 and 5)
                L.fst[4] += 1;
                L.fst[5] += STAMP_SINCE(hg0);
            });
            if (lds_acquire(&S.done)) break;  // nobody reads the cache any more
            if (lane < kKP)
                S.cache_box[q][lane] = plan_box(
                    red, msr, occ, lane,
                    make_float4(L.a.data[lane][0], L.a.data[lane][1], L.a.data[lane][2], L.a.joint_scales[lane]));
            publish_cached(S, cache, q, L);  // (its release orders the boxes too)
            STAMP_T0(hp1);
            // plan this wave's next grow itself, with its own annotation now in the cache (its
            // occupancy boxes rule out the other seeds of the same person); wave 0 plans only
            // when it has to grow a seed itself
            plan_lock(S);
            uint64_t left = 1ull << wave;
            if (!lds_acquire(&S.done)) {
                const int dec = lds_acquire(&S.decided);
                left = spec_plan(S, seeds, n_seeds, dec, kSelfScan, occ, red, msr, far_img, left,
                                 socc);
            }
            if (left && lane == 0) lds_release(&S.task[wave], -1);
            plan_unlock(S);
            idle_dec = left ? lds_acquire(&S.decided) : -1;
            STAMP_DO(if (lane == 0) {
                L.fst[8] += STAMP_SINCE(hp1);
                L.fst[9] += 1;
            });
        }
    } else {
        __builtin_amdgcn_s_setprio(3);  // the committer is the critical path: issue first
        grow_initial<CS, NS>(g, L, img, cstage, n_anns, [&](const pp_ann *a) {
            commit(a, lane < K ? a->data[lane][0] : 0.0f, lane < K ? a->data[lane][1] : 0.0f,
                   lane < K ? a->data[lane][2] : 0.0f, lane < K ? a->joint_scales[lane] : 0.0f);
        });
        for (;;) {
            const int t = next_free_seed(s, n_seeds, socc_on ? &s_occ : nullptr, seeds, occ, red);
            STAMP(0);
            if (t < 0 || n_anns >= g.ann_cap) {
                if (lane == 0 && t >= 0) L.status |= PP_ST_ANN_OVERFLOW;
                break;
            }
            const int cs = lane < kSpecCache ? S.cache_seed[lane] : -1;
            const uint64_t hit = __ballot(lane < kSpecCache && cs == t);
            if (hit) {  // a helper grew it, or is growing it
                const int slot = __ffsll((unsigned long long)hit) - 1;
                STAMP_T0(hw0);
                while (lds_acquire(&S.cache_state[slot]) != 2) __builtin_amdgcn_s_sleep(1);
                STAMP_DO(if (lane == 0) L.fst[8] += STAMP_SINCE(hw0));
                const float4 jq = lane < kKP ? S.cache_j[slot][lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                commit(&cache[slot], jq.x, jq.y, jq.z, jq.w);
                s = t + 1;
                if (lane == 0) lds_release(&S.decided, s);  // the slot is free again
                STAMP_DO(n_hits++);
                STAMP(4);
                continue;
            }
            // hand far-away free seeds to the idle helpers (an idle helper plans them), then
            // grow t here
            const pp_seed st = seeds[t];
            if (lane == 0) {
                S.own_pm = 0u;  // (grow publishes the seed joint first)
                S.own_x = st.x;
                S.own_y = st.y;
                S.own_s = st.s;
                lds_release(&S.own_on, 1);
                lds_release(&S.decided, t);
                lds_release(&S.plan_req, 1);
            }
            wave_sync();
            STAMP_DO(n_rounds++);
            STAMP(1);
            ann_from_seed(L, st, K, img);
            grow<true, CS, NS>(g, L, img, 0, true, cstage, nullptr, S.own_j, &S.own_pm);
            STAMP(2);
            commit(&L.a, lane < K ? L.a.data[lane][0] : 0.0f, lane < K ? L.a.data[lane][1] : 0.0f,
                   lane < K ? L.a.data[lane][2] : 0.0f, lane < K ? L.a.joint_scales[lane] : 0.0f);
            s = t + 1;
            if (lane == 0) {
                lds_release(&S.own_on, 0);
                lds_release(&S.decided, s);
            }
            STAMP(3);
        }
        if (lane == 0) lds_release(&S.done, 1);
    }
    __syncthreads();  // helpers drained: no wave is still growing into the cache
    if (wave == 0) {
        occ_clear(g, L, log, occ);
        STAMP(5);
#ifdef PP_STAMPS
        st_acc[6] = n_rounds;
        st_acc[7] = n_hits;
        {  // helpers' grows (count into slot 8, cycles into slot 5 in place of occ_clear)
            uint64_t hn = 0, hc = 0, hp = 0, hpn = 0;
            for (int w = 1; w < kSeedWaves; w++) {
                hn += Ls[w].fst[4];
                hc += Ls[w].fst[5];
                hp += Ls[w].fst[8];
                hpn += Ls[w].fst[9];
            }
            L.fst[3] = hn;
            st_acc[5] = hc;
            st_acc[14] = hp;  // the helpers' plans (self plans and wave 0's requests)
            st_acc[15] = L.fst[8] | (hpn << 40);  // wave 0's hit waits; self plans << 40
            L.fst[6] = L.fst[4];  // (diagnostic: wave 0's copy / mark cycles in slots 12 / 13)
            L.fst[7] = L.fst[5];
        }
#endif
        STAMP_FLUSH(1);
        seed_loop_outputs(g, Ls, img, n_anns, unset_mask);
    }
}

template <bool CS, int NS>
__global__ __launch_bounds__(64 * kSeedWaves) __attribute__((amdgpu_waves_per_eu(3)))
void seed_loop_kernel(GrowArgs g) {
    seed_loop_body<CS, NS>(g, nullptr);
}

template <bool CS, int NS>
__global__ __launch_bounds__(64 * kSeedWaves) __attribute__((amdgpu_waves_per_eu(3)))
void seed_loop_ragged_kernel(GrowArgs g, const int32_t *ext) {
    seed_loop_body<CS, NS>(g, ext);
}

// ---------------------------------------------------------------------------------------
// host: the kernel's launcher (decode.hip has the rest of the host side)
// ---------------------------------------------------------------------------------------
// The seed loop of a decode whose images get no external helper workgroups (g.n_ext == 0).
int launch_seed_loop(const GrowArgs &g, int n_img, hipStream_t s, const int32_t *ext) {
    const size_t dyn = kColLds * sizeof(float);
    if (ext) {  // a ragged batch: the same instances over the extent table
        const dim3 rblk(64 * kSeedWaves);
        if (g.has_cs)
            hipLaunchKernelGGL((seed_loop_ragged_kernel<true, 2>), dim3(n_img), rblk, dyn, s, g, ext);
        else if (g.nd <= 64)
            hipLaunchKernelGGL((seed_loop_ragged_kernel<false, 1>), dim3(n_img), rblk, dyn, s, g, ext);
        else
            hipLaunchKernelGGL((seed_loop_ragged_kernel<false, 2>), dim3(n_img), rblk, dyn, s, g, ext);
        return check_launch("pp_decode_ragged(seed loop)");
    }
    // confidence_scales: their own kernel instances (the default ones carry no
    // registers for them: complete_kernel stays at 128 VGPRs, 4 waves per SIMD); they keep
    // the two-slot frontier at every skeleton size (fewer instances to compile)
    const dim3 blk(64 * kSeedWaves);
    if (g.has_cs)
        hipLaunchKernelGGL((seed_loop_kernel<true, 2>), dim3(n_img), blk, dyn, s, g);
    else if (g.nd <= 64)
        hipLaunchKernelGGL((seed_loop_kernel<false, 1>), dim3(n_img), blk, dyn, s, g);
    else
        hipLaunchKernelGGL((seed_loop_kernel<false, 2>), dim3(n_img), blk, dyn, s, g);
    return check_launch("pp_decode_batch(seed loop)");
}

}  // namespace pp

// nms.hip — nms.Keypoints.annotations (nms.py:17-57): the NMS kernels of a decode, their
// launcher, and the stand-alone pp_nms_keypoints* entry points over caller records.
#include "grow_device.hpp"

namespace pp {

// np.sum of K float64 terms in NumPy's pairwise order (n <= 128: eight accumulators over
// blocks of 8, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail)
__device__ double pw_sum(const double *a, int K) {
    if (K < 8) {
        double res = 0.0;
        for (int i = 0; i < K; i++) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < K - (K % 8); i += 8) {
        r0 += a[i];
        r1 += a[i + 1];
        r2 += a[i + 2];
        r3 += a[i + 3];
        r4 += a[i + 4];
        r5 += a[i + 5];
        r6 += a[i + 6];
        r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < K; i++) res += a[i];
    return res;
}

// stable sort of idx[0..n) by descending score (sorted(anns, key=lambda a: -a.score()))
__device__ void sort_by_score(int *perm, int np, int n, const double *score) {
    for (int i = threadIdx.x & 63; i < np; i += 64) perm[i] = i;
    wave_sync();
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x & 63; i < np; i += 64) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = perm[i], b = perm[ixj];
                    auto before = [&](int p, int q) {
                        if (p >= n) return false;
                        if (q >= n) return true;
                        const double kp = -score[p], kq = -score[q];
                        if (kp != kq) return kp < kq;
                        return p < q;
                    };
                    const bool asc = (i & k) == 0;
                    if (asc ? before(b, a) : before(a, b)) {
                        perm[i] = b;
                        perm[ixj] = a;
                    }
                }
            }
            wave_sync();
        }
    }
}

// ---- nms.Keypoints.annotations (nms.py:17-57) + output, one workgroup per image ----
// The score filters are per annotation: spread over the waves.  The suppression pass
// (nms.py:34-45) is sequential over the sorted annotations, but each joint lives on its
// own occupancy plane, so the planes are independent: wave w walks planes w, w + 8, ...
// and keeps the plane's marked boxes in a list instead of a u8 grid.  A joint is
// "occupied" iff the number of earlier marked boxes covering its cell is non-zero mod 256
// (the grid's u8 += 1 wraps), which is exactly what the grid lookup returns.
// Workgroups of kNmsWaves (8) waves for dense batches on the one-CU seed loop
// (PP_STAGE_NMS_WIDE), else kNmsNarrow (4): at 155 VGPRs a 4-wave workgroup (one wave per
// SIMD) fits on a CU beside a seed-loop workgroup (two waves per SIMD at 168), an 8-wave one
// does not, so in the overlapped pipeline the narrow NMS of batch i runs beside batch i + 1's
// seed loop instead of waiting for its CUs.  A/B on one box: planted cfg3 370-375k ->
// 385-394k images/s, cfg5 uniform 1356-1365 -> 1434-1443; uniform cfg3 (400 annotations per
// image, 17 planes on 4 waves) 15.1-15.3k -> 14.4-14.5k, hence the wide form there.
constexpr int kNmsWaves = 8;
constexpr int kNmsNarrow = 4;
static_assert(kNmsBoxLists >= kNmsWaves, "one box list per NMS wave");
// boxes per plane kept in REGISTERS, kNmsRegBoxes per lane (box i: lane i % 64, slot
// i / 64), global scratch beyond: a check is ALU over the lane's slots plus one wave sum,
// and the kernel needs no LDS for them: beside a seed-loop workgroup (124,608 B) and a set-A
// workgroup (37,440 B) a CU has 1,792 B left, which nms_kernel<4, 0> stays inside
// (tests/test_nms_resources.py).  With the
// list in LDS (448 per plane) and global memory beyond, uniform cfg5 (1370 annotations per
// image) spent 20M cycles per image in the suppression pass on global-list loads.
constexpr int kNmsRegBoxes = 24;

struct ScoreLDS {
    double prod[kKP];
    double score_bc;
#ifdef PP_STAMPS
    uint64_t fst[8];  // unused here; keeps STAMP_FLUSH uniform
#endif
};

// Annotation.score() (annotation.py:24-28, 60-71) in float64, collective over one wave:
// lane j finds the rank of v_j in descending order, the rank-ordered products go to LDS
// and lane 0 adds them in NumPy's pairwise order.  `zero_j` (suppress_score_index, >= 0)
// reads as v = 0; `w` (the record's own score_weights) replaces the default weights.
__device__ double ann_score_w(ScoreLDS &L, const float (*data)[3], int K, int zero_j = -1,
                              const double *w = nullptr) {
    const int lane = threadIdx.x & 63;
    const double ws = (double)(3 * min(K, 3) + (K - min(K, 3)));
    if (lane < K) {
        const float vj = lane == zero_j ? 0.0f : data[lane][2];
        int rank = 0;
        for (int i = 0; i < K; i++) {
            const float vi = i == zero_j ? 0.0f : data[i][2];
            rank += (vi > vj) || (vi == vj && i < lane);
        }
        L.prod[rank] = (w ? w[rank] : (rank < 3 ? 3.0 : 1.0) / ws) * (double)vj;
    }
    wave_sync();
    if (lane == 0) L.score_bc = pw_sum(L.prod, K);
    wave_sync();
    const double res = L.score_bc;
    wave_sync();
    return res;
}

// the score nms.Keypoints sorts and filters record i of image img by: the default
// Annotation.score(), or with the caller's per-record fixed_score / suppress_score_index /
// score_weights (standalone NMS)
__device__ double nms_ann_score(const GrowArgs &g, ScoreLDS &L, int img, int i,
                                const float (*data)[3], int K) {
    if (!g.nms_spec) return ann_score_w(L, data, K);
    const int64_t gi = (int64_t)img * g.ann_cap + i;
    const int spec = g.nms_spec[gi];
    if (spec == -2) return g.nms_fixed[gi];
    return ann_score_w(L, data, K, spec, g.nms_sw + gi * K);
}

// the grid cell occ_get reads: 1 = occupied whatever the grid holds (f beyond the planes),
// 0 = free whatever it holds (empty grid), -1 = look at (xi, yi)
__device__ __forceinline__ int occ_cell(const OccGrid &o, int f, float x, float y, float red,
                                        int &xi, int &yi) {
    if (f >= o.f) return 1;
    if (o.h <= 0 || o.w <= 0) return 0;
    xi = (int)clip_ref(x / red, 0.0f, (float)(o.w - 1));
    yi = (int)clip_ref(y / red, 0.0f, (float)(o.h - 1));
    return -1;
}

// nms.py:34-45 for plane f: the m kept annotations in sorted order, whose joint f
// `load(r0, wi, x, y, v, s)` gives per lane (annotation r0 + lane: work index, joint f; v = 0
// beyond m).  The plane's marked boxes are kept in a list instead of a u8 grid: kNmsRegBoxes
// per lane in registers, `gbox` beyond.  A joint is "occupied" iff the number of earlier
// marked boxes covering its cell is non-zero mod 256 (the grid's u8 += 1 wraps).  Suppressed
// joints are written (v * suppression) as they are found.
template <typename Load>
__device__ __forceinline__ void nms_plane_boxes(const GrowArgs &g, pp_ann *work, int m, int f,
                                                const OccGrid &no, float red, int2 *gbox,
                                                Load load) {
    const int lane = threadIdx.x & 63;
    int nbox = 0;
    int2 rb[kNmsRegBoxes];  // (x0 | x1 << 16, y0 | y1 << 16); zero: covers nothing
#pragma unroll
    for (int q = 0; q < kNmsRegBoxes; q++) rb[q] = make_int2(0, 0);
    for (int r0 = 0; r0 < m; r0 += 64) {
        int wi = 0;
        float jx = 0.0f, jy = 0.0f, jv = 0.0f, js = 0.0f;
        load(r0, wi, jx, jy, jv, js);
        const int nr = min(64, m - r0);
        for (int l = 0; l < nr; l++) {
            const float v = rl_f(jv, l);
            if (v == 0.0f) continue;
            const float x = rl_f(jx, l), y = rl_f(jy, l);
            int xi = 0, yi = 0;
            const int fixed = occ_cell(no, f, x, y, red, xi, yi);
            int cnt = 0;
            if (fixed < 0) {
#pragma unroll
                for (int q = 0; q < kNmsRegBoxes; q += 4) {  // unused slots are zero
                    if (q * 64 >= nbox) continue;  // uniform: skip empty groups
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int2 b = rb[q + u];
                        cnt += (xi >= (b.x & 0xFFFF) && xi < (b.x >> 16) &&
                                yi >= (b.y & 0xFFFF) && yi < (b.y >> 16));
                    }
                }
                for (int q = kNmsRegBoxes * 64 + lane; q < nbox; q += 64) {
                    const int2 b = gbox[q];
                    cnt += (xi >= (b.x & 0xFFFF) && xi < (b.x >> 16) &&
                            yi >= (b.y & 0xFFFF) && yi < (b.y >> 16));
                }
                cnt = wave_total(cnt);
            }
            const bool occupied = fixed < 0 ? (cnt & 255) != 0 : fixed == 1;
            if (occupied) {
                if (lane == 0) work[rl_i(wi, l)].data[f][2] = v * g.cfg.nms_suppression;
            } else {
                int box[4];
                if (occ_box(g, no, f, x, y, rl_f(js, l), box)) {
                    const int2 nb = make_int2(box[0] | (box[1] << 16), box[2] | (box[3] << 16));
                    if (nbox < kNmsRegBoxes * 64) {
#pragma unroll
                        for (int q = 0; q < kNmsRegBoxes; q++)
                            if (q == (nbox >> 6) && lane == (nbox & 63)) rb[q] = nb;
                    } else if (lane == 0) {
                        gbox[nbox] = nb;
                    }
                    nbox++;
                    // only a box in global memory needs the fence (a fence here waits
                    // for every outstanding store, e.g. the suppressed v above)
                    if (nbox > kNmsRegBoxes * 64) wave_sync();
                }
            }
        }
    }
}

// ---- nms.Keypoints.annotations for an image of at most kNmsSmall annotations ----
// The same result as the general path of nms_kernel<W, 0> below, bit for bit and byte for byte
// in work[]; only the schedule differs.  With one lane per annotation nothing has to be walked
// pose by pose or sorted through memory:
// - scores: lane j holds joint j of the annotation, the rank of v_j comes from K readlanes of
//   the lane-held v (ann_score_lanes) and the per-annotation maxima from an ordered readlane
//   walk (the `a > ax ? a : ax` chain from joint 0 on, which has the reference's NaN behaviour);
// - sorts: a kept score is never NaN (`sc >= it` is false for NaN), so "-score ascending, then
//   index ascending" is a strict total order and any correct sort gives the stable sort's
//   permutation: each lane counts the kept lanes that come before it, by sort_by_score's
//   comparator (-0.0 and +0.0 tie), over readlanes of the double;
// - planes: lane r holds joint f of the r-th sorted annotation, its cell and its box.  Bit q
//   of lane r's row mask says that q < r and box q covers cell r; the plane is then resolved
//   in order over two scalar masks (marked, suppressed).  At most 63 earlier boxes cover a
//   cell, so the reference's u8 count cannot wrap: "count non-zero mod 256" is "any".
// Scores cross the waves through s_sc[] and the sorted work indices through s_ix[] (LDS, 576
// B), the maxima through amax[] in the workspace; keep[] / perm[] / surv[] / flag[] / score[] /
// kscore[] / gbox of the workspace are not written: nothing reads them after a PHASE 0 launch.
// Records that carry their own score inputs (g.nms_spec, the standalone scored entry point)
// stay on the general path.
constexpr int kNmsSmall = 64;

__device__ __forceinline__ double rl_d(double v, int l) {
    return __hiloint2double(rl_i(__double2hiint(v), l), rl_i(__double2loint(v), l));
}

// ann_score_w with the default weights over lane-held confidences: lane j < K holds v_j (the
// value of lanes >= K is ignored); collective over one wave, uniform result
__device__ __forceinline__ double ann_score_lanes(ScoreLDS &L, float vj, int K) {
    const int lane = threadIdx.x & 63;
    const double ws = (double)(3 * min(K, 3) + (K - min(K, 3)));
    int rank = 0;
    for (int i = 0; i < K; i++) {
        const float vi = rl_f(vj, i);
        rank += (vi > vj) || (vi == vj && i < lane);
    }
    if (lane < K) L.prod[rank] = ((rank < 3 ? 3.0 : 1.0) / ws) * (double)vj;
    wave_sync();
    double res = 0.0;
    if (lane == 0) res = pw_sum(L.prod, K);
    wave_sync();  // prod[] may be written again
    return rl_d(res, 0);
}

// the rank of this lane's (key, lane) among the lanes of `km` under sort_by_score's order
__device__ __forceinline__ int nms_rank_lanes(uint64_t km, double key) {
    const int lane = threadIdx.x & 63;
    int rank = 0;
    for (uint64_t rest = km; rest; rest &= rest - 1) {
        const int q = __ffsll((unsigned long long)rest) - 1;
        const double kq = rl_d(key, q);
        rank += kq != key ? kq < key : q < lane;
    }
    return rank;
}

// returns the number of survivors written to out[] (with out_idx); the caller writes counts
// and status.  s_m, s_m2, s_mx, s_my: the kernel's shared words.
template <int W>
__device__ __forceinline__ int nms_small(const GrowArgs &g, ScoreLDS &L, int img, pp_ann *work,
                                         pp_ann *out, int n, float *amax, int &s_m, int &s_m2,
                                         float &s_mx, float &s_my) {
    __shared__ double s_sc[kNmsSmall];   // scores: by work index, sorted rank, output rank
    __shared__ uint8_t s_ix[kNmsSmall];  // work indices: by sorted rank, then by output rank
    const int K = g.K, cap = g.ann_cap;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float red = (float)g.cfg.occupancy_reduction;
    const float kt = g.cfg.nms_keypoint_threshold;
    const double it = g.nms_it;
    STAMP_DECL
    // nms.py:20-22: zero joints below keypoint_threshold; the scores and maxima per annotation
    for (int i = wave; i < n; i += W) {
        float x = 0.0f, y = 0.0f, v = 0.0f;
        if (lane < K) {
            x = work[i].data[lane][0];
            y = work[i].data[lane][1];
            v = work[i].data[lane][2];
        }
        const bool low = lane < K && v < kt;
        if (low) x = y = v = 0.0f;
        const double sc = ann_score_lanes(L, v, K);
        float ax = rl_f(x, 0), ay = rl_f(y, 0);
        for (int j = 1; j < K; j++) {
            const float bx = rl_f(x, j), by = rl_f(y, j);
            ax = bx > ax ? bx : ax;
            ay = by > ay ? by : ay;
        }
        if (low) {
            work[i].data[lane][0] = 0.0f;
            work[i].data[lane][1] = 0.0f;
            work[i].data[lane][2] = 0.0f;
        }
        if (lane == 0) {
            s_sc[i] = sc;
            amax[i] = ax;
            amax[cap + i] = ay;
        }
    }
    __syncthreads();
    STAMP(2);
    // the keep list in work order with the occupancy shape (nms.py:27-31) and the sort
    // (nms.py:33), lane i for annotation i
    if (wave == 0) {
        const double sc = lane < n ? s_sc[lane] : 0.0;
        const bool k = lane < n && sc >= it;
        float ax = 0.0f, ay = 0.0f;
        if (k) {
            ax = amax[lane];
            ay = amax[cap + lane];
        }
        const uint64_t km = __ballot(k);
        int m = 0;
        float mx = 0.0f, my = 0.0f;
        for (uint64_t rest = km; rest; rest &= rest - 1) {  // in order (NaN behaviour)
            const int l = __ffsll((unsigned long long)rest) - 1;
            const float lx = rl_f(ax, l), ly = rl_f(ay, l);
            if (m == 0 || lx > mx) mx = lx;
            if (m == 0 || ly > my) my = ly;
            m++;
        }
        const int rank = nms_rank_lanes(km, -sc);
        if (k) s_ix[rank] = (uint8_t)lane;
        if (lane == 0) {
            s_m = m;
            s_mx = mx;
            s_my = my;
        }
    }
    __syncthreads();
    STAMP(3);
    const int m = s_m;
    int n_out = 0;
    if (m > 0) {
        // Occupancy((K, int(max y + 1), int(max x + 1)), 2, min_scale=4)
        const long oh = (long)((double)(long)(s_my + 1.0f) / g.cfg.occupancy_reduction);
        const long ow = (long)((double)(long)(s_mx + 1.0f) / g.cfg.occupancy_reduction);
        const OccGrid no = occ_grid(nullptr, K, (int)(oh > 0 ? oh : 0), (int)(ow > 0 ? ow : 0));
        // nms.py:34-45: wave w takes planes w, w + W, ...; their joints of the sorted
        // annotations in one round trip
        constexpr int kPlanes = (kKP + W - 1) / W;
        const int wi0 = lane < m ? s_ix[lane] : 0;
        float px[kPlanes], py[kPlanes], pv[kPlanes], ps[kPlanes];
#pragma unroll
        for (int u = 0; u < kPlanes; u++) {
            const int f = wave + u * W;
            px[u] = py[u] = pv[u] = ps[u] = 0.0f;
            if (f < K && lane < m) {
                px[u] = work[wi0].data[f][0];
                py[u] = work[wi0].data[f][1];
                pv[u] = work[wi0].data[f][2];
                ps[u] = work[wi0].joint_scales[f];
            }
        }
        // every plane's cells and boxes first (independent: their latencies overlap), then
        // the planes' loops.  A plane beyond K has no live lane and no box.
        int pcx[kPlanes], pcy[kPlanes], pbx[kPlanes], pby[kPlanes];
        int fixed = 0;  // the same for every plane below K: the grid is empty or it is not
#pragma unroll
        for (int u = 0; u < kPlanes; u++) {
            const int f = min(wave + u * W, K - 1);
            int box[4] = {0, 0, 0, 0};
            pcx[u] = pcy[u] = 0;
            fixed = occ_cell(no, f, px[u], py[u], red, pcx[u], pcy[u]);  // uniform
            const bool hb = wave + u * W < K && lane < m && !(pv[u] == 0.0f) &&
                            occ_box(g, no, f, px[u], py[u], ps[u], box);
            // (x0 | x1 << 16, y0 | y1 << 16); zero: covers nothing (x1 >= 1 with a box)
            pbx[u] = hb ? box[0] | (box[1] << 16) : 0;
            pby[u] = hb ? box[2] | (box[3] << 16) : 0;
        }
#pragma unroll
        for (int u = 0; u < kPlanes; u++) {
            const int f = wave + u * W;
            if (f < K) {
                const float v = pv[u];
                const int xi = pcx[u], yi = pcy[u], bxp = pbx[u], byp = pby[u];
                const bool live = lane < m && !(v == 0.0f);  // nms.py:37 skips v == 0
                const uint64_t lm = __ballot(live), bm = __ballot(bxp != 0);
                uint32_t row_lo = 0u, row_hi = 0u;
                if (fixed < 0) {
                    for (uint64_t rest = bm; rest; rest &= rest - 1) {  // all cells per box
                        const int q = __ffsll((unsigned long long)rest) - 1;
                        const int bx = rl_i(bxp, q), by = rl_i(byp, q);
                        const bool c = q < lane && xi >= (bx & 0xFFFF) && xi < (bx >> 16) &&
                                       yi >= (by & 0xFFFF) && yi < (by >> 16);
                        if (q < 32)
                            row_lo |= c ? 1u << q : 0u;
                        else
                            row_hi |= c ? 1u << (q - 32) : 0u;
                    }
                }
                // a cell that no earlier box covers is free whatever gets marked: its box
                // counts from the start (only later rows can hold its bit), the walk skips it
                const uint64_t nz = fixed < 0 ? __ballot((row_lo | row_hi) != 0u) : ~0ull;
                uint64_t marked = bm & lm & ~nz, supp = 0;
                for (uint64_t rest = lm & nz; rest; rest &= rest - 1) {  // in sorted order, scalar
                    const int r = __ffsll((unsigned long long)rest) - 1;
                    const uint64_t bit = 1ull << r;
                    const uint64_t row = (uint64_t)(uint32_t)rl_i((int)row_lo, r) |
                                         (uint64_t)(uint32_t)rl_i((int)row_hi, r) << 32;
                    const bool occupied = fixed < 0 ? (row & marked) != 0 : fixed == 1;
                    if (occupied)
                        supp |= bit;
                    else
                        marked |= bm & bit;
                }
                if ((supp >> lane) & 1ull) work[wi0].data[f][2] = v * g.cfg.nms_suppression;
            }
        }
        __syncthreads();
        STAMP(4);
        // nms.py:51-53 in sorted order: zero low joints, the scores again
        for (int r = wave; r < m; r += W) {
            const int wi = s_ix[r];
            float v = 0.0f;
            if (lane < K) v = work[wi].data[lane][2];
            const bool low = lane < K && v < kt;
            if (low) v = 0.0f;
            const double sc = ann_score_lanes(L, v, K);
            if (low) {
                work[wi].data[lane][0] = 0.0f;
                work[wi].data[lane][1] = 0.0f;
                work[wi].data[lane][2] = 0.0f;
            }
            if (lane == 0) s_sc[r] = sc;
        }
        __syncthreads();
        STAMP(6);
        // survivors in sorted order and the second sort (nms.py:53-54), lane r for rank r
        if (wave == 0) {
            const double sc = lane < m ? s_sc[lane] : 0.0;
            const int wi = lane < m ? s_ix[lane] : 0;
            const bool k = lane < m && sc >= it;
            const uint64_t km = __ballot(k);
            const int rank = nms_rank_lanes(km, -sc);
            wave_sync();  // every lane has read its slots
            if (k) {
                s_sc[rank] = sc;
                s_ix[rank] = (uint8_t)wi;
            }
            if (lane == 0) s_m2 = __popcll(km);
        }
        __syncthreads();
        STAMP(7);
        n_out = s_m2;
        for (int r = wave; r < n_out; r += W) {
            const int wi = s_ix[r];
            copy_ann(&out[r], &work[wi]);
            if (lane == 0) {
                out[r].score = s_sc[r];
                if (g.out_idx) g.out_idx[(int64_t)img * cap + r] = wi;
            }
        }
    }
    __syncthreads();
    STAMP(8);
    if (wave == 0) {
        STAMP_FLUSH(3);
    }
    return n_out;
}

// PHASE 0: the whole of nms.Keypoints.annotations in one launch (images of at most kNmsSmall
// annotations by nms_small, the others' suppression planes by nms_plane_boxes); 1: up to the
// sorted keep list, whose count and occupancy-grid shape go
// to the meta words (nms_planes_kernel runs the planes); 3: from the suppressed planes on.
template <int W, int PHASE = 0>
__global__ __launch_bounds__(64 * W) void nms_kernel(GrowArgs g) {
    __shared__ ScoreLDS Ls[W];
    __shared__ int s_m, s_m2, s_status;
    __shared__ float s_mx, s_my;
    const int img = blockIdx.x;
    const int K = g.K;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ScoreLDS &L = Ls[wave];
    pp_ann *work = g.work + (int64_t)img * g.ann_cap;
    pp_ann *out = g.out + (int64_t)img * g.ann_cap;
    const int n_anns = max(0, min(g.n_work[img], g.ann_cap));
    const int cap = g.ann_cap;
    int *keep = g.nms_idx + (int64_t)img * (4 * cap + g.ann_np);  // kept work indices
    int *surv = keep + cap;                                           // survivors
    int *flag = surv + cap;                                           // per-index pass flags
    int *perm2 = flag + cap;                                          // meta: m, grid h, w
    int *perm = perm2 + cap;                                          // sort permutation
    double *score = g.nms_score + (int64_t)img * 2 * cap;             // by work index
    double *kscore = score + cap;                                     // by kept / survivor rank
    float *amax = g.nms_f + (int64_t)img * 2 * cap;                   // per-ann max x, max y
    int2 *gbox = g.nms_box + ((int64_t)img * kNmsBoxLists + wave) * cap;
    const float red = (float)g.cfg.occupancy_reduction;
    const float kt = g.cfg.nms_keypoint_threshold;
    const double it = g.nms_it;
    if (threadIdx.x == 0) {
        s_status = g.status[img];
        g.complete_next[img] = 0;  // workspace contract: left zero
    }
    STAMP_DO(if (lane == 0) for (int q = 0; q < 8; q++) L.fst[q] = 0);
    __syncthreads();
    STAMP_DECL

    if (PHASE == 0 && !g.cfg.apply_nms) {
        for (int i = wave; i < n_anns; i += W) {
            copy_ann(&out[i], &work[i]);
            const double sc = nms_ann_score(g, L, img, i, work[i].data, K);
            if (lane == 0) {
                out[i].score = sc;
                if (g.out_idx) g.out_idx[(int64_t)img * cap + i] = i;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            g.counts[img] = n_anns;
            g.status[img] = s_status;
        }
        return;
    }

    if constexpr (PHASE == 0) {
        // uniform over the workgroup: every barrier below and in nms_small stays uniform
        if (n_anns <= kNmsSmall && !g.nms_spec) {
            const int n_small = nms_small<W>(g, L, img, work, out, n_anns, amax, s_m, s_m2, s_mx, s_my);
            if (threadIdx.x == 0) {
                g.counts[img] = n_small;
                g.status[img] = s_status;
            }
            return;
        }
    }

    int m = 0;
    if constexpr (PHASE != 3) {
    // nms.py:20-22: zero joints below keypoint_threshold, drop low scores (per annotation)
    for (int i = wave; i < n_anns; i += W) {
        pp_ann &a = work[i];
        if (lane < K && a.data[lane][2] < kt) {
            a.data[lane][0] = 0.0f;
            a.data[lane][1] = 0.0f;
            a.data[lane][2] = 0.0f;
        }
        wave_sync();
        const double sc = nms_ann_score(g, L, img, i, a.data, K);
        if (lane == 0) {
            float ax = a.data[0][0], ay = a.data[0][1];
            for (int j = 1; j < K; j++) {
                ax = a.data[j][0] > ax ? a.data[j][0] : ax;
                ay = a.data[j][1] > ay ? a.data[j][1] : ay;
            }
            score[i] = sc;
            flag[i] = sc >= it;
            amax[i] = ax;
            amax[cap + i] = ay;
        }
    }
    __syncthreads();
    STAMP(2);
    // keep list in work order + the occupancy shape (nms.py:27-31), then the stable sort
    if (wave == 0) {
        int m = 0;
        float mx = 0.0f, my = 0.0f;
        for (int i0 = 0; i0 < n_anns; i0 += 64) {
            const int i = i0 + lane;
            const bool k = i < n_anns && flag[i];
            float ax = 0.0f, ay = 0.0f;
            double sc = 0.0;
            if (k) {
                ax = amax[i];
                ay = amax[cap + i];
                sc = score[i];
            }
            const uint64_t km = __ballot(k);
            if (k) {
                const int r = m + lane_prefix(km);
                keep[r] = i;
                kscore[r] = sc;
            }
            uint64_t rest = km;
            while (rest) {  // max over the kept annotations, in order (NaN behaviour)
                const int l = __ffsll((unsigned long long)rest) - 1;
                rest &= rest - 1;
                const float lx = rl_f(ax, l), ly = rl_f(ay, l);
                if (m == 0 || lx > mx) mx = lx;
                if (m == 0 || ly > my) my = ly;
                m++;
            }
        }
        wave_sync();
        if (m > 0) {
            int np = 1;
            while (np < m) np <<= 1;
            sort_by_score(perm, np, m, kscore);  // nms.py:33 (stable)
        }
        if (lane == 0) {
            s_m = m;
            s_mx = mx;
            s_my = my;
        }
    }
    __syncthreads();
    STAMP(3);
    m = s_m;
    } else {
        m = perm2[0];
    }
    if constexpr (PHASE == 1) {
        if (threadIdx.x == 0) {
            perm2[0] = m;
            perm2[1] = perm2[2] = 0;
            if (m > 0) {  // Occupancy((K, int(max y + 1), int(max x + 1)), 2, min_scale=4)
                const long oh = (long)((double)(long)(s_my + 1.0f) / g.cfg.occupancy_reduction);
                const long ow = (long)((double)(long)(s_mx + 1.0f) / g.cfg.occupancy_reduction);
                perm2[1] = (int)(oh > 0 ? oh : 0);
                perm2[2] = (int)(ow > 0 ? ow : 0);
            }
        }
        return;
    }
    int n_out = 0;
    if (m > 0) {
        if constexpr (PHASE == 0) {
        // Occupancy((K, int(max y + 1), int(max x + 1)), 2, min_scale=4)
        const long oh = (long)((double)(long)(s_my + 1.0f) / g.cfg.occupancy_reduction);
        const long ow = (long)((double)(long)(s_mx + 1.0f) / g.cfg.occupancy_reduction);
        const OccGrid no = occ_grid(nullptr, K, (int)(oh > 0 ? oh : 0), (int)(ow > 0 ? ow : 0));
        // the first 64 sorted annotations' joints of every plane this wave walks, loaded in
        // one round trip (their work indices in one more) instead of three per plane
        constexpr int kNmsPre = 4;  // planes per wave prefetched (K <= 32)
        int wi0 = 0;
        float pre[kNmsPre][4];
        if (lane < m) wi0 = keep[perm[lane]];
#pragma unroll
        for (int u = 0; u < kNmsPre; u++) {
            const int f = wave + u * W;
            pre[u][0] = pre[u][1] = pre[u][2] = pre[u][3] = 0.0f;
            if (f < K && lane < m) {
                pre[u][0] = work[wi0].data[f][0];
                pre[u][1] = work[wi0].data[f][1];
                pre[u][2] = work[wi0].data[f][2];
                pre[u][3] = work[wi0].joint_scales[f];
            }
        }
        for (int f = wave, u = 0; f < K; f += W, u++) {  // nms.py:34-45, one plane per pass
            nms_plane_boxes(g, work, m, f, no, red, gbox, [&](int r0, int &wi, float &jx, float &jy,
                                                                float &jv, float &js) {
                const int r = r0 + lane;
                if (r0 == 0 && u < kNmsPre) {  // prefetched (selects: no dynamic index)
                    wi = wi0;
#pragma unroll
                    for (int w = 0; w < kNmsPre; w++)
                        if (w == u) {
                            jx = pre[w][0];
                            jy = pre[w][1];
                            jv = pre[w][2];
                            js = pre[w][3];
                        }
                } else if (r < m) {
                    wi = keep[perm[r]];
                    jx = work[wi].data[f][0];
                    jy = work[wi].data[f][1];
                    jv = work[wi].data[f][2];
                    js = work[wi].joint_scales[f];
                }
            });
        }
        __syncthreads();
        STAMP(4);
        }
        // nms.py:51-53 in sorted order: zero low joints, drop low scores
        for (int r = wave; r < m; r += W) {
            const int wi = keep[perm[r]];
            pp_ann &a = work[wi];
            if (lane < K && a.data[lane][2] < kt) {
                a.data[lane][0] = 0.0f;
                a.data[lane][1] = 0.0f;
                a.data[lane][2] = 0.0f;
            }
            wave_sync();
            const double sc = nms_ann_score(g, L, img, wi, a.data, K);
            if (lane == 0) {
                flag[r] = sc >= it;
                score[r] = sc;  // by sorted rank now (the work-index scores are consumed)
            }
        }
        __syncthreads();
        STAMP(6);
        if (wave == 0) {
            int m2 = 0;
            for (int r0 = 0; r0 < m; r0 += 64) {
                const int r = r0 + lane;
                const bool k = r < m && flag[r];
                int wi = 0;
                double sc = 0.0;
                if (k) {
                    wi = keep[perm[r]];
                    sc = score[r];
                }
                const uint64_t km = __ballot(k);
                if (k) {
                    const int q = m2 + lane_prefix(km);
                    surv[q] = wi;
                    kscore[q] = sc;
                }
                m2 += __popcll(km);
            }
            wave_sync();
            if (m2 > 0) {
                int np2 = 1;
                while (np2 < m2) np2 <<= 1;
                sort_by_score(perm, np2, m2, kscore);  // nms.py:54
            }
            if (lane == 0) s_m2 = m2;
        }
        __syncthreads();
        STAMP(7);
        n_out = s_m2;
        for (int r = wave; r < n_out; r += W) {
            copy_ann(&out[r], &work[surv[perm[r]]]);
            if (lane == 0) {
                out[r].score = kscore[perm[r]];
                if (g.out_idx) g.out_idx[(int64_t)img * cap + r] = surv[perm[r]];
            }
        }
    }
    __syncthreads();
    STAMP(8);
    if (wave == 0) {
        STAMP_FLUSH(3);
    }
    if (threadIdx.x == 0) {
        g.counts[img] = n_out;
        g.status[img] = s_status;
    }
}

// ---- nms.py:34-45 per (image, plane), the plane's occupancy as a bitmap in LDS ----
// Between nms_kernel<W, 1> (the sorted keep list, its count and grid shape in the meta words)
// and nms_kernel<W, 3> (the refilter and output): one wave per (image, joint plane), walking
// the image's kept annotations in sorted order.  The reference's grid holds u8 counts and a
// joint is occupied iff its cell's count is non-zero (mod 256: += 1 wraps).  Here a cell is
// one bit, set when a marked box covers it: the same answer while no cell is covered by 256
// boxes or more.  Counts of the boxes meeting each 32 x 32-cell block (never below any of
// its cells' counts) guard that: a plane where a block reaches 256 boxes is decided again by
// nms_plane_boxes (the exact counting form), which also takes grids larger than the LDS
// bitmap (keypoints far outside the field).  Suppressed joints are written only after the
// plane is decided.  A check is one LDS word, a mark one OR per (box row, word): O(m) per
// plane instead of nms_plane_boxes' O(m * marked boxes / 64).
constexpr int kNmsBlk = 32;

struct NmsBitmapGeo {  // the LDS bitmap's capacity (the launch's dynamic LDS)
    int cap_h, cap_w;  // grid rows and columns it holds
    __host__ __device__ int wpr() const { return (cap_w + 31) >> 5; }
    __host__ __device__ int blocks() const {
        return ((cap_h + kNmsBlk - 1) / kNmsBlk) * ((cap_w + kNmsBlk - 1) / kNmsBlk);
    }
    __host__ __device__ size_t bytes(int ann_cap) const {
        return sizeof(uint32_t) * ((size_t)cap_h * wpr() + blocks() + (ann_cap + 31) / 32);
    }
};

__global__ __launch_bounds__(64) void nms_planes_kernel(GrowArgs g, NmsBitmapGeo geo) {
    extern __shared__ uint32_t s_bm[];
    const int img = blockIdx.x, f = blockIdx.y;
    const int lane = threadIdx.x;
    const int K = g.K, cap = g.ann_cap;
    pp_ann *work = g.work + (int64_t)img * cap;
    const int *keep = g.nms_idx + (int64_t)img * (4 * cap + g.ann_np);
    const int *meta = keep + 3 * cap;  // nms_kernel<W, 1>: m, grid h, grid w
    const int *perm = meta + cap;
    const int m = meta[0], oh = meta[1], ow = meta[2];
    if (m <= 0 || f >= K) return;
    const float red = (float)g.cfg.occupancy_reduction;
    const OccGrid no = occ_grid(nullptr, K, oh, ow);
    auto load = [&](int r0, int &wi, float &jx, float &jy, float &jv, float &js) {
        const int r = r0 + lane;
        if (r < m) {
            wi = keep[perm[r]];
            jx = work[wi].data[f][0];
            jy = work[wi].data[f][1];
            jv = work[wi].data[f][2];
            js = work[wi].joint_scales[f];
        }
    };
    int2 *gbox = g.nms_box + ((int64_t)img * kNmsBoxLists + f) * cap;
    if (oh <= 0 || ow <= 0 || oh > geo.cap_h || ow > geo.cap_w) {
        nms_plane_boxes(g, work, m, f, no, red, gbox, load);
        return;
    }
    const int wpr = (ow + 31) >> 5;
    const int bcols = (ow + kNmsBlk - 1) / kNmsBlk;
    uint32_t *bits = s_bm;                                // oh rows of wpr words
    uint32_t *bcnt = s_bm + (size_t)geo.cap_h * geo.wpr();  // boxes per block
    uint32_t *supp = bcnt + geo.blocks();                   // suppressed ranks
    const int nbits = oh * wpr, nblk = ((oh + kNmsBlk - 1) / kNmsBlk) * bcols;
    for (int i = lane; i < nbits; i += 64) bits[i] = 0u;
    for (int i = lane; i < nblk; i += 64) bcnt[i] = 0u;
    for (int i = lane; i < (m + 31) / 32; i += 64) supp[i] = 0u;
    wave_sync();
    bool over = false;
    for (int r0 = 0; r0 < m; r0 += 64) {
        int wi = 0;
        float jx = 0.0f, jy = 0.0f, jv = 0.0f, js = 0.0f;
        load(r0, wi, jx, jy, jv, js);
        // per lane: its joint's cell, and the box it marks when free (0: none)
        int xi = 0, yi = 0;
        (void)occ_cell(no, f, jx, jy, red, xi, yi);  // -1: f < K and a non-empty grid
        int box[4] = {0, 0, 0, 0};
        const bool hb = r0 + lane < m && jv != 0.0f && occ_box(g, no, f, jx, jy, js, box);
        const int cellp = xi | (yi << 16);
        const int bxp = hb ? box[0] | (box[1] << 16) : 0;  // x1 >= 1 when hb: nonzero
        const int byp = box[2] | (box[3] << 16);
        const int nr = min(64, m - r0);
        for (int l = 0; l < nr; l++) {
            if (rl_f(jv, l) == 0.0f) continue;
            const int cp = rl_i(cellp, l);
            const int cx = cp & 0xFFFF, cy = cp >> 16;
            if ((bits[cy * wpr + (cx >> 5)] >> (cx & 31)) & 1u) {  // occupied
                if (lane == 0) atomicOr(&supp[(r0 + l) >> 5], 1u << ((r0 + l) & 31));
                continue;
            }
            const int bx = rl_i(bxp, l);
            if (bx == 0) continue;  // no box (empty after clipping)
            const int by = rl_i(byp, l);
            const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
            const int w0 = x0 >> 5, nw = ((x1 - 1) >> 5) - w0 + 1;
            const int items = (y1 - y0) * nw;
            for (int t = lane; t < items; t += 64) {  // (box row, word) pairs
                const int ry = y0 + t / nw, wq = w0 + t % nw;
                const int lo = max(x0 - 32 * wq, 0), hi = min(x1 - 32 * wq, 32);
                const uint32_t mk = (hi - lo >= 32) ? ~0u : (((1u << (hi - lo)) - 1u) << lo);
                atomicOr(&bits[ry * wpr + wq], mk);
            }
            const int bx0 = x0 / kNmsBlk, bx1 = (x1 - 1) / kNmsBlk;
            const int by0 = y0 / kNmsBlk, by1 = (y1 - 1) / kNmsBlk;
            const int nbk = (bx1 - bx0 + 1) * (by1 - by0 + 1);
            for (int t = lane; t < nbk; t += 64) {  // the guard: boxes per block
                const int bq = (by0 + t / (bx1 - bx0 + 1)) * bcols + bx0 + t % (bx1 - bx0 + 1);
                over |= atomicAdd(&bcnt[bq], 1u) >= 255u;
            }
            wave_sync();  // the marks before the next check
        }
    }
    if (__ballot(over)) {  // a cell may have wrapped: decide the plane by counting
        nms_plane_boxes(g, work, m, f, no, red, gbox, load);
        return;
    }
    for (int r = lane; r < m; r += 64)  // nms.py:43: data[f, 2] *= suppression
        if ((supp[r >> 5] >> (r & 31)) & 1u) {
            float *v = &work[keep[perm[r]]].data[f][2];
            *v = *v * g.cfg.nms_suppression;
        }
}

// nms.Keypoints (nms.py:17-57) of a decode: nms_kernel<W> in one launch, or with `bitmap`
// (PP_STAGE_NMS_BITMAP) nms_kernel<W, 1>, the planes as
// bitmaps (nms_planes_kernel, one wave per (image, plane)), nms_kernel<W, 3> -- unless NMS
// is off or the bitmap would not fit kNmsBitmapLds.  `wide`: 8-wave workgroups
// (PP_STAGE_NMS_WIDE).  The bitmap holds the nominal grid (CifHr map / reduction) plus
// kNmsMargin cells; an image whose keypoints reach further takes nms_plane_boxes in the
// plane kernel.  Measured (round 5, one box): the three launches take 60 vs 76 us per planted
// cfg3 step and 1.48 vs 2.51 ms per uniform one, one step at a time; but in the overlapped
// pipeline planted 397k-402k vs 405k-410k and uniform 14.7k vs 15.5k-15.8k images/s (the
// 4352 one-wave workgroups of the plane kernel beside the next batch's seed loop), so the
// single launch stays the default.
constexpr int kNmsMargin = 16;
constexpr size_t kNmsBitmapLds = 64 * 1024;

int launch_nms(const GrowArgs &g, int n_img, bool wide, bool bitmap, hipStream_t s) {
    NmsBitmapGeo geo{};
    geo.cap_h = (int)((double)g.hh / g.cfg.occupancy_reduction) + kNmsMargin;
    geo.cap_w = (int)((double)g.ww / g.cfg.occupancy_reduction) + kNmsMargin;
    const size_t lds = geo.bytes(g.ann_cap);
    if (bitmap && g.cfg.apply_nms && lds <= kNmsBitmapLds) {
        if (wide)
            hipLaunchKernelGGL((nms_kernel<kNmsWaves, 1>), dim3(n_img), dim3(64 * kNmsWaves), 0, s, g);
        else
            hipLaunchKernelGGL((nms_kernel<kNmsNarrow, 1>), dim3(n_img), dim3(64 * kNmsNarrow), 0, s, g);
        hipLaunchKernelGGL(nms_planes_kernel, dim3(n_img, g.K), dim3(64), lds, s, g, geo);
        if (wide)
            hipLaunchKernelGGL((nms_kernel<kNmsWaves, 3>), dim3(n_img), dim3(64 * kNmsWaves), 0, s, g);
        else
            hipLaunchKernelGGL((nms_kernel<kNmsNarrow, 3>), dim3(n_img), dim3(64 * kNmsNarrow), 0, s, g);
        return check_launch("pp_decode_batch(nms)");
    }
    if (wide)
        hipLaunchKernelGGL(nms_kernel<kNmsWaves>, dim3(n_img), dim3(64 * kNmsWaves), 0, s, g);
    else
        hipLaunchKernelGGL(nms_kernel<kNmsNarrow>, dim3(n_img), dim3(64 * kNmsNarrow), 0, s, g);
    return check_launch("pp_decode_batch(nms)");
}

}  // namespace pp

using namespace pp;

extern "C" {

// ---- standalone nms.Keypoints.annotations (nms.py:17-57) over caller records ----------
namespace {
struct NmsLayout {
    size_t off_status, off_wq, off_score, off_idx, off_f, off_box, total;
    int ann_np;
};
NmsLayout nms_layout(int n_img, int cap) {
    NmsLayout l{};
    l.ann_np = 1;
    while (l.ann_np < cap) l.ann_np <<= 1;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes);
        return at;
    };
    const size_t n = (size_t)n_img;
    l.off_status = take(n * sizeof(int));
    l.off_wq = take(n * sizeof(int));
    l.off_score = take(n * 2 * cap * sizeof(double));
    l.off_idx = take(n * (4 * (size_t)cap + l.ann_np) * sizeof(int));
    l.off_f = take(n * 2 * cap * sizeof(float));
    l.off_box = take(n * kNmsWaves * (size_t)cap * sizeof(int2));
    l.total = o;
    return l;
}
}  // namespace

size_t pp_nms_workspace_size(int32_t n_img, int32_t ann_capacity) {
    if (n_img < 0 || ann_capacity <= 0) return 0;
    return nms_layout(n_img, ann_capacity).total;
}

int pp_nms_keypoints(pp_ann *d_anns, const int32_t *d_counts, int32_t n_img, int32_t K,
                     int32_t ann_capacity, const pp_config *cfg, pp_ann *d_out,
                     int32_t *d_out_counts, int32_t *d_out_index, void *d_workspace,
                     size_t workspace_bytes, void *stream) {
    if (!cfg) return fail(PP_EINVAL, "pp_nms_keypoints: NULL argument");
    return pp_nms_keypoints_scored(d_anns, d_counts, n_img, K, ann_capacity, cfg,
                                   (double)cfg->nms_instance_threshold, nullptr, nullptr,
                                   nullptr, d_out, d_out_counts, d_out_index, d_workspace,
                                   workspace_bytes, stream);
}

int pp_nms_keypoints_scored(pp_ann *d_anns, const int32_t *d_counts, int32_t n_img, int32_t K,
                            int32_t ann_capacity, const pp_config *cfg,
                            double instance_threshold, const int32_t *d_score_spec, const double *d_score_weights,
                            const double *d_fixed_score, pp_ann *d_out, int32_t *d_out_counts,
                            int32_t *d_out_index, void *d_workspace, size_t workspace_bytes,
                            void *stream) {
    if (!d_anns || !d_counts || !cfg || !d_out || !d_out_counts || !d_workspace)
        return fail(PP_EINVAL, "pp_nms_keypoints: NULL argument");
    if (d_score_spec && (!d_score_weights || !d_fixed_score))
        return fail(PP_EINVAL, "pp_nms_keypoints_scored: d_score_spec needs the weights and "
                               "fixed scores");
    if (n_img < 0 || K <= 0 || K > PP_MAX_KP || ann_capacity <= 0 || cfg->occupancy_reduction <= 0)
        return fail(PP_ESHAPE, "pp_nms_keypoints: shape outside the supported envelope");
    if (n_img == 0) return PP_OK;
    const NmsLayout l = nms_layout(n_img, ann_capacity);
    if (workspace_bytes < l.total) return fail(PP_ENOMEM, "pp_nms_keypoints: workspace too small");
    char *ws = (char *)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    GrowArgs g{};
    g.K = K;
    g.cfg = *cfg;
    g.cfg.apply_nms = 1;
    g.work = d_anns;
    g.n_work = const_cast<int *>(d_counts);
    g.ann_cap = ann_capacity;
    g.ann_np = l.ann_np;
    g.status = (int *)(ws + l.off_status);
    g.complete_next = (int *)(ws + l.off_wq);
    g.nms_score = (double *)(ws + l.off_score);
    g.nms_idx = (int *)(ws + l.off_idx);
    g.nms_f = (float *)(ws + l.off_f);
    g.nms_box = (int2 *)(ws + l.off_box);
    g.nms_spec = d_score_spec;
    g.nms_sw = d_score_weights;
    g.nms_fixed = d_fixed_score;
    g.nms_it = instance_threshold;
    g.out = d_out;
    g.counts = d_out_counts;
    g.out_idx = d_out_index;
    if (hipMemsetAsync(g.status, 0, (size_t)n_img * sizeof(int), s) != hipSuccess)
        return fail(PP_EHIP, "pp_nms_keypoints: memset failed");
    hipLaunchKernelGGL(nms_kernel<kNmsWaves>, dim3(n_img), dim3(64 * kNmsWaves), 0, s, g);
    return check_launch("pp_nms_keypoints");
}

}  // extern "C"

// encode_plan.hip — the host's share of the CIF / CAF target encoders: the argument checks
// and the per-annotation scalars of openpifpaf/encoder/annrescaler.py, cif.py and caf.py,
// restated operation by operation with NumPy 2's result types (a Python float is "weak":
// float32 op Python float stays float32; float32 op NumPy float64 is float64), nothing
// fused.  The result is a job list per (image, field) in the reference's order, which the
// kernel (encode.hip) and the host twins (encode_cpu.hip) rasterise.
#pragma clang fp contract(off)
#include "encode.hpp"

#include <cmath>
#include <cstring>
#include <limits>

namespace pp {

namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();

struct Kp {
    float x, y, v;
};

// a NumPy scalar that is float32 or float64 (or the Python float nan)
struct Num {
    double v;
    bool f32;
};

// annrescaler.py:77-109 AnnRescaler.scale
Num ann_scale(const Kp *kp, int K, const double *pose, const double *pose45, double total,
              double total45) {
    const double nan = std::nan("");
    int n = 0;
    float x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    double p[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    bool xn = false, yn = false;
    for (int k = 0; k < K; k++) {
        if (!(kp[k].v > 0.0f)) continue;  // :78
        const double px = pose[2 * k], py = pose[2 * k + 1];
        const double qx = pose45[2 * k], qy = pose45[2 * k + 1];
        xn = xn || kp[k].x != kp[k].x;
        yn = yn || kp[k].y != kp[k].y;
        if (n == 0) {
            x0 = x1 = kp[k].x, y0 = y1 = kp[k].y;
            p[0] = p[1] = px, p[2] = p[3] = py;
            q[0] = q[1] = qx, q[2] = q[3] = qy;
        } else {
            x0 = kp[k].x < x0 ? kp[k].x : x0, x1 = kp[k].x > x1 ? kp[k].x : x1;
            y0 = kp[k].y < y0 ? kp[k].y : y0, y1 = kp[k].y > y1 ? kp[k].y : y1;
            p[0] = px < p[0] ? px : p[0], p[1] = px > p[1] ? px : p[1];
            p[2] = py < p[2] ? py : p[2], p[3] = py > p[3] ? py : p[3];
            q[0] = qx < q[0] ? qx : q[0], q[1] = qx > q[1] ? qx : q[1];
            q[2] = qy < q[2] ? qy : q[2], q[3] = qy > q[3] ? qy : q[3];
        }
        n++;
    }
    if (n < 3) return {nan, false};  // :79-80
    // :82-85 float32; np.max / np.min propagate NaN
    const float dx = xn ? std::nanf("") : x1 - x0, dy = yn ? std::nanf("") : y1 - y0;
    const float area = dx * dy;
    const double area_ref = (p[1] - p[0]) * (p[3] - p[2]);       // :86-89
    const double area_ref_45 = (q[1] - q[0]) * (q[3] - q[2]);    // :90-93
    const double a = area_ref > 0.1 ? total / area_ref : kInf;   // :96
    const double b = area_ref_45 > 0.1 ? total45 / area_ref_45 : kInf;
    const double factor = sqrt(b < a ? b : a);                   // :95 Python min
    if (std::isinf(factor)) return {nan, false};                 // :99-100
    Num scale;
    if (factor < 5.0) {  // :102 min(5.0, factor) is the NumPy float64
        scale = {(double)sqrtf(area) * factor, false};
    } else {             // ... or the Python float 5.0: float32
        const float s = sqrtf(area) * 5.0f;
        scale = {(double)s, true};
    }
    if (scale.v < 0.1) return {nan, false};  // :104-105
    return scale;
}

// cif.py:87-101 max_r: the nearest other annotation's joint by quadrant, float32
void max_r(const Kp *sets, int n_sets, int K, int self, int joint, double thr, float out[4]) {
    const float inf = std::numeric_limits<float>::infinity();
    out[0] = out[1] = out[2] = out[3] = inf;
    const Kp &me = sets[(size_t)self * K + joint];
    for (int o = 0; o < n_sets; o++) {
        if (o == self) continue;
        const Kp &k = sets[(size_t)o * K + joint];
        if (!((double)k.v > thr)) continue;
        const float dx = k.x - me.x, dy = k.y - me.y;  // :94
        const int q = (dx < 0.0f ? 1 : 0) + (dy < 0.0f ? 2 : 0);
        const float d = norm2_f32(dx, dy);             // :99 (axis=1: sqrt(sum(x * x)))
        out[q] = d < out[q] ? d : out[q];
    }
}

// cif.py:113-114, caf.py:153-159: scale * sigmas[f], then np.min([., np.min(max_r) * 0.25])
float joint_scale(Num scale, const double *sigmas, int joint, const float mr[4]) {
    Num js = scale;
    if (sigmas && js.v == js.v) {
        if (js.f32) {
            const float t = (float)js.v * (float)sigmas[joint];
            js.v = (double)t;
        } else {
            js.v = js.v * sigmas[joint];
        }
    }
    float m = mr[0];
    for (int q = 1; q < 4; q++) m = mr[q] < m ? mr[q] : m;
    const float cap = m * 0.25f;
    if (js.v != js.v) return f32_of(kNaN);  // np.min propagates NaN
    const double r = (double)cap < js.v ? (double)cap : js.v;
    return (float)r;
}

int checked_int(double v) {  // int() of a value known to be finite; far values saturate
    if (v > 1e9) return 1000000000;
    if (v < -1e9) return -1000000000;
    return (int)v;
}

}  // namespace

size_t encode_tables_bound(int32_t n_img, int32_t n_ann, int32_t F, bool is_caf) {
    if (n_img <= 0 || n_ann < 0 || F <= 0) return 0;
    const size_t job = is_caf ? sizeof(CafJob) : sizeof(CifJob);
    return (size_t)n_img * sizeof(EncImage) + (size_t)round_up(((int64_t)n_img * F + 1) * 4, 8) +
           (size_t)n_ann * sizeof(EncBox) + (size_t)n_ann * F * job;
}

void EncPlan::layout(bool is_caf) {
    off_fj = images.size() * sizeof(EncImage);
    off_boxes = off_fj + (size_t)round_up((int64_t)fj.size() * 4, 8);
    off_jobs = off_boxes + boxes.size() * sizeof(EncBox);
    bytes = off_jobs + (is_caf ? caf.size() * sizeof(CafJob) : cif.size() * sizeof(CifJob));
}

void EncPlan::stage(char *dst, bool is_caf) const {
    memcpy(dst, images.data(), images.size() * sizeof(EncImage));
    memcpy(dst + off_fj, fj.data(), fj.size() * 4);
    if (!boxes.empty()) memcpy(dst + off_boxes, boxes.data(), boxes.size() * sizeof(EncBox));
    if (is_caf && !caf.empty()) memcpy(dst + off_jobs, caf.data(), caf.size() * sizeof(CafJob));
    if (!is_caf && !cif.empty()) memcpy(dst + off_jobs, cif.data(), cif.size() * sizeof(CifJob));
}

int encode_plan(const char *who, bool is_caf, const pp_encoder *enc, const pp_enc_image *images,
                int32_t n_img, const pp_enc_ann *anns, const float *keypoints, int32_t n_ann,
                const void *out, int64_t out_elems, EncPlan *plan) {
    const std::string w(who);
    if (!enc) return fail(PP_EINVAL, w + ": NULL argument");
    if (!enc->pose || !enc->pose_45 || (is_caf && !enc->skeleton) ||
        (is_caf && enc->n_sparse > 0 && !enc->sparse_skeleton))
        return fail(PP_EINVAL, w + ": NULL argument");
    const int K = enc->K, C = enc->C, F = is_caf ? C : K;
    if (K < 1 || K > PP_MAX_KP) return fail(PP_ESHAPE, w + ": K outside [1, PP_MAX_KP]");
    if (is_caf && (C < 1 || C > PP_MAX_EDGES))
        return fail(PP_ESHAPE, w + ": C outside [1, PP_MAX_EDGES]");
    if (is_caf && enc->aspect_ratio != 0.0)
        return fail(PP_EINVAL, w + ": aspect_ratio != 0 is not built");
    if (enc->side < 1 || enc->side > 8) return fail(PP_ESHAPE, w + ": side outside 1..8");
    if (enc->padding < 0 || enc->padding > 64) return fail(PP_ESHAPE, w + ": padding outside 0..64");
    if (enc->stride < 1) return fail(PP_ESHAPE, w + ": stride < 1");
    if (n_img < 0 || n_ann < 0) return fail(PP_ESHAPE, w + ": negative count");
    if (is_caf) {
        if (enc->n_sparse < 0) return fail(PP_ESHAPE, w + ": negative count");
        for (int e = 0; e < 2 * C; e++)
            if (enc->skeleton[e] < 1 || enc->skeleton[e] > K)
                return fail(PP_ESHAPE, w + ": skeleton joint index out of 1..K");
        for (int e = 0; e < 2 * enc->n_sparse; e++)
            if (enc->sparse_skeleton[e] < 1 || enc->sparse_skeleton[e] > K)
                return fail(PP_ESHAPE, w + ": skeleton joint index out of 1..K");
    }
    if (n_img == 0) return PP_OK;
    if (!images || !out || (n_ann > 0 && (!anns || !keypoints)))
        return fail(PP_EINVAL, w + ": NULL argument");
    if ((uintptr_t)out & 3u) return fail(PP_EINVAL, w + ": misaligned output");
    if (out_elems < 0) return fail(PP_ESHAPE, w + ": negative buffer size");

    const int side = enc->side, padding = enc->padding;
    const double thr = enc->v_threshold;
    const double so = ((double)side - 1.0) / 2.0;
    const float stride_f = (float)enc->stride;
    // annrescaler.py:13-16, 23-26
    double pr[8];
    for (int k = 0; k < K; k++)
        for (int c = 0; c < 2; c++) {
            const double a = enc->pose[2 * k + c], b = enc->pose_45[2 * k + c];
            if (k == 0) pr[2 * c] = pr[2 * c + 1] = a, pr[4 + 2 * c] = pr[5 + 2 * c] = b;
            pr[2 * c] = a < pr[2 * c] ? a : pr[2 * c];
            pr[2 * c + 1] = a > pr[2 * c + 1] ? a : pr[2 * c + 1];
            pr[4 + 2 * c] = b < pr[4 + 2 * c] ? b : pr[4 + 2 * c];
            pr[5 + 2 * c] = b > pr[5 + 2 * c] ? b : pr[5 + 2 * c];
        }
    const double total = (pr[1] - pr[0]) * (pr[3] - pr[2]);
    const double total45 = (pr[5] - pr[4]) * (pr[7] - pr[6]);

    plan->F = F;
    plan->images.assign((size_t)n_img, EncImage{});
    plan->fj.assign((size_t)n_img * F + 1, 0);
    int64_t blocks = 0;
    std::vector<Kp> sets;
    std::vector<int> field_of;  // of each job of the image, in the reference's order
    std::vector<CifJob> cif_jobs;
    std::vector<CafJob> caf_jobs;
    std::vector<int> count((size_t)F + 1);

    for (int i = 0; i < n_img; i++) {
        const pp_enc_image &im = images[i];
        EncImage &m = plan->images[(size_t)i];
        if (im.height < 1 || im.width < 1 || im.h != (im.height - 1) / enc->stride + 1 ||
            im.w != (im.width - 1) / enc->stride + 1)  // annrescaler.py:51-54
            return fail(PP_ESHAPE, w + ": field size is not the pixel size's");
        if (im.h > kEncMaxSide || im.w > kEncMaxSide)
            return fail(PP_ESHAPE, w + ": field beyond 16384 cells per side");
        if (im.n_ann < 0 || im.ann0 < 0 || im.ann0 > n_ann || im.n_ann > n_ann - im.ann0)
            return fail(PP_ESHAPE, w + ": annotation range outside the table");
        const int64_t hw = (int64_t)im.h * im.w;
        const int n_out = is_caf ? 5 : 3;
        for (int t = 0; t < n_out; t++) {
            const int64_t planes = (is_caf ? (t == 1 || t == 2) : t == 1) ? 6 : 1;
            const int64_t n = planes * F * hw;
            if (im.out_offset[t] < 0 || im.out_offset[t] > out_elems ||
                n > out_elems - im.out_offset[t])
                return fail(PP_ESHAPE, w + ": an output region beyond the output buffer");
            m.out_offset[t] = im.out_offset[t];
        }
        m.h = im.h, m.w = im.w;
        m.bpp = (int32_t)((hw + kEncBlock - 1) / kEncBlock);
        m.block0 = (int32_t)blocks;
        blocks += (int64_t)m.bpp * F;
        if (blocks > INT32_MAX) return fail(PP_ESHAPE, w + ": too many cells for one launch");
        m.fj0 = i * F;

        // utils.py:19-37 mask_valid_area with annrescaler.py:28-37 valid_area / stride
        m.y_lo = m.x_lo = 0, m.y_hi = im.h, m.x_hi = im.w;
        if (im.has_valid_area) {
            double va[4];
            for (int c = 0; c < 4; c++) {
                va[c] = im.valid_area[c] / (double)enc->stride;
                if (!std::isfinite(va[c])) return fail(PP_EINVAL, w + ": valid_area not finite");
            }
            if (va[1] >= 1.0) m.y_lo = checked_int(va[1]);
            if (va[0] >= 1.0) m.x_lo = checked_int(va[0]);
            const int max_i = checked_int(ceil(va[1] + va[3])) + 1;
            const int max_j = checked_int(ceil(va[0] + va[2])) + 1;
            if (0 < max_i && max_i < im.h) m.y_hi = max_i;
            if (0 < max_j && max_j < im.w) m.x_hi = max_j;
        }

        // annrescaler.py:39-47 keypoint_sets and :49-75 bg_mask
        sets.clear();
        m.box0 = (int32_t)plan->boxes.size();
        for (int a = im.ann0; a < im.ann0 + im.n_ann; a++) {
            const pp_enc_ann &ann = anns[a];
            const float *kp = keypoints + (size_t)a * K * 3;
            const bool has_kp = (ann.flags & PP_ENC_HAS_KEYPOINTS) != 0;
            if (!ann.iscrowd) {
                if (!has_kp) return fail(PP_EINVAL, w + ": an annotation without keypoints");
                bool valid = false;
                for (int k = 0; k < K; k++) {
                    const Kp p{kp[3 * k] / stride_f, kp[3 * k + 1] / stride_f, kp[3 * k + 2]};
                    if ((double)p.v > thr && !(std::isfinite(p.x) && std::isfinite(p.y)))
                        return fail(PP_EINVAL, w + ": non-finite coordinate of a visible joint");
                    valid = valid || p.v > 0.0f;  // :57
                    sets.push_back(p);
                }
                if (valid) continue;
            }
            if (!(ann.flags & PP_ENC_HAS_BBOX)) return fail(PP_EINVAL, w + ": an annotation without bbox");
            float bb[4];
            for (int c = 0; c < 4; c++) bb[c] = ann.bbox[c] / stride_f;  // :63
            bb[2] = bb[2] + bb[0], bb[3] = bb[3] + bb[1];                // :64
            for (int c = 0; c < 4; c++)
                if (!std::isfinite(bb[c])) return fail(PP_EINVAL, w + ": bbox not finite");
            auto clip = [](int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; };
            EncBox b;
            b.left = clip(checked_int((double)bb[0]), 0, im.w - 1);              // :65
            b.top = clip(checked_int((double)bb[1]), 0, im.h - 1);               // :66
            b.right = clip(checked_int(ceil((double)bb[2])), b.left + 1, im.w);  // :67
            b.bottom = clip(checked_int(ceil((double)bb[3])), b.top + 1, im.h);  // :68
            plan->boxes.push_back(b);
        }
        m.n_box = (int32_t)plan->boxes.size() - m.box0;

        const int n_sets = (int)(sets.size() / (size_t)K);
        const int wp = im.w + 2 * padding, hp = im.h + 2 * padding;
        field_of.clear();
        cif_jobs.clear();
        caf_jobs.clear();
        for (int s = 0; s < n_sets; s++) {
            const Kp *kp = sets.data() + (size_t)s * K;
            const Num scale = ann_scale(kp, K, enc->pose, enc->pose_45, total, total45);
            if (!is_caf) {
                for (int f = 0; f < K; f++) {  // cif.py:105-116
                    if (!((double)kp[f].v > thr)) continue;
                    CifJob job{};
                    float mr[4];
                    max_r(sets.data(), n_sets, K, s, f, thr, mr);
                    job.scale = joint_scale(scale, enc->sigmas, f, mr);
                    // cif.py:119-124: float32 minus the Python float, half-to-even
                    const float rx = rintf(kp[f].x - (float)so), ry = rintf(kp[f].y - (float)so);
                    const int minx = checked_int((double)rx) + padding;
                    const int miny = checked_int((double)ry) + padding;
                    if (minx < 0 || minx + side > wp || miny < 0 || miny + side > hp) continue;
                    // :126 float32 - (int64 + float - int): float64
                    job.offx = (double)kp[f].x - (((double)minx + so) - (double)padding);
                    job.offy = (double)kp[f].y - (((double)miny + so) - (double)padding);
                    job.x0 = minx - padding, job.y0 = miny - padding;
                    for (int q = 0; q < 4; q++) job.mr[q] = mr[q] * 0.5f;  // :141
                    if (job.scale == job.scale && !(job.scale > 0.0f))     // :144
                        return fail(PP_EINVAL, w + ": joint scale <= 0 (the reference asserts scale > 0)");
                    cif_jobs.push_back(job);
                    field_of.push_back(f);
                }
                continue;
            }
            for (int e = 0; e < C; e++) {  // caf.py:118-160
                const int j1 = enc->skeleton[2 * e] - 1, j2 = enc->skeleton[2 * e + 1] - 1;
                const Kp &a = kp[j1], &b = kp[j2];
                if (!((double)a.v > thr) || !((double)b.v > thr)) continue;
                CafJob job{};
                job.ox = b.x - a.x, job.oy = b.y - a.y;          // :164
                const float offset_d = norm2_f32(job.ox, job.oy);  // :165
                if (!std::isfinite(offset_d))
                    return fail(PP_EINVAL, w + ": limb length not finite");
                if (enc->n_sparse > 0) {  // :125-129
                    const float d = offset_d / (float)enc->dense_to_sparse_radius;
                    bool shorter[2];
                    for (int t = 0; t < 2; t++) {  // :100-114 shortest_sparse
                        const int joint = t == 0 ? j1 : j2;
                        double shortest = kInf;
                        for (int g = 0; g < enc->n_sparse; g++) {
                            const int s1 = enc->sparse_skeleton[2 * g] - 1;
                            const int s2 = enc->sparse_skeleton[2 * g + 1] - 1;
                            if (joint != s1 && joint != s2) continue;
                            if (!((double)kp[s1].v > thr) || !((double)kp[s2].v > thr)) continue;
                            const double dd =
                                (double)norm2_f32(kp[s1].x - kp[s2].x, kp[s1].y - kp[s2].y);
                            shortest = dd < shortest ? dd : shortest;
                        }
                        shorter[t] = shortest < (double)d;
                    }
                    if (shorter[0] && shorter[1]) continue;
                }
                if (enc->only_in_field_of_view) {  // :133-144
                    const float mx = (float)(im.w - 1), my = (float)(im.h - 1);
                    if (a.x < 0 || b.x < 0 || a.x > mx || b.x > mx) continue;
                    if (a.y < 0 || b.y < 0 || a.y > my || b.y > my) continue;
                }
                float mr1[4], mr2[4];
                max_r(sets.data(), n_sets, K, s, j1, thr, mr1);  // :150-151
                max_r(sets.data(), n_sets, K, s, j2, thr, mr2);
                job.scale1 = joint_scale(scale, enc->sigmas, j1, mr1);  // :153-159
                job.scale2 = joint_scale(scale, enc->sigmas, j2, mr2);
                for (int q = 0; q < 4; q++) job.mr1[q] = mr1[q] * 0.5f, job.mr2[q] = mr2[q] * 0.5f;
                job.j1x = a.x, job.j1y = a.y, job.j2x = b.x, job.j2y = b.y;
                job.denom = offset_d + 0.01f;  // :203 float32 + Python float
                // :174-177: int(np.ceil(float32)); float32 + np.spacing(1) is float64
                const double nd = ceil((double)offset_d);
                job.num = nd > 2.0 ? checked_int(nd) : 2;
                const double fm = (so + 1.0) / ((double)offset_d + 0x1p-52);
                const double fmargin = fm < 0.4 ? fm : 0.4;
                job.start = fmargin;
                job.stop = 1.0 - fmargin;
                job.step = (job.stop - job.start) / (double)(job.num - 1);
                // no patch centre leaves the segment, and a patch reaches side / 2 + 1 / 2
                // cells from its centre: two more cells of margin
                const double lox = (double)(a.x < b.x ? a.x : b.x), hix = (double)(a.x < b.x ? b.x : a.x);
                const double loy = (double)(a.y < b.y ? a.y : b.y), hiy = (double)(a.y < b.y ? b.y : a.y);
                job.bx0 = checked_int(floor(lox - so - 2.0)), job.bx1 = checked_int(ceil(hix + so + 2.0));
                job.by0 = checked_int(floor(loy - so - 2.0)), job.by1 = checked_int(ceil(hiy + so + 2.0));
                const bool bad1 = job.scale1 == job.scale1 && !(job.scale1 > 0.0f);
                const bool bad2 = job.scale2 == job.scale2 && !(job.scale2 > 0.0f);
                if (bad1 || bad2) {  // :219-221 fire at the first step inside the field
                    const int n = caf_steps(job, enc->fixed_size != 0);
                    for (int t = 0; t < n; t++)
                        if (caf_step(job, t, side, padding, enc->fixed_size != 0, wp, hp).ok)
                            return fail(PP_EINVAL,
                                        w + ": joint scale <= 0 (the reference asserts scale > 0)");
                }
                caf_jobs.push_back(job);
                field_of.push_back(e);
            }
        }
        // the image's jobs by field, the reference's order kept within a field
        std::fill(count.begin(), count.end(), 0);
        for (int f : field_of) count[(size_t)f + 1]++;
        const int32_t base = plan->fj[(size_t)i * F];
        for (int f = 0; f < F; f++) {
            count[(size_t)f + 1] += count[(size_t)f];
            plan->fj[(size_t)i * F + f + 1] = base + count[(size_t)f + 1];
        }
        if (is_caf) {
            plan->caf.resize((size_t)base + caf_jobs.size());
            for (size_t j = 0; j < caf_jobs.size(); j++)
                plan->caf[(size_t)base + (size_t)count[(size_t)field_of[j]]++] = caf_jobs[j];
        } else {
            plan->cif.resize((size_t)base + cif_jobs.size());
            for (size_t j = 0; j < cif_jobs.size(); j++)
                plan->cif[(size_t)base + (size_t)count[(size_t)field_of[j]]++] = cif_jobs[j];
        }
    }
    plan->blocks = blocks;
    plan->layout(is_caf);
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" {

size_t pp_encode_cif_tables_size(int32_t n_img, int32_t n_ann, int32_t K) {
    return encode_tables_bound(n_img, n_ann, K, false);
}

size_t pp_encode_caf_tables_size(int32_t n_img, int32_t n_ann, int32_t C) {
    return encode_tables_bound(n_img, n_ann, C, true);
}

int64_t pp_encode_cif_output_size(int32_t h, int32_t w, int32_t K) {
    if (h < 1 || w < 1 || K < 1 || K > PP_MAX_KP) return 0;
    return 8 * (int64_t)K * h * w;
}

int64_t pp_encode_caf_output_size(int32_t h, int32_t w, int32_t C) {
    if (h < 1 || w < 1 || C < 1 || C > PP_MAX_EDGES) return 0;
    return 15 * (int64_t)C * h * w;
}

}  // extern "C"

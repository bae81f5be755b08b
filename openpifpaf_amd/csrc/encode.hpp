// encode.hpp — the CIF / CAF target encoders (openpifpaf/encoder/cif.py, caf.py,
// annrescaler.py, utils.py): the records the host plans per batch and the per-cell
// functions the gfx950 kernel (encode.hip) and the host twins (encode_cpu.hip) both run, so
// that the two agree bit for bit by construction.
//
// Every cell of a target field is independent of every other: the reference's
// `mask = sink_l < fields_reg_l[patch]` tests each cell of a patch on its own.  A cell's
// result is therefore its own fold over the patches that cover it, in the reference's order
// (annotation, then field, then step along the limb), starting from inf (1.0 inside a crowd
// box): test `sink_l (float64) < l (float32 as stored)`, and on a win store sink_l rounded
// to float32.  The cells of the 10-cell padding are cropped from the result and decide
// nothing, so they have no state; the padding only decides whether a whole patch is skipped
// (cif.py:122-124, caf.py:184-186), which is part of a job's plan (CIF) or of a step (CAF).
#pragma once
#pragma clang fp contract(off)

#include "pp_common.hpp"

#include <cmath>
#include <vector>

namespace pp {

constexpr int kEncBlock = 256;       // cells per workgroup: one cell per lane
constexpr int kEncMaxSide = 16384;   // field edge (float32 cell coordinates stay exact to 2^-9)
constexpr uint32_t kNaN = 0x7FC00000u;

// one image of the batch as the kernel reads it
struct EncImage {
    int64_t out_offset[5];
    int32_t h, w;
    int32_t block0;            // first workgroup of this image
    int32_t bpp;               // workgroups per field plane = ceil(h w / kEncBlock)
    int32_t box0, n_box;       // crowd boxes (bg_mask == 0)
    int32_t y_lo, x_lo;        // mask_valid_area: rows < y_lo and columns < x_lo
    int32_t y_hi, x_hi;        //                  rows >= y_hi and columns >= x_hi
    int32_t fj0;               // first entry of this image in the (image, field) job prefix
    int32_t pad_;
};
static_assert(sizeof(EncImage) == 88, "EncImage layout");

struct EncBox {
    int32_t left, top, right, bottom;  // annrescaler.py:65-69, half open
};

// cif.py:118-145 fill_coordinate of one joint whose patch lies inside the padded field
struct CifJob {
    double offx, offy;   // cif.py:126 offset (float64)
    int32_t x0, y0;      // minx - padding, miny - padding: the patch's first cell
    float scale;         // cif.py:114 joint_scale as stored (float32)
    float mr[4];         // cif.py:141 max_r * 0.5
    int32_t pad_;
};
static_assert(sizeof(CifJob) == 48, "CifJob layout");

// caf.py:162-222 fill_association of one limb: the steps are walked per cell
struct CafJob {
    double start, step, stop;  // caf.py:177 np.linspace(fmargin, 1 - fmargin, num)
    float j1x, j1y, j2x, j2y;
    float ox, oy;              // caf.py:164 offset (float32)
    float denom;               // caf.py:203 offset_d + 0.01 (float32)
    int32_t num;
    float scale1, scale2;
    float mr1[4], mr2[4];
    int32_t bx0, bx1, by0, by1;  // cells outside this box are covered by no step
};
static_assert(sizeof(CafJob) == 112, "CafJob layout");

struct CifCell {
    float l, rx, ry;
    int32_t win;
};
struct CafCell {
    float l, r1x, r1y, r2x, r2y;
    int32_t win;
};

// np.linalg.norm of a float32 pair: sqrt(x0 * x0 + x1 * x1), every operation float32,
// nothing fused (what x.dot(x) gives for two elements; tests/test_encoder_cpu.py)
__host__ __device__ __forceinline__ float norm2_f32(float x, float y) {
    const float a = x * x, b = y * y;
    return sqrtf(a + b);
}

// element i of np.linspace(start, stop, num) for num >= 2: i * step + start with
// step = (stop - start) / (num - 1), the last element exactly stop
__host__ __device__ __forceinline__ double linspace_at(double start, double step, double stop,
                                                       int num, int i) {
    if (i == num - 1) return stop;
    const double t = (double)i * step;
    return t + start;
}

// cif.py:129-145 for the cell (x, y) and job `ji`; side = Cif.side_length
__host__ __device__ __forceinline__ void cif_apply(const CifJob &j, int ji, int side, int x, int y,
                                                   CifCell &c) {
    const int cx = x - j.x0, cy = y - j.y0;
    if (cx < 0 || cx >= side || cy < 0 || cy >= side) return;
    const double so = ((double)side - 1.0) / 2.0;
    // utils.py:11 sink1d[c] = so - c, exact in float32; cif.py:130 float32 + float64
    const double sx = (so - (double)cx) + j.offx;
    const double sy = (so - (double)cy) + j.offy;
    const double xx = sx * sx, yy = sy * sy;
    const double l = sqrt(xx + yy);  // cif.py:131
    if (l < (double)c.l) {           // cif.py:132
        c.l = (float)l;
        c.rx = (float)sx;
        c.ry = (float)sy;
        c.win = ji;
    }
}

// One step of caf.py:180-193: the patch's first cell in padded coordinates and the joints'
// offsets from the patch centre.  The linspace steps are float64 (a NumPy float64 times a
// float32 array); with Caf.fixed_size the step is the Python float 0.5, which leaves every
// array float32.  `ok` false: the patch does not lie inside the padded field (caf.py:184).
struct CafStep {
    int fminx, fminy;
    double a1x, a1y, a2x, a2y;  // joint1_offset, joint2_offset (float32 values when fixed)
    bool ok;
};
__host__ __device__ __forceinline__ CafStep caf_step(const CafJob &j, int i, int s, int padding,
                                                     bool fixed, int wp, int hp) {
    CafStep st;
    const double so = ((double)s - 1.0) / 2.0;
    double fijx, fijy;
    if (!fixed) {
        const double f = linspace_at(j.start, j.step, j.stop, j.num, i);
        const double tx = f * (double)j.ox, ty = f * (double)j.oy;
        const double ux = (double)j.j1x + tx, uy = (double)j.j1y + ty;
        fijx = rint(ux - so) + (double)padding;  // caf.py:181
        fijy = rint(uy - so) + (double)padding;
        const double fx = (fijx - (double)padding) + so;  // caf.py:187
        const double fy = (fijy - (double)padding) + so;
        st.a1x = (double)j.j1x - fx;
        st.a1y = (double)j.j1y - fy;
        st.a2x = (double)j.j2x - fx;
        st.a2y = (double)j.j2y - fy;
    } else {
        const float sof = (float)so, pf = (float)padding;
        const float tx = 0.5f * j.ox, ty = 0.5f * j.oy;
        const float ux = j.j1x + tx, uy = j.j1y + ty;
        const float gx = rintf(ux - sof) + pf, gy = rintf(uy - sof) + pf;
        const float fx = (gx - pf) + sof, fy = (gy - pf) + sof;
        fijx = (double)gx;
        fijy = (double)gy;
        st.a1x = (double)(j.j1x - fx);
        st.a1y = (double)(j.j1y - fy);
        st.a2x = (double)(j.j2x - fx);
        st.a2y = (double)(j.j2y - fy);
    }
    st.ok = fabs(fijx) < 1e9 && fabs(fijy) < 1e9;
    st.fminx = st.ok ? (int)fijx : 0;
    st.fminy = st.ok ? (int)fijy : 0;
    st.ok = st.ok && st.fminx >= 0 && st.fminx + s <= wp && st.fminy >= 0 && st.fminy + s <= hp;
    return st;
}

__host__ __device__ __forceinline__ int caf_steps(const CafJob &j, bool fixed) {
    return fixed ? 1 : j.num;
}

// caf.py:180-222 for the cell (x, y) and job `ji`: every step whose patch covers the cell
__host__ __device__ __forceinline__ void caf_apply(const CafJob &j, int ji, int s, int padding,
                                                   bool fixed, int w, int h, int x, int y,
                                                   CafCell &c) {
    if (x < j.bx0 || x > j.bx1 || y < j.by0 || y > j.by1) return;
    const double so = ((double)s - 1.0) / 2.0;
    const bool f32 = fixed && s > 1;  // float32 sink + float32 offsets: all float32
    const int n = caf_steps(j, fixed);
    for (int i = 0; i < n; i++) {
        const CafStep st = caf_step(j, i, s, padding, fixed, w + 2 * padding, h + 2 * padding);
        if (!st.ok) continue;
        const int cx = x + padding - st.fminx, cy = y + padding - st.fminy;
        if (cx < 0 || cx >= s || cy < 0 || cy >= s) continue;
        double s1x, s1y, s2x, s2y, l;
        if (f32) {
            const float kx = (float)(so - (double)cx), ky = (float)(so - (double)cy);
            const float p1x = kx + (float)st.a1x, p1y = ky + (float)st.a1y;
            const float p2x = kx + (float)st.a2x, p2y = ky + (float)st.a2y;
            const float m1 = j.oy * p1x, m2 = j.ox * p1y;
            l = (double)(fabsf(m1 - m2) / j.denom);  // caf.py:200-203
            s1x = p1x, s1y = p1y, s2x = p2x, s2y = p2y;
        } else {
            const double kx = so - (double)cx, ky = so - (double)cy;
            s1x = kx + st.a1x, s1y = ky + st.a1y;  // caf.py:192-193
            s2x = kx + st.a2x, s2y = ky + st.a2y;
            const double m1 = (double)j.oy * s1x, m2 = (double)j.ox * s1y;
            l = fabs(m1 - m2) / (double)j.denom;
        }
        if (l < (double)c.l) {  // caf.py:204
            c.l = (float)l;
            c.r1x = (float)s1x, c.r1y = (float)s1y;
            c.r2x = (float)s2x, c.r2y = (float)s2y;
            c.win = ji;
        }
    }
}

// the cell lies in a crowd box (cif.py:70-71: reg_l starts at 1.0, the intensity at NaN)
__host__ __device__ __forceinline__ bool enc_in_box(const EncBox *boxes, int n, int x, int y) {
    bool in = false;
    for (int b = 0; b < n; b++)
        in = in || (x >= boxes[b].left && x < boxes[b].right && y >= boxes[b].top &&
                    y < boxes[b].bottom);
    return in;
}

// utils.py:19-37 mask_valid_area
__host__ __device__ __forceinline__ bool enc_masked(const EncImage &m, int x, int y) {
    return y < m.y_lo || x < m.x_lo || y >= m.y_hi || x >= m.x_hi;
}

__host__ __device__ __forceinline__ float canon(float v) { return v != v ? f32_of(kNaN) : v; }

// cif.py:147-162 fields(): the three tensors' elements of one cell of field f, each stored once
__host__ __device__ __forceinline__ void cif_emit(float *out, const EncImage &m, int f, int cell,
                                                  bool bg, bool masked, const CifCell &c,
                                                  const CifJob *jobs) {
    const int64_t hw = (int64_t)m.h * m.w;
    const float nan = f32_of(kNaN), inf = __builtin_inff();
    const bool won = c.win >= 0;
    out[m.out_offset[0] + f * hw + cell] = masked ? 0.0f : won ? 1.0f : bg ? nan : 0.0f;
    float *reg = out + m.out_offset[1] + (int64_t)f * 6 * hw + cell;
    reg[0] = masked || !won ? nan : canon(c.rx);
    reg[hw] = masked || !won ? nan : canon(c.ry);
    for (int q = 0; q < 4; q++) reg[(2 + q) * hw] = won ? jobs[c.win].mr[q] : inf;
    out[m.out_offset[2] + f * hw + cell] = masked || !won ? nan : canon(jobs[c.win].scale);
}

// caf.py:224-246 fields()
__host__ __device__ __forceinline__ void caf_emit(float *out, const EncImage &m, int f, int cell,
                                                  bool bg, bool masked, const CafCell &c,
                                                  const CafJob *jobs) {
    const int64_t hw = (int64_t)m.h * m.w;
    const float nan = f32_of(kNaN), inf = __builtin_inff();
    const bool won = c.win >= 0;
    out[m.out_offset[0] + f * hw + cell] = masked ? 0.0f : won ? 1.0f : bg ? nan : 0.0f;
    float *reg1 = out + m.out_offset[1] + (int64_t)f * 6 * hw + cell;
    float *reg2 = out + m.out_offset[2] + (int64_t)f * 6 * hw + cell;
    reg1[0] = masked || !won ? nan : canon(c.r1x);
    reg1[hw] = masked || !won ? nan : canon(c.r1y);
    reg2[0] = masked || !won ? nan : canon(c.r2x);
    reg2[hw] = masked || !won ? nan : canon(c.r2y);
    for (int q = 0; q < 4; q++) {
        reg1[(2 + q) * hw] = won ? jobs[c.win].mr1[q] : inf;
        reg2[(2 + q) * hw] = won ? jobs[c.win].mr2[q] : inf;
    }
    out[m.out_offset[3] + f * hw + cell] = masked || !won ? nan : canon(jobs[c.win].scale1);
    out[m.out_offset[4] + f * hw + cell] = masked || !won ? nan : canon(jobs[c.win].scale2);
}

// one cell from its initial state to its stored elements
__host__ __device__ __forceinline__ void cif_cell(float *out, const EncImage &m,
                                                  const EncBox *boxes, const int32_t *fj,
                                                  const CifJob *jobs, int side, int f, int cell) {
    const int y = cell / m.w, x = cell - y * m.w;
    const bool bg = enc_in_box(boxes + m.box0, m.n_box, x, y);
    CifCell c{bg ? 1.0f : __builtin_inff(), 0.0f, 0.0f, -1};
    const int j1 = fj[m.fj0 + f + 1];
    for (int j = fj[m.fj0 + f]; j < j1; j++) cif_apply(jobs[j], j, side, x, y, c);
    cif_emit(out, m, f, cell, bg, enc_masked(m, x, y), c, jobs);
}

__host__ __device__ __forceinline__ void caf_cell(float *out, const EncImage &m,
                                                  const EncBox *boxes, const int32_t *fj,
                                                  const CafJob *jobs, int s, int padding,
                                                  bool fixed, int f, int cell) {
    const int y = cell / m.w, x = cell - y * m.w;
    const bool bg = enc_in_box(boxes + m.box0, m.n_box, x, y);
    CafCell c{bg ? 1.0f : __builtin_inff(), 0.0f, 0.0f, 0.0f, 0.0f, -1};
    const int j1 = fj[m.fj0 + f + 1];
    for (int j = fj[m.fj0 + f]; j < j1; j++)
        caf_apply(jobs[j], j, s, padding, fixed, m.w, m.h, x, y, c);
    caf_emit(out, m, f, cell, bg, enc_masked(m, x, y), c, jobs);
}

// The host's plan of one batch (encode_plan.hip): the argument checks, the per-annotation
// scalars of annrescaler.py and cif.py / caf.py, and the job lists per (image, field).
struct EncPlan {
    std::vector<EncImage> images;
    std::vector<int32_t> fj;      // (n_img * F + 1) prefix of jobs per (image, field)
    std::vector<EncBox> boxes;
    std::vector<CifJob> cif;
    std::vector<CafJob> caf;
    int64_t blocks = 0;
    int F = 0;
    // the staged table block: images, fj, boxes, jobs, each 8-byte aligned
    size_t off_fj = 0, off_boxes = 0, off_jobs = 0, bytes = 0;
    void layout(bool is_caf);
    void stage(char *dst, bool is_caf) const;
};
int encode_plan(const char *who, bool is_caf, const pp_encoder *enc, const pp_enc_image *images,
                int32_t n_img, const pp_enc_ann *anns, const float *keypoints, int32_t n_ann,
                const void *out, int64_t out_elems, EncPlan *plan);
size_t encode_tables_bound(int32_t n_img, int32_t n_ann, int32_t F, bool is_caf);

}  // namespace pp

// inverse.hpp — Preprocess.annotations_inverse / anndet_inverse (transforms/preprocess.py:35-95)
// stated once, per joint and per box, for the in-place kernels (inverse.hip), the COCO record
// kernels (coco.hip) and their host twins (coco_cpu.hip).
//
// NumPy semantics, step by step: the meta's offset / scale are float64 arrays and
// width_height an int64 array (transforms/annotations.py:39-44), so those in-place steps
// on the float32 records compute in float64 and round to float32; the rotation mixes
// float32 arrays with Python floats, so it runs in float32 with the constants rounded.
#pragma once

#include <math.h>

#include "pp_common.hpp"

namespace pp {

#define PP_HD __host__ __device__ __forceinline__

// The rotation's constants of one image (preprocess.py:51-56): Python floats rounded to
// float32 where NumPy multiplies them with the float32 arrays
struct InverseXf {
    float c, s, hw, hh;
    int rot;
};
PP_HD InverseXf inverse_xf(const pp_inverse_meta &m) {
    InverseXf t{};
    const double angle = -m.rotation_angle;
    t.rot = angle != 0.0;
    if (t.rot) {
        t.c = (float)cos(angle / 180.0 * M_PI);
        t.s = (float)sin(angle / 180.0 * M_PI);
        t.hw = (float)((m.rotation_width - 1.0) / 2.0);
        t.hh = (float)((m.rotation_height - 1.0) / 2.0);
    }
    return t;
}
PP_HD void inverse_rotate(const InverseXf &t, float &x, float &y) {
    const float xo = x - t.hw, yo = y - t.hh;
    x = (t.hw + t.c * xo) + t.s * yo;
    y = (t.hh - t.s * xo) + t.c * yo;
}

// coordinate c (0 = x, 1 = y) through offset, then scale: all that the decoding order gets
// (preprocess.py:76-81)
PP_HD float inverse_coord(const pp_inverse_meta &m, int c, float v) {
    v = (float)((double)v + m.offset[c]);
    return (float)((double)v / m.scale[c]);
}

// one joint's (x, y) through rotation, offset, scale; `nan` as the reference's assert sees
// it (preprocess.py:67, before the flip); then the flip's x (preprocess.py:69-71)
PP_HD void inverse_point(const pp_inverse_meta &m, const InverseXf &t, float &x, float &y, float v,
                         bool &nan) {
    if (t.rot) inverse_rotate(t, x, y);
    x = inverse_coord(m, 0, x);
    y = inverse_coord(m, 1, y);
    nan = nan || x != x || y != y || v != v;
    if (m.hflip) x = (float)(-(double)x + (m.width - 1.0));
}
PP_HD float inverse_jscale(const pp_inverse_meta &m, float s) {
    return (float)((double)s / m.scale[0]);
}

// np.minimum / np.maximum of two float32 scalars in rotate_box's order
PP_HD float np_min2(float a, float b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }
PP_HD float np_max2(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

// anndet_inverse (preprocess.py:84-95) with utils.rotate_box (transforms/utils.py:5-28) on
// one (x, y, w, h)
PP_HD void inverse_box(const pp_inverse_meta &m, const InverseXf &t, float *b) {
    if (t.rot) {
        float rx[4] = {b[0], b[0] + b[2], b[0], b[0] + b[2]};
        float ry[4] = {b[1], b[1], b[1] + b[3], b[1] + b[3]};
        for (int i = 0; i < 4; i++) inverse_rotate(t, rx[i], ry[i]);
        float x = rx[0], y = ry[0], xm = rx[0], ym = ry[0];
        for (int i = 1; i < 4; i++) {
            x = np_min2(x, rx[i]);
            y = np_min2(y, ry[i]);
            xm = np_max2(xm, rx[i]);
            ym = np_max2(ym, ry[i]);
        }
        b[0] = x;
        b[1] = y;
        b[2] = xm - x;
        b[3] = ym - y;
    }
    b[0] = inverse_coord(m, 0, b[0]);
    b[1] = inverse_coord(m, 1, b[1]);
    b[2] = (float)((double)b[2] / m.scale[0]);
    b[3] = (float)((double)b[3] / m.scale[1]);
}

}  // namespace pp

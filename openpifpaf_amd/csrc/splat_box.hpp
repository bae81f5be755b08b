// splat_box.hpp — what the square-splat primitives (splat.hip) and the CifHr maps (cifhr.hip)
// share: the splat modes, the output tile edge and a splat's box.
#pragma once

#include "pp_common.hpp"

namespace pp {

enum SplatMode { M_GAUSS_MAX = 0, M_GAUSS = 1, M_MAXG = 2, M_CONST = 3, M_CUMAVG = 4 };

constexpr int kTile = 64;     // output tile edge (pixels)

// Box of one splat.  ext = truncate*sigma (gauss modes) or width (const / cumavg).
template <int MODE>
__device__ __forceinline__ int4 splat_box(float cx, float cy, float ext, int h, int w) {
    int4 b;
    b.x = (int)clip_ref(cx - ext, 0.0f, (float)(w - 1));
    float hx = cx + ext;
    if (MODE == M_GAUSS_MAX) hx = hx + 1.0f;  // functional.pyx:123 `... + 1`
    b.y = (int)clip_ref(hx, (float)(b.x + 1), (float)w);
    b.z = (int)clip_ref(cy - ext, 0.0f, (float)(h - 1));
    float hy = cy + ext;
    if (MODE == M_GAUSS_MAX) hy = hy + 1.0f;
    b.w = (int)clip_ref(hy, (float)(b.z + 1), (float)h);
    return b;
}

}  // namespace pp

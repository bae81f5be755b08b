// by_source.hpp — the skeleton as CifCaf's by_source (cifcaf.py:62-65), host only: the
// decoder's GrowArgs (decode.hip) and its host twin (decode_cpu.hip) both read it.
#pragma once

#include <stdint.h>

#include "pifpaf_amd.h"

namespace pp {

// per start joint, its (end, CAF, forward) entries in dict insertion order; a later
// duplicate key overwrites the value in place
struct BySource {
    int n[PP_MAX_KP] = {};
    int end[PP_MAX_KP][PP_MAX_KP];
    int caf[PP_MAX_KP][PP_MAX_KP];
    bool fwd[PP_MAX_KP][PP_MAX_KP];

    BySource(const int32_t *skeleton, int C) {
        for (int ci = 0; ci < C; ci++) {
            const int j1 = skeleton[2 * ci] - 1, j2 = skeleton[2 * ci + 1] - 1;
            put(j1, j2, ci, true);
            put(j2, j1, ci, false);
        }
    }
    void put(int s, int e, int ci, bool f) {
        int at = -1;
        for (int i = 0; i < n[s]; i++)
            if (end[s][i] == e) at = i;
        if (at < 0) at = n[s]++;
        end[s][at] = e;
        caf[s][at] = ci;
        fwd[s][at] = f;
    }
};

}  // namespace pp

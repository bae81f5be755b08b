// coco_asan_main.hip — sanitizer driver for the host twins of the COCO record kernels
// (pp_coco_keypoints_cpu / pp_coco_dets_cpu, csrc/coco_cpu.hip with csrc/coco.hpp and the
// inverse transform of csrc/inverse.hpp, which the in-place kernels share).  Host
// code only, a program of its own; build and run where no GPU is needed:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host \
//       -fsanitize=address,undefined -I include -I openpifpaf_amd/csrc \
//       openpifpaf_amd/csrc/coco_cpu.hip tools/coco_asan_main.hip -o coco_asan && ./coco_asan
//
// Random records at odd shapes (K 1..24, counts around and above the capacity, output
// blocks one record short, every meta kind, swap tables that drop rows) with every buffer
// allocated to its exact size, so an access past an end aborts.  Prints "coco asan ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pifpaf_amd.h"

namespace pp {  // the library's error plumbing (pp_host.hip), not linked here
int fail(int status, const std::string &msg) {
    std::fprintf(stderr, "refused: %s\n", msg.c_str());
    return status;
}
}  // namespace pp

static uint64_t rng = 88172645463325252ull;
static double urand() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (double)(rng >> 11) * (1.0 / 9007199254740992.0);
}

int main() {
    long records = 0;
    for (int K = 1; K <= PP_MAX_KP; K += (K < 5 ? 1 : 6)) {
        for (int n_img : {1, 3, 9}) {
            for (int cap : {1, 7, 65}) {
                std::vector<pp_ann> anns((size_t)n_img * cap);
                std::vector<pp_det> dets((size_t)n_img * cap);
                std::vector<int32_t> counts(n_img), hswap(K);
                std::vector<pp_inverse_meta> metas(n_img);
                std::vector<int64_t> ids(n_img);
                for (auto &a : anns) {
                    std::memset(&a, 0, sizeof(a));
                    for (int j = 0; j < K; j++) {
                        a.data[j][0] = (float)(urand() * 600 - 50);
                        a.data[j][1] = (float)(urand() * 400 - 50);
                        a.data[j][2] = urand() < 0.3 ? 0.0f : (float)(urand() * (urand() < 0.2 ? 0.02 : 1.0));
                        a.joint_scales[j] = (float)(urand() * 8);
                    }
                    if (urand() < 0.02) a.data[K - 1][1] = NAN;
                    a.score = urand() < 0.05 ? NAN : urand();
                }
                for (auto &d : dets) {
                    d.field = (int32_t)(urand() * 80);
                    d.score = (float)urand();
                    for (int i = 0; i < 4; i++) d.bbox[i] = (float)(urand() * 300);
                    d.image = d.pad_ = 0;
                }
                for (int i = 0; i < n_img; i++) {
                    counts[i] = (int32_t)(urand() * (cap + 3)) - 1;  // -1 .. cap + 1
                    ids[i] = (int64_t)(urand() * 1e12);
                    pp_inverse_meta &m = metas[i];
                    m.offset[0] = urand() * 40 - 20;
                    m.offset[1] = urand() * 40 - 20;
                    m.scale[0] = 0.4 + urand();
                    m.scale[1] = 0.4 + urand();
                    const bool rot = urand() < 0.4;
                    m.rotation_angle = rot ? urand() * 60 - 30 : 0.0;
                    m.rotation_width = rot ? 481 : 0;
                    m.rotation_height = rot ? 361 : 0;
                    m.width = 300 + (int)(urand() * 400);
                    m.hflip = urand() < 0.5;
                    m.pad_ = 0;
                }
                for (int j = 0; j < K; j++) hswap[j] = (int32_t)(urand() * K);  // may drop rows
                for (int maxp : {1, 3, 200}) {
                    for (double th : {0.0, 60.0, 1e9}) {
                        const pp_coco_params P{th, maxp, 1};
                        std::vector<int32_t> oc(n_img), of(n_img);
                        // first call: nothing fits; the counts size the second block
                        std::vector<char> none(1);
                        if (pp_coco_keypoints_cpu(anns.data(), counts.data(), n_img, cap, K,
                                                  metas.data(), ids.data(), hswap.data(), &P,
                                                  none.data(), 0, oc.data(), of.data()))
                            return 1;
                        long total = 0;
                        for (int c : oc) total += c;
                        for (long fit : {total, total - 1}) {
                            std::vector<char> out((size_t)(fit * (56 + 24 * K)) + 1);  // pp_coco_record_size(K)
                            if (pp_coco_keypoints_cpu(anns.data(), counts.data(), n_img, cap, K,
                                                      metas.data(), ids.data(),
                                                      fit == total ? hswap.data() : nullptr, &P,
                                                      out.data(), fit, oc.data(), of.data()))
                                return 1;
                        }
                        records += total;
                        if (pp_coco_dets_cpu(dets.data(), counts.data(), n_img, cap, metas.data(),
                                             ids.data(), &P, (pp_coco_det *)none.data(), 0,
                                             oc.data(), of.data()))
                            return 1;
                        total = 0;
                        for (int c : oc) total += c;
                        std::vector<pp_coco_det> dout((size_t)total);
                        if (pp_coco_dets_cpu(dets.data(), counts.data(), n_img, cap, metas.data(),
                                             ids.data(), &P, dout.data(), total, oc.data(),
                                             of.data()))
                            return 1;
                        records += total;
                    }
                }
            }
        }
    }
    std::printf("coco asan ok (%ld records)\n", records);
    return 0;
}

// preprocess_asan_main.hip — sanitizer driver for pp_preprocess_views_cpu and
// pp_preprocess_images_cpu, the host twin of the eval preprocessing kernels
// (csrc/preprocess.hip with csrc/preprocess_pixel.hpp; the kernels run the same
// __host__ __device__ index arithmetic).  Host code only, a program of its own; build and
// run where no GPU is needed:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host \
//       -fsanitize=address,undefined -I include -I openpifpaf_amd/csrc \
//       openpifpaf_amd/csrc/preprocess.hip tools/preprocess_asan_main.hip \
//       -o preprocess_asan && ./preprocess_asan
//
// Views: three random images per call at every canvas edge from 2 to 70, random turns,
// reduction masks, mirror on and off, four dtypes and both layouts.  Images: three per call
// on H x W canvases with H != W, both from 2 to 70.  The source and the output are allocated
// to their exact sizes, so an access past an end aborts.  Prints "views asan ok" and
// "images asan ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pifpaf_amd.h"
namespace pp {  // the library's error plumbing (pp_host.hip), not linked here
int fail(int status, const std::string &msg) { std::fprintf(stderr, "refused: %s\n", msg.c_str()); return status; }
int check_launch(const char *) { return 0; }
}
static uint64_t rng = 88172645463325252ull;
static uint32_t nxt() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 16); }
int main() {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const uint8_t fill[3] = {124, 116, 104};
    int runs = 0;
    for (int N = 2; N <= 70; N++)
        for (int mask = 1; mask < 32; mask += (N % 7 == 0 ? 1 : 6))
            for (int mirror = 0; mirror < 2; mirror++)
                for (int dtype = 0; dtype < 4; dtype++)
                    for (int layout = 0; layout < 2; layout++) {
                        const int n_img = 3;
                        int sizes[5] = {N, N - N / 3, (N + 1) / 2, (N + 2) / 3, (N + 4) / 5};
                        int n_red = 0;
                        for (int r = 0; r < 5; r++) n_red += (mask >> r) & 1;
                        const int n_views = n_red * (mirror ? 2 : 1);
                        std::vector<pp_view_image> im(n_img);
                        std::vector<int64_t> offs((size_t)n_img * n_views);
                        int64_t so = 0, oo = 0;
                        // exact-size source
                        std::vector<int> hs(n_img), ws(n_img);
                        for (int i = 0; i < n_img; i++) {
                            hs[i] = 2 + nxt() % 20; ws[i] = 2 + nxt() % 20;
                            const int th = 2 + nxt() % (N - 1), tw = 2 + nxt() % (N - 1);
                            pp_view_image &d = im[i];
                            d.src_offset = so; d.h = hs[i]; d.w = ws[i]; d.th = th; d.tw = tw;
                            d.left = (N - tw) / 2; d.top = (N - th) / 2; d.H = N; d.W = N;
                            d.rot = nxt() % 4; d.reserved = 0;
                            so += (int64_t)hs[i] * ws[i] * 3;
                        }
                        int v = 0;
                        for (int side = 0; side < (mirror ? 2 : 1); side++)
                            for (int r = 0; r < 5; r++) {
                                if (!((mask >> r) & 1)) continue;
                                for (int i = 0; i < n_img; i++) {
                                    offs[(size_t)i * n_views + v] = oo;
                                    oo += 3LL * sizes[r] * sizes[r];
                                }
                                v++;
                            }
                        const size_t es = dtype == 0 ? 4 : dtype == 3 ? 1 : 2;
                        uint8_t *src = (uint8_t *)malloc((size_t)so);
                        for (int64_t k = 0; k < so; k++) src[k] = (uint8_t)nxt();
                        void *out = malloc((size_t)oo * es);
                        memset(out, 0xAB, (size_t)oo * es);
                        const int rc = pp_preprocess_views_cpu(src, so, im.data(), offs.data(), n_img, mask, mirror, out, oo, dtype, layout, mean, sd, fill);
                        if (rc != 0) { printf("rc %d at N %d mask %d\n", rc, N, mask); return 1; }
                        free(src); free(out);
                        runs++;
                    }
    printf("views asan ok: %d runs\n", runs);
    runs = 0;
    for (int H = 2; H <= 70; H++)
        for (int W = 2 + H % 3; W <= 70; W += 3)
            for (int dtype = 0; dtype < 4; dtype++)
                for (int layout = 0; layout < 2; layout++) {
                    if (H == W) continue;
                    const int n_img = 3;
                    std::vector<pp_image_desc> im(n_img);
                    int64_t so = 0, oo = 0;
                    for (int i = 0; i < n_img; i++) {
                        pp_image_desc &d = im[i];
                        d.h = 2 + nxt() % 20; d.w = 2 + nxt() % 20;
                        d.th = 2 + nxt() % (H - 1); d.tw = 2 + nxt() % (W - 1);
                        d.left = (W - d.tw) / 2; d.top = (H - d.th) / 2; d.H = H; d.W = W;
                        d.src_offset = so; d.out_offset = oo;
                        so += (int64_t)d.h * d.w * 3;
                        oo += 3LL * H * W;
                    }
                    const size_t es = dtype == 0 ? 4 : dtype == 3 ? 1 : 2;
                    uint8_t *src = (uint8_t *)malloc((size_t)so);
                    for (int64_t k = 0; k < so; k++) src[k] = (uint8_t)nxt();
                    void *out = malloc((size_t)oo * es);
                    memset(out, 0xAB, (size_t)oo * es);
                    const int rc = pp_preprocess_images_cpu(src, so, im.data(), n_img, out, oo, dtype, layout, mean, sd, fill);
                    if (rc != 0) { printf("rc %d at H %d W %d\n", rc, H, W); return 1; }
                    free(src); free(out);
                    runs++;
                }
    printf("images asan ok: %d runs\n", runs);
    return 0;
}

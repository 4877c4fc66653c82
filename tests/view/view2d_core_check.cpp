// stereo-vision_amd/csrc/view2d_core.h built by the host compiler alone (g++ -ffp-contract=off, no HIP): one render of
// a pane with the header's own functions, the texels and the overlay filled by plain loops in draw order.
// tests/test_view2d.py compares its output with the numpy restatement tests/view2d_ref.py byte for byte.
//
//   view2d_core_check <job>   job: int32 W, H, kind (0 none, 1 grey, 2 float RGB, 3 disparity), w, h, n, left;
//                                  the source (w * h bytes, w * h * 3 floats or w * h floats; nothing for kind 0);
//                                  n x Match (48 bytes); n x uint8 inlier flag
//   stdout: W * H * 3 bytes, row 0 = top
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../stereo-vision_amd/csrc/view2d_core.h"

using namespace svh::view2d;

static void rd(FILE* f, void* p, size_t bytes) {
    if (bytes && fread(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "short job file\n");
        exit(2);
    }
}

struct OverlayPlot {
    const Pane& f;
    std::vector<uint32_t>& ovl;
    void operator()(int32_t x, int32_t y, uint32_t word) { ovl[pixel_index(f, x, y)] = word; }   // drawn in order
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[7];
    rd(in, head, sizeof(head));
    const int32_t W = head[0], H = head[1], kind = head[2], w = head[3], h = head[4], n = head[5], left = head[6];
    const size_t ntex = (size_t)w * h;
    std::vector<uint8_t> tex;
    Pane f{W, H, 1, 1, 0, 0};
    if (kind == 1) {
        tex.resize(ntex);
        rd(in, tex.data(), ntex);
        f = Pane{W, H, w, h, 1, (uint32_t)w};
    } else if (kind == 2 || kind == 3) {
        std::vector<float> src(ntex * (kind == 2 ? 3 : 1));
        rd(in, src.data(), src.size() * 4);
        tex.resize(3 * ntex);
        for (size_t i = 0; i < ntex; i++) {
            float c[3] = {0, 0, 0};
            if (kind == 3) disparity_colour(src[i], c);
            else c[0] = src[3 * i], c[1] = src[3 * i + 1], c[2] = src[3 * i + 2];
            for (int k = 0; k < 3; k++) tex[3 * i + k] = byte_of(c[k]);
        }
        f = Pane{W, H, w, h, 3, 3u * (uint32_t)w};
    }
    std::vector<Match> m((size_t)n);
    std::vector<uint8_t> inl((size_t)n);
    rd(in, m.data(), m.size() * sizeof(Match));
    rd(in, inl.data(), inl.size());
    fclose(in);

    const size_t npix = (size_t)W * H;
    std::vector<uint32_t> ovl(npix, 0);
    OverlayPlot plot{f, ovl};
    for (int32_t i = 0; i < n; i++) raster_match(f, m[i], left != 0, (uint32_t)i, plot);
    std::vector<uint8_t> rgb(3 * npix);
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t at = pixel_index(f, x, y);
            resolve_pixel(f, tex.data(), ovl[at], m.data(), inl.data(), x, y, &rgb[3 * at]);
        }
    fwrite(rgb.data(), 1, rgb.size(), stdout);
    return 0;
}

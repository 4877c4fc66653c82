// stereo-vision_amd/csrc/view_core.h built by the host compiler alone (g++ -ffp-contract=off, no HIP): one render
// of a scene with the header's own functions, the two layers filled by plain loops in draw order.
// tests/test_view.py compares its output with the numpy restatement tests/view_ref.py byte for byte.
//
//   view_core_check <job>   job: int32 W, H, show_cams, show_grid, white, ncam, npts; float pose[6];
//                                ncam x (double H_total[16], float s, int32 keyframe); npts x float[4]
//   stdout: W * H * 3 bytes, row 0 = top
//   view_core_check poses <job>   job: int32 n; n x float pose[6]; stdout: the poses of play_sequence, 6 floats each
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../stereo-vision_amd/csrc/view_core.h"

using namespace svh::view;

template <typename T>
static T rd(FILE* f) {
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) {
        fprintf(stderr, "short job file\n");
        exit(2);
    }
    return v;
}

struct DepthPlot {
    const Frame& f;
    std::vector<uint64_t>& key;
    uint32_t index;
    void operator()(int32_t x, int32_t y, uint32_t zb) {
        const uint64_t k = ((uint64_t)zb << 32) | index;
        uint64_t& at = key[pixel_index(f, x, y)];
        if (k < at) at = k;
    }
};

struct OverlayPlot {
    const Frame& f;
    std::vector<uint32_t>& ovl;
    uint32_t value;
    void operator()(int32_t x, int32_t y, uint32_t) { ovl[pixel_index(f, x, y)] = value; }   // drawn in order
};

int main(int argc, char** argv) {
    if (argc == 3) {
        FILE* in = fopen(argv[2], "rb");
        if (!in) return 2;
        const int32_t n = rd<int32_t>(in);
        std::vector<Pose> poses(n), seq;
        for (auto& p : poses) p = rd<Pose>(in);
        play_sequence(poses.data(), n, &seq);
        fwrite(seq.data(), sizeof(Pose), seq.size(), stdout);
        return 0;
    }
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    const int32_t W = rd<int32_t>(in), H = rd<int32_t>(in), show_cams = rd<int32_t>(in), show_grid = rd<int32_t>(in);
    const int32_t white = rd<int32_t>(in), ncam = rd<int32_t>(in), npts = rd<int32_t>(in);
    const Pose pose = rd<Pose>(in);
    std::vector<Cam> cams(ncam);
    for (auto& c : cams) {
        double Ht[16];
        for (double& v : Ht) v = rd<double>(in);
        const float s = rd<float>(in);
        make_camera(Ht, s, rd<int32_t>(in), &c);
    }
    std::vector<float> pts(4 * (size_t)npts);
    for (float& v : pts) v = rd<float>(in);

    Frame f;
    make_frame(pose, W, H, &f);
    std::vector<Seg> segs;
    build_segments(cams.data(), cams.size(), show_grid != 0, show_cams != 0, &segs);
    const size_t npix = (size_t)W * H;
    std::vector<uint64_t> key(npix, EMPTY_KEY);
    std::vector<uint32_t> ovl(npix, 0);
    for (const Seg& s : segs) {
        if (s.flags & SEG_OVERLAY) {
            OverlayPlot plot{f, ovl, s.value};
            raster_segment(f, s, plot);
        } else {
            DepthPlot plot{f, key, s.value};
            raster_segment(f, s, plot);
        }
    }
    int32_t ix, iy;
    uint32_t zb;
    for (int32_t i = 0; i < npts; i++) {
        if (!point_window(f, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], true, &ix, &iy, &zb)) continue;
        DepthPlot plot{f, key, GRID_SEGS + (uint32_t)i};
        for (int32_t dy = -1; dy <= 0; dy++)
            for (int32_t dx = -1; dx <= 0; dx++)
                if (in_image(f, ix + dx, iy + dy)) plot(ix + dx, iy + dy, zb);
    }
    const uint32_t anchor = show_cams ? GRID_SEGS + (uint32_t)npts : NO_ANCHOR;
    if (show_cams && point_window(f, -pose.tx, -pose.ty, -pose.tz, false, &ix, &iy, &zb)) {
        DepthPlot plot{f, key, anchor};
        for (int32_t dy = -1; dy <= 1; dy++)
            for (int32_t dx = -1; dx <= 1; dx++)
                if (in_image(f, ix + dx, iy + dy)) plot(ix + dx, iy + dy, zb);
    }
    std::vector<uint8_t> rgb(3 * npix);
    for (size_t i = 0; i < npix; i++) resolve_pixel(key[i], ovl[i], anchor, pts.data(), white != 0, &rgb[3 * i]);
    fwrite(rgb.data(), 1, rgb.size(), stdout);
    return 0;
}

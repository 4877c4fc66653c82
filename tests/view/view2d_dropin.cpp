// include/view2d.h as a caller of the reference's View2D uses it (maindialog.cpp:451-452, 506-511, 588-598): built with
// only include/ on the path and linked against libsvhip.so by tests/test_view2d_gpu.py.
//
//   view2d_dropin <job.bin> <out_dir>   job.bin: int32 w, h, n; w * h bytes; n x p_match; n x uint8 inlier; w * h floats D
//   writes <out_dir>/left.rgb and right.rgb (w x h panes: setImage + setMatches), disp.ppm (a w/2 x h/2 pane after
//   resizeGL + setDisparity, the right pane's matches still over it) and clear.rgb (the same after clearMatches)
#include <stdio.h>
#include <stdlib.h>

#include "view2d.h"

static bool dump(const std::string& path, const std::vector<uint8_t>& rgb) {
    FILE* out = fopen(path.c_str(), "wb");
    if (!out || rgb.empty()) return false;
    fwrite(rgb.data(), 1, rgb.size(), out);
    return fclose(out) == 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    int32_t head[3];
    if (!in || fread(head, 4, 3, in) != 3) return 2;
    const int32_t w = head[0], h = head[1], n = head[2];
    std::vector<unsigned char> I((size_t)w * h);
    std::vector<Matcher::p_match> m((size_t)n);
    std::vector<unsigned char> flag((size_t)n);
    std::vector<float> D((size_t)w * h);
    if (fread(I.data(), 1, I.size(), in) != I.size()) return 2;
    if (n > 0 && fread(&m[0], sizeof(Matcher::p_match), m.size(), in) != m.size()) return 2;
    if (n > 0 && fread(flag.data(), 1, flag.size(), in) != flag.size()) return 2;
    if (fread(D.data(), 4, D.size(), in) != D.size()) return 2;
    fclose(in);
    std::vector<bool> inliers(flag.begin(), flag.end());

    View2D pane(w, h);
    if (!pane.valid()) {
        fprintf(stderr, "no pane: %s\n", svh_last_error());
        return 3;
    }
    const std::string dir = argv[2];
    pane.setImage(I.data(), w, h);
    pane.setMatches(m, inliers, true);
    if (!dump(dir + "/left.rgb", pane.grabFrameBuffer())) return 4;
    pane.setMatches(m, inliers, false);
    if (!dump(dir + "/right.rgb", pane.grabFrameBuffer())) return 5;
    pane.resizeGL(w / 2, h / 2);
    if (pane.width() != w / 2 || pane.height() != h / 2) return 6;
    pane.setDisparity(D.data(), w, h);
    if (!pane.writePPM(dir + "/disp.ppm")) return 7;
    pane.clearMatches();
    if (!dump(dir + "/clear.rgb", pane.grabFrameBuffer())) return 8;
    pane.resizeGL(0, 5);                                   // refused: the size stays
    if (pane.width() != w / 2) return 9;
    printf("view2d ok\n");
    return 0;
}

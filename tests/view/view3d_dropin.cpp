// include/view3d.h as a caller of the reference's View3D uses it (maindialog.cpp:602-606, :880-890): built with only
// include/ on the path and linked against libsvhip.so by tests/test_view_gpu.py.
//
//   view3d_dropin <points.bin> <out_dir>   points.bin: int32 n0, n1; (n0 + n1) x float[4]: the two lists of one frame
//   writes <out_dir>/render.rgb (32 x 24 x 3 bytes after addCamera x 2 + addPoints) and recordHuman's images
#include <stdio.h>
#include <stdlib.h>

#include "view3d.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    int32_t n[2];
    if (!in || fread(n, 4, 2, in) != 2) return 2;
    std::vector<std::vector<View3D::point_3d>> lists(2);
    for (int k = 0; k < 2; k++)
        for (int32_t i = 0; i < n[k]; i++) {
            float p[4];
            if (fread(p, 4, 4, in) != 4) return 2;
            lists[k].push_back(View3D::point_3d(p[0], p[1], p[2], p[3]));
        }
    fclose(in);

    View3D view(32, 24);
    if (!view.valid()) {
        fprintf(stderr, "no view: %s\n", svh_last_error());
        return 3;
    }
    Matrix H = Matrix::eye(4);
    view.addCamera(H, 0.1f, true);
    H._val[2][3] = 0.8;
    H._val[0][3] = 0.1;
    view.addCamera(H, 0.1f, false);
    std::vector<std::vector<View3D::point_3d>> first(1, lists[1]);
    view.addPoints(first);      // frame 1: one list
    view.addPoints(lists);      // frame 2: drops it, appends both
    view.setGridFlag(true);
    view.setShowCamerasFlag(true);
    view.setWhiteFlag(false);
    std::vector<uint8_t> rgb((size_t)view.width() * view.height() * 3);
    if (view.render(rgb.data()) != 0) return 4;
    const std::string dir = argv[2];
    FILE* out = fopen((dir + "/render.rgb").c_str(), "wb");
    if (!out) return 5;
    fwrite(rgb.data(), 1, rgb.size(), out);
    fclose(out);
    view.addPose();
    view.delPose();
    if (view.playPoses() != 0) return 6;            // no poses: no frames
    if (view.recordHuman(dir) != 102) return 7;
    if (view.getPose().roty != -45.f) return 8;     // the last pose rendered is recordHuman's first again
    view.clearAll();
    printf("view3d ok\n");
    return 0;
}

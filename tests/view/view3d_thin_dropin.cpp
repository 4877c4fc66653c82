// include/view3d.h's additions past the widget, with only include/ on the path: thin(voxel) and getPoints().
//   view3d_thin_dropin <points.bin> <voxel> <out.bin>
// points.bin: int32 nlists, int32 n[nlists], then the points (x, y, z, val floats) of every list back to back.  Each
// list is added on its own (one list per addPoints call appends), the map is thinned, and out.bin receives int64 the
// return value of thin(), int32 nlists, int32 n[nlists] and the points getPoints() returns.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "view3d.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nl = 0;
    if (fread(&nl, 4, 1, f) != 1) return 2;
    std::vector<int32_t> n((size_t)nl);
    if (nl > 0 && fread(n.data(), 4, (size_t)nl, f) != (size_t)nl) return 2;
    View3D view(64, 48);
    if (!view.valid()) return 3;
    for (int32_t i = 0; i < nl; i++) {
        std::vector<std::vector<View3D::point_3d> > lists(1);
        lists[0].resize((size_t)n[i], View3D::point_3d(0, 0, 0, 0));
        if (n[i] > 0 && fread(&lists[0][0].x, 16, (size_t)n[i], f) != (size_t)n[i]) return 2;
        view.addPoints(lists);
    }
    fclose(f);
    const int64_t left = view.thin((float)atof(argv[2]));
    const std::vector<std::vector<View3D::point_3d> > got = view.getPoints();
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    const int32_t gl = (int32_t)got.size();
    fwrite(&left, 8, 1, o);
    fwrite(&gl, 4, 1, o);
    for (size_t i = 0; i < got.size(); i++) {
        const int32_t c = (int32_t)got[i].size();
        fwrite(&c, 4, 1, o);
    }
    for (size_t i = 0; i < got.size(); i++)
        if (!got[i].empty()) fwrite(&got[i][0].x, 16, got[i].size(), o);
    fclose(o);
    return view.thin(0.f) == SVH_ERR_BAD_ARG ? 0 : 4;   // a bad voxel comes back as the error code
}

// Boundary test: the loop of libviso2/matlab/demo_structure_from_motion.m (:27-67) in C++, written against
// include/viso_mono.h and include/reconstruction.h exactly as a caller includes the reference's headers:
// process(I) -> getMatches() + getDeltaMotion() -> Reconstruction::update -> getPoints().
//
//   recon_dropin <frames_dir> point_type min_track_length max_dist min_angle
//
// The odometry runs with bucketing disabled and motion_threshold 1e6, as the fixture's `frames` scene does (the car
// hardly moves in the seven frames).  Prints one line per frame and the final point count.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "reconstruction.h"
#include "viso_mono.h"

static bool read_pgm(const char* path, std::vector<uint8_t>& img, int32_t& w, int32_t& h) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char magic[3] = {0, 0, 0};
    int maxv = 0;
    if (fscanf(f, "%2s %d %d %d", magic, &w, &h, &maxv) != 4 || strcmp(magic, "P5") != 0) {
        fclose(f);
        return false;
    }
    fgetc(f);
    img.resize((size_t)w * h);
    bool ok = fread(img.data(), 1, img.size(), f) == img.size();
    fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s DIR point_type min_track_length max_dist min_angle\n", argv[0]);
        return 2;
    }
    VisualOdometryMono::parameters param;
    param.calib.f = 645.2;
    param.calib.cu = 635.9;
    param.calib.cv = 194.1;
    param.height = 1.6;
    param.pitch = -0.08;
    param.motion_threshold = 1e6;
    param.bucket.max_features = 1000;   // disable bucketing
    VisualOdometryMono viso(param);
    Reconstruction recon;
    recon.setCalibration(param.calib.f, param.calib.cu, param.calib.cv);
    bool replace = false;
    for (int k = 0; k < 7; k++) {
        char path[4096];
        snprintf(path, sizeof(path), "%s/I1_%06d.pgm", argv[1], k);
        std::vector<uint8_t> img;
        int32_t w = 0, h = 0;
        if (!read_pgm(path, img, w, h)) {
            fprintf(stderr, "cannot read %s\n", path);
            return 1;
        }
        int32_t dims[] = {w, h, w};
        const bool ok = viso.process(img.data(), dims, replace);
        if (k == 0) continue;
        if (!ok) {
            replace = true;
        } else {
            recon.update(viso.getMatches(), viso.getDeltaMotion(), atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atof(argv[5]));
            replace = false;
        }
        std::vector<Reconstruction::point3d> p = recon.getPoints();
        printf("frame %d ok %d matches %d tracks %d points %d\n", k, (int)ok, (int)viso.getNumberOfMatches(),
               (int)svh_recon_num_tracks(recon.handle()), (int)p.size());
        for (size_t i = 0; i < p.size(); i++)
            if (!(p[i].x == p[i].x && p[i].y == p[i].y && p[i].z == p[i].z)) return 3;   // NaN
    }
    printf("points %d\n", (int)recon.getPoints().size());
    return 0;
}

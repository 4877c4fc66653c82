// Boundary test: the frame loop of libviso2/matlab/demo_viso_mono.m (:33-56) driven the way
// matlab/visualOdometryMonoMex.cpp:61-120 drives the class -- parameters set field by field,
// new VisualOdometryMono(param), process(I, dims, replace), getDeltaMotion -- compiled against
// include/viso_mono.h exactly as a caller includes the reference's header.
//
//   mono_dropin seq <frames_dir> <demo_replace 0|1> f cu cv height pitch ransac_iters inlier_threshold
//               motion_threshold max_features bucket_width bucket_height
//
// Output (stdout, binary) per frame, the format of tests/mono/ref_mono_harness.cpp: int32 ok, int32 n, n matches
// (getMatches), int32 n_inliers, the inlier indices, 16 doubles getDeltaMotion (row major).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }
static void put_i(int32_t v) { put(&v, 4); }

int main(int argc, char** argv) {
    if (argc < 15 || strcmp(argv[1], "seq") != 0) {
        fprintf(stderr, "usage: %s seq DIR DEMO_REPLACE f cu cv height pitch iters thr motion_thr mf bw bh\n", argv[0]);
        return 2;
    }
    char** a = argv + 4;
    VisualOdometryMono::parameters param;
    param.calib.f = atof(a[0]);
    param.calib.cu = atof(a[1]);
    param.calib.cv = atof(a[2]);
    param.height = atof(a[3]);
    param.pitch = atof(a[4]);
    param.ransac_iters = atoi(a[5]);
    param.inlier_threshold = atof(a[6]);
    param.motion_threshold = atof(a[7]);
    param.bucket.max_features = atoi(a[8]);
    param.bucket.bucket_width = atof(a[9]);
    param.bucket.bucket_height = atof(a[10]);
    const bool demo_replace = atoi(argv[3]) != 0;
    VisualOdometryMono* viso = new VisualOdometryMono(param);
    bool replace = false;
    for (int k = 0; k < 7; k++) {
        char path[4096];
        snprintf(path, sizeof(path), "%s/I1_%06d.pgm", argv[2], k);
        std::vector<uint8_t> img;
        int32_t w = 0, h = 0;
        if (!read_pgm(path, img, w, h)) {
            fprintf(stderr, "cannot read %s\n", path);
            return 1;
        }
        int32_t dims[] = {w, h, w};
        const bool ok = viso->process(img.data(), dims, replace);
        if (demo_replace && k > 0) replace = !ok;
        put_i(ok);
        std::vector<Matcher::p_match> m = viso->getMatches();
        put_i((int32_t)m.size());
        if (!m.empty()) put(m.data(), m.size() * sizeof(Matcher::p_match));
        std::vector<int32_t> inl = viso->getInlierIndices();
        put_i((int32_t)inl.size());
        if (!inl.empty()) put(inl.data(), inl.size() * 4);
        Matrix T = viso->getDeltaMotion();
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) put(&T._val[i][j], 8);
    }
    delete viso;
    return 0;
}

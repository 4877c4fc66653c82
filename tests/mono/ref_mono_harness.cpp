// Driver of the reference's VisualOdometryMono for tests/golden/make_goldens_mono.py (and the live check in
// tests/test_vo_mono.py).  Linked against libviso2/src/{matcher,filter,matrix,triangle,viso}.cpp and viso_mono.cpp
// (the latter with tests/mono/mono_prelude.h force-included).  Never part of the library.
//
//   ref_mono_harness seq <frames_dir> <demo_replace 0|1> P...    the seven frames I1_00000k.pgm through process()
//   ref_mono_harness est <matches.bin> P...                      VisualOdometry::process(p_matched), fresh object,
//                                                                then the RANSAC loop replayed for its vote counts
//   ref_mono_harness bench <frames_dir> <reps> <matches.bin> P... timing (text): ms per process() of frames 1-6 on a
//                                                                fresh object per repetition, ms per estimate
// P = f cu cv height pitch ransac_iters inlier_threshold motion_threshold max_features bucket_width bucket_height
// Output (stdout, binary little endian), per frame / case:
//   int32 ok, int32 n_matches, n_matches x p_match (seq only), int32 n_inliers, n_inliers x int32, 16 x double
//   (getDeltaMotion, row major); est then adds int32 iters, iters x int32 (inliers of each RANSAC hypothesis;
//   iters = 0 when the estimate returns before the loop).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#define private public
#define protected public
#include "viso_mono.h"
#undef private
#undef protected

static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }
static void put_i(int32_t v) { put(&v, 4); }

static std::vector<uint8_t> read_pgm(const char* path, int32_t& w, int32_t& h) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    int mx;
    if (fscanf(f, "P5 %d %d %d", &w, &h, &mx) != 3) exit(2);
    fgetc(f);
    std::vector<uint8_t> b((size_t)w * h);
    if (fread(b.data(), 1, b.size(), f) != b.size()) exit(2);
    fclose(f);
    return b;
}

static VisualOdometryMono::parameters parse(char** a) {
    VisualOdometryMono::parameters p;
    p.calib.f = atof(a[0]);
    p.calib.cu = atof(a[1]);
    p.calib.cv = atof(a[2]);
    p.height = atof(a[3]);
    p.pitch = atof(a[4]);
    p.ransac_iters = atoi(a[5]);
    p.inlier_threshold = atof(a[6]);
    p.motion_threshold = atof(a[7]);
    p.bucket.max_features = atoi(a[8]);
    p.bucket.bucket_width = atof(a[9]);
    p.bucket.bucket_height = atof(a[10]);
    return p;
}

static void put_state(VisualOdometryMono& vo) {
    std::vector<int32_t> inl = vo.getInlierIndices();
    put_i((int32_t)inl.size());
    if (!inl.empty()) put(inl.data(), inl.size() * 4);
    Matrix T = vo.getDeltaMotion();
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) put(&T._val[i][j], 8);
}

int main(int argc, char** argv) {
    if (argc >= 15 && !strcmp(argv[1], "seq")) {
        VisualOdometryMono::parameters p = parse(argv + 4);
        const bool demo_replace = atoi(argv[3]) != 0;
        VisualOdometryMono vo(p);
        bool replace = false;
        for (int k = 0; k < 7; k++) {
            char path[4096];
            snprintf(path, sizeof(path), "%s/I1_%06d.pgm", argv[2], k);
            int32_t w, h;
            std::vector<uint8_t> im = read_pgm(path, w, h);
            int32_t dims[3] = {w, h, w};
            const bool ok = vo.process(im.data(), dims, replace);
            if (demo_replace && k > 0) replace = !ok;   // demo_viso_mono.m:33-56
            put_i(ok);
            std::vector<Matcher::p_match> m = vo._p_matched;
            put_i((int32_t)m.size());
            if (!m.empty()) put(m.data(), m.size() * sizeof(Matcher::p_match));
            put_state(vo);
        }
        return 0;
    }
    if (argc >= 14 && !strcmp(argv[1], "est")) {
        VisualOdometryMono::parameters p = parse(argv + 3);
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        int32_t N;
        if (fread(&N, 4, 1, f) != 1) return 2;
        std::vector<Matcher::p_match> m(N);
        if (N && fread(m.data(), sizeof(Matcher::p_match), N, f) != (size_t)N) return 2;
        fclose(f);
        {
            VisualOdometryMono vo(p);   // srand(0)
            const bool ok = vo.VisualOdometry::process(m);
            put_i(ok);
            put_state(vo);
        }
        // viso_mono.cpp:45-70 once more on a fresh object: the same random stream, every hypothesis' inlier count
        VisualOdometryMono vo(p);
        std::vector<int32_t> votes;
        std::vector<Matcher::p_match> q = m;
        Matrix Tp, Tc, F;
        if (N >= 10 && vo.normalizeFeaturePoints(q, Tp, Tc)) {
            for (int32_t k = 0; k < p.ransac_iters; k++) {
                std::vector<int32_t> active = vo.getRandomSample(N, 8);
                vo.fundamentalMatrix(q, active, F);
                votes.push_back((int32_t)vo.getInlier(q, F).size());
            }
        }
        put_i((int32_t)votes.size());
        if (!votes.empty()) put(votes.data(), votes.size() * 4);
        return 0;
    }
    if (argc >= 16 && !strcmp(argv[1], "bench")) {
        VisualOdometryMono::parameters p = parse(argv + 5);
        const int reps = atoi(argv[3]);
        std::vector<std::vector<uint8_t> > im(7);
        int32_t w = 0, h = 0;
        for (int k = 0; k < 7; k++) {
            char path[4096];
            snprintf(path, sizeof(path), "%s/I1_%06d.pgm", argv[2], k);
            im[k] = read_pgm(path, w, h);
        }
        int32_t dims[3] = {w, h, w};
        auto now = [] { return std::chrono::steady_clock::now(); };
        std::vector<double> frame_ms, est_ms;
        for (int r = 0; r < reps; r++) {
            VisualOdometryMono vo(p);
            for (int k = 0; k < 7; k++) {
                const auto t0 = now();
                vo.process(im[k].data(), dims, false);
                const double ms = std::chrono::duration<double, std::milli>(now() - t0).count();
                if (k) frame_ms.push_back(ms);
            }
        }
        FILE* f = fopen(argv[4], "rb");
        if (!f) return 2;
        int32_t N;
        if (fread(&N, 4, 1, f) != 1) return 2;
        std::vector<Matcher::p_match> m(N);
        if (N && fread(m.data(), sizeof(Matcher::p_match), N, f) != (size_t)N) return 2;
        fclose(f);
        VisualOdometryMono vo(p);
        for (int r = 0; r < reps; r++) {
            const auto t0 = now();
            vo.VisualOdometry::process(m);
            est_ms.push_back(std::chrono::duration<double, std::milli>(now() - t0).count());
        }
        std::sort(frame_ms.begin(), frame_ms.end());
        std::sort(est_ms.begin(), est_ms.end());
        printf("process_ms_median %.3f min %.3f n %d\n", frame_ms[frame_ms.size() / 2], frame_ms[0], (int)frame_ms.size());
        printf("estimate_ms_median %.3f min %.3f N %d\n", est_ms[est_ms.size() / 2], est_ms[0], N);
        return 0;
    }
    fprintf(stderr, "usage: ref_mono_harness seq DIR DEMO_REPLACE P... | est MATCHES P... | bench DIR REPS MATCHES P...\n");
    return 1;
}

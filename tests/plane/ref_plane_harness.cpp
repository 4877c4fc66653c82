// Driver of the reference's PlaneEstimation for tests/golden/make_goldens_plane.py (and the live check in
// tests/test_plane.py).  Linked against libviso2/src/matrix.cpp and stereomapper/planeestimation.cpp, the latter
// compiled unchanged with tests/plane/plane_prelude.h force-included (time -> the seed, rand -> counted, private ->
// public).  Never part of the library.
//
//   ref_plane_harness run   <job>
//   ref_plane_harness bench <job> reps
// Job file (binary, little endian): int32 n_calls, then per call int32 width, height, step, float f, cu, cv, base,
// uint32 seed, height * step floats.  All calls run on ONE PlaneEstimation object, in order (_pitch carries over).
// run writes to stdout per call:
//   int32 status (0: more than 3 inliers, 3: not), 3 doubles _plane_d, 3 doubles _plane_e, 16 doubles _H, float _pitch,
//   int32 n, n x 3 floats (the list), int32 S, S x 3 doubles (plane per hypothesis), S x int32 draws consumed,
//   S x int32 votes, int32 best hypothesis (-1: none), int32 n_in, n_in x int32 inlier indices of the best.
// The final outputs come from the whole call; the per-hypothesis records from a second object that this driver steps
// through sparseDisparityGrid / drawRandomPlaneSample with the same seed and its own copy of the vote loop.  The
// driver stops with an error unless both routes end with the same _plane_d.  bench prints the time of the call (text).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <chrono>
#include <vector>

#define private public
#include "planeestimation.h"
#undef private

static uint32_t g_seed = 0;
static long long g_draws = 0;
time_t plane_harness_time() { return (time_t)g_seed; }
int plane_harness_rand() {
    g_draws++;
    return rand();
}

struct Call {
    int32_t width, height, step;
    float f, cu, cv, base;
    uint32_t seed;
    std::vector<float> D;
};

static std::vector<Call> read_job(const char* path) {
    FILE* fp = fopen(path, "rb");
    if (!fp) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    int32_t n;
    if (fread(&n, 4, 1, fp) != 1) exit(2);
    std::vector<Call> calls(n);
    for (Call& c : calls) {
        if (fread(&c.width, 4, 3, fp) != 3 || fread(&c.f, 4, 4, fp) != 4 || fread(&c.seed, 4, 1, fp) != 1) exit(2);
        c.D.resize((size_t)c.height * c.step);
        if (fread(c.D.data(), 4, c.D.size(), fp) != c.D.size()) exit(2);
    }
    fclose(fp);
    return calls;
}

static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }
static void put_i(int32_t v) { put(&v, 4); }

int main(int argc, char** argv) {
    if (argc < 3 || (strcmp(argv[1], "run") && strcmp(argv[1], "bench"))) {
        fprintf(stderr, "usage: ref_plane_harness run|bench JOB [reps]\n");
        return 1;
    }
    std::vector<Call> calls = read_job(argv[2]);
    if (!strcmp(argv[1], "bench")) {
        const int reps = argc > 3 ? atoi(argv[3]) : 5;
        for (size_t k = 0; k < calls.size(); k++) {
            Call& c = calls[k];
            std::vector<double> ms;
            PlaneEstimation P;
            for (int r = 0; r < reps; r++) {
                g_seed = c.seed;
                const auto t0 = std::chrono::steady_clock::now();
                P.computeTransformationFromDisparityMap(c.D.data(), c.width, c.height, c.step, c.f, c.cu, c.cv, c.base);
                ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("call %d ms_median %.3f min %.3f max %.3f reps %d\n", (int)k, ms[ms.size() / 2], ms.front(), ms.back(),
                   reps);
        }
        return 0;
    }
    PlaneEstimation P;
    for (size_t k = 0; k < calls.size(); k++) {
        Call& c = calls[k];
        // ---- the whole call
        g_seed = c.seed;
        g_draws = 0;
        P.computeTransformationFromDisparityMap(c.D.data(), c.width, c.height, c.step, c.f, c.cu, c.cv, c.base);
        const long long whole_draws = g_draws;

        // ---- the same, stepped (planeestimation.cpp:32-69 with the reference's own private members)
        PlaneEstimation Q;
        int32_t roi[4] = {0, c.height / 3, c.width - 1, c.height - 1};
        const int32_t num_samples = 5000;
        const FLOAT d_threshold = 5;
        srand(c.seed);
        g_draws = 0;
        std::vector<PlaneEstimation::disp> list = Q.sparseDisparityGrid(c.D.data(), c.width, c.height, c.step, roi, 5);
        std::vector<double> planes;
        std::vector<int32_t> draws, votes, curr, best_inlier;
        int32_t best = -1;
        for (int32_t i = 0; i < num_samples; i++) {
            const long long before = g_draws;
            Q.drawRandomPlaneSample(list);
            draws.push_back((int32_t)(g_draws - before));
            for (int j = 0; j < 3; j++) planes.push_back(Q._plane_d._val[j][0]);
            curr.clear();
            for (int32_t j = 0; j < (int32_t)list.size(); j++) {
                float result = Q._plane_d._val[0][0] * list[j].u + Q._plane_d._val[1][0] * list[j].v +
                               Q._plane_d._val[2][0] - list[j].d;
                if (fabs(result) < d_threshold) curr.push_back(j);
            }
            votes.push_back((int32_t)curr.size());
            if (curr.size() > best_inlier.size()) {
                best_inlier = curr;
                best = i;
            }
        }
        const bool enough = best_inlier.size() > 3;
        if (enough) Q.leastSquarePlane(list, best_inlier);
        double pd[3], qd[3];
        for (int j = 0; j < 3; j++) {
            pd[j] = P._plane_d._val[j][0];
            qd[j] = Q._plane_d._val[j][0];
        }
        if (memcmp(pd, qd, sizeof(pd)) || whole_draws != g_draws) {
            fprintf(stderr, "call %d: the stepped run does not end where the whole call does (draws %lld / %lld)\n",
                    (int)k, g_draws, whole_draws);
            return 3;
        }
        put_i(enough ? 0 : 3);
        put(pd, sizeof(pd));
        double e[3], H[16];
        for (int j = 0; j < 3; j++) e[j] = P._plane_e._val[j][0];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) H[4 * i + j] = P._H._val[i][j];
        put(e, sizeof(e));
        put(H, sizeof(H));
        const float pitch = P.getPitch();
        put(&pitch, 4);
        put_i((int32_t)list.size());
        for (size_t j = 0; j < list.size(); j++) {
            const float t[3] = {list[j].u, list[j].v, list[j].d};
            put(t, sizeof(t));
        }
        put_i(num_samples);
        put(planes.data(), 8 * planes.size());
        put(draws.data(), 4 * draws.size());
        put(votes.data(), 4 * votes.size());
        put_i(best);
        put_i((int32_t)best_inlier.size());
        if (!best_inlier.empty()) put(best_inlier.data(), 4 * best_inlier.size());
    }
    return 0;
}

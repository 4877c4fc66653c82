// Driver of the reference's Reconstruction for tests/golden/make_goldens_recon.py (and the live check in
// tests/test_recon.py).  Linked against libviso2/src/matrix.cpp and reconstruction.cpp (the latter with
// tests/recon/recon_prelude.h force-included).  Never part of the library.
//
//   ref_recon_harness run   <scene> f cu cv point_type min_track_length max_dist min_angle
//   ref_recon_harness bench <scene> f cu cv point_type min_track_length max_dist min_angle reps
// Scene file (binary, little endian): int32 n_updates, then per update 16 doubles Tr (row major), int32 n and n
// matches of 24 bytes: float u1p, float v1p, int32 i1p, float u1c, float v1c, int32 i1c.
// run writes to stdout per update:
//   int32 n_active (tracks alive after the update), int32 n_appended, n_appended x 3 floats (the points update()
//   appended), int32 n_lost, n_lost x int32 outcome code, n_lost x 3 floats (the point as far as it got).
// The outcomes come from the reference's own private initPoint / pointType / refinePoint / pointDistance / rayAngle,
// called on the tracks this driver finds lost with its own copy of the association loop; the driver stops with an
// error unless the tracks it calls ACCEPTED are exactly the points update() appended and its active count is
// update()'s.  bench prints the time of update() (text).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#define private public
#include "reconstruction.h"
#undef private

enum { TOO_SHORT, INIT_FAILED, TYPE_BELOW, REFINE_FAILED, TOO_FAR, ANGLE_SMALL, ACCEPTED };

struct M6 {
    float u1p, v1p;
    int32_t i1p;
    float u1c, v1c;
    int32_t i1c;
};
struct Update {
    double Tr[16];
    std::vector<Matcher::p_match> m;
};

static std::vector<Update> read_scene(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    int32_t nu;
    if (fread(&nu, 4, 1, f) != 1) exit(2);
    std::vector<Update> s(nu);
    for (Update& u : s) {
        int32_t n;
        if (fread(u.Tr, 8, 16, f) != 16 || fread(&n, 4, 1, f) != 1) exit(2);
        std::vector<M6> m(n);
        if (n && fread(m.data(), sizeof(M6), n, f) != (size_t)n) exit(2);
        for (const M6& a : m) {
            Matcher::p_match p;
            memset(&p, 0, sizeof(p));
            p.u1p = a.u1p; p.v1p = a.v1p; p.i1p = a.i1p;
            p.u1c = a.u1c; p.v1c = a.v1c; p.i1c = a.i1c;
            u.m.push_back(p);
        }
    }
    fclose(f);
    return s;
}

static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }
static void put_i(int32_t v) { put(&v, 4); }

// the tracks that update() is about to lose, in its order, and how many stay alive
static std::vector<Reconstruction::track> lost_tracks(const Reconstruction& R, const std::vector<Matcher::p_match>& m,
                                                      int32_t& n_active) {
    std::vector<Reconstruction::track> tr = R.tracks;
    const int32_t cur = (int32_t)R.Tr_total.size();   // the frame number update() will give this frame
    const size_t old = tr.size();
    int32_t top = 0;
    for (size_t i = 0; i < m.size(); i++) top = std::max(top, m[i].i1p);
    for (size_t i = 0; i < old; i++) top = std::max(top, tr[i].last_idx);
    std::vector<int32_t> slot((size_t)top + 1, -1);
    for (size_t i = 0; i < old; i++) slot[tr[i].last_idx] = (int32_t)i;
    size_t created = 0;
    for (size_t i = 0; i < m.size(); i++) {
        const int32_t k = slot[m[i].i1p];
        if (k >= 0 && tr[k].last_frame == cur - 1) {
            tr[k].last_frame = cur;
            tr[k].last_idx = m[i].i1c;
        } else {
            created++;
        }
    }
    std::vector<Reconstruction::track> lost;
    for (size_t i = 0; i < old; i++)
        if (tr[i].last_frame != cur) lost.push_back(tr[i]);
    n_active = (int32_t)(old - lost.size() + created);
    return lost;
}

int main(int argc, char** argv) {
    if (argc < 10 || (strcmp(argv[1], "run") && strcmp(argv[1], "bench"))) {
        fprintf(stderr, "usage: ref_recon_harness run|bench SCENE f cu cv point_type min_track_length max_dist min_angle [reps]\n");
        return 1;
    }
    const std::vector<Update> scene = read_scene(argv[2]);
    const double f = atof(argv[3]), cu = atof(argv[4]), cv = atof(argv[5]);
    const int32_t point_type = atoi(argv[6]), min_len = atoi(argv[7]);
    const double max_dist = atof(argv[8]), min_angle = atof(argv[9]);
    if (!strcmp(argv[1], "bench")) {
        const int reps = argc > 10 ? atoi(argv[10]) : 5;
        std::vector<double> ms, total;
        size_t points = 0;
        for (int r = 0; r < reps; r++) {
            Reconstruction R;
            R.setCalibration(f, cu, cv);
            double sum = 0;
            for (const Update& u : scene) {
                const Matrix Tr(4, 4, u.Tr);
                const auto t0 = std::chrono::steady_clock::now();
                R.update(u.m, Tr, point_type, min_len, max_dist, min_angle);
                const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                ms.push_back(d);
                sum += d;
            }
            total.push_back(sum);
            points = R.getPoints().size();
        }
        std::sort(ms.begin(), ms.end());
        std::sort(total.begin(), total.end());
        printf("update_ms_median %.4f mean %.4f max %.4f updates %d points %d\n", ms[ms.size() / 2],
               total[total.size() / 2] / scene.size(), ms.back(), (int)scene.size(), (int)points);
        return 0;
    }
    Reconstruction R;
    R.setCalibration(f, cu, cv);
    for (size_t k = 0; k < scene.size(); k++) {
        const Update& u = scene[k];
        int32_t n_active = 0;
        std::vector<Reconstruction::track> lost = lost_tracks(R, u.m, n_active);
        const size_t before = R.points.size();
        R.update(u.m, Matrix(4, 4, u.Tr), point_type, min_len, max_dist, min_angle);
        if ((int32_t)R.tracks.size() != n_active) {
            fprintf(stderr, "update %d: %d active tracks, the driver expected %d\n", (int)k, (int)R.tracks.size(), n_active);
            return 3;
        }
        std::vector<int32_t> code;
        std::vector<float> xyz;
        std::vector<float> accepted;
        for (size_t i = 0; i < lost.size(); i++) {
            const Reconstruction::track& t = lost[i];
            Reconstruction::point3d p(0, 0, 0);
            int32_t c;
            if (!(t.pixels.size() >= min_len)) c = TOO_SHORT;
            else if (!R.initPoint(t, p)) { c = INIT_FAILED; p = Reconstruction::point3d(0, 0, 0); }
            else if (!(R.pointType(t, p) >= point_type)) c = TYPE_BELOW;
            else if (!R.refinePoint(t, p)) c = REFINE_FAILED;
            else if (!(R.pointDistance(t, p) < max_dist)) c = TOO_FAR;
            else if (!(R.rayAngle(t, p) > min_angle)) c = ANGLE_SMALL;
            else c = ACCEPTED;
            code.push_back(c);
            xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z);
            if (c == ACCEPTED) { accepted.push_back(p.x); accepted.push_back(p.y); accepted.push_back(p.z); }
        }
        const size_t appended = R.points.size() - before;
        if (accepted.size() != 3 * appended ||
            (appended && memcmp(accepted.data(), &R.points[before], 12 * appended))) {
            fprintf(stderr, "update %d: the driver's accepted tracks are not what update() appended\n", (int)k);
            return 3;
        }
        put_i((int32_t)R.tracks.size());
        put_i((int32_t)appended);
        if (appended) put(&R.points[before], 12 * appended);
        put_i((int32_t)lost.size());
        if (!lost.empty()) {
            put(code.data(), 4 * code.size());
            put(xyz.data(), 4 * xyz.size());
        }
    }
    return 0;
}

// K monocular sequences in one process through the C-ABI alone (include/svh.h): the frame loop of demo_viso_mono.m
// (process(I, replace), replace = !ok from the second frame on) for K VisualOdometryMono objects -- once as K
// svh_vo_mono_process calls per frame, once as ONE svh_vo_mono_process_batch per frame, once as the pipelined loop
// (svh_vo_mono_prefetch_batch / svh_vo_mono_process_next_batch).  Sequence k starts at frame k of the directory
// (cyclically), so the objects of a batch differ in their images, their match counts and their `replace`.  With equal
// srand() the three loops must agree bit for bit.  The counterpart of tests/cxx/vo_lockstep.cpp.
//
//   mono_lockstep DIR [K] [frames] [motion_threshold]     DIR holds I1_000000.pgm .. I1_000006.pgm
//   prints "mono_lockstep: OK ..." or the mismatch
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "svh.h"

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
    const bool ok = fread(img.data(), 1, img.size(), f) == img.size();
    fclose(f);
    return ok;
}

struct Log {   // what the caller of a frame sees, per object
    std::vector<int32_t> ok, inliers, votes;   // inliers / votes: count, then the values
    std::vector<double> motion;                // 16 per (frame, object)
    std::vector<svh_p_match> matches;
};

static void record(Log& log, svh_vo* v, int32_t ok) {
    log.ok.push_back(ok);
    double T[16];
    svh_vo_get_motion(v, T);
    log.motion.insert(log.motion.end(), T, T + 16);
    int32_t n = svh_vo_get_inliers(v, 0, 0);
    std::vector<int32_t> a((size_t)n + 1);
    svh_vo_get_inliers(v, a.data(), n);
    log.inliers.push_back(n);
    log.inliers.insert(log.inliers.end(), a.begin(), a.begin() + n);
    n = svh_vo_mono_get_votes(v, 0, 0);
    a.resize((size_t)n + 1);
    svh_vo_mono_get_votes(v, a.data(), n);
    log.votes.push_back(n);
    log.votes.insert(log.votes.end(), a.begin(), a.begin() + n);
    n = svh_vo_get_matches(v, 0, 0);
    std::vector<svh_p_match> m((size_t)n + 1);
    svh_vo_get_matches(v, m.data(), n);
    log.matches.insert(log.matches.end(), m.begin(), m.begin() + n);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s DIR [K] [frames] [motion_threshold]\n", argv[0]);
        return 2;
    }
    const int K = argc > 2 ? atoi(argv[2]) : 4, frames = argc > 3 ? atoi(argv[3]) : 7;
    const int NF = 7;
    std::vector<uint8_t> im[NF];
    int32_t w = 0, h = 0;
    for (int k = 0; k < NF; k++) {
        char name[64];
        snprintf(name, sizeof(name), "/I1_%06d.pgm", k);
        if (!read_pgm((std::string(argv[1]) + name).c_str(), im[k], w, h)) {
            fprintf(stderr, "cannot read %s%s\n", argv[1], name);
            return 2;
        }
    }
    svh_vo_mono_params param;   // demo_viso_mono.m
    svh_vo_mono_params_default(&param);
    param.f = 645.2;
    param.cu = 635.9;
    param.cv = 194.1;
    param.height = 1.6;
    param.pitch = -0.08;
    param.motion_threshold = argc > 4 ? atof(argv[4]) : 1e6;
    const int32_t dims[3] = {w, h, w};

    Log log[3];
    for (int mode = 0; mode < 3; mode++) {
        std::vector<svh_vo*> vos(K);
        for (int k = 0; k < K; k++)
            if (!(vos[k] = svh_vo_mono_create(&param))) return 3;
        srand(4711);   // (the constructors called srand(0), viso.cpp:36)
        std::vector<const uint8_t*> I(K), N(K);
        std::vector<int32_t> ok(K, 0), replace(K, 0);
        auto frame_ptrs = [&](int i, std::vector<const uint8_t*>& a) {
            for (int k = 0; k < K; k++) a[k] = im[(i + k) % NF].data();
        };
        if (mode == 2) {
            frame_ptrs(0, I);
            if (svh_vo_mono_prefetch_batch(vos.data(), K, I.data(), dims) < 0) return 3;
        }
        for (int i = 0; i < frames; i++) {
            frame_ptrs(i, I);
            int32_t rc = 0;
            if (mode == 0) {
                for (int k = 0; k < K && rc >= 0; k++) rc = ok[k] = svh_vo_mono_process(vos[k], I[k], dims, replace[k]);
            } else if (mode == 1) {
                rc = svh_vo_mono_process_batch(vos.data(), K, I.data(), dims, replace.data(), ok.data());
            } else {
                const bool more = i + 1 < frames;
                if (more) frame_ptrs(i + 1, N);
                rc = svh_vo_mono_process_next_batch(vos.data(), K, more ? N.data() : 0, dims, replace.data(), ok.data());
            }
            if (rc < 0) {
                printf("mono_lockstep: mode %d frame %d: error %d: %s\n", mode, i, rc, svh_last_error());
                return 3;
            }
            for (int k = 0; k < K; k++) {
                record(log[mode], vos[k], ok[k]);
                if (i > 0) replace[k] = !ok[k];   // demo_viso_mono.m: a failed frame keeps the previous one
            }
        }
        for (int k = 0; k < K; k++) svh_vo_destroy(vos[k]);
    }
    int good = 0;
    for (size_t i = 0; i < log[0].ok.size(); i++) good += log[0].ok[i];
    for (int mode = 1; mode < 3; mode++) {
        const char* name = mode == 1 ? "process_batch" : "process_next_batch";
        if (log[mode].ok != log[0].ok) { printf("mono_lockstep: %s: return values differ\n", name); return 1; }
        if (log[mode].matches.size() != log[0].matches.size() ||
            memcmp(log[mode].matches.data(), log[0].matches.data(), log[0].matches.size() * sizeof(svh_p_match)) != 0) {
            printf("mono_lockstep: %s: matches differ\n", name);
            return 1;
        }
        if (log[mode].votes != log[0].votes) { printf("mono_lockstep: %s: votes differ\n", name); return 1; }
        if (log[mode].inliers != log[0].inliers) { printf("mono_lockstep: %s: inlier sets differ\n", name); return 1; }
        if (log[mode].motion.size() != log[0].motion.size() ||
            memcmp(log[mode].motion.data(), log[0].motion.data(), log[0].motion.size() * sizeof(double)) != 0) {
            printf("mono_lockstep: %s: motions differ\n", name);
            return 1;
        }
    }
    printf("mono_lockstep: OK %d objects x %d frames, %d motion updates, three loops bit-identical\n", K, frames, good);
    return good > 0 ? 0 : 1;
}

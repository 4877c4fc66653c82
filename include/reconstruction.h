/*
 * reconstruction.h -- source-compatible stand-in for libviso2/src/reconstruction.h.
 *
 * class Reconstruction with the reference's public interface (:35-69): point3d, setCalibration(f,cu,cv),
 * update(p_matched,Tr,point_type=1,min_track_length=2,max_dist=30,min_angle=2) and getPoints(), over the svh_recon_*
 * entries of svh.h, so a caller written against the reference (e.g. matlab/reconstructionMex.cpp, the loop of
 * matlab/demo_structure_from_motion.m) compiles unchanged and runs on the MI355X: the tracks are kept on the host
 * (or, with the opt-in constructor argument, in device memory), every lost track is triangulated, refined and tested
 * on the device (reconstruction.cpp:131-349).
 *
 * Two misuses the reference leaves undefined are refused (the call does nothing): update() before
 * setCalibration() (P_total is empty there) and a second setCalibration() (it would misalign P_total).
 */
#ifndef RECONSTRUCTION_H
#define RECONSTRUCTION_H

#include <stdint.h>

#include <vector>

#include "matcher.h"
#include "matrix.h"
#include "svh.h"

class Reconstruction {
public:
    Reconstruction() : _r(svh_recon_create()) {}
    // extension: resident = true keeps the track table in device memory for the object's lifetime
    // (svh_recon_create_resident, svh.h); such objects can be updated K at a time by svh_recon_update_batch(handle()s)
    explicit Reconstruction(bool resident) : _r(resident ? svh_recon_create_resident() : svh_recon_create()) {}
    ~Reconstruction() { svh_recon_destroy(_r); }

    // a generic 3d point
    struct point3d {
        float x, y, z;
        point3d() {}
        point3d(float x, float y, float z) : x(x), y(y), z(z) {}
    };

    // set calibration parameters (intrinsics), must be called exactly once
    void setCalibration(FLOAT f, FLOAT cu, FLOAT cv) { svh_recon_set_calibration(_r, f, cu, cv); }

    // takes a set of monocular feature matches (flow method) and the egomotion estimate between the 2 frames Tr,
    // associates the features with previous frames (tracking) and computes 3d points once tracks get lost.
    // point types: 0 everything, 1 road and above, 2 only above road
    void update(std::vector<Matcher::p_match> p_matched, Matrix Tr, int32_t point_type = 1,
                int32_t min_track_length = 2, double max_dist = 30, double min_angle = 2) {
        if (Tr._m != 4 || Tr._n != 4) return;
        double T[16];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) T[4 * i + j] = Tr._val[i][j];
        static_assert(sizeof(Matcher::p_match) == sizeof(svh_p_match), "p_match layout");
        svh_recon_update(_r, reinterpret_cast<const svh_p_match*>(p_matched.data()), (int32_t)p_matched.size(), T,
                         point_type, min_track_length, max_dist, min_angle);
    }

    // return currently computed 3d points (finished tracks)
    std::vector<point3d> getPoints() {
        std::vector<point3d> p((size_t)svh_recon_num_points(_r), point3d(0, 0, 0));
        if (!p.empty()) svh_recon_get_points(_r, &p[0].x, (int32_t)p.size());
        return p;
    }

    // ---- extension (not in the reference) ----
    svh_recon* handle() { return _r; }   // for the svh_recon_* getters (outcomes, tracks, resident points, timing)

private:
    Reconstruction(const Reconstruction&);
    Reconstruction& operator=(const Reconstruction&);
    svh_recon* _r;
};

#endif  // RECONSTRUCTION_H

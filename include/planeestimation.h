/*
 * planeestimation.h -- source-compatible stand-in for stereomapper/planeestimation.h.
 *
 * class PlaneEstimation with the reference's public interface (:11-19): computeTransformationFromDisparityMap(D,
 * width, height, step, f, cu, cv, base), getTransformation(), getPlaneDsi(), getPlaneEuclidean(), getPitch(), over
 * the svh_plane_* entries of svh_plane.h, so a caller written against the reference (stereothread.cpp:155-163)
 * compiles unchanged and runs on the MI355X.  Like the reference it seeds with time(NULL); unlike the reference it
 * does not reseed the process-wide rand(): the draws come from a private generator with glibc's sequence.  An empty
 * list (no lattice point with d >= 1) leaves zero planes and the identity instead of dividing by zero.
 */
#ifndef PLANEESTIMATION_H
#define PLANEESTIMATION_H

#include <stdint.h>
#include <time.h>

#include "matrix.h"
#include "svh_plane.h"

class PlaneEstimation {
public:
    PlaneEstimation() : _p(svh_plane_create(0)) {}
    ~PlaneEstimation() { svh_plane_destroy(_p); }

    void computeTransformationFromDisparityMap(float* D, int32_t width, int32_t height, int32_t step, float f, float cu,
                                               float cv, float base) {
        svh_plane_estimate(_p, D, 0, width, height, step, f, cu, cv, base, (uint32_t)time(NULL));
    }
    Matrix getTransformation() {
        double H[16];
        svh_plane_get_transformation(_p, H);
        return Matrix(4, 4, H);
    }
    Matrix getPlaneDsi() {
        double v[3];
        svh_plane_get_plane_dsi(_p, v);
        return Matrix(3, 1, v);
    }
    Matrix getPlaneEuclidean() {
        double v[3];
        svh_plane_get_plane_euclidean(_p, v);
        return Matrix(3, 1, v);
    }
    float getPitch() { return svh_plane_get_pitch(_p); }

    // ---- extension (not in the reference) ----
    // the same call with the caller's seed (the draws of srand(seed)) and, with d_on_device, a device-resident map
    // (what svh_elas_process_batch_device leaves); returns the status of svh_plane_estimate
    int32_t computeTransformationFromDisparityMap(const float* D, bool d_on_device, int32_t width, int32_t height,
                                                  int32_t step, float f, float cu, float cv, float base, uint32_t seed) {
        return svh_plane_estimate(_p, D, d_on_device ? 1 : 0, width, height, step, f, cu, cv, base, seed);
    }
    svh_plane* handle() { return _p; }   // for the svh_plane_* taps and timing

private:
    PlaneEstimation(const PlaneEstimation&);
    PlaneEstimation& operator=(const PlaneEstimation&);
    svh_plane* _p;
};

#endif  // PLANEESTIMATION_H

/*
 * viso_mono.h -- source-compatible stand-in for libviso2/src/viso_mono.h.
 *
 * class VisualOdometryMono : public VisualOdometry with the reference's nested
 * `parameters` (:30-45: height, pitch, ransac_iters, inlier_threshold, motion_threshold on
 * top of VisualOdometry::parameters), constructor and
 *     bool process(uint8_t* I, int32_t* dims, bool replace = false)
 * so a caller written against the reference (e.g. matlab/visualOdometryMonoMex.cpp:61-120)
 * compiles unchanged and runs on the MI355X: feature matching (svh_matcher_*) and the motion
 * estimate of viso_mono.cpp:40-159 (RANSAC over 8-point fundamental matrices, chirality,
 * ground-plane scale) execute on the device; libc rand() is consumed exactly like the
 * reference does (srand(0) in the constructor, viso.cpp:36).
 */
#ifndef VISO_MONO_H
#define VISO_MONO_H

#include "viso.h"

class VisualOdometryMono : public VisualOdometry {
public:
    struct parameters : public VisualOdometry::parameters {
        double  height;            // camera height above ground (meters)
        double  pitch;             // camera pitch (rad, negative = pointing down)
        int32_t ransac_iters;      // number of RANSAC iterations
        double  inlier_threshold;  // fundamental matrix inlier threshold
        double  motion_threshold;  // directly return false on small motions
        parameters() {
            height = 1.0;
            pitch = 0.0;
            ransac_iters = 2000;
            inlier_threshold = 0.00001;
            motion_threshold = 100.0;
        }
    };

    VisualOdometryMono(parameters param) : VisualOdometry(create(param)), _param(param) {}
    virtual ~VisualOdometryMono() {}

    bool process(uint8_t* I, int32_t* dims, bool replace = false) {
        return svh_vo_mono_process(_vo, I, dims, replace ? 1 : 0) == 1;
    }
    using VisualOdometry::process;
    // ---- extension (not in the reference): the image is in DEVICE memory (svh_vo_mono_process_device) ----
    bool processDevice(const uint8_t* dI, int32_t* dims, bool replace = false) { return svh_vo_mono_process_device(_vo, dI, dims, replace ? 1 : 0) == 1; }

    // ---- extension (not in the reference) ----
    // bucketing / RANSAC samples from a private generator with glibc's srand(seed) sequence instead of the
    // process-wide rand() (seed 0 = what the reference's constructor seeds)
    void usePrivateRand(uint32_t seed = 0) { svh_vo_set_private_rand(_vo, 1, seed); }

private:
    static svh_vo* create(const parameters& p) {
        svh_vo_mono_params q;
        svh_vo_mono_params_default(&q);
        q.match.nms_n = p.match.nms_n;
        q.match.nms_tau = p.match.nms_tau;
        q.match.match_binsize = p.match.match_binsize;
        q.match.match_radius = p.match.match_radius;
        q.match.match_disp_tolerance = p.match.match_disp_tolerance;
        q.match.outlier_disp_tolerance = p.match.outlier_disp_tolerance;
        q.match.outlier_flow_tolerance = p.match.outlier_flow_tolerance;
        q.match.multi_stage = p.match.multi_stage;
        q.match.half_resolution = p.match.half_resolution;
        q.match.refinement = p.match.refinement;
        q.match.f = p.match.f; q.match.cu = p.match.cu; q.match.cv = p.match.cv; q.match.base = p.match.base;
        q.bucket_max_features = p.bucket.max_features;
        q.bucket_width = p.bucket.bucket_width;
        q.bucket_height = p.bucket.bucket_height;
        q.f = p.calib.f; q.cu = p.calib.cu; q.cv = p.calib.cv;
        q.height = p.height;
        q.pitch = p.pitch;
        q.ransac_iters = p.ransac_iters;
        q.inlier_threshold = p.inlier_threshold;
        q.motion_threshold = p.motion_threshold;
        return svh_vo_mono_create(&q);
    }
    parameters _param;
};

#endif  // VISO_MONO_H

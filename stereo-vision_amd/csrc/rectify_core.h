// The numeric core of the rectification in front of Elas::process and VisualOdometryStereo::process
// (stereomapper/framecapturethread.cpp:100-131, 328-349: cv::initUndistortRectifyMap once per camera, cv::remap with
// INTER_LINEAR per frame).  OpenCV is not part of this project, so the arithmetic is written out here as OpenCV's
// documentation publishes it (the pinhole model with the distortion k1 k2 p1 p2 k3) and in the form its 8-bit bilinear
// remap uses (1/32-pixel fractions, integer weights that sum to 1024).  THE CONTRACT IS THIS ARITHMETIC; equality with an
// OpenCV build is not verified anywhere in this project.  Compiled from this one header by
//   * hipcc into the kernels of csrc/rectify_kernels.hip (k_rect_maps in fp64, k_rect_remap in integers),
//   * the host compiler into csrc/rectify_engine.cpp (create's inverse, the maps of an object without a device),
//   * g++ -ffp-contract=off into tests/rectify/rectify_core_check.cpp, which pins it against the numpy restatement
//     tests/rectify_ref.py on the CPU.
// Nothing may be contracted into an FMA (-ffp-contract=off on every build): every double operation below rounds once.
#pragma once
#include "mono_core.h"   // MC_FN

namespace svh {
namespace rect {

enum { WRAP = 0, ZERO = 1 };              // SVH_RECTIFY_WRAP / SVH_RECTIFY_ZERO
constexpr int32_t NO_SAMPLE = INT32_MIN;  // fixed-point coordinate of a map entry that yields 0

// one camera as the map formula reads it
struct Cam {
    double fx, fy, cx, cy;       // K[0], K[4], K[2], K[5]
    double k1, k2, p1, p2, k3;   // D
    double ir[9];                // (P[:3,:3] R)^-1, row major
};

// A = P[:3,:3] * R; every entry is ((P[r][0] R[0][c] + P[r][1] R[1][c]) + P[r][2] R[2][c]).  P is 3x4 row major.
MC_FN void mul_p_r(const double* P, const double* R, double* A) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            A[3 * r + c] = (P[4 * r + 0] * R[c] + P[4 * r + 1] * R[3 + c]) + P[4 * r + 2] * R[6 + c];
}

// ir = A^-1 as the adjugate over the determinant.  Order of operations: every cofactor is one difference of two
// products, written out below; det = (A[0] c0 + A[1] c1) + A[2] c2 with the first row's cofactors; every entry of the
// adjugate is DIVIDED by det (no reciprocal).  Returns false when det is 0 or not finite.
MC_FN bool invert3(const double* A, double* ir) {
    const double c0 = A[4] * A[8] - A[5] * A[7];
    const double c1 = A[5] * A[6] - A[3] * A[8];
    const double c2 = A[3] * A[7] - A[4] * A[6];
    const double det = (A[0] * c0 + A[1] * c1) + A[2] * c2;
    if (det == 0.0 || !(fabs(det) <= 1.7976931348623157e308)) return false;
    ir[0] = c0 / det;
    ir[1] = (A[2] * A[7] - A[1] * A[8]) / det;
    ir[2] = (A[1] * A[5] - A[2] * A[4]) / det;
    ir[3] = c1 / det;
    ir[4] = (A[0] * A[8] - A[2] * A[6]) / det;
    ir[5] = (A[2] * A[3] - A[0] * A[5]) / det;
    ir[6] = c2 / det;
    ir[7] = (A[1] * A[6] - A[0] * A[7]) / det;
    ir[8] = (A[0] * A[4] - A[1] * A[3]) / det;
    return true;
}

MC_FN bool make_cam(const double* K, const double* D, const double* R, const double* P, Cam* c) {
    double A[9];
    mul_p_r(P, R, A);
    c->fx = K[0], c->fy = K[4], c->cx = K[2], c->cy = K[5];
    c->k1 = D[0], c->k2 = D[1], c->p1 = D[2], c->p2 = D[3], c->k3 = D[4];
    return invert3(A, c->ir);
}

// The map entry of output pixel (row i, column j): where in the source it samples.  The direct form -- OpenCV walks a
// row with running sums -- so that every pixel is independent; left to right, one rounding per operation.
MC_FN void map_entry(const Cam& c, int32_t i, int32_t j, float* mx, float* my) {
    const double dj = (double)j, di = (double)i;
    const double X = (dj * c.ir[0] + di * c.ir[1]) + c.ir[2];
    const double Y = (dj * c.ir[3] + di * c.ir[4]) + c.ir[5];
    const double W = (dj * c.ir[6] + di * c.ir[7]) + c.ir[8];
    const double w = 1.0 / W;
    const double x = X * w, y = Y * w;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2;
    const double xy2 = (2.0 * x) * y;
    const double kr = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double u = c.fx * ((x * kr + c.p1 * xy2) + c.p2 * (r2 + 2.0 * x2)) + c.cx;
    const double v = c.fy * ((y * kr + c.p1 * (r2 + 2.0 * y2)) + c.p2 * xy2) + c.cy;
    *mx = (float)u;
    *my = (float)v;
}

MC_FN int32_t floor_mod(int32_t a, int32_t m) {
    const int32_t r = a % m;
    return r < 0 ? r + m : r;
}

// The resident fixed-point form of a map entry: sx = rint(mx * 32), sy = rint(my * 32) (float products, ties to even),
// so that x0 = sx >> 5 is the left tap and a = sx & 31 the fraction in 1/32 pixel.  An entry that is not finite or has
// |m| >= 2^20 becomes (NO_SAMPLE, NO_SAMPLE), whose taps lie outside every image.  For WRAP the tap is reduced here,
// once: sx becomes (floor_mod(x0, sw) << 5) | a, so the per-frame kernel wraps the second tap with one compare.
MC_FN void fixed_entry(float mx, float my, int32_t sw, int32_t sh, int32_t border, int32_t* sx, int32_t* sy) {
    const float lim = 1048576.0f;
    if (!(fabsf(mx) < lim) || !(fabsf(my) < lim)) {   // (a NaN fails both comparisons)
        *sx = *sy = NO_SAMPLE;
        return;
    }
    int32_t x = (int32_t)rintf(mx * 32.0f), y = (int32_t)rintf(my * 32.0f);
    if (border == WRAP) {
        x = (floor_mod(x >> 5, sw) << 5) | (x & 31);
        y = (floor_mod(y >> 5, sh) << 5) | (y & 31);
    }
    *sx = x;
    *sy = y;
}

// One output byte from the fixed-point entry.  A tap outside the image is 0: under ZERO that is the border rule, under
// WRAP it happens only for NO_SAMPLE, the first tap being reduced already and the second wrapped here.
MC_FN uint8_t sample_fixed(const uint8_t* S, int32_t sw, int32_t sh, size_t row_stride, int32_t border, int32_t sx,
                           int32_t sy) {
    const int32_t x0 = sx >> 5, y0 = sy >> 5, a = sx & 31, b = sy & 31;
    int32_t x1 = x0 + 1, y1 = y0 + 1;
    if (border == WRAP) {
        x1 = x1 == sw ? 0 : x1;
        y1 = y1 == sh ? 0 : y1;
    }
    const bool vx0 = (uint32_t)x0 < (uint32_t)sw, vx1 = (uint32_t)x1 < (uint32_t)sw;
    const bool vy0 = (uint32_t)y0 < (uint32_t)sh, vy1 = (uint32_t)y1 < (uint32_t)sh;
    const uint8_t* r0 = S + (size_t)(vy0 ? y0 : 0) * row_stride;
    const uint8_t* r1 = S + (size_t)(vy1 ? y1 : 0) * row_stride;
    const int32_t p00 = vy0 && vx0 ? r0[x0] : 0;
    const int32_t p01 = vy0 && vx1 ? r0[x1] : 0;
    const int32_t p10 = vy1 && vx0 ? r1[x0] : 0;
    const int32_t p11 = vy1 && vx1 ? r1[x1] : 0;
    return (uint8_t)(((32 - a) * (32 - b) * p00 + a * (32 - b) * p01 + (32 - a) * b * p10 + a * b * p11 + 512) >> 10);
}

// the two together: what cv::remap(..., INTER_LINEAR) computes for one pixel in this project's arithmetic
MC_FN uint8_t sample(const uint8_t* S, int32_t sw, int32_t sh, size_t row_stride, int32_t border, float mx, float my) {
    int32_t sx, sy;
    fixed_entry(mx, my, sw, sh, border, &sx, &sy);
    return sample_fixed(S, sw, sh, row_stride, border, sx, sy);
}

}  // namespace rect
}  // namespace svh

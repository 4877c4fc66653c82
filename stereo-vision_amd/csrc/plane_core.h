// The numeric core of PlaneEstimation (stereomapper/planeestimation.cpp), restated in the reference's operation order
// and number formats: the lattice of sparseDisparityGrid (:130-152), the two distance tests and the draw loop of
// drawRandomPlaneSample (:156-218), the sums and the solve of leastSquarePlane (:222-256), the vote (:53-62) and
// planeDsiTo3d (:84-126).  Compiled from this one header by
//   * hipcc into the kernels of csrc/plane_kernels.hip (lattice compaction, three-point fits, vote, winner),
//   * the host compiler into csrc/plane_engine.cpp (the draw walk, the final refit in list order, planeDsiTo3d),
//   * g++ -ffp-contract=off into tests/plane/plane_core_check.cpp, which pins it against the reference on the CPU.
// Nothing may be contracted into an FMA (-ffp-contract=off on every build): the float products of the sums and the
// double expression of the vote round after every operation, as the reference's SSE code does.
#pragma once
#include "recon_core.h"   // recon::solve3: Matrix::solve for a 3x3 system (the same Gauss-Jordan, eps 1e-20)

namespace svh {
namespace plane {

// the reference's constants (planeestimation.cpp:32-34, 40, 163, 183, 200) as parameters
struct Params {
    int32_t num_samples;   // 5000
    int32_t step_size;     // 5: lattice step in u and v
    int32_t max_draws;     // 1000: draws one hypothesis may consume
    int32_t roi[4];        // u0, v0, u1, v1 (inclusive), already resolved against the image
    float min_dist;        // 50: second point from the first, third point from the line through both
    double d_threshold;    // 5 (FLOAT in the reference): |a u + b v + c - d| < d_threshold
};

// sparseDisparityGrid: the lattice is u = u0, u0 + s, ... <= u1 (outer) by v = v0, ... <= v1 (inner); cell t of the
// u-major order is column t / nv, row t % nv.  An empty range has 0 cells.
struct Lattice {
    int32_t u0, v0, nu, nv, step_size;
};
MC_FN Lattice lattice_of(const Params& p, int32_t width, int32_t height) {
    Lattice L;
    L.u0 = p.roi[0] > 0 ? p.roi[0] : 0;
    L.v0 = p.roi[1] > 0 ? p.roi[1] : 0;
    const int32_t u1 = p.roi[2] < width - 1 ? p.roi[2] : width - 1;
    const int32_t v1 = p.roi[3] < height - 1 ? p.roi[3] : height - 1;
    L.step_size = p.step_size;
    L.nu = u1 >= L.u0 ? (u1 - L.u0) / p.step_size + 1 : 0;
    L.nv = v1 >= L.v0 ? (v1 - L.v0) / p.step_size + 1 : 0;
    return L;
}
MC_FN int32_t cell_u(const Lattice& L, int32_t t) { return L.u0 + (t / L.nv) * L.step_size; }
MC_FN int32_t cell_v(const Lattice& L, int32_t t) { return L.v0 + (t % L.nv) * L.step_size; }
MC_FN bool cell_kept(float d) { return d >= 1; }

// drawRandomPlaneSample's tests (:181-203), all in float
MC_FN bool second_far_enough(float u0, float v0, float uc, float vc, float min_dist) {
    const float diff_u = uc - u0, diff_v = vc - v0;
    return sqrtf(diff_u * diff_u + diff_v * diff_v) > min_dist;
}
MC_FN bool third_far_enough(float u0, float v0, float u1, float v1, float uc, float vc, float min_dist) {
    const float vu = u1 - u0, vv = v1 - v0;
    const float norm = sqrtf(vu * vu + vv * vv);
    const float nu = +vv / norm, nv = -vu / norm;
    const float ru = uc - u0, rv = vc - v0;
    return fabsf(nu * ru + nv * rv) > min_dist;
}

// One hypothesis' draws: `next()` yields rand(); lu / lv are the list's coordinates, n > 0 its length.  ind receives
// up to three list indices; returns how many (0 only when max_draws < 1), *consumed the draws taken.
template <typename Next>
inline int draw_sample(Next&& next, const float* lu, const float* lv, int32_t n, int32_t max_draws, float min_dist,
                       int32_t* ind, int32_t* consumed) {
    int have = 0;
    int32_t k = 0;
    while (have < 3 && k < max_draws) {
        const int32_t c = (int32_t)(next() % n);
        if (have == 0) {
            ind[have++] = c;
        } else if (have == 1) {
            if (second_far_enough(lu[ind[0]], lv[ind[0]], lu[c], lv[c], min_dist)) ind[have++] = c;
        } else {
            if (third_far_enough(lu[ind[0]], lv[ind[0]], lu[ind[1]], lv[ind[1]], lu[c], lv[c], min_dist)) ind[have++] = c;
        }
        k++;
    }
    *consumed = k;
    return have;
}

// leastSquarePlane's sums: float products added to doubles, in index order
struct Sums {
    double a00, a01, a02, a11, a12, a22, b0, b1, b2;
};
MC_FN void sums_zero(Sums& s) { s.a00 = s.a01 = s.a02 = s.a11 = s.a12 = s.a22 = s.b0 = s.b1 = s.b2 = 0.0; }
MC_FN void sums_add(Sums& s, float u, float v, float d) {
    const float uu = u * u, uv = u * v, vv = v * v, ud = u * d, vd = v * d;
    s.a00 += uu;
    s.a01 += uv;
    s.a02 += u;
    s.a11 += vv;
    s.a12 += v;
    s.a22 += 1;
    s.b0 += ud;
    s.b1 += vd;
    s.b2 += d;
}
// _b.solve(_A); a failed solve gives the zero plane (:248-255)
MC_FN bool sums_solve(const Sums& s, double* abc) {
    double A[9] = {s.a00, s.a01, s.a02, s.a01, s.a11, s.a12, s.a02, s.a12, s.a22};
    double B[3] = {s.b0, s.b1, s.b2};
    if (recon::solve3(A, B)) {
        abc[0] = B[0];
        abc[1] = B[1];
        abc[2] = B[2];
        return true;
    }
    abc[0] = abc[1] = abc[2] = 0.0;
    return false;
}
// the plane through the listed points ind[0 .. cnt-1]; cnt == 0: the zero plane (:210-214)
MC_FN void fit_indexed(const float* lu, const float* lv, const float* ld, const int32_t* ind, int32_t cnt,
                       double* abc) {
    if (cnt <= 0) {
        abc[0] = abc[1] = abc[2] = 0.0;
        return;
    }
    Sums s;
    sums_zero(s);
    for (int32_t i = 0; i < cnt; i++) sums_add(s, lu[ind[i]], lv[ind[i]], ld[ind[i]]);
    sums_solve(s, abc);
}

// the vote (:55-58): a double expression, evaluated left to right, rounded to float
MC_FN bool is_inlier(double a, double b, double c, float u, float v, float d, double thr) {
    const double au = a * (double)u;
    const double bv = b * (double)v;
    const float result = (float)(((au + bv) + c) - (double)d);
    return (double)fabsf(result) < thr;
}

// planeDsiTo3d (:84-126).  e: _plane_e; H: _H row major; returns true on the road branch, where *pitch is set (it
// keeps its value otherwise).  The reference tests _plane_d._val[0][1], which is b (the rows of a Matrix are one block).
inline bool plane_to_3d(const double* abc, float f, float cu, float cv, float base, double* e, double* H, float* pitch) {
    const double a = abc[0], b = abc[1], c = abc[2];
    e[0] = a / base;
    e[1] = b / base;
    e[2] = (a * cu + b * cv + c) / (f * base);   // (f * base is a float product)
    for (int i = 0; i < 16; i++) H[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!(fabs(b) > 0.1)) return false;
    double norm = 0.0;
    for (int i = 0; i < 3; i++) norm += e[i] * e[i];
    norm = sqrt(norm);
    if (fabs(norm) < 1e-20) return false;   // (the reference's operator/ ends the process here)
    double r2[3], r1[3], r3[3];
    for (int i = 0; i < 3; i++) r2[i] = e[i] / norm;
    r1[0] = +sqrt(r2[1] * r2[1] / (r2[0] * r2[0] + r2[1] * r2[1]));
    r1[1] = -r1[0] * r2[0] / r2[1];
    r1[2] = 0;
    r3[0] = r1[1] * r2[2] - r1[2] * r2[1];
    r3[1] = r1[2] * r2[0] - r1[0] * r2[2];
    r3[2] = r1[0] * r2[1] - r1[1] * r2[0];
    *pitch = (float)atan2(r3[1], r3[2]);
    for (int i = 0; i < 3; i++) {
        H[4 * i + 0] = r1[i];
        H[4 * i + 1] = r2[i];
        H[4 * i + 2] = r3[i];
    }
    return true;
}

}  // namespace plane
}  // namespace svh

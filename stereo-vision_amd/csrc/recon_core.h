// The numeric core of Reconstruction (libviso2/src/reconstruction.cpp:153-349), restated for fp64 in the reference's
// operation order: what happens to ONE lost track -- initPoint, pointType, refinePoint / updatePoint /
// computePredictionsAndJacobian, pointDistance, rayAngle -- and the outcome code of the chain of tests in update()
// (:131-141).  Compiled from this one header by
//   * hipcc into k_recon_tracks of csrc/recon_kernels.hip (one lane per lost track, the 4x4 SVD state of a lane
//     in LDS, the Gauss-Newton sums in registers),
//   * g++ -ffp-contract=off into tests/recon/recon_core_check.cpp, which pins it against the reference on the CPU.
// As in mono_core.h every dot product runs serially in ascending index order from 0.0 (Matrix::operator*,
// matrix.cpp:396-420) and nothing is contracted into an FMA.  The point is three FLOATS (point3d,
// reconstruction.h:46-50): it is rounded to float when it is initialised and after every Gauss-Newton step.
// Nothing is sized by a track length: the frame loop reads the projection matrices and the pixels from memory.
#pragma once
#include "mono_core.h"

namespace svh {
namespace recon {

using mono::Mat;
using mono::Vec;

// outcome of a lost track, in the order update() tests them (reconstruction.cpp:131-141)
enum Outcome {
    TOO_SHORT = 0,       // pixels.size() < min_track_length
    INIT_FAILED = 1,     // initPoint: the point is at infinity (|w| < 1e-10)
    TYPE_BELOW = 2,      // pointType(...) < point_type (not visible: -1)
    REFINE_FAILED = 3,   // refinePoint: singular projection / system, or no convergence after 22 updates
    TOO_FAR = 4,         // pointDistance >= max_dist
    ANGLE_SMALL = 5,     // !(rayAngle > min_angle)   (a NaN angle lands here, as in the reference)
    ACCEPTED = 6
};

// per-frame record of the pose chain: P_total (3x4), Tr_total (4x4), Tr_inv_total (4x4), row major
constexpr int FRAME_P = 0, FRAME_TR = 12, FRAME_TRI = 28, FRAME_STRIDE = 44;

// B.solve(A) for a 3x3 A and a 3x1 B (Matrix::solve, matrix.cpp:648-737): Gauss-Jordan with full pivoting, the
// pivot search with >=, eps = 1e-20 on the pivot, rows swapped physically.  A is destroyed.
MC_FN bool solve3(double* A, double* B) {
    int ipiv[3] = {0, 0, 0};
    int icol = 0, irow = 0;
    for (int i = 0; i < 3; i++) {
        double big = 0.0;
        for (int j = 0; j < 3; j++)
            if (ipiv[j] != 1)
                for (int k = 0; k < 3; k++)
                    if (ipiv[k] == 0 && fabs(A[3 * j + k]) >= big) {
                        big = fabs(A[3 * j + k]);
                        irow = j;
                        icol = k;
                    }
        ++ipiv[icol];
        if (irow != icol) {
            for (int l = 0; l < 3; l++) {
                const double t = A[3 * irow + l];
                A[3 * irow + l] = A[3 * icol + l];
                A[3 * icol + l] = t;
            }
            const double t = B[irow];
            B[irow] = B[icol];
            B[icol] = t;
        }
        if (fabs(A[3 * icol + icol]) < 1e-20) return false;
        const double pivinv = 1.0 / A[3 * icol + icol];
        A[3 * icol + icol] = 1.0;
        for (int l = 0; l < 3; l++) A[3 * icol + l] *= pivinv;
        B[icol] *= pivinv;
        for (int ll = 0; ll < 3; ll++)
            if (ll != icol) {
                const double dum = A[3 * ll + icol];
                A[3 * ll + icol] = 0.0;
                for (int l = 0; l < 3; l++) A[3 * ll + l] -= A[3 * icol + l] * dum;
                B[ll] -= B[icol] * dum;
            }
    }
    return true;
}

// initPoint (:153-182): orthogonal regression through the first and the last observation.  J, V (16 each) and
// w, rv1 (4 each) are the lane's SVD scratch.
MC_FN bool init_point(const double* P1, const double* P2, float u1, float v1, float u2, float v2, const Mat& J,
                      const Mat& V, const Vec& w, const Vec& rv1, float* p) {
    for (int j = 0; j < 4; j++) {
        J(0, j) = P1[8 + j] * u1 - P1[0 + j];
        J(1, j) = P1[8 + j] * v1 - P1[4 + j];
        J(2, j) = P2[8 + j] * u2 - P2[0 + j];
        J(3, j) = P2[8 + j] * v2 - P2[4 + j];
    }
    mono::svd(4, 4, J, V, w, rv1);
    const float wf = (float)V(3, 3);   // "float w = V.val[3][3]"
    if (fabs((double)wf) < 1e-10) return false;
    p[0] = (float)(V(0, 3) / wf);
    p[1] = (float)(V(1, 3) / wf);
    p[2] = (float)(V(2, 3) / wf);
    return true;
}

// row r of a 4x4 matrix times (p, 1), Matrix::operator* order
MC_FN double row_dot(const double* T, int r, const double* x) {
    double s = 0.0;
    for (int k = 0; k < 4; k++) s += T[4 * r + k] * x[k];
    return s;
}

// pointType (:235-261).  Ti1, Ti2: Tr_inv_total of the first and the last frame; cp, sp: cos and sin of the camera
// pitch of Tr_cam_road (:43-53, taken on the host), its height is 1.6
MC_FN int point_type(const double* Ti1, const double* Ti2, double cp, double sp, const float* p) {
    const double x[4] = {(double)p[0], (double)p[1], (double)p[2], 1.0};
    const double z1 = row_dot(Ti1, 2, x);
    double x2c[4];
    for (int r = 0; r < 4; r++) x2c[r] = row_dot(Ti2, r, x);
    const double road[4] = {0.0, cp, -sp, -1.6};   // row 1 of Tr_cam_road
    double y = 0.0;
    for (int k = 0; k < 4; k++) y += road[k] * x2c[k];
    if (z1 <= 1 || x2c[2] <= 1) return -1;
    if (y > 0.5) return 0;
    if (y > -1) return 1;
    return 2;
}

// updatePoint (:263-307) with computePredictionsAndJacobian (:316-349): one Gauss-Newton step over the nf frames
// of the track.  P: the 3x4 matrix of the first frame, `stride` doubles from one frame to the next; px: nf pixel
// pairs (u, v).  The sums of A and B run over i < 2 nf in ascending order, as the reference's loops do for each
// entry; A is symmetric term by term (a product commutes), so six sums are formed.  0 UPDATED, 1 FAILED, 2 CONVERGED
MC_FN int update_point(const double* P, int stride, const float* px, int nf, float* p) {
    const double X = p[0], Y = p[1], Z = p[2];
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0;
    for (int k = 0; k < nf; k++) {
        const double* Pk = P + (size_t)k * stride;
        const double a = Pk[0] * X + Pk[1] * Y + Pk[2] * Z + Pk[3];
        const double b = Pk[4] * X + Pk[5] * Y + Pk[6] * Z + Pk[7];
        const double c = Pk[8] * X + Pk[9] * Y + Pk[10] * Z + Pk[11];
        const double cc = c * c;
        if (cc < 1e-10) return 1;
        const double j0 = (Pk[0] * c - Pk[8] * a) / cc;
        const double j1 = (Pk[1] * c - Pk[9] * a) / cc;
        const double j2 = (Pk[2] * c - Pk[10] * a) / cc;
        const double j3 = (Pk[4] * c - Pk[8] * b) / cc;
        const double j4 = (Pk[5] * c - Pk[9] * b) / cc;
        const double j5 = (Pk[6] * c - Pk[10] * b) / cc;
        const double ru = (double)px[2 * k + 0] - a / c;
        const double rv = (double)px[2 * k + 1] - b / c;
        a00 += j0 * j0; a00 += j3 * j3;
        a01 += j0 * j1; a01 += j3 * j4;
        a02 += j0 * j2; a02 += j3 * j5;
        a11 += j1 * j1; a11 += j4 * j4;
        a12 += j1 * j2; a12 += j4 * j5;
        a22 += j2 * j2; a22 += j5 * j5;
        b0 += j0 * ru; b0 += j3 * rv;
        b1 += j1 * ru; b1 += j4 * rv;
        b2 += j2 * ru; b2 += j5 * rv;
    }
    double A[9] = {a00, a01, a02, a01, a11, a12, a02, a12, a22};
    double B[3] = {b0, b1, b2};
    if (!solve3(A, B)) return 1;
    p[0] = (float)(p[0] + 1.0 * B[0]);   // point3d holds floats: rounded after every step
    p[1] = (float)(p[1] + 1.0 * B[1]);
    p[2] = (float)(p[2] + 1.0 * B[2]);
    return fabs(B[0]) < 1e-5 && fabs(B[1]) < 1e-5 && fabs(B[2]) < 1e-5 ? 2 : 0;
}

// refinePoint (:184-207): at most 22 updates ("iter++ > 20" is tested after the update)
MC_FN bool refine_point(const double* P, int stride, const float* px, int nf, float* p) {
    int iter = 0, result = 0;
    while (result == 0) {
        result = update_point(P, stride, px, nf, p);
        if (iter++ > 20 || result == 2) break;
    }
    return result == 2;
}

// pointDistance (:209-215); Tm: Tr_total of the middle frame
MC_FN double point_distance(const double* Tm, const float* p) {
    const double dx = Tm[3] - p[0], dy = Tm[7] - p[1], dz = Tm[11] - p[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// rayAngle (:217-233); T1, T2: Tr_total of the first and the last frame.  acos may see an argument above 1 and give
// NaN; the caller's "> min_angle" is then false, as in the reference.
MC_FN double ray_angle(const double* T1, const double* T2, const float* p) {
    double v1[3], v2[3], s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < 3; i++) {
        v1[i] = T1[4 * i + 3] - (double)p[i];
        v2[i] = T2[4 * i + 3] - (double)p[i];
    }
    for (int i = 0; i < 3; i++) s1 += v1[i] * v1[i];
    for (int i = 0; i < 3; i++) s2 += v2[i] * v2[i];
    const double n1 = sqrt(s1), n2 = sqrt(s2);
    if (n1 < 1e-10 || n2 < 1e-10) return 1000;
    double d = 0.0;
    for (int i = 0; i < 3; i++) {
        v1[i] = v1[i] / n1;
        v2[i] = v2[i] / n2;
    }
    for (int i = 0; i < 3; i++) d += v1[i] * v2[i];
    return acos(fabs(d)) * 180.0 / M_PI;
}

struct Settings {
    int32_t point_type, min_track_length;
    double max_dist, min_angle;
    double cp, sp;   // cos / sin of Tr_cam_road's pitch
};

// One lost track through the tests of update() (:131-141).  frames: FRAME_STRIDE doubles per frame, the track covers
// frames first .. first + nf - 1; px: its nf pixel pairs.  p receives the point as far as it got (0 before initPoint
// succeeded).
MC_FN int track_outcome(const double* frames, int32_t first, const float* px, int32_t nf, const Settings& s,
                        const Mat& J, const Mat& V, const Vec& w, const Vec& rv1, float* p) {
    p[0] = p[1] = p[2] = 0.f;
    // "pixels.size() >= min_track_length": the int is converted to size_t, a negative one admits nothing
    if (!((uint64_t)nf >= (uint64_t)(int64_t)s.min_track_length)) return TOO_SHORT;
    const int32_t last = first + nf - 1;
    const double* F1 = frames + (size_t)first * FRAME_STRIDE;
    const double* F2 = frames + (size_t)last * FRAME_STRIDE;
    if (!init_point(F1 + FRAME_P, F2 + FRAME_P, px[0], px[1], px[2 * nf - 2], px[2 * nf - 1], J, V, w, rv1, p))
        return INIT_FAILED;
    if (!(point_type(F1 + FRAME_TRI, F2 + FRAME_TRI, s.cp, s.sp, p) >= s.point_type)) return TYPE_BELOW;
    if (!refine_point(F1 + FRAME_P, FRAME_STRIDE, px, nf, p)) return REFINE_FAILED;
    const double* Fm = frames + (size_t)((first + last) / 2) * FRAME_STRIDE;
    if (!(point_distance(Fm + FRAME_TR, p) < s.max_dist)) return TOO_FAR;
    if (!(ray_angle(F1 + FRAME_TR, F2 + FRAME_TR, p) > s.min_angle)) return ANGLE_SMALL;
    return ACCEPTED;
}

}  // namespace recon
}  // namespace svh

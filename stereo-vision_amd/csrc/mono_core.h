// The numeric core of VisualOdometryMono::estimateMotion (libviso2/src/viso_mono.cpp:40-400), restated for fp64 in
// the reference's operation order.  Compiled from this one header by
//   * hipcc into the kernels of csrc/vo_mono_kernels.hip (one lane per RANSAC hypothesis / per triangulated point,
//     the SVD state of a lane in LDS),
//   * hipcc's host pass into csrc/vo_mono_engine.cpp (normalisation, the k x 9 refit, E -> R|t),
//   * g++ -ffp-contract=off into tests/mono/mono_core_check.cpp, which pins it against the reference on the CPU.
// Every dot product runs serially in ascending index order, starting from 0.0 as Matrix::operator* does
// (matrix.cpp:396-420), and nothing is contracted into an FMA (the library is built with -ffp-contract=off), so the
// three builds and the reference round the same way.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MC_FN __host__ __device__ __forceinline__
#else
#define MC_FN inline
#endif

namespace svh {
namespace mono {

// A matrix of a lane: element (r, c) of an m x n matrix at p[(r * ld + c) * S].  S > 1 interleaves the matrices of
// S lanes (consecutive lanes -> consecutive 8-byte words of LDS: no bank conflicts); the host uses S = 1.
struct Mat {
    double* p;
    int ld, S;
    MC_FN double& operator()(int r, int c) const { return p[(r * ld + c) * S]; }
};
struct Vec {
    double* p;
    int S;
    MC_FN double& operator[](int i) const { return p[i * S]; }
};

MC_FN double sign_of(double a, double b) { return b >= 0.0 ? fabs(a) : -fabs(a); }
MC_FN double sqr(double a) { return a == 0.0 ? 0.0 : a * a; }

// Matrix::pythag (matrix.cpp:1213-1225)
MC_FN double pythag(double a, double b) {
    const double absa = fabs(a), absb = fabs(b);
    if (absa > absb) return absa * sqrt(1.0 + sqr(absb / absa));
    return absb == 0.0 ? 0.0 : absb * sqrt(1.0 + sqr(absa / absb));
}

// Matrix::svd (matrix.cpp:870-1153) on an m x n matrix held in U (overwritten with the m x n left factor, as the
// reference's working copy), V (n x n) and w (n singular values), rv1 (n) its work vector.  Householder
// bidiagonalisation, accumulation of both sides, implicit-shift QR with the (fabs(x)+anorm)==anorm splitting tests,
// then the shell sort by decreasing w and the sign flip that maximises positive entries.  The column moves of the
// sort are made as swaps of columns j and j-inc, which is the same permutation as the reference's insertion with a
// held column.  Shapes used: 8x9, k x 9 (k >= 10), 3x3, 4x4.
MC_FN void svd(int m, int n, const Mat& U, const Mat& V, const Vec& w, const Vec& rv1) {
    int flag, i, its, j, jj, k, l = 0, nm = 0;
    double anorm, c, f, g, h, s, scale, x, y, z;
    g = scale = anorm = 0.0;
    for (i = 0; i < n; i++) {
        l = i + 1;
        rv1[i] = scale * g;
        g = s = scale = 0.0;
        if (i < m) {
            for (k = i; k < m; k++) scale += fabs(U(k, i));
            if (scale) {
                for (k = i; k < m; k++) {
                    U(k, i) /= scale;
                    s += U(k, i) * U(k, i);
                }
                f = U(i, i);
                g = -sign_of(sqrt(s), f);
                h = f * g - s;
                U(i, i) = f - g;
                for (j = l; j < n; j++) {
                    for (s = 0.0, k = i; k < m; k++) s += U(k, i) * U(k, j);
                    f = s / h;
                    for (k = i; k < m; k++) U(k, j) += f * U(k, i);
                }
                for (k = i; k < m; k++) U(k, i) *= scale;
            }
        }
        w[i] = scale * g;
        g = s = scale = 0.0;
        if (i < m && i != n - 1) {
            for (k = l; k < n; k++) scale += fabs(U(i, k));
            if (scale) {
                for (k = l; k < n; k++) {
                    U(i, k) /= scale;
                    s += U(i, k) * U(i, k);
                }
                f = U(i, l);
                g = -sign_of(sqrt(s), f);
                h = f * g - s;
                U(i, l) = f - g;
                for (k = l; k < n; k++) rv1[k] = U(i, k) / h;
                for (j = l; j < m; j++) {
                    for (s = 0.0, k = l; k < n; k++) s += U(j, k) * U(i, k);
                    for (k = l; k < n; k++) U(j, k) += s * rv1[k];
                }
                for (k = l; k < n; k++) U(i, k) *= scale;
            }
        }
        const double a = fabs(w[i]) + fabs(rv1[i]);
        anorm = anorm > a ? anorm : a;
    }
    // accumulation of right-hand transformations
    for (i = n - 1; i >= 0; i--) {
        if (i < n - 1) {
            if (g) {
                for (j = l; j < n; j++) V(j, i) = (U(i, j) / U(i, l)) / g;
                for (j = l; j < n; j++) {
                    for (s = 0.0, k = l; k < n; k++) s += U(i, k) * V(k, j);
                    for (k = l; k < n; k++) V(k, j) += s * V(k, i);
                }
            }
            for (j = l; j < n; j++) V(i, j) = V(j, i) = 0.0;
        }
        V(i, i) = 1.0;
        g = rv1[i];
        l = i;
    }
    // accumulation of left-hand transformations
    for (i = (m < n ? m : n) - 1; i >= 0; i--) {
        l = i + 1;
        g = w[i];
        for (j = l; j < n; j++) U(i, j) = 0.0;
        if (g) {
            g = 1.0 / g;
            for (j = l; j < n; j++) {
                for (s = 0.0, k = l; k < m; k++) s += U(k, i) * U(k, j);
                f = (s / U(i, i)) * g;
                for (k = i; k < m; k++) U(k, j) += f * U(k, i);
            }
            for (j = i; j < m; j++) U(j, i) *= g;
        } else {
            for (j = i; j < m; j++) U(j, i) = 0.0;
        }
        ++U(i, i);
    }
    // diagonalisation of the bidiagonal form
    for (k = n - 1; k >= 0; k--) {
        for (its = 0; its < 30; its++) {
            flag = 1;
            for (l = k; l >= 0; l--) {
                nm = l - 1;
                if ((double)(fabs(rv1[l]) + anorm) == anorm) {
                    flag = 0;
                    break;
                }
                if ((double)(fabs(w[nm]) + anorm) == anorm) break;
            }
            if (flag) {
                c = 0.0;
                s = 1.0;
                for (i = l; i <= k; i++) {
                    f = s * rv1[i];
                    rv1[i] = c * rv1[i];
                    if ((double)(fabs(f) + anorm) == anorm) break;
                    g = w[i];
                    h = pythag(f, g);
                    w[i] = h;
                    h = 1.0 / h;
                    c = g * h;
                    s = -f * h;
                    for (j = 0; j < m; j++) {
                        y = U(j, nm);
                        z = U(j, i);
                        U(j, nm) = y * c + z * s;
                        U(j, i) = z * c - y * s;
                    }
                }
            }
            z = w[k];
            if (l == k) {
                if (z < 0.0) {
                    w[k] = -z;
                    for (j = 0; j < n; j++) V(j, k) = -V(j, k);
                }
                break;
            }
            x = w[l];
            nm = k - 1;
            y = w[nm];
            g = rv1[nm];
            h = rv1[k];
            f = ((y - z) * (y + z) + (g - h) * (g + h)) / (2.0 * h * y);
            g = pythag(f, 1.0);
            f = ((x - z) * (x + z) + h * ((y / (f + sign_of(g, f))) - h)) / x;
            c = s = 1.0;
            for (j = l; j <= nm; j++) {
                i = j + 1;
                g = rv1[i];
                y = w[i];
                h = s * g;
                g = c * g;
                z = pythag(f, h);
                rv1[j] = z;
                c = f / z;
                s = h / z;
                f = x * c + g * s;
                g = g * c - x * s;
                h = y * s;
                y *= c;
                for (jj = 0; jj < n; jj++) {
                    x = V(jj, j);
                    z = V(jj, i);
                    V(jj, j) = x * c + z * s;
                    V(jj, i) = z * c - x * s;
                }
                z = pythag(f, h);
                w[j] = z;
                if (z) {
                    z = 1.0 / z;
                    c = f * z;
                    s = h * z;
                }
                f = c * g + s * y;
                x = c * y - s * g;
                for (jj = 0; jj < m; jj++) {
                    y = U(jj, j);
                    z = U(jj, i);
                    U(jj, j) = y * c + z * s;
                    U(jj, i) = z * c - y * s;
                }
            }
            rv1[l] = 0.0;
            rv1[k] = f;
            w[k] = x;
        }
    }
    // sort by decreasing singular value (shell sort, gaps 1, 4, 13, ...)
    int inc = 1;
    do {
        inc *= 3;
        inc++;
    } while (inc <= n);
    do {
        inc /= 3;
        for (i = inc; i < n; i++) {
            for (j = i; j >= inc && w[j - inc] < w[j]; j -= inc) {
                double t = w[j];
                w[j] = w[j - inc];
                w[j - inc] = t;
                for (k = 0; k < m; k++) {
                    t = U(k, j);
                    U(k, j) = U(k, j - inc);
                    U(k, j - inc) = t;
                }
                for (k = 0; k < n; k++) {
                    t = V(k, j);
                    V(k, j) = V(k, j - inc);
                    V(k, j - inc) = t;
                }
            }
        }
    } while (inc > 1);
    // flip signs
    for (k = 0; k < n; k++) {
        int s2 = 0;
        for (i = 0; i < m; i++) s2 += U(i, k) < 0.0;
        for (j = 0; j < n; j++) s2 += V(j, k) < 0.0;
        if (s2 > (m + n) / 2) {
            for (i = 0; i < m; i++) U(i, k) = -U(i, k);
            for (j = 0; j < n; j++) V(j, k) = -V(j, k);
        }
    }
}

// C = A * B for 3x3 row-major matrices, Matrix::operator* order (C starts at 0, k ascending); tb: B transposed
MC_FN void mul3(const double* A, const double* B, double* C, bool tb) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += A[3 * i + k] * (tb ? B[3 * j + k] : B[3 * k + j]);
            C[3 * i + j] = s;
        }
}

// F = U * diag(w0, w1, 0) * V' for the 3x3 factors of an SVD (viso_mono.cpp:262-264, :81-84): U*diag(W) first
MC_FN void rank2(const Mat& U, const Mat& V, const Vec& w, double* F) {
    double UD[9], D[9], Vr[9];
    for (int i = 0; i < 9; i++) D[i] = 0.0;
    D[0] = w[0];
    D[4] = w[1];
    D[8] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += U(i, k) * D[3 * k + j];
            UD[3 * i + j] = s;
            Vr[3 * i + j] = V(i, j);
        }
    mul3(UD, Vr, F, true);
}

// one row of the constraint matrix A (viso_mono.cpp:243-253): the products are float, as p_match holds floats
MC_FN void f_row(float u1p, float v1p, float u1c, float v1c, double* a, int S) {
    a[0 * S] = (double)(float)(u1c * u1p);
    a[1 * S] = (double)(float)(u1c * v1p);
    a[2 * S] = (double)u1c;
    a[3 * S] = (double)(float)(v1c * u1p);
    a[4 * S] = (double)(float)(v1c * v1p);
    a[5 * S] = (double)v1c;
    a[6 * S] = (double)u1p;
    a[7 * S] = (double)v1p;
    a[8 * S] = 1.0;
}

// getInlier's Sampson test for one match (viso_mono.cpp:267-314)
MC_FN bool sampson_inlier(const double* F, double u1, double v1, double u2, double v2, double thr) {
    const double Fx1u = F[0] * u1 + F[1] * v1 + F[2];
    const double Fx1v = F[3] * u1 + F[4] * v1 + F[5];
    const double Fx1w = F[6] * u1 + F[7] * v1 + F[8];
    const double Ftx2u = F[0] * u2 + F[3] * v2 + F[6];
    const double Ftx2v = F[1] * u2 + F[4] * v2 + F[7];
    const double x2tFx1 = u2 * Fx1u + v2 * Fx1v + Fx1w;
    const double d = x2tFx1 * x2tFx1 / (Fx1u * Fx1u + Fx1v * Fx1v + Ftx2u * Ftx2u + Ftx2v * Ftx2v);
    return fabs(d) < thr;
}

// normalizeFeaturePoints (viso_mono.cpp:186-232) on n matches given as four float arrays of stride 4 (u1p, v1p,
// u1c, v1c).  The sums are double, every -= and *= stores into a float, and the distance of a point is the float
// sqrt of a float sum.  Returns false when a scale sum vanishes; T[0..8] = Tp, T[9..17] = Tc (row major).
MC_FN bool normalize(float* q, int n, double* T) {
    double cpu = 0, cpv = 0, ccu = 0, ccv = 0;
    for (int i = 0; i < n; i++) {
        cpu += q[4 * i + 0];
        cpv += q[4 * i + 1];
        ccu += q[4 * i + 2];
        ccv += q[4 * i + 3];
    }
    cpu /= (double)n;
    cpv /= (double)n;
    ccu /= (double)n;
    ccv /= (double)n;
    for (int i = 0; i < n; i++) {
        q[4 * i + 0] = (float)(q[4 * i + 0] - cpu);
        q[4 * i + 1] = (float)(q[4 * i + 1] - cpv);
        q[4 * i + 2] = (float)(q[4 * i + 2] - ccu);
        q[4 * i + 3] = (float)(q[4 * i + 3] - ccv);
    }
    double sp = 0, sc = 0;
    for (int i = 0; i < n; i++) {
        const float a = q[4 * i + 0], b = q[4 * i + 1], c = q[4 * i + 2], d = q[4 * i + 3];
        sp += sqrtf(a * a + b * b);
        sc += sqrtf(c * c + d * d);
    }
    if (fabs(sp) < 1e-10 || fabs(sc) < 1e-10) return false;
    sp = sqrt(2.0) * (double)n / sp;
    sc = sqrt(2.0) * (double)n / sc;
    for (int i = 0; i < n; i++) {
        q[4 * i + 0] = (float)(q[4 * i + 0] * sp);
        q[4 * i + 1] = (float)(q[4 * i + 1] * sp);
        q[4 * i + 2] = (float)(q[4 * i + 2] * sc);
        q[4 * i + 3] = (float)(q[4 * i + 3] * sc);
    }
    const double Tp[9] = {sp, 0, -sp * cpu, 0, sp, -sp * cpv, 0, 0, 1};
    const double Tc[9] = {sc, 0, -sc * ccu, 0, sc, -sc * ccv, 0, 0, 1};
    for (int i = 0; i < 9; i++) {
        T[i] = Tp[i];
        T[9 + i] = Tc[i];
    }
    return true;
}

// One point of triangulateChieral (viso_mono.cpp:363-400): the 4x4 orthogonal regression through the two
// projection matrices P1, P2 (3x4 row major), its last right singular vector into X[4], and whether the point lies
// in front of both cameras.  J, V (16 each) and w, rv1 (4 each) are the lane's scratch.
MC_FN bool triangulate(const double* P1, const double* P2, float u1p, float v1p, float u1c, float v1c,
                       const Mat& J, const Mat& V, const Vec& w, const Vec& rv1, double* X) {
    for (int j = 0; j < 4; j++) {
        J(0, j) = P1[8 + j] * u1p - P1[0 + j];
        J(1, j) = P1[8 + j] * v1p - P1[4 + j];
        J(2, j) = P2[8 + j] * u1c - P2[0 + j];
        J(3, j) = P2[8 + j] * v1c - P2[4 + j];
    }
    svd(4, 4, J, V, w, rv1);
    for (int r = 0; r < 4; r++) X[r] = V(r, 3);
    double a = 0.0, b = 0.0;
    for (int k = 0; k < 4; k++) a += P1[8 + k] * X[k];
    for (int k = 0; k < 4; k++) b += P2[8 + k] * X[k];
    return a * X[3] > 0 && b * X[3] > 0;
}

}  // namespace mono
}  // namespace svh

// The 3x3 plane fit of k_prior (csrc/elas_kernels.hip): Matrix::solve of the reference for one right-hand side
// (libelas/src/matrix.cpp:414-501 -- Gauss-Jordan with full pivoting, ">=" pivot search so that the LAST maximum
// wins, eps 1e-20), with every pivot position resolved into selects between named registers instead of run-time
// array indices (which the device compiler turns into v_cndmask chains over whole arrays, two per double).
// Compiled from this one header by
//   * hipcc into k_prior,
//   * g++ -ffp-contract=off into tests/prior/solve3_check.cpp, which compares it bit for bit with a plain
//     transcription of the generic form on random integer systems (ties and singular systems included).
// Nothing may be contracted into an FMA (-ffp-contract=off on every build); `/` on doubles is IEEE division.
//
// What is left out, and why the result cannot change.  The generic form inverts A in place: after a step with
// pivot column pc, column pc of every row holds a part of the inverse.  Those entries are never read again by
// anything that reaches B or the singularity test: later pivot searches skip used columns, the factor f of a later
// step is read from that step's (unused) pivot column, and A[r][l] -= A[pc][l] * f feeds column l only from
// column l.  So only the UNUSED columns of each row and B are carried, and every value that is carried goes
// through exactly the generic form's operations in the generic form's order:
//   inv = 1 / pivot;  row_pc[l] *= inv;  B_pc *= inv;  row_r[l] -= row_pc[l] * f;  B_r -= B_pc * f.
// Positions matter in two places only: the search order (rows, then columns, ascending -- ties) and the slot of B an
// unknown lands in.  After step 0 swapped rows pr and pc, the two remaining row positions and the two remaining
// columns are the same set {0,1,2} \ {pc}; taking them in ascending order ("lo", "hi") keeps the search order of
// step 1, and step 2 has one candidate.  (A NaN could send the generic form's search elsewhere; the entries are
// integers below 2^31, every normalised row is bounded by 1 in the pivot's column set, so none arises.)
#pragma once
#include <math.h>
#include "mono_core.h"   // MC_FN

namespace svh {
namespace prior {

// one of three values by position.  By VALUE on purpose: `i == 0 ? B[0] : B[1]` on array elements is an lvalue, i.e.
// a select between addresses in front of ONE load -- a run-time index after all (the device compiler answered it by
// moving the array to LDS)
MC_FN double pick3(int i, double a0, double a1, double a2) { return i == 0 ? a0 : i == 1 ? a1 : a2; }

// A row major, B: solved in place like the generic form (B = the solution when true is returned; A is left alone)
MC_FN bool solve3(const double A[3][3], double B[3]) {
    const double B0 = B[0], B1 = B[1], B2 = B[2];
    // ---- step 0: the last maximum of |A[j][k]|, rows then columns ascending
    double big = 0.0;
    int pr = 0, pc = 0;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) {
            const double a = fabs(A[j][k]);
            const bool ge = a >= big;
            big = ge ? a : big;
            pr = ge ? j : pr;
            pc = ge ? k : pc;
        }
    // columns of every row: the pivot column and the two others in ascending order
    double c[3], x[3], y[3];
    for (int j = 0; j < 3; j++) {
        const double a0 = A[j][0], a1 = A[j][1], a2 = A[j][2];
        c[j] = pick3(pc, a0, a1, a2);
        x[j] = pc == 0 ? a1 : a0;
        y[j] = pc == 2 ? a1 : a2;
    }
    // rows pr and pc change places: P = the pivot row (now at position pc), Q = what went to position pr
    const double c0 = c[0], c1_ = c[1], c2 = c[2], x0 = x[0], x1 = x[1], x2 = x[2], y0 = y[0], y1 = y[1], y2 = y[2];
    const double Pc = pick3(pr, c0, c1_, c2);
    double Px = pick3(pr, x0, x1, x2);
    double Py = pick3(pr, y0, y1, y2);
    double Pb = pick3(pr, B0, B1, B2);
    const double Qc = pick3(pc, c0, c1_, c2);
    const double Qx = pick3(pc, x0, x1, x2);
    const double Qy = pick3(pc, y0, y1, y2);
    const double Qb = pick3(pc, B0, B1, B2);
    // the rows at the two positions other than pc, ascending: position lo = (pc == 0 ? 1 : 0), hi = (pc == 2 ? 1 : 2)
    const int lo = pc == 0 ? 1 : 0, hi = pc == 2 ? 1 : 2;
    const bool lo_q = lo == pr, hi_q = hi == pr;     // that position received Q in the swap
    double m[2][2], f[2], b[2];
    f[0] = lo_q ? Qc : (pc == 0 ? c1_ : c0);
    m[0][0] = lo_q ? Qx : (pc == 0 ? x1 : x0);
    m[0][1] = lo_q ? Qy : (pc == 0 ? y1 : y0);
    b[0] = lo_q ? Qb : (pc == 0 ? B1 : B0);
    f[1] = hi_q ? Qc : (pc == 2 ? c1_ : c2);
    m[1][0] = hi_q ? Qx : (pc == 2 ? x1 : x2);
    m[1][1] = hi_q ? Qy : (pc == 2 ? y1 : y2);
    b[1] = hi_q ? Qb : (pc == 2 ? B1 : B2);
    bool ok = !(fabs(Pc) < 1e-20);
    {
        const double inv = 1.0 / Pc;
        Px = Px * inv;
        Py = Py * inv;
        Pb = Pb * inv;
        for (int r = 0; r < 2; r++) {
            m[r][0] = m[r][0] - Px * f[r];
            m[r][1] = m[r][1] - Py * f[r];
            b[r] = b[r] - Pb * f[r];
        }
    }
    // ---- step 1: the last maximum of the 2x2 rest, (lo,lo) (lo,hi) (hi,lo) (hi,hi)
    big = 0.0;
    int qr = 0, qc = 0;
    for (int j = 0; j < 2; j++)
        for (int k = 0; k < 2; k++) {
            const double a = fabs(m[j][k]);
            const bool ge = a >= big;
            big = ge ? a : big;
            qr = ge ? j : qr;
            qc = ge ? k : qc;
        }
    // rows qr and qc of the rest change places; R = the pivot row (at position qc), S = the other position.
    // Of each row: its entry in the pivot column (p) and in the last column (z).
    const bool r1 = qr == 1, c1 = qc == 1;
    const double m00 = m[0][0], m01 = m[0][1], m10 = m[1][0], m11 = m[1][1], b0 = b[0], b1 = b[1];
    const double Rp = r1 ? (c1 ? m11 : m10) : (c1 ? m01 : m00);
    double Rz = r1 ? (c1 ? m10 : m11) : (c1 ? m00 : m01);
    double Rb = r1 ? b1 : b0;
    // the other position holds the row that was not the pivot row (swapped or not: the rest has two rows)
    const double Sp = r1 ? (c1 ? m01 : m00) : (c1 ? m11 : m10);
    double Sz = r1 ? (c1 ? m00 : m01) : (c1 ? m10 : m11);
    double Sb = r1 ? b0 : b1;
    const double Pp = c1 ? Py : Px;     // row of step 0: its entries in this step's pivot column and in the last one
    double Pz = c1 ? Px : Py;
    ok = ok && !(fabs(Rp) < 1e-20);
    {
        const double inv = 1.0 / Rp;
        Rz = Rz * inv;
        Rb = Rb * inv;
        // (rows in ascending position; the three are independent of one another)
        Pz = Pz - Rz * Pp;
        Pb = Pb - Rb * Pp;
        Sz = Sz - Rz * Sp;
        Sb = Sb - Rb * Sp;
    }
    // ---- step 2: one candidate left, on the diagonal (|a| >= 0 holds): no swap
    ok = ok && !(fabs(Sz) < 1e-20);
    {
        const double inv = 1.0 / Sz;
        Sb = Sb * inv;
        Pb = Pb - Sb * Pz;
        Rb = Rb - Sb * Rz;
    }
    // unknowns back to their slots: P at pc; of the rest, R at position qc and S at the other one
    const double blo = c1 ? Sb : Rb, bhi = c1 ? Rb : Sb;
    B[0] = pc == 0 ? Pb : blo;
    B[1] = pc == 1 ? Pb : (pc == 0 ? blo : bhi);
    B[2] = pc == 2 ? Pb : bhi;
    return ok;
}

}  // namespace prior
}  // namespace svh

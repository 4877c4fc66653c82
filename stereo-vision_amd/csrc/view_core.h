// The numeric core of the map view (stereomapper/view3d.cpp:127-166 addCamera, :271-384 paintGL, :388-399 resizeGL,
// :403-463 playPoses) behind the svh_view_* entries of include/svh_view.h.  View3D is a QGLWidget and OpenGL leaves the
// rasterisation of points and lines partly to the implementation, so the arithmetic is written out here once.  THE
// CONTRACT IS THIS ARITHMETIC; equality with any OpenGL implementation is not verified anywhere in this project, and the
// widget's multisampling (QGL::SampleBuffers) is not reproduced.  Compiled from this one header by
//   * hipcc into the kernels of csrc/view_kernels.hip (everything per primitive, fp32),
//   * the host compiler into csrc/view_engine.cpp (the matrices, the camera outlines, the segment list, the poses of a
//     fly-through, all in double on the host),
//   * g++ -ffp-contract=off into tests/view/view_core_check.cpp, which pins it against the numpy restatement
//     tests/view_ref.py on the CPU.
// Nothing may be contracted into an FMA (-ffp-contract=off on every build): every operation below rounds once, in the
// order written.  No transcendental function is evaluated per primitive.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "mono_core.h"   // MC_FN

namespace svh {
namespace view {

constexpr uint64_t EMPTY_KEY = ~(uint64_t)0;   // a pixel of the depth layer nothing has been drawn to
constexpr uint32_t GRID_SEGS = 162;            // draw indices 0..161 belong to the grid, shown or not
constexpr uint32_t NO_ANCHOR = 0xFFFFFFFFu;
// colour codes of the overlay layer: bit 2 red, bit 1 green, bit 0 blue
enum { COL_BLUE = 1, COL_GREEN = 2, COL_RED = 4, COL_YELLOW = 6 };
enum { SEG_OVERLAY = 1, SEG_WIDE = 2 };

struct Pose {
    float zoom, rotx, roty, tx, ty, tz;
};

// what every primitive is drawn with: MVP = P * M rounded to float once, the image and glViewport's square
struct Frame {
    float m[16];   // row major
    int32_t W, H, side, ox, oy;
};

// One line segment in world coordinates.  value: the draw index of a depth-tested segment; of an overlay segment
// ((order + 1) << 3) | colour code, so that the later primitive is the larger number and 0 is "nothing".
struct Seg {
    float a[3], b[3];
    uint32_t value, flags;
};

struct Cam {
    float p[10][3];
    int32_t keyframe;
};

// ---------------------------------------------------------------------------------------------------- host, double
// C = A * B, 4x4 row major; every entry is ((a0 b0 + a1 b1) + a2 b2) + a3 b3
inline void mul4(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++)
            C[4 * r + c] = ((A[4 * r + 0] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

inline void translate4(double x, double y, double z, double* T) {
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    T[3] = x, T[7] = y, T[11] = z;
}

// paintGL's modelview M = T(0,0,zoom) Rx(rotx) Ry(roty) T(tx,ty,tz), multiplied left to right, resizeGL's
// P = gluPerspective(45, 1, 0.1, 10000), MVP = P M rounded to float; angles are deg * M_PI / 180.0.
inline void make_frame(const Pose& p, int32_t W, int32_t H, Frame* f) {
    const double ax = (double)p.rotx * M_PI / 180.0, ay = (double)p.roty * M_PI / 180.0;
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay);
    double Tz[16], Rx[16], Ry[16], Tt[16], A[16], B[16], M[16], P[16], MVP[16];
    translate4(0.0, 0.0, (double)p.zoom, Tz);
    translate4(0.0, 0.0, 0.0, Rx);
    Rx[5] = cx, Rx[6] = -sx, Rx[9] = sx, Rx[10] = cx;
    translate4(0.0, 0.0, 0.0, Ry);
    Ry[0] = cy, Ry[2] = sy, Ry[8] = -sy, Ry[10] = cy;
    translate4((double)p.tx, (double)p.ty, (double)p.tz, Tt);
    mul4(Tz, Rx, A);
    mul4(A, Ry, B);
    mul4(B, Tt, M);
    const double half = 45.0 / 2.0 * M_PI / 180.0;
    const double ct = cos(half) / sin(half), zn = 0.1, zf = 10000.0;
    for (int i = 0; i < 16; i++) P[i] = 0.0;
    P[0] = ct / 1.0;
    P[5] = ct;
    P[10] = -(zf + zn) / (zf - zn);
    P[11] = -2.0 * zn * zf / (zf - zn);
    P[14] = -1.0;
    mul4(P, M, MVP);
    for (int i = 0; i < 16; i++) f->m[i] = (float)MVP[i];
    f->W = W, f->H = H;
    f->side = W > H ? W : H;
    f->ox = (W - f->side) / 2;   // C division: towards zero
    f->oy = (H - f->side) / 2;
}

// addCamera (view3d.cpp:127-166): the ten points of the outline, H_total (4x4 row major) times (x, y, z, 1) in double,
// every row ((h0 x + h1 y) + h2 z) + h3, stored as float
inline void make_camera(const double* Ht, float s, int32_t keyframe, Cam* c) {
    const double h = 0.5 * (double)s, o = 1.0 * (double)s;
    const double C[10][3] = {{-h, -h, o}, {h, -h, o}, {h, h, o}, {-h, h, o}, {-h, -h, o},
                             {0, 0, 0},   {h, -h, o}, {h, h, o}, {0, 0, 0},  {-h, h, o}};
    for (int i = 0; i < 10; i++)
        for (int j = 0; j < 3; j++)
            c->p[i][j] = (float)(((Ht[4 * j + 0] * C[i][0] + Ht[4 * j + 1] * C[i][1]) + Ht[4 * j + 2] * C[i][2]) + Ht[4 * j + 3] * 1.0);
    c->keyframe = keyframe ? 1 : 0;
}

inline Seg make_seg(const float* a, const float* b, uint32_t value, uint32_t flags) {
    Seg s;
    for (int j = 0; j < 3; j++) s.a[j] = a[j], s.b[j] = b[j];
    s.value = value, s.flags = flags;
    return s;
}

// paintGL's line primitives in its order: the grid (depth-tested, draw indices 0..161), then -- depth test off, later
// over earlier -- every camera's strip, the track through the cameras' point 5 in the colour the last camera left
// behind, and the three axes, three pixels wide
inline void build_segments(const Cam* cams, size_t ncam, bool show_grid, bool show_cams, std::vector<Seg>* out) {
    out->clear();
    if (show_grid) {
        const float r = 200.f, h = 2.f;
        uint32_t k = 0;
        for (float x = -r; x <= r + 0.001; x += 5) {
            const float a0[3] = {x, h, -r}, b0[3] = {x, h, +r}, a1[3] = {-r, h, x}, b1[3] = {+r, h, x};
            out->push_back(make_seg(a0, b0, k++, 0));
            out->push_back(make_seg(a1, b1, k++, 0));
        }
    }
    if (!show_cams) return;
    uint32_t order = 0;
    uint32_t col = COL_RED;
    for (size_t c = 0; c < ncam; c++) {
        col = cams[c].keyframe ? COL_RED : COL_YELLOW;
        for (int i = 0; i < 9; i++) out->push_back(make_seg(cams[c].p[i], cams[c].p[i + 1], (++order << 3) | col, SEG_OVERLAY));
    }
    for (size_t c = 0; c + 1 < ncam; c++) out->push_back(make_seg(cams[c].p[5], cams[c + 1].p[5], (++order << 3) | col, SEG_OVERLAY));
    const float s = 0.3f, O[3] = {0, 0, 0}, X[3] = {s, 0, 0}, Y[3] = {0, s, 0}, Z[3] = {0, 0, s};
    out->push_back(make_seg(O, X, (++order << 3) | COL_RED, SEG_OVERLAY | SEG_WIDE));
    out->push_back(make_seg(O, Y, (++order << 3) | COL_GREEN, SEG_OVERLAY | SEG_WIDE));
    out->push_back(make_seg(O, Z, (++order << 3) | COL_BLUE, SEG_OVERLAY | SEG_WIDE));
}

// playPoses (view3d.cpp:418-458): for (float pos = 0; pos <= 1; pos += 0.02f) per pair of poses -- 51 steps in float --
// with pos2 = (1 + sin(-M_PI/2 + pos*M_PI)) / 2 in double and every member p1 + (p2 - p1) * pos2 rounded to float
inline void play_sequence(const Pose* poses, int32_t n, std::vector<Pose>* out) {
    out->clear();
    const float step_size = 0.02f;
    for (int32_t i = 0; i + 1 < n; i++) {
        const float* a = &poses[i].zoom;
        const float* b = &poses[i + 1].zoom;
        for (float pos = 0; pos <= 1; pos += step_size) {
            const double pos2 = (1 + sin(-M_PI / 2 + (double)pos * M_PI)) / 2;
            Pose q;
            float* o = &q.zoom;
            for (int k = 0; k < 6; k++) o[k] = (float)((double)a[k] + (double)(b[k] - a[k]) * pos2);
            out->push_back(q);
        }
    }
}

// ------------------------------------------------------------------------------------------- per primitive, fp32
MC_FN uint32_t float_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// the upper half of a depth key: window depths are >= 0, where the bit pattern orders like the number; an
// interpolated depth that rounding carried below 0 counts as 0
MC_FN uint32_t depth_bits(float zw) { return zw > 0.f ? float_bits(zw) : 0u; }

MC_FN bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

MC_FN void clip_coords(const float* m, float x, float y, float z, float* c) {
    c[0] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    c[1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    c[2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    c[3] = ((m[12] * x + m[13] * y) + m[14] * z) + m[15];
}

// a point is drawn only inside the clip volume; NaN fails a comparison, and an infinite cw is refused by name (with it
// +-inf would pass -cw <= c <= cw and divide to NaN)
MC_FN bool in_volume(const float* c) {
    const float w = c[3];
    return w > 0.f && w <= FLT_MAX && -w <= c[0] && c[0] <= w && -w <= c[1] && c[1] <= w && -w <= c[2] && c[2] <= w;
}

MC_FN void to_window(const Frame& f, const float* c, float* xw, float* yw, float* zw) {
    const float nx = c[0] / c[3], ny = c[1] / c[3], nz = c[2] / c[3];
    *xw = (nx * 0.5f + 0.5f) * (float)f.side + (float)f.ox;
    *yw = (ny * 0.5f + 0.5f) * (float)f.side + (float)f.oy;
    *zw = nz * 0.5f + 0.5f;
}

// glColor3f(val, val, val) as a byte: floor(clamp(val, 0, 1) * 255 + 0.5), 0 for NaN
MC_FN uint8_t grey_of(float val) {
    if (!(val == val)) return 0;
    const float lo = val < 0.f ? 0.f : val;
    const float hi = lo > 1.f ? 1.f : lo;
    return (uint8_t)floorf(hi * 255.0f + 0.5f);
}

// A world point of the 2-pixel kind: false when it is clipped; else it covers the window pixels {ix-1, ix} x {iy-1, iy}
// at depth bits zb.  round_half: the centre rule of an even size (floor(w + 0.5)); the 3-pixel anchor has the centre
// pixel floor(w) and covers {ix-1 .. ix+1} x {iy-1 .. iy+1}.
MC_FN bool point_window(const Frame& f, float x, float y, float z, bool round_half, int32_t* ix, int32_t* iy, uint32_t* zb) {
    float c[4], xw, yw, zw;
    clip_coords(f.m, x, y, z, c);
    if (!in_volume(c)) return false;
    to_window(f, c, &xw, &yw, &zw);
    const float h = round_half ? 0.5f : 0.0f;
    *ix = (int32_t)floorf(xw + h);
    *iy = (int32_t)floorf(yw + h);
    *zb = depth_bits(zw);
    return true;
}

// index of a window pixel in an image whose row 0 is the top
MC_FN size_t pixel_index(const Frame& f, int32_t x, int32_t y) { return (size_t)(f.H - 1 - y) * (size_t)f.W + (size_t)x; }
MC_FN bool in_image(const Frame& f, int32_t x, int32_t y) { return (uint32_t)x < (uint32_t)f.W && (uint32_t)y < (uint32_t)f.H; }

// Liang-Barsky in clip space against -x, +x, -y, +y, -z, +z in that order.  A, B are replaced by the clipped ends
// (each component a + t * (b - a)); false: nothing of the segment is inside, or a coordinate is not finite.
MC_FN bool clip_segment(float* A, float* B) {
    for (int i = 0; i < 4; i++)
        if (!finite_f(A[i]) || !finite_f(B[i])) return false;
    float t0 = 0.f, t1 = 1.f;
    for (int pl = 0; pl < 6; pl++) {
        const int ax = pl >> 1;
        const float da = (pl & 1) ? A[3] - A[ax] : A[3] + A[ax];
        const float db = (pl & 1) ? B[3] - B[ax] : B[3] + B[ax];
        if (da < 0.f && db < 0.f) return false;
        if (da < 0.f) {
            const float t = da / (da - db);
            t0 = t > t0 ? t : t0;
        } else if (db < 0.f) {
            const float t = da / (da - db);
            t1 = t < t1 ? t : t1;
        }
    }
    if (!(t0 <= t1)) return false;
    float a[4], b[4];
    for (int i = 0; i < 4; i++) {
        const float d = B[i] - A[i];
        a[i] = A[i] + t0 * d;
        b[i] = A[i] + t1 * d;
    }
    for (int i = 0; i < 4; i++) A[i] = a[i], B[i] = b[i];
    return A[3] > 0.f && B[3] > 0.f && finite_f(A[3]) && finite_f(B[3]);
}

// first integer p with p + 0.5 >= v, clamped to [0, lim]
MC_FN int32_t first_cell(float v, int32_t lim) {
    const float c = ceilf(v - 0.5f);
    return c > 0.f ? (c < (float)lim ? (int32_t)c : lim) : 0;
}

// One segment: plot(window x, window y, depth bits) for every pixel it covers.  The major axis is x when |dx| >= |dy|;
// it covers the cells p with min <= p + 0.5 < max along it, at t = ((p + 0.5) - a) / d the cell floor(na + t dn) of
// the minor axis and the depth za + t (zb - za); three pixels wide adds the minor neighbours -1 and +1.  The loop
// bounds are integers in [0, W] or [0, H] fixed before the loop.
template <class Plot>
MC_FN void raster_segment(const Frame& f, const Seg& s, Plot& plot) {
    float A[4], B[4], xa, ya, za, xb, yb, zb;
    clip_coords(f.m, s.a[0], s.a[1], s.a[2], A);
    clip_coords(f.m, s.b[0], s.b[1], s.b[2], B);
    if (!clip_segment(A, B)) return;
    to_window(f, A, &xa, &ya, &za);
    to_window(f, B, &xb, &yb, &zb);
    const float dx = xb - xa, dy = yb - ya, dz = zb - za;
    const bool xmajor = fabsf(dx) >= fabsf(dy);
    const float ma = xmajor ? xa : ya, mb = xmajor ? xb : yb, dm = xmajor ? dx : dy;
    const float na = xmajor ? ya : xa, dn = xmajor ? dy : dx;
    if (!(dm != 0.f) || !finite_f(dm)) return;   // zero length (|dn| <= |dm|)
    const int32_t lim = xmajor ? f.W : f.H, nlim = xmajor ? f.H : f.W;
    const int32_t p0 = first_cell(ma < mb ? ma : mb, lim), p1 = first_cell(ma < mb ? mb : ma, lim);
    const int32_t w = (s.flags & SEG_WIDE) ? 1 : 0;
    for (int32_t p = p0; p < p1; p++) {
        const float t = (((float)p + 0.5f) - ma) / dm;
        const float nf = floorf(na + t * dn);
        const float z = za + t * dz;
        if (!(nf >= -2.f && nf <= (float)nlim + 1.f)) continue;
        const int32_t q = (int32_t)nf;
        const uint32_t zbv = depth_bits(z);
        for (int32_t k = -w; k <= w; k++) {
            const int32_t x = xmajor ? p : q + k, y = xmajor ? q + k : p;
            if (in_image(f, x, y)) plot(x, y, zbv);
        }
    }
}

// Resolve of one pixel: the anchor where it won the depth test, else the overlay, else the depth winner's colour (the
// grid's grey 128, a point's grey gathered by its draw index), else the background
MC_FN void resolve_pixel(uint64_t key, uint32_t ovl, uint32_t anchor_index, const float* pts_xyzv, bool white, uint8_t* rgb) {
    const uint32_t idx = (uint32_t)key;
    uint8_t r, g, b;
    if (key != EMPTY_KEY && idx == anchor_index) {
        r = 255, g = 0, b = 0;
    } else if (ovl != 0u) {
        r = (ovl & COL_RED) ? 255 : 0, g = (ovl & COL_GREEN) ? 255 : 0, b = (ovl & COL_BLUE) ? 255 : 0;
    } else if (key != EMPTY_KEY) {
        r = g = b = idx < GRID_SEGS ? (uint8_t)128 : grey_of(pts_xyzv[4 * (size_t)(idx - GRID_SEGS) + 3]);
    } else {
        r = g = b = white ? 255 : 0;
    }
    rgb[0] = r, rgb[1] = g, rgb[2] = b;
}

}  // namespace view
}  // namespace svh

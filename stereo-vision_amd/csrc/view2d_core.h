// The numeric core of the 2-D panes (stereomapper/view2d.cpp:18-154 setImage, setColorImage, setMatches, paintGL; the
// colour-coded disparity map of stereothread.cpp:117-147) behind the svh_view2d_* entries of include/svh_view2d.h.
// View2D is a QGLWidget and OpenGL leaves the rasterisation of textured quads, lines and points partly to the
// implementation, so the arithmetic is written out here once.  THE CONTRACT IS THIS ARITHMETIC; equality with any
// OpenGL implementation is not verified anywhere in this project, and the widget's multisampling (QGL::SampleBuffers)
// and its blending (every colour here is opaque) are not reproduced.  Compiled from this one header by
//   * hipcc into the kernels of csrc/view2d_kernels.hip and into k_disp_color of csrc/map_kernels.hip,
//   * g++ -ffp-contract=off into tests/view/view2d_core_check.cpp, which pins it against the numpy restatement
//     tests/view2d_ref.py on the CPU.
// Nothing may be contracted into an FMA (-ffp-contract=off on every build): every fp32 operation below rounds once, in
// the order written, and a division is IEEE (div_rn).  The image is sampled in exact integers.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "view_core.h"   // MC_FN, first_cell, finite_f

namespace svh {
namespace view2d {

using view::finite_f;
using view::first_cell;

// Matcher::p_match / svh_p_match, field for field (csrc/view2d_engine.cpp asserts the size)
struct Match {
    float u1p, v1p;
    int32_t i1p;
    float u2p, v2p;
    int32_t i2p;
    float u1c, v1c;
    int32_t i1c;
    float u2c, v2c;
    int32_t i2c;
};

// the pane (W x H pixels, row 0 = top) and the image it shows: w x h texels, ch = 1 grey bytes `pitch` apart per row,
// ch = 3 RGB8 with pitch = 3 w, ch = 0 nothing set yet.  The image is drawn only if w > 1 && h > 1 (view2d.cpp:83).
struct Pane {
    int32_t W, H;
    int32_t w, h, ch;
    uint32_t pitch;
};

MC_FN float div_rn(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// a colour component as a byte: floor(clamp(c, 0, 1) * 255 + 0.5), 0 for NaN
MC_FN uint8_t byte_of(float c) {
    if (!(c == c)) return 0;
    const float lo = c < 0.f ? 0.f : c;
    const float hi = lo > 1.f ? 1.f : lo;
    return (uint8_t)floorf(hi * 255.0f + 0.5f);
}

// The colour of one disparity (stereothread.cpp:117-147), three floats: what svh_disparity_colormap returns and, through
// byte_of, what the disparity pane shows.  std::min(D / d_max, 1.0f) as its comparison: a NaN disparity stays NaN and
// the pixel black (fminf would give 1: red).  The double-typed sub-expressions are evaluated in double, narrowed once.
MC_FN void disparity_colour(float D, float* rgb) {
    const float q = div_rn(D, 200.f);
    const float val = (1.0f < q) ? 1.0f : q;
    float r = 0.f, g = 0.f, b = 0.f;
    if (val > 0) {
        const float h2 = (float)(6.0 * (1.0 - (double)val));
        const float x = (float)(1.0 * (1.0 - fabs((double)fmodf(h2, 2.0f) - 1.0)));
        if (0 <= h2 && h2 < 1)       { r = 1; g = x; b = 0; }
        else if (1 <= h2 && h2 < 2)  { r = x; g = 1; b = 0; }
        else if (2 <= h2 && h2 < 3)  { r = 0; g = 1; b = x; }
        else if (3 <= h2 && h2 < 4)  { r = 0; g = x; b = 1; }
        else if (4 <= h2 && h2 < 5)  { r = x; g = 0; b = 1; }
        else if (5 <= h2 && h2 <= 6) { r = 1; g = 0; b = x; }
    }
    rgb[0] = r, rgb[1] = g, rgb[2] = b;
}

// GL_NEAREST over the unit quad under glOrtho(0, 1, 1, 0): pane pixel p of n_pane shows texel ((2 p + 1) n_img) / (2 n_pane)
// by integer division -- the texel under the pixel's centre.  p < n_pane <= 16384 and n_img <= 16384: below 2^30.
MC_FN int32_t texel_of(int32_t p, int32_t n_pane, int32_t n_img) {
    return (int32_t)((((uint32_t)p * 2u + 1u) * (uint32_t)n_img) / ((uint32_t)n_pane * 2u));
}

MC_FN bool in_pane(const Pane& f, int32_t x, int32_t y) { return (uint32_t)x < (uint32_t)f.W && (uint32_t)y < (uint32_t)f.H; }
MC_FN size_t pixel_index(const Pane& f, int32_t x, int32_t y) { return (size_t)y * (size_t)f.W + (size_t)x; }

// glVertex3f(u / (float)_image_width, v / (float)_image_height, 0) through glOrtho(0, 1, 1, 0) and the viewport
MC_FN void to_window(const Pane& f, float u, float v, float* xw, float* yw) {
    *xw = div_rn(u, (float)f.w) * (float)f.W;
    *yw = div_rn(v, (float)f.h) * (float)f.H;
}

// the two ends of match m in the pane: (u1p, v1p) -> (u1c, v1c) in the left pane, (u2p, v2p) -> (u2c, v2c) in the right
MC_FN void match_ends(const Pane& f, const Match& m, bool left, float* xa, float* ya, float* xb, float* yb) {
    to_window(f, left ? m.u1p : m.u2p, left ? m.v1p : m.v2p, xa, ya);
    to_window(f, left ? m.u1c : m.u2c, left ? m.v1c : m.v2c, xb, yb);
}

// glLineWidth(2): plot(x, y) for every pane pixel of the line (xa, ya) -> (xb, yb).  The major axis is x when
// |dx| >= |dy|; it covers the cells p with min <= p + 0.5 < max along it and, at t = ((p + 0.5) - a) / d, the two minor
// cells q = floor((na + t dn) - 0.5) and q + 1.  The loop bounds are integers in [0, W] or [0, H] fixed before the loop;
// nothing is clipped geometrically, pixels outside the pane are dropped.  A zero-length line and one with an end that
// is not finite draw nothing.
template <class Plot>
MC_FN void raster_line(const Pane& f, float xa, float ya, float xb, float yb, Plot& plot) {
    if (!finite_f(xa) || !finite_f(ya) || !finite_f(xb) || !finite_f(yb)) return;
    const float dx = xb - xa, dy = yb - ya;
    const bool xmajor = fabsf(dx) >= fabsf(dy);
    const float ma = xmajor ? xa : ya, mb = xmajor ? xb : yb, dm = xmajor ? dx : dy;
    const float na = xmajor ? ya : xa, dn = xmajor ? dy : dx;
    if (!(dm != 0.f) || !finite_f(dm)) return;   // zero length (|dn| <= |dm|)
    const int32_t lim = xmajor ? f.W : f.H, nlim = xmajor ? f.H : f.W;
    const int32_t p0 = first_cell(ma < mb ? ma : mb, lim), p1 = first_cell(ma < mb ? mb : ma, lim);
    for (int32_t p = p0; p < p1; p++) {
        const float t = div_rn(((float)p + 0.5f) - ma, dm);
        const float nf = floorf((na + t * dn) - 0.5f);
        if (!(nf >= -3.f && nf <= (float)nlim + 2.f)) continue;
        const int32_t q = (int32_t)nf;
        for (int32_t k = 0; k <= 1; k++) {
            const int32_t x = xmajor ? p : q + k, y = xmajor ? q + k : p;
            if (in_pane(f, x, y)) plot(x, y);
        }
    }
}

// glPointSize(5): drawn iff the centre is finite and 0 <= xw <= W, 0 <= yw <= H (the clip volume, borders included);
// the centre pixel is (floor(xw), floor(yw)), the footprint +-2 around it, cut by the pane's border
template <class Plot>
MC_FN void raster_point(const Pane& f, float xw, float yw, Plot& plot) {
    if (!finite_f(xw) || !finite_f(yw)) return;
    if (!(0.f <= xw && xw <= (float)f.W && 0.f <= yw && yw <= (float)f.H)) return;
    const int32_t cx = (int32_t)floorf(xw), cy = (int32_t)floorf(yw);
    for (int32_t dy = -2; dy <= 2; dy++)
        for (int32_t dx = -2; dx <= 2; dx++)
            if (in_pane(f, cx + dx, cy + dy)) plot(cx + dx, cy + dy);
}

// the overlay word of match i: its line writes 2 i + 1, its point 2 i + 2; the larger word was drawn later.  0 is
// "nothing drawn", and every int32 count fits: 2 (2^31 - 2) + 2 < 2^32.
MC_FN uint32_t line_word(uint32_t i) { return 2u * i + 1u; }
MC_FN uint32_t point_word(uint32_t i) { return 2u * i + 2u; }

// match i, line then point, through plot(x, y, word)
template <class Plot3>
MC_FN void raster_match(const Pane& f, const Match& m, bool left, uint32_t i, Plot3& plot) {
    float xa, ya, xb, yb;
    match_ends(f, m, left, &xa, &ya, &xb, &yb);
    struct With {
        Plot3& plot;
        uint32_t word;
        MC_FN void operator()(int32_t x, int32_t y) { plot(x, y, word); }
    };
    With line{plot, line_word(i)}, point{plot, point_word(i)};
    raster_line(f, xa, ya, xb, yb, line);
    raster_point(f, xb, yb, point);
}

// glColor3f of a match (view2d.cpp:106-115): an outlier is blue; an inlier (col, 1 - col, 0) with
// col = max(min(u1p - u2p, 100), 0) / 100 in BOTH panes, std::min / std::max as their comparisons so that NaN stays NaN
MC_FN void match_colour(const Match& m, bool inlier, uint8_t* rgb) {
    if (!inlier) {
        rgb[0] = 0, rgb[1] = 0, rgb[2] = 255;
        return;
    }
    float d = m.u1p - m.u2p;
    d = (100.f < d) ? 100.f : d;
    d = (d < 0.f) ? 0.f : d;
    const float col = div_rn(d, 100.f);
    rgb[0] = byte_of(col), rgb[1] = byte_of(1.f - col), rgb[2] = 0;
}

// Resolve of pane pixel (px, py): the overlay if something was drawn there (the colour gathered from the match record),
// else the texel under the pixel's centre, else black
MC_FN void resolve_pixel(const Pane& f, const uint8_t* tex, uint32_t ovl, const Match* m, const uint8_t* inlier,
                         int32_t px, int32_t py, uint8_t* rgb) {
    if (ovl != 0u) {
        const uint32_t i = (ovl - 1u) >> 1;
        match_colour(m[i], inlier[i] != 0, rgb);
    } else if (f.ch != 0 && f.w > 1 && f.h > 1) {
        const int32_t sx = texel_of(px, f.W, f.w), sy = texel_of(py, f.H, f.h);
        if (f.ch == 1) {
            rgb[0] = rgb[1] = rgb[2] = tex[(size_t)sy * f.pitch + (size_t)sx];
        } else {
            const uint8_t* t = tex + (size_t)sy * f.pitch + 3 * (size_t)sx;
            rgb[0] = t[0], rgb[1] = t[1], rgb[2] = t[2];
        }
    } else {
        rgb[0] = rgb[1] = rgb[2] = 0;
    }
}

}  // namespace view2d
}  // namespace svh

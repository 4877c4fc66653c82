// The numeric core of StereoImage::histogramNormalization (stereomapper/stereoimage.cpp:94-134), one source for the
// host (csrc/histnorm_engine.cpp: the segment table, svh_histnorm_table_host) and the device (csrc/histnorm_kernels.hip:
// k_hist_table).
//
// THE CONTRACT is the reference's operations in the reference's order, as its x86-64 build performs them.  With
// N = width * height (an int) and count[g] the number of pixels of grey level g:
//     c      = (float)(1.0 / (double)(float)N)
//     p[g]   = f(count[g]),  f(0) = 0,  f(n) = fl32(f(n-1) + c)          (the reference adds c once per pixel)
//     cdf[0] = p[0],  cdf[g] = fl32(cdf[g-1] + p[g])                      strictly in the order of g
//     map[g] = (uint8_t)(int32_t)((double)cdf[g] * 255.0)
// The last line is what `(uint8_t)(cdf[i]*255.0)` compiles to on x86-64: a truncating conversion to a 32-bit integer
// whose low byte is kept.  The chain can pass 1 (a flat 1392x512 frame ends at 1.009): the product is then 257.3 and
// the byte WRAPS to 1.  The wrap is part of the contract, not an accident to be repaired.  The fp64 product is exact
// (24 bits by 8 bits).
//
// f(n) is not evaluated by n additions.  While x = f(n) stays inside one binade [2^e, 2^(e+1)) and the exact sum
// x + c stays below 2^(e+1), the sum is rounded to a multiple of ulp = 2^(e-23); with c = q ulp + r, 0 <= r < ulp, the
// step is q ulp (r < ulp/2), (q+1) ulp (r > ulp/2) and, for r = ulp/2 exactly, ties-to-even: the parity of x / ulp
// decides the FIRST such step of the binade, and every later one starts from an even multiple (q odd) or from the
// parity the first one left (q even), so it repeats.  Two equal consecutive steps inside a binade therefore repeat until
// the exact sum reaches the binade's end.  Once c <= ulp/2 the chain stands still (or moves once more, to an even
// multiple, and then stands still).  So f is piecewise linear in n; build_segments walks it binade by binade:
// single real float additions where a step may differ (the first step of a binade, a step across a binade's end), one
// integer division for the length of a run of equal steps.  Its cost is a few operations per binade, never per pixel.
//
// Every value below is a multiple of 2^-52 smaller than 2^10 (c >= 2^-28 has 24 significant bits; f stays below 4), so
// the run lengths are computed in int64 units of 2^-52, exactly.
// No operation here may be contracted into an FMA (-ffp-contract=off on every build).
#pragma once
#include "mono_core.h"   // MC_FN

namespace svh {
namespace hn {

constexpr int32_t MAX_SIDE = 16384;   // N <= 2^28, so c >= 2^-28
constexpr int32_t MAX_SEG = 192;      // <= 4 segments per binade from 2^-28 to 2^2, and the closing one

// f(n) = f + (n - n0) * inc for n0 <= n < the next segment's n0; the last segment starts at N or where the chain stands
struct Seg {
    int32_t n0;
    float f, inc;
};

MC_FN float fraction(int32_t width, int32_t height) { return (float)(1.0 / (double)(float)(width * height)); }

// one step of the chain: a float addition that rounds once (the volatile keeps a host compiler from carrying excess
// precision or folding consecutive steps)
MC_FN float step(float x, float c) {
    volatile float y = x + c;
    return y;
}

// ---- host only: the table is built once per image size
inline int64_t units(float v) { return (int64_t)ldexp((double)v, 52); }   // exact: see above
inline float from_units(int64_t u) { return (float)ldexp((double)u, -52); }

// the segments of f for N additions of c; returns their number, or -1 if MAX_SEG does not hold them (it does for
// every N <= 2^28)
inline int build_segments(float c, int32_t N, Seg* seg) {
    int ns = 0;
    int32_t n = 0;
    float x = 0.f;
    const int64_t C = units(c);
    while (n < N) {
        if (ns + 2 > MAX_SEG) return -1;
        const float y = step(x, c);
        if (y == x) break;   // stands still from here on
        bool run = false;
        if (x > 0.f) {
            int e;
            (void)frexp((double)x, &e);                      // x in [2^(e-1), 2^e)
            const int64_t HI = (int64_t)1 << (e + 52);        // the end of x's binade
            const int64_t X = units(x), Y = units(y);
            if (X + C < HI && Y + C < HI) {                   // both steps are rounded at this binade's ulp
                const float z = step(y, c);
                const int64_t D = Y - X;
                if (units(z) - Y == D) {
                    // steps j = 0, 1, ... while X + j D + C < HI
                    int64_t k = (HI - C - X + D - 1) / D;
                    if (k > (int64_t)(N - n)) k = N - n;
                    seg[ns++] = {n, x, from_units(D)};
                    n += (int32_t)k;
                    x = from_units(X + k * D);
                    run = true;
                }
            }
        }
        if (!run) {
            seg[ns++] = {n, x, (float)((double)y - (double)x)};
            n += 1;
            x = y;
        }
    }
    seg[ns++] = {n, x, 0.f};
    // a segment that continues the line of the one before it (a single step that came out as the run's step) joins it
    int m = 0;
    for (int i = 0; i < ns; i++) {
        if (m > 0 && seg[m - 1].inc == seg[i].inc &&
            (double)seg[m - 1].f + (double)(seg[i].n0 - seg[m - 1].n0) * (double)seg[m - 1].inc == (double)seg[i].f)
            continue;
        seg[m++] = seg[i];
    }
    return m;
}

// f(count) from the table: the last segment that starts at or below count, by bisection.  The product and the sum are
// exact in fp64, and the result is a float by construction.
MC_FN float eval(const Seg* seg, int ns, int32_t count) {
    int lo = 0, hi = ns - 1;   // seg[0].n0 == 0 <= count
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].n0 <= count) lo = mid;
        else hi = mid - 1;
    }
    return (float)((double)seg[lo].f + (double)(count - seg[lo].n0) * (double)seg[lo].inc);
}

// the serial part: cdf in the order of g
MC_FN void cdf_chain(const float* p, float* cdf) {
    float s = p[0];
    cdf[0] = s;
    for (int g = 1; g < 256; g++) {
        s = s + p[g];
        cdf[g] = s;
    }
}

MC_FN uint8_t map_entry(float cdf) { return (uint8_t)(int32_t)((double)cdf * 255.0); }

}  // namespace hn
}  // namespace svh

// The integer paths of stereo-vision_amd/csrc/grid_dyn_core.h at their extremes, compiled by the host compiler alone, as a program
// of its own: tests/test_grid_dyn.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a signed overflow in
// rdiv64, the height of a line, the stepper, a body or the settle ends the run, and compares what it prints with
// tests/grid_dyn_ref.py.
//
//   grid_dyn_check
//   stdout: "height q_o q_e n sum hash" per line: the sum of its heights and a hash of their sequence, every step checked here against
//           a 128-bit evaluation and against the stepper (exit status 1); "body count hmin hmax margin lo hi" per probe cell;
//           "settle case contra last event count overhead" per probe of the settle at its limits.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "grid_dyn_core.h"

using namespace svh;

static __int128 floor_div(__int128 a, __int128 b) {   // b > 0
    __int128 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

static int run_height(int32_t q_o, int32_t q_e, int32_t n) {
    long long sum = 0;
    uint64_t h = 1469598103934665603ull;
    grid::HeightStepper st(q_o, q_e, n);
    for (int32_t k = 0; k < n; k++) {
        const int32_t q = grid::line_height(q_o, q_e, n, k);
        const __int128 want = (__int128)q_o + floor_div((__int128)2 * k * ((__int128)q_e - q_o) + n, (__int128)2 * n);
        if ((__int128)q != want || st.height() != q) {
            fprintf(stderr, "height (%d, %d, %d) step %d: closed form %d, stepper %d, wanted %lld\n", q_o, q_e, n, k, q, st.height(), (long long)want);
            return 1;
        }
        sum += q;
        h = (h ^ (uint64_t)(uint32_t)q) * 1099511628211ull;
        st.step();
    }
    printf("height %d %d %d %lld %llu\n", q_o, q_e, n, sum, (unsigned long long)h);
    return 0;
}

int main() {
    const int32_t L = 1 << 30;   // |q| <= 2^30
    const int32_t qs[] = {0, 1, -1, 1536, -307, L, -L, L - 1, -(L - 1)};
    const int32_t ns[] = {1, 2, 3, 5, 64, 4095, grid::MAX_SIDE - 1};
    for (int32_t q_o : qs)
        for (int32_t q_e : qs)
            for (int32_t n : ns)
                if (run_height(q_o, q_e, n)) return 1;
    // rdiv64 at negative numerators and at the largest product
    const int64_t big = (int64_t)8191 * ((int64_t)2 * L);
    if (grid::rdiv64(-6144, 5) != -1229 || grid::rdiv64(-1, 2) != 0 || grid::rdiv64(-3, 2) != -1 || grid::rdiv64(1, 2) != 1 ||
        grid::rdiv64(-big, 8191) != -(int64_t)2 * L || grid::rdiv64(big, 8191) != (int64_t)2 * L || grid::rdiv64(-big, 8192) != -2147221504ll)
        return 2;
    grid::Params p;
    p.nx = p.nz = 4;
    p.cell = 1.f, p.x0 = 0.f, p.z0 = 0.f;
    const float T[12] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0};
    for (int k = 0; k < 12; k++) p.T[k] = T[k];
    p.min_points = 1, p.step = 0.2f, p.drop = 0.3f, p.clearance = 2.f, p.h_lo = 0.f, p.h_hi = 2.f;
    if (!grid::params_ok(p)) return 3;
    // bodies: heights and margins up to their limits; a tall cell's top is above the step, so q_hi stays above -2^30
    const float top = 1048575.9375f;   // the largest binned height, just inside 2^20
    const float hs[][2] = {{0.25f, 1.0f}, {-top, top}, {top, top}, {-top, 0.25f}, {0.1f, 0.2f}, {-top, -top}};
    const float ms[] = {0.f, 0.1f, 0.75f, 2.f, 1048575.f, top};
    for (const auto& h : hs)
        for (float m : ms)
            for (int32_t count : {0, 1}) {
                grid::DynParams d{2, 3, m, 0, 0};
                if (!grid::dyn_derive(d)) return 4;
                const grid::Body b = grid::body_of(p, d, count, grid::key_of(h[0]), grid::key_of(h[1]));
                printf("body %d %.9g %.9g %.9g %d %d\n", count, (double)h[0], (double)h[1], (double)m, b.lo, b.hi);
                if (grid::goes_through(b, b.lo) != (b.lo <= b.hi) || grid::goes_through(b, b.hi) != (b.lo <= b.hi)) return 5;
            }
    grid::DynParams bad{2, 3, 1048576.f, 0, 0};
    if (grid::dyn_derive(bad)) return 6;
    // settle at the limits of the stamp and of the counters
    const int32_t S = grid::STAMP_LIMIT;
    struct Probe {
        int32_t clear_frames, max_age, stamp, contra, last, through, fcount;
        float fh;
    };
    const Probe probes[] = {{65535, 0, S, 65534, S - 1, 1 << 30, 0, 0.f},   // the last contradiction of the longest run, at the last stamp
                            {0, 0, S, S - 1, 0, S, 0, 0.f},                  // never cleared: CONTRA reaches the stamp
                            {2, S - 1, S, 0, 0, 0, 0, 0.f},                  // age S > max_age S - 1 with LAST never
                            {2, S - 1, S, 0, 1, 0, 0, 0.f},                  // age S - 1: exactly max_age, kept
                            {1, 1, S, 0, S - 2, 3, 0, 0.f},                  // cleared and old at once
                            {2, 0, S, 1, S - 1, 3, S - 8, 1.5f}};            // a confirming frame whose count fills the cell to 2^31 - 1
    int k = 0;
    for (const Probe& q : probes) {
        grid::DynParams d{q.clear_frames, 3, 0.1f, q.max_age, 0};
        if (!grid::dyn_derive(d)) return 7;
        grid::Cell c{7, 2, grid::key_of(0.25f), grid::key_of(1.0f), 7 * 640, 7 * 100};
        grid::Cell f = grid::empty_cell();
        if (q.fcount > 0) f = grid::Cell{q.fcount, 1, grid::key_of(q.fh), grid::key_of(q.fh), (int64_t)q.fcount * 1536, (uint64_t)q.fcount * 255u};
        int32_t contra = q.contra, last = q.last;
        const uint8_t ev = grid::settle(p, d, q.stamp, c, contra, last, f, q.through);
        printf("settle %d %d %d %d %d %d\n", k++, contra, last, (int)ev, c.count, c.overhead);
    }
    return 0;
}

// The local-map arithmetic of stereo-vision_amd/csrc/grid_core.h -- the line of a ray and place() under window offsets --
// compiled by the host compiler alone, as a program of its own: tests/test_grid_local.py builds it with
// -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all, so a signed overflow in rdiv or an out-of-range
// conversion in place() at the extremes ends the run, and compares what it prints with tests/grid_local_ref.py.
//
//   grid_line_check
//   stdout: "line dx dz n sa sb h" per line from cell (0, 0) to (dx, dz): its length, the sums of its cells' coordinates and
//           a hash of the cell sequence; then "place oa ob k fate cell slot" per probe point of an 8192 x 8192 window of
//           unit cells at offsets (oa, ob).  Every line is also checked here against a 64-bit evaluation: exit status 1.
#include <stdint.h>
#include <stdio.h>

#include "grid_core.h"

using namespace svh;

static long long floor_div(long long a, long long b) {   // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

static int run_line(int32_t dx, int32_t dz) {
    const int32_t n = grid::line_len(dx, dz);
    long long sa = 0, sb = 0;
    uint64_t h = 1469598103934665603ull;
    for (int32_t k = 0; k < n; k++) {
        int32_t sx, sz;
        grid::line_step(dx, dz, n, k, &sx, &sz);
        const long long wx = floor_div(2ll * k * dx + n, 2ll * n), wz = floor_div(2ll * k * dz + n, 2ll * n);
        if (sx != wx || sz != wz) {
            fprintf(stderr, "line (%d, %d) step %d: (%d, %d), wanted (%lld, %lld)\n", dx, dz, k, sx, sz, wx, wz);
            return 1;
        }
        sa += sx, sb += sz;
        h = (h ^ (uint64_t)(uint32_t)sx) * 1099511628211ull;
        h = (h ^ (uint64_t)(uint32_t)sz) * 1099511628211ull;
    }
    printf("line %d %d %d %lld %lld %llu\n", dx, dz, n, sa, sb, (unsigned long long)h);
    return 0;
}

int main() {
    const int32_t M = grid::MAX_SIDE - 1;   // the longest line of a window: k * dx reaches 8190 * 8191
    const int32_t ds[] = {0, 1, -1, 2, -2, 3, 4095, -4096, M - 1, -(M - 1), M, -M};
    for (int32_t dx : ds)
        for (int32_t dz : ds)
            if (run_line(dx, dz)) return 1;
    grid::Params p;
    p.nx = p.nz = grid::MAX_SIDE;
    p.cell = 1.f, p.x0 = 0.f, p.z0 = 0.f;
    const float T[12] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0};
    for (int k = 0; k < 12; k++) p.T[k] = T[k];
    p.min_points = 1, p.step = 0.2f, p.drop = 0.3f, p.clearance = 2.f, p.h_lo = 0.f, p.h_hi = 2.f;
    const int32_t L = grid::OFFSET_LIMIT;
    const int32_t offs[][2] = {{L, L}, {-L, -L}, {L, -L}, {-L, L}, {0, 0}, {-1, 1}, {L - 1, -L + 1}};
    for (const auto& o : offs) {
        p.oa = o[0], p.ob = o[1];
        if (!grid::params_ok(p)) return 2;
        // around both edges of the window on both axes, its middle, far outside, and what is no position at all
        const float as[] = {(float)o[0] - 1.f, (float)o[0] - 0.5f, (float)o[0], (float)o[0] + 0.5f, (float)o[0] + 4096.f,
                            (float)(o[0] + grid::MAX_SIDE) - 1.f, (float)(o[0] + grid::MAX_SIDE) - 0.5f,
                            (float)(o[0] + grid::MAX_SIDE), 3e38f, -3e38f, 1e10f, -1e10f, 1048576.f, -1048577.f};
        const float bs[] = {(float)o[1] - 1.f, (float)o[1], (float)o[1] + 0.25f, (float)(o[1] + grid::MAX_SIDE) - 1.f,
                            (float)(o[1] + grid::MAX_SIDE), -3e38f, 3e38f};
        int k = 0;
        for (float a : as)
            for (float b : bs) {
                const grid::Placed r = grid::place(p, a, -0.5f, b, 0.5f);
                int32_t ga = 0, gb = 0;
                const bool has = grid::global_cell(p, a, -0.5f, b, &ga, &gb);
                printf("place %d %d %d %d %u %u %d %d %d\n", o[0], o[1], k++, r.fate, r.cell,
                       r.cell == grid::NO_CELL ? grid::NO_CELL : r.slot, (int)has, ga, gb);
            }
    }
    return 0;
}

// The archive's arithmetic (stereo-vision_amd/csrc/grid_archive_core.h) on the host, as a program of its own for the address and
// undefined-behaviour sanitizers (tests/test_grid_archive.py builds and runs it): every lane of every strip of the contract's scroll
// list lies in the window, outside the displaced window and is met once, the count is that of the set difference, and the keys at
// the ends of the global cells read back.  Prints "archive core ok, N scrolls".
#include <cstdio>
#include <set>
#include <utility>
#include "grid_archive_core.h"
using namespace svh::grid;
int main() {
    long checked = 0;
    const int sizes[][2] = {{40, 24}, {16, 16}, {1, 1}, {17, 1}, {8192, 3}};
    for (auto& s : sizes) {
        const int nx = s[0], nz = s[1];
        const int steps[] = {1, 15, 16, 17, nx - 1, nx, nx + 1, 3 * nx, nz - 1, nz, nz + 1, 3 * nz, 0};
        for (int da : steps) for (int db : steps) for (int sa : {1, -1}) for (int sb : {1, -1}) {
            const int a = sa * da, b = sb * db;
            if (!a && !b) continue;
            const uint32_t n = strip_count(nx, nz, a, b);
            std::set<std::pair<int, int>> seen;
            for (uint32_t t = 0; t < n; t++) {
                int ia, ib;
                strip_cell(nx, nz, a, b, t, &ia, &ib);
                if (ia < 0 || ia >= nx || ib < 0 || ib >= nz) { printf("out of window\n"); return 1; }
                const bool in_new = ia - a >= 0 && ia - a < nx && ib - b >= 0 && ib - b < nz;
                if (in_new || !seen.insert({ia, ib}).second) { printf("bad cell\n"); return 1; }
            }
            long want = 0;
            for (int ib = 0; ib < nz; ib++) for (int ia = 0; ia < nx; ia++) want += !(ia - a >= 0 && ia - a < nx && ib - b >= 0 && ib - b < nz);
            if (want != (long)n) { printf("count %ld != %u\n", want, n); return 1; }
            checked++;
        }
    }
    const int lim = (1 << 20) - 1;
    for (int g : {-lim, -17, -16, -1, 0, 15, 16, lim}) {
        const unsigned long long k = cell_key(g, -g);
        if (key_ta(k) != tile_of(g) || key_tb(k) != tile_of(-g) || k == TILE_NONE || tile_index(g, -g) > 255) { printf("key\n"); return 1; }
        (void)tile_home(k, archive_table_size(ARCHIVE_MAX_TILES) - 1);
    }
    printf("archive core ok, %ld scrolls\n", checked);
    return 0;
}

// The frontiers of stereo-vision_amd/csrc/grid_front_core.h -- the frontier bit at the window's edges, the flood fill, the
// centroid in int64 and the representative's key -- compiled by the host compiler alone, as a program of its own:
// tests/test_grid_front.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane at
// the window's edge or a signed overflow ends the run, and compares what it writes with tests/grid_front_ref.py.
//
//   grid_front_check job.bin
//   job.bin: int32 nx, nz, oa, ob, max_cell_cost, min_size, unexplored, border; then STATE and COST (nx * nz bytes each)
//   stdout:  int64 stats[5]; FRONT (nx * nz bytes), LABEL (nx * nz int32); the records (10 int32 each, stats[2] of them).
//            Exit status 3: the parameters are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_front_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[8];
    if (fread(head, 4, 8, f) != 8) return 2;
    const int32_t nx = head[0], nz = head[1], oa = head[2], ob = head[3];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob)) return 2;
    const grid::FrontParams p{head[4], head[5], (uint32_t)head[6], head[7]};
    const size_t cells = (size_t)nx * (size_t)nz;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<uint8_t> state(cells), cost(cells);
    if (fread(state.data(), 1, cells, f) != cells || fread(cost.data(), 1, cells, f) != cells) return 2;
    fclose(f);
    if (!grid::front_ok(p)) return 3;
    std::vector<uint8_t> flags(cells);
    std::vector<int32_t> label(cells), recs;
    int64_t stats[grid::FS_WORDS];
    grid::front_window(p, nx, nz, oa, ob, state.data(), cost.data(), flags.data(), label.data(), &recs, stats);
    if ((int64_t)recs.size() != stats[grid::FS_KEPT] * grid::FRONT_REC) return 1;
    fwrite(stats, 8, grid::FS_WORDS, stdout);
    fwrite(flags.data(), 1, cells, stdout);
    fwrite(label.data(), 4, cells, stdout);
    fwrite(recs.data(), 4, recs.size(), stdout);
    return 0;
}

// The pose planner of stereo-vision_amd/csrc/grid_pose_core.h -- CF from the footprint table, the prices, the six moves with the
// corner rule, the heap Dijkstra over the reversed graph with its cap, PDIR and the walk -- compiled by the host compiler alone, as
// a program of its own: tests/test_grid_pose.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read
// beyond a plane at the window's edge or a heading's end, or a signed overflow in a candidate next to max_cost = 0x7FFFFFFE, ends
// the run, and compares what it writes with tests/grid_pose_ref.py.
//
//   grid_pose_check job.bin
//   job.bin: int32 nx, nz, oa, ob, neutral, max_cost, turn, reverse, spin, headings_m, stop_cost, unknown_cost, n goals, start a,
//            start b, start d; float32 front, rear, half_width, cell; then the goals (3 n int32) and COST (nx * nz bytes)
//   stdout:  int64 goal states that count; CF (8 nx nz bytes), PPOT (8 nx nz int32), PDIR (8 nx nz bytes); int64 len of the walk
//            from the start state and its poses (3 len int32).  Exit status 3: the parameters are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_pose_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[16];
    float len4[4];
    if (fread(head, 4, 16, f) != 16 || fread(len4, 4, 4, f) != 4) return 2;
    const int32_t nx = head[0], nz = head[1], oa = head[2], ob = head[3], n = head[12];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || n < 0 || n > grid::POSE_MAX_GOALS) return 2;
    const grid::PoseParams p{head[4], head[5], head[6], head[7], head[8]};
    const grid::RollParams r{len4[0], len4[1], len4[2], head[9], head[10], head[11], 0, 0, 0};
    const size_t cells = (size_t)nx * (size_t)nz, states = cells * grid::POSE_HEADINGS;
    std::vector<int32_t> goals(3 * (size_t)n);
    std::vector<uint8_t> cost(cells);
    if (fread(goals.data(), 4, goals.size(), f) != goals.size() || fread(cost.data(), 1, cells, f) != cells) return 2;
    fclose(f);
    if (!grid::pose_ok(p)) return 3;
    for (int32_t k = 0; k < n; k++)
        if (!grid::pose_goal_ok(goals.data() + 3 * k)) return 3;
    std::vector<int32_t> offs;
    std::vector<int64_t> start;
    if (!grid::roll_table(r, len4[3], &offs, &start)) return 3;
    offs.shrink_to_fit();
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<uint8_t> cf(states), dir(states);
    std::vector<int32_t> pot(states);
    grid::pose_cf_window(nx, nz, cost.data(), offs.data(), start.data(), r.m, r.unknown_cost, cf.data());
    const int64_t counted = grid::pose_window(p, r.stop_cost, nx, nz, oa, ob, cf.data(), goals.data(), n, pot.data(), dir.data());
    std::vector<int32_t> path(3 * states);
    const int64_t len = grid::pose_walk(nx, nz, oa, ob, r.m, dir.data(), head[13], head[14], head[15], path.data(), (int64_t)states);
    // the walk with no room writes nothing and counts the same
    if (grid::pose_walk(nx, nz, oa, ob, r.m, dir.data(), head[13], head[14], head[15], nullptr, 0) != len) return 1;
    fwrite(&counted, 8, 1, stdout);
    fwrite(cf.data(), 1, states, stdout);
    fwrite(pot.data(), 4, states, stdout);
    fwrite(dir.data(), 1, states, stdout);
    fwrite(&len, 8, 1, stdout);
    fwrite(path.data(), 4, 3 * (size_t)len, stdout);
    return 0;
}

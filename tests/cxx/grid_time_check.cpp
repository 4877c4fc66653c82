// The time layer of stereo-vision_amd/csrc/grid_time_core.h -- the released cells, the distance passes on FLAGS', the planner on
// RCOST, the sweep over the layers with the blocks read by global cell, TDIR and the walk -- compiled by the host compiler alone, as a
// program of its own: tests/test_grid_time.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond
// a plane at the window's edge or beyond the last layer, a shift of a signed word at slot 31, or a signed overflow in a candidate next
// to max_cost = 0x7FFFFFFE ends the run, and compares what it writes with tests/grid_time_ref.py.
//
//   grid_time_check job.bin
//   job.bin: int32 nx, nz, oa, ob, poa, pob, neutral, unknown, max_cost, slots, stride, poses_per_step, only_moving, layers, wait,
//            release, reach, n goals, n tracks, start a, start b; then the goals (2 n int32), the tracks (14 per track), COST, FLAGS and
//            CLASS (nx * nz bytes each), the cost table (reach^2 + 1 bytes), PRED (nx * nz uint32), the ID plane (nx * nz int32)
//   stdout:  int64 released; RCOST (bytes), RPOT (int32), RDIR (bytes); TPOT (L nx nz int32), TDIR (L nx nz bytes); int64 stats[4];
//            int64 status, len of the walk from the start and its triples (3 len int32).
//            Exit status 3: the parameters are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_time_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[21];
    if (fread(h, 4, 21, f) != 21) return 2;
    const int32_t nx = h[0], nz = h[1], oa = h[2], ob = h[3], poa = h[4], pob = h[5], reach = h[16], n = h[17], nt = h[18];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || !grid::offsets_ok(poa, pob) || n < 0 ||
        n > grid::PLAN_MAX_GOALS || nt < 0 || nt > grid::OBJ_MAX_TRACKS || reach < 1 || reach > grid::MAX_REACH)
        return 2;
    const grid::PlanParams pl{h[6], h[7], h[8]};
    const grid::PredParams pp{h[9], h[10], h[11], 0, 0, h[12]};
    const grid::TimeParams tp{h[13], h[14], h[15]};
    if (!grid::plan_ok(pl) || !grid::pred_ok(pp) || !grid::time_ok(tp) || !grid::time_fits(tp, nx, nz)) return 3;
    const size_t cells = (size_t)nx * (size_t)nz, states = cells * (size_t)tp.layers;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<int32_t> goals(2 * (size_t)n), tracks((size_t)nt * grid::TRACK_REC), id(cells);
    std::vector<uint8_t> cost(cells), flags(cells), cls(cells), table((size_t)reach * (size_t)reach + 1);
    std::vector<uint32_t> pred(cells);
    if (fread(goals.data(), 4, goals.size(), f) != goals.size() || fread(tracks.data(), 4, tracks.size(), f) != tracks.size() ||
        fread(cost.data(), 1, cells, f) != cells || fread(flags.data(), 1, cells, f) != cells || fread(cls.data(), 1, cells, f) != cells ||
        fread(table.data(), 1, table.size(), f) != table.size() || fread(pred.data(), 4, cells, f) != cells || fread(id.data(), 4, cells, f) != cells)
        return 2;
    fclose(f);
    std::vector<uint8_t> f2(cells), rcost(cost), rdir(cells), tdir(states);
    std::vector<uint16_t> gcol(cells), price(cells);
    std::vector<int32_t> rpot(cells), tpot(states);
    const int64_t released = (tp.release && nt > 0) ? grid::time_release_window(pp, nx, nz, oa, ob, poa, pob, id.data(), tracks.data(), nt, flags.data(), f2.data()) : 0;
    if (released > 0) grid::dist_window(reach, nx, nz, cls.data(), table.data(), f2.data(), gcol.data(), nullptr, rcost.data());
    (void)grid::plan_window(pl, nx, nz, oa, ob, rcost.data(), goals.data(), n, rpot.data(), rdir.data());
    for (size_t i = 0; i < cells; i++) price[i] = grid::price_of(pl, rcost[i]);
    int64_t stats[grid::TM_WORDS] = {0, 0, 0, 0, 0, 0};
    grid::time_window(pl, tp, pp, nx, nz, oa, ob, price.data(), rpot.data(), rdir.data(), pred.data(), poa, pob, tpot.data(), tdir.data(), stats);
    int64_t status = grid::PATH_OUTSIDE, len = 0;
    const int32_t a = h[19], b = h[20];
    std::vector<int32_t> path(3 * ((size_t)tp.layers + cells));
    if (a >= 0 && a < nx && b >= 0 && b < nz) {
        const size_t i = (size_t)b * (size_t)nx + (size_t)a;
        const grid::TimeBlock B{pred.data(), nx, nz, oa, ob, poa, pob};
        status = grid::time_start_status(price[i], B(a, b), tpot[i]);
        if (status == grid::PATH_FOUND) {
            len = grid::time_walk(nx, nz, oa, ob, tp.layers, tdir.data(), rdir.data(), a, b, path.data(), (int64_t)(path.size() / 3));
            // the walk with no room writes nothing and counts the same
            if (grid::time_walk(nx, nz, oa, ob, tp.layers, tdir.data(), rdir.data(), a, b, nullptr, 0) != len) return 1;
            if (len == 0) status = grid::PATH_UNREACHABLE;
        }
    }
    fwrite(&released, 8, 1, stdout);
    fwrite(rcost.data(), 1, cells, stdout);
    fwrite(rpot.data(), 4, cells, stdout);
    fwrite(rdir.data(), 1, cells, stdout);
    fwrite(tpot.data(), 4, states, stdout);
    fwrite(tdir.data(), 1, states, stdout);
    fwrite(stats, 8, 4, stdout);
    fwrite(&status, 8, 1, stdout);
    fwrite(&len, 8, 1, stdout);
    fwrite(path.data(), 4, 3 * (size_t)len, stdout);
    return 0;
}

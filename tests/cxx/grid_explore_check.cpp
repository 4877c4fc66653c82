// The exploration layer of stereo-vision_amd/csrc/grid_explore_core.h -- the rays at the window's edges, the square of marks of
// gain_window, the VIEW plane, the ranking with its int64 scores -- compiled by the host compiler alone, as a program of its own:
// tests/test_grid_explore.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane at the
// window's edge or a signed overflow ends the run, and compares what it writes with tests/grid_explore_ref.py.
//
//   grid_explore_check job.bin
//   job.bin: int32 nx, nz, oa, ob; max_cell_cost, min_size, unexplored, border; neutral, unknown, max_cost; min_gain, w_gain, w_reach;
//            view_ga, view_gb, start_ga, start_gb, n_cells; float range, cell; then STATE and COST (nx * nz bytes each) and the
//            viewpoints (2 * n_cells int32)
//   stdout:  GAIN (n_cells int32); VIEW of the view cell (nx * nz bytes; nothing when it is outside the window); int64 n, best,
//            feasible; the records (5 int32 each, n of them); the scores (n int64).
//            Exit status 3: the parameters are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_explore_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[19];
    float fl[2];
    if (fread(head, 4, 19, f) != 19 || fread(fl, 4, 2, f) != 2) return 2;
    const int32_t nx = head[0], nz = head[1], oa = head[2], ob = head[3], n_cells = head[18];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || n_cells < 0) return 2;
    const grid::FrontParams fp{head[4], head[5], (uint32_t)head[6], head[7]};
    const grid::PlanParams pp{head[8], head[9], head[10]};
    const grid::ExploreParams ep{fl[0], head[11], head[12], head[13]};
    const size_t cells = (size_t)nx * (size_t)nz;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<uint8_t> state(cells), cost(cells);
    std::vector<int32_t> view_cells(2 * (size_t)n_cells);
    if (fread(state.data(), 1, cells, f) != cells || fread(cost.data(), 1, cells, f) != cells ||
        fread(view_cells.data(), 4, view_cells.size(), f) != view_cells.size())
        return 2;
    fclose(f);
    const int32_t R = (grid::front_ok(fp) && grid::plan_ok(pp) && grid::explore_ok(ep) && grid::finite_f(fl[1]) && fl[1] > 0.f) ? grid::explore_range(ep.range, fl[1]) : 0;
    if (!R) return 3;
    std::vector<int32_t> gains((size_t)n_cells);
    grid::gain_window(fp, R, nx, nz, oa, ob, state.data(), view_cells.data(), n_cells, gains.data());
    if (!gains.empty()) fwrite(gains.data(), 4, gains.size(), stdout);
    const int64_t va = (int64_t)head[14] - oa, vb = (int64_t)head[15] - ob;
    if (va >= 0 && va < nx && vb >= 0 && vb < nz) {
        std::vector<uint8_t> view(cells);
        const int32_t own[2] = {head[14], head[15]};
        int32_t again = -2;
        const int32_t gain = grid::view_window(fp, R, nx, nz, state.data(), (int32_t)va, (int32_t)vb, view.data());
        grid::gain_window(fp, R, nx, nz, oa, ob, state.data(), own, 1, &again);
        if (gain != again) return 1;                   // the two host forms count the same set
        fwrite(view.data(), 1, cells, stdout);
    }
    std::vector<int32_t> recs;
    std::vector<int64_t> scores;
    int64_t out[3] = {0, 0, 0};
    out[1] = grid::explore_window(fp, pp, ep, R, nx, nz, oa, ob, state.data(), cost.data(), head[16], head[17], &recs, &scores, &out[2]);
    out[0] = (int64_t)scores.size();
    if (recs.size() != scores.size() * grid::EXPLORE_REC) return 1;
    fwrite(out, 8, 3, stdout);
    if (!scores.empty()) {   // an empty vector has no array to write from
        fwrite(recs.data(), 4, recs.size(), stdout);
        fwrite(scores.data(), 8, scores.size(), stdout);
    }
    return 0;
}

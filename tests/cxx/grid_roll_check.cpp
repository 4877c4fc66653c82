// The rollouts of stereo-vision_amd/csrc/grid_roll_core.h -- the footprint table in double, the footprint cost at the window's edges,
// the cut, the int64 score and the best -- compiled by the host compiler alone, as a program of its own: tests/test_grid_roll.py builds
// it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane, a list or the table, or a signed overflow,
// ends the run, and compares what it writes with tests/grid_roll_ref.py.
//
//   grid_roll_check job.bin
//   job.bin: int32 nx, nz, oa, ob, headings_m, stop_cost, unknown_cost, w_pot, w_cost, w_cut, S, K, T, set, ga0, gb0, n_poses, has_pot;
//            float cell, front, rear, half_width; COST (nx * nz bytes); POT (nx * nz int32, if has_pot); the table (S * K * T * 3
//            int32, if S > 0); the poses (n_poses * 3 int32)
//   stdout:  int32 R; per heading int64 n and the n pairs (da, db); F (n_poses int32); if S > 0 the records (5 K int32), the scores
//            (K int64) and int32 best.  Exit status 3: the parameters or the table are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_roll_core.h"

using namespace svh;

template <class V>
static bool take(FILE* f, std::vector<V>& v) {
    return v.empty() || fread(v.data(), sizeof(V), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[18];
    float len[4];
    if (fread(head, 4, 18, f) != 18 || fread(len, 4, 4, f) != 4) return 2;
    const int32_t nx = head[0], nz = head[1], oa = head[2], ob = head[3], S = head[10], K = head[11], T = head[12], set = head[13];
    const int32_t ga0 = head[14], gb0 = head[15], n_poses = head[16], has_pot = head[17];
    if (nx < 1 || nx > grid::MAX_SIDE || nz < 1 || nz > grid::MAX_SIDE || !grid::offsets_ok(oa, ob) || n_poses < 0 || S < 0) return 2;
    const grid::RollParams p{len[1], len[2], len[3], head[4], head[5], head[6], head[7], head[8], head[9]};
    if (!grid::roll_ok(p)) return 3;
    if (S > 0 && (K < 1 || T < 1 || T > grid::ROLL_MAX_T || K > grid::ROLL_MAX_K || (int64_t)S * K * T > grid::ROLL_MAX_TABLE || set < 0 || set >= S)) return 3;
    if (p.w_pot != 0 && !has_pot) return 2;
    const size_t cells = (size_t)nx * (size_t)nz;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<uint8_t> cost(cells);
    std::vector<int32_t> pot(has_pot ? cells : 0), table(S > 0 ? (size_t)S * K * T * 3 : 0), poses((size_t)n_poses * 3);
    if (!take(f, cost) || !take(f, pot) || !take(f, table) || !take(f, poses)) return 2;
    fclose(f);
    if (S > 0 && !grid::roll_table_ok(table.data(), S, K, T, 8 * p.m)) return 3;
    std::vector<int32_t> offs;
    std::vector<int64_t> start;
    const int32_t R = grid::roll_table(p, len[0], &offs, &start);
    if (R == 0) return 3;
    fwrite(&R, 4, 1, stdout);
    for (int32_t k = 0; k < 8 * p.m; k++) {
        const int64_t n = start[k + 1] - start[k];
        fwrite(&n, 8, 1, stdout);
        fwrite(offs.data() + 2 * start[k], 4, (size_t)n * 2, stdout);
    }
    std::vector<int32_t> fout((size_t)n_poses);
    grid::footprint_window(p, nx, nz, oa, ob, cost.data(), offs.data(), start.data(), poses.data(), n_poses, fout.data());
    fwrite(fout.data(), 4, fout.size(), stdout);
    if (S > 0) {
        std::vector<int32_t> recs((size_t)K * grid::ROLL_REC);
        std::vector<int64_t> scores((size_t)K);
        const int32_t best = grid::roll_window(p, nx, nz, oa, ob, cost.data(), has_pot ? pot.data() : nullptr, offs.data(), start.data(),
                                               table.data() + (size_t)set * K * T * 3, K, T, ga0, gb0, recs.data(), scores.data());
        fwrite(recs.data(), 4, recs.size(), stdout);
        fwrite(scores.data(), 8, scores.size(), stdout);
        fwrite(&best, 4, 1, stdout);
    }
    return 0;
}

// The prediction of stereo-vision_amd/csrc/grid_pred_core.h -- the displacements in 64 bits, the radii, PRED with its separable
// inflation, the slot of a pose, the scoring with the object cut -- compiled by the host compiler alone, as a program of its own:
// tests/test_grid_pred.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane, a shift by
// 32 or a signed overflow ends the run.
//
//   grid_pred_check extremes     drives the header where its integers are largest: |v16| at its largest times 31 * 64 (the 64-bit
//                                path), 4096 tracks, radius 16 on a frame of 1 x 1, 32 slots.  Prints "extremes ok"; exit status 1 with
//                                the line of the first value that is not the one worked out here.
//   grid_pred_check plane job.bin
//     job.bin: int32 slots, stride, poses_per_step, margin, grow16, only_moving, nx, nz, n_tracks; the ID plane (nx * nz int32); the
//              track records (14 int32 each)
//     stdout:  one line: the three statistics, then the words of PRED
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "grid_pred_core.h"

using namespace svh;
using namespace svh::grid;

#define EXPECT(cond)                                        \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("line %d: %s\n", __LINE__, #cond);       \
            return 1;                                       \
        }                                                   \
    } while (0)

static void track(int32_t* t, int32_t id, int32_t va, int32_t vb, int32_t flags = TK_MOVING, int32_t label = 0) {
    memset(t, 0, TRACK_REC * sizeof(int32_t));
    t[TR_ID] = id, t[TR_FLAGS] = flags, t[TR_LABEL] = label, t[TR_V16_A] = va, t[TR_V16_B] = vb;
}

static int extremes() {
    const PredParams wide{32, 64, 1024, 16, 256, 0};
    EXPECT(pred_ok(wide));
    // the largest product: 2^31 * 31 * 64 = 2^42 * 0.97: the quotient by 16 lies far beyond every frame and is clamped
    const int32_t vmax = 0x7FFFFFFF, vmin = (int32_t)0x80000000;
    EXPECT(pred_disp(wide, vmax, 31) == (int32_t)PRED_FAR && pred_disp(wide, vmin, 31) == -(int32_t)PRED_FAR);
    EXPECT(pred_disp(wide, vmax, 0) == 0 && pred_disp(wide, vmin, 0) == 0);
    EXPECT(rdiv64((int64_t)vmax * 31 * 64, 16) == ((int64_t)vmax * 31 * 64 + 8) / 16);
    EXPECT(rdiv64((int64_t)vmin * 31 * 64, 16) == (int64_t)vmin * 31 * 4);   // exact: a multiple of 16
    const PredParams one{8, 1, 1, 0, 0, 1};
    EXPECT(pred_disp(one, 8, 1) == 1 && pred_disp(one, -8, 1) == 0 && pred_disp(one, 7, 1) == 0 && pred_disp(one, -9, 1) == -1);
    EXPECT(pred_disp(one, 24, 1) == 2 && pred_disp(one, -24, 1) == -1);
    // radii and their masks
    EXPECT(pred_radius(wide, 0) == 16 && pred_radius(wide, 31) == 16 && pred_ge(wide, 16) == 0xFFFFFFFFu && pred_all(wide) == 0xFFFFFFFFu);
    const PredParams grow{8, 1, 1, 1, 8, 1};
    EXPECT(pred_radius(grow, 0) == 1 && pred_radius(grow, 1) == 1 && pred_radius(grow, 2) == 2 && pred_radius(grow, 7) == 4);
    EXPECT(pred_ge(grow, 0) == 0xFFu && pred_ge(grow, 1) == 0xFFu && pred_ge(grow, 2) == 0xFCu && pred_ge(grow, 5) == 0u && pred_all(grow) == 0xFFu);
    // the slots of the poses at the largest divisor and at the smallest
    EXPECT(pred_slot(wide, 0) == 0 && pred_slot(wide, 1023) == 0);            // rdiv(1024, 65536) = 0
    EXPECT(pred_slot(one, 0) == 1 && pred_slot(one, 5) == 6 && pred_slot(one, 6) == 7 && pred_slot(one, 1023) == 7);
    // radius 16 on a frame of one cell, all 32 slots, the fastest track there can be: slot 0 alone stays in the frame
    {
        int32_t id = 5, t[TRACK_REC];
        uint32_t pred = 0xDEADBEEFu;
        int64_t st[PS_WORDS];
        track(t, 5, vmax, vmin);
        pred_window(wide, 1, 1, &id, t, 1, &pred, st);
        EXPECT(pred == 1u && st[PS_TRACKS] == 1 && st[PS_SOURCES] == 1 && st[PS_CELLS] == 1);
        track(t, 5, 0, 0);
        pred_window(wide, 1, 1, &id, t, 1, &pred, st);
        EXPECT(pred == 0xFFFFFFFFu);
        pred_window(wide, 1, 1, nullptr, t, 1, &pred, st);
        EXPECT(pred == 0u && st[PS_SOURCES] == 0);
        EXPECT(pred_at(&pred, 1, 1, OFFSET_LIMIT, -OFFSET_LIMIT, (int64_t)OFFSET_LIMIT + 1, -OFFSET_LIMIT) == 0u);
    }
    // 4096 tracks of one cell each on 128 x 128 cells (every second id: the ids are not contiguous), standing still, radius 0 and 16
    {
        const int32_t nx = 128, nz = 128, n = OBJ_MAX_TRACKS;
        std::vector<int32_t> id((size_t)nx * nz, -1), tracks((size_t)n * TRACK_REC);
        for (int32_t k = 0; k < n; k++) {
            track(tracks.data() + (size_t)k * TRACK_REC, 2 * k + 1, (k & 1) ? vmax : 0, 0, (k % 3) ? (int32_t)TK_MOVING : 0, k);
            id[(size_t)(2 * (k / 64)) * nx + (size_t)(2 * (k % 64))] = 2 * k + 1;
        }
        std::vector<uint32_t> pred((size_t)nx * nz);
        int64_t st[PS_WORDS];
        PredParams p{32, 64, 1, 0, 0, 1};
        pred_window(p, nx, nz, id.data(), tracks.data(), n, pred.data(), st);
        EXPECT(st[PS_TRACKS] == n - (n + 2) / 3 && st[PS_SOURCES] == st[PS_TRACKS] && st[PS_CELLS] == st[PS_TRACKS]);
        EXPECT(pred[0] == 0u && pred[2] == 1u && pred[4] == 0xFFFFFFFFu);    // k = 0 does not move; k = 1 leaves at once; k = 2 stands
        p.margin = 16, p.only_moving = 0;
        pred_window(p, nx, nz, id.data(), tracks.data(), n, pred.data(), st);
        EXPECT(st[PS_TRACKS] == n && st[PS_SOURCES] == n && st[PS_CELLS] == (int64_t)nx * nz && pred[(size_t)nx * nz - 1] == 0xFFFFFFFFu);
    }
    // the scoring at the ends: a point vehicle, T = 1024, an object at the last pose's cell in the last slot
    {
        RollParams rp{0.f, 0.f, 0.f, 1, 253, 254, 0, 1, 1};
        std::vector<int32_t> offs;
        std::vector<int64_t> start;
        EXPECT(roll_table(rp, 1.f, &offs, &start) == 1);
        const int32_t nx = 1024, nz = 1, T = ROLL_MAX_T;
        std::vector<uint8_t> cost((size_t)nx, 0);
        std::vector<uint32_t> pred((size_t)nx, 0u);
        std::vector<int32_t> cand((size_t)T * 3);
        for (int32_t t = 0; t < T; t++) cand[3 * t] = t, cand[3 * t + 1] = 0, cand[3 * t + 2] = 0;
        const PredParams pp{32, 1, 1, 0, 0, 0};
        int32_t rec[ROLL_PRED_REC];
        int64_t score;
        pred[1023] = 0x80000000u;
        int32_t best = roll_pred_window(rp, pp, nx, nz, 0, 0, cost.data(), nullptr, nx, nz, 0, 0, pred.data(), offs.data(), start.data(), cand.data(), 1, T,
                                        0, 0, rec, &score);
        EXPECT(best == 0 && rec[RR_LEN] == 1023 && rec[RR_STATUS] == ROLL_CUT_OBJECT && rec[RR_SLOT] == 31 && score == 1);
        pred[1023] = 0x7FFFFFFFu;                                             // every slot but the pose's
        best = roll_pred_window(rp, pp, nx, nz, 0, 0, cost.data(), nullptr, nx, nz, 0, 0, pred.data(), offs.data(), start.data(), cand.data(), 1, T, 0, 0,
                                rec, &score);
        EXPECT(best == 0 && rec[RR_LEN] == 1024 && rec[RR_STATUS] == ROLL_COMPLETE && rec[RR_SLOT] == -1 && score == 0);
        // the frame elsewhere: nothing is read outside it
        best = roll_pred_window(rp, pp, nx, nz, 0, 0, cost.data(), nullptr, nx, nz, OFFSET_LIMIT, -OFFSET_LIMIT, pred.data(), offs.data(), start.data(),
                                cand.data(), 1, T, 0, 0, nullptr, nullptr);
        EXPECT(best == 0);
    }
    printf("extremes ok\n");
    return 0;
}

static int plane(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    int32_t head[9];
    if (fread(head, sizeof(int32_t), 9, f) != 9) return 2;
    const PredParams p{head[0], head[1], head[2], head[3], head[4], head[5]};
    const int32_t nx = head[6], nz = head[7], n = head[8];
    if (!pred_ok(p) || nx < 1 || nz < 1 || n < 0) return 2;
    const size_t cells = (size_t)nx * (size_t)nz;
    std::vector<int32_t> id(cells), tracks((size_t)n * TRACK_REC + 1);
    if (fread(id.data(), sizeof(int32_t), cells, f) != cells || fread(tracks.data(), sizeof(int32_t), (size_t)n * TRACK_REC, f) != (size_t)n * TRACK_REC) return 2;
    fclose(f);
    std::vector<uint32_t> pred(cells);
    int64_t st[PS_WORDS];
    pred_window(p, nx, nz, id.data(), tracks.data(), n, pred.data(), st);
    printf("%lld %lld %lld", (long long)st[PS_TRACKS], (long long)st[PS_SOURCES], (long long)st[PS_CELLS]);
    for (size_t i = 0; i < cells; i++) printf(" %u", pred[i]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "extremes")) return extremes();
    if (argc == 3 && !strcmp(argv[1], "plane")) return plane(argv[2]);
    fprintf(stderr, "usage: grid_pred_check extremes | plane job.bin\n");
    return 2;
}

// The objects and tracks of stereo-vision_amd/csrc/grid_obj_core.h -- the flood fill, the centroid in int64, the claims, the gate's
// distances, the update -- compiled by the host compiler alone, as a program of its own: tests/test_grid_obj.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane or a signed overflow ends the run.
//
//   grid_obj_check extremes      drives the header where its integers are largest: coordinates at +-2^20 cells, a size of 2^26, sums
//                                near 2^40, velocities and misses at their bounds.  Prints "extremes ok"; exit status 1 with the line
//                                of the first value that is not the one worked out here.
//   grid_obj_check history job.bin
//     job.bin: int32 nx, nz, frames, min_size, max_size, max_tracks, min_overlap, gate, max_missed, min_age, move_cells, smooth_shift;
//              float min_height; then per frame int32 oa, ob, STATE (nx * nz bytes), HMAX (float), COUNT (int32)
//     stdout:  per frame three lines of integers: the number of object records and the records; the number of track records and
//              the records; ASSIGN and then the sum of the ID plane
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "grid_obj_core.h"

using namespace svh;
using namespace svh::grid;

#define EXPECT(cond)                                        \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("line %d: %s\n", __LINE__, #cond);       \
            return 1;                                       \
        }                                                   \
    } while (0)

static const ObjParams kWide{1, OBJ_MAX_SIZE, 0.f, OBJ_MAX_TRACKS, 1, OBJ_MAX_GATE, OBJ_MAX_MISSED, 0, OBJ_MAX_MOVE, OBJ_MAX_SHIFT};

static int extremes() {
    // the centroid of the largest component there can be: 2^26 cells whose coordinates are all 8191 (more than any real one sums to)
    const int64_t size = (int64_t)OBJ_MAX_SIZE, sum = size * 8191;             // 2^39 and a bit
    EXPECT(obj_c16(sum, size) == 16 * 8191 + 8);
    EXPECT(obj_c16(0, size) == 8 && obj_c16(0, 1) == 8 && obj_c16(1, 2) == 16 && obj_c16(1, 3) == 13);
    EXPECT(obj_points(((int64_t)1 << 57)) == 0x7FFFFFFF && obj_points(0x7FFFFFFF) == 0x7FFFFFFF && obj_points(0x7FFFFFFE) == 0x7FFFFFFE);
    EXPECT(obj_verdict(kWide, OBJ_MAX_SIZE, (int32_t)bits_of(0.25f)) == OF_KEPT);
    ObjParams p = kWide;
    p.max_size = OBJ_MAX_SIZE - 1, p.min_height = 0.25f;
    EXPECT(obj_verdict(p, OBJ_MAX_SIZE, 0) == OF_LARGE && obj_verdict(p, 5, (int32_t)bits_of(0.25f)) == OF_KEPT);
    EXPECT(obj_verdict(p, 5, (int32_t)bits_of(0.25f) - 1) == OF_OBJECT && obj_verdict(p, 5, (int32_t)NAN_BITS) == OF_OBJECT);
    EXPECT(obj_verdict(p, 5, (int32_t)0x80000000) == OF_OBJECT);
    EXPECT(obj_claim_index(obj_claim_key(OBJ_MAX_SIZE, 0)) == 0 && obj_claim_index(obj_claim_key(1, 0x7FFFFFFF)) == 0x7FFFFFFF);
    EXPECT(obj_claim_key(2, 4095) > obj_claim_key(1, 0) && obj_claim_key(2, 3) > obj_claim_key(2, 4) && obj_claim_overlap(obj_claim_key(OBJ_MAX_SIZE, 7)) == OBJ_MAX_SIZE);

    // a whole row of the widest window at both ends of the offsets: one component of 8192 cells; then 64 such rows
    for (const int32_t off : {-OFFSET_LIMIT, OFFSET_LIMIT}) {
        for (const int32_t nz : {1, 64}) {
            const int32_t nx = MAX_SIDE;
            const size_t cells = (size_t)nx * (size_t)nz;
            std::vector<uint8_t> state(cells, (uint8_t)C_OBSTACLE), flags(cells);
            std::vector<float> hmax(cells, 1.5f);
            std::vector<int32_t> count(cells, 0x7FFFFFFF), label(cells), recs;
            int64_t st[OS_WORDS];
            obj_window(kWide, nx, nz, off, -off, state.data(), hmax.data(), count.data(), flags.data(), label.data(), &recs, st);
            EXPECT(st[OS_KEPT] == 1 && st[OS_KEPT_CELLS] == (int64_t)cells && recs.size() == (size_t)OBJ_REC);
            EXPECT(recs[OR_GA_MIN] == off && recs[OR_GA_MAX] == off + nx - 1 && recs[OR_GB_MIN] == -off && recs[OR_GB_MAX] == -off + nz - 1);
            EXPECT(recs[OR_C16_A] == 16 * off + 16 * 4096 && recs[OR_C16_B] == -16 * off + 8 * nz);   // the middle of 0 .. n - 1, plus one half
            EXPECT(recs[OR_POINTS] == 0x7FFFFFFF && recs[OR_HMAX_BITS] == (int32_t)bits_of(1.5f) && flags[cells - 1] == (OF_OBJECT | OF_KEPT));
            // a step onto itself, and onto the ID plane of a window at the far end of the world
            std::vector<int32_t> tracks, tracks2, assign(1), id(cells), id2(cells);
            int64_t ts[TS_WORDS];
            int32_t next = obj_step(kWide, nx, nz, off, -off, recs.data(), 1, label.data(), 0, 0, nullptr, nullptr, 0, 0x7FFFFFFE, &tracks, assign.data(),
                                    id.data(), ts);
            EXPECT(next == 0x7FFFFFFF && assign[0] == 0x7FFFFFFE && ts[TS_NEW] == 1 && id[cells - 1] == 0x7FFFFFFE);
            next = obj_step(kWide, nx, nz, off, -off, recs.data(), 1, label.data(), off, -off, id.data(), tracks.data(), 1, next, &tracks2, assign.data(),
                            id2.data(), ts);
            EXPECT(ts[TS_BY_OVERLAP] == 1 && tracks2[TR_OVERLAP] == (int32_t)cells && tracks2[TR_AGE] == 1 && tracks2[TR_V16_A] == 0);
            ObjParams blind = kWide;                                        // without the gate, which would find the track where it stands
            blind.gate = 0;
            next = obj_step(blind, nx, nz, off, -off, recs.data(), 1, label.data(), -off, off, id.data(), tracks.data(), 1, next, &tracks2, assign.data(),
                            id2.data(), ts);
            EXPECT(ts[TS_MISSED] == 1 && ts[TS_UNTRACKED] == 1 && assign[0] == ASSIGN_UNTRACKED && next == 0x7FFFFFFF);   // no id is left
        }
    }

    // a track that crosses the world in one match, and the smoothing of the largest difference
    int32_t before[TRACK_REC] = {0}, after[TRACK_REC], obj[OBJ_REC] = {0};
    const int32_t far = 16 * ((1 << 20) - 1) + 15;                             // the last sixteenth of the last cell
    before[TR_C16_A] = -far - 1, before[TR_C16_B] = far, before[TR_BIRTH_A] = -far - 1, before[TR_BIRTH_B] = far;
    obj[OR_C16_A] = far, obj[OR_C16_B] = -far - 1, obj[OR_SIZE] = OBJ_MAX_SIZE;
    track_match(kWide, before, obj, TK_BY_GATE, 0, 0, after);
    EXPECT(after[TR_V16_A] == 2 * far + 1 && after[TR_V16_B] == -2 * far - 1 && after[TR_AGE] == 1 && (after[TR_FLAGS] & TK_MOVING));
    before[TR_AGE] = 0x7FFFFFFF, before[TR_V16_A] = -2 * far - 1, before[TR_V16_B] = 2 * far + 1, before[TR_MISSED] = 0;
    track_match(kWide, before, obj, TK_BY_OVERLAP, 5, TK_SPLIT, after);
    EXPECT(after[TR_AGE] == 0x7FFFFFFF && after[TR_V16_A] == -2 * far - 1 + rdiv(4 * far + 2, 16) && after[TR_V16_B] == 2 * far + 1 + rdiv(-4 * far - 2, 16));
    before[TR_MISSED] = OBJ_MAX_MISSED;
    track_match(kWide, before, obj, TK_BY_GATE, 0, 0, after);
    EXPECT(after[TR_MISSED] == 0);
    EXPECT(!track_miss(kWide, before, 0, after) && after[TR_MISSED] == OBJ_MAX_MISSED + 1 && after[TR_LABEL] == -1);
    // the gate at its widest against a prediction far outside the world: no overflow, no match; and one that lands on the object
    before[TR_C16_A] = far, before[TR_C16_B] = far, before[TR_V16_A] = 2 * far + 1, before[TR_V16_B] = -2 * far - 1, before[TR_MISSED] = OBJ_MAX_MISSED;
    EXPECT(obj_gate_key(kWide, before, obj, 9) == GATE_NONE);
    before[TR_MISSED] = 1, before[TR_V16_A] = 0, before[TR_V16_B] = -far;      // far - 2 far = -far, one sixteenth from the object
    EXPECT(obj_gate_key(kWide, before, obj, 9) == (((uint64_t)1 << 32) | 9u));
    before[TR_V16_A] = -16 * OBJ_MAX_GATE / 2, before[TR_V16_B] = -far - 1 + 16 * OBJ_MAX_GATE / 2;   // (-1024, +1023): beyond; (-1024, 0): at the bound
    EXPECT(obj_gate_key(kWide, before, obj, 0) == GATE_NONE);
    before[TR_V16_B] = -far;
    before[TR_C16_B] = far - 1;
    EXPECT(obj_gate_key(kWide, before, obj, 3) == ((((uint64_t)1024 * 1024) << 32) | 3u));
    EXPECT(track_room(kWide, 4095, 0) == 1 && track_room(kWide, 4096, 0) == 0 && track_room(kWide, 0, 0x7FFFFFFF) == 0 && track_room(kWide, 0, 0x7FFFFFF0) == 15);
    EXPECT(cell_of_c16(-1) == -1 && cell_of_c16(-16) == -1 && cell_of_c16(-17) == -2 && cell_of_c16(15) == 0 && cell_of_c16((int64_t)far + 8 * (2 * (int64_t)far + 1)) == 17825791);
    uint8_t rgb[3];
    colour_track(0x7FFFFFFF, true, rgb);
    printf("extremes ok\n");
    return 0;
}

static int history(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    int32_t head[12];
    float min_height;
    if (fread(head, 4, 12, f) != 12 || fread(&min_height, 4, 1, f) != 1) return 2;
    const int32_t nx = head[0], nz = head[1], frames = head[2];
    const ObjParams p{head[3], head[4], min_height, head[5], head[6], head[7], head[8], head[9], head[10], head[11]};
    if (nx < 1 || nx > MAX_SIDE || nz < 1 || nz > MAX_SIDE || !obj_ok(p)) return 3;
    const size_t cells = (size_t)nx * (size_t)nz;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<int32_t> tracks, prev_id;
    int32_t poa = 0, pob = 0, next = 0;
    for (int32_t k = 0; k < frames; k++) {
        int32_t off[2];
        std::vector<uint8_t> state(cells), flags(cells);
        std::vector<float> hmax(cells);
        std::vector<int32_t> count(cells), label(cells), recs, id(cells), now;
        if (fread(off, 4, 2, f) != 2 || fread(state.data(), 1, cells, f) != cells || fread(hmax.data(), 4, cells, f) != cells ||
            fread(count.data(), 4, cells, f) != cells)
            return 2;
        if (!offsets_ok(off[0], off[1])) return 3;
        int64_t st[OS_WORDS], ts[TS_WORDS];
        obj_window(p, nx, nz, off[0], off[1], state.data(), hmax.data(), count.data(), flags.data(), label.data(), &recs, st);
        const int32_t n_obj = (int32_t)(recs.size() / OBJ_REC);
        std::vector<int32_t> assign((size_t)n_obj);
        next = obj_step(p, nx, nz, off[0], off[1], recs.data(), n_obj, label.data(), poa, pob, prev_id.empty() ? nullptr : prev_id.data(),
                        tracks.data(), prev_id.empty() ? 0 : (int32_t)(tracks.size() / TRACK_REC), next, &now, assign.data(), id.data(), ts);
        tracks.swap(now), prev_id.swap(id), poa = off[0], pob = off[1];
        printf("%d", n_obj);
        for (const int32_t v : recs) printf(" %d", v);
        printf("\n%d", (int32_t)(tracks.size() / TRACK_REC));
        for (const int32_t v : tracks) printf(" %d", v);
        printf("\n");
        for (const int32_t v : assign) printf("%d ", v);
        int64_t sum = 0;
        for (const int32_t v : prev_id) sum += v;
        printf("%lld\n", (long long)sum);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "extremes")) return extremes();
    if (argc == 3 && !strcmp(argv[1], "history")) return history(argv[2]);
    return 2;
}

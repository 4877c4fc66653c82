/* The rollout part of include/svh_grid.h is plain C: compiled by tests/test_grid_roll.py with -std=c99 -pedantic -Wall -Werror and
 * only include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_roll_params p;
    const double xyz[3] = {0.0, 0.0, 1.0};
    int32_t recs[SVH_GRID_ROLL_RECORD], k = -7, best = -7, R = -7, pose[3] = {0, 0, 0}, table[3] = {0, 0, 0};
    int64_t score = -7, n = -7;
    uint8_t px[3];
    svh_grid_roll_params_default(&p);
    svh_grid_roll_params_default(NULL);
    if (p.front != 3.5f || p.rear != 1.0f || p.half_width != 0.9f || p.headings_m != 8 || p.stop_cost != 253 || p.unknown_cost != 254) return 1;
    if (p.w_pot != 1 || p.w_cost != 1 || p.w_cut != 0) return 1;
    if (svh_grid_set_roll(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_roll(NULL, &p, &R, &n) != SVH_ERR_BAD_ARG || R != -7) return 2;
    if (svh_grid_heading_of(NULL, xyz, &k) != SVH_ERR_BAD_ARG || k != -7) return 3;
    if (svh_grid_roll_footprint(NULL, 0, recs, 1, &n) != SVH_ERR_BAD_ARG || n != -7) return 4;
    if (svh_grid_footprint_cost(NULL, pose, 1, 0, recs) != SVH_ERR_BAD_ARG) return 5;
    if (svh_grid_roll_set_candidates(NULL, table, 1, 1, 1) != SVH_ERR_BAD_ARG) return 6;
    if (svh_grid_roll_get_candidates(NULL, pose) != SVH_ERR_BAD_ARG || pose[0] != 0) return 6;
    if (svh_grid_roll_score(NULL, xyz, 0, recs, &score, 0, &best) != SVH_ERR_BAD_ARG || best != -7 || score != -7) return 7;
    if (svh_grid_render_roll(NULL, px, 0) != SVH_ERR_BAD_ARG) return 8;
    printf("svh_grid.h: rollouts C99 ok, records of %d, statuses %d..%d\n", SVH_GRID_ROLL_RECORD, SVH_GRID_ROLL_COMPLETE, SVH_GRID_ROLL_EMPTY);
    return 0;
}

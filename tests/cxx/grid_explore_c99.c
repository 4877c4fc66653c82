/* The exploration part of include/svh_grid.h is plain C: compiled by tests/test_grid_explore.py with -std=c99 -pedantic -Wall
 * -Werror and only include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_explore_params p;
    const double start[3] = {0.0, 0.0, 0.0};
    int64_t st[4], n = -1;
    int32_t recs[SVH_GRID_EXPLORE_RECORD], cells[2] = {0, 0}, gain = -7, best = -7, R = -7;
    uint8_t px[3];
    svh_grid_explore_params_default(&p);
    svh_grid_explore_params_default(NULL);
    if (p.range != 10.0f || p.min_gain != 1 || p.w_gain != 500 || p.w_reach != 1) return 1;
    if (svh_grid_set_explore(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_explore(NULL, &p, &R) != SVH_ERR_BAD_ARG || R != -7) return 2;
    if (svh_grid_view_gain(NULL, cells, 1, 0, &gain) != SVH_ERR_BAD_ARG || gain != -7) return 3;
    if (svh_grid_view_mask(NULL, 0, 0, px, 0) != SVH_ERR_BAD_ARG) return 4;
    if (svh_grid_explore_rank(NULL, start, recs, NULL, 1, &n, &best) != SVH_ERR_BAD_ARG || n != -1 || best != -7) return 5;
    if (svh_grid_plan_set_goal_explore(NULL, start) != SVH_ERR_BAD_ARG) return 6;
    if (svh_grid_get_explore_stats(NULL, st) != SVH_ERR_BAD_ARG) return 7;
    if (svh_grid_render_view(NULL, 0, 0, px, 0) != SVH_ERR_BAD_ARG) return 8;
    printf("svh_grid.h: exploration C99 ok, view bytes %d..%d, records of %d\n", SVH_GRID_VIEW_NONE, SVH_GRID_VIEW_COUNTED, SVH_GRID_EXPLORE_RECORD);
    return 0;
}

/* The frontier part of include/svh_grid.h is plain C: compiled by tests/test_grid_front.py with -std=c99 -pedantic -Wall
 * -Werror and only include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_front_params p;
    int64_t st[5], n = -1;
    int32_t recs[SVH_GRID_FRONT_RECORD];
    uint8_t px[3];
    svh_grid_front_params_default(&p);
    svh_grid_front_params_default(NULL);
    if (p.max_cell_cost != 252 || p.min_size != 8 || p.unexplored != SVH_GRID_LETHAL_UNSEEN || p.border != 0) return 1;
    if (svh_grid_set_frontier(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_frontier(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_get_front_plane(NULL, SVH_GRID_FRONT_LABEL, recs, 0) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_get_frontiers(NULL, recs, 1, &n) != SVH_ERR_BAD_ARG || n != -1) return 4;
    if (svh_grid_get_frontier_stats(NULL, st) != SVH_ERR_BAD_ARG) return 5;
    if (svh_grid_plan_set_goals_frontiers(NULL) != SVH_ERR_BAD_ARG) return 6;
    if (svh_grid_render_frontiers(NULL, px, 0) != SVH_ERR_BAD_ARG) return 7;
    printf("svh_grid.h: frontiers C99 ok, planes %d..%d, records of %d\n", SVH_GRID_FRONT_FLAGS, SVH_GRID_FRONT_LABEL, SVH_GRID_FRONT_RECORD);
    return 0;
}

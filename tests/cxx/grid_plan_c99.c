/* The planning part of include/svh_grid.h is plain C: compiled by tests/test_grid_plan.py with -std=c99 -pedantic -Wall
 * -Werror and only include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_plan_params p;
    int64_t st[4], len = -1;
    int32_t cells[2] = {0, 0}, cost = -1;
    double xyz[3] = {0.0, 0.0, 0.0};
    uint8_t px[3];
    svh_grid_plan_params_default(&p);
    svh_grid_plan_params_default(NULL);
    if (p.neutral != 50 || p.unknown != -1 || p.max_cost != 0x7FFFFFFE || p.max_cost + 1 != SVH_GRID_PLAN_FAR) return 1;
    if (svh_grid_set_plan(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_plan(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_plan_set_goals(NULL, cells, 1) != SVH_ERR_BAD_ARG || svh_grid_plan_set_goal(NULL, xyz) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_get_plan_plane(NULL, SVH_GRID_PLAN_POT, cells, 0) != SVH_ERR_BAD_ARG) return 4;
    if (svh_grid_get_plan_stats(NULL, st) != SVH_ERR_BAD_ARG) return 5;
    if (svh_grid_plan_path(NULL, xyz, cells, 1, &len, &cost) != SVH_ERR_BAD_ARG || len != -1 || cost != -1) return 6;
    if (svh_grid_render_plan(NULL, cells, 1, px, 0) != SVH_ERR_BAD_ARG) return 7;
    printf("svh_grid.h: planning C99 ok, planes %d..%d, statuses %d..%d\n", SVH_GRID_PLAN_POT, SVH_GRID_PLAN_DIR, SVH_GRID_PATH_FOUND,
           SVH_GRID_PATH_OUTSIDE);
    return 0;
}

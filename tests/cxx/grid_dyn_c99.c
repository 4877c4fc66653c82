/* The dynamics part of include/svh_grid.h is plain C: compiled by tests/test_grid_dyn.py with -std=c99 -pedantic -Wall -Werror and
 * only include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_dyn_params p;
    const double xyz[3] = {0.0, 0.0, 1.0};
    const float pts[4] = {0.f, 0.f, 1.f, 0.5f};
    int32_t plane[1] = {-7};
    int64_t st[4] = {-7, -7, -7, -7};
    uint8_t px[3] = {0, 0, 0};
    svh_grid_dyn_params_default(&p);
    svh_grid_dyn_params_default(NULL);
    if (p.clear_frames != 2 || p.min_through != 3 || p.margin != 0.1f || p.max_age != 0) return 1;
    if (svh_grid_set_dynamics(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_set_dynamics(NULL, NULL) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_get_dynamics(NULL, &p) != SVH_ERR_BAD_ARG || p.clear_frames != 2) return 3;
    if (svh_grid_observe_points(NULL, pts, 1, 0, xyz) != SVH_ERR_BAD_ARG) return 4;
    if (svh_grid_observe_view_lists(NULL, NULL, 0, 1, xyz) != SVH_ERR_BAD_ARG) return 5;
    if (svh_grid_get_dyn(NULL, SVH_GRID_DYN_AGE, plane, 0) != SVH_ERR_BAD_ARG || plane[0] != -7) return 6;
    if (svh_grid_get_dyn_stats(NULL, st) != SVH_ERR_BAD_ARG || st[0] != -7) return 7;
    if (svh_grid_render_dyn(NULL, px, 0) != SVH_ERR_BAD_ARG) return 8;
    printf("svh_grid.h: dynamics C99 ok, planes %d..%d\n", SVH_GRID_DYN_AGE, SVH_GRID_DYN_THROUGH);
    return 0;
}

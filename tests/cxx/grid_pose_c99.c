/* include/svh_grid_pose.h is plain C: compiled by tests/test_grid_pose.py with -std=c99 -pedantic -Wall -Werror and only
 * include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_pose_params p;
    int64_t st[4], len = -1;
    int32_t poses[3] = {0, 0, 0}, cost = -1, d = -5;
    double xyz[3] = {0.0, 0.0, 1.0};
    uint8_t px[3];
    svh_grid_pose_params_default(&p);
    svh_grid_pose_params_default(NULL);
    if (p.neutral != 50 || p.max_cost != 0x7FFFFFFE || p.turn != 100 || p.reverse != -1 || p.spin != -1) return 1;
    if (svh_grid_set_pose(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_pose(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_pose_set_goals(NULL, poses, 1) != SVH_ERR_BAD_ARG || svh_grid_pose_set_goal(NULL, xyz, -1) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_get_pose_plane(NULL, SVH_GRID_POSE_POT, poses, 0) != SVH_ERR_BAD_ARG) return 4;
    if (svh_grid_get_pose_stats(NULL, st) != SVH_ERR_BAD_ARG) return 5;
    if (svh_grid_pose_heading_of(NULL, xyz, &d) != SVH_ERR_BAD_ARG || d != -5) return 6;
    if (svh_grid_pose_path(NULL, xyz, 0, poses, 1, &len, &cost) != SVH_ERR_BAD_ARG || len != -1 || cost != -1) return 7;
    if (svh_grid_render_pose(NULL, poses, 1, px, 0) != SVH_ERR_BAD_ARG) return 8;
    printf("svh_grid_pose.h: C99 ok, planes %d..%d, statuses %d..%d\n", SVH_GRID_POSE_CF, SVH_GRID_POSE_DIR, SVH_GRID_PATH_FOUND,
           SVH_GRID_PATH_OUTSIDE);
    return 0;
}

/* The alignment part of include/svh_grid.h is plain C: compiled by tests/test_grid_align.py with -std=c99 -pedantic -Wall -Werror
 * and only include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_align_params p;
    const double pivot[3] = {0.0, 0.0, 0.0};
    const float pts[4] = {0.f, 0.f, 0.f, 0.f};
    double M[16];
    int64_t n = -1;
    int32_t rec[SVH_GRID_ALIGN_RECORD], subs[2] = {-7, -7}, vol[1] = {-7};
    uint8_t px[3] = {7, 7, 7};
    rec[0] = -7, M[0] = -7.0;
    svh_grid_align_params_default(&p);
    svh_grid_align_params_default(NULL);
    if (p.reach != 0.6f || p.range != 25.6f || p.rot_den != 256 || p.rot_n != 8 || p.trans_n != 8 || p.min_scan != 32) return 1;
    if (svh_grid_set_align(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_get_align_field(NULL, px, 0) != SVH_ERR_BAD_ARG || px[0] != 7) return 3;
    if (svh_grid_align_points(NULL, pts, 1, 0, pivot, rec) != SVH_ERR_BAD_ARG || rec[0] != -7) return 4;
    if (svh_grid_align_view_lists(NULL, NULL, 0, 1, pivot, rec) != SVH_ERR_BAD_ARG || rec[0] != -7) return 5;
    if (svh_grid_get_align_volume(NULL, vol, 0) != SVH_ERR_BAD_ARG || vol[0] != -7) return 6;
    if (svh_grid_get_align_scan(NULL, subs, 1, &n) != SVH_ERR_BAD_ARG || n != -1 || subs[0] != -7) return 7;
    if (svh_grid_align_correction(NULL, 0, 0, 0, pivot, M) != SVH_ERR_BAD_ARG || M[0] != -7.0) return 8;
    if (svh_grid_render_align(NULL, px, 0) != SVH_ERR_BAD_ARG) return 9;
    printf("svh_grid.h: alignment C99 ok, statuses %d..%d, records of %d\n", SVH_GRID_ALIGN_OK, SVH_GRID_ALIGN_FLAT, SVH_GRID_ALIGN_RECORD);
    return 0;
}

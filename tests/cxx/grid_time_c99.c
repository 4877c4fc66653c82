/* include/svh_grid_time.h is plain C: compiled by tests/test_grid_time.py with -std=c99 -pedantic -Wall -Werror and only
 * include/ on the path.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_time_params p;
    int64_t st[6], len = -1;
    int32_t triples[3] = {0, 0, 0}, cost = -1;
    double xyz[3] = {0.0, 0.0, 1.0};
    uint8_t px[3];
    svh_grid_time_params_default(&p);
    svh_grid_time_params_default(NULL);
    if (p.layers != 32 || p.wait != 100 || p.release != 1) return 1;
    if (svh_grid_set_time(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_time(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_get_time_plane(NULL, SVH_GRID_TIME_TPOT, 0, 1, triples, 0) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_get_time_stats(NULL, st) != SVH_ERR_BAD_ARG) return 4;
    if (svh_grid_time_path(NULL, xyz, triples, 1, &len, &cost) != SVH_ERR_BAD_ARG || len != -1 || cost != -1) return 5;
    if (svh_grid_render_time(NULL, 0, triples, 1, px, 0) != SVH_ERR_BAD_ARG) return 6;
    printf("svh_grid_time.h: C99 ok, planes %d..%d, wait %d, statuses %d..%d\n", SVH_GRID_TIME_TPOT, SVH_GRID_TIME_RPOT, SVH_GRID_TIME_WAIT,
           SVH_GRID_PATH_FOUND, SVH_GRID_PATH_OUTSIDE);
    return 0;
}

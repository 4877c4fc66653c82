/* include/svh_grid.h is plain C: compiled by tests/test_grid.py with -std=c99 -pedantic -Wall -Werror and only include/
 * on the path.  It needs no device: the defaults, the two frames and the argument checks. */
#include <stdio.h>

#include "svh_grid.h"

int main(void) {
    svh_grid_params p;
    svh_grid_stats st;
    double T[12], H[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, e[3] = {0.0, 0.5, 0.0}, zero[3] = {0.0, 0.0, 0.0};
    int k;
    svh_grid_params_default(&p);
    if (p.nx != 256 || p.nz != 256 || p.min_points != 3 || p.T[11] != 1.65) return 1;
    if (svh_grid_frame_plane(e, H, T) != SVH_OK || T[11] != 2.0 || T[9] != -1.0 || T[0] != 1.0 || T[6] != 1.0) return 2;
    if (svh_grid_frame_plane(zero, H, T) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_frame_camera(2.0, p.T) != SVH_OK) return 4;
    for (k = 0; k < 12; k++)
        if (p.T[k] != T[k]) return 5;
    if (svh_grid_clear(NULL) != SVH_ERR_BAD_ARG || svh_grid_get_stats(NULL, &st) != SVH_ERR_BAD_ARG) return 6;
    if (svh_grid_get(NULL, SVH_GRID_CLASS, T, 0) != SVH_ERR_BAD_ARG) return 7;
    if (svh_grid_render(NULL, SVH_GRID_RENDER_HEIGHT, (uint8_t*)T, 0) != SVH_ERR_BAD_ARG) return 8;
    p.nx = 0;
    if (svh_grid_create(&p) != NULL) return 9;
    printf("svh_grid.h: C99 ok, planes %d..%d, modes %d..%d\n", SVH_GRID_COUNT, SVH_GRID_CLASS, SVH_GRID_RENDER_CLASS,
           SVH_GRID_RENDER_INTENSITY);
    return 0;
}

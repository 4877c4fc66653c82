/* include/svh_grid_obj.h, the objects of the ground grid, is plain C: compiled by tests/test_grid_obj.py with -std=c99 -pedantic -Wall
 * -Werror and only include/ on the path, alone and through svh_grid.h.  It needs no device: the defaults and the argument checks. */
#include <stdio.h>

#include "svh_grid_obj.h"
#include "svh_grid.h"

int main(void) {
    svh_grid_obj_params p;
    int64_t st[8], n = -1;
    int32_t recs[SVH_GRID_TRACK_RECORD], off[2];
    uint8_t px[3];
    svh_grid_obj_params_default(&p);
    svh_grid_obj_params_default(NULL);
    if (p.min_size != 4 || p.max_size != 4096 || p.max_tracks != 1024 || p.min_overlap != 1 || p.gate != 4 || p.max_missed != 2 || p.min_age != 3 ||
        p.move_cells != 2 || p.smooth_shift != 1 || !(p.min_height > 0.29f && p.min_height < 0.31f))
        return 1;
    if (svh_grid_set_objects(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_objects_params(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_get_obj_plane(NULL, SVH_GRID_OBJ_LABEL, recs, 0) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_get_objects(NULL, recs, 1, &n) != SVH_ERR_BAD_ARG || n != -1) return 4;
    if (svh_grid_get_object_stats(NULL, st) != SVH_ERR_BAD_ARG) return 5;
    if (svh_grid_objects_step(NULL, recs, 1, &n) != SVH_ERR_BAD_ARG || svh_grid_objects_reset(NULL) != SVH_ERR_BAD_ARG) return 6;
    if (svh_grid_get_tracks(NULL, recs, 1, &n) != SVH_ERR_BAD_ARG || svh_grid_get_track_plane(NULL, recs, 0, off) != SVH_ERR_BAD_ARG) return 7;
    if (svh_grid_get_track_stats(NULL, st) != SVH_ERR_BAD_ARG || svh_grid_render_objects(NULL, px, 0) != SVH_ERR_BAD_ARG) return 8;
    if ((SVH_GRID_TRACK_NEW | SVH_GRID_TRACK_BY_OVERLAP | SVH_GRID_TRACK_BY_GATE | SVH_GRID_TRACK_MISSED | SVH_GRID_TRACK_MOVING |
         SVH_GRID_TRACK_MERGED | SVH_GRID_TRACK_SPLIT) != 127)
        return 9;
    printf("svh_grid_obj.h: objects C99 ok, planes %d..%d, records of %d and %d\n", SVH_GRID_OBJ_FLAGS, SVH_GRID_OBJ_LABEL, SVH_GRID_OBJ_RECORD,
           SVH_GRID_TRACK_RECORD);
    return 0;
}

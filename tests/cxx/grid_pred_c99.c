/* include/svh_grid_pred.h, the prediction of the ground grid, is plain C: compiled by tests/test_grid_pred.py with -std=c99 -pedantic
 * -Wall -Werror and only include/ on the path, alone and through svh_grid.h.  It needs no device: the defaults and the argument
 * checks. */
#include <stdio.h>

#include "svh_grid_pred.h"
#include "svh_grid.h"

int main(void) {
    svh_grid_pred_params p;
    int64_t st[4], scores[1];
    int32_t recs[SVH_GRID_ROLL_PRED_RECORD], off[2], best = -7, poses[3] = {0, 0, 0};
    uint32_t words[1];
    uint8_t px[3];
    const double xyz[3] = {0.0, 0.0, 0.0};
    svh_grid_pred_params_default(&p);
    svh_grid_pred_params_default(NULL);
    if (p.slots != 8 || p.stride != 1 || p.poses_per_step != 1 || p.margin != 1 || p.grow16 != 0 || p.only_moving != 1) return 1;
    if (svh_grid_set_predict(NULL, &p) != SVH_ERR_BAD_ARG || svh_grid_get_predict(NULL, &p) != SVH_ERR_BAD_ARG) return 2;
    if (svh_grid_get_pred_plane(NULL, words, 0, off) != SVH_ERR_BAD_ARG || svh_grid_get_pred_stats(NULL, st) != SVH_ERR_BAD_ARG) return 3;
    if (svh_grid_footprint_pred(NULL, poses, 1, 0, words) != SVH_ERR_BAD_ARG) return 4;
    if (svh_grid_roll_score_pred(NULL, xyz, 0, recs, scores, 0, &best) != SVH_ERR_BAD_ARG || best != -7) return 5;
    if (svh_grid_render_pred(NULL, 0, px, 0) != SVH_ERR_BAD_ARG) return 6;
    printf("svh_grid_pred.h: prediction C99 ok, status %d, records of %d\n", SVH_GRID_ROLL_CUT_OBJECT, SVH_GRID_ROLL_PRED_RECORD);
    return 0;
}

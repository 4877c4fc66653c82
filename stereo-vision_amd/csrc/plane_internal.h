// internal interface between plane_engine.cpp (host) and plane_kernels.hip (device)
#ifndef SVH_PLANE_INTERNAL_H
#define SVH_PLANE_INTERNAL_H
#include <stdint.h>

#include "plane_core.h"

namespace svh {

// Device arrays of a PlaneEstimation call over `nmaps` maps of equal size.  Every per-map array has the stride given
// beside it; `cap` is the number of lattice cells (the longest list possible), S the number of hypotheses.
struct PlaneDev {
    const float* const* maps;   // [nmaps] device pointers to the disparity maps
    int32_t* n_list;            // [nmaps] list length
    float* lu;                  // [nmaps][cap]   } the list as three planes, in the reference's u-major order
    float* lv;                  // [nmaps][cap]   }
    float* ld;                  // [nmaps][cap]   }
    const int32_t* samples;     // [nmaps][4 S]   per hypothesis: how many indices (0..3), then the three indices
    double* planes;             // [nmaps][3 S]   a, b, c per hypothesis
    int32_t* counts;            // [nmaps][S]     votes (zeroed by the caller before planelaunch_vote)
    int32_t* sel;               // [nmaps][2]     winner (-1: no hypothesis has an inlier), its votes
    int32_t* inl;               // [nmaps][cap]   the winner's inlier indices, ascending
    int32_t cap, S;
};

// k_plane_grid: sparseDisparityGrid.  Row v of a map starts at maps[m] + (v - row0) * step.
void planelaunch_grid(void* stream, const PlaneDev& P, int32_t nmaps, const plane::Lattice& L, int32_t step,
                      int32_t row0);
// k_plane_fit + k_plane_vote + k_plane_select; max_n: the longest list of the call
void planelaunch_vote(void* stream, const PlaneDev& P, int32_t nmaps, int32_t max_n, double d_threshold);

}  // namespace svh
#endif

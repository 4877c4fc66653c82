// internal interface between histnorm_engine.cpp (host) and histnorm_kernels.hip (device)
#ifndef SVH_HISTNORM_INTERNAL_H
#define SVH_HISTNORM_INTERNAL_H
#include <stddef.h>
#include <stdint.h>

#include "histnorm_core.h"

namespace svh {

// All images of one call: image z belongs to pair z / slots and slot z % slots (1: a list of images, 2: left and right
// of a pair) and starts at (slot ? img1 : img0) + pair * image_stride; its rows are w bytes, row_stride apart.  counts, cdf and
// map hold 256 entries per image, in the order of z.
struct HistJob {
    uint8_t* img0;
    uint8_t* img1;   // (two fields, not an array: a lane picks one by a select, never by an index)
    size_t image_stride;
    int32_t row_stride, w, h;
    int32_t slots, images;
    int32_t* counts;      // zeroed before k_hist_count
    float* cdf;
    uint8_t* map;
    const hn::Seg* seg;   // the segment table of (w, h)
    int32_t nseg;
};

// the three kernels of a call, each ONE launch over all images of the job
void histlaunch_count(void* stream, const HistJob& a);
void histlaunch_table(void* stream, const HistJob& a);
void histlaunch_apply(void* stream, const HistJob& a);

}  // namespace svh
#endif

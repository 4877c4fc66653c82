// internal interface between recon_engine.cpp (host) and recon_track_kernels.hip (device): the RESIDENT form of
// Reconstruction, whose track table lives in device memory (svh_recon_create_resident, include/svh.h).
//
// The tracks of an object are a CSR in two buffers, A (read by an update) and B (written by it): per track its first
// frame, the feature index it ended on and its pixel offset (offs has one entry more than there are tracks, so a
// length is offs[t + 1] - offs[t]); the pixels as (u, v) floats in track order.  An update of K objects is one launch
// per kernel below with blockIdx.y = object, every kernel reading its object's ReconJob from a table in device
// memory and its counts from the object's device header, so nothing returns to the host inside an update:
//
//   k_rt_stage      new frame records and host matches from pinned memory to the device; feature-index table = -1,
//                   claim = none, header = 0
//   k_rt_scatter    old track t: atomicMax(track_idx[last_idx[t]], t) -- "a later track overwrites the slot"
//                   (reconstruction.cpp:86-87)
//   k_rt_associate  match i: idx = track_idx[i1p]; idx >= 0: atomicMin(claim[idx], i).  The first match in match order
//                   that reaches a track extends it (the test of :96 fails only for a track already extended in this
//                   update), every other match creates a track; tracks created in this update are never indexed
//   k_rt_scan       one workgroup: ordered prefix sums -- extended old tracks in old order, then created tracks in
//                   match order; lost old tracks in old order; the pixel offsets of B
//   k_rt_gather     one lane per track of B: copies / creates its pixels, first frame and feature index
//   k_rt_tracks     recon::track_outcome per lost track, read where it lies in A
//   k_rt_compact    accepted points appended in lost order; header, codes and points to pinned host memory
#ifndef SVH_RECON_INTERNAL_H
#define SVH_RECON_INTERNAL_H
#include <stdint.h>

#include "../../include/svh.h"
#include "recon_core.h"

namespace svh {

// device header of an object, int32 each
enum { RT_EXTENDED = 0, RT_CREATED = 1, RT_LOST = 2, RT_PIXELS = 3, RT_ERROR = 4, RT_POINTS = 5, RT_HDR = 8 };
// RT_ERROR bits
enum { RT_BAD_INDEX = 1,     // a match with i1p or i1c outside [0, max_index)
       RT_NO_ROOM = 2 };     // the job's capacities do not hold the update (the host sizes them: never expected)

struct ReconJob {
    // buffer A (this update reads it) and buffer B (this update writes it)
    const int32_t *a_first, *a_last, *a_offs;
    const float* a_px;
    int32_t *b_first, *b_last, *b_offs;
    float* b_px;
    const svh_p_match* m;        // n matches, device memory
    int32_t n, n_old, old_px;    // matches, tracks and pixels of A
    int32_t max_index;           // feature indices of the matches lie in [0, max_index)
    int32_t tbl;                 // entries of track_idx: >= max_index and above every last_idx of A
    int32_t cap_tracks, cap_px;  // room in B (tracks; pixels)
    int32_t frame_prev;          // first frame of a created track (current frame - 1)
    int32_t n_frames, n_points;  // frame records after this update's upload; points before it
    int32_t *track_idx, *claim;  // tbl; n_old
    int32_t *midx;               // n: the track a match reaches, or -1
    int32_t *src, *lost;         // n_old + n: where a track of B comes from (t, or ~match); n_old: lost tracks
    int32_t* hdr;                // RT_HDR
    const double* frames;
    recon::Settings s;
    int32_t* code;               // per lost track, device
    float *xyz, *points;
    int32_t *out_hdr, *out_code; // pinned host memory
    float* out_xyz;
    // pinned -> device copies in front of everything else (bytes: multiples of 16; 0: none)
    const uint8_t* up_src[2];
    uint8_t* up_dst[2];
    uint32_t up_bytes[2];
};

// the seven kernels over K jobs (d_jobs: device memory).  max_*: the largest n, n_old, tbl and up_bytes of the jobs.
void rlaunch_resident(void* stream, const ReconJob* d_jobs, int32_t K, int32_t max_n, int32_t max_old, int32_t max_tbl,
                      uint32_t max_up);

}  // namespace svh
#endif

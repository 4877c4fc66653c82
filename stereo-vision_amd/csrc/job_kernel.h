// One definition per kernel that the lockstep recorder (batch_rec.h) can batch.
//
// Such a kernel is a __device__ body of (job struct, block index) and two entries generated here from one line:
//   plain     one object: the job by value as the kernel argument (pointers stay in scalar registers);
//   batched   K objects in lockstep: job blockIdx.z of a table in device memory, grid = the largest job's.
// Both run the same body, so a batched lane computes bit for bit what the single launch computes.  What differs is
// stated once each:
//   Job globalise(Job)   per job type, next to the struct: its pointer fields through as_global (dev_common.h).
//                        Batched entry only: the plain form's pointers are kernel arguments and must not leave their
//                        scalar registers;
//   a predicate          per kernel, last argument of its line, an expression over the job `a`: false for a workgroup
//                        beyond this job's own extent (the grid is the largest job's), which then leaves before it
//                        touches anything; `true` where every job fills the grid.  Batched entry only: a plain grid
//                        is the job's own.
// A launcher states its sequence of kernels, grids and conditions once, through launch_or_record.
#ifndef SVH_JOB_KERNEL_H
#define SVH_JOB_KERNEL_H

#include <hip/hip_runtime.h>

#include "batch_rec.h"
#include "dev_common.h"

namespace svh {

template <class Job>
struct JobKernel {
    void (*plain)(Job);
    BatchLaunchFn batched;
    unsigned tx, ty;   // workgroup
};

// the batched entry `batched` of `body` and its BatchLaunchFn def_batch; on its own for a kernel without a plain form
// (tmpl: empty, or `template <>` where the entry is a specialisation of a declared kernel template)
#define SVH_BATCHED_KERNEL(def, tmpl, batched, Job, tx, ty, body, guard)                                           \
    tmpl __global__ __launch_bounds__((tx) * (ty)) void batched(const Job* J) {                                    \
        const Job& a = J[blockIdx.z];                                                                              \
        if (guard) body(globalise(a), blockIdx.x, blockIdx.y);                                                     \
    }                                                                                                              \
    static void def##_batch(const void* jobs, int njobs, unsigned gx, unsigned gy, size_t lds, hipStream_t s) {    \
        hipLaunchKernelGGL(batched, dim3(gx, gy, (unsigned)njobs), dim3(tx, ty), lds, s,                           \
                           reinterpret_cast<const Job*>(jobs));                                                    \
    }
// both entries and the definition `def` that launch_or_record takes
#define SVH_JOB_KERNEL(def, tmpl, plain, batched, Job, tx, ty, body, guard)                                        \
    tmpl __global__ __launch_bounds__((tx) * (ty)) void plain(Job a) { body(a, blockIdx.x, blockIdx.y); }          \
    SVH_BATCHED_KERNEL(def, tmpl, batched, Job, tx, ty, body, guard)                                               \
    const JobKernel<Job> def = {plain, def##_batch, tx, ty};

// launch the plain entry now, or -- while the calling thread records a batch -- append the job to the recorder
template <class Job>
inline void launch_or_record(void* stream, const JobKernel<Job>& k, const Job& job, dim3 grid, size_t lds = 0) {
    if (t_rec) return t_rec->add(k.batched, job, grid.x, grid.y, lds);
    void* args[] = {const_cast<Job*>(&job)};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(k.plain), grid, dim3(k.tx, k.ty), args, lds, (hipStream_t)stream);
}
// dynamic LDS beyond the default 64 KB, for both entries
template <class Job>
inline void allow_dynamic_lds(const JobKernel<Job>& k, void (*batched)(const Job*), int bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k.plain), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(batched), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace svh
#endif

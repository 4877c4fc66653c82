// Map fusion on the device (include/svh_map.h): 3-D reprojection of D1 and the
// frame-to-frame association of stereomapper, kernels + the small host engine around them.
//   StereoThread::createCurrentMap                  stereomapper/stereothread.cpp:180-255
//   StereoThread::addDisparityMapToReconstruction   stereomapper/stereothread.cpp:290-437
//
// What is sequential in the reference and how it is kept:
//  * the association scans the previous map column by column and READ-MODIFY-WRITES the current
//    map at the projected pixel, so several previous points landing on one pixel see each
//    other's effect in scan order.  Here every previous point first files itself under its target
//    pixel (one atomicExch per point: per-target linked lists), then one thread per target pixel
//    replays its list in scan order -- different targets never interact;
//  * the two point lists are push_back'ed in scan order (columns left to right, top to bottom):
//    ordered stream compaction over that order (count per 1024 elements, scan, scatter).
// fp32 with IEEE division and no contraction (the file is compiled with -ffp-contract=off): the
// reference's float expressions operation by operation; the double-typed sub-expressions
// (x / 255.0, the gain ramp, (a + b) / 2.0) are evaluated in double and narrowed once.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/matrix.h"
#include "../../include/svh.h"
#include "../../include/svh_map.h"
#include "batch_rec.h"
#include "hip_guard.h"
#include "job_kernel.h"
#include "map_internal.h"
#include "svh_config.h"
#include "view2d_core.h"

using namespace svh;

// Every kernel of the fusion is a job struct with its globalise, a __device__ body and one SVH_JOB_KERNEL line
// (job_kernel.h): the plain entry serves svh_map_add / svh_map_add_device, the batched one K maps in lockstep
// (svh_map_add_batch_device).  Both run the same body.
namespace {

struct MapCoef {
    float hcf[12];      // rows 0..2 of H_total
    float hfc[4];       // row 2 of inv(H_total)
    float pfc[12];      // K * inv(H_total)[0:3, 0:4]
    float f, cu, cv, base, max_dist;
    float gain_inv;
    int32_t margin;
};

struct Planes {
    float *I, *D, *X, *Y, *Z;
};
__device__ __forceinline__ void planes_global(Planes& p) { all_global(p.I, p.D, p.X, p.Y, p.Z); }

// (int32_t)float as x86's cvttss2si does it: out of range / NaN -> INT_MIN
__device__ __forceinline__ int32_t f2i_x86(float f) {
    return (f >= -2147483648.f && f < 2147483648.f) ? (int32_t)f : (int32_t)0x80000000;
}

// ---- createCurrentMap ---------------------------------------------------------------------
// head (a lockstep batch only, else null): the target lists of the association start empty, head[a] = -1 -- what the
// single call's memset leaves there
struct MapCreateJob {
    const float* D1;
    const uint8_t* I1;
    int w, h, step;
    MapCoef c;
    Planes cur;
    int32_t* head;
};
__device__ __forceinline__ MapCreateJob globalise(MapCreateJob a) {
    all_global(a.D1, a.I1, a.head);
    planes_global(a.cur);
    return a;
}
__device__ __forceinline__ void d_map_create(const MapCreateJob& j, unsigned bx, unsigned by) {
    const int w = j.w, h = j.h;
    const MapCoef& c = j.c;
    const Planes& cur = j.cur;
    const int u = (int)bx * 64 + (threadIdx.x & 63), v = (int)by * 4 + (threadIdx.x >> 6);
    if (u >= w || v >= h) return;
    const int a = v * w + u;
    if (j.head) j.head[a] = -1;
    float I = (float)((double)(float)j.I1[(size_t)v * j.step + u] / 255.0);
    // gain ramp over the image border (:232-252): every pixel is touched by at most one (i, side)
    const int m = c.margin;
    int i = -1;
    if (u >= m && u < w - m) {
        if (v < m) i = v;
        else if (v >= h - m) i = h - 1 - v;
    } else if (v >= m && v < h - m) {
        if (u < m) i = u;
        else if (u >= w - m) i = w - 1 - u;
    }
    if (i >= 0) {
        const float g = (float)(((double)__fmul_rn((float)(m - i), c.gain_inv) + (double)(float)i * 1.0) / (double)(float)m);
        // std::min(std::max(t, 0.f), 1.f) as its two comparisons: -0.0f and NaN pass through, which fmaxf / fminf
        // do not promise
        const float t = __fmul_rn(g, I);
        const float lo = (t < 0.f) ? 0.f : t;
        I = (1.f < lo) ? 1.f : lo;
    }
    float d = j.D1[a], X = 0.f, Y = 0.f, Z = 0.f;
    if (d > 0) {
        const float z = __fdiv_rn(__fmul_rn(c.f, c.base), d);
        if ((double)z > 0.1 && z < c.max_dist) {
            const float x = __fdiv_rn(__fmul_rn(__fsub_rn((float)u, c.cu), c.base), d);
            const float y = __fdiv_rn(__fmul_rn(__fsub_rn((float)v, c.cv), c.base), d);
            X = c.hcf[0] * x + c.hcf[1] * y + c.hcf[2] * z + c.hcf[3];
            Y = c.hcf[4] * x + c.hcf[5] * y + c.hcf[6] * z + c.hcf[7];
            Z = c.hcf[8] * x + c.hcf[9] * y + c.hcf[10] * z + c.hcf[11];
        } else {
            d = -1.f;
        }
    }
    cur.I[a] = I;
    cur.D[a] = d;
    cur.X[a] = X;
    cur.Y[a] = Y;
    cur.Z[a] = Z;
}
SVH_JOB_KERNEL(kd_map_create, , k_map_create, k_map_create_b, MapCreateJob, 256, 1, d_map_create,
               (int)blockIdx.x * 64 < a.w && (int)blockIdx.y * 4 < a.h)

// ---- association, step 1: every valid previous point finds its target pixel -----------------
// state: 0 = no point here, 1 = point that stays in the previous list, 2 = filed under a target
struct MapProjectJob {
    Planes prev;
    int pw, ph, cw, chh;
    MapCoef c;
    int32_t *head, *next;
    uint8_t* state;
};
__device__ __forceinline__ MapProjectJob globalise(MapProjectJob a) {
    planes_global(a.prev);
    all_global(a.head, a.next, a.state);
    return a;
}
__device__ __forceinline__ void d_map_project(const MapProjectJob& j, unsigned bx, unsigned) {
    const Planes& prev = j.prev;
    const MapCoef& c = j.c;
    const int cw = j.cw, chh = j.chh;
    int32_t* const head = j.head;
    int32_t* const next = j.next;
    const int a = (int)bx * 256 + threadIdx.x;
    if (a >= j.pw * j.ph) return;
    uint8_t st = 0;
    if (prev.D[a] > 0) {
        st = 1;
        const float x = prev.X[a], y = prev.Y[a], z = prev.Z[a];
        const float z2 = c.hfc[0] * x + c.hfc[1] * y + c.hfc[2] * z + c.hfc[3];
        if ((double)z2 > 0.1 && z2 < c.max_dist) {
            const float w2 = c.pfc[8] * x + c.pfc[9] * y + c.pfc[10] * z + c.pfc[11];
            const int32_t u2 = f2i_x86(__fdiv_rn(c.pfc[0] * x + c.pfc[1] * y + c.pfc[2] * z + c.pfc[3], w2));
            const int32_t v2 = f2i_x86(__fdiv_rn(c.pfc[4] * x + c.pfc[5] * y + c.pfc[6] * z + c.pfc[7], w2));
            if (u2 >= 0 && u2 < cw && v2 >= 0 && v2 < chh) {
                st = 2;
                next[a] = atomicExch(&head[v2 * cw + u2], a);
            }
        }
    }
    j.state[a] = st;
}
SVH_JOB_KERNEL(kd_map_project, , k_map_project, k_map_project_b, MapProjectJob, 256, 1, d_map_project,
               (int)blockIdx.x * 256 < a.pw * a.ph)

// ---- association, step 2: one thread per target pixel replays its points in scan order -------
struct MapFuseJob {
    Planes prev;
    int pw, ph;
    Planes cur;
    int cn;
    const int32_t *head, *next;
    uint8_t* state;
};
__device__ __forceinline__ MapFuseJob globalise(MapFuseJob a) {
    planes_global(a.prev);
    planes_global(a.cur);
    all_global(a.head, a.next, a.state);
    return a;
}
__device__ __forceinline__ void d_map_fuse(const MapFuseJob& j, unsigned bx, unsigned) {
    const Planes& prev = j.prev;
    const Planes& cur = j.cur;
    const int pw = j.pw, ph = j.ph;
    const int32_t* const head = j.head;
    const int32_t* const next = j.next;
    uint8_t* const state = j.state;
    const int a2 = (int)bx * 256 + threadIdx.x;
    if (a2 >= j.cn) return;
    int first = head[a2];
    if (first < 0) return;
    float D = cur.D[a2], X = cur.X[a2], Y = cur.Y[a2], Z = cur.Z[a2], I = cur.I[a2];
    // scan order of a previous pixel a = v * pw + u is u * ph + v
    long long last = -1;
    for (;;) {
        int pick = -1;
        long long best = 0x7FFFFFFFFFFFFFFFll;
        for (int s = first; s >= 0; s = next[s]) {
            const int v = s / pw, u = s - v * pw;
            const long long key = (long long)u * ph + v;
            if (key > last && key < best) {
                best = key;
                pick = s;
            }
        }
        if (pick < 0) break;
        last = best;
        const float x = prev.X[pick], y = prev.Y[pick], z = prev.Z[pick], pi = prev.I[pick];
        bool added = false;
        if (D > 0) {
            // fabs(float) + fabs(float) + fabs(float) < 0.2 (:355)
            const float dist = __fadd_rn(__fadd_rn(fabsf(__fsub_rn(x, X)), fabsf(__fsub_rn(y, Y))), fabsf(__fsub_rn(z, Z)));
            if ((double)dist < 0.2) {
                X = (float)((double)__fadd_rn(X, x) / 2.0);
                Y = (float)((double)__fadd_rn(Y, y) / 2.0);
                Z = (float)((double)__fadd_rn(Z, z) / 2.0);
                I = (float)((double)__fadd_rn(I, pi) / 2.0);
                added = true;
            }
        } else {
            X = x;
            Y = y;
            Z = z;
            I = pi;
            D = 1.f;
            added = true;
        }
        state[pick] = added ? 0 : 1;
    }
    cur.D[a2] = D;
    cur.X[a2] = X;
    cur.Y[a2] = Y;
    cur.Z[a2] = Z;
    cur.I[a2] = I;
}
SVH_JOB_KERNEL(kd_map_fuse, , k_map_fuse, k_map_fuse_b, MapFuseJob, 256, 1, d_map_fuse, (int)blockIdx.x * 256 < a.cn)

// ---- ordered compaction over the scan order e = u * h + v -------------------------------------
// kFromState: element taken iff state == 1 (previous list); else iff D > 0 (current list)
template <bool kFromState>
__device__ __forceinline__ bool map_taken(const uint8_t* state, const float* D, int a) {
    return kFromState ? state[a] == 1 : D[a] > 0;
}

// (the jobs of count and scatter: `aux` = the block counts written / the block offsets read, out = scatter's list)
struct MapListJob {
    const uint8_t* state;
    Planes pl;
    int w, h;
    int32_t* aux;
    float4* out;
};
__device__ __forceinline__ MapListJob globalise(MapListJob a) {
    planes_global(a.pl);
    all_global(a.state, a.aux, a.out);
    return a;
}
template <bool kFromState>
__global__ void k_map_count(MapListJob a);
template <bool kFromState>
__global__ void k_map_count_b(const MapListJob* J);
template <bool kFromState>
__device__ __forceinline__ void d_map_count(const MapListJob& j, unsigned bx, unsigned) {
    __shared__ int s_sum[4];
    const int w = j.w, h = j.h;
    const int n = w * h;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int e = (int)bx * 1024 + threadIdx.x * 4 + k;
        if (e < n) {
            const int u = e / h, v = e - u * h;
            mine += map_taken<kFromState>(j.state, j.pl.D, v * w + u) ? 1 : 0;
        }
    }
    for (int off = 32; off; off >>= 1) mine += __shfl_down(mine, off);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) j.aux[bx] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}
SVH_JOB_KERNEL(kd_map_count0, template <>, k_map_count<false>, k_map_count_b<false>, MapListJob, 256, 1,
               d_map_count<false>, (int)blockIdx.x * 1024 < a.w * a.h)
SVH_JOB_KERNEL(kd_map_count1, template <>, k_map_count<true>, k_map_count_b<true>, MapListJob, 256, 1,
               d_map_count<true>, (int)blockIdx.x * 1024 < a.w * a.h)

// exclusive scan of the block counts in place (one workgroup); total -> *total
struct MapScanJob {
    int32_t* blockcnt;
    int nb;
    int64_t* total;
};
__device__ __forceinline__ MapScanJob globalise(MapScanJob a) { all_global(a.blockcnt, a.total); return a; }
__device__ __forceinline__ void d_map_scan(const MapScanJob& j, unsigned, unsigned) {
    __shared__ int s[1024];
    int32_t* const blockcnt = j.blockcnt;
    const int nb = j.nb;
    int carry = 0;
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int x = i < nb ? blockcnt[i] : 0;
        s[threadIdx.x] = x;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nb) blockcnt[i] = carry + s[threadIdx.x] - x;
        const int chunk = s[1023];
        __syncthreads();
        carry += chunk;
    }
    if (threadIdx.x == 0) *j.total = carry;
}
SVH_JOB_KERNEL(kd_map_scan, , k_map_scan, k_map_scan_b, MapScanJob, 1024, 1, d_map_scan, blockIdx.x == 0)

template <bool kFromState>
__global__ void k_map_scatter(MapListJob a);
template <bool kFromState>
__global__ void k_map_scatter_b(const MapListJob* J);
template <bool kFromState>
__device__ __forceinline__ void d_map_scatter(const MapListJob& j, unsigned bx, unsigned) {
    __shared__ int s[256];
    const uint8_t* const state = j.state;
    const Planes& pl = j.pl;
    float4* const out = j.out;
    const int w = j.w, h = j.h;
    const int n = w * h;
    int addr[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int e = (int)bx * 1024 + threadIdx.x * 4 + k;
        addr[k] = -1;
        if (e < n) {
            const int u = e / h, v = e - u * h;
            const int a = v * w + u;
            if (map_taken<kFromState>(state, pl.D, a)) {
                addr[k] = a;
                mine++;
            }
        }
    }
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    int pos = j.aux[bx] + s[threadIdx.x] - mine;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (addr[k] >= 0) out[pos++] = make_float4(pl.X[addr[k]], pl.Y[addr[k]], pl.Z[addr[k]], pl.I[addr[k]]);
}
SVH_JOB_KERNEL(kd_map_scatter0, template <>, k_map_scatter<false>, k_map_scatter_b<false>, MapListJob, 256, 1,
               d_map_scatter<false>, (int)blockIdx.x * 1024 < a.w * a.h)
SVH_JOB_KERNEL(kd_map_scatter1, template <>, k_map_scatter<true>, k_map_scatter_b<true>, MapListJob, 256, 1,
               d_map_scatter<true>, (int)blockIdx.x * 1024 < a.w * a.h)

// ---- colour-coded disparity (stereothread.cpp:117-147) -------------------------------------------
__global__ __launch_bounds__(256) void k_disp_color(const float* __restrict__ D, long long n, float* __restrict__ rgb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // the arithmetic is shared with the disparity pane (k_view2d_texels): csrc/view2d_core.h
    float c[3];
    svh::view2d::disparity_colour(D[i], c);
    rgb[3 * i + 0] = c[0];
    rgb[3 * i + 1] = c[1];
    rgb[3 * i + 2] = c[2];
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host engine
// ---------------------------------------------------------------------------------------------
// struct svh_map: csrc/map_internal.h (the map view reads the point lists where they lie)
static Planes planes_of(const svh_map* m, int k) {
    const svh_map::Bufs& b = m->b;
    return Planes{b.pl[k][0], b.pl[k][1], b.pl[k][2], b.pl[k][3], b.pl[k][4]};
}

#define MAP_TRY(kind, expr) SVH_HIP_TRY("map", kind, expr)
#define MAP_GROW(buf, bytes) SVH_HIP_GROW("map", buf, bytes)

static int32_t map_ensure(svh_map* m, int32_t w, int32_t h) {
    if (m->w == w && m->h == h) return SVH_OK;
    // a change of geometry starts a new reconstruction: the previous map cannot be addressed
    // with the new dimensions' buffers
    m->b = svh_map::Bufs();
    m->w = m->h = 0;             // (until every buffer exists: a failure below is repaired by the next call)
    const size_t n = (size_t)w * h;
    svh_map::Bufs& b = m->b;
    for (int k = 0; k < 2; k++) {
        for (int i = 0; i < 5; i++) MAP_GROW(b.pl[k][i], n * 4);
        MAP_GROW(b.pts[k], n * sizeof(float4));
    }
    MAP_GROW(b.dD1, n * 4);
    MAP_GROW(b.dI1, n);
    MAP_GROW(b.head, n * 4);
    MAP_GROW(b.next, n * 4);
    MAP_GROW(b.state, n);
    MAP_GROW(b.blockcnt, ((n + 1023) / 1024 + 1) * 4);
    MAP_GROW(b.h_stage, n * 5);
    m->w = w;
    m->h = h;
    m->have_prev = false;
    m->npts[0] = m->npts[1] = 0;
    return SVH_OK;
}

// coefficients (stereothread.cpp:196-199, 306-314, 450-455) with the Matrix class of the boundary
static MapCoef map_coef(const svh_map* m, int32_t w, int32_t h, const double* H_total, float gain) {
    MapCoef c;
    {
        Matrix Ht(4, 4, H_total);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) c.hcf[4 * i + j] = (float)Ht._val[i][j];
        Matrix Hi = Matrix::inv(Ht);
        const bool ok = Hi._m == 4;
        for (int j = 0; j < 4; j++) c.hfc[j] = ok ? (float)Hi._val[2][j] : 0.f;
        Matrix K(3, 3);
        K._val[0][0] = m->p.f; K._val[1][1] = m->p.f; K._val[0][2] = m->p.cu; K._val[1][2] = m->p.cv; K._val[2][2] = 1;
        if (ok) {
            Matrix top(3, 4);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 4; j++) top._val[i][j] = Hi._val[i][j];
            Matrix P = K * top;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 4; j++) c.pfc[4 * i + j] = (float)P._val[i][j];
        } else {
            for (int i = 0; i < 12; i++) c.pfc[i] = 0.f;
        }
    }
    c.f = m->p.f; c.cu = m->p.cu; c.cv = m->p.cv; c.base = m->p.base; c.max_dist = m->p.max_dist;
    c.margin = std::min(std::min(200, w / 2), h / 2);
    c.gain_inv = 1;
    if (gain) c.gain_inv = 1.0 / gain;
    return c;
}

// The device work of one frame of one map, launched on the map's stream or -- while the calling thread records a batch
// (batch_rec.h) -- appended to the recorder.  A map without a previous one issues the shorter sequence.  The reset of
// `head`: the single call's memset; a recorded frame has k_map_create write it (a memset cannot be recorded).
// The point counts arrive in m->h_total ([0] only when the frame fuses).
static int32_t map_enqueue(svh_map* m, const float* dD, const uint8_t* dI, int32_t w, int32_t h, int32_t dstep,
                           const MapCoef& c) {
    hipStream_t s = m->stream;
    const size_t n = (size_t)w * h;
    const svh_map::Bufs& b = m->b;
    const bool fuse = m->have_prev;
    const Planes cur = planes_of(m, m->cur), prev = planes_of(m, 1 - m->cur);
    const MapCreateJob jc = {dD, dI, w, h, dstep, c, cur, fuse && t_rec ? (int32_t*)b.head : nullptr};
    launch_or_record(s, kd_map_create, jc, dim3((w + 63) / 64, (h + 3) / 4));
    const int nb = (int)((n + 1023) / 1024);
    if (fuse) {
        const int pn = m->pw * m->ph;   // == n: a geometry change resets the reconstruction
        if (!t_rec) MAP_TRY(copy, hipMemsetAsync(b.head, 0xFF, n * 4, s));
        const MapProjectJob jp = {prev, m->pw, m->ph, w, h, c, b.head, b.next, b.state};
        launch_or_record(s, kd_map_project, jp, dim3((pn + 255) / 256));
        const MapFuseJob jf = {prev, m->pw, m->ph, cur, (int)n, b.head, b.next, b.state};
        launch_or_record(s, kd_map_fuse, jf, dim3((unsigned)((n + 255) / 256)));
        const int pb = (pn + 1023) / 1024;
        const MapListJob jl = {b.state, prev, m->pw, m->ph, b.blockcnt, b.pts[0]};
        launch_or_record(s, kd_map_count1, jl, dim3(pb));
        const MapScanJob js = {b.blockcnt, pb, m->h_total};
        launch_or_record(s, kd_map_scan, js, dim3(1));
        launch_or_record(s, kd_map_scatter1, jl, dim3(pb));
    }
    const MapListJob jl = {b.state, cur, w, h, b.blockcnt, b.pts[1]};
    launch_or_record(s, kd_map_count0, jl, dim3(nb));
    const MapScanJob js = {b.blockcnt, nb, m->h_total + 1};
    launch_or_record(s, kd_map_scan, js, dim3(1));
    launch_or_record(s, kd_map_scatter0, jl, dim3(nb));
    return SVH_OK;
}

// the frame's device work is done: the object takes it
static void map_take_frame(svh_map* m, int32_t w, int32_t h) {
    m->last_fused = m->have_prev;
    m->npts[0] = m->have_prev ? m->h_total[0] : 0;
    m->npts[1] = m->h_total[1];
    // the current map becomes the previous one (the intended ":432")
    m->cur = 1 - m->cur;
    m->pw = w;
    m->ph = h;
    m->have_prev = true;
}

extern "C" {

svh_map* svh_map_create(const svh_map_params* p) {
    svh::ensure_init();
    if (!p) return nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
        return nullptr;
    }
    svh_map* m = new svh_map();
    m->p = *p;
    (void)hipGetDevice(&m->device);
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
        m->h_total.grow(2 * sizeof(int64_t)) != hipSuccess) {
        delete m;
        return nullptr;
    }
    return m;
}

void svh_map_destroy(svh_map* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    const hipStream_t s = m->stream;
    delete m;   // the buffers free themselves, on the device selected above
    if (s) (void)hipStreamDestroy(s);
}

void svh_map_clear(svh_map* m) {
    if (!m) return;
    m->have_prev = false;
    m->npts[0] = m->npts[1] = 0;
}

// svh_map_add / svh_map_add_device.  i1_on_device: I1 is read where it lies, at its own pitch (k_map_create takes
// one), and D1 is on the device as well: no host staging at all
static int32_t map_add(svh_map* m, const float* D1, int32_t d1_on_device, const uint8_t* I1, bool i1_on_device,
                       const int32_t* dims, const double* H_total, float gain) {
    if (!m || !D1 || !I1 || !dims || !H_total) return svh::fail(SVH_ERR_BAD_ARG, "null argument");
    const int32_t w = dims[0], h = dims[1], step = dims[2];
    if (w < 1 || h < 1 || step < w || (int64_t)w * h > (1 << 28)) return svh::fail(SVH_ERR_BAD_ARG, "bad dimensions");
    MAP_TRY(none, hipSetDevice(m->device));
    int32_t rc = map_ensure(m, w, h);
    if (rc) return rc;
    hipStream_t s = m->stream;
    const size_t n = (size_t)w * h;
    const svh_map::Bufs& b = m->b;
    // inputs: the image rows are packed on the way into pinned memory
    const uint8_t* dI = I1;
    int32_t dstep = step;
    if (!i1_on_device) {
        for (int32_t v = 0; v < h; v++) memcpy(b.h_stage + (size_t)v * w, I1 + (size_t)v * step, w);
        MAP_TRY(copy, hipMemcpyAsync(b.dI1, b.h_stage, n, hipMemcpyHostToDevice, s));
        dI = b.dI1;
        dstep = w;
    }
    const float* dD = D1;
    if (!d1_on_device) {
        memcpy(b.h_stage + n, D1, n * 4);
        MAP_TRY(copy, hipMemcpyAsync(b.dD1, b.h_stage + n, n * 4, hipMemcpyHostToDevice, s));
        dD = b.dD1;
    }
    const MapCoef c = map_coef(m, w, h, H_total, gain);
    rc = map_enqueue(m, dD, dI, w, h, dstep, c);
    if (rc) return rc;
    MAP_TRY(wait, hipStreamSynchronize(s));
    MAP_TRY(launch, hipGetLastError());
    map_take_frame(m, w, h);
    return SVH_OK;
}

int32_t svh_map_add(svh_map* m, const float* D1, int32_t d1_on_device, const uint8_t* I1, const int32_t* dims,
                    const double* H_total, float gain) {
    return map_add(m, D1, d1_on_device, I1, false, dims, H_total, gain);
}

int32_t svh_map_add_device(svh_map* m, const float* dD1, const uint8_t* dI1, const int32_t* dims, const double* H_total,
                           float gain) {
    return map_add(m, dD1, 1, dI1, true, dims, H_total, gain);
}

// K maps in lockstep, one frame each, everything in device memory: the device work of all maps that fuse is recorded
// and issued as ONE launch per kernel on ms[0]'s stream (batch_rec.h), and so is that of the maps that start a
// reconstruction -- two recorded phases at the most, one wait each.  Results are those of K svh_map_add_device calls.
int32_t svh_map_add_batch_device(svh_map* const* ms, int32_t K, const float* const* dD1, const uint8_t* const* dI1,
                                 const int32_t* dims, const double* const* H_total, const float* gain) {
    if (!ms || !dD1 || !dI1 || !dims || !H_total || !gain || K < 0) return svh::fail(SVH_ERR_BAD_ARG, "null argument");
    const int32_t w = dims[0], h = dims[1], step = dims[2];
    if (w < 1 || h < 1 || step < w || (int64_t)w * h > (1 << 28)) return svh::fail(SVH_ERR_BAD_ARG, "bad dimensions");
    for (int i = 0; i < K; i++)
        if (!dD1[i] || !dI1[i] || !H_total[i]) return svh::fail(SVH_ERR_BAD_ARG, "null argument in the batch");
    bool lockstep = false;
    const int32_t bad = check_batch(ms, K, "map", &lockstep, [](int) { return true; });
    if (bad) return bad;
    if (K == 0) return SVH_OK;
    if (!lockstep || K == 1) {
        for (int i = 0; i < K; i++) {
            const int32_t rc = svh_map_add_device(ms[i], dD1[i], dI1[i], dims, H_total[i], gain[i]);
            if (rc) return rc;
        }
        return SVH_OK;
    }
    MAP_TRY(none, hipSetDevice(ms[0]->device));
    std::vector<MapCoef> coef((size_t)K);
    std::vector<int> group[2];   // 0: the maps that fuse, 1: those that start a reconstruction
    for (int i = 0; i < K; i++) {
        const int32_t rc = map_ensure(ms[i], w, h);   // (a change of geometry starts a new reconstruction)
        if (rc) return rc;
        coef[i] = map_coef(ms[i], w, h, H_total[i], gain[i]);
        group[ms[i]->have_prev ? 0 : 1].push_back(i);
    }
    BatchRec& rec = batch_recorder(ms[0]->device);
    hipStream_t s = ms[0]->stream;
    for (int g = 0; g < 2; g++) {
        if (group[g].empty()) continue;
        const int32_t rc = run_recorded(
            rec, s, group[g].data(), (int)group[g].size(), Phase{"map", FI_wait},
            [&](int i) -> int { return map_enqueue(ms[i], dD1[i], dI1[i], w, h, step, coef[i]); },
            [&](int i) -> int {
                MAP_TRY(wait, hipStreamSynchronize(ms[i]->stream));
                return SVH_OK;
            },
            no_undo);
        if (rc < 0) return rc;   // (no object has taken the frame)
    }
    for (int i = 0; i < K; i++) map_take_frame(ms[i], w, h);
    return SVH_OK;
}

int64_t svh_map_points(svh_map* m, int32_t which, float* xyzv, int64_t cap) {
    if (!m) return 0;
    const int k = which ? 1 : 0;
    const int64_t n = m->npts[k];
    if (xyzv && n > 0 && cap > 0) {
        (void)hipSetDevice(m->device);
        (void)hipMemcpy(xyzv, m->b.pts[k], (size_t)std::min(n, cap) * sizeof(float4), hipMemcpyDeviceToHost);
    }
    return n;
}

int32_t svh_disparity_colormap(const float* D, int32_t d_on_device, int64_t n, float* rgb) {
    if (!D || !rgb || n < 0) return svh::fail(SVH_ERR_BAD_ARG, "null argument");
    if (n == 0) return SVH_OK;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        return svh::fail(SVH_ERR_NO_DEVICE, "no HIP device visible: libsvhip has no CPU fallback");
    svh::HipBuf<float> dD, dC;
    MAP_GROW(dC, (size_t)n * 12);
    const float* src = D;
    if (!d_on_device) {
        MAP_GROW(dD, (size_t)n * 4);
        MAP_TRY(copy, hipMemcpy(dD, D, (size_t)n * 4, hipMemcpyHostToDevice));
        src = dD;
    }
    hipLaunchKernelGGL(k_disp_color, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, src, (long long)n, dC);
    const hipError_t e = hipMemcpy(rgb, dC, (size_t)n * 12, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return svh::fail(SVH_ERR_HIP, std::string("colormap: ") + hipGetErrorString(e));
    return SVH_OK;
}

int32_t svh_map_planes(svh_map* m, float* out5, size_t cap_floats) {
    if (!m || !out5 || !m->have_prev) return svh::fail(SVH_ERR_BAD_ARG, "no map yet");
    const size_t n = (size_t)m->w * m->h;
    if (cap_floats < 5 * n) return svh::fail(SVH_ERR_BAD_ARG, "buffer too small");
    MAP_TRY(none, hipSetDevice(m->device));
    const Planes p = planes_of(m, 1 - m->cur);   // the map of the last frame
    float* src[5] = {p.I, p.D, p.X, p.Y, p.Z};
    for (int k = 0; k < 5; k++) MAP_TRY(copy, hipMemcpy(out5 + k * n, src[k], n * 4, hipMemcpyDeviceToHost));
    return SVH_OK;
}

}  // extern "C"

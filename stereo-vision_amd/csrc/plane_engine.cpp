// PlaneEstimation (stereomapper/planeestimation.{h,cpp}) behind the svh_plane_* entries of include/svh_plane.h.
//
// Device (plane_kernels.hip): the ordered compaction of the lattice out of the map, the num_samples three-point fits,
// the vote of every hypothesis on every list entry, the first-maximum winner and its inlier indices in list order.
// Host (this file): the draw walk and the last few microseconds -- the refit over the winner's inliers, whose ~10 k
// terms are added in list order because the order shows in the last bits of the sums, and planeDsiTo3d with atan2.
//
// The draw walk: rand()'s raw stream does not depend on the data, but how many draws a hypothesis consumes does, so
// hypothesis i + 1 starts where hypothesis i stopped.  The walk is done on the host over the list the first kernel
// copied back (u and v of <= 12 450 entries at 1242x375): a few draws per hypothesis, ~20 k dependent steps, against a
// device form that has to evaluate every start offset of a raw block and then still walk the chain serially.  It
// costs a second stream wait per call; the phase times (svh_plane_get_timing) say what it is worth.  The raw stream of a seed is
// cached per object, so a caller that keeps its seed draws nothing twice.
//
// One call is: [upload of a host map] k_plane_grid, list copy-back, wait; walk; sample upload, k_plane_fit,
// k_plane_vote, k_plane_select, copy-back, wait; refit.  A call is a transaction: the results are written to the
// object(s) after the last step that can fail.  There is no CPU path for the device part.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/svh_plane.h"
#include "batch_rec.h"
#include "hip_guard.h"
#include "plane_internal.h"
#include "vo_internal.h"

using namespace svh;

namespace {

#define PLANE_TRY(kind, expr) SVH_HIP_TRY("PlaneEstimation", kind, expr)
#define PLANE_GROW(buf, bytes) SVH_HIP_GROW("PlaneEstimation", buf, bytes)

constexpr size_t RAW_KEEP = 1u << 20;   // raw draws an object keeps between calls (4 MB); a longer walk is not cached

// section offsets of the device block and of its pinned mirror (same layout) for nmaps maps, cap cells, S hypotheses
struct Layout {
    size_t maps, samples, n_list, lu, lv, ld, sel, planes, counts, inl, end;
    Layout(size_t nmaps, size_t cap, size_t S) {
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t o = at;
            at += up16(bytes);
            return o;
        };
        maps = take(8 * nmaps);
        samples = take(16 * nmaps * S);
        n_list = take(4 * nmaps);   // n_list .. ld: copied back after k_plane_grid
        lu = take(4 * nmaps * cap);
        lv = take(4 * nmaps * cap);
        ld = take(4 * nmaps * cap);
        sel = take(8 * nmaps);      // sel .. inl: copied back after k_plane_select
        planes = take(24 * nmaps * S);
        counts = take(4 * nmaps * S);
        inl = take(4 * nmaps * cap);
        end = at;
    }
};

// what one estimate leaves in an object
struct Result {
    int32_t status = SVH_OK;
    double plane_d[3] = {0, 0, 0}, plane_e[3] = {0, 0, 0}, H[16];
    float pitch = 0;
    std::vector<float> list;          // u v d per entry
    std::vector<double> planes;       // per hypothesis
    std::vector<int32_t> draws, votes, inliers;
    int32_t best = -1;
    Result() {
        for (int i = 0; i < 16; i++) H[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
};

}  // namespace

struct svh_plane {
    svh_plane_params prm;
    int device = 0;
    Result res;                         // _plane_d, _plane_e, _H, _pitch and the taps of the last call
    bool timing = false;
    double ms[7] = {0, 0, 0, 0, 0, 0, 0};
    // the raw rand() stream of raw_seed, as far as it was needed
    bool raw_ok = false;
    uint32_t raw_seed = 0;
    std::vector<int32_t> raw;
    RandStream rs;
    // device side
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    HipBuf<uint8_t> d_all;
    PinnedBuf<uint8_t> h_all;
    HipBuf<float> d_map;                        // a host map on its way to the device
    PinnedBuf<float> h_map;
};

namespace {

void release_buffers(svh_plane* p) {
    p->d_all.release();
    p->h_all.release();
    p->d_map.release();
    p->h_map.release();
}

int ensure(svh_plane* p, size_t all_bytes, size_t map_bytes) {
    PLANE_TRY(none, hipSetDevice(p->device));
    if (!p->stream) {
        hipStream_t s = nullptr;
        PLANE_TRY(none, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        p->stream = s;
    }
    for (int i = 0; i < 4; i++)
        if (!p->ev[i]) PLANE_TRY(none, hipEventCreate(&p->ev[i]));
    PLANE_GROW(p->d_all, all_bytes + 16);
    PLANE_GROW(p->h_all, all_bytes + 16);
    if (map_bytes) {
        PLANE_GROW(p->d_map, map_bytes + 16);
        PLANE_GROW(p->h_map, map_bytes + 16);
    }
    return SVH_OK;
}

plane::Params core_params(const svh_plane_params& s, int32_t width, int32_t height) {
    plane::Params c;
    c.num_samples = s.num_samples;
    c.step_size = s.step_size;
    c.max_draws = s.max_draws;
    c.min_dist = s.min_dist;
    c.d_threshold = s.d_threshold;
    const bool ref_roi = s.roi[0] == -1 && s.roi[1] == -1 && s.roi[2] == -1 && s.roi[3] == -1;
    const int32_t ref[4] = {0, height / 3, width - 1, height - 1};   // planeestimation.cpp:32
    for (int i = 0; i < 4; i++) c.roi[i] = ref_roi ? ref[i] : s.roi[i];
    return c;
}

bool params_ok(const svh_plane_params& s) {
    return s.num_samples >= 1 && s.num_samples <= (1 << 20) && s.step_size >= 1 && s.max_draws >= 0 &&
           s.min_dist == s.min_dist && s.d_threshold == s.d_threshold;
}

// drawRandomPlaneSample for every hypothesis, in order, from the stream of `seed`
void walk(svh_plane* p, uint32_t seed, const plane::Params& c, const float* lu, const float* lv, int32_t n,
          int32_t* samples, std::vector<int32_t>& draws) {
    if (!p->raw_ok || p->raw_seed != seed) {
        p->rs.seed(seed);
        p->raw.clear();
        p->raw_seed = seed;
        p->raw_ok = true;
    }
    size_t pos = 0;
    auto next = [&]() -> int32_t {
        if (pos == p->raw.size()) p->raw.push_back((int32_t)p->rs.next());
        return p->raw[pos++];
    };
    draws.resize((size_t)c.num_samples);
    for (int32_t h = 0; h < c.num_samples; h++) {
        int32_t ind[3] = {0, 0, 0}, consumed = 0;
        const int cnt = plane::draw_sample(next, lu, lv, n, c.max_draws, c.min_dist, ind, &consumed);
        samples[4 * h + 0] = cnt;
        for (int k = 0; k < 3; k++) samples[4 * h + 1 + k] = k < cnt ? ind[k] : 0;
        draws[(size_t)h] = consumed;
    }
    if (p->raw.size() > RAW_KEEP) {
        std::vector<int32_t>().swap(p->raw);
        p->raw_ok = false;
    }
}

// the whole call for n maps; res[i] receives what object i is to hold.  D: host map (n == 1) or device maps.
int run(svh_plane* const* objs, const float* const* D, bool on_device, int32_t n, int32_t width, int32_t height,
        int32_t step, float f, float cu, float cv, float base, const uint32_t* seeds, std::vector<Result>& res) {
    svh_plane* w = objs[0];   // its stream and buffers carry the call
    const double t_start = now_ms();
    const plane::Params c = core_params(w->prm, width, height);
    const plane::Lattice L = plane::lattice_of(c, width, height);
    const int64_t cells64 = (int64_t)L.nu * L.nv;
    if (cells64 > (1 << 26)) return svh::fail(SVH_ERR_BAD_ARG, "svh_plane_estimate: the lattice has too many cells");
    const int32_t cells = (int32_t)cells64, S = c.num_samples;
    res.assign((size_t)n, Result());
    for (int32_t i = 0; i < n; i++) res[i].pitch = objs[i]->res.pitch;   // kept unless the road branch sets it
    if (cells == 0) {
        for (int32_t i = 0; i < n; i++) res[i].status = SVH_PLANE_NO_POINTS;
        return SVH_OK;
    }
    ActiveCaller active;
    const Layout lay((size_t)n, (size_t)cells, (size_t)S);
    // a host map travels as the rows the lattice reads: v0 .. the last lattice row
    const int32_t row0 = on_device ? 0 : L.v0;
    const int32_t v_last = L.v0 + (L.nv - 1) * L.step_size;
    const size_t map_floats = on_device ? 0 : (size_t)(v_last - row0) * (size_t)step + (size_t)width;
    int rc = ensure(w, lay.end, 4 * map_floats);
    if (rc) return rc;
    uint8_t *d = w->d_all, *h = w->h_all;
    const float** h_maps = reinterpret_cast<const float**>(h + lay.maps);
    if (on_device) {
        for (int32_t i = 0; i < n; i++) h_maps[i] = D[i];
    } else {
        memcpy(w->h_map, D[0] + (size_t)row0 * (size_t)step, 4 * map_floats);
        h_maps[0] = w->d_map;
    }
    PlaneDev P;
    P.maps = reinterpret_cast<const float* const*>(d + lay.maps);
    P.n_list = reinterpret_cast<int32_t*>(d + lay.n_list);
    P.lu = reinterpret_cast<float*>(d + lay.lu);
    P.lv = reinterpret_cast<float*>(d + lay.lv);
    P.ld = reinterpret_cast<float*>(d + lay.ld);
    P.samples = reinterpret_cast<const int32_t*>(d + lay.samples);
    P.planes = reinterpret_cast<double*>(d + lay.planes);
    P.counts = reinterpret_cast<int32_t*>(d + lay.counts);
    P.sel = reinterpret_cast<int32_t*>(d + lay.sel);
    P.inl = reinterpret_cast<int32_t*>(d + lay.inl);
    P.cap = cells;
    P.S = S;

    // ---- phase 0: the list
    if (w->timing) (void)hipEventRecord(w->ev[0], w->stream);
    if (!on_device) PLANE_TRY(copy, hipMemcpyAsync(w->d_map, w->h_map, 4 * map_floats, hipMemcpyHostToDevice, w->stream));
    PLANE_TRY(copy, hipMemcpyAsync(d + lay.maps, h + lay.maps, 8 * (size_t)n, hipMemcpyHostToDevice, w->stream));
    planelaunch_grid(w->stream, P, n, L, step, row0);
    PLANE_TRY(launch, hipGetLastError());
    PLANE_TRY(copy, hipMemcpyAsync(h + lay.n_list, d + lay.n_list, lay.sel - lay.n_list, hipMemcpyDeviceToHost, w->stream));
    if (w->timing) (void)hipEventRecord(w->ev[1], w->stream);
    PLANE_TRY(wait, (hipError_t)wait_stream(w->stream));
    const double t_list = now_ms();
    const int32_t* n_list = reinterpret_cast<const int32_t*>(h + lay.n_list);
    const float* lu = reinterpret_cast<const float*>(h + lay.lu);
    const float* lv = reinterpret_cast<const float*>(h + lay.lv);
    const float* ld = reinterpret_cast<const float*>(h + lay.ld);
    int32_t max_n = 0;
    for (int32_t i = 0; i < n; i++) {
        if (n_list[i] < 0 || n_list[i] > cells)
            return svh::fail(SVH_ERR_HIP, "PlaneEstimation: the device returned an impossible list length");
        max_n = std::max(max_n, n_list[i]);
    }

    // ---- phase 1: the draws
    int32_t* h_samples = reinterpret_cast<int32_t*>(h + lay.samples);
    for (int32_t i = 0; i < n; i++) {
        const int32_t ni = n_list[i];
        if (ni == 0) {
            res[i].status = SVH_PLANE_NO_POINTS;
            memset(h_samples + 4 * (size_t)S * i, 0, 16 * (size_t)S);
            continue;
        }
        const size_t o = (size_t)i * cells;
        walk(objs[i], seeds[i], c, lu + o, lv + o, ni, h_samples + 4 * (size_t)S * i, res[i].draws);
        res[i].list.resize(3 * (size_t)ni);
        for (int32_t k = 0; k < ni; k++) {
            res[i].list[3 * (size_t)k + 0] = lu[o + k];
            res[i].list[3 * (size_t)k + 1] = lv[o + k];
            res[i].list[3 * (size_t)k + 2] = ld[o + k];
        }
    }
    const double t_walk = now_ms();
    double t_vote = t_walk;
    if (max_n > 0) {
        // ---- phase 2: fits, votes, winner
        if (w->timing) (void)hipEventRecord(w->ev[2], w->stream);
        PLANE_TRY(copy, hipMemcpyAsync(d + lay.samples, h + lay.samples, 16 * (size_t)S * n, hipMemcpyHostToDevice, w->stream));
        PLANE_TRY(copy, hipMemsetAsync(d + lay.counts, 0, 4 * (size_t)S * n, w->stream));
        planelaunch_vote(w->stream, P, n, max_n, c.d_threshold);
        PLANE_TRY(launch, hipGetLastError());
        PLANE_TRY(copy, hipMemcpyAsync(h + lay.sel, d + lay.sel, lay.end - lay.sel, hipMemcpyDeviceToHost, w->stream));
        if (w->timing) (void)hipEventRecord(w->ev[3], w->stream);
        PLANE_TRY(wait, (hipError_t)wait_stream(w->stream));
        t_vote = now_ms();

        // ---- phase 3: refit in list order, planeDsiTo3d
        const int32_t* sel = reinterpret_cast<const int32_t*>(h + lay.sel);
        const double* planes = reinterpret_cast<const double*>(h + lay.planes);
        const int32_t* counts = reinterpret_cast<const int32_t*>(h + lay.counts);
        const int32_t* inl = reinterpret_cast<const int32_t*>(h + lay.inl);
        for (int32_t i = 0; i < n; i++) {
            const int32_t ni = n_list[i];
            if (ni == 0) continue;
            Result& r = res[i];
            const size_t o = (size_t)i * cells;
            const int32_t best = sel[2 * i], nin = sel[2 * i + 1];
            if (best < -1 || best >= S || nin < 0 || nin > ni || (best < 0 && nin != 0) ||
                (best >= 0 && counts[(size_t)i * S + best] != nin))
                return svh::fail(SVH_ERR_HIP, "PlaneEstimation: the device returned an impossible winner");
            r.planes.assign(planes + 3 * (size_t)S * i, planes + 3 * (size_t)S * (i + 1));
            r.votes.assign(counts + (size_t)S * i, counts + (size_t)S * (i + 1));
            r.best = best;
            r.inliers.assign(inl + o, inl + o + nin);
            if (nin > 3) {
                plane::Sums s;
                plane::sums_zero(s);
                for (int32_t k = 0; k < nin; k++) {
                    const int32_t j = inl[o + k];
                    if (j < 0 || j >= ni)
                        return svh::fail(SVH_ERR_HIP, "PlaneEstimation: the device returned an impossible inlier");
                    plane::sums_add(s, lu[o + j], lv[o + j], ld[o + j]);
                }
                plane::sums_solve(s, r.plane_d);
                if (plane::plane_to_3d(r.plane_d, f, cu, cv, base, r.plane_e, r.H, &r.pitch)) {}
                r.status = SVH_OK;
            } else {
                for (int k = 0; k < 3; k++) r.plane_d[k] = planes[3 * ((size_t)S * i + (S - 1)) + k];
                r.status = SVH_PLANE_FEW_INLIERS;
            }
        }
    }
    if (w->timing) {
        const double t_end = now_ms();
        float a = 0, b = 0;
        w->ms[0] = t_list - t_start;
        w->ms[1] = t_walk - t_list;
        w->ms[2] = t_vote - t_walk;
        w->ms[3] = t_end - t_vote;
        w->ms[4] = t_end - t_start;
        w->ms[5] = hipEventElapsedTime(&a, w->ev[0], w->ev[1]) == hipSuccess ? a : 0;
        w->ms[6] = max_n > 0 && hipEventElapsedTime(&b, w->ev[2], w->ev[3]) == hipSuccess ? b : 0;
    }
    return SVH_OK;
}

int run_guarded(svh_plane* const* objs, const float* const* D, bool on_device, int32_t n, int32_t width,
                int32_t height, int32_t step, float f, float cu, float cv, float base, const uint32_t* seeds,
                std::vector<Result>& res) {
    const int rc = run(objs, D, on_device, n, width, height, step, f, cu, cv, base, seeds, res);
    if (rc == SVH_ERR_HIP && objs[0]->stream) {
        (void)hipSetDevice(objs[0]->device);
        (void)hipStreamSynchronize(objs[0]->stream);   // nothing of this call is in flight when the caller goes on
    }
    return rc;
}

}  // namespace

extern "C" {

void svh_plane_params_default(svh_plane_params* p) {
    if (!p) return;
    p->num_samples = 5000;
    p->step_size = 5;
    p->max_draws = 1000;
    for (int i = 0; i < 4; i++) p->roi[i] = -1;
    p->min_dist = 50;
    p->d_threshold = 5;
}

svh_plane* svh_plane_create(const svh_plane_params* prm) {
    svh::ensure_init();
    svh_plane_params d;
    svh_plane_params_default(&d);
    if (prm) d = *prm;
    if (!params_ok(d)) {
        svh::fail(SVH_ERR_BAD_ARG, "svh_plane_create: bad parameters");
        return nullptr;
    }
    svh_plane* p = new svh_plane();
    p->prm = d;
    int nd = 0;
    if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0) (void)hipGetDevice(&p->device);
    return p;
}

void svh_plane_destroy(svh_plane* p) {
    if (!p) return;
    if (p->stream) {
        (void)hipSetDevice(p->device);
        (void)hipStreamSynchronize(p->stream);
        (void)hipStreamDestroy(p->stream);
    }
    for (int i = 0; i < 4; i++)
        if (p->ev[i]) (void)hipEventDestroy(p->ev[i]);
    delete p;
}

int64_t svh_plane_release(svh_plane* p) {
    if (!p) return 0;
    auto payload = [](size_t cap) { return cap ? cap - 16 : 0; };   // (without the slack every buffer carries)
    const int64_t bytes = (int64_t)(2 * payload(p->d_all.cap) + 2 * payload(p->d_map.cap) + 4 * p->raw.capacity());
    if (p->stream) {
        (void)hipSetDevice(p->device);
        (void)hipStreamSynchronize(p->stream);
    }
    release_buffers(p);
    std::vector<int32_t>().swap(p->raw);
    p->raw_ok = false;
    return bytes;
}

int32_t svh_plane_estimate(svh_plane* p, const float* D, int32_t d_on_device, int32_t width, int32_t height,
                           int32_t step, float f, float cu, float cv, float base, uint32_t seed) {
    if (!p || !D || width < 1 || height < 1 || step < width)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_plane_estimate: bad arguments");
    std::vector<Result> res;
    const int rc = run_guarded(&p, &D, d_on_device != 0, 1, width, height, step, f, cu, cv, base, &seed, res);
    if (rc < 0) return rc;
    p->res = std::move(res[0]);
    return p->res.status;
}

int32_t svh_plane_estimate_batch(svh_plane* const* p, const float* const* D, int32_t n, int32_t width,
                                 int32_t height, int32_t step, float f, float cu, float cv, float base,
                                 const uint32_t* seeds, int32_t* status) {
    if (!p || !D || !seeds || n < 1 || n > 4096 || width < 1 || height < 1 || step < width)
        return svh::fail(SVH_ERR_BAD_ARG, "svh_plane_estimate_batch: bad arguments");
    bool uniform = true;
    const int32_t bad = check_batch(p, n, "object", &uniform, [&](int i) {
        return memcmp(&p[i]->prm, &p[0]->prm, sizeof(svh_plane_params)) == 0;
    });
    if (bad) return bad;
    if (!uniform) return svh::fail(SVH_ERR_BAD_ARG, "svh_plane_estimate_batch: the objects differ in parameters or device");
    for (int32_t i = 0; i < n; i++)
        if (!D[i]) return svh::fail(SVH_ERR_BAD_ARG, "svh_plane_estimate_batch: null map");
    std::vector<Result> res;
    const int rc = run_guarded(p, D, true, n, width, height, step, f, cu, cv, base, seeds, res);
    if (rc < 0) return rc;
    for (int32_t i = 0; i < n; i++) {
        p[i]->res = std::move(res[i]);
        if (status) status[i] = p[i]->res.status;
    }
    return SVH_OK;
}

void svh_plane_get_plane_dsi(svh_plane* p, double abc[3]) {
    for (int i = 0; i < 3 && p && abc; i++) abc[i] = p->res.plane_d[i];
}
void svh_plane_get_plane_euclidean(svh_plane* p, double abc[3]) {
    for (int i = 0; i < 3 && p && abc; i++) abc[i] = p->res.plane_e[i];
}
void svh_plane_get_transformation(svh_plane* p, double H[16]) {
    for (int i = 0; i < 16 && p && H; i++) H[i] = p->res.H[i];
}
float svh_plane_get_pitch(svh_plane* p) { return p ? p->res.pitch : 0.f; }

int32_t svh_plane_get_list(svh_plane* p, float* uvd, int32_t cap) {
    if (!p) return 0;
    const int32_t n = (int32_t)(p->res.list.size() / 3), k = std::min(n, cap);
    if (uvd && k > 0) memcpy(uvd, p->res.list.data(), 12 * (size_t)k);
    return n;
}

int32_t svh_plane_get_hypotheses(svh_plane* p, double* planes, int32_t* draws, int32_t* votes, int32_t cap) {
    if (!p) return 0;
    const int32_t n = (int32_t)p->res.votes.size(), k = std::min(n, cap);
    if (k > 0) {
        if (planes) memcpy(planes, p->res.planes.data(), 24 * (size_t)k);
        if (draws) memcpy(draws, p->res.draws.data(), 4 * (size_t)k);
        if (votes) memcpy(votes, p->res.votes.data(), 4 * (size_t)k);
    }
    return n;
}

int32_t svh_plane_get_best(svh_plane* p, int32_t* best, int32_t* inliers, int32_t cap) {
    if (!p) return 0;
    if (best) *best = p->res.best;
    const int32_t n = (int32_t)p->res.inliers.size(), k = std::min(n, cap);
    if (inliers && k > 0) memcpy(inliers, p->res.inliers.data(), 4 * (size_t)k);
    return n;
}

void svh_plane_set_timing(svh_plane* p, int32_t on) {
    if (p) p->timing = on != 0;
}

int32_t svh_plane_get_timing(svh_plane* p, double* ms7) {
    if (!p) return 0;
    for (int i = 0; i < 7 && ms7; i++) ms7[i] = p->ms[i];
    return 7;
}

}  // extern "C"

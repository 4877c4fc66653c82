// The alignment layer of stereo-vision_amd/csrc/grid_align_core.h -- the subs of points at the limits of the float-to-integer
// conversions, the shifts of negative values, the bilinear sample at the window's edges, the volume and its key, the correction --
// compiled by the host compiler alone, as a program of its own: tests/test_grid_align.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all, so a read beyond a plane, a conversion out of range or a signed overflow
// ends the run, and compares what it writes with tests/grid_align_ref.py.
//
//   grid_align_check job.bin
//   job.bin: int32 nx, nz, oa, ob; rot_den, rot_n, trans_n, min_scan; n_pts, n_subs, use_subs, Pa, Pb; k, ta, tb (of the correction);
//            float reach, range, cell, x0, z0, step, clearance, pivot[3], T[12]; then STATE (nx * nz bytes), the points (4 * n_pts float)
//            and the subs (2 * n_subs int32).  With use_subs the frame is the subs about (Pa, Pb), else the points about the pivot
//   stdout:  F (nx * nz bytes); int64 n_scan, n_points; the scan (2 * n_scan int32); the record (8 int32); the volume unless the
//            status is FEW; the rotation table (2 * (2 K + 1) int32); M (16 double).
//            Exit status 3: the parameters or the pivot are refused, nothing is written.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "grid_align_core.h"

using namespace svh;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[16];
    float fl[22];
    if (fread(head, 4, 16, f) != 16 || fread(fl, 4, 22, f) != 22) return 2;
    grid::Params p{};
    p.nx = head[0], p.nz = head[1], p.oa = head[2], p.ob = head[3];
    p.cell = fl[2], p.x0 = fl[3], p.z0 = fl[4], p.step = fl[5], p.clearance = fl[6];
    p.min_points = 1, p.drop = 0.f, p.h_lo = 0.f, p.h_hi = 1.f;
    for (int i = 0; i < 12; i++) p.T[i] = fl[10 + i];
    grid::AlignParams a{fl[0], fl[1], head[4], head[5], head[6], head[7], 0, 0};
    const int32_t n_pts = head[8], n_subs = head[9];
    if (!grid::params_ok(p) || n_pts < 0 || n_subs < 0) return 2;
    const size_t cells = (size_t)p.nx * (size_t)p.nz;
    // exact-size buffers: the sanitizer sees every byte beyond them
    std::vector<uint8_t> state(cells), F(cells);
    std::vector<float> pts(4 * (size_t)n_pts);
    std::vector<int32_t> subs(2 * (size_t)n_subs);
    if (fread(state.data(), 1, cells, f) != cells || fread(pts.data(), 4, pts.size(), f) != pts.size() ||
        fread(subs.data(), 4, subs.size(), f) != subs.size())
        return 2;
    fclose(f);
    if (!grid::align_derive(a, p.cell)) return 3;
    int32_t Pa = head[11], Pb = head[12];
    if (head[10]) {
        for (int32_t v : subs)
            if (v <= -grid::ALIGN_SUB_LIMIT || v >= grid::ALIGN_SUB_LIMIT) return 3;
        if (Pa <= -grid::ALIGN_SUB_LIMIT || Pa >= grid::ALIGN_SUB_LIMIT || Pb <= -grid::ALIGN_SUB_LIMIT || Pb >= grid::ALIGN_SUB_LIMIT) return 3;
    } else if (!grid::align_pivot(p, fl[7], fl[8], fl[9], &Pa, &Pb)) {
        return 3;
    }
    grid::align_field_window(a.reach_cells, p.nx, p.nz, state.data(), F.data());
    std::vector<int32_t> scan;
    const int64_t kept = head[10] ? grid::align_scan_subs(a.Rg, Pa, Pb, subs.data(), n_subs, &scan) : grid::align_scan_points(p, a.Rg, Pa, Pb, pts.data(), n_pts, &scan);
    const int64_t counts[2] = {(int64_t)(scan.size() / 2), kept};
    std::vector<int32_t> volume((size_t)grid::align_volume_size(a.rot_n, a.trans_n));
    int32_t rec[grid::ALIGN_REC];
    grid::align_window(a, p.nx, p.nz, p.oa, p.ob, F.data(), Pa, Pb, scan.data(), counts[0], volume.data(), rec);
    int32_t rot[2 * grid::ALIGN_MAX_ROTS];
    grid::align_rot_table(a.rot_den, a.rot_n, rot);
    if (rot[2 * a.rot_n] != grid::ALIGN_ROT || rot[2 * a.rot_n + 1] != 0) return 1;   // k = 0 is the identity
    for (int32_t ra = -4 * grid::ALIGN_MAX_RG; ra <= 4 * grid::ALIGN_MAX_RG; ra += 4 * grid::ALIGN_MAX_RG)
        for (int32_t rb = -4 * grid::ALIGN_MAX_RG; rb <= 4 * grid::ALIGN_MAX_RG; rb += 4 * grid::ALIGN_MAX_RG) {
            int32_t qa, qb;
            grid::align_turn(grid::ALIGN_ROT, 0, ra, rb, &qa, &qb);
            if (qa != ra || qb != rb) return 1;
            for (int32_t i = 0; i <= 2 * a.rot_n; i++) grid::align_turn(rot[2 * i], rot[2 * i + 1], ra, rb, &qa, &qb);   // the extremes of the products
        }
    double M[16];
    const float pivot[3] = {fl[7], fl[8], fl[9]};
    grid::align_correction(p, a.rot_den, head[13], head[14], head[15], pivot, M);
    fwrite(F.data(), 1, cells, stdout);
    fwrite(counts, 8, 2, stdout);
    if (!scan.empty()) fwrite(scan.data(), 4, scan.size(), stdout);
    fwrite(rec, 4, grid::ALIGN_REC, stdout);
    if (rec[grid::AR_STATUS] != grid::ALIGN_FEW) fwrite(volume.data(), 4, volume.size(), stdout);
    fwrite(rot, 4, 2 * (size_t)(2 * a.rot_n + 1), stdout);
    fwrite(M, 8, 16, stdout);
    return 0;
}

"""CPU: the contract of the ground grid's archive (include/svh_grid_archive.h: svh_grid_set_archive, svh_grid_get_region, ...).
tests/grid_archive_ref.py restates stereo-vision_amd/csrc/grid_archive_core.h in numpy and plain Python integers; this file pins the
restatement with cases derived by hand, compares the header itself with it -- evaluated on the host by the library's test entries
svh_test_grid_archive_key and svh_test_grid_archive_strip --, and checks what needs no device: the refusals, the exports and the
property the layer exists for, on the restatement.  Every comparison is exact.

tests/test_grid_archive_gpu.py compares the device with the same header and restatement.

Planes are indexed [ib, ia]."""
import itertools

import numpy as np
import pytest

import grid_archive_ref as AR
import grid_dyn_ref as DR
import grid_ref as R
import test_grid as TG
import test_grid_dyn as TD

F = np.float32
CELL = TD.CELL
WINDOWS = [(40, 24), (16, 16)]
OFFSETS = [(0, 0), (-53, 7), (9, -70)]   # on both sides of 0, tiles straddling every edge


@pytest.fixture(scope="module")
def G():
    from svhip import grid
    grid._bind()
    return grid


def steps(n):
    return [1, 15, 16, 17, n - 1, n, n + 1, 3 * n]


def scrolls(nx, nz):
    """the scroll list of the contract: every step of both axes with each sign, alone and diagonal"""
    A, B = steps(nx), steps(nz)
    out = [(s * a, 0) for a in A for s in (1, -1)] + [(0, s * b) for b in B for s in (1, -1)]
    for k in (0, 3):
        for i, a in enumerate(A):
            b = B[(i + k) % len(B)]
            out += [(sa * a, sb * b) for sa, sb in itertools.product((1, -1), repeat=2)]
    return [d for d in out if d != (0, 0)]   # n - 1 is 0 in a window of one cell


# ---- the restatement by hand ----------------------------------------------------------------------------------------------------
def test_tiles_and_keys_by_hand():
    assert [AR.tile_of(g) for g in (-17, -16, -1, 0, 15, 16)] == [-2, -1, -1, 0, 0, 1]
    assert AR.tile_index(0, 0) == 0 and AR.tile_index(15, 0) == 15 and AR.tile_index(0, 1) == 16 and AR.tile_index(-1, -1) == 255
    assert AR.tile_index(-16, -17) == 15 * 16 + 0 and AR.tile_index(17, -1) == 15 * 16 + 1
    assert AR.tile_key(0, 0) == (2 ** 20 << 32) | 2 ** 20 and AR.tile_key(-1, 2) == ((2 ** 20 + 2) << 32) | (2 ** 20 - 1)
    assert AR.tile_key(-2 ** 16, -2 ** 16) == ((2 ** 20 - 2 ** 16) << 32) | (2 ** 20 - 2 ** 16) and AR.tile_key(2 ** 16 - 1, 0) != AR.TILE_NONE
    assert AR.tile_key(5, -3) < AR.tile_key(-7, -2) < AR.tile_key(-6, -2), "keys ascend by (tb, ta)"
    assert [AR.table_size(n) for n in (0, 1, 2, 3, 16384, 2 ** 20)] == [2, 2, 4, 8, 32768, 2 ** 21]
    assert AR.PAGE_BYTES == 11264


def test_strips_by_hand():
    # 4 x 3, one column up: the low column leaves, rows 0..2
    assert AR.strip(4, 3, 1, 0).tolist() == [[0, 0], [0, 1], [0, 2]]
    assert AR.strip(4, 3, -1, 0).tolist() == [[3, 0], [3, 1], [3, 2]]
    # diagonal: the column, then the row without the corner
    assert AR.strip(4, 3, 1, 1).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [2, 0], [3, 0]]
    assert AR.strip(4, 3, -2, -1).tolist() == [[2, 0], [3, 0], [2, 1], [3, 1], [2, 2], [3, 2], [0, 2], [1, 2]]
    assert len(AR.strip(4, 3, 4, 0)) == 12 and len(AR.strip(4, 3, 1, -3)) == 12 and AR.strip(4, 3, 0, 7).tolist()[:5] == [[0, 0], [1, 0], [2, 0], [3, 0], [0, 1]]


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_strips_are_the_leaving_and_entering_sets(nx, nz):
    """for every scroll of the list: the strip holds each leaving cell exactly once, and the strip of the opposite displacement in the
    new window each entering cell"""
    for (oa, ob), (da, db) in itertools.product(OFFSETS[:2], scrolls(nx, nz)):
        out = AR.strip(nx, nz, da, db) + (oa, ob)
        assert len(out) == len({tuple(c) for c in out.tolist()}) and {tuple(c) for c in out.tolist()} == AR.leaving_set(nx, nz, oa, ob, da, db), (da, db)
        inn = AR.strip(nx, nz, -da, -db) + (oa + da, ob + db)
        assert len(inn) == len({tuple(c) for c in inn.tolist()}) and {tuple(c) for c in inn.tolist()} == AR.entering_set(nx, nz, oa, ob, da, db), (da, db)


# ---- the header against the restatement -----------------------------------------------------------------------------------------
def test_header_keys(G):
    rng = np.random.default_rng(1)
    edge = np.array([-2 ** 20 + 1, -17, -16, -15, -1, 0, 1, 15, 16, 17, 2 ** 20 - 1])
    ga = np.concatenate([np.repeat(edge, len(edge)), rng.integers(-2 ** 20 + 1, 2 ** 20, 500)])
    gb = np.concatenate([np.tile(edge, len(edge)), rng.integers(-2 ** 20 + 1, 2 ** 20, 500)])
    key, tile, index, _ = G.core_archive_key(ga, gb)
    for k in range(len(ga)):
        a, b = int(ga[k]), int(gb[k])
        assert int(key[k]) == AR.tile_key(AR.tile_of(a), AR.tile_of(b)) != AR.TILE_NONE
        assert tuple(tile[k]) == (AR.tile_of(a), AR.tile_of(b)) and int(index[k]) == AR.tile_index(a, b), (a, b)
    for n in (0, 1, 2, 3, 5, 1000, 16384, 16385, 2 ** 20):
        assert G.core_archive_key([], [], n)[3] == AR.table_size(n) >= 2 * n
    with pytest.raises(G.SvhError):
        G.core_archive_key([2 ** 20], [0])


@pytest.mark.parametrize("nx,nz", WINDOWS + [(1, 1), (17, 1), (1, 33)])
def test_header_strips(G, nx, nz):
    for da, db in scrolls(nx, nz):
        got = G.core_archive_strip(nx, nz, da, db)
        assert got.tolist() == AR.strip(nx, nz, da, db).tolist(), (da, db)


# ---- the property, on the restatement -------------------------------------------------------------------------------------------
def scene(ref, rng, n):
    """n random points over the window as it stands: ground, tall things, overhead points, drops"""
    P = ref.P
    ia, ib = rng.uniform(0, P.nx, n), rng.uniform(0, P.nz, n)
    kind = rng.random(n)
    h = np.where(kind < 0.3, rng.uniform(0.21, 1.9, n), np.where(kind < 0.9, rng.uniform(-0.05, 0.15, n), np.where(kind < 0.95, 2.5, -1.0)))
    return np.stack([(ref.oa + ia) * CELL, 1.5 - h, (ref.ob + ib) * CELL, rng.uniform(0, 1, n)], 1).astype(F)


def centre(ref, ia, ib, h=1.5):
    return [(ref.oa + ia + 0.5) * CELL, 1.5 - h, (ref.ob + ib + 0.5) * CELL]


def everything(ref):
    out = ref.planes()
    out.update(ref.local_planes())
    return out


def same(a, b):
    return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def filled(G, nx, nz, off, max_tiles, seed=3):
    P, _ = TG.both(G, **TD.hand_kw(nx=nx, nz=nz))
    ref = AR.Grid(P, None, max_tiles)
    ref.scroll(*off) if off != (0, 0) else None
    ref.archive_clear()
    rng = np.random.default_rng(seed)
    ref.add_from(scene(ref, rng, 6 * nx * nz), centre(ref, nx // 2, 0))
    return ref


@pytest.mark.parametrize("nx,nz", WINDOWS)
def test_away_and_back_equals_never_moved(G, nx, nz):
    ref = filled(G, nx, nz, OFFSETS[1], 64)
    want = everything(ref)
    assert (want["count"] > 0).sum() > nx * nz // 2
    for da, db in scrolls(nx, nz)[::3]:
        ref.scroll(da, db)
        ref.scroll(-da, -db)
        assert same(everything(ref), want), (da, db)
    st = ref.archive_stats()
    assert st["lost"] == 0 and st["refused"] == 0 and st["stored"] == st["restored"] > 0 and 0 < st["pages"] <= 12
    # without the layer the strips come back empty
    off = filled(G, nx, nz, OFFSETS[1], 0)
    off.scroll(1, 0).scroll(-1, 0)
    got = everything(off)
    assert not same(got, want) and (got["count"][:, 0] == 0).all() and np.array_equal(got["count"][:, 1:], want["count"][:, 1:])


def test_capacity_by_hand(G):
    """16 x 16 at offsets (8, 8): the window straddles the tiles (0,0) (1,0) (0,1) (1,1); max_tiles 2"""
    P, _ = TG.both(G, **TD.hand_kw(nx=16, nz=16))
    ref = AR.Grid(P, None, 2)
    ref.scroll(8, 8)
    ia, ib = np.meshgrid(np.arange(16), np.arange(16))
    pts = TD.at(ia.ravel() + 8, ib.ravel() + 8, 0.1)
    ref.add(np.concatenate([pts, pts]))
    full = everything(ref)
    # a jump away needs 4 tiles with 2 free: none is paged, 256 cells are lost, the window comes back empty
    ref.scroll(100, 0).scroll(-100, 0)
    assert ref.archive_stats() == dict(pages=0, max_tiles=2, stored=0, restored=0, lost=256, refused=1)
    assert (everything(ref)["count"] == 0).all()
    # one column of the low tiles' cells: rows 8..15 are tile (0, 0), rows 16..23 tile (0, 1): 2 tiles, 2 free
    ref.add(np.concatenate([pts, pts]))
    ref.scroll(1, 0)
    assert ref.archive_stats() == dict(pages=2, max_tiles=2, stored=16, restored=0, lost=256, refused=1)
    assert ref.archive_tiles().tolist() == [[0, 0], [0, 1]]
    # eight more columns: the columns 9..15 belong to the paged tiles, column 16 to the tiles (1, 0) and (1, 1), which are refused; the
    # paged ones are stored all the same
    ref.scroll(8, 0)
    assert ref.archive_stats() == dict(pages=2, max_tiles=2, stored=16 + 7 * 16, restored=0, lost=256 + 16, refused=2)
    ref.scroll(-9, 0)
    got = everything(ref)
    assert np.array_equal(got["count"][:, :8], full["count"][:, :8]) and (got["count"][:, 8] == 0).all() and np.array_equal(got["count"][:, 9:], full["count"][:, 9:])
    assert ref.archive_stats()["restored"] == 8 * 16   # the columns 8..15; column 16 has no page and the columns 17..23 never left
    # trim to a box that meets tile (0, 1) alone; its page is usable again
    ref.archive_trim(0, 16, 40, 16)
    assert ref.archive_tiles().tolist() == [[0, 1]] and ref.archive_stats()["pages"] == 1
    ref.set_archive(2)
    assert ref.archive_stats()["pages"] == 1
    ref.set_archive(3)
    assert ref.archive_stats() == dict(pages=0, max_tiles=3, stored=0, restored=0, lost=0, refused=0)


def test_region_on_the_restatement(G):
    ref = filled(G, 40, 24, OFFSETS[2], 64)
    ref.scroll(30, 10)
    oa, ob = ref.window()
    box = ref.region(oa, ob, 40, 24)
    assert same({k: box[k] for k in everything(ref)}, everything(ref))
    assert np.array_equal(ref.render_region(oa, ob, 40, 24), ref.render_local()) and np.array_equal(ref.render_region(oa, ob, 40, 24, 1), ref.render(1))
    wide = ref.region(oa - 30, ob - 10, 70, 34)
    assert (wide["count"][:10, :30] > 0).sum() > 100 and same({k: wide[k][10:, 30:] for k in everything(ref)}, everything(ref))
    with pytest.raises(ValueError):
        ref.region(0, 0, 0, 1)


# ---- what needs no device -------------------------------------------------------------------------------------------------------
def test_exports_and_refusals_without_a_device(G):
    assert (G.REGION_GRID, G.REGION_LOCAL, G.RENDER_LOCAL) == (0, 1, 3) and G.ARCHIVE_STATS == AR.STATS
    assert (G.ARCHIVE_TILE, G.ARCHIVE_MAX_TILES, G.ARCHIVE_DEFAULT_TILES, G.ARCHIVE_PAGE_BYTES) == (AR.TILE, AR.MAX_TILES, AR.DEFAULT_TILES, AR.PAGE_BYTES)
    assert G.default_archive().max_tiles == AR.DEFAULT_TILES
    L = G._bind()
    buf = np.zeros(8, np.int64)
    p = G.default_archive()
    import ctypes as C
    assert L.svh_grid_set_archive(None, C.byref(p)) == G.ERR_BAD_ARG and L.svh_grid_get_archive(None, C.byref(p)) == G.ERR_BAD_ARG
    assert L.svh_grid_get_archive_stats(None, buf.ctypes.data) == G.ERR_BAD_ARG and L.svh_grid_archive_clear(None) == G.ERR_BAD_ARG
    assert L.svh_grid_archive_trim(None, 0, 0, 1, 1) == G.ERR_BAD_ARG and L.svh_grid_archive_tiles(None, buf.ctypes.data, 1, buf.ctypes.data) == G.ERR_BAD_ARG
    assert L.svh_grid_get_region(None, 0, 0, 0, 0, 1, 1, buf.ctypes.data, 0) == G.ERR_BAD_ARG
    assert L.svh_grid_render_region(None, 3, 0, 0, 1, 1, buf.ctypes.data, 0) == G.ERR_BAD_ARG and "svh_grid_render_region" in G.last_error()


def test_the_header_under_the_sanitizers(tmp_path):
    """tests/cxx/grid_archive_check.cpp: a program of its own over the header's host functions, nothing loaded into Python"""
    import os
    import subprocess
    import helpers as H
    exe = str(tmp_path / "grid_archive_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(H.PKG, "csrc"), "-o", exe, os.path.join(H.ROOT, "tests", "cxx", "grid_archive_check.cpp")])
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    assert r.stdout.decode().startswith("archive core ok, ") and int(r.stdout.decode().split()[3]) > 3000

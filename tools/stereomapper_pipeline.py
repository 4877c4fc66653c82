#!/usr/bin/env python3
"""The data path of stereomapper on the GPU, frame by frame, from a KITTI raw drive:

    drive (include/svh_kitti.h)  ->  VisualOdometryStereo::process  (pose, gain; include/svh.h svh_vo_*)
                                 ->  Elas::process                  (D1 on the device; svh_elas_*)
                                 ->  map fusion                     (point lists; include/svh_map.h)
                                 ->  View3D::addCamera / addPoints  (the global map, on the device; include/svh_view.h)
                                 ->  View2D x 3                     (the image panes, on the device; include/svh_view2d.h)

i.e. what ReadFromFilesThread, VisualOdometryThread, StereoThread and MainDialog::onNewDisparityMapArrived do between
them (readfromfilesthread.cpp:25-112, visualodometrythread.cpp:95-140, stereothread.cpp:62-170, maindialog.cpp:602-606),
without the GUI.  Usage:

    python tools/stereomapper_pipeline.py [--unrectified] [--resident] [--normalize] [--render DIR]
                                          [--panes DIR [--pane-size WxH]] [--lockstep K]
                                          [--thin S [--thin-every N]] [--ply FILE]
                                          [--grid DIR [--grid-cell S] [--grid-size NXxNZ] [--level]]
                                          [--grid-local DIR [--grid-cell S] [--grid-size NXxNZ]]
                                          [--grid-cost DIR [--grid-slope S] [--grid-inscribed M] [--grid-inflate M]]
                                         [--grid-plan DIR [--grid-goal-ahead M]]
                                         [--grid-pose DIR [--grid-pose-params TURN,REVERSE,SPIN]]
                                         [--grid-roll DIR [--grid-roll-vehicle FRONT,REAR,HALFWIDTH] [--grid-roll-unknown N]]
                                          [--grid-frontiers DIR [--grid-unexplored unseen|seen|both] [--grid-frontier-min N]]
                                          [--grid-explore DIR [--grid-explore-range M]]
                                          [--grid-align DIR [--grid-align-apply] [--grid-align-window K,W]]
                                          [--grid-dynamic DIR [--grid-dynamic-params CLEAR,THROUGH,MARGIN,AGE]]
                                         [--grid-archive DIR [--grid-archive-tiles N]]
                                          [--grid-objects DIR [--grid-objects-params MIN,MAX,HEIGHT,GATE,MISSED]]
                                          [--grid-predict DIR [--grid-predict-params SLOTS,STRIDE,MARGIN,GROW16]]
                                          [--grid-time DIR [--grid-time-params L,WAIT,RELEASE]]
                                          <drive_dir> <calib_cam_to_cam.txt> [max_frames]

--render DIR: the accumulated map is drawn after every frame (320 x 480, the reference's recording size) into
DIR/frame_%06d.ppm, and at the end View3D::recordHuman's fly-through into DIR/img_320_480_%06d.ppm.  Without the flag
the map is still accumulated on the device and the printed output is what it was.

--panes DIR: the window's three 2-D panes (maindialog.cpp:451-452, 506-511, 588-598) after every frame: the left and the
right image with the matches over them (inliers coloured by disparity, outliers blue) into DIR/left_%06d.ppm and
DIR/right_%06d.ppm, the colour-coded disparity map into DIR/disp_%06d.ppm.  A pane has the frame's size unless
--pane-size WxH is given.  D1 is read where ELAS wrote it on the device, and with --resident so is the frame.  The
printed output is what it is without the flag.

--unrectified: the drive holds RAW frames (KITTI's "extract" drives, S_xx pixels).  They are uploaded once and rectified
on the device with K_xx, D_xx, R_rect_xx, P_rect_xx of cameras 0 and 1 (include/svh_rectify.h; what
framecapturethread.cpp:100-131, 328-349 does with OpenCV), ELAS reads the rectified pair where it lies, and one copy
back feeds svh_vo_process, which takes host images.

--resident: the frame never returns to the host.  A rectified drive's pair is uploaded once, a raw pair is rectified in
place (--unrectified), and the visual odometry (svh_vo_process_device), ELAS and the map fusion (svh_map_add_device) all
read that one device copy: no download, no second or third upload.  Results are the same bit for bit.

--normalize: StereoImage::histogramNormalization (stereoimage.cpp:94-134; include/svh_histnorm.h) on both images of
every pair, on the device, in place where ELAS and the visual odometry read them, after the rectification if there is
one.  The reference has the function and does not call it; neither does this tool without the flag.  Works with
--resident and --lockstep K (one call for the K pairs).

--thin S: voxel-grid thinning of the accumulated map (svh_view_thin): of the points that fall into one cube of side S
(metres) the first one drawn stays.  It runs after every N-th append of the map's lists (--thin-every N, default 1) and
once more at the end, which gives the map that thinning only at the end gives.  With --lockstep K every drive's view is
thinned.  The per-frame lines are what they are without the flag; one line at the end states the map's size.

--ply FILE: the map at the end (View.points(), after the last thinning if there is one) as a binary little-endian PLY
with the float properties x y z val; with --lockstep K one file per drive, FILE with _<drive> before its extension.

--grid DIR: the ground grid (include/svh_grid.h) after every frame into DIR/grid_%06d.ppm, forward up: unknown cells dark
grey, free cells green by their intensity, obstacles red, drops blue, cells under an overhang with a full blue byte.  The
map fusion revises the store, so the grid is cleared and rebuilt from the view's whole store (svh_grid_add_view, device to
device) instead of accumulating.  --grid-cell S: the side of a cell in metres (0.2); --grid-size NXxNZ: cells across and
along (256x256); the window is centred on the first camera and starts at it.  The frame is that of a level camera 1.65 m
above the road unless --level is given: then the road plane is estimated once, from the first frame's D1 on the device
(include/svh_plane.h), and levels the grid (svh_grid_frame_plane); if that estimate finds no plane the tool says so and
falls back to the level camera.  The per-frame lines are what they are without the flag.  Not with --lockstep.

--grid-local DIR: the ground grid as a local map, after every frame into DIR/local_%06d.ppm.  Nothing is cleared or
rebuilt.  Per frame the window follows the camera centre (the translation of the pose given to add_camera) so that it
stands in the middle cell (svh_grid_follow: what stays inside is kept, the strips that enter are empty), the NEWEST list
the frame appended to the view is binned with one ray per low point from that centre
(svh_grid_add_view_lists_from, device to device), and svh_grid_render_local colours the grid as --grid does, with the
cells that are unknown but were looked through -- at least min_points rays passed -- in grey-green (96, 112, 96).  The
list the map fusion revises (the one before the newest) is NOT added again: the local map keeps the points that list
had when it was the newest.  --grid-cell and --grid-size apply; the frame is the level camera's.  --grid stays what it
is and may be given too.  Not with --lockstep.

--grid-cost DIR: needs --grid-local.  After every local step the cost map of the local grid (svh_grid_render_cost) into
DIR/cost_%06d.ppm: lethal cells red, cells within the inscribed radius orange, the inflation ramp from red to blue, free
space dark green, unknown cells dark grey, steep cells with a full green byte.  --grid-slope S: the largest rise over run
between neighbouring free cells (0.35); --grid-inscribed M and --grid-inflate M: the two radii in metres (0.4, 1.5).  The
inflation radius must be at most 256 cells.

--grid-plan DIR: needs --grid-cost.  After every local step a route on the cost map (svh_grid_plan_*): the goals are all
cells of the window row M metres (--grid-goal-ahead, 20) in front of the camera's cell -- the farthest row where the window
ends sooner --, so a blocked cell ahead does not end the route; the start is the camera's position; unknown cells are
passable at a price of 100 above the neutral one.  The plan image (svh_grid_render_plan: the cost map, the goals that count
yellow, the path white) goes into DIR/plan_%06d.ppm and one line {"frame", "status", "length", "cost"} per frame is appended
to DIR/plan.jsonl (status 0 found, 1 unreachable, 2 the camera's cell is impassable, 3 outside).

--grid-pose DIR: needs --grid-cost.  After every local step a pose sequence for the vehicle's rectangle (svh_grid_pose_*): the goals
are every heading of the cells of the row that --grid-plan aims at (--grid-goal-ahead), the start the camera's cell at the planning
heading of its forward axis (svh_grid_pose_heading_of); the vehicle and what an unknown cell counts as are the rollouts'
(--grid-roll-vehicle, --grid-roll-unknown).  --grid-pose-params TURN,REVERSE,SPIN: what a turning move, a reverse move and a spin on
the spot add (100,-1,-1: no reverse, no spin).  The image (svh_grid_render_pose: the cost map, the goal cells that count yellow, the
poses' cells white) goes into DIR/pose_%06d.ppm and one line {"frame", "heading", "status", "length", "cost", "poses"} per frame is
appended to DIR/pose.jsonl.

--grid-roll DIR: needs --grid-plan, and runs after it on its goals.  After every local step short motions are scored on the device
(svh_grid_roll_score): nine constant-curvature arcs (-0.2 .. 0.2 per metre) of 24 poses, one every two cells, that start at the
camera's cell along the heading of its forward axis (svh_grid_heading_of); each is cut where the vehicle's rectangle (3.5 m to the
front, 1.0 m to the rear, 0.9 m to either side; --grid-roll-vehicle FRONT,REAR,HALFWIDTH) first touches a cell of cost 253 or more,
an unknown cell among them (--grid-roll-unknown N: an unknown cell counts as a cost of N, 0..254, instead of 254), or leaves the
window, and scored by the field at its end plus the costs it collected.  The image
(svh_grid_render_roll: the cost map, the poses before the cuts light blue, those of the best arc white) goes into
DIR/roll_%06d.ppm and one line {"frame", "set", "best", "feasible", "length", "status", "score"} per frame is appended to
DIR/roll.jsonl (length, status and score of the best arc; -1, -1, null when no arc is feasible).

--grid-frontiers DIR: needs --grid-cost.  After every local step the frontiers of the local grid (svh_grid_get_frontiers: the
free cells beside ground that was never looked at, grouped into 8-connected components, those of fewer than 8 cells dropped),
the representatives of the kept components as the planner's goals (svh_grid_plan_set_goals_frontiers) and the path from the
camera's position to the cheapest of them; unknown cells are passable at a price of 100 above the neutral one.  The image
(svh_grid_render_frontiers: the cost map, kept frontier cells cyan, dropped ones dark cyan, representatives yellow; the path
white over it) goes into DIR/frontiers_%06d.ppm and one line {"frame", "frontier_cells", "components", "kept", "status",
"length", "cost"} per frame is appended to DIR/frontiers.jsonl.  --grid-unexplored: which unknown cells count as unexplored:
those no ray passed (unseen, the default), those that rays passed and that hold no ground (seen), or both.
--grid-frontier-min N: components of fewer than N cells are dropped (8).  May be given with --grid-plan; it runs after it.

--grid-explore DIR: needs --grid-cost; --grid-unexplored and --grid-frontier-min apply to it too.  After every local step the kept
frontier components are ranked from the camera's cell (svh_grid_explore_rank: for each representative the unexplored cells it
would see within --grid-explore-range M metres, 10 by default, and the cost of the path to it; score = reach - 500 gain), the
best one becomes the planner's only goal (svh_grid_plan_set_goal_explore) and the path to it is walked.  The image
(svh_grid_render_view of the chosen representative: the frontier image with the cells it would count magenta, the cells it sees
brightened, itself white; the path white over it; the plain frontier image when nothing is feasible) goes into
DIR/explore_%06d.ppm and one line {"frame", "kept", "records", "feasible", "best", "rep", "gain", "reach", "score", "status",
"length", "cost"} per frame is appended to DIR/explore.jsonl (rep, gain, reach and score null, status -1 when there is no best).
It runs last: the goal it sets is the one the next frame's --grid-plan replaces.

--grid-align DIR: needs --grid-local.  Before a frame's list goes into the local grid its obstacle points are aligned to the
obstacle cells the grid already holds (svh_grid_align_view_lists, the camera's position as the pivot): every rotation of
-K..K steps of 1/256 about the vertical through the camera and every translation of -W..W quarter cells (--grid-align-window K,W;
8,8) is scored and the best taken.  One line {"frame", "status", "k", "ta", "tb", "score", "identity", "n_scan", "ties", "applied"}
per frame is appended to DIR/align.jsonl and the image (svh_grid_render_align: the local image with the scan's cells yellow, the
scan placed at the best cyan, the camera's cell white) goes into DIR/align_%06d.ppm.  With --grid-align-apply a frame whose status
is 0 and whose best is unique (ties 1: no direction was left open) is added to the local grid under the correction M (svh_grid_align_correction), its rays cast from the corrected camera
position; the map view and the odometry are left alone.

--grid-objects DIR: needs --grid-local; works with --grid-dynamic.  After every local step the obstacle cells of the local grid are
grouped into objects and one step of their tracks is taken (svh_grid_objects_step; --grid-objects-params MIN,MAX,HEIGHT,GATE,MISSED:
min_size, max_size, min_height in metres, gate in cells and max_missed of svh_grid_obj_params; 4,4096,0.3,4,2).  The image
(svh_grid_render_objects: the class image, the kept cells in the colour of their track, bright when it moves, structure grey, the
centroid and the cell eight steps ahead marked) goes into DIR/objects_%06d.ppm and one line {"frame", "window", "stats", "tracks"} with
the track table (the fields of svhip.grid.TRACK_FIELDS) is appended to DIR/tracks.jsonl.

--grid-predict DIR: needs --grid-objects and --grid-roll.  After the rollouts of a frame the same nine arcs are scored once more
against where the tracked objects will be (svh_grid_roll_score_pred; --grid-predict-params SLOTS,STRIDE,MARGIN,GROW16: slots, stride,
margin and grow16 of svh_grid_pred_params; 8,1,1,0; a pose per track step, moving tracks only).  The image (svh_grid_render_pred: the
class image with the predicted cells over it, coloured by their first slot) goes into DIR/predict_%06d.ppm and one line {"frame",
"set", "best", "best_pred", "cut_by_object", "score", "score_pred", "pred_stats"} -- both bests, without and with the prediction, and
how many arcs a predicted object cut -- is appended to DIR/predict.jsonl.

--grid-time DIR: needs --grid-objects and --grid-predict.  After the prediction of a frame a path over cell x time from the camera's
cell to the planner's goals that waits for the predicted objects (svh_grid_time_path; --grid-time-params L,WAIT,RELEASE: layers, wait
and release of svh_grid_time_params; 32,100,1).  The images of the layers 0 and L / 2 (svh_grid_render_time: the cost map without
the released objects, the cells blocked at that layer, the goals, the path) go into DIR/time_%06d_t%03d.ppm and one line {"frame",
"status", "length", "cost", "waits", "triples", "time_stats"} -- the path's triples (ga, gb, t) and how many of its moves are waits --
is appended to DIR/time.jsonl.

--grid-dynamic DIR: needs --grid-local.  The local step takes a frame as an OBSERVATION (svh_grid_observe_view_lists) instead of an
add: the frame's sight lines contradict obstacle cells they pass through at the height of their body, CLEAR contradicting frames in a row
forget a cell's points, and a cell that AGE frames have not seen is emptied (--grid-dynamic-params CLEAR,THROUGH,MARGIN,AGE: clear_frames,
min_through, margin in metres and max_age of svh_grid_dyn_params; 2,3,0.1,0).  After every local step the image (svh_grid_render_dyn: the
local image, cells under contradiction tinted, cells the frame cleared or aged magenta) goes into DIR/dyn_%06d.ppm and one line {"frame",
"observations", "cleared", "aged", "confirmed"}, the totals so far, is appended to DIR/dyn.jsonl.  With --grid-align-apply a corrected
frame is observed under its correction.

--grid-archive DIR: needs --grid-local; works with --grid-dynamic.  The local grid keeps the cells that scroll out of its window in
tiles of 16 x 16 and puts them back when the window returns (svh_grid_set_archive; --grid-archive-tiles N: max_tiles, 16384).  After
every local step one line {"frame", "window", "pages", "max_tiles", "stored", "restored", "lost", "refused"} is appended to
DIR/archive.jsonl; at the end the mosaic -- svh_grid_render_region in the local colours over the bounding box of the window and of
every tile that has a page, clipped to 8192 x 8192 cells round the window -- goes into DIR/mosaic.ppm.

--lockstep K: K drives on one GPU, one frame of each per step, through the lockstep entries (LockstepPipeline): the K
pairs are uploaded (or rectified, --unrectified) into one device buffer, then svh_vo_process_batch_device,
svh_vo_get_gain_batch, svh_elas_process_batch_device and svh_map_add_batch_device run once for all K, then one view per
drive.  Always resident.  The K drives are the given drive, drive i starting i frames in; per drive the results are
those of `--resident` on that drive alone.  --render / --panes do not apply.

Python is glue here (ctypes over libsvhip.so); the pose accumulation H_total = H_total * inv(H_delta)
uses numpy where the reference uses Matrix::solve."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROLL_CURVATURES = (-0.2, -0.15, -0.1, -0.05, 0.0, 0.05, 0.1, 0.15, 0.2)   # --grid-roll: per metre; the arcs of one set
ROLL_POSES = 24                                                            # ... of this many poses, one every two cells


class DeviceBuffer:
    """device memory through the HIP runtime libsvhip has loaded"""

    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.ptr = C.c_void_p()
        if self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)):
            raise MemoryError("hipMalloc")
        self.nbytes = nbytes

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.ptr, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1) == 0

    def download(self, arr):
        assert self.hip.hipMemcpy(C.c_void_p(arr.ctypes.data), self.ptr, C.c_size_t(arr.nbytes), 2) == 0
        return arr

    def __del__(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)


class Pipeline:
    def __init__(self, f, cu, cv, base, elas_params=None, max_dist=20.0, rectify_params=None, view_size=(320, 480),
                 resident=False, normalize=False, thin=None, thin_every=1):
        import helpers as Hh
        import svhip as S
        from svhip import mapper, view
        self.S = S
        self.vo = Hh.ProductVo(Hh.vo_defaults(f=f, cu=cu, cv=cv, base=base))
        self.elas = S.Elas(elas_params if elas_params is not None else Hh.robotics())
        self.map = mapper.Mapper(f, cu, cv, base, max_dist)
        self.view = view.View(*view_size)
        self.H_total = np.eye(4)
        self.buf = None
        self.poses = []
        self.rect = None
        self.resident = resident
        self.normalize = normalize
        self.thin, self.thin_every, self.appends = thin, thin_every, 0
        self.histnorm = None   # svhip.histnorm.HistNorm of the frame size, made on the first frame
        self.grid = None       # svhip.grid.Grid once enable_grid() has been called
        self.local = None      # svhip.grid.Grid once enable_grid_local() has been called
        self.grid_level = False
        self.grid_note = None
        self.frame = None      # what render_panes() shows: (I1, I2 or None when resident, w, h, vo ok, ELAS ok)
        self.pane = None
        if rectify_params is not None:
            from svhip import rectify
            self.rect = rectify.Rectifier(rectify_params)
            self.raw = None

    def enable_grid(self, cell=0.2, size=(256, 256), level=False):
        """a ground grid of size = (nx, nz) cells of side `cell`, centred on the first camera and starting at it;
        level: the road plane of the first frame's D1 levels it (else a level camera 1.65 m above the road)"""
        from svhip import grid
        self.grid_kw = dict(nx=size[0], nz=size[1], cell=cell, x0=-0.5 * size[0] * cell, z0=0.0)
        self.grid = grid.Grid(grid.default_params(**self.grid_kw))
        self.grid_level = level

    def level_grid(self, dD1, w, h):
        """the road plane of this frame's D1 (on the device) becomes the grid's frame; the note says what happened"""
        from svhip import grid
        self.grid_level = False
        c = self.vo.params
        pe = self.S.PlaneEstimation()
        status = pe.estimate(dD1, w, h, w, f=c.f, cu=c.cu, cv=c.cv, base=c.base, seed=0)
        try:
            T = grid.frame_plane(pe.plane_euclidean(), pe.transformation())
        except self.S.SvhError:
            self.grid_note = "grid: the road plane estimate found no plane (status %d): falls back to frame_camera(1.65)" % status
            return
        self.grid = grid.Grid(grid.default_params(T=T, **self.grid_kw))
        self.grid_note = "grid levelled by the road plane of frame 0: camera %.3f m above the road, pitch %.4f rad" % (
            T[2, 3], float(pe.pitch()))

    def enable_grid_local(self, cell=0.2, size=(256, 256)):
        """a second ground grid of size = (nx, nz) cells that accumulates and follows the camera (local_step)"""
        from svhip import grid
        self.local = grid.Grid(grid.default_params(nx=size[0], nz=size[1], cell=cell, x0=-0.5 * size[0] * cell, z0=0.0))
        self.local_appends = 0
        self.align_apply = None    # False / True once enable_grid_align() has been called
        self.align_last = None     # (record, applied, image) of the last local step that aligned a frame
        self.dynamic = False       # True once enable_grid_dynamic() has been called: frames are observations

    def enable_grid_dynamic(self, **kw):
        """the local step observes (svh_grid_observe_*) instead of adding; kw: clear_frames, min_through, margin, max_age"""
        self.local.set_dynamics(**kw)
        self.dynamic = True

    def enable_grid_align(self, apply=False, window=(8, 8)):
        """align every frame's list to the local grid before it is added (local_step); apply: add it under the correction"""
        c = self.local.params.cell
        self.local.set_align(reach=min(max(0.6, c), 32 * c), range=min(25.6, 256 * c), rot_n=window[0], trans_n=window[1])
        self.align_apply = bool(apply)

    def set_grid_cost(self, **kw):
        """the traversability parameters of the local grid: max_slope, inscribed, inflate"""
        self.local.set_traversability(**kw)

    def plan_step(self, ahead=20.0):
        """goals on the window row `ahead` metres in front of the camera's cell, the path from the camera's position:
        (status, cells [n, 2], cost, the plan image [nz, nx, 3])"""
        g = self.local
        centre = self.H_total[:3, 3].copy()
        (_, gb), (oa, ob) = g.cell_of(centre), g.window()
        row = min(gb + int(round(ahead / g.params.cell)), ob + g.nz - 1)
        g.set_goals([(oa + ia, row) for ia in range(g.nx)])
        status, cells, cost = g.path(centre)
        return status, cells, cost, g.render_plan(cells)

    def pose_step(self, ahead=20.0):
        """every heading of the cells of the window row `ahead` metres in front of the camera's cell a goal of the pose planner, the
        pose sequence from the camera's cell at the heading of its forward axis: (heading, status, poses [n, 3], cost, the pose image
        [nz, nx, 3])"""
        g = self.local
        centre = self.H_total[:3, 3].copy()
        (_, gb), (oa, ob) = g.cell_of(centre), g.window()
        row = min(gb + int(round(ahead / g.params.cell)), ob + g.nz - 1)
        g.pose_set_goals([(oa + ia, row, -1) for ia in range(g.nx)])
        d = g.pose_heading_of(self.H_total[:3, 2].copy())
        status, poses, cost = g.pose_path(centre, d)
        return d, status, poses, cost, g.render_pose(poses)

    def enable_roll(self, curvatures, step_len, poses, **kw):
        """the vehicle (kw: front, rear, half_width, stop_cost, ...) and one set of constant-curvature arcs per start heading"""
        from svhip import grid
        g = self.local
        if kw:
            g.set_roll(**kw)
        g.set_candidates(grid.arc_candidates(g.params.cell, g.roll_params()[0].headings_m, curvatures, step_len, poses))

    def roll_step(self):
        """the arcs that start along the camera's forward axis scored at the camera's cell on the cost map and the field as they
        stand: (set, best, records [K, 5], scores [K], the rollout image [nz, nx, 3])"""
        g = self.local
        s = g.heading_of(self.H_total[:3, 2].copy())
        best, recs, scores = g.roll_score(self.H_total[:3, 3].copy(), s)
        return s, best, recs, scores, g.render_roll()

    def frontier_step(self):
        """the frontiers of the local grid, goals from them, the path from the camera's position:
        (stats, status, cells [n, 2], cost, the frontier image with the path over it [nz, nx, 3])"""
        g = self.local
        centre = self.H_total[:3, 3].copy()
        stats = g.frontier_stats()
        g.set_goals_frontiers()
        status, cells, cost = g.path(centre)
        img = g.render_frontiers()
        oa, ob = g.window()
        for ga, gb in cells:                                     # global cells of the window: row 0 is the farthest
            img[g.nz - 1 - (gb - ob), ga - oa] = (255, 255, 255)
        return stats, status, cells, cost, img

    def explore_step(self):
        """the kept frontier components ranked from the camera's cell, the best one as the planner's goal, the path to it:
        (kept, best, recs [n, 5], scores [n], status, cells [n, 2], cost, the view image of the chosen representative with the path
        over it [nz, nx, 3]); status -1, no cells: nothing is feasible"""
        g = self.local
        centre = self.H_total[:3, 3].copy()
        kept = g.frontier_stats()[2]
        best, recs, scores = g.explore_rank(centre)
        status, cells, cost = -1, np.zeros((0, 2), np.int32), 0x7FFFFFFF
        if g.set_goal_explore(centre):
            status, cells, cost = g.path(centre)
        img = g.render_view(int(recs[best, 1]), int(recs[best, 2])) if best >= 0 else g.render_frontiers()
        oa, ob = g.window()
        for ga, gb in cells:                                     # global cells of the window: row 0 is the farthest
            img[g.nz - 1 - (gb - ob), ga - oa] = (255, 255, 255)
        return kept, best, recs, scores, status, cells, cost, img

    def local_step(self):
        """follow the camera centre to the middle cell, add (or, with the dynamics, observe) the newest list with rays from it, render:
        [nz, nx, 3]"""
        from svhip import view
        g = self.local
        if self.appends > self.local_appends:   # a frame whose ELAS failed appends nothing
            self.local_appends = self.appends
            centre = self.H_total[:3, 3].copy()
            g.follow(centre, g.nx // 2, g.nz // 2)
            last = self.view.count(view.LISTS) - 1
            applied = False
            if self.align_apply is not None:
                rec = g.align_view_lists(self.view, last, 1, centre)
                img = g.render_align()
                if self.align_apply and rec[0] == 0 and rec[7] == 1 and rec[1:4].any():
                    M = g.align_correction(int(rec[1]), int(rec[2]), int(rec[3]), centre)
                    pts = self.view.points(last).copy()
                    pts[:, :3] = (pts[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
                    (g.observe_points if self.dynamic else g.add_points_from)(pts, M[:3, :3] @ centre + M[:3, 3])
                    applied = True
                self.align_last = (rec, applied, img)
            if not applied:
                (g.observe_view_lists if self.dynamic else g.add_view_lists_from)(self.view, last, 1, centre)
        return g.render_local()

    def render_grid(self):
        """the grid of the view's store as it is now, rebuilt: [nz, nx, 3] uint8, forward up"""
        self.grid.clear()
        self.grid.add_view(self.view)
        return self.grid.render()

    def push(self, I1, I2):
        """one stereo frame; returns (vo_ok, points_prev, points_curr)"""
        if self.rect is not None:
            sh, sw = I1.shape
            h, w = self.rect.dst_shape
        else:
            h, w = I1.shape
        n = w * h
        if self.buf is None or self.buf[0].nbytes != n:
            self.buf = [DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(4 * n), DeviceBuffer(4 * n)]
        if self.rect is not None:
            # framecapturethread.cpp:328-349: the raw pair goes up once, is rectified where ELAS will read it, and comes
            # back once for the visual odometry
            if self.raw is None:
                self.raw = [DeviceBuffer(sw * sh), DeviceBuffer(sw * sh)]
            self.raw[0].upload(I1)
            self.raw[1].upload(I2)
            self.rect.pairs_device(1, self.raw[0].ptr.value, self.raw[1].ptr.value, sw, sw * sh,
                                   self.buf[0].ptr.value, self.buf[1].ptr.value, w, n)
        uploaded = self.rect is not None   # the pair ELAS will read lies in buf[0], buf[1]
        if self.normalize:
            # stereoimage.cpp:94-134 on both images, in place on the device
            if not uploaded:
                self.buf[0].upload(I1)
                self.buf[1].upload(I2)
                uploaded = True
            if self.histnorm is None or (self.histnorm.width, self.histnorm.height) != (w, h):
                from svhip import histnorm
                self.histnorm = histnorm.HistNorm(w, h)
            self.histnorm.pairs_device(1, self.buf[0].ptr.value, self.buf[1].ptr.value, w, n)
        if uploaded and not self.resident:   # one copy back for svh_vo_process, which takes host images
            I1 = self.buf[0].download(np.empty((h, w), np.uint8))
            I2 = self.buf[1].download(np.empty((h, w), np.uint8))
        # visualodometrythread.cpp:100-137
        if self.resident:
            # the pair is on the device once (uploaded here, or rectified there) and every stage reads that copy
            from svhip import resident
            if not uploaded:
                self.buf[0].upload(I1)
                self.buf[1].upload(I2)
                uploaded = True
            ok = resident.vo_process(self.vo, self.buf[0].ptr.value, self.buf[1].ptr.value, w, h, w) == 1
        else:
            ok = self.vo.process(I1, I2) == 1
        gain = 0.0
        if ok:
            Hd = self.vo.motion()
            gain = float(self.vo.gain(self.vo.inliers()))
            try:
                self.H_total = self.H_total @ np.linalg.inv(Hd)
            except np.linalg.LinAlgError:
                pass
        self.poses.append(self.H_total.copy())
        # stereothread.cpp:62-115: ELAS with the disparity maps left on the device
        dI1, dI2, dD1, dD2 = self.buf
        if not uploaded:
            dI1.upload(I1)
            dI2.upload(I2)
        st = self.elas.process_batch_device(1, dI1.ptr.value, dI2.ptr.value, n, dD1.ptr.value, dD2.ptr.value,
                                            4 * n, w, h, w)
        self.frame = (None, None, w, h, ok, st[0] == 0) if self.resident else (I1, I2, w, h, ok, st[0] == 0)
        if st[0] != 0:
            return ok, 0, 0
        if self.grid is not None and self.grid_level:
            self.level_grid(dD1.ptr.value, w, h)
        # stereothread.cpp:166-170
        if self.resident:
            resident.map_add(self.map, dD1.ptr.value, dI1.ptr.value, w, h, self.H_total, gain, pitch=w)
        else:
            self.map.add(None, I1, self.H_total, gain, device_ptr=dD1.ptr.value)
        # maindialog.cpp:602-606: the lists go from the map to the view without leaving the device
        self.view.add_camera(self.H_total, 0.1, True)
        self.view.add_map(self.map)
        self.appends += 1
        if self.thin and self.appends % self.thin_every == 0:
            self.view.thin(self.thin)
        return ok, self.map._L.svh_map_points(self.map._h, 0, None, 0), self.map._L.svh_map_points(self.map._h, 1, None, 0)

    def render_panes(self, size=None):
        """the three View2D panes of the frame push() has just processed, as [H, W, 3] uint8 images (left, right,
        disparity); size = (W, H), the frame's size by default.  The frame is read on the device when it is resident,
        D1 always; the matches are those of the visual odometry, none when it failed (setImage clears them)."""
        from svhip import view2d
        I1, I2, w, h, ok, have_d = self.frame
        W, Ht = size if size is not None else (w, h)
        if self.pane is None:
            self.pane = [view2d.View2D(W, Ht) for _ in range(3)]
        for pane in self.pane:
            if (pane.width, pane.height) != (W, Ht):
                pane.resize(W, Ht)
        left, right, disp = self.pane
        for k, (pane, I) in enumerate(((left, I1), (right, I2))):
            if I is None:
                pane.set_image_device(self.buf[k].ptr.value, w, h, w)
            else:
                pane.set_image(I)
            if ok:
                pane.set_matches_indexed(self.vo.matches(), self.vo.inliers(), left=(k == 0))
        if have_d:
            disp.set_disparity_device(self.buf[2].ptr.value, w, h)
        return left.render(), right.render(), disp.render()


class LockstepPipeline:
    """Pipeline(resident=True) for K drives in lockstep: push() takes one pair per drive.  Drive i's objects are vos[i],
    maps[i], views[i], H_total[i], poses[i]; per drive every result equals that of a resident Pipeline of its own."""

    def __init__(self, K, f, cu, cv, base, elas_params=None, max_dist=20.0, rectify_params=None, view_size=(320, 480),
                 private_rand=None, normalize=False, thin=None, thin_every=1):
        import helpers as Hh
        import svhip as S
        from svhip import mapper, view
        self.S, self.K = S, K
        self.vos = [Hh.ProductVo(Hh.vo_defaults(f=f, cu=cu, cv=cv, base=base), private_rand=private_rand)
                    for _ in range(K)]
        self.elas = S.Elas(elas_params if elas_params is not None else Hh.robotics())
        self.maps = [mapper.Mapper(f, cu, cv, base, max_dist) for _ in range(K)]
        self.views = [view.View(*view_size) for _ in range(K)]
        self.H_total = [np.eye(4) for _ in range(K)]
        self.poses = [[] for _ in range(K)]
        self.buf = None
        self.rect = None
        self.normalize = normalize
        self.thin, self.thin_every, self.appends = thin, thin_every, [0] * K
        self.histnorm = None
        if rectify_params is not None:
            from svhip import rectify
            self.rect = rectify.Rectifier(rectify_params)
            self.raw = None

    def push(self, pairs):
        """one stereo frame per drive: pairs = K (I1, I2); returns K (vo_ok, points_prev, points_curr)"""
        from svhip import resident
        K = self.K
        assert len(pairs) == K
        if self.rect is not None:
            sh, sw = pairs[0][0].shape
            h, w = self.rect.dst_shape
        else:
            h, w = pairs[0][0].shape
        n = w * h
        if self.buf is None or self.buf[0].nbytes != K * n:
            self.buf = [DeviceBuffer(K * n), DeviceBuffer(K * n), DeviceBuffer(4 * K * n), DeviceBuffer(4 * K * n)]
        dI1, dI2, dD1, dD2 = (b.ptr.value for b in self.buf)
        if self.rect is not None:
            # the K raw pairs go up once and are rectified in one launch where every later stage reads them
            if self.raw is None:
                self.raw = [DeviceBuffer(K * sw * sh), DeviceBuffer(K * sw * sh)]
            self.raw[0].upload(np.stack([p[0] for p in pairs]))
            self.raw[1].upload(np.stack([p[1] for p in pairs]))
            self.rect.pairs_device(K, self.raw[0].ptr.value, self.raw[1].ptr.value, sw, sw * sh, dI1, dI2, w, n)
        else:
            self.buf[0].upload(np.stack([p[0] for p in pairs]))
            self.buf[1].upload(np.stack([p[1] for p in pairs]))
        if self.normalize:
            # stereoimage.cpp:94-134 on the 2 K images in one call, each with its own table
            if self.histnorm is None or (self.histnorm.width, self.histnorm.height) != (w, h):
                from svhip import histnorm
                self.histnorm = histnorm.HistNorm(w, h)
            self.histnorm.pairs_device(K, dI1, dI2, w, n)
        a1 = [dI1 + i * n for i in range(K)]
        a2 = [dI2 + i * n for i in range(K)]
        # visualodometrythread.cpp:100-137 for the K drives
        oks = [o == 1 for o in resident.vo_process_batch(self.vos, a1, a2, w, h, w)]
        inl = [self.vos[i].inliers() if oks[i] else np.zeros(0, np.int32) for i in range(K)]
        gains = resident.vo_gain_batch(self.vos, inl)
        gain = [float(gains[i]) if oks[i] else 0.0 for i in range(K)]
        for i in range(K):
            if oks[i]:
                try:
                    self.H_total[i] = self.H_total[i] @ np.linalg.inv(self.vos[i].motion())
                except np.linalg.LinAlgError:
                    pass
            self.poses[i].append(self.H_total[i].copy())
        # stereothread.cpp:62-115: ELAS over the K pairs, the disparity maps left on the device
        st = self.elas.process_batch_device(K, dI1, dI2, n, dD1, dD2, 4 * n, w, h, w)
        live = [i for i in range(K) if st[i] == 0]
        # stereothread.cpp:166-170 for the drives that have a disparity map
        if live:
            resident.map_add_batch([self.maps[i] for i in live], [dD1 + 4 * i * n for i in live], [a1[i] for i in live],
                                   w, h, [self.H_total[i] for i in live], [gain[i] for i in live], pitch=w)
        out = []
        for i in range(K):
            if st[i] != 0:
                out.append((oks[i], 0, 0))
                continue
            self.views[i].add_camera(self.H_total[i], 0.1, True)
            self.views[i].add_map(self.maps[i])
            self.appends[i] += 1
            if self.thin and self.appends[i] % self.thin_every == 0:
                self.views[i].thin(self.thin)
            m = self.maps[i]
            out.append((oks[i], m._L.svh_map_points(m._h, 0, None, 0), m._L.svh_map_points(m._h, 1, None, 0)))
        return out


def finish_map(v, thin, ply, tag=""):
    """the last thinning and the PLY file of one view; prints the one line --thin / --ply add"""
    from svhip import view
    if thin:
        st = v.thin(thin)
        print("%smap thinned at %g: %d points of %d left, %d without a voxel" % (tag, thin, st.after, st.before, st.unplaced))
    if ply:
        pts = v.points()
        view.write_ply(ply, pts)
        print("%smap of %d points in %d lists written to %s" % (tag, len(pts), v.count(view.LISTS), ply))


def main_lockstep(K, drive_dir, calib, limit, rp, normalize=False, thin=None, thin_every=1, ply=None):
    import collections
    from svhip import kitti
    p = LockstepPipeline(K, calib.f, calib.cu, calib.cv, calib.base, rectify_params=rp, normalize=normalize, thin=thin,
                         thin_every=thin_every)
    window = collections.deque(maxlen=K)
    t0 = time.perf_counter()
    steps = 0
    for I1, I2, _ in kitti.Sequence(drive_dir):
        window.append((I1, I2))
        if len(window) < K:
            continue
        res = p.push(list(window))   # drive i is i frames ahead of drive 0
        steps += 1
        print("step %4d  " % (steps - 1) + "  ".join("[%d] vo=%d z=%.2f kept=%d new=%d" % (
            i, ok, p.H_total[i][2, 3], n0, n1) for i, (ok, n0, n1) in enumerate(res)))
        if steps >= limit:
            break
    dt = time.perf_counter() - t0
    print("%d steps of %d drives in %.2f s = %.1f frames/s (PNG decode included)" % (
        steps, K, dt, steps * K / max(dt, 1e-9)))
    for i in range(K):
        name = None
        if ply:
            stem, ext = os.path.splitext(ply)
            name = "%s_%d%s" % (stem, i, ext)
        finish_map(p.views[i], thin, name, "[%d] " % i)


def mosaic_box(g):
    """(ga0, gb0, w, h): the bounding box of the window and of every tile that has a page, clipped to 8192 x 8192 cells round the window"""
    (oa, ob), tiles = g.window(), g.archive_tiles()
    lo = [oa, ob]
    hi = [oa + g.nx - 1, ob + g.nz - 1]
    for axis, n in ((0, g.nx), (1, g.nz)):
        if len(tiles):
            lo[axis] = min(lo[axis], 16 * int(tiles[:, axis].min()))
            hi[axis] = max(hi[axis], 16 * int(tiles[:, axis].max()) + 15)
        if hi[axis] - lo[axis] + 1 > 8192:                # the cells beside the window are shared between its two sides
            lo[axis] = max(lo[axis], (oa, ob)[axis] - (8192 - n) // 2)
            hi[axis] = min(hi[axis], lo[axis] + 8191)
    return lo[0], lo[1], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1


def main():
    lockstep = 0
    if "--lockstep" in sys.argv:
        k = sys.argv.index("--lockstep")
        try:
            lockstep = int(sys.argv[k + 1])
            assert lockstep >= 1
        except (IndexError, ValueError, AssertionError):
            raise SystemExit(__doc__)
        del sys.argv[k:k + 2]
    unrectified = "--unrectified" in sys.argv
    if unrectified:
        sys.argv.remove("--unrectified")
    resident = "--resident" in sys.argv
    if resident:
        sys.argv.remove("--resident")
    normalize = "--normalize" in sys.argv
    if normalize:
        sys.argv.remove("--normalize")
    thin, thin_every, ply = None, 1, None
    grid_dir, grid_cell, grid_size = None, 0.2, (256, 256)
    local_dir, cost_dir, cost_kw = None, None, {}
    plan_dir, goal_ahead, front_dir, front_kw = None, None, None, {}
    explore_dir, explore_kw = None, {}
    align_dir, align_apply, align_window = None, False, None
    roll_dir, roll_kw = None, {}
    pose_dir, pose_kw = None, {}
    dyn_dir, dyn_kw = None, {}
    archive_dir, archive_tiles = None, None
    obj_dir, obj_kw = None, {}
    pred_dir, pred_kw = None, {}
    time_dir, time_kw = None, {}
    level = "--level" in sys.argv
    if level:
        sys.argv.remove("--level")
    try:
        if "--grid-cell" in sys.argv:
            k = sys.argv.index("--grid-cell")
            grid_cell = float(sys.argv[k + 1])
            assert grid_cell > 0 and grid_cell < float("inf")
            del sys.argv[k:k + 2]
        if "--grid-size" in sys.argv:
            k = sys.argv.index("--grid-size")
            grid_size = tuple(int(v) for v in sys.argv[k + 1].lower().split("x"))
            assert len(grid_size) == 2 and all(1 <= v <= 8192 for v in grid_size)
            del sys.argv[k:k + 2]
        if "--grid" in sys.argv:
            k = sys.argv.index("--grid")
            grid_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-local" in sys.argv:
            k = sys.argv.index("--grid-local")
            local_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-cost" in sys.argv:
            k = sys.argv.index("--grid-cost")
            cost_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        for flag, name in (("--grid-slope", "max_slope"), ("--grid-inscribed", "inscribed"), ("--grid-inflate", "inflate")):
            if flag in sys.argv:
                k = sys.argv.index(flag)
                cost_kw[name] = float(sys.argv[k + 1])
                del sys.argv[k:k + 2]
        if "--grid-plan" in sys.argv:
            k = sys.argv.index("--grid-plan")
            plan_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-goal-ahead" in sys.argv:
            k = sys.argv.index("--grid-goal-ahead")
            goal_ahead = float(sys.argv[k + 1])
            assert goal_ahead >= 0 and goal_ahead < float("inf")
            del sys.argv[k:k + 2]
        if "--grid-pose" in sys.argv:
            k = sys.argv.index("--grid-pose")
            pose_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-pose-params" in sys.argv:
            k = sys.argv.index("--grid-pose-params")
            turn, reverse, spin = (int(v) for v in sys.argv[k + 1].split(","))
            pose_kw = dict(turn=turn, reverse=reverse, spin=spin)
            del sys.argv[k:k + 2]
        if "--grid-roll" in sys.argv:
            k = sys.argv.index("--grid-roll")
            roll_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-roll-vehicle" in sys.argv:
            k = sys.argv.index("--grid-roll-vehicle")
            dims = [float(v) for v in sys.argv[k + 1].split(",")]
            assert len(dims) == 3 and all(0 <= v < float("inf") for v in dims)
            roll_kw.update(front=dims[0], rear=dims[1], half_width=dims[2])
            del sys.argv[k:k + 2]
        if "--grid-roll-unknown" in sys.argv:
            k = sys.argv.index("--grid-roll-unknown")
            roll_kw["unknown_cost"] = int(sys.argv[k + 1])
            assert 0 <= roll_kw["unknown_cost"] <= 254
            del sys.argv[k:k + 2]
        if "--grid-frontiers" in sys.argv:
            k = sys.argv.index("--grid-frontiers")
            front_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-unexplored" in sys.argv:
            k = sys.argv.index("--grid-unexplored")
            front_kw["unexplored"] = {"unseen": 8, "seen": 16, "both": 24}[sys.argv[k + 1]]
            del sys.argv[k:k + 2]
        if "--grid-frontier-min" in sys.argv:
            k = sys.argv.index("--grid-frontier-min")
            front_kw["min_size"] = int(sys.argv[k + 1])
            assert 1 <= front_kw["min_size"] <= 1 << 26
            del sys.argv[k:k + 2]
        if "--grid-explore" in sys.argv:
            k = sys.argv.index("--grid-explore")
            explore_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-explore-range" in sys.argv:
            k = sys.argv.index("--grid-explore-range")
            explore_kw["range"] = float(sys.argv[k + 1])
            assert 0 < explore_kw["range"] < float("inf")
            del sys.argv[k:k + 2]
        if "--grid-align" in sys.argv:
            k = sys.argv.index("--grid-align")
            align_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-align-apply" in sys.argv:
            sys.argv.remove("--grid-align-apply")
            align_apply = True
        if "--grid-align-window" in sys.argv:
            k = sys.argv.index("--grid-align-window")
            align_window = tuple(int(v) for v in sys.argv[k + 1].split(","))
            assert len(align_window) == 2 and 0 <= align_window[0] <= 32 and 0 <= align_window[1] <= 32
            del sys.argv[k:k + 2]
        if "--grid-dynamic" in sys.argv:
            k = sys.argv.index("--grid-dynamic")
            dyn_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-dynamic-params" in sys.argv:
            k = sys.argv.index("--grid-dynamic-params")
            v = sys.argv[k + 1].split(",")
            assert len(v) == 4
            dyn_kw = dict(clear_frames=int(v[0]), min_through=int(v[1]), margin=float(v[2]), max_age=int(v[3]))
            assert 0 <= dyn_kw["clear_frames"] <= 65535 and dyn_kw["min_through"] >= 1 and 0 <= dyn_kw["margin"] < 2 ** 20 and dyn_kw["max_age"] >= 0
            del sys.argv[k:k + 2]
        if "--grid-archive" in sys.argv:
            k = sys.argv.index("--grid-archive")
            archive_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-archive-tiles" in sys.argv:
            k = sys.argv.index("--grid-archive-tiles")
            archive_tiles = int(sys.argv[k + 1])
            assert 1 <= archive_tiles <= 2 ** 20
            del sys.argv[k:k + 2]
        if "--grid-objects" in sys.argv:
            k = sys.argv.index("--grid-objects")
            obj_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-objects-params" in sys.argv:
            k = sys.argv.index("--grid-objects-params")
            v = sys.argv[k + 1].split(",")
            assert len(v) == 5
            obj_kw = dict(min_size=int(v[0]), max_size=int(v[1]), min_height=float(v[2]), gate=int(v[3]), max_missed=int(v[4]))
            assert 1 <= obj_kw["min_size"] <= obj_kw["max_size"] <= 2 ** 26 and obj_kw["min_height"] >= 0 and 0 <= obj_kw["gate"] <= 64
            assert 0 <= obj_kw["max_missed"] <= 255
            del sys.argv[k:k + 2]
        if "--grid-predict" in sys.argv:
            k = sys.argv.index("--grid-predict")
            pred_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-predict-params" in sys.argv:
            k = sys.argv.index("--grid-predict-params")
            v = [int(x) for x in sys.argv[k + 1].split(",")]
            assert len(v) == 4
            pred_kw = dict(slots=v[0], stride=v[1], margin=v[2], grow16=v[3])
            assert 1 <= pred_kw["slots"] <= 32 and 1 <= pred_kw["stride"] <= 64 and 0 <= pred_kw["margin"] <= 16 and 0 <= pred_kw["grow16"] <= 256
            del sys.argv[k:k + 2]
        if "--grid-time" in sys.argv:
            k = sys.argv.index("--grid-time")
            time_dir = sys.argv[k + 1]
            del sys.argv[k:k + 2]
        if "--grid-time-params" in sys.argv:
            k = sys.argv.index("--grid-time-params")
            v = [int(x) for x in sys.argv[k + 1].split(",")]
            assert len(v) == 3
            time_kw = dict(layers=v[0], wait=v[1], release=v[2])
            assert 1 <= time_kw["layers"] <= 256 and (time_kw["wait"] == -1 or 1 <= time_kw["wait"] <= 65535) and time_kw["release"] in (0, 1)
            del sys.argv[k:k + 2]
        assert (obj_dir and pred_dir) or not time_dir
        assert time_dir or not time_kw
        assert (obj_dir and roll_dir) or not pred_dir
        assert pred_dir or not pred_kw
        assert local_dir or not obj_dir
        assert obj_dir or not obj_kw
        assert local_dir or not dyn_dir
        assert local_dir or not archive_dir
        assert archive_dir or archive_tiles is None
        assert dyn_dir or not dyn_kw
        assert local_dir or not align_dir
        assert align_dir or not (align_apply or align_window)
        assert cost_dir or not plan_dir
        assert cost_dir or not front_dir
        assert cost_dir or not explore_dir
        assert front_dir or explore_dir or not front_kw
        assert explore_dir or not explore_kw
        assert plan_dir or pose_dir or goal_ahead is None
        assert plan_dir or not roll_dir
        assert roll_dir or pose_dir or not roll_kw
        assert cost_dir or not pose_dir
        assert pose_dir or not pose_kw
        assert local_dir or not (cost_dir or cost_kw)
        assert cost_dir or not cost_kw
        assert grid_dir or not level
        assert not ((grid_dir or local_dir) and lockstep)
        if "--thin" in sys.argv:
            k = sys.argv.index("--thin")
            thin = float(sys.argv[k + 1])
            assert thin > 0 and thin < float("inf")
            del sys.argv[k:k + 2]
        if "--thin-every" in sys.argv:
            k = sys.argv.index("--thin-every")
            thin_every = int(sys.argv[k + 1])
            assert thin_every >= 1 and thin
            del sys.argv[k:k + 2]
        if "--ply" in sys.argv:
            k = sys.argv.index("--ply")
            ply = sys.argv[k + 1]
            del sys.argv[k:k + 2]
    except (IndexError, ValueError, KeyError, AssertionError):
        raise SystemExit(__doc__)
    render_dir = None
    if "--render" in sys.argv:
        k = sys.argv.index("--render")
        if k + 1 >= len(sys.argv):
            raise SystemExit(__doc__)
        render_dir = sys.argv[k + 1]
        del sys.argv[k:k + 2]
        os.makedirs(render_dir, exist_ok=True)
    panes_dir, pane_size = None, None
    if "--pane-size" in sys.argv:
        k = sys.argv.index("--pane-size")
        try:
            pane_size = tuple(int(v) for v in sys.argv[k + 1].lower().split("x"))
            assert len(pane_size) == 2
        except (IndexError, ValueError, AssertionError):
            raise SystemExit(__doc__)
        del sys.argv[k:k + 2]
    if "--panes" in sys.argv:
        k = sys.argv.index("--panes")
        if k + 1 >= len(sys.argv):
            raise SystemExit(__doc__)
        panes_dir = sys.argv[k + 1]
        del sys.argv[k:k + 2]
        os.makedirs(panes_dir, exist_ok=True)
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    from svhip import grid, kitti, view
    calib = kitti.read_cam_to_cam(sys.argv[2])
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 30
    rp = None
    if unrectified:
        from svhip import rectify
        rp = rectify.params_from_kitti(calib, 0, 1)
    if grid_dir:
        os.makedirs(grid_dir, exist_ok=True)
    if local_dir:
        os.makedirs(local_dir, exist_ok=True)
    if cost_dir:
        os.makedirs(cost_dir, exist_ok=True)
    if plan_dir:
        os.makedirs(plan_dir, exist_ok=True)
        open(os.path.join(plan_dir, "plan.jsonl"), "w").close()
    if pose_dir:
        os.makedirs(pose_dir, exist_ok=True)
        open(os.path.join(pose_dir, "pose.jsonl"), "w").close()
    if front_dir:
        os.makedirs(front_dir, exist_ok=True)
        open(os.path.join(front_dir, "frontiers.jsonl"), "w").close()
    if roll_dir:
        os.makedirs(roll_dir, exist_ok=True)
        open(os.path.join(roll_dir, "roll.jsonl"), "w").close()
    if explore_dir:
        os.makedirs(explore_dir, exist_ok=True)
        open(os.path.join(explore_dir, "explore.jsonl"), "w").close()
    if align_dir:
        os.makedirs(align_dir, exist_ok=True)
        open(os.path.join(align_dir, "align.jsonl"), "w").close()
    if archive_dir:
        os.makedirs(archive_dir, exist_ok=True)
        open(os.path.join(archive_dir, "archive.jsonl"), "w").close()
    if dyn_dir:
        os.makedirs(dyn_dir, exist_ok=True)
        open(os.path.join(dyn_dir, "dyn.jsonl"), "w").close()
    if obj_dir:
        os.makedirs(obj_dir, exist_ok=True)
        open(os.path.join(obj_dir, "tracks.jsonl"), "w").close()
    if pred_dir:
        os.makedirs(pred_dir, exist_ok=True)
        open(os.path.join(pred_dir, "predict.jsonl"), "w").close()
    if time_dir:
        os.makedirs(time_dir, exist_ok=True)
        open(os.path.join(time_dir, "time.jsonl"), "w").close()
    if lockstep:
        return main_lockstep(lockstep, sys.argv[1], calib, limit, rp, normalize, thin, thin_every, ply)
    p = Pipeline(calib.f, calib.cu, calib.cv, calib.base, rectify_params=rp, resident=resident, normalize=normalize,
                 thin=thin, thin_every=thin_every)
    if grid_dir:
        p.enable_grid(grid_cell, grid_size, level)
    if local_dir:
        p.enable_grid_local(grid_cell, grid_size)
    if align_dir:
        p.enable_grid_align(align_apply, align_window or (8, 8))
    if dyn_dir:
        p.enable_grid_dynamic(**dyn_kw)
    if archive_dir:
        p.local.set_archive(max_tiles=archive_tiles or grid.ARCHIVE_DEFAULT_TILES)
    if obj_dir:
        p.local.set_objects(**obj_kw)
    if cost_dir:
        p.set_grid_cost(**cost_kw)
    if plan_dir or front_dir or explore_dir:
        p.local.set_plan(unknown=100)
    if front_kw:
        p.local.set_frontier(**front_kw)
    if explore_kw:
        p.local.set_explore(**explore_kw)
    if roll_dir:
        p.enable_roll(ROLL_CURVATURES, 2.0 * grid_cell, ROLL_POSES, **roll_kw)
    if pred_kw:
        p.local.set_predict(**pred_kw)
    if time_dir:
        p.local.set_time(**time_kw)
    if pose_dir:
        if roll_kw and not roll_dir:
            p.local.set_roll(**roll_kw)
        p.local.set_pose(**pose_kw)
    found = explored = rolled = ranked = aligned = cut_frames = posed = timed = waited = 0
    t0 = time.perf_counter()
    frames = 0
    for I1, I2, (tl, _) in kitti.Sequence(sys.argv[1]):
        ok, n0, n1 = p.push(I1, I2)
        frames += 1
        print("frame %4d  t=%.3f  vo=%d  pose z=%.2f  points kept=%d new=%d" % (
            frames - 1, tl, ok, p.H_total[2, 3], n0, n1))
        if render_dir:
            view.write_ppm(os.path.join(render_dir, "frame_%06d.ppm" % (frames - 1)), p.view.render())
        if panes_dir:
            for name, img in zip(("left", "right", "disp"), p.render_panes(pane_size)):
                view.write_ppm(os.path.join(panes_dir, "%s_%06d.ppm" % (name, frames - 1)), img)
        if grid_dir:
            view.write_ppm(os.path.join(grid_dir, "grid_%06d.ppm" % (frames - 1)), p.render_grid())
        if local_dir:
            p.align_last = None
            view.write_ppm(os.path.join(local_dir, "local_%06d.ppm" % (frames - 1)), p.local_step())
        if dyn_dir:
            view.write_ppm(os.path.join(dyn_dir, "dyn_%06d.ppm" % (frames - 1)), p.local.render_dyn())
            with open(os.path.join(dyn_dir, "dyn.jsonl"), "a") as f:
                f.write(json.dumps(dict(p.local.dyn_stats(), frame=frames - 1)) + "\n")
        if archive_dir:
            with open(os.path.join(archive_dir, "archive.jsonl"), "a") as f:
                f.write(json.dumps(dict(p.local.archive_stats(), frame=frames - 1, window=list(p.local.window()))) + "\n")
        if obj_dir:
            p.local.objects_step(0)
            view.write_ppm(os.path.join(obj_dir, "objects_%06d.ppm" % (frames - 1)), p.local.render_objects())
            with open(os.path.join(obj_dir, "tracks.jsonl"), "a") as f:
                f.write(json.dumps(dict(frame=frames - 1, window=list(p.local.window()), stats=list(p.local.track_stats()),
                                        tracks=p.local.tracks().tolist())) + "\n")
        if align_dir and p.align_last is not None:
            rec, applied, img = p.align_last
            aligned += int(rec[0] == 0)
            view.write_ppm(os.path.join(align_dir, "align_%06d.ppm" % (frames - 1)), img)
            with open(os.path.join(align_dir, "align.jsonl"), "a") as f:
                f.write(json.dumps(dict(zip(("frame",) + grid.ALIGN_FIELDS + ("applied",), [frames - 1] + [int(v) for v in rec] + [bool(applied)]))) + "\n")
        if cost_dir:
            view.write_ppm(os.path.join(cost_dir, "cost_%06d.ppm" % (frames - 1)), p.local.render_cost())
        if plan_dir:
            status, cells, cost, img = p.plan_step(20.0 if goal_ahead is None else goal_ahead)
            found += status == 0
            view.write_ppm(os.path.join(plan_dir, "plan_%06d.ppm" % (frames - 1)), img)
            with open(os.path.join(plan_dir, "plan.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "status": int(status), "length": int(len(cells)), "cost": int(cost)}) + "\n")
        if pose_dir:
            d, status, poses, cost, img = p.pose_step(20.0 if goal_ahead is None else goal_ahead)
            posed += status == 0
            view.write_ppm(os.path.join(pose_dir, "pose_%06d.ppm" % (frames - 1)), img)
            with open(os.path.join(pose_dir, "pose.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "heading": int(d), "status": int(status), "length": int(len(poses)), "cost": int(cost),
                                    "poses": poses.tolist()}) + "\n")
        if roll_dir:
            s, best, recs, scores, img = p.roll_step()
            rolled += best >= 0
            view.write_ppm(os.path.join(roll_dir, "roll_%06d.ppm" % (frames - 1)), img)
            with open(os.path.join(roll_dir, "roll.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "set": int(s), "best": int(best), "feasible": int((scores != (1 << 63) - 1).sum()),
                                    "length": int(recs[best, 0]) if best >= 0 else -1, "status": int(recs[best, 1]) if best >= 0 else -1,
                                    "score": int(scores[best]) if best >= 0 else None}) + "\n")
        if pred_dir:
            best_p, recs_p, scores_p = p.local.roll_score_pred(p.H_total[:3, 3].copy(), s)
            cut = int((recs_p[:, 1] == grid.ROLL_CUT_OBJECT).sum())
            cut_frames += cut > 0
            view.write_ppm(os.path.join(pred_dir, "predict_%06d.ppm" % (frames - 1)), p.local.render_pred())
            with open(os.path.join(pred_dir, "predict.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "set": int(s), "best": int(best), "best_pred": int(best_p), "cut_by_object": cut,
                                    "score": int(scores[best]) if best >= 0 else None, "score_pred": int(scores_p[best_p]) if best_p >= 0 else None,
                                    "pred_stats": list(p.local.pred_stats())}) + "\n")
        if time_dir:
            status, triples, cost = p.local.time_path(p.H_total[:3, 3].copy())
            layers = p.local.time_params().layers
            same = (triples[1:, :2] == triples[:-1, :2]).all(1) if len(triples) > 1 else np.zeros(0, bool)
            waits = int((same & (triples[:-1, 2] < layers - 1)).sum())
            timed += status == 0
            waited += waits > 0
            for t in sorted({0, layers // 2}):
                view.write_ppm(os.path.join(time_dir, "time_%06d_t%03d.ppm" % (frames - 1, t)), p.local.render_time(t, triples))
            with open(os.path.join(time_dir, "time.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "status": int(status), "length": int(len(triples)), "cost": int(cost), "waits": waits,
                                    "triples": triples.tolist(), "time_stats": list(p.local.time_stats())}) + "\n")
        if front_dir:
            stats, status, cells, cost, img = p.frontier_step()
            explored += status == 0
            view.write_ppm(os.path.join(front_dir, "frontiers_%06d.ppm" % (frames - 1)), img)
            with open(os.path.join(front_dir, "frontiers.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "frontier_cells": stats[0], "components": stats[1], "kept": stats[2],
                                    "status": int(status), "length": int(len(cells)), "cost": int(cost)}) + "\n")
        if explore_dir:
            kept, best, recs, scores, status, cells, cost, img = p.explore_step()
            ranked += best >= 0
            view.write_ppm(os.path.join(explore_dir, "explore_%06d.ppm" % (frames - 1)), img)
            with open(os.path.join(explore_dir, "explore.jsonl"), "a") as f:
                f.write(json.dumps({"frame": frames - 1, "kept": int(kept), "records": int(len(recs)), "feasible": int((scores != (1 << 63) - 1).sum()),
                                    "best": int(best), "rep": [int(recs[best, 1]), int(recs[best, 2])] if best >= 0 else None,
                                    "gain": int(recs[best, 3]) if best >= 0 else None, "reach": int(recs[best, 4]) if best >= 0 else None,
                                    "score": int(scores[best]) if best >= 0 else None, "status": int(status), "length": int(len(cells)),
                                    "cost": int(cost)}) + "\n")
        if frames >= limit:
            break
    dt = time.perf_counter() - t0
    print("%d frames in %.2f s = %.1f frames/s (PNG decode included)" % (frames, dt, frames / max(dt, 1e-9)))
    finish_map(p.view, thin, ply)
    if grid_dir:
        if p.grid_note:
            print(p.grid_note)
        st = p.grid.stats()
        print("grid %d x %d cells of %g: %d of %d points binned, %d overhead, %d outside, %d unplaced; %d images in %s" % (
            p.grid.nx, p.grid.nz, grid_cell, st.binned, st.added, st.overhead, st.outside, st.unplaced, frames, grid_dir))
    if local_dir:
        st, (rays, ray_cells), (oa, ob) = p.local.stats(), p.local.ray_stats(), p.local.window()
        print("local grid %d x %d cells of %g at offsets (%d, %d): %d of %d points binned, %d rays over %d cells; %d images in %s" % (
            p.local.nx, p.local.nz, grid_cell, oa, ob, st.binned, st.added, rays, ray_cells, frames, local_dir))
    if dyn_dir:
        d, ds = p.local.dynamics(), p.local.dyn_stats()
        print("dynamics: clear after %d frames of %d through-lines, margin %g m, age %d: %d observations, %d cells cleared, %d aged; %d images and dyn.jsonl in %s" % (
            d.clear_frames, d.min_through, d.margin, d.max_age, ds["observations"], ds["cleared"], ds["aged"], frames, dyn_dir))
    if archive_dir:
        box, st = mosaic_box(p.local), p.local.archive_stats()
        view.write_ppm(os.path.join(archive_dir, "mosaic.ppm"), p.local.render_region(*box))
        print("archive: %d of %d pages in use, %d cells stored, %d restored, %d lost in %d refused calls; archive.jsonl and a mosaic of %d x %d cells from (%d, %d) in %s" % (
            st["pages"], st["max_tiles"], st["stored"], st["restored"], st["lost"], st["refused"], box[2], box[3], box[0], box[1], archive_dir))
    if obj_dir:
        o, os_, ts = p.local.objects_params(), p.local.object_stats(), p.local.track_stats()
        print("objects: size %d..%d, height %g m, gate %d cells, %d misses: %d kept of %d components in the last frame, %d tracks after %d steps; "
              "%d images and tracks.jsonl in %s" % (o.min_size, o.max_size, o.min_height, o.gate, o.max_missed, os_[2], os_[1], ts[1], ts[0], frames, obj_dir))
    if cost_dir:
        t, reach = p.local.traversability()
        print("cost map: slope %g, inscribed %g m, inflation %g m = %d cells; %d images in %s" % (
            t.max_slope, t.inscribed, t.inflate, reach, frames, cost_dir))
    if plan_dir:
        print("plan: goals %g m ahead, a route in %d of %d frames; %d images and plan.jsonl in %s" % (
            20.0 if goal_ahead is None else goal_ahead, found, frames, frames, plan_dir))
    if pose_dir:
        q = p.local.pose_params()
        print("pose plan: goals %g m ahead, turn %d, reverse %d, spin %d: a pose sequence in %d of %d frames; %d images and pose.jsonl in %s" % (
            20.0 if goal_ahead is None else goal_ahead, q.turn, q.reverse, q.spin, posed, frames, frames, pose_dir))
    if roll_dir:
        print("rollouts: %d arcs of %d poses per heading, a feasible one in %d of %d frames; %d images and roll.jsonl in %s" % (
            len(ROLL_CURVATURES), ROLL_POSES, rolled, frames, frames, roll_dir))
    if pred_dir:
        q = p.local.get_predict()
        print("prediction: %d slots of %d steps, margin %d cells growing %d/16 per slot: an arc cut by a predicted object in %d of %d frames; "
              "%d images and predict.jsonl in %s" % (q.slots, q.stride, q.margin, q.grow16, cut_frames, frames, frames, pred_dir))
    if time_dir:
        q = p.local.time_params()
        print("time layer: %d layers, wait %d, release %d: a path in %d of %d frames, one that waits in %d; %d images and time.jsonl in %s" % (
            q.layers, q.wait, q.release, timed, frames, waited, len({0, q.layers // 2}) * frames, time_dir))
    if front_dir:
        print("frontiers: goals from the kept components, a route in %d of %d frames; %d images and frontiers.jsonl in %s" % (
            explored, frames, frames, front_dir))
    if explore_dir:
        print("exploration: the kept frontiers ranked within %d cells, a best one in %d of %d frames; %d images and explore.jsonl in %s" % (
            p.local.explore_params()[1], ranked, frames, frames, explore_dir))
    if align_dir:
        print("alignment: %d rotations x %d x %d translations per frame, a match in %d of %d frames%s; images and align.jsonl in %s" % (
            2 * p.local.align_params.rot_n + 1, 2 * p.local.align_params.trans_n + 1, 2 * p.local.align_params.trans_n + 1, aligned, frames,
            ", applied to the local grid" if align_apply else "", align_dir))
    if render_dir:
        n, images = p.view.record_human()
        for k in range(n):
            view.write_ppm(os.path.join(render_dir, "img_%d_%d_%06d.ppm" % (p.view.width, p.view.height, k)), images[k])
        print("map of %d points in %d lists, %d cameras: %d frames and a fly-through of %d images in %s" % (
            p.view.count(view.POINTS), p.view.count(view.LISTS), p.view.count(view.CAMERAS), frames, n, render_dir))


if __name__ == "__main__":
    main()

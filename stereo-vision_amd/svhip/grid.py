"""ctypes binding of the ground grid in libsvhip.so (C-ABI: include/svh_grid.h): a 2.5-D bird's-eye grid over the road
plane -- per cell how many points, how high, how bright, drivable or not -- binned on the device from the map view's store
or from a list of points.  The arithmetic is stereo-vision_amd/csrc/grid_core.h, grid_plan_core.h, grid_front_core.h and
grid_roll_core.h; that of the objects and their tracks grid_obj_core.h, that of the exploration layer grid_explore_core.h, that of the alignment layer grid_align_core.h, that of the
dynamics grid_dyn_core.h."""
import ctypes as C

import numpy as np

from . import ERR_BAD_ARG, SvhError, last_error, lib

COUNT, OVERHEAD, HMIN, HMAX, HMEAN, INTENSITY, CLASS = range(7)
RENDER_CLASS, RENDER_HEIGHT, RENDER_INTENSITY = range(3)
UNKNOWN, FREE, OBSTACLE, DROP, OVERHANG = 0, 1, 2, 3, 0x80
LOW, FATE_OVERHEAD, OUTSIDE, UNPLACED = range(4)
PLANE_DTYPE = [np.int32, np.int32, np.float32, np.float32, np.float32, np.uint8, np.uint8]
LOCAL_PASS, LOCAL_STATE = range(2)
LOCAL_DTYPE = [np.int32, np.uint8]
SEEN = 0x40
SEEN_COLOUR = (96, 112, 96)
TRAV_FLAGS, TRAV_DIST2, TRAV_COST = range(3)
TRAV_DTYPE = [np.uint8, np.int32, np.uint8]
STEEP, LETHAL = 1, 2
LETHAL_OBSTACLE, LETHAL_DROP, LETHAL_STEEP, LETHAL_UNSEEN, LETHAL_UNKNOWN_SEEN = 1, 2, 4, 8, 16
DIST2_FAR = 0x7FFFFFFF
PLAN_POT, PLAN_DIR = range(2)
PLAN_DTYPE = [np.int32, np.uint8]
PLAN_FAR = 0x7FFFFFFF
DIR_GOAL, DIR_NONE = 8, 9
PATH_FOUND, PATH_UNREACHABLE, PATH_BLOCKED, PATH_OUTSIDE = range(4)
GOAL_COLOUR, PATH_COLOUR = (255, 255, 0), (255, 255, 255)
FRONT_FLAGS, FRONT_LABEL = range(2)
FRONT_DTYPE = [np.uint8, np.int32]
FRONTIER, FRONT_KEPT, FRONT_REP = 1, 2, 4
FRONT_RECORD = 10
FRONT_FIELDS = ("label", "size", "ga_min", "gb_min", "ga_max", "gb_max", "cen_ga", "cen_gb", "rep_ga", "rep_gb")
FRONT_KEPT_COLOUR, FRONT_DROPPED_COLOUR, FRONT_REP_COLOUR = (0, 255, 255), (0, 96, 128), (255, 255, 0)
ROLL_RECORD = 5
ROLL_FIELDS = ("len", "status", "max_f", "sum_f", "pot_end")
ROLL_COMPLETE, ROLL_CUT_COST, ROLL_CUT_WINDOW, ROLL_EMPTY = range(4)
ROLL_INFEASIBLE = 2 ** 63 - 1
ROLL_COLOUR, ROLL_BEST_COLOUR = (0, 192, 255), (255, 255, 255)
EXPLORE_RECORD = 5
EXPLORE_FIELDS = ("label", "rep_ga", "rep_gb", "gain", "reach")
EXPLORE_INFEASIBLE = 2 ** 63 - 1
VIEW_NONE, VIEW_VISITED, VIEW_COUNTED = range(3)
VIEW_COLOUR, VIEWPOINT_COLOUR = (255, 0, 255), (255, 255, 255)
ALIGN_RECORD = 8
ALIGN_FIELDS = ("status", "k", "ta", "tb", "score", "identity", "n_scan", "ties")
ALIGN_OK, ALIGN_FEW, ALIGN_FLAT = range(3)
ALIGN_SUB = 4
ALIGN_SCAN_COLOUR, ALIGN_BEST_COLOUR, ALIGN_PIVOT_COLOUR = (255, 224, 0), (0, 224, 255), (255, 255, 255)
DYN_AGE, DYN_CONTRA, DYN_THROUGH = range(3)
DYN_CLEARED, DYN_AGED, DYN_CONFIRMED = 1, 2, 4
DYN_STATS = ("observations", "cleared", "aged", "confirmed")
DYN_EVENT_COLOUR = (255, 0, 255)
OBJ_FLAGS, OBJ_LABEL = range(2)
OBJ_DTYPE = [np.uint8, np.int32]
OBJ_CELL, OBJ_KEPT, OBJ_LARGE = 1, 2, 4
OBJ_RECORD = 10
OBJ_FIELDS = ("label", "size", "ga_min", "gb_min", "ga_max", "gb_max", "c16_a", "c16_b", "hmax_bits", "points")
OBJ_STATS = ("cells", "components", "kept", "kept_cells", "large", "low", "launches")
TRACK_RECORD = 14
TRACK_FIELDS = ("id", "flags", "age", "missed", "label", "size", "c16_a", "c16_b", "v16_a", "v16_b", "birth_a", "birth_b", "overlap", "hmax_bits")
TRACK_NEW, TRACK_BY_OVERLAP, TRACK_BY_GATE, TRACK_MISSED, TRACK_MOVING, TRACK_MERGED, TRACK_SPLIT = 1, 2, 4, 8, 16, 32, 64
TRACK_STATS = ("steps", "tracks", "by_overlap", "by_gate", "new", "missed", "dropped", "untracked")
ASSIGN_UNTRACKED = -2
OBJ_LARGE_COLOUR, OBJ_UNTRACKED_COLOUR, OBJ_CENTRE_COLOUR, OBJ_AHEAD_COLOUR = (128, 128, 128), (128, 0, 0), (255, 255, 255), (255, 255, 0)
POSE_CF, POSE_POT, POSE_DIR = 0, 1, 2
POSE_DTYPE = [np.uint8, np.int32, np.uint8]
POSE_HEADINGS = 8
POSE_DIR_GOAL, POSE_DIR_NONE = 8, 9
ROLL_CUT_OBJECT = 4
ROLL_PRED_RECORD = 6
ROLL_PRED_FIELDS = ROLL_FIELDS + ("slot",)
PRED_STATS = ("tracks", "sources", "cells", "launches")
TIME_TPOT, TIME_TDIR, TIME_RCOST, TIME_RPOT = 0, 1, 2, 3
TIME_DTYPE = [np.int32, np.uint8, np.uint8, np.int32]
TIME_WAIT = 10
TIME_STATS = ("layers", "reached", "blocked", "waits", "released", "rounds")
PRED_MAX_SLOTS, PRED_MAX_RADIUS = 32, 16
REGION_GRID, REGION_LOCAL = range(2)
RENDER_LOCAL = 3
ARCHIVE_STATS = ("pages", "max_tiles", "stored", "restored", "lost", "refused")
ARCHIVE_TILE, ARCHIVE_MAX_TILES, ARCHIVE_DEFAULT_TILES, ARCHIVE_PAGE_BYTES = 16, 2 ** 20, 16384, 11264
REGION_MAX_SIDE = 8192


class Params(C.Structure):
    """svh_grid_params"""
    _fields_ = [("nx", C.c_int32), ("nz", C.c_int32), ("cell", C.c_float), ("x0", C.c_float), ("z0", C.c_float),
                ("T", C.c_double * 12), ("min_points", C.c_int32), ("step", C.c_float), ("drop", C.c_float),
                ("clearance", C.c_float), ("render_h_lo", C.c_float), ("render_h_hi", C.c_float)]

    def copy(self, **kw):
        q = Params.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            if k == "T":
                q.T = (C.c_double * 12)(*np.asarray(v, np.float64).ravel())
            else:
                setattr(q, k, v)
        return q


class TravParams(C.Structure):
    """svh_grid_trav_params"""
    _fields_ = [("max_slope", C.c_float), ("inscribed", C.c_float), ("inflate", C.c_float), ("lethal", C.c_uint32)]

    def copy(self, **kw):
        q = TravParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PlanParams(C.Structure):
    """svh_grid_plan_params"""
    _fields_ = [("neutral", C.c_int32), ("unknown", C.c_int32), ("max_cost", C.c_int32)]

    def copy(self, **kw):
        q = PlanParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PoseParams(C.Structure):
    """svh_grid_pose_params"""
    _fields_ = [("neutral", C.c_int32), ("max_cost", C.c_int32), ("turn", C.c_int32), ("reverse", C.c_int32), ("spin", C.c_int32)]

    def copy(self, **kw):
        q = PoseParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TimeParams(C.Structure):
    """svh_grid_time_params"""
    _fields_ = [("layers", C.c_int32), ("wait", C.c_int32), ("release", C.c_int32)]

    def copy(self, **kw):
        q = TimeParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class FrontParams(C.Structure):
    """svh_grid_front_params"""
    _fields_ = [("max_cell_cost", C.c_int32), ("min_size", C.c_int32), ("unexplored", C.c_uint32), ("border", C.c_int32)]

    def copy(self, **kw):
        q = FrontParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ObjParams(C.Structure):
    """svh_grid_obj_params"""
    _fields_ = [("min_size", C.c_int32), ("max_size", C.c_int32), ("min_height", C.c_float), ("max_tracks", C.c_int32), ("min_overlap", C.c_int32),
                ("gate", C.c_int32), ("max_missed", C.c_int32), ("min_age", C.c_int32), ("move_cells", C.c_int32), ("smooth_shift", C.c_int32)]

    def copy(self, **kw):
        q = ObjParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PredParams(C.Structure):
    """svh_grid_pred_params"""
    _fields_ = [("slots", C.c_int32), ("stride", C.c_int32), ("poses_per_step", C.c_int32), ("margin", C.c_int32), ("grow16", C.c_int32),
                ("only_moving", C.c_int32)]

    def copy(self, **kw):
        q = PredParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RollParams(C.Structure):
    """svh_grid_roll_params"""
    _fields_ = [("front", C.c_float), ("rear", C.c_float), ("half_width", C.c_float), ("headings_m", C.c_int32), ("stop_cost", C.c_int32),
                ("unknown_cost", C.c_int32), ("w_pot", C.c_int32), ("w_cost", C.c_int32), ("w_cut", C.c_int32)]

    def copy(self, **kw):
        q = RollParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ExploreParams(C.Structure):
    """svh_grid_explore_params"""
    _fields_ = [("range", C.c_float), ("min_gain", C.c_int32), ("w_gain", C.c_int32), ("w_reach", C.c_int32)]

    def copy(self, **kw):
        q = ExploreParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AlignParams(C.Structure):
    """svh_grid_align_params"""
    _fields_ = [("reach", C.c_float), ("range", C.c_float), ("rot_den", C.c_int32), ("rot_n", C.c_int32), ("trans_n", C.c_int32),
                ("min_scan", C.c_int32)]

    def copy(self, **kw):
        q = AlignParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DynParams(C.Structure):
    """svh_grid_dyn_params"""
    _fields_ = [("clear_frames", C.c_int32), ("min_through", C.c_int32), ("margin", C.c_float), ("max_age", C.c_int32)]

    def copy(self, **kw):
        q = DynParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ArchiveParams(C.Structure):
    """svh_grid_archive_params"""
    _fields_ = [("max_tiles", C.c_int32)]

    def copy(self, **kw):
        q = ArchiveParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Stats(C.Structure):
    """svh_grid_stats"""
    _fields_ = [("added", C.c_int64), ("binned", C.c_int64), ("overhead", C.c_int64), ("outside", C.c_int64),
                ("unplaced", C.c_int64)]

    def asdict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}

    def __repr__(self):
        return "Stats(%s)" % ", ".join("%s=%d" % kv for kv in self.asdict().items())


def _bind():
    L = lib()
    if not getattr(L, "_grid_bound", False):
        L.svh_grid_params_default.argtypes = [C.POINTER(Params)]
        L.svh_grid_params_default.restype = None
        L.svh_grid_frame_camera.argtypes = [C.c_double, C.c_void_p]
        L.svh_grid_frame_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_grid_create.restype = C.c_void_p
        L.svh_grid_create.argtypes = [C.POINTER(Params)]
        L.svh_grid_destroy.argtypes = [C.c_void_p]
        L.svh_grid_destroy.restype = None
        L.svh_grid_clear.argtypes = [C.c_void_p]
        L.svh_grid_set_window.argtypes = [C.c_void_p, C.c_float, C.c_float]
        L.svh_grid_add_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.svh_grid_add_view.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.svh_grid_get.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_render.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_test_grid_points.argtypes = [C.POINTER(Params), C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.svh_test_grid_finalise.argtypes = [C.POINTER(Params), C.c_int64] + [C.c_void_p] * 12
        L.svh_grid_scroll.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.svh_grid_get_window.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_cell_of.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_grid_follow.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.svh_grid_add_points_from.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.svh_grid_add_view_lists_from.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.svh_grid_get_ray_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_get_local.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_render_local.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_test_grid_points_at.argtypes = [C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        L.svh_test_grid_line.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_test_grid_local.argtypes = [C.POINTER(Params), C.c_int64] + [C.c_void_p] * 5
        L.svh_grid_trav_params_default.argtypes = [C.POINTER(TravParams)]
        L.svh_grid_trav_params_default.restype = None
        L.svh_grid_set_traversability.argtypes = [C.c_void_p, C.POINTER(TravParams)]
        L.svh_grid_get_traversability.argtypes = [C.c_void_p, C.POINTER(TravParams), C.c_void_p]
        L.svh_grid_get_trav.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_render_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_test_grid_trav.argtypes = [C.POINTER(Params), C.POINTER(TravParams)] + [C.c_void_p] * 7
        L.svh_test_grid_cost_table.argtypes = [C.c_float, C.POINTER(TravParams), C.c_void_p, C.c_void_p, C.c_int64]
        L.svh_grid_plan_params_default.argtypes = [C.POINTER(PlanParams)]
        L.svh_grid_plan_params_default.restype = None
        L.svh_grid_set_plan.argtypes = [C.c_void_p, C.POINTER(PlanParams)]
        L.svh_grid_get_plan.argtypes = [C.c_void_p, C.POINTER(PlanParams)]
        L.svh_grid_plan_set_goals.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_grid_plan_set_goal.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_get_plan_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_get_plan_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_plan_path.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.svh_grid_render_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
        L.svh_test_grid_plan.argtypes = [C.POINTER(PlanParams)] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.svh_test_grid_path.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_test_grid_plan_tile.argtypes = []
        L.svh_test_grid_plan_device.argtypes = [C.c_int32, C.c_int32, C.POINTER(PlanParams), C.c_void_p, C.c_void_p, C.c_int32,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_grid_front_params_default.argtypes = [C.POINTER(FrontParams)]
        L.svh_grid_front_params_default.restype = None
        L.svh_grid_set_frontier.argtypes = [C.c_void_p, C.POINTER(FrontParams)]
        L.svh_grid_get_frontier.argtypes = [C.c_void_p, C.POINTER(FrontParams)]
        L.svh_grid_get_front_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_get_frontiers.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_get_frontier_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_plan_set_goals_frontiers.argtypes = [C.c_void_p]
        L.svh_grid_render_frontiers.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        front = [C.POINTER(FrontParams)] + [C.c_int32] * 4 + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_void_p]
        L.svh_test_grid_front.argtypes = front
        L.svh_test_grid_front_device.argtypes = front
        L.svh_test_grid_front_label_device.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_test_grid_front_tile.argtypes = []
        L.svh_grid_obj_params_default.argtypes = [C.POINTER(ObjParams)]
        L.svh_grid_obj_params_default.restype = None
        L.svh_grid_set_objects.argtypes = [C.c_void_p, C.POINTER(ObjParams)]
        L.svh_grid_get_objects_params.argtypes = [C.c_void_p, C.POINTER(ObjParams)]
        L.svh_grid_get_obj_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_get_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_get_object_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_objects_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_objects_reset.argtypes = [C.c_void_p]
        L.svh_grid_get_tracks.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_get_track_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.svh_grid_get_track_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_render_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        obj = [C.POINTER(ObjParams)] + [C.c_int32] * 4 + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p]
        L.svh_test_grid_obj.argtypes = obj
        L.svh_test_grid_obj_device.argtypes = obj
        L.svh_test_grid_obj_step.argtypes = ([C.POINTER(ObjParams)] + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6)
        L.svh_test_grid_obj_colour.argtypes = [C.c_int64] + [C.c_void_p] * 4
        L.svh_grid_pred_params_default.argtypes = [C.POINTER(PredParams)]
        L.svh_grid_pred_params_default.restype = None
        L.svh_grid_set_predict.argtypes = [C.c_void_p, C.POINTER(PredParams)]
        L.svh_grid_get_predict.argtypes = [C.c_void_p, C.POINTER(PredParams)]
        L.svh_grid_get_pred_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.svh_grid_get_pred_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_footprint_pred.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.svh_grid_roll_score_pred.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.svh_grid_render_pred.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        pred = [C.POINTER(PredParams), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.svh_test_grid_pred.argtypes = pred
        L.svh_test_grid_pred_device.argtypes = pred
        L.svh_test_grid_pred_slots.argtypes = [C.POINTER(PredParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.svh_test_grid_pred_roll.argtypes = ([C.POINTER(RollParams), C.POINTER(PredParams), C.c_float] + [C.c_int32] * 4 + [C.c_void_p] * 2 +
                                              [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_int32] * 6 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 4)
        L.svh_grid_roll_params_default.argtypes = [C.POINTER(RollParams)]
        L.svh_grid_roll_params_default.restype = None
        L.svh_grid_set_roll.argtypes = [C.c_void_p, C.POINTER(RollParams)]
        L.svh_grid_get_roll.argtypes = [C.c_void_p, C.POINTER(RollParams), C.c_void_p, C.c_void_p]
        L.svh_grid_heading_of.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_grid_roll_footprint.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_footprint_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.svh_grid_roll_set_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.svh_grid_roll_get_candidates.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_roll_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.svh_grid_render_roll.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_test_grid_roll_table.argtypes = [C.c_float, C.POINTER(RollParams), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_test_grid_roll_heading.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        roll = [C.POINTER(RollParams), C.c_float] + [C.c_int32] * 4 + [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        L.svh_test_grid_roll.argtypes = roll
        L.svh_test_grid_roll_device.argtypes = roll
        L.svh_test_grid_roll_group.argtypes = [C.c_int64]
        L.svh_grid_pose_params_default.argtypes = [C.POINTER(PoseParams)]
        L.svh_grid_pose_params_default.restype = None
        L.svh_grid_set_pose.argtypes = [C.c_void_p, C.POINTER(PoseParams)]
        L.svh_grid_get_pose.argtypes = [C.c_void_p, C.POINTER(PoseParams)]
        L.svh_grid_pose_set_goals.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_grid_pose_set_goal.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_grid_get_pose_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_get_pose_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_pose_heading_of.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.svh_grid_pose_path.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.svh_grid_render_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
        pose = ([C.POINTER(RollParams), C.POINTER(PoseParams), C.c_float] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p, C.c_int32] +
                [C.c_void_p] * 4)
        L.svh_test_grid_pose.argtypes = pose
        L.svh_test_grid_pose_device.argtypes = pose
        L.svh_grid_time_params_default.argtypes = [C.POINTER(TimeParams)]
        L.svh_grid_time_params_default.restype = None
        L.svh_grid_set_time.argtypes = [C.c_void_p, C.POINTER(TimeParams)]
        L.svh_grid_get_time.argtypes = [C.c_void_p, C.POINTER(TimeParams)]
        L.svh_grid_get_time_plane.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_get_time_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_time_path.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.svh_grid_render_time.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
        time_ = ([C.POINTER(PlanParams), C.POINTER(PredParams), C.POINTER(TimeParams), C.POINTER(TravParams), C.c_float] + [C.c_int32] * 4 +
                 [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6 +
                 [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p])
        L.svh_test_grid_time.argtypes = time_
        L.svh_test_grid_time_device.argtypes = time_
        L.svh_test_grid_pose_walk.argtypes = [C.c_int32] * 5 + [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_explore_params_default.argtypes = [C.POINTER(ExploreParams)]
        L.svh_grid_explore_params_default.restype = None
        L.svh_grid_set_explore.argtypes = [C.c_void_p, C.POINTER(ExploreParams)]
        L.svh_grid_get_explore.argtypes = [C.c_void_p, C.POINTER(ExploreParams), C.c_void_p]
        L.svh_grid_view_gain.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.svh_grid_view_mask.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_explore_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.svh_grid_plan_set_goal_explore.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_get_explore_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_render_view.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        explore = ([C.POINTER(FrontParams), C.POINTER(PlanParams), C.POINTER(ExploreParams), C.c_float] + [C.c_int32] * 4 + [C.c_void_p] * 3 +
                   [C.c_int64] + [C.c_void_p] * 7 + [C.c_int64] + [C.c_void_p] * 3)
        L.svh_test_grid_explore.argtypes = explore
        L.svh_test_grid_explore_device.argtypes = explore
        L.svh_grid_align_params_default.argtypes = [C.POINTER(AlignParams)]
        L.svh_grid_align_params_default.restype = None
        L.svh_grid_set_align.argtypes = [C.c_void_p, C.POINTER(AlignParams)]
        L.svh_grid_get_align_field.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_grid_align_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.svh_grid_align_view_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.svh_grid_get_align_volume.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_grid_get_align_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_align_correction.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.svh_grid_render_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        align = ([C.POINTER(Params), C.POINTER(AlignParams), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] +
                 [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3)
        L.svh_test_grid_align.argtypes = align
        L.svh_test_grid_align_device.argtypes = align
        L.svh_test_grid_align_form.argtypes = [C.c_int32]
        L.svh_grid_dyn_params_default.argtypes = [C.POINTER(DynParams)]
        L.svh_grid_dyn_params_default.restype = None
        L.svh_grid_set_dynamics.argtypes = [C.c_void_p, C.POINTER(DynParams)]
        L.svh_grid_get_dynamics.argtypes = [C.c_void_p, C.POINTER(DynParams)]
        L.svh_grid_observe_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.svh_grid_observe_view_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.svh_grid_get_dyn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.svh_grid_get_dyn_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_render_dyn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.svh_test_grid_dyn_params.argtypes = [C.POINTER(DynParams), C.c_void_p]
        L.svh_test_grid_dyn_height.argtypes = [C.c_int64] + [C.c_void_p] * 8
        L.svh_test_grid_dyn_through.argtypes = [C.POINTER(Params), C.POINTER(DynParams), C.c_int64] + [C.c_void_p] * 7
        L.svh_test_grid_dyn_settle.argtypes = [C.POINTER(Params), C.POINTER(DynParams), C.c_int32, C.c_int64] + [C.c_void_p] * 6
        L.svh_test_grid_dyn_colour.argtypes = [C.POINTER(Params), C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p]
        L.svh_grid_archive_params_default.argtypes = [C.POINTER(ArchiveParams)]
        L.svh_grid_archive_params_default.restype = None
        L.svh_grid_set_archive.argtypes = [C.c_void_p, C.POINTER(ArchiveParams)]
        L.svh_grid_get_archive.argtypes = [C.c_void_p, C.POINTER(ArchiveParams)]
        L.svh_grid_get_archive_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.svh_grid_archive_clear.argtypes = [C.c_void_p]
        L.svh_grid_archive_trim.argtypes = [C.c_void_p] + [C.c_int32] * 4
        L.svh_grid_archive_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.svh_grid_get_region.argtypes = [C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p, C.c_int32]
        L.svh_grid_render_region.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32]
        L.svh_test_grid_archive_key.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]
        L.svh_test_grid_archive_strip.argtypes = [C.c_int32] * 4 + [C.c_void_p, C.c_int64, C.c_void_p]
        L._grid_bound = True
    return L


def _check(rc):
    if rc < 0:
        raise SvhError(int(rc), last_error())
    return rc


def default_params(**kw):
    p = Params()
    _bind().svh_grid_params_default(C.byref(p))
    return p.copy(**kw)


def frame_camera(cam_height):
    """T [3, 4] of a level camera cam_height above the road: a = x, b = z, h = cam_height - y"""
    T = np.zeros((3, 4), np.float64)
    _check(_bind().svh_grid_frame_camera(cam_height, T.ctypes.data))
    return T


def frame_plane(plane_e, H):
    """T [3, 4] from PlaneEstimation's plane_euclidean() and transformation(); SvhError when no plane was found"""
    e = np.ascontiguousarray(plane_e, np.float64).reshape(3)
    Hm = np.ascontiguousarray(H, np.float64).reshape(16)
    T = np.zeros((3, 4), np.float64)
    _check(_bind().svh_grid_frame_plane(e.ctypes.data, Hm.ctypes.data, T.ctypes.data))
    return T


def core_points(params, xyzv):
    """csrc/grid_core.h on the host (svh_test_grid_points): (fate int32, cell uint32, key uint32, q int32, v uint8) per
    point; needs no device"""
    p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
    n = len(p)
    out = (np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.uint8))
    _check(_bind().svh_test_grid_points(C.byref(params), p.ctypes.data if n else None, n, *[a.ctypes.data for a in out]))
    return out


def core_finalise(params, count, overhead, kmin, kmax, hsum, vsum):
    """csrc/grid_core.h on the host (svh_test_grid_finalise): (hmin, hmax, hmean, intensity, class, rgb [n, 3, 3]) per
    accumulated cell; needs no device"""
    ins = [np.ascontiguousarray(a, t).ravel() for a, t in ((count, np.int32), (overhead, np.int32), (kmin, np.uint32),
                                                            (kmax, np.uint32), (hsum, np.int64), (vsum, np.uint64))]
    n = len(ins[0])
    out = [np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8),
           np.zeros(n, np.uint8), np.zeros((n, 3, 3), np.uint8)]
    _check(_bind().svh_test_grid_finalise(C.byref(params), n, *[a.ctypes.data for a in ins + out]))
    return tuple(out)


def core_points_at(params, oa, ob, xyzv):
    """place() of csrc/grid_core.h under window offsets (oa, ob), on the host: (fate int32, logical cell uint32, slot uint32)"""
    p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
    n = len(p)
    out = (np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    _check(_bind().svh_test_grid_points_at(C.byref(params), oa, ob, p.ctypes.data if n else None, n, *[a.ctypes.data for a in out]))
    return out


def core_line(oa, ob, ea, eb):
    """the line of csrc/grid_core.h from cell (oa, ob) to cell (ea, eb), on the host: [n, 2] int32, the end cell excluded"""
    n = C.c_int32(-1)
    cap = max(abs(ea - oa), abs(eb - ob), 1)
    cells = np.zeros((cap, 2), np.int32)
    _check(_bind().svh_test_grid_line(oa, ob, ea, eb, C.addressof(n), cells.ctypes.data, cap))
    return cells[:n.value].copy()


def core_local(params, cls, intensity, pass_):
    """state byte and local colour of csrc/grid_core.h on the host: (state uint8 [n], rgb uint8 [n, 3])"""
    ins = [np.ascontiguousarray(cls, np.uint8).ravel(), np.ascontiguousarray(intensity, np.uint8).ravel(),
           np.ascontiguousarray(pass_, np.int32).ravel()]
    n = len(ins[0])
    out = [np.zeros(n, np.uint8), np.zeros((n, 3), np.uint8)]
    _check(_bind().svh_test_grid_local(C.byref(params), n, *[a.ctypes.data for a in ins + out]))
    return tuple(out)


def default_trav(**kw):
    t = TravParams()
    _bind().svh_grid_trav_params_default(C.byref(t))
    return t.copy(**kw)


def core_trav(params, trav, cls, hmean, state):
    """the traversability layer of csrc/grid_core.h on the host (svh_test_grid_trav) for a window of params.nx x params.nz
    cells: (flags uint8, dist2 int32, cost uint8, each [nz, nx]; rgb uint8 [nz, nx, 3] in cell order); needs no device"""
    sh = (params.nz, params.nx)
    ins = [np.ascontiguousarray(cls, np.uint8).reshape(sh), np.ascontiguousarray(hmean, np.float32).reshape(sh),
           np.ascontiguousarray(state, np.uint8).reshape(sh)]
    out = [np.zeros(sh, np.uint8), np.zeros(sh, np.int32), np.zeros(sh, np.uint8), np.zeros(sh + (3,), np.uint8)]
    _check(_bind().svh_test_grid_trav(C.byref(params), C.byref(trav), *[a.ctypes.data for a in ins + out]))
    return tuple(out)


def core_cost_table(cell, trav):
    """the cost table of csrc/grid_core.h for a cell side (svh_test_grid_cost_table): uint8 [reach^2 + 1]; needs no device"""
    reach = C.c_int32(0)
    L = _bind()
    _check(L.svh_test_grid_cost_table(cell, C.byref(trav), C.addressof(reach), None, 0))
    table = np.zeros(reach.value ** 2 + 1, np.uint8)
    _check(L.svh_test_grid_cost_table(cell, C.byref(trav), C.addressof(reach), table.ctypes.data, len(table)))
    return table


def default_plan(**kw):
    p = PlanParams()
    _bind().svh_grid_plan_params_default(C.byref(p))
    return p.copy(**kw)


def _cells(cells):
    c = np.ascontiguousarray(cells, np.int32).reshape(-1, 2)
    return c, (c.ctypes.data if len(c) else None)


def core_plan(params, plan, cost, goals, oa=0, ob=0):
    """the planner of csrc/grid_plan_core.h on the host (svh_test_grid_plan), a heap Dijkstra, for a window of params.nx x
    params.nz cells under the offsets (oa, ob): (pot int32, dir uint8, each [nz, nx]; the goals that count); needs no device"""
    sh = (params.nz, params.nx)
    c = np.ascontiguousarray(cost, np.uint8).reshape(sh)
    g, gp = _cells(goals)
    pot, dir_ = np.zeros(sh, np.int32), np.zeros(sh, np.uint8)
    n = _check(_bind().svh_test_grid_plan(C.byref(plan), params.nx, params.nz, oa, ob, c.ctypes.data, gp, len(g), pot.ctypes.data,
                                          dir_.ctypes.data))
    return pot, dir_, n


def core_path(dir_, a, b, oa=0, ob=0):
    """the walk of csrc/grid_plan_core.h over a DIR plane [nz, nx] from the window cell (a, b), on the host: [n, 2] int32
    global cells, n = 0 where DIR leads to no goal; needs no device"""
    d = np.ascontiguousarray(dir_, np.uint8)
    nz, nx = d.shape
    cells, n = np.zeros((nx * nz, 2), np.int32), C.c_int64(-1)
    _check(_bind().svh_test_grid_path(nx, nz, oa, ob, d.ctypes.data, a, b, cells.ctypes.data, nx * nz, C.addressof(n)))
    return cells[:n.value].copy()


def plan_tile():
    """the tile side the planner's kernels were built with"""
    return int(_bind().svh_test_grid_plan_tile())


def device_plan(nx, nz, plan, cost, goals):
    """TEST ENTRY: the planner's device kernels on a caller's cost plane (uint8 [nz, nx], window offsets 0):
    (pot int32 [nz, nx], dir uint8 [nz, nx], rounds)"""
    c = np.ascontiguousarray(cost, np.uint8).reshape(nz, nx)
    g, gp = _cells(goals)
    pot, dir_, out = np.zeros((nz, nx), np.int32), np.zeros((nz, nx), np.uint8), np.zeros(3, np.int64)
    _check(_bind().svh_test_grid_plan_device(nx, nz, C.byref(plan), c.ctypes.data, gp, len(g), pot.ctypes.data, dir_.ctypes.data,
                                             out.ctypes.data))
    return pot, dir_, int(out[2])


def default_front(**kw):
    p = FrontParams()
    _bind().svh_grid_front_params_default(C.byref(p))
    return p.copy(**kw)


def _front(entry, front, state, cost, oa, ob):
    s = np.ascontiguousarray(state, np.uint8)
    nz, nx = s.shape
    c = np.ascontiguousarray(cost, np.uint8).reshape(nz, nx)
    flags, label = np.zeros((nz, nx), np.uint8), np.zeros((nz, nx), np.int32)
    cap = ((nx + 1) // 2) * ((nz + 1) // 2)             # components do not touch: at most one per 2 x 2 cells
    recs, n, stats = np.zeros((cap, FRONT_RECORD), np.int32), C.c_int64(-1), np.zeros(5, np.int64)
    _check(entry(C.byref(front), nx, nz, oa, ob, s.ctypes.data, c.ctypes.data, flags.ctypes.data, label.ctypes.data, recs.ctypes.data, cap,
                 C.addressof(n), stats.ctypes.data))
    return flags, label, recs[:n.value].copy(), tuple(int(v) for v in stats)


def core_front(front, state, cost, oa=0, ob=0):
    """the frontiers of csrc/grid_front_core.h on the host (svh_test_grid_front) for STATE and COST planes [nz, nx] under the
    offsets (oa, ob): (flags uint8 [nz, nx], label int32 [nz, nx], records int32 [kept, 10], stats (5)); needs no device"""
    return _front(_bind().svh_test_grid_front, front, state, cost, oa, ob)


def device_front(front, state, cost, oa=0, ob=0):
    """TEST ENTRY: the same through the device kernels on a caller's planes"""
    return _front(_bind().svh_test_grid_front_device, front, state, cost, oa, ob)


def device_front_label(mask):
    """TEST ENTRY: the labelling stage of the frontiers alone on a mask [nz, nx] (nonzero: a cell to label):
    (label int32 [nz, nx], kernel launches)"""
    m = np.ascontiguousarray(mask, np.uint8)
    nz, nx = m.shape
    label, launches = np.zeros((nz, nx), np.int32), C.c_int64(-1)
    _check(_bind().svh_test_grid_front_label_device(nx, nz, m.ctypes.data, label.ctypes.data, C.addressof(launches)))
    return label, launches.value


def front_tile():
    """the tile side the labelling kernel of the frontiers was built with"""
    return int(_bind().svh_test_grid_front_tile())


def default_obj(**kw):
    p = ObjParams()
    _bind().svh_grid_obj_params_default(C.byref(p))
    return p.copy(**kw)


def _obj(entry, obj, state, hmax, count, oa, ob):
    s = np.ascontiguousarray(state, np.uint8)
    nz, nx = s.shape
    h, c = np.ascontiguousarray(hmax, np.float32).reshape(nz, nx), np.ascontiguousarray(count, np.int32).reshape(nz, nx)
    flags, label = np.zeros((nz, nx), np.uint8), np.zeros((nz, nx), np.int32)
    cap = ((nx + 1) // 2) * ((nz + 1) // 2)             # components do not touch: at most one per 2 x 2 cells
    recs, n, stats = np.zeros((cap, OBJ_RECORD), np.int32), C.c_int64(-1), np.zeros(7, np.int64)
    _check(entry(C.byref(obj), nx, nz, oa, ob, s.ctypes.data, h.ctypes.data, c.ctypes.data, flags.ctypes.data, label.ctypes.data,
                 recs.ctypes.data, cap, C.addressof(n), stats.ctypes.data))
    return flags, label, recs[:n.value].copy(), tuple(int(v) for v in stats)


def core_obj(obj, state, hmax, count, oa=0, ob=0):
    """the objects of csrc/grid_obj_core.h on the host (svh_test_grid_obj) for STATE, HMAX and COUNT planes [nz, nx] under the offsets
    (oa, ob): (flags uint8 [nz, nx], label int32 [nz, nx], records int32 [kept, 10], stats (7)); needs no device"""
    return _obj(_bind().svh_test_grid_obj, obj, state, hmax, count, oa, ob)


def device_obj(obj, state, hmax, count, oa=0, ob=0):
    """TEST ENTRY: the same through the device kernels on a caller's planes"""
    return _obj(_bind().svh_test_grid_obj_device, obj, state, hmax, count, oa, ob)


def core_obj_step(obj, recs, label, off, prev_id, prev_off, prev, next_id):
    """one step of the tracks of csrc/grid_obj_core.h on the host (svh_test_grid_obj_step): the object records [n, 10] and LABEL plane
    [nz, nx] of a window under off = (oa, ob), the ID plane of the step before (or None) under prev_off, its track records [m, 14] and
    the next id -> (tracks int32 [k, 14], assign int32 [n], id int32 [nz, nx], stats (8; steps is 0), next id); needs no device"""
    lab = np.ascontiguousarray(label, np.int32)
    nz, nx = lab.shape
    r = np.ascontiguousarray(recs, np.int32).reshape(-1, OBJ_RECORD)
    t = np.ascontiguousarray(prev, np.int32).reshape(-1, TRACK_RECORD)
    pid = None if prev_id is None else np.ascontiguousarray(prev_id, np.int32).reshape(nz, nx)
    tracks, n_tracks = np.zeros((obj.max_tracks, TRACK_RECORD), np.int32), C.c_int32(-1)
    assign, ids, stats, nxt = np.zeros(max(len(r), 1), np.int32), np.zeros((nz, nx), np.int32), np.zeros(8, np.int64), C.c_int32(-1)
    _check(_bind().svh_test_grid_obj_step(C.byref(obj), nx, nz, off[0], off[1], r.ctypes.data if len(r) else None, len(r), lab.ctypes.data,
                                          prev_off[0], prev_off[1], None if pid is None else pid.ctypes.data, t.ctypes.data if len(t) else None,
                                          len(t), next_id, tracks.ctypes.data, C.addressof(n_tracks), assign.ctypes.data, ids.ctypes.data,
                                          stats.ctypes.data, C.addressof(nxt)))
    return tracks[:n_tracks.value].copy(), assign[:len(r)].copy(), ids, tuple(int(v) for v in stats), nxt.value


def core_obj_colour(flags, ids, moving):
    """colour_obj of csrc/grid_obj_core.h on the host, per cell: (rgb uint8 [n, 3], zero where the cell keeps its colour)"""
    f, i, m = np.ascontiguousarray(flags, np.uint8).ravel(), np.ascontiguousarray(ids, np.int32).ravel(), np.ascontiguousarray(moving, np.uint8).ravel()
    rgb = np.zeros((len(f), 3), np.uint8)
    _check(_bind().svh_test_grid_obj_colour(len(f), f.ctypes.data, i.ctypes.data, m.ctypes.data, rgb.ctypes.data))
    return rgb


def default_roll(**kw):
    p = RollParams()
    _bind().svh_grid_roll_params_default(C.byref(p))
    return p.copy(**kw)


def core_roll_table(cell, roll):
    """the footprint table of csrc/grid_roll_core.h for a cell side (svh_test_grid_roll_table): (R, [int32 [n_k, 2] offsets (da, db) for
    each of the 8 m headings]); needs no device"""
    L, R, total, n = _bind(), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    _check(L.svh_test_grid_roll_table(cell, C.byref(roll), C.addressof(R), C.addressof(total), -1, None, 0, None))
    lists = []
    for k in range(8 * roll.headings_m):
        _check(L.svh_test_grid_roll_table(cell, C.byref(roll), C.addressof(R), None, k, None, 0, C.addressof(n)))
        offs = np.zeros((max(n.value, 1), 2), np.int32)
        _check(L.svh_test_grid_roll_table(cell, C.byref(roll), C.addressof(R), None, k, offs.ctypes.data, n.value, C.addressof(n)))
        lists.append(offs[:n.value].copy())
    assert sum(len(l) for l in lists) == total.value
    return R.value, lists


def core_heading(m, ua, ub):
    """the heading of a direction by csrc/grid_roll_core.h (svh_test_grid_roll_heading): (k, (ux, uz)), or (-1, None); needs no device"""
    k, vec = C.c_int32(-9), np.zeros(2, np.int32)
    _check(_bind().svh_test_grid_roll_heading(m, ua, ub, C.addressof(k), vec.ctypes.data))
    return k.value, ((int(vec[0]), int(vec[1])) if k.value >= 0 else None)


def headings_of(m, ua, ub):
    """the same rule in numpy float32, elementwise: int32, -1 where a direction has no heading"""
    ua, ub = np.broadcast_arrays(np.asarray(ua, np.float32), np.asarray(ub, np.float32))
    aa, ab, fm = np.abs(ua), np.abs(ub), np.float32(m)
    wide = aa >= ab
    with np.errstate(all="ignore"):
        q = np.rint(np.where(wide, ub * fm, ua * fm) / np.where(wide, aa, ab))
    ok = np.isfinite(ua) & np.isfinite(ub) & ((ua != 0) | (ub != 0)) & (np.abs(q) <= fm)
    q = np.where(ok, q, 0).astype(np.int64)
    k = np.where(wide, np.where(ua > 0, (q + 8 * m) % (8 * m), 4 * m - q), np.where(ub > 0, 2 * m - q, 6 * m + q))
    return np.where(ok, k, -1).astype(np.int32)


def heading_vectors(m):
    """int64 [8 m, 2]: the vector (ux, uz) of every heading"""
    k = np.arange(8 * m)
    ux = np.select([k <= m, k <= 3 * m, k <= 5 * m, k <= 7 * m], [m, 2 * m - k, -m, k - 6 * m], m)
    uz = np.select([k <= m, k <= 3 * m, k <= 5 * m, k <= 7 * m], [k, m, 4 * m - k, -m], k - 8 * m)
    return np.stack([ux, uz], axis=1).astype(np.int64)


def arc_candidates(cell, m, curvatures, step_len, T):
    """int32 [8 m, K, T, 3]: set s holds, for each of the K curvatures (1/m, positive turns towards rising headings), the arc that
    starts at the anchor along heading s, sampled every step_len metres: pose t lies (t + 1) step_len along it.  numpy double; a cell
    offset is floor(x / cell + 0.5), the heading that of the tangent.  A candidate ends (k = -1 from there on) where an offset would
    leave +-16384.  Plumbing, not part of the contract"""
    kap = np.asarray(curvatures, np.float64).reshape(1, -1, 1)
    u = heading_vectors(m).astype(np.float64)
    u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
    ua, ub = u[:, 0].reshape(-1, 1, 1), u[:, 1].reshape(-1, 1, 1)
    s = (np.arange(T, dtype=np.float64) + 1.0).reshape(1, 1, -1) * float(step_len)
    phi = kap * s
    safe = np.where(kap == 0, 1.0, kap)
    along = np.where(kap == 0, s, np.sin(phi) / safe)                 # along the start heading
    left = np.where(kap == 0, 0.0, (1.0 - np.cos(phi)) / safe)        # along its left normal (-ub, ua)
    xa, xb = along * ua - left * ub, along * ub + left * ua
    ta, tb = np.cos(phi) * ua - np.sin(phi) * ub, np.cos(phi) * ub + np.sin(phi) * ua
    da, db = np.floor(xa / float(cell) + 0.5), np.floor(xb / float(cell) + 0.5)
    k = headings_of(m, ta.astype(np.float32), tb.astype(np.float32))
    live = np.logical_and.accumulate((np.abs(da) <= 16384) & (np.abs(db) <= 16384) & (k >= 0), axis=2)
    out = np.zeros(da.shape + (3,), np.int32)
    out[..., 0], out[..., 1], out[..., 2] = np.where(live, da, 0), np.where(live, db, 0), np.where(live, k, -1)
    return out


def _roll(entry, roll, cell, cost, pot, table, set_, anchor, oa, ob, poses):
    c = np.ascontiguousarray(cost, np.uint8)
    nz, nx = c.shape
    p = None if pot is None else np.ascontiguousarray(pot, np.int32).reshape(nz, nx)
    out = {}
    S = K = T = 0
    tp = rp = sp = None
    best = C.c_int32(-9)
    if table is not None:
        t = np.ascontiguousarray(table, np.int32)
        S, K, T = t.shape[:3]
        recs, scores = np.zeros((K, ROLL_RECORD), np.int32), np.zeros(K, np.int64)
        tp, rp, sp = t.ctypes.data, recs.ctypes.data, scores.ctypes.data
    q = np.ascontiguousarray(poses if poses is not None else np.zeros((0, 3)), np.int32).reshape(-1, 3)
    f = np.zeros(len(q), np.int32)
    _check(entry(C.byref(roll), cell, nx, nz, oa, ob, c.ctypes.data, None if p is None else p.ctypes.data, tp, S, K, T, set_, anchor[0], anchor[1],
                 q.ctypes.data if len(q) else None, len(q), f.ctypes.data if len(q) else None, rp, sp, C.addressof(best)))
    if table is not None:
        out.update(recs=recs, scores=scores, best=best.value)
    if poses is not None:
        out.update(f=f)
    return out


def core_roll(roll, cell, cost, pot=None, table=None, set_=0, anchor=(0, 0), oa=0, ob=0, poses=None):
    """the rollouts of csrc/grid_roll_core.h on the host (svh_test_grid_roll) on COST uint8 [nz, nx] and POT int32 [nz, nx] (needed when
    w_pot != 0) under the offsets (oa, ob): with a table int32 [S, K, T, 3], set `set_` scored at the global cell `anchor` -- recs int32
    [K, 5], scores int64 [K], best; with poses int32 [n, 3] (global cells, heading) their F as f int32 [n].  A dict; needs no device"""
    return _roll(_bind().svh_test_grid_roll, roll, cell, cost, pot, table, set_, anchor, oa, ob, poses)


def device_roll(roll, cell, cost, pot=None, table=None, set_=0, anchor=(0, 0), oa=0, ob=0, poses=None):
    """TEST ENTRY: the same through the device kernels on a caller's planes"""
    return _roll(_bind().svh_test_grid_roll_device, roll, cell, cost, pot, table, set_, anchor, oa, ob, poses)


def default_pose(**kw):
    p = PoseParams()
    _bind().svh_grid_pose_params_default(C.byref(p))
    return p.copy(**kw)


def _triples(triples):
    t = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    return t, (t.ctypes.data if len(t) else None)


def _pose(entry, roll, pose, cell, cost, goals, oa, ob):
    c = np.ascontiguousarray(cost, np.uint8)
    nz, nx = c.shape
    g, gp = _triples(goals)
    sh = (POSE_HEADINGS, nz, nx)
    cf, pot, dir_, out = np.zeros(sh, np.uint8), np.zeros(sh, np.int32), np.zeros(sh, np.uint8), np.zeros(3, np.int64)
    _check(entry(C.byref(roll), C.byref(pose), cell, nx, nz, oa, ob, c.ctypes.data, gp, len(g), cf.ctypes.data, pot.ctypes.data,
                 dir_.ctypes.data, out.ctypes.data))
    return cf, pot, dir_, out


def core_pose(roll, pose, cell, cost, goals, oa=0, ob=0):
    """the pose planner of csrc/grid_pose_core.h on the host (svh_test_grid_pose) for the vehicle of `roll` on cells of side `cell`, a
    COST plane uint8 [nz, nx] under the offsets (oa, ob) and goal triples (ga, gb, d): (cf uint8, pot int32, dir uint8, each
    [8, nz, nx]; the goal states that count); needs no device"""
    cf, pot, dir_, out = _pose(_bind().svh_test_grid_pose, roll, pose, cell, cost, goals, oa, ob)
    return cf, pot, dir_, int(out[0])


def device_pose(roll, pose, cell, cost, goals, oa=0, ob=0):
    """TEST ENTRY: the same through the kernels of csrc/grid_pose_kernels.hip: (cf, pot, dir, (counted, reached, rounds))"""
    cf, pot, dir_, out = _pose(_bind().svh_test_grid_pose_device, roll, pose, cell, cost, goals, oa, ob)
    return cf, pot, dir_, tuple(int(v) for v in out)


def core_pose_walk(dir_, a, b, d, m=1, oa=0, ob=0, cap=None):
    """the walk of csrc/grid_pose_core.h over a PDIR field [8, nz, nx] from the window state (a, b, d), on the host: (poses [n, 3]
    int32 (ga, gb, d m), the length of the whole path; 0 where PDIR leads to no goal); needs no device"""
    f = np.ascontiguousarray(dir_, np.uint8)
    _, nz, nx = f.shape
    room = POSE_HEADINGS * nx * nz if cap is None else int(cap)
    poses, n = np.zeros((max(room, 1), 3), np.int32), C.c_int64(-1)
    _check(_bind().svh_test_grid_pose_walk(nx, nz, oa, ob, m, f.ctypes.data, a, b, d, poses.ctypes.data if room else None, room, C.addressof(n)))
    return poses[:min(n.value, room)].copy(), n.value


def default_time(**kw):
    p = TimeParams()
    _bind().svh_grid_time_params_default(C.byref(p))
    return p.copy(**kw)


def _time(entry, plan, pred, time, cost, flags, goals, plane, oa, ob, pred_off, ids, tracks, cls, trav, cell, start, cap):
    c = np.ascontiguousarray(cost, np.uint8)
    nz, nx = c.shape
    f = np.ascontiguousarray(flags if flags is not None else np.zeros((nz, nx)), np.uint8).reshape(nz, nx)
    w = np.ascontiguousarray(plane if plane is not None else np.zeros((nz, nx)), np.uint32).reshape(nz, nx)
    g = np.ascontiguousarray(goals, np.int32).reshape(-1, 2)
    i = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(nz, nx)
    t = np.ascontiguousarray(tracks if tracks is not None else np.zeros((0, TRACK_RECORD)), np.int32).reshape(-1, TRACK_RECORD)
    k = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(nz, nx)
    L = time.layers
    tpot, tdir = np.zeros((max(L, 1), nz, nx), np.int32), np.zeros((max(L, 1), nz, nx), np.uint8)
    rcost, rpot, rdir = np.zeros((nz, nx), np.uint8), np.zeros((nz, nx), np.int32), np.zeros((nz, nx), np.uint8)
    stats, walk = np.zeros(6, np.int64), np.zeros(3, np.int64)
    a, b = start if start is not None else (-1, -1)
    room = (max(L, 0) + nx * nz if cap is None else int(cap)) if start is not None else 0
    triples = np.zeros((max(room, 1), 3), np.int32)
    _check(entry(C.byref(plan), C.byref(pred), C.byref(time), None if trav is None else C.byref(trav), cell, nx, nz, oa, ob, c.ctypes.data,
                 f.ctypes.data, None if k is None else k.ctypes.data, g.ctypes.data if len(g) else None, len(g), w.ctypes.data, pred_off[0],
                 pred_off[1], None if i is None else i.ctypes.data, t.ctypes.data if len(t) else None, len(t), tpot.ctypes.data, tdir.ctypes.data,
                 rcost.ctypes.data, rpot.ctypes.data, rdir.ctypes.data, stats.ctypes.data, a, b, triples.ctypes.data if room else None, room,
                 walk.ctypes.data))
    out = dict(tpot=tpot, tdir=tdir, rcost=rcost, rpot=rpot, rdir=rdir, stats=tuple(int(v) for v in stats))
    if start is not None:
        out.update(status=int(walk[0]), path_len=int(walk[1]), cost=int(walk[2]), path=triples[:min(int(walk[1]), room)].copy())
    return out


def core_time(plan, pred, time, cost, flags=None, goals=(), plane=None, oa=0, ob=0, pred_off=(0, 0), ids=None, tracks=None, cls=None, trav=None,
              cell=0.0, start=None, cap=None):
    """the time layer of csrc/grid_time_core.h on the host (svh_test_grid_time): the COST and FLAGS planes uint8 [nz, nx] of a window under
    (oa, ob), the planner's goals (global cells), the PRED plane uint32 [nz, nx] under pred_off (None: all 0) and, for release = 1, the ID
    plane of that frame, the track records [n, 14], the CLASS plane and the traversability parameters on cells of side `cell`.  A dict:
    tpot int32 and tdir uint8 [L, nz, nx], rcost, rpot, rdir [nz, nx], stats (6; the rounds are 0) and, with start = (a, b) a window
    cell, status, path int32 [n, 3], path_len, cost.  Needs no device"""
    return _time(_bind().svh_test_grid_time, plan, pred, time, cost, flags, goals, plane, oa, ob, pred_off, ids, tracks, cls, trav, cell, start, cap)


def device_time(plan, pred, time, cost, flags=None, goals=(), plane=None, oa=0, ob=0, pred_off=(0, 0), ids=None, tracks=None, cls=None, trav=None,
                cell=0.0, start=None, cap=None):
    """TEST ENTRY: the same through the kernels of csrc/grid_time_kernels.hip; stats[5] the rounds of RPOT"""
    return _time(_bind().svh_test_grid_time_device, plan, pred, time, cost, flags, goals, plane, oa, ob, pred_off, ids, tracks, cls, trav, cell, start, cap)


def default_pred(**kw):
    p = PredParams()
    _bind().svh_grid_pred_params_default(C.byref(p))
    return p.copy(**kw)


def _pred(entry, pred, ids, tracks, shape):
    t = np.ascontiguousarray(tracks, np.int32).reshape(-1, TRACK_RECORD)
    i = None if ids is None else np.ascontiguousarray(ids, np.int32)
    nz, nx = shape if i is None else i.shape
    out, stats = np.zeros((nz, nx), np.uint32), np.zeros(4, np.int64)
    _check(entry(C.byref(pred), nx, nz, None if i is None else i.ctypes.data, t.ctypes.data if len(t) else None, len(t), out.ctypes.data,
                 stats.ctypes.data))
    return out, tuple(int(v) for v in stats)


def core_pred(pred, ids, tracks, shape=None):
    """PRED of csrc/grid_pred_core.h on the host (svh_test_grid_pred) from the ID plane int32 [nz, nx] (None with shape = (nz, nx): all
    -1) and the track records [n, 14]: (pred uint32 [nz, nx], stats (4; the launches are 0)); needs no device"""
    return _pred(_bind().svh_test_grid_pred, pred, ids, tracks, shape)


def device_pred(pred, ids, tracks, shape=None):
    """TEST ENTRY: the same through the device kernels on a caller's plane and table; stats[3] the launches"""
    return _pred(_bind().svh_test_grid_pred_device, pred, ids, tracks, shape)


def core_pred_slots(pred, T=0, v16=()):
    """the small functions of csrc/grid_pred_core.h on the host (svh_test_grid_pred_slots): (slot int32 [T] of the poses, radius int32
    [32] of the slots, ge uint32 [17] the slots whose radius is at least r, disp int32 [n, 32] of the velocities v16 on one axis)"""
    v = np.ascontiguousarray(v16, np.int32).ravel()
    slot, radius, ge, disp = np.zeros(max(T, 1), np.int32), np.zeros(32, np.int32), np.zeros(17, np.uint32), np.zeros((max(len(v), 1), 32), np.int32)
    _check(_bind().svh_test_grid_pred_slots(C.byref(pred), T, slot.ctypes.data, radius.ctypes.data, ge.ctypes.data, v.ctypes.data if len(v) else None,
                                            len(v), disp.ctypes.data if len(v) else None))
    return slot[:T].copy(), radius, ge, disp[:len(v)].copy()


def core_pred_roll(roll, pred, cell, cost, plane, pot=None, table=None, set_=0, anchor=(0, 0), oa=0, ob=0, pred_off=(0, 0), poses=None):
    """the scoring with prediction of csrc/grid_pred_core.h on the host (svh_test_grid_pred_roll): the arguments of core_roll, the
    prediction parameters and the PRED plane uint32 [nz, nx] under pred_off.  With a table: recs int32 [K, 6], scores int64 [K], best;
    with poses int32 [n, 3] their footprint predictions as mask uint32 [n].  A dict; needs no device"""
    c = np.ascontiguousarray(cost, np.uint8)
    nz, nx = c.shape
    p = None if pot is None else np.ascontiguousarray(pot, np.int32).reshape(nz, nx)
    w = np.ascontiguousarray(plane, np.uint32).reshape(nz, nx)
    out = {}
    S = K = T = 0
    tp = rp = sp = None
    best = C.c_int32(-9)
    if table is not None:
        t = np.ascontiguousarray(table, np.int32)
        S, K, T = t.shape[:3]
        recs, scores = np.zeros((K, ROLL_PRED_RECORD), np.int32), np.zeros(K, np.int64)
        tp, rp, sp = t.ctypes.data, recs.ctypes.data, scores.ctypes.data
    q = np.ascontiguousarray(poses if poses is not None else np.zeros((0, 3)), np.int32).reshape(-1, 3)
    m = np.zeros(len(q), np.uint32)
    _check(_bind().svh_test_grid_pred_roll(C.byref(roll), C.byref(pred), cell, nx, nz, oa, ob, c.ctypes.data, None if p is None else p.ctypes.data,
                                           pred_off[0], pred_off[1], w.ctypes.data, tp, S, K, T, set_, anchor[0], anchor[1],
                                           q.ctypes.data if len(q) else None, len(q), m.ctypes.data if len(q) else None, rp, sp, C.addressof(best)))
    if table is not None:
        out.update(recs=recs, scores=scores, best=best.value)
    if poses is not None:
        out.update(mask=m)
    return out


def roll_group(longest):
    """the lanes that share a pose in the rollout kernels when the longest footprint list has `longest` cells"""
    return int(_bind().svh_test_grid_roll_group(longest))


def default_explore(**kw):
    p = ExploreParams()
    _bind().svh_grid_explore_params_default(C.byref(p))
    return p.copy(**kw)


def _explore(entry, explore, cell, state, cost, front, plan, oa, ob, cells, view, rgb, start):
    s = np.ascontiguousarray(state, np.uint8)
    nz, nx = s.shape
    c = None if cost is None else np.ascontiguousarray(cost, np.uint8).reshape(nz, nx)
    front = front if front is not None else default_front()
    plan = plan if plan is not None else default_plan()
    out = {}
    q = np.ascontiguousarray(cells if cells is not None else np.zeros((0, 2)), np.int32).reshape(-1, 2)
    gains = np.zeros(len(q), np.int32)
    v = None if view is None else np.ascontiguousarray(view, np.int32).reshape(2)
    mask = None if view is None else np.zeros((nz, nx), np.uint8)
    img = None if (view is None or rgb is None) else np.array(rgb, np.uint8).reshape(nz, nx, 3)
    st = None if start is None else np.ascontiguousarray(start, np.int32).reshape(2)
    cap = ((nx + 1) // 2) * ((nz + 1) // 2) if start is not None else 0
    recs, scores = np.zeros((max(cap, 1), EXPLORE_RECORD), np.int32), np.zeros(max(cap, 1), np.int64)
    n, best, stats = C.c_int64(-1), C.c_int32(-9), np.zeros(2, np.int64)
    _check(entry(C.byref(front), C.byref(plan), C.byref(explore), cell, nx, nz, oa, ob, s.ctypes.data, None if c is None else c.ctypes.data,
                 q.ctypes.data if len(q) else None, len(q), gains.ctypes.data if len(q) else None,
                 None if v is None else v.ctypes.data, None if mask is None else mask.ctypes.data, None if img is None else img.ctypes.data,
                 None if st is None else st.ctypes.data, recs.ctypes.data if cap else None, scores.ctypes.data if cap else None, cap,
                 C.addressof(n), C.addressof(best), stats.ctypes.data))
    if cells is not None:
        out.update(gains=gains)
    if view is not None:
        out.update(mask=mask)
        if img is not None:
            out.update(image=img)
    if start is not None:
        out.update(recs=recs[:n.value].copy(), scores=scores[:n.value].copy(), best=best.value, stats=tuple(int(x) for x in stats))
    return out


def core_explore(explore, cell, state, cost=None, front=None, plan=None, oa=0, ob=0, cells=None, view=None, rgb=None, start=None):
    """the exploration layer of csrc/grid_explore_core.h on the host (svh_test_grid_explore) on STATE and COST planes [nz, nx] under the
    offsets (oa, ob), R from explore.range and `cell`.  A dict: with cells int32 [n, 2] (global) their GAIN as gains; with view, a
    global cell inside the window, its VIEW plane as mask and (with rgb, an image [nz, nx, 3] whose row 0 is ib = nz - 1) the overlay as
    image; with start, a global cell, the ranking: recs int32 [n, 5], scores int64 [n], best, stats (records, feasible).  Needs no
    device"""
    return _explore(_bind().svh_test_grid_explore, explore, cell, state, cost, front, plan, oa, ob, cells, view, rgb, start)


def device_explore(explore, cell, state, cost=None, front=None, plan=None, oa=0, ob=0, cells=None, view=None, rgb=None, start=None):
    """TEST ENTRY: the same through the device kernels on a caller's planes"""
    return _explore(_bind().svh_test_grid_explore_device, explore, cell, state, cost, front, plan, oa, ob, cells, view, rgb, start)


def default_align(**kw):
    p = AlignParams()
    _bind().svh_grid_align_params_default(C.byref(p))
    return p.copy(**kw)


def _align(entry, params, align, state, oa, ob, points, pivot, subs, pivot_sub):
    s = np.ascontiguousarray(state, np.uint8)
    nz, nx = s.shape
    q = params.copy(nx=nx, nz=nz)
    K, W = align.rot_n, align.trans_n
    field = np.zeros((nz, nx), np.uint8)
    volume = np.full((2 * K + 1, 2 * W + 1, 2 * W + 1), -1, np.int32)
    rec, counts = np.zeros(ALIGN_RECORD, np.int32), np.zeros(2, np.int64)
    if pivot_sub is not None:
        u = np.ascontiguousarray(subs, np.int32).reshape(-1, 2)
        ps = np.ascontiguousarray(pivot_sub, np.int32).reshape(2)
        cap = len(u)
        frame = (None, 0, u.ctypes.data if len(u) else None, len(u), None, ps.ctypes.data)
    else:
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        cap = len(pts)
        frame = (pts.ctypes.data if len(pts) else None, len(pts), None, 0, _xyz(pivot).ctypes.data, None)
    scan = np.zeros((max(cap, 1), 2), np.int32)
    _check(entry(C.byref(q), C.byref(align), oa, ob, s.ctypes.data, *frame, field.ctypes.data, scan.ctypes.data if cap else None, cap,
                 counts.ctypes.data, volume.ctypes.data, rec.ctypes.data))
    return dict(field=field, scan=scan[:int(counts[0])].copy(), n_points=int(counts[1]), volume=None if rec[0] == ALIGN_FEW else volume, rec=rec)


def core_align(params, align, state, oa=0, ob=0, points=None, pivot=None, subs=None, pivot_sub=None):
    """the alignment layer of csrc/grid_align_core.h on the host (svh_test_grid_align) on a STATE plane [nz, nx] under the offsets
    (oa, ob) with the frame, cell, step and clearance of `params`: either points float32 [n, 4] about the map-frame position `pivot`, or
    global subs int32 [n, 2] about the pivot's global sub `pivot_sub`.  A dict: field uint8 [nz, nx], scan int32 [n_scan, 2] ascending
    by (ub, ua), n_points, volume int32 [2 K + 1, 2 W + 1, 2 W + 1] (None when the status is ALIGN_FEW), rec int32 [8] in the order of
    ALIGN_FIELDS.  Needs no device"""
    return _align(_bind().svh_test_grid_align, params, align, state, oa, ob, points, pivot, subs, pivot_sub)


def device_align(params, align, state, oa=0, ob=0, points=None, pivot=None, subs=None, pivot_sub=None):
    """TEST ENTRY: the same through the device kernels on a caller's plane"""
    return _align(_bind().svh_test_grid_align_device, params, align, state, oa, ob, points, pivot, subs, pivot_sub)


def align_form(form=-1):
    """TEST ENTRY: the form of the alignment's score kernel becomes `form` (0 chunk, 1 plain, 2 tiled, plus 4 for the field in three launches instead of two; -1 only reads); what it was"""
    return int(_bind().svh_test_grid_align_form(form))


def default_dyn(**kw):
    p = DynParams()
    _bind().svh_grid_dyn_params_default(C.byref(p))
    return p.copy(**kw)


def core_dyn_margin_q(dyn):
    """the checks of svh_grid_set_dynamics on the host: margin_q, or SvhError"""
    q = C.c_int32(0)
    _check(_bind().svh_test_grid_dyn_params(C.byref(dyn), C.addressof(q)))
    return q.value


def core_dyn_rdiv64(p, n):
    """rdiv64 of csrc/grid_dyn_core.h on the host, elementwise: int64"""
    p, n = np.ascontiguousarray(p, np.int64).ravel(), np.ascontiguousarray(n, np.int64).ravel()
    out = np.zeros(len(p), np.int64)
    _check(_bind().svh_test_grid_dyn_height(len(p), p.ctypes.data, n.ctypes.data, out.ctypes.data, None, None, None, None, None))
    return out


def core_dyn_height(q_o, q_e, n, k):
    """line_height of csrc/grid_dyn_core.h on the host, elementwise: int32"""
    a = [np.ascontiguousarray(v, np.int32).ravel() for v in np.broadcast_arrays(q_o, q_e, n, k)]
    out = np.zeros(len(a[0]), np.int32)
    _check(_bind().svh_test_grid_dyn_height(len(out), None, None, None, *[v.ctypes.data for v in a], out.ctypes.data))
    return out


def core_dyn_through(params, dyn, count, kmin, kmax, q=None):
    """body_of and goes_through of csrc/grid_dyn_core.h on the host, per stored cell: (lo int32, hi int32, through uint8 or None)"""
    ins = [np.ascontiguousarray(count, np.int32).ravel(), np.ascontiguousarray(kmin, np.uint32).ravel(), np.ascontiguousarray(kmax, np.uint32).ravel()]
    n = len(ins[0])
    qq = None if q is None else np.ascontiguousarray(q, np.int32).ravel()
    lo, hi, thr = np.zeros(n, np.int32), np.zeros(n, np.int32), None if q is None else np.zeros(n, np.uint8)
    _check(_bind().svh_test_grid_dyn_through(C.byref(params), C.byref(dyn), n, *[a.ctypes.data for a in ins], None if q is None else qq.ctypes.data,
                                             lo.ctypes.data, hi.ctypes.data, None if q is None else thr.ctypes.data))
    return lo, hi, thr


_CELL_DTYPES = (np.int32, np.int32, np.uint32, np.uint32, np.int64, np.uint64)


def core_dyn_settle(params, dyn, stamp, cell, contra, last, frame, through):
    """settle of csrc/grid_dyn_core.h on the host, per cell: cell and frame are (count, overhead, kmin, kmax, hsum, vsum); returns
    (cell', contra', last', event uint8); the inputs are not changed"""
    cell = [np.array(a, t).ravel() for a, t in zip(cell, _CELL_DTYPES)]
    frame = [np.ascontiguousarray(a, t).ravel() for a, t in zip(frame, _CELL_DTYPES)]
    contra, last = np.array(contra, np.int32).ravel(), np.array(last, np.int32).ravel()
    through = np.ascontiguousarray(through, np.int32).ravel()
    n = len(contra)
    event = np.zeros(n, np.uint8)
    cp, fp = (C.c_void_p * 6)(*[a.ctypes.data for a in cell]), (C.c_void_p * 6)(*[a.ctypes.data for a in frame])
    _check(_bind().svh_test_grid_dyn_settle(C.byref(params), C.byref(dyn), stamp, n, C.addressof(cp), contra.ctypes.data, last.ctypes.data, C.addressof(fp),
                                            through.ctypes.data, event.ctypes.data))
    return cell, contra, last, event


def core_dyn_colour(params, cls, intensity, pass_, contra, event):
    """colour_dyn of csrc/grid_dyn_core.h on the host: rgb uint8 [n, 3]"""
    ins = [np.ascontiguousarray(cls, np.uint8).ravel(), np.ascontiguousarray(intensity, np.uint8).ravel(), np.ascontiguousarray(pass_, np.int32).ravel(),
           np.ascontiguousarray(contra, np.int32).ravel(), np.ascontiguousarray(event, np.uint8).ravel()]
    n = len(ins[0])
    rgb = np.zeros((n, 3), np.uint8)
    _check(_bind().svh_test_grid_dyn_colour(C.byref(params), n, *[a.ctypes.data for a in ins], rgb.ctypes.data, 0, None, None))
    return rgb


def core_dyn_age(params, stamp, last):
    """age_of of csrc/grid_dyn_core.h on the host: int32"""
    last = np.ascontiguousarray(last, np.int32).ravel()
    age = np.zeros(len(last), np.int32)
    _check(_bind().svh_test_grid_dyn_colour(C.byref(params), len(last), None, None, None, None, None, None, stamp, last.ctypes.data, age.ctypes.data))
    return age


def default_archive(**kw):
    p = ArchiveParams()
    _bind().svh_grid_archive_params_default(C.byref(p))
    return p.copy(**kw)


def core_archive_key(ga, gb, max_tiles=0):
    """cell_key, the tile read back from it and tile_index of csrc/grid_archive_core.h on the host, per global cell: (key uint64,
    tile int32 [n, 2] as (ta, tb), index uint32, archive_table_size(max_tiles))"""
    ga, gb = np.ascontiguousarray(ga, np.int32).ravel(), np.ascontiguousarray(gb, np.int32).ravel()
    n = len(ga)
    key, tile, index, table = np.zeros(n, np.uint64), np.zeros((n, 2), np.int32), np.zeros(n, np.uint32), C.c_uint32(0)
    _check(_bind().svh_test_grid_archive_key(n, ga.ctypes.data, gb.ctypes.data, key.ctypes.data, tile.ctypes.data, index.ctypes.data, max_tiles,
                                             C.addressof(table)))
    return key, tile, index, table.value


def core_archive_strip(nx, nz, da, db):
    """strip_cell of csrc/grid_archive_core.h on the host for every lane: int32 [n, 2] window cells (ia, ib) in lane order.  A scroll by
    (da, db) leaves the strip of (da, db) in the old window and enters the strip of (-da, -db) in the new one"""
    n = C.c_int64(0)
    L = _bind()
    _check(L.svh_test_grid_archive_strip(nx, nz, da, db, None, 0, C.addressof(n)))
    cells = np.zeros((n.value, 2), np.int32)
    _check(L.svh_test_grid_archive_strip(nx, nz, da, db, cells.ctypes.data, n.value, C.addressof(n)))
    return cells


def __getattr__(name):
    if name == "PLAN_TILE":
        return plan_tile()
    if name == "FRONT_TILE":
        return front_tile()
    raise AttributeError(name)


def _xyz(p):
    return np.ascontiguousarray(p, np.float64).reshape(3)


class Grid:
    """g = Grid(params); g.add_view(view) or g.add_points(xyzv); g.plane(CLASS); img = g.render(RENDER_CLASS)"""

    def __init__(self, params=None, **kw):
        self._L = _bind()
        self.params = (params if params is not None else default_params()).copy(**kw)
        self._h = self._L.svh_grid_create(C.byref(self.params))
        if not self._h:
            raise SvhError(ERR_BAD_ARG, last_error())
        self.nx, self.nz = self.params.nx, self.params.nz

    def clear(self):
        _check(self._L.svh_grid_clear(self._h))

    def set_window(self, x0, z0):
        _check(self._L.svh_grid_set_window(self._h, x0, z0))   # the offsets are zero again
        self.params.x0, self.params.z0 = x0, z0

    def add_points(self, xyzv):
        """[n, 4] float32 (x, y, z, val) on the host"""
        p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
        _check(self._L.svh_grid_add_points(self._h, p.ctypes.data if len(p) else None, len(p), 0))

    def add_points_device(self, ptr, n):
        """the same from a raw device address (int), 16-byte aligned"""
        _check(self._L.svh_grid_add_points(self._h, ptr, n, 1))

    def add_view(self, view):
        """the whole store of a svhip.view.View, device to device"""
        _check(self._L.svh_grid_add_view(self._h, view._h))

    def scroll(self, da, db):
        """the window moves by whole cells and keeps what stays inside"""
        _check(self._L.svh_grid_scroll(self._h, da, db))

    def follow(self, xyz, ia, ib):
        """scrolls so that the cell of the map-frame position xyz becomes window cell (ia, ib)"""
        _check(self._L.svh_grid_follow(self._h, _xyz(xyz).ctypes.data, ia, ib))

    def window(self):
        """the offsets (oa, ob) in cells"""
        off = np.zeros(2, np.int32)
        _check(self._L.svh_grid_get_window(self._h, off.ctypes.data))
        return int(off[0]), int(off[1])

    def cell_of(self, xyz):
        """the global cell (ga, gb) of a map-frame position"""
        cell = np.zeros(2, np.int32)
        _check(self._L.svh_grid_cell_of(self._h, _xyz(xyz).ctypes.data, cell.ctypes.data))
        return int(cell[0]), int(cell[1])

    def add_points_from(self, xyzv, origin):
        """add_points, and one ray per low point from the cell of the map-frame position `origin`"""
        p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
        _check(self._L.svh_grid_add_points_from(self._h, p.ctypes.data if len(p) else None, len(p), 0, _xyz(origin).ctypes.data))

    def add_points_device_from(self, ptr, n, origin):
        """the same from a raw device address (int), 16-byte aligned"""
        _check(self._L.svh_grid_add_points_from(self._h, ptr, n, 1, _xyz(origin).ctypes.data))

    def add_view_lists_from(self, view, first_list, n_lists, origin):
        """lists first_list .. first_list + n_lists - 1 of a svhip.view.View, device to device, with rays from `origin`"""
        _check(self._L.svh_grid_add_view_lists_from(self._h, view._h, first_list, n_lists, _xyz(origin).ctypes.data))

    def ray_stats(self):
        """(rays, ray_cells) since the last clear"""
        out = np.zeros(2, np.int64)
        _check(self._L.svh_grid_get_ray_stats(self._h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def local_plane(self, which, device_ptr=None):
        """LOCAL_PASS int32 or LOCAL_STATE uint8, [nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_local(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(LOCAL_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((self.nz, self.nx), LOCAL_DTYPE[which])
        _check(self._L.svh_grid_get_local(self._h, which, out.ctypes.data, 0))
        return out

    def render_local(self, device_ptr=None):
        """render(RENDER_CLASS) with the cells that are unknown and seen in SEEN_COLOUR"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_local(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_local(self._h, img.ctypes.data, 0))
        return img

    def set_traversability(self, params=None, **kw):
        """the parameters in force (or `params`) with the fields of kw replaced: max_slope, inscribed, inflate, lethal"""
        t = (params if params is not None else self.traversability()[0]).copy(**kw)
        _check(self._L.svh_grid_set_traversability(self._h, C.byref(t)))

    def traversability(self):
        """(TravParams in force, their reach in cells; 0 while the defaults do not fit the grid's cell)"""
        t, reach = TravParams(), C.c_int32(0)
        _check(self._L.svh_grid_get_traversability(self._h, C.byref(t), C.addressof(reach)))
        return t, reach.value

    def trav_plane(self, which, device_ptr=None):
        """TRAV_FLAGS uint8, TRAV_DIST2 int32 or TRAV_COST uint8, [nz, nx]; with device_ptr it is written there and None
        returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_trav(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(TRAV_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((self.nz, self.nx), TRAV_DTYPE[which])
        _check(self._L.svh_grid_get_trav(self._h, which, out.ctypes.data, 0))
        return out

    def render_cost(self, device_ptr=None):
        """the cost map, [nz, nx, 3] uint8, row 0 the farthest; with device_ptr the image is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_cost(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_cost(self._h, img.ctypes.data, 0))
        return img

    def set_plan(self, params=None, **kw):
        """the plan parameters in force (or `params`) with the fields of kw replaced: neutral, unknown, max_cost"""
        p = (params if params is not None else self.plan_params()).copy(**kw)
        _check(self._L.svh_grid_set_plan(self._h, C.byref(p)))

    def plan_params(self):
        p = PlanParams()
        _check(self._L.svh_grid_get_plan(self._h, C.byref(p)))
        return p

    def set_goals(self, cells):
        """[n, 2] global cells (ga, gb); an empty list forgets the goals"""
        c, ptr = _cells(cells)
        _check(self._L.svh_grid_plan_set_goals(self._h, ptr, len(c)))

    def set_goal(self, xyz):
        """one goal, the cell of a map-frame position"""
        _check(self._L.svh_grid_plan_set_goal(self._h, _xyz(xyz).ctypes.data))

    def plan_plane(self, which, device_ptr=None):
        """PLAN_POT int32 or PLAN_DIR uint8, [nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_plan_plane(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(PLAN_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((self.nz, self.nx), PLAN_DTYPE[which])
        _check(self._L.svh_grid_get_plan_plane(self._h, which, out.ctypes.data, 0))
        return out

    def plan_stats(self):
        """(goals given, goals that count, cells with POT != FAR, relaxation rounds)"""
        out = np.zeros(4, np.int64)
        _check(self._L.svh_grid_get_plan_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def path(self, start_xyz, cap=None):
        """(status, cells [n, 2] int32 global, cost): the shortest path from the cell of a map-frame position; with cap only
        its first cells, and n is still the length of the whole path in `path_len`"""
        room = self.nx * self.nz if cap is None else int(cap)
        cells = np.zeros((max(room, 1), 2), np.int32)
        n, cost = C.c_int64(-1), C.c_int32(-1)
        status = _check(self._L.svh_grid_plan_path(self._h, _xyz(start_xyz).ctypes.data, cells.ctypes.data if room else None, room,
                                                   C.addressof(n), C.addressof(cost)))
        self.path_len = n.value
        return status, cells[:min(n.value, room)].copy(), cost.value

    def render_plan(self, cells=(), device_ptr=None):
        """render_cost with the goals that count in GOAL_COLOUR and the given global cells in PATH_COLOUR over them"""
        c, ptr = _cells(cells)
        if device_ptr is not None:
            _check(self._L.svh_grid_render_plan(self._h, ptr, len(c), device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_plan(self._h, ptr, len(c), img.ctypes.data, 0))
        return img

    def set_frontier(self, params=None, **kw):
        """the frontier parameters in force (or `params`) with the fields of kw replaced: max_cell_cost, min_size, unexplored,
        border"""
        p = (params if params is not None else self.frontier_params()).copy(**kw)
        _check(self._L.svh_grid_set_frontier(self._h, C.byref(p)))

    def frontier_params(self):
        p = FrontParams()
        _check(self._L.svh_grid_get_frontier(self._h, C.byref(p)))
        return p

    def front_plane(self, which, device_ptr=None):
        """FRONT_FLAGS uint8 or FRONT_LABEL int32, [nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_front_plane(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(FRONT_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((self.nz, self.nx), FRONT_DTYPE[which])
        _check(self._L.svh_grid_get_front_plane(self._h, which, out.ctypes.data, 0))
        return out

    def frontiers(self, cap=None):
        """the records of the kept components, int32 [n, 10] in the order of FRONT_FIELDS, ascending by label; with cap only
        the first, and the count of all is in `frontier_count`"""
        n = C.c_int64(-1)
        if cap is None:
            _check(self._L.svh_grid_get_frontiers(self._h, None, 0, C.addressof(n)))
            cap = n.value
        recs = np.zeros((max(int(cap), 1), FRONT_RECORD), np.int32)
        _check(self._L.svh_grid_get_frontiers(self._h, recs.ctypes.data if cap else None, int(cap), C.addressof(n)))
        self.frontier_count = n.value
        return recs[:min(n.value, int(cap))].copy()

    def frontier_stats(self):
        """(frontier cells, components, kept components, cells in kept components, kernel launches of the last computation)"""
        out = np.zeros(5, np.int64)
        _check(self._L.svh_grid_get_frontier_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def set_goals_frontiers(self):
        """the representatives of the kept components become the planner's goals; returns how many"""
        return _check(self._L.svh_grid_plan_set_goals_frontiers(self._h))

    def render_frontiers(self, device_ptr=None):
        """render_cost with the frontier cells over it: kept, dropped, representatives"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_frontiers(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_frontiers(self._h, img.ctypes.data, 0))
        return img

    def set_objects(self, params=None, **kw):
        """the object parameters in force (or `params`) with the fields of kw replaced; the tracks are emptied"""
        p = (params if params is not None else self.objects_params()).copy(**kw)
        _check(self._L.svh_grid_set_objects(self._h, C.byref(p)))

    def objects_params(self):
        p = ObjParams()
        _check(self._L.svh_grid_get_objects_params(self._h, C.byref(p)))
        return p

    def obj_plane(self, which, device_ptr=None):
        """OBJ_FLAGS uint8 or OBJ_LABEL int32, [nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_obj_plane(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(OBJ_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((self.nz, self.nx), OBJ_DTYPE[which])
        _check(self._L.svh_grid_get_obj_plane(self._h, which, out.ctypes.data, 0))
        return out

    def objects(self, cap=None):
        """the records of the kept components, int32 [n, 10] in the order of OBJ_FIELDS, ascending by label; with cap only the first,
        and the count of all is in `object_count`"""
        n = C.c_int64(0)
        if cap is None:
            _check(self._L.svh_grid_get_objects(self._h, None, 0, C.addressof(n)))
            cap = n.value
        recs = np.zeros((max(int(cap), 1), OBJ_RECORD), np.int32)
        _check(self._L.svh_grid_get_objects(self._h, recs.ctypes.data if cap else None, int(cap), C.addressof(n)))
        self.object_count = n.value
        return recs[:min(n.value, int(cap))].copy()

    def object_stats(self):
        """(object cells, components, kept, cells in kept components, too large, too low, kernel launches of the computation)"""
        out = np.zeros(7, np.int64)
        _check(self._L.svh_grid_get_object_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def objects_step(self, cap=None):
        """one step of the tracks: assign int32 [n], per kept object by rank the id of its track or ASSIGN_UNTRACKED; with cap only the
        first, and the count of all is in `object_count`"""
        n = C.c_int64(0)
        if cap is None:
            cap = self.object_stats()[2]
        assign = np.zeros(max(int(cap), 1), np.int32)
        _check(self._L.svh_grid_objects_step(self._h, assign.ctypes.data if cap else None, int(cap), C.addressof(n)))
        self.object_count = n.value
        return assign[:min(n.value, int(cap))].copy()

    def objects_reset(self):
        _check(self._L.svh_grid_objects_reset(self._h))

    def tracks(self, cap=None):
        """the track records, int32 [n, 14] in the order of TRACK_FIELDS, ascending by id"""
        n = C.c_int64(0)
        if cap is None:
            _check(self._L.svh_grid_get_tracks(self._h, None, 0, C.addressof(n)))
            cap = n.value
        recs = np.zeros((max(int(cap), 1), TRACK_RECORD), np.int32)
        _check(self._L.svh_grid_get_tracks(self._h, recs.ctypes.data if cap else None, int(cap), C.addressof(n)))
        self.track_count = n.value
        return recs[:min(n.value, int(cap))].copy()

    def track_plane(self, device_ptr=None):
        """(the ID plane of the last step int32 [nz, nx], the offsets (oa, ob) it was written under); with device_ptr the plane is
        written there and (None, offsets) returned"""
        off = np.zeros(2, np.int32)
        if device_ptr is not None:
            _check(self._L.svh_grid_get_track_plane(self._h, device_ptr, 1, off.ctypes.data))
            return None, (int(off[0]), int(off[1]))
        out = np.zeros((self.nz, self.nx), np.int32)
        _check(self._L.svh_grid_get_track_plane(self._h, out.ctypes.data, 0, off.ctypes.data))
        return out, (int(off[0]), int(off[1]))

    def track_stats(self):
        """TRACK_STATS: steps, tracks; of the last step: by overlap, by gate, new, missed, dropped, untracked"""
        out = np.zeros(8, np.int64)
        _check(self._L.svh_grid_get_track_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def render_objects(self, device_ptr=None):
        """render(RENDER_CLASS) with the objects over it, coloured by track"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_objects(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_objects(self._h, img.ctypes.data, 0))
        return img

    def set_predict(self, params=None, **kw):
        """the prediction parameters in force (or `params`) with the fields of kw replaced: slots, stride, poses_per_step, margin,
        grow16, only_moving"""
        p = (params if params is not None else self.get_predict()).copy(**kw)
        _check(self._L.svh_grid_set_predict(self._h, C.byref(p)))

    def get_predict(self):
        p = PredParams()
        _check(self._L.svh_grid_get_predict(self._h, C.byref(p)))
        return p

    def pred_plane(self, device_ptr=None):
        """(PRED uint32 [nz, nx], the offsets (oa, ob) of the ID frame it lies under); with device_ptr the plane is written there and
        (None, offsets) returned"""
        off = np.zeros(2, np.int32)
        if device_ptr is not None:
            _check(self._L.svh_grid_get_pred_plane(self._h, device_ptr, 1, off.ctypes.data))
            return None, (int(off[0]), int(off[1]))
        out = np.zeros((self.nz, self.nx), np.uint32)
        _check(self._L.svh_grid_get_pred_plane(self._h, out.ctypes.data, 0, off.ctypes.data))
        return out, (int(off[0]), int(off[1]))

    def pred_stats(self):
        """PRED_STATS: predicting tracks, source cells, PRED cells with a bit set, launches of the computation"""
        out = np.zeros(4, np.int64)
        _check(self._L.svh_grid_get_pred_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def footprint_pred(self, poses=None, device_ptrs=None, n=None):
        """the slot masks uint32 [n] of poses int32 [n, 3] (ga, gb, k); with device_ptrs = (poses, out) and n both lie on the device
        and None is returned"""
        if device_ptrs is not None:
            _check(self._L.svh_grid_footprint_pred(self._h, device_ptrs[0], n, 1, device_ptrs[1]))
            return None
        q = np.ascontiguousarray(poses, np.int32).reshape(-1, 3)
        out = np.zeros(len(q), np.uint32)
        _check(self._L.svh_grid_footprint_pred(self._h, q.ctypes.data if len(q) else None, len(q), 0, out.ctypes.data if len(q) else None))
        return out

    def roll_score_pred(self, anchor_xyz, set_=0, device_ptrs=None, want=(True, True)):
        """(best, recs int32 [K, 6] in the order of ROLL_PRED_FIELDS, scores int64 [K]) of set `set_` anchored at the cell of a map-frame
        position, cut by the prediction too; want = (recs, scores): False passes NULL and returns None in its place; with device_ptrs =
        (recs, scores), either may be None, they are written there and only best is returned"""
        best = C.c_int32(-9)
        if device_ptrs is not None:
            _check(self._L.svh_grid_roll_score_pred(self._h, _xyz(anchor_xyz).ctypes.data, set_, device_ptrs[0], device_ptrs[1], 1, C.addressof(best)))
            return best.value
        K = self.candidates()[1]
        recs, scores = np.zeros((max(K, 1), ROLL_PRED_RECORD), np.int32), np.zeros(max(K, 1), np.int64)
        _check(self._L.svh_grid_roll_score_pred(self._h, _xyz(anchor_xyz).ctypes.data, set_, recs.ctypes.data if want[0] else None,
                                                scores.ctypes.data if want[1] else None, 0, C.addressof(best)))
        return best.value, (recs[:K] if want[0] else None), (scores[:K] if want[1] else None)

    def render_pred(self, mode=RENDER_CLASS, device_ptr=None):
        """render(mode) with the window cells that PRED covers over it, coloured by their lowest slot"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_pred(self._h, mode, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_pred(self._h, mode, img.ctypes.data, 0))
        return img

    def set_roll(self, params=None, **kw):
        """the rollout parameters in force (or `params`) with the fields of kw replaced: front, rear, half_width, headings_m, stop_cost,
        unknown_cost, w_pot, w_cost, w_cut"""
        p = (params if params is not None else self.roll_params()[0]).copy(**kw)
        _check(self._L.svh_grid_set_roll(self._h, C.byref(p)))

    def roll_params(self):
        """(RollParams in force, their reach R in cells -- 0 while the defaults do not fit the grid's cell --, the cells of all lists)"""
        p, R, total = RollParams(), C.c_int32(-1), C.c_int64(-1)
        _check(self._L.svh_grid_get_roll(self._h, C.byref(p), C.addressof(R), C.addressof(total)))
        return p, R.value, total.value

    def heading_of(self, dir_xyz):
        """the heading of a map-frame direction"""
        k = C.c_int32(-1)
        _check(self._L.svh_grid_heading_of(self._h, _xyz(dir_xyz).ctypes.data, C.addressof(k)))
        return k.value

    def roll_footprint(self, k):
        """int32 [n, 2]: the cell offsets (da, db) under the vehicle at heading k, ascending by (db, da)"""
        n = C.c_int64(-1)
        _check(self._L.svh_grid_roll_footprint(self._h, k, None, 0, C.addressof(n)))
        offs = np.zeros((max(n.value, 1), 2), np.int32)
        _check(self._L.svh_grid_roll_footprint(self._h, k, offs.ctypes.data, n.value, C.addressof(n)))
        return offs[:n.value].copy()

    def footprint_cost(self, poses=None, device_ptrs=None, n=None):
        """F int32 [n] of poses int32 [n, 3] (ga, gb, k); with device_ptrs = (poses, out) and n both lie on the device and None is
        returned"""
        if device_ptrs is not None:
            _check(self._L.svh_grid_footprint_cost(self._h, device_ptrs[0], n, 1, device_ptrs[1]))
            return None
        q = np.ascontiguousarray(poses, np.int32).reshape(-1, 3)
        out = np.zeros(len(q), np.int32)
        _check(self._L.svh_grid_footprint_cost(self._h, q.ctypes.data if len(q) else None, len(q), 0, out.ctypes.data if len(q) else None))
        return out

    def set_candidates(self, table):
        """int32 [S, K, T, 3]: S sets of K candidates of T poses (dga, dgb, k); k = -1 ends a candidate"""
        t = np.ascontiguousarray(table, np.int32)
        if t.ndim != 4 or t.shape[3] != 3:
            raise SvhError(ERR_BAD_ARG, "a table [S, K, T, 3] is needed")
        _check(self._L.svh_grid_roll_set_candidates(self._h, t.ctypes.data, t.shape[0], t.shape[1], t.shape[2]))

    def candidates(self):
        """(S, K, T) of the candidate table in force, (0, 0, 0) while there is none"""
        skt = np.zeros(3, np.int32)
        _check(self._L.svh_grid_roll_get_candidates(self._h, skt.ctypes.data))
        return tuple(int(v) for v in skt)

    def roll_score(self, anchor_xyz, set_=0, device_ptrs=None):
        """(best, recs int32 [K, 5] in the order of ROLL_FIELDS, scores int64 [K]) of set `set_` anchored at the cell of a map-frame
        position; with device_ptrs = (recs, scores), either may be None, they are written there and only best is returned"""
        best = C.c_int32(-9)
        if device_ptrs is not None:
            _check(self._L.svh_grid_roll_score(self._h, _xyz(anchor_xyz).ctypes.data, set_, device_ptrs[0], device_ptrs[1], 1, C.addressof(best)))
            return best.value
        K = self.candidates()[1]                           # asked of the library: a table whose upload failed is in force all the same
        recs, scores = np.zeros((max(K, 1), ROLL_RECORD), np.int32), np.zeros(max(K, 1), np.int64)
        _check(self._L.svh_grid_roll_score(self._h, _xyz(anchor_xyz).ctypes.data, set_, recs.ctypes.data, scores.ctypes.data, 0, C.addressof(best)))
        return best.value, recs[:K], scores[:K]

    def render_roll(self, device_ptr=None):
        """render_cost with the poses before the cut of every candidate of the last roll_score in ROLL_COLOUR, the best's in
        ROLL_BEST_COLOUR over them"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_roll(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_roll(self._h, img.ctypes.data, 0))
        return img

    def set_pose(self, params=None, **kw):
        """the pose planner's parameters in force (or `params`) with the fields of kw replaced: neutral, max_cost, turn, reverse, spin"""
        p = (params if params is not None else self.pose_params()).copy(**kw)
        _check(self._L.svh_grid_set_pose(self._h, C.byref(p)))

    def pose_params(self):
        p = PoseParams()
        _check(self._L.svh_grid_get_pose(self._h, C.byref(p)))
        return p

    def pose_set_goals(self, triples):
        """[n, 3] goal states (ga, gb, d), global cells; d = -1: every passable heading; an empty list forgets the goals"""
        t, ptr = _triples(triples)
        _check(self._L.svh_grid_pose_set_goals(self._h, ptr, len(t)))

    def pose_set_goal(self, xyz, d=-1):
        """one goal, the cell of a map-frame position at heading d"""
        _check(self._L.svh_grid_pose_set_goal(self._h, _xyz(xyz).ctypes.data, d))

    def pose_plane(self, which, device_ptr=None):
        """POSE_CF uint8, POSE_POT int32 or POSE_DIR uint8, [8, nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_pose_plane(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(POSE_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((POSE_HEADINGS, self.nz, self.nx), POSE_DTYPE[which])
        _check(self._L.svh_grid_get_pose_plane(self._h, which, out.ctypes.data, 0))
        return out

    def pose_stats(self):
        """(goals given, goal states that count, states with PPOT != FAR, relaxation rounds)"""
        out = np.zeros(4, np.int64)
        _check(self._L.svh_grid_get_pose_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def pose_heading_of(self, dir_xyz):
        """the planning heading 0..7 nearest to a map-frame direction"""
        d = C.c_int32(-1)
        _check(self._L.svh_grid_pose_heading_of(self._h, _xyz(dir_xyz).ctypes.data, C.addressof(d)))
        return d.value

    def pose_path(self, start_xyz, d, cap=None):
        """(status, poses [n, 3] int32 (ga, gb, k = d headings_m), cost): the cheapest pose sequence from the cell of a map-frame
        position at heading d; with cap only its first poses, and the length of the whole path is in `pose_path_len`"""
        room = POSE_HEADINGS * self.nx * self.nz if cap is None else int(cap)
        poses = np.zeros((max(room, 1), 3), np.int32)
        n, cost = C.c_int64(-1), C.c_int32(-1)
        status = _check(self._L.svh_grid_pose_path(self._h, _xyz(start_xyz).ctypes.data, d, poses.ctypes.data if room else None, room,
                                                   C.addressof(n), C.addressof(cost)))
        self.pose_path_len = n.value
        return status, poses[:min(n.value, room)].copy(), cost.value

    def render_pose(self, poses=(), device_ptr=None):
        """render_cost with the cells of the goals that count in GOAL_COLOUR and the reference cells of the given poses in
        PATH_COLOUR over them"""
        t, ptr = _triples(poses)
        if device_ptr is not None:
            _check(self._L.svh_grid_render_pose(self._h, ptr, len(t), device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_pose(self._h, ptr, len(t), img.ctypes.data, 0))
        return img

    def set_time(self, params=None, **kw):
        """switches the time layer on with the parameters in force (or `params`) and the fields of kw replaced: layers, wait, release"""
        p = (params if params is not None else self.time_params()).copy(**kw)
        _check(self._L.svh_grid_set_time(self._h, C.byref(p)))

    def time_params(self):
        p = TimeParams()
        _check(self._L.svh_grid_get_time(self._h, C.byref(p)))
        return p

    def time_plane(self, which, t0=0, count=None, device_ptr=None):
        """TIME_TPOT int32 or TIME_TDIR uint8, [count, nz, nx] from layer t0 (count None: all that follow); TIME_RCOST uint8 or TIME_RPOT
        int32, [nz, nx]; with device_ptr it is written there and None returned"""
        if not 0 <= which < len(TIME_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        static = which in (TIME_RCOST, TIME_RPOT)
        n = (1 if static else self.time_params().layers - t0) if count is None else int(count)
        if device_ptr is not None:
            _check(self._L.svh_grid_get_time_plane(self._h, which, t0, n, device_ptr, 1))
            return None
        out = np.zeros((max(n, 1), self.nz, self.nx), TIME_DTYPE[which])
        _check(self._L.svh_grid_get_time_plane(self._h, which, t0, n, out.ctypes.data, 0))
        return out[0] if static else out

    def time_stats(self):
        """(layers, states with TPOT != FAR, passable states with BLOCK, states whose TDIR is wait, released cells, rounds of RPOT)"""
        out = np.zeros(6, np.int64)
        _check(self._L.svh_grid_get_time_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def time_path(self, start_xyz, cap=None):
        """(status, triples [n, 3] int32 (ga, gb, t), cost): the cheapest sequence from the cell of a map-frame position at layer 0; a
        wait repeats the cell.  With cap only its first entries, and the length of the whole path is in `time_path_len`"""
        room = self.time_params().layers + self.nx * self.nz if cap is None else int(cap)
        triples = np.zeros((max(room, 1), 3), np.int32)
        n, cost = C.c_int64(-1), C.c_int32(-1)
        status = _check(self._L.svh_grid_time_path(self._h, _xyz(start_xyz).ctypes.data, triples.ctypes.data if room else None, room,
                                                   C.addressof(n), C.addressof(cost)))
        self.time_path_len = n.value
        return status, triples[:min(n.value, room)].copy(), cost.value

    def render_time(self, t=0, triples=(), device_ptr=None):
        """the image of RCOST with the cells blocked at layer t in the prediction's colour of its slot, the goals that count in
        GOAL_COLOUR and the cells of the given triples in PATH_COLOUR over it"""
        q, ptr = _triples(triples)
        if device_ptr is not None:
            _check(self._L.svh_grid_render_time(self._h, t, ptr, len(q), device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_time(self._h, t, ptr, len(q), img.ctypes.data, 0))
        return img

    def set_explore(self, params=None, **kw):
        """the exploration parameters in force (or `params`) with the fields of kw replaced: range, min_gain, w_gain, w_reach"""
        p = (params if params is not None else self.explore_params()[0]).copy(**kw)
        _check(self._L.svh_grid_set_explore(self._h, C.byref(p)))

    def explore_params(self):
        """(ExploreParams in force, their range R in cells; 0 while the defaults do not fit the grid's cell)"""
        p, R = ExploreParams(), C.c_int32(-1)
        _check(self._L.svh_grid_get_explore(self._h, C.byref(p), C.addressof(R)))
        return p, R.value

    def view_gain(self, cells=None, device_ptrs=None, n=None):
        """GAIN int32 [n] of viewpoints int32 [n, 2], global cells (-1: outside the window); with device_ptrs = (cells, out) and n both
        lie on the device and None is returned"""
        if device_ptrs is not None:
            _check(self._L.svh_grid_view_gain(self._h, device_ptrs[0], n, 1, device_ptrs[1]))
            return None
        q = np.ascontiguousarray(cells, np.int32).reshape(-1, 2)
        out = np.zeros(len(q), np.int32)
        _check(self._L.svh_grid_view_gain(self._h, q.ctypes.data if len(q) else None, len(q), 0, out.ctypes.data if len(q) else None))
        return out

    def view_mask(self, ga, gb, device_ptr=None):
        """the VIEW plane uint8 [nz, nx] of the viewpoint (ga, gb), a global cell inside the window: VIEW_NONE, VIEW_VISITED,
        VIEW_COUNTED; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_view_mask(self._h, ga, gb, device_ptr, 1))
            return None
        out = np.zeros((self.nz, self.nx), np.uint8)
        _check(self._L.svh_grid_view_mask(self._h, ga, gb, out.ctypes.data, 0))
        return out

    def explore_rank(self, start_xyz, cap=None):
        """(best, recs int32 [n, 5] in the order of EXPLORE_FIELDS, scores int64 [n]) of the kept frontier components ranked from the
        cell of a map-frame position; with cap only the first, and the count of all is in `explore_count`"""
        n, best = C.c_int64(-1), C.c_int32(-9)
        room = 65536 if cap is None else int(cap)
        recs, scores = np.zeros((max(room, 1), EXPLORE_RECORD), np.int32), np.zeros(max(room, 1), np.int64)
        _check(self._L.svh_grid_explore_rank(self._h, _xyz(start_xyz).ctypes.data, recs.ctypes.data if room else None,
                                             scores.ctypes.data if room else None, room, C.addressof(n), C.addressof(best)))
        self.explore_count = n.value
        m = min(n.value, room)
        return best.value, recs[:m].copy(), scores[:m].copy()

    def set_goal_explore(self, start_xyz):
        """ranks from the cell of a map-frame position and makes the best record's representative the planner's only goal: 1, or 0
        when there is no best (the goals are then left alone)"""
        return _check(self._L.svh_grid_plan_set_goal_explore(self._h, _xyz(start_xyz).ctypes.data))

    def explore_stats(self):
        """(records of the last ranking, feasible records, reach fields computed since create, launches of the last gain computation)"""
        out = np.zeros(4, np.int64)
        _check(self._L.svh_grid_get_explore_stats(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def render_view(self, ga, gb, device_ptr=None):
        """render_frontiers with the VIEW plane of the viewpoint (ga, gb) over it: counted cells in VIEW_COLOUR, visited cells
        brightened, the viewpoint in VIEWPOINT_COLOUR"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_view(self._h, ga, gb, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_view(self._h, ga, gb, img.ctypes.data, 0))
        return img

    def set_align(self, params=None, **kw):
        """the align parameters `params` (or the defaults) with the fields of kw replaced: reach, range, rot_den, rot_n, trans_n,
        min_scan.  A grid has none until this succeeds"""
        p = (params if params is not None else default_align()).copy(**kw)
        _check(self._L.svh_grid_set_align(self._h, C.byref(p)))
        self.align_params = p

    def align_field(self, device_ptr=None):
        """the field F uint8 [nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_align_field(self._h, device_ptr, 1))
            return None
        out = np.zeros((self.nz, self.nx), np.uint8)
        _check(self._L.svh_grid_get_align_field(self._h, out.ctypes.data, 0))
        return out

    def align_points(self, xyzv, pivot):
        """aligns [n, 4] float32 points on the host about the map-frame position `pivot`: the record int32 [8] in the order of
        ALIGN_FIELDS.  Nothing is added"""
        p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
        rec = np.zeros(ALIGN_RECORD, np.int32)
        _check(self._L.svh_grid_align_points(self._h, p.ctypes.data if len(p) else None, len(p), 0, _xyz(pivot).ctypes.data, rec.ctypes.data))
        return rec

    def align_points_device(self, ptr, n, pivot):
        """the same from a raw device address (int), 16-byte aligned"""
        rec = np.zeros(ALIGN_RECORD, np.int32)
        _check(self._L.svh_grid_align_points(self._h, ptr, n, 1, _xyz(pivot).ctypes.data, rec.ctypes.data))
        return rec

    def align_view_lists(self, view, first_list, n_lists, pivot):
        """the same for lists first_list .. first_list + n_lists - 1 of a svhip.view.View, read where they lie"""
        rec = np.zeros(ALIGN_RECORD, np.int32)
        _check(self._L.svh_grid_align_view_lists(self._h, view._h, first_list, n_lists, _xyz(pivot).ctypes.data, rec.ctypes.data))
        return rec

    def align_volume(self, device_ptr=None):
        """the scores of the last alignment, int32 [2 K + 1, 2 W + 1, 2 W + 1] indexed [k + K, tb + W, ta + W]"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_align_volume(self._h, device_ptr, 1))
            return None
        K, W = self.align_params.rot_n, self.align_params.trans_n
        out = np.zeros((2 * K + 1, 2 * W + 1, 2 * W + 1), np.int32)
        _check(self._L.svh_grid_get_align_volume(self._h, out.ctypes.data, 0))
        return out

    def align_scan(self, cap=None):
        """the scan of the last alignment, int32 [n_scan, 2] global subs (ua, ub) ascending by (ub, ua); with cap only the first"""
        n = C.c_int64(-1)
        if cap is None:
            _check(self._L.svh_grid_get_align_scan(self._h, None, 0, C.addressof(n)))
            cap = n.value
        out = np.zeros((max(cap, 1), 2), np.int32)
        _check(self._L.svh_grid_get_align_scan(self._h, out.ctypes.data if cap else None, cap, C.addressof(n)))
        return out[:min(n.value, cap)].copy()

    def align_correction(self, k, ta, tb, pivot):
        """the map-frame transform M float64 [4, 4] of the candidate (k, ta, tb) about `pivot`.  Needs no device"""
        M = np.zeros((4, 4), np.float64)
        _check(self._L.svh_grid_align_correction(self._h, k, ta, tb, _xyz(pivot).ctypes.data, M.ctypes.data))
        return M

    def render_align(self, device_ptr=None):
        """render_local with the last alignment over it: the scan at the identity in ALIGN_SCAN_COLOUR, placed at the best in
        ALIGN_BEST_COLOUR, the pivot's cell in ALIGN_PIVOT_COLOUR"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_align(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_align(self._h, img.ctypes.data, 0))
        return img

    def set_dynamics(self, params=None, **kw):
        """the dynamics: the parameters in force, else the defaults (or `params`), with the fields of kw replaced: clear_frames,
        min_through, margin, max_age"""
        if params is None:
            try:
                params = self.dynamics()
            except SvhError:
                params = default_dyn()
        p = params.copy(**kw)
        _check(self._L.svh_grid_set_dynamics(self._h, C.byref(p)))
        return p

    def drop_dynamics(self):
        """the layer and its planes go"""
        _check(self._L.svh_grid_set_dynamics(self._h, None))

    def dynamics(self):
        p = DynParams()
        _check(self._L.svh_grid_get_dynamics(self._h, C.byref(p)))
        return p

    def observe_points(self, xyzv, origin):
        """one observation: [n, 4] float32 (x, y, z, val) on the host, seen from the map-frame position `origin`"""
        p = np.ascontiguousarray(xyzv, np.float32).reshape(-1, 4)
        _check(self._L.svh_grid_observe_points(self._h, p.ctypes.data if len(p) else None, len(p), 0, _xyz(origin).ctypes.data))

    def observe_points_device(self, ptr, n, origin):
        """the same from a raw device address (int), 16-byte aligned"""
        _check(self._L.svh_grid_observe_points(self._h, ptr, n, 1, _xyz(origin).ctypes.data))

    def observe_view_lists(self, view, first_list, n_lists, origin):
        """lists first_list .. first_list + n_lists - 1 of a svhip.view.View as one observation, device to device"""
        _check(self._L.svh_grid_observe_view_lists(self._h, view._h, first_list, n_lists, _xyz(origin).ctypes.data))

    def dyn_plane(self, which, device_ptr=None):
        """DYN_AGE, DYN_CONTRA or DYN_THROUGH, int32 [nz, nx]; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_dyn(self._h, which, device_ptr, 1))
            return None
        out = np.zeros((self.nz, self.nx), np.int32)
        _check(self._L.svh_grid_get_dyn(self._h, which, out.ctypes.data, 0))
        return out

    def dyn_stats(self):
        """dict of observations, cleared, aged, confirmed since the last clear"""
        out = np.zeros(4, np.int64)
        _check(self._L.svh_grid_get_dyn_stats(self._h, out.ctypes.data))
        return dict(zip(DYN_STATS, (int(v) for v in out)))

    def render_dyn(self, device_ptr=None):
        """render_local with the cells of CONTRA > 0 tinted and those the last observation cleared or aged in DYN_EVENT_COLOUR"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_dyn(self._h, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render_dyn(self._h, img.ctypes.data, 0))
        return img

    def set_archive(self, params=None, **kw):
        """the archive: the parameters in force (or `params`) with the fields of kw replaced: max_tiles, 0 = off.  The cells that scroll
        out of the window are kept by tiles of 16 x 16 and put back when the window returns"""
        p = (params if params is not None else self.archive()).copy(**kw)
        _check(self._L.svh_grid_set_archive(self._h, C.byref(p)))
        return p

    def archive(self):
        p = ArchiveParams()
        _check(self._L.svh_grid_get_archive(self._h, C.byref(p)))
        return p

    def archive_stats(self):
        """dict of pages, max_tiles, stored, restored, lost, refused since the archive was last emptied"""
        out = np.zeros(6, np.int64)
        _check(self._L.svh_grid_get_archive_stats(self._h, out.ctypes.data))
        return dict(zip(ARCHIVE_STATS, (int(v) for v in out)))

    def archive_clear(self):
        _check(self._L.svh_grid_archive_clear(self._h))

    def archive_trim(self, ga0, gb0, ga1, gb1):
        """drops every tile without a cell in the box of global cells, bounds inclusive"""
        _check(self._L.svh_grid_archive_trim(self._h, ga0, gb0, ga1, gb1))

    def archive_tiles(self, cap=None):
        """int32 [n, 2]: the tiles (ta, tb) that have a page, ascending by (tb, ta)"""
        n = C.c_int64(0)
        if cap is None:
            _check(self._L.svh_grid_archive_tiles(self._h, None, 0, C.addressof(n)))
            cap = n.value
        keys = np.zeros((max(cap, 1), 2), np.int32)
        _check(self._L.svh_grid_archive_tiles(self._h, keys.ctypes.data, cap, C.addressof(n)))
        return keys[:min(cap, n.value)].copy()

    def region(self, which, ga0, gb0, w, h, kind=REGION_GRID, device_ptr=None):
        """[h, w] of the plane's type over the box of global cells from (ga0, gb0), from the window and the archive together; kind
        REGION_GRID: a plane of plane(), REGION_LOCAL: one of local_plane().  With device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get_region(self._h, kind, which, ga0, gb0, w, h, device_ptr, 1))
            return None
        dtypes = PLANE_DTYPE if kind == REGION_GRID else LOCAL_DTYPE
        if kind not in (REGION_GRID, REGION_LOCAL) or not 0 <= which < len(dtypes) or not (1 <= w <= REGION_MAX_SIDE and 1 <= h <= REGION_MAX_SIDE):
            raise SvhError(ERR_BAD_ARG, "no such plane or box")
        out = np.zeros((h, w), dtypes[which])
        _check(self._L.svh_grid_get_region(self._h, kind, which, ga0, gb0, w, h, out.ctypes.data, 0))
        return out

    def render_region(self, ga0, gb0, w, h, mode=RENDER_LOCAL, device_ptr=None):
        """[h, w, 3] uint8 over the box, row 0 the farthest: render(mode), or render_local() with RENDER_LOCAL"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render_region(self._h, mode, ga0, gb0, w, h, device_ptr, 1))
            return None
        if not (1 <= w <= REGION_MAX_SIDE and 1 <= h <= REGION_MAX_SIDE):
            raise SvhError(ERR_BAD_ARG, "no such box")
        img = np.zeros((h, w, 3), np.uint8)
        _check(self._L.svh_grid_render_region(self._h, mode, ga0, gb0, w, h, img.ctypes.data, 0))
        return img

    def stats(self):
        st = Stats()
        _check(self._L.svh_grid_get_stats(self._h, C.byref(st)))
        return st

    def plane(self, which, device_ptr=None):
        """[nz, nx] of the plane's type; with device_ptr it is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_get(self._h, which, device_ptr, 1))
            return None
        if not 0 <= which < len(PLANE_DTYPE):
            raise SvhError(ERR_BAD_ARG, "no such plane")
        out = np.zeros((self.nz, self.nx), PLANE_DTYPE[which])
        _check(self._L.svh_grid_get(self._h, which, out.ctypes.data, 0))
        return out

    def count(self):
        return self.plane(COUNT)

    def overhead(self):
        return self.plane(OVERHEAD)

    def hmin(self):
        return self.plane(HMIN)

    def hmax(self):
        return self.plane(HMAX)

    def hmean(self):
        return self.plane(HMEAN)

    def intensity(self):
        return self.plane(INTENSITY)

    def classes(self):
        return self.plane(CLASS)

    def render(self, mode=RENDER_CLASS, device_ptr=None):
        """[nz, nx, 3] uint8, row 0 the farthest; with device_ptr the image is written there and None returned"""
        if device_ptr is not None:
            _check(self._L.svh_grid_render(self._h, mode, device_ptr, 1))
            return None
        img = np.zeros((self.nz, self.nx, 3), np.uint8)
        _check(self._L.svh_grid_render(self._h, mode, img.ctypes.data, 0))
        return img

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.svh_grid_destroy(h)

    def __del__(self):
        self.close()

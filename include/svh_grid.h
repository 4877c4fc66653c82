/*
 * svh_grid.h -- the ground grid: a 2.5-D bird's-eye grid over the road plane, binned on the device from the
 * accumulated map (svh_view.h) or from any list of (x, y, z, val) points.  Per cell: how many points, how high, how
 * bright, and whether the cell is drivable.  It is the consumer of the road plane of svh_plane.h, which the reference
 * computes and never applies (stereomapper/stereothread.cpp:152-164, under `if (0)`); the reference has no such grid.
 *
 * The contract is the arithmetic of stereo-vision_amd/csrc/grid_core.h (restated in tests/grid_ref.py and summarised in
 * DESIGN.md, "Ground grid").  Per point: a = T0.(x,y,z,1) lateral, b = T1.(x,y,z,1) forward, h = T2.(x,y,z,1) height,
 * in fp32; the cell is (floorf((a - x0) / cell), floorf((b - z0) / cell)).  A point is
 *   unplaced  if a coordinate or one of a, b, h is not finite,
 *   outside   if its cell is not in the window or not |h| < 2^20,
 *   overhead  if h > clearance (bridges, branches): only the cell's overhead count grows,
 *   low       otherwise: the cell's count, lowest and highest height, height sum (in 1/1024) and intensity sum grow.
 * Everything a cell accumulates is an integer under a commutative, associative update, so the grid depends only on
 * the multiset of points added since the last clear: never on their order, the launch shape or the scheduling.
 * The class of a cell (bits 0-1 of the class byte), tested in this order: 0 unknown (fewer than min_points low
 * points), 2 obstacle (HMAX > step), 3 drop (HMIN < -drop), 1 free.  Bit 7 (overhang): overhead >= min_points.
 *
 * A LOCAL MAP.  The window scrolls in whole cells and keeps what stays inside.  A point's global cell is (ga, gb) =
 * (floorf((a - x0) / cell), floorf((b - z0) / cell)); the window holds ga in oa .. oa + nx - 1 and gb in ob .. ob + nz - 1,
 * with the offsets (oa, ob) = (0, 0) at create and |oa|, |ob| <= 2^20 - 8192.  Every plane is in the window's order, index
 * (gb - ob) * nx + (ga - oa).  svh_grid_scroll moves the offsets: cells that stay keep everything they accumulated, the
 * strips that enter are empty, and the statistics go on counting since the last clear.
 * Free space is ray-cast: svh_grid_add_*_from bins points as svh_grid_add_* does and, for each LOW point, walks the line
 * from the origin's cell (ca, cb) to the point's cell (ea, eb): with dx = ea - ca, dz = eb - cb, n = max(|dx|, |dz|) and
 * rdiv(p, n) = floor((2 p + n) / (2 n)) (nearest, halves up) the cells (ca + rdiv(k dx, n), cb + rdiv(k dz, n)) for
 * k = 0 .. n - 1 -- the origin's cell is counted, the end cell is not.  Each gains one in the cell's PASS count.  The origin
 * itself must be a low point of the window (finite, inside, not above clearance), so every cell of a ray is inside the
 * window and below the clearance.  PASS is an integer sum too: it depends only on the multiset of (origin cell, end
 * cell) pairs.  A cell is SEEN when PASS >= min_points: unknown and seen is "looked through and found empty", unknown
 * and not seen is "never looked at".
 *
 * TRAVERSABILITY: what a planner reads, derived on the device from the finished planes (svh_grid_trav_params below).
 * A free cell is STEEP if one of its up to eight neighbours inside the window is free too and fabsf(HMEAN - HMEAN') exceeds
 * the rise: rise4 = max_slope * cell across an edge, rise8 = rise4 * 1.41421354f across a corner (one fp32 operation each).
 * Only free-free pairs are tested -- an obstacle does not thicken through its neighbours -- and both cells of a steep pair
 * are steep.  A cell is LETHAL if it matches a bit of the `lethal` mask: obstacle, drop, steep, unknown and not seen, unknown
 * and seen.  DIST2 is the exact squared Euclidean distance in cells to the nearest lethal cell of the window where that is at
 * most reach^2, reach = (int)ceil((double)inflate / (double)cell) in 1..256, else SVH_GRID_DIST2_FAR; a lethal cell has 0.
 * COST is one byte, a function of DIST2 alone, from a table filled in double on the host: 254 for DIST2 0; with
 * d = sqrt((double)DIST2) * (double)cell, 253 for d <= inscribed, 1 + (int)floor(251.0 * (inflate - d) / (inflate - inscribed))
 * (1..252) for d < inflate, else 0, and 0 for FAR.  A cell that is unknown and not lethal has 255, "no information", where
 * the table says 0.  The three planes are cached until the grid or the parameters change; a scroll needs nothing new.
 *
 * PLANNING: from a set of goal cells a cost-to-go field POT over the window, a direction field DIR and the shortest path
 * from any start, on the device; the arithmetic is stereo-vision_amd/csrc/grid_plan_core.h (restated in
 * tests/grid_plan_ref.py): integers on the finished COST plane in the window's order.  The PRICE of a cell of COST c is
 * neutral + c for c in 0..252 and neutral + unknown for 255 when unknown >= 0; cells of 253 and 254, and of 255 when
 * unknown < 0, are impassable.  The steps d = 0..7 are (da, db) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1).  A
 * step exists between two passable cells of the window; across a corner (odd d) only if the two cells that share an edge
 * with both, (a + da, b) and (a, b + db), are passable too -- there is no squeezing between two diagonal obstacles.  Its
 * weight is k (price(u) + price(v)), k = 5 across an edge, 7 across a corner: symmetric, 10..7098.  POT is 0 at a goal
 * that is inside the window and passable, elsewhere the least sum of weights over all step sequences to a goal where that
 * is at most max_cost (the cap drops every candidate above it), else SVH_GRID_PLAN_FAR.  DIR is 8 where POT is 0, 9 where
 * it is FAR, else the LOWEST d among the existing steps whose POT(v) + w(u, v) is least (that value is POT(u)).  A path
 * follows DIR from the start's cell until it reaches 8, at most nx * nz cells, and is a list of GLOBAL cells (ga, gb),
 * start first, goal last; its cost is POT(start).  POT is the unique fixed point of the relaxation and DIR and the path are
 * functions of it, so none depends on launch shape, scheduling or the order of the goals.
 * Goals are global cells: they survive svh_grid_scroll, svh_grid_follow and svh_grid_add_*, and are forgotten by
 * svh_grid_clear and svh_grid_set_window.  A goal that is outside the window, impassable or a duplicate does not count; it
 * is no error, the cost map changes from frame to frame.  The field is computed lazily and cached beside the cost planes
 * until the accumulators, the window's offsets, the traversability, the plan parameters or the goals change; unlike the
 * cost planes it is not kept under a scroll.  The planning entries return SVH_ERR_BAD_ARG while the traversability is not
 * set, as svh_grid_get_trav does.  After SVH_ERR_HIP in a planning entry the accumulated grid and the goals are untouched;
 * the field is invalid and the next call computes it again.
 *
 * FRONTIERS: where drivable ground ends and unlooked-at ground begins, grouped and handed to the planner as goals; the
 * arithmetic is stereo-vision_amd/csrc/grid_front_core.h (restated in tests/grid_front_ref.py): integers on the finished STATE
 * and COST planes in the window's order.  A cell is UNEXPLORED if its class is unknown and its seen bit matches the mask
 * `unexplored` (not seen matches SVH_GRID_LETHAL_UNSEEN, seen matches SVH_GRID_LETHAL_UNKNOWN_SEEN).  A cell is a FRONTIER cell
 * if its class is free, its COST is <= max_cell_cost and one of its four edge neighbours is unexplored; a neighbour position
 * outside the window counts as unexplored only when border != 0.  Components are the 8-connected sets of frontier cells.
 * LABEL is -1 off the frontier, elsewhere the LOWEST window index ib * nx + ia of the cell's component.  A component is KEPT
 * when it has at least min_size cells; each kept one has a record of ten int32, the records ascending by label: label, size,
 * the bounding box ga_min, gb_min, ga_max, gb_max in GLOBAL cells, the centroid cen_ga, cen_gb (per axis
 * floor((2 * sum + size) / (2 * size)) in window coordinates, then the offset) and the representative rep_ga, rep_gb: the
 * component's cell with the least squared distance to the centroid cell, ties to the lowest window index.  The centroid of a
 * curved frontier usually lies off it; the representative is always a frontier cell and is what goes to the planner.  Labels
 * are minima, sizes and sums integer sums, boxes minima and maxima, the representative the minimum of a unique key: no byte
 * depends on launch shape or scheduling.  The result is computed lazily and cached until the accumulators, the window's
 * offsets, the traversability or the frontier parameters change.  The frontier entries return SVH_ERR_BAD_ARG while the
 * traversability is not set, as svh_grid_get_trav does.  After SVH_ERR_HIP in a frontier entry the accumulated grid, the cost
 * planes, the goals and the field are untouched; the frontier result is invalid and the next call computes it again.
 *
 * ROLLOUT: what a controller asks every frame -- of these short motions, which keep the whole vehicle off the obstacles, and which
 * ends nearest the goal?  The arithmetic is stereo-vision_amd/csrc/grid_roll_core.h (restated in tests/grid_roll_ref.py): integers
 * on the finished COST and POT planes in the window's order.  HEADINGS are integer direction vectors, no trigonometric function
 * appears: with m = headings_m there are H = 8 m of them, heading k the vector (ux, uz) in (lateral a, forward b) on the perimeter of
 * the square [-m, m]^2, counter-clockwise from (m, 0): (m, k) for k in 0..m, (2m - k, m) for m..3m, (-m, 4m - k) for 3m..5m,
 * (k - 6m, -m) for 5m..7m, (m, k - 8m) for 7m..8m; straight ahead is k = 2m.  The heading of a direction (ua, ub), in fp32 with one
 * rounding per operation: if |ua| >= |ub|, q = (int)rintf(ub * (float)m / |ua|) and k = (q + 8m) mod 8m for ua > 0, 4m - q for
 * ua < 0; otherwise q = (int)rintf(ua * (float)m / |ub|) and k = 2m - q for ub > 0, 6m + q for ub < 0; a direction that is not finite,
 * zero, or whose quotient is not within [-m, m] has none.  The FOOTPRINT TABLE, filled on the host in double once per
 * svh_grid_set_roll, has one list of cell offsets (da, db) per heading, the vehicle's reference point at the centre of its cell:
 * with c = (double)cell, h = 0.5 c, rt = sqrt((double)(ux ux + uz uz)), l = da ux + db uz and t = db ux - da uz the offset is in the
 * list iff (double)l c <= ((double)front + h) rt, -(double)l c <= ((double)rear + h) rt and fabs((double)t) c <= ((double)half_width
 * + h) rt, each product one double operation; (0, 0) is always in, a point vehicle covers one cell at every heading.  Offsets are
 * searched in [-R, R]^2, R = (int)ceil((max(front, rear) + half_width + c) / c) in 1..128; a list is ascending by (db, da).  The
 * FOOTPRINT COST F of a pose (ga, gb, k), a global cell and a heading, is -1 if a footprint cell lies outside the window, else the
 * maximum over the footprint cells of r(COST), r(c) = c for 0..254 and r(255) = unknown_cost.  CANDIDATES are a table of S sets x K
 * candidates x T poses of three int32 (dga, dgb, k): offsets from an anchor cell and an absolute heading; k = -1 ends a candidate,
 * its length n_c is the number of poses before the first -1 (what follows is not looked at).  S, K, T >= 1, T <= 1024, K <= 65536,
 * S K T <= 2^22, |dga|, |dgb| <= 16384.  SCORING a set at an anchor: F_t at every t < n_c; the candidate is cut at the first t with
 * F_t = -1 (status 2, the window) or F_t >= stop_cost (status 1, cost; 255 never cuts), else it is complete (status 0); n_c = 0 has
 * status 3.  L is the number of poses before the cut.  The record is five int32: L, status, maxF over the L poses (-1 for L = 0),
 * sumF over them, and pot_end, POT at the reference cell of pose L - 1 -- SVH_GRID_PLAN_FAR if L = 0 or w_pot = 0, when the field is
 * neither computed nor read.  A candidate is feasible iff L >= 1 and (w_pot = 0 or pot_end != FAR); its score, int64, is w_pot pot_end
 * + w_cost sumF + w_cut (n_c - L), INT64_MAX when infeasible; the best is the feasible candidate with the least (score, index), -1 if
 * none.  F is a maximum, sumF an integer sum, the cut a first index, the best the minimum of unique keys: no byte depends on launch
 * shape or scheduling.  Both tables are relative: they survive svh_grid_scroll, svh_grid_follow, svh_grid_add_*, svh_grid_clear
 * and svh_grid_set_window; svh_grid_set_roll with another headings_m forgets the candidates, whose headings it renumbers.  A scoring
 * is computed per call and not cached; it uses the cached cost planes and, for w_pot > 0, the cached field.  The scoring entries
 * return SVH_ERR_BAD_ARG while the traversability is not set or the vehicle does not fit (below).  After SVH_ERR_HIP in a rollout
 * entry the accumulated grid, the cost planes, the goals, the field, the frontier result and both tables are untouched.
 *
 * EXPLORATION: which frontier to drive to -- what would be seen from it, and what it costs to get there.  The arithmetic is
 * stereo-vision_amd/csrc/grid_explore_core.h (restated in tests/grid_explore_ref.py): integers on the finished STATE and COST planes
 * in the window's order.  R = (int)floorf(range / cell), 1..128.  From a VIEWPOINT, a window cell (va, vb), one ray goes to each of
 * the 8 R offsets (dx, dz) on the perimeter of the square [-R, R]^2; for k = 1..R it visits the offset (sx, sz) = (rdiv(k dx, R),
 * rdiv(k dz, R)), rdiv(p, n) = floor((2 p + n) / (2 n)), the line of the free-space rays.  A ray ends before the first k at which
 * sx^2 + sz^2 > R^2, the cell lies outside the window, or the cell's class is obstacle.  Unknown cells, drops, steep cells and the
 * lethal inflation do not block; only visited cells block, so a viewpoint on an obstacle cell still casts its rays, and a diagonal
 * step between two obstacle cells passes.  VIEW of a viewpoint, one byte per cell: 0 no ray visits the cell (the viewpoint's own
 * cell included), 1 visited, 2 visited and UNEXPLORED under the frontier parameters in force.  GAIN is the number of cells with
 * VIEW 2, each counted once however many rays visit it; -1 for a viewpoint outside the window.  In a window without obstacles the
 * visited set is the disc 0 < sx^2 + sz^2 <= R^2 clipped to the window.  REACH of a cell from a start cell is POT of PLANNING under
 * the plan parameters in force with the start as the only goal, read at the cell -- weights and the corner rule are symmetric, so
 * it is the cost of the path from the start to the cell; SVH_GRID_PLAN_FAR when the start is outside the window or impassable, the
 * cell unreachable or the cost beyond max_cost.  RANKING: for each kept frontier component, the first 65536 in ascending label, a
 * record of five int32: label, rep_ga, rep_gb, the gain of the representative, its reach.  A record is feasible iff reach != FAR
 * and gain >= min_gain; its int64 score is w_reach reach - w_gain gain, INT64_MAX when infeasible; the best is the feasible record
 * with the least (score, index), -1 if none.  GAIN is the size of a set, REACH a value of the planner's fixed point, the best the
 * minimum of unique keys: no byte depends on launch shape or scheduling.  Gains and VIEW planes are computed per call and not
 * cached.  The reach field lives in buffers of its own beside the planner's: a ranking neither changes the goals nor touches or
 * invalidates the planner's field.  It is cached until the start cell, the accumulators, the window's offsets, the
 * traversability or the plan parameters change.  The exploration entries return SVH_ERR_BAD_ARG while the traversability is not
 * set or the range does not fit the grid's cell (below).  After SVH_ERR_HIP in an exploration entry the accumulated grid, the
 * cost planes, the goals, the field, the frontier result and the roll tables are untouched; the reach field is invalid and the
 * next ranking computes it again.
 *
 * ALIGN: where a frame's obstacle points fit the obstacle cells the window already holds -- correlative scan-to-map matching over a
 * small window of pose corrections.  A FRAME IS ALIGNED BEFORE IT IS ADDED: a frame already in the grid matches itself.  The
 * arithmetic is stereo-vision_amd/csrc/grid_align_core.h (restated in tests/grid_align_ref.py); after the fp32 placement of a point
 * it is integer arithmetic on the finished STATE plane.
 *   SUBS.  A sub is a quarter of a cell per axis.  The global sub of a ground position (a, b) is ua = (int)floorf(((a - x0) / cell)
 *   * 4), ub likewise with z0, fp32 with one rounding per operation; a position has one iff |floorf((a - x0) / cell)| < 2^20 on
 *   both axes, and ua >> 2 is its global cell.
 *   PIVOT.  A map-frame position (the camera's), rounded to float once; its global sub is (Pa, Pb).  It need not lie inside the
 *   window.  A pivot that is not finite or has no sub is SVH_ERR_BAD_ARG before anything is read or changed.
 *   SCAN.  A point is a scan point iff x, y, z, a, b, h are finite, |h| < 2^20, step < h <= clearance -- what would make its cell
 *   an obstacle -- and it has a global sub.  With Rg = floor(range / cell) in 1..256 it is kept iff |ua - Pa| <= 4 Rg and
 *   |ub - Pb| <= 4 Rg.  The scan is the SET of distinct kept subs: it depends on neither order nor multiplicity.  n_scan is its
 *   size, at most (8 Rg + 1)^2.  It may hold subs outside the window.
 *   FIELD.  F, one byte per window cell: with reach_cells = ceil(reach / cell) in 1..32, R2 = reach_cells^2 and d2 the exact squared
 *   distance in cells to the nearest obstacle cell (bits 0-1 of STATE) of the window, F = (255 (R2 + 1 - d2)) / (R2 + 1) in integer
 *   division for d2 <= R2, else 0.  It reads neither the traversability nor the cost planes.  Cached until the accumulators, the
 *   window's offsets or the align parameters change.
 *   SAMPLE.  F at a global sub is bilinear between cell centres in eighths of a cell: pa = 2 ua - 3 - 8 oa, g0a = pa >> 3
 *   (arithmetic), fa = pa - 8 g0a in {1, 3, 5, 7}, the b axis alike; the cells (g0a + i, g0b + j), i, j in {0, 1}, weigh
 *   (i ? fa : 8 - fa) (j ? fb : 8 - fb), a cell outside the window contributes 0, and the sample is (sum + 32) >> 6, 0..255.
 *   CANDIDATES (k, ta, tb): k in -K..K (K = rot_n), ta, tb in -W..W subs (W = trans_n).  Rotation k turns by the direction (D, k),
 *   D = rot_den, from the a axis towards the b axis: n = sqrt(D D + k k), cq = rint(16384 D / n), sq = rint(16384 k / n) in double.
 *   A scan sub with (ra, rb) = (ua - Pa, ub - Pb) is placed at (Pa + ((cq ra - sq rb + 8192) >> 14) + ta,
 *   Pb + ((sq ra + cq rb + 8192) >> 14) + tb).  k = 0 is the identity.
 *   VOLUME AND BEST.  SCORE(k, ta, tb) is the int32 sum of the samples over the scan, stored as [k + K][tb + W][ta + W].  The best
 *   is the greatest score; among equal scores the least k^2 + ta^2 + tb^2, among those the lowest volume index.  `ties` counts the
 *   candidates whose score equals the best: it is how a caller sees the aperture problem of a single straight wall.  A flat volume
 *   returns the identity.  No byte depends on launch shape or scheduling.
 *   RECORD, eight int32: status, k, ta, tb, score, SCORE(0, 0, 0), n_scan, ties.  SVH_GRID_ALIGN_FEW: n_scan < min_scan, no volume is
 *   computed, k = ta = tb = score = identity = ties = 0.  SVH_GRID_ALIGN_FLAT: the best score is 0 -- the map has no obstacle within
 *   reach of any candidate -- and the identity is returned.
 *   CORRECTION.  svh_grid_align_correction turns (k, ta, tb) and the pivot into a map-frame transform M, on the host in double from
 *   the float-rounded T and pivot: X' = p + Rot(X - p) + (ta cell / 4) e_a + (tb cell / 4) e_b, with e_a, e_b, e_h the first three
 *   columns of T's rows and Rot turning the e_a / e_b components by (cos, sin) = (D / n, k / n).  Exact for a T with orthonormal
 *   rows, which svh_grid_frame_camera and svh_grid_frame_plane give.  A caller multiplies its camera pose by M before it adds the
 *   frame.
 * The align entries return SVH_ERR_BAD_ARG while the align parameters are not set.  An alignment changes nothing else: the
 * accumulators, the statistics, the cost planes, the goals, the planner's field, the frontier result, the roll tables and the reach
 * field stay as they were.  After SVH_ERR_HIP in an align entry the same holds; the align field and the last volume are invalid and
 * the next call computes them again.
 *
 * DYNAMICS: the world moves.  Everything above accumulates since the last clear, so a car that crosses in front of the camera
 * leaves a wall of obstacle cells along its track.  With the dynamics set (svh_grid_set_dynamics) a frame can be given as an
 * OBSERVATION (svh_grid_observe_*) instead of an add: it clears obstacle cells that the frame's sight lines contradict, and ages
 * cells that have not been seen for long.  The arithmetic is stereo-vision_amd/csrc/grid_dyn_core.h (restated in
 * tests/grid_dyn_ref.py); integers after the placement of a point.  Observations are numbered by a STAMP, int32, 1 for the first
 * after a clear; svh_grid_clear and svh_grid_set_window reset it.  An observation has three phases, each a pure function of its
 * inputs, so the result depends only on the state before and the MULTISET of the frame's points:
 *   1  FRAME RECORD.  Every point is placed as an add places it; the frame's low and overhead points are accumulated per cell into
 *      a frame record (fcount, foverhead, fkmin, fkmax, fhsum, fvsum) beside the cell, not into it.  The statistics count as in an add.
 *   2  SIGHT LINES.  For every end cell with fcount > 0 one line of weight fcount runs from the origin's cell: the cells of a
 *      free-space ray, k = 0 .. n - 1.  Each gains fcount in PASS, so PASS and the ray statistics are what svh_grid_add_points_from
 *      would have left.  The line has a height in 1/1024: q_k = q_o + rdiv64(k (q_e - q_o), n), rdiv64 being rdiv in 64 bits,
 *      q_o = rintf(h * 1024) of the origin and q_e = rintf(fhmin * 1024), the frame's lowest low point of the end cell.  A stored
 *      cell is TALL if COUNT > 0 and HMAX > step; its body is [rintf(HMIN * 1024), rintf(HMAX * 1024) - rintf(margin * 1024)].  A line
 *      step in a tall cell goes THROUGH it iff q_k lies in the body, ends included.  A line above the body sees over the obstacle,
 *      one below passes under it (a trailer); neither contradicts it.  THROUGH of a cell is the sum of the weights of the lines that
 *      go through.
 *   3  SETTLE, per window cell, in this order.  Confirm: fcount > 0 and the frame's highest low point > step: CONTRA = 0.  Otherwise,
 *      if the cell is tall and THROUGH >= min_through: CONTRA += 1.  If clear_frames > 0 and CONTRA >= clear_frames the cell is
 *      CLEARED: its low points are forgotten (OVERHEAD and PASS stay: a bridge over a cleared car is still a bridge), CONTRA = 0.
 *      If max_age > 0, the cell stores a point and stamp - LAST > max_age it is AGED: everything but PASS is forgotten, CONTRA = 0; a
 *      cell cleared in the same observation counts as cleared only.  Then the frame record is merged into the cell, and LAST = stamp
 *      if the frame had a point in it.
 * CONTRA and LAST (0 = never) belong to the cell: a scroll keeps them for cells that stay and empties them in the strips that
 * enter, svh_grid_clear and svh_grid_set_window empty them.  With clear_frames = 0 and max_age = 0 an observation leaves every
 * plane of svh_grid_get and svh_grid_get_local and the statistics bit-equal to svh_grid_add_points_from of the same arguments.
 * The plain add entries stay legal with the layer set: they write the accumulators directly and leave CONTRA and LAST alone -- a
 * cell filled only by adds has LAST 0 and, under max_age > 0, is aged by the first observation after stamp max_age.  An observation
 * invalidates what an add invalidates.  After SVH_ERR_HIP inside svh_grid_observe_* the grid is EMPTY as after a failed add:
 * statistics, stamp, CONTRA and LAST included; the parameters of the layer stay set and the next observation has stamp 1.
 *
 * OBJECTS: the obstacle cells grouped into things, and their tracks from frame to frame (svh_grid_set_objects, svh_grid_get_objects,
 * svh_grid_objects_step, svh_grid_get_tracks, svh_grid_render_objects).  The text and the entries are in svh_grid_obj.h, which this
 * header includes at its end.
 *
 * Plain C like svh_view.h.  An object has its own stream and every call returns when it is complete.  Calls return
 * SVH_OK or a negative SVH_ERR_*; svh_last_error() has the text.  SVH_ERR_BAD_ARG -- a null pointer, parameters out of
 * the ranges below, n < 0, n > 0 with a null array, a device array that is not 16-byte aligned, an unknown plane or
 * mode -- is decided before anything is read or changed.  svh_grid_create returns NULL without a HIP device.
 * SVH_ERR_UNSUPPORTED, nothing changed: the object would have been given more than 2^31 - 1 points since the last
 * clear (counts are 32 bits).  After SVH_ERR_HIP inside svh_grid_add_* or svh_grid_scroll / svh_grid_follow the grid is
 * EMPTY (accumulation is in place, a half-done call cannot be taken back): all statistics are zero, the next add starts
 * afresh, and after a failed scroll the window stands at its new offsets.  After SVH_ERR_HIP
 * inside svh_grid_get, svh_grid_render, svh_grid_get_trav, svh_grid_render_cost or svh_grid_set_traversability the
 * accumulated grid is untouched.
 */
#ifndef SVH_GRID_H
#define SVH_GRID_H

#include <stddef.h>
#include <stdint.h>

#include "svh.h"       /* SVH_OK, SVH_ERR_*, svh_last_error */
#include "svh_view.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svh_grid svh_grid;

typedef struct svh_grid_params {
    int32_t nx, nz;            /* cells across (lateral) and along (forward); each 1..8192 */
    float   cell;              /* side of a cell, finite, > 0 */
    float   x0, z0;            /* ground coordinates of the low corner of cell (0, 0), finite */
    double  T[12];             /* 3x4 row major, camera/map frame -> ground frame; rounded to float once at create
                                  (the rounded values must be finite): rows a lateral, b forward, h height, road h = 0 */
    int32_t min_points;        /* 3: fewer low points than this -> the cell is unknown; >= 1 */
    float   step;              /* 0.2: a cell whose highest low point is above this is an obstacle; finite, >= 0 */
    float   drop;              /* 0.3: a cell whose lowest point is below -drop is a drop; finite, >= 0 */
    float   clearance;         /* 2.0: points above this are overhead, not obstacles; finite, > step */
    float   render_h_lo, render_h_hi;   /* 0, 2: range of the height colouring; finite, lo < hi */
} svh_grid_params;

typedef struct svh_grid_stats { int64_t added, binned, overhead, outside, unplaced; } svh_grid_stats;

/* planes of svh_grid_get, row major, index = ib * nx + ia (ia lateral, ib forward) */
#define SVH_GRID_COUNT      0   /* int32: low points */
#define SVH_GRID_OVERHEAD   1   /* int32: overhead points */
#define SVH_GRID_HMIN       2   /* float: lowest low point, NaN where COUNT is 0 */
#define SVH_GRID_HMAX       3   /* float: highest low point, NaN where COUNT is 0 */
#define SVH_GRID_HMEAN      4   /* float: (float)((double)sum of rintf(h * 1024) / (1024.0 * COUNT)), NaN where COUNT is 0 */
#define SVH_GRID_INTENSITY  5   /* uint8: mean of (uint8)rintf(clamp(val, 0, 1) * 255), rounded half up; 0 where COUNT is 0 */
#define SVH_GRID_CLASS      6   /* uint8: class in bits 0-1, overhang in bit 7 */
/* modes of svh_grid_render */
#define SVH_GRID_RENDER_CLASS      0   /* unknown (32,32,32), free (0, 64 + 3 I / 4, 0), obstacle (255,0,0), drop (0,0,160);
                                          with the overhang bit the blue byte is 255 */
#define SVH_GRID_RENDER_HEIGHT     1   /* HMAX over render_h_lo..render_h_hi through the disparity colour map; black where
                                          COUNT is 0 and at or below render_h_lo */
#define SVH_GRID_RENDER_INTENSITY  2   /* grey; black where COUNT is 0 */

/* 256 x 256 cells of 0.2 m, x0 = -25.6, z0 = 0, T = svh_grid_frame_camera(1.65), the thresholds above */
void      svh_grid_params_default(svh_grid_params* p);
/* a level camera cam_height above the road, x right, y down, z forward: rows (1,0,0,0), (0,0,1,0), (0,-1,0,cam_height) */
int32_t   svh_grid_frame_camera(double cam_height, double T[12]);
/* from svh_plane_get_plane_euclidean (the road is e.X = 1) and svh_plane_get_transformation (columns r1 right, r2 down,
 * r3 forward): rows a = r1.X, b = r3.X, h = 1/|e| - (e/|e|).X.  SVH_ERR_BAD_ARG for |e| == 0 -- what the estimate leaves
 * after SVH_PLANE_NO_POINTS or SVH_PLANE_FEW_INLIERS -- or an input that is not finite.  Needs no device.           */
int32_t   svh_grid_frame_plane(const double plane_e[3], const double H[16], double T[12]);

svh_grid* svh_grid_create(const svh_grid_params* p);   /* NULL: bad parameters, or no HIP device */
void      svh_grid_destroy(svh_grid* g);
int32_t   svh_grid_clear(svh_grid* g);
int32_t   svh_grid_set_window(svh_grid* g, float x0, float z0);   /* a new low corner; clears, and the offsets are 0 again */

/* the window moves by (da, db) whole cells and keeps what stays inside; |da| >= nx or |db| >= nz empties the grid.
 * SVH_ERR_BAD_ARG, nothing changed: an offset would leave -(2^20 - 8192) .. 2^20 - 8192 */
int32_t   svh_grid_scroll(svh_grid* g, int32_t da, int32_t db);
int32_t   svh_grid_get_window(svh_grid* g, int32_t off[2]);            /* (oa, ob) */
/* the global cell (ga, gb) of a map-frame position (rounded to float once); SVH_ERR_BAD_ARG: not finite, or |ga| or |gb|
 * not below 2^20 */
int32_t   svh_grid_cell_of(svh_grid* g, const double xyz[3], int32_t cell[2]);
/* scrolls so that the cell of xyz becomes window cell (ia, ib), 0 <= ia < nx, 0 <= ib < nz */
int32_t   svh_grid_follow(svh_grid* g, const double xyz[3], int32_t ia, int32_t ib);

/* n points (x, y, z, val), on the host or (on_device) in device memory, 16-byte aligned there */
int32_t   svh_grid_add_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device);
/* the view's whole store, device to device, no host copy; an empty view: SVH_OK, nothing changes */
int32_t   svh_grid_add_view(svh_grid* g, svh_view* v);
/* svh_grid_add_points, and one ray per low point from the cell of `origin` (a map-frame position, rounded to float once).
 * SVH_ERR_BAD_ARG, before anything is read or changed: the origin is not a low point of the window */
int32_t   svh_grid_add_points_from(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device, const double origin[3]);
/* the same for the lists first_list .. first_list + n_lists - 1 of the view's sequence, device to device;
 * SVH_ERR_BAD_ARG: the range is not inside the sequence */
int32_t   svh_grid_add_view_lists_from(svh_grid* g, svh_view* v, int32_t first_list, int32_t n_lists, const double origin[3]);
/* since the last clear: out[0] rays (the low points added through the _from entries), out[1] the sum of PASS increments */
int32_t   svh_grid_get_ray_stats(svh_grid* g, int64_t out[2]);
/* totals since the last clear; added = binned + overhead + outside + unplaced */
int32_t   svh_grid_get_stats(svh_grid* g, svh_grid_stats* stats);

/* one plane, nx * nz elements of its type, to the host or (on_device) a device pointer */
int32_t   svh_grid_get(svh_grid* g, int32_t plane, void* out, int32_t on_device);
/* nx x nz RGB8; row 0 is the farthest row (ib = nz - 1): forward is up */
int32_t   svh_grid_render(svh_grid* g, int32_t mode, uint8_t* rgb, int32_t on_device);


/* planes of svh_grid_get_local, laid out as those of svh_grid_get */
#define SVH_GRID_LOCAL_PASS   0   /* int32: rays that passed the cell */
#define SVH_GRID_LOCAL_STATE  1   /* uint8: the byte of SVH_GRID_CLASS with bit 6 (seen) where PASS >= min_points */
int32_t   svh_grid_get_local(svh_grid* g, int32_t plane, void* out, int32_t on_device);
/* SVH_GRID_RENDER_CLASS, except that a cell that is unknown and seen is (96, 112, 96) instead of (32, 32, 32) */
int32_t   svh_grid_render_local(svh_grid* g, uint8_t* rgb, int32_t on_device);


/* bits of svh_grid_trav_params.lethal */
#define SVH_GRID_LETHAL_OBSTACLE      1u    /* class obstacle */
#define SVH_GRID_LETHAL_DROP          2u    /* class drop */
#define SVH_GRID_LETHAL_STEEP         4u    /* steep */
#define SVH_GRID_LETHAL_UNSEEN        8u    /* unknown and not seen */
#define SVH_GRID_LETHAL_UNKNOWN_SEEN  16u   /* unknown and seen */
#define SVH_GRID_DIST2_FAR  0x7FFFFFFF      /* DIST2 of a cell with no lethal cell within reach */

typedef struct svh_grid_trav_params {
    float    max_slope;        /* 0.35: rise over run between neighbouring free cells; finite, > 0 */
    float    inscribed;        /* 0.4: metres; closer to a lethal cell than this is as good as lethal; finite, >= 0 */
    float    inflate;          /* 1.5: metres; beyond this a lethal cell costs nothing; finite, > inscribed */
    uint32_t lethal;           /* obstacle, drop, steep: a mask of SVH_GRID_LETHAL_*, no other bits */
} svh_grid_trav_params;

void      svh_grid_trav_params_default(svh_grid_trav_params* t);
/* checks the parameters, derives rise4, rise8 and reach for the grid's cell and uploads the cost table.  SVH_ERR_BAD_ARG,
 * nothing changed: a parameter out of its range, or a reach outside 1..256.  A grid is created with the defaults; if their
 * reach is outside 1..256 for the grid's cell the object exists, and svh_grid_get_trav and svh_grid_render_cost return
 * SVH_ERR_BAD_ARG until this call succeeds.  After SVH_ERR_HIP the parameters are set and the next svh_grid_get_trav or
 * svh_grid_render_cost uploads the table again. */
int32_t   svh_grid_set_traversability(svh_grid* g, const svh_grid_trav_params* t);
/* the parameters in force and their reach in cells (0 while the defaults do not fit); either output may be NULL, not both */
int32_t   svh_grid_get_traversability(svh_grid* g, svh_grid_trav_params* t, int32_t* reach);
/* planes of svh_grid_get_trav, laid out as those of svh_grid_get */
#define SVH_GRID_TRAV_FLAGS 0   /* uint8: bit 0 steep, bit 1 lethal */
#define SVH_GRID_TRAV_DIST2 1   /* int32 */
#define SVH_GRID_TRAV_COST  2   /* uint8 */
int32_t   svh_grid_get_trav(svh_grid* g, int32_t plane, void* out, int32_t on_device);
/* the cost as nx x nz RGB8, rows as svh_grid_render: 254 (255, 0, 0), 253 (255, 128, 0), c in 1..252 (c, 0, 255 - c),
 * 0 (0, 96, 0), 255 (32, 32, 32); a steep cell has the green byte 255 */
int32_t   svh_grid_render_cost(svh_grid* g, uint8_t* rgb, int32_t on_device);


#define SVH_GRID_PLAN_FAR  0x7FFFFFFF       /* POT of a cell that no goal is reached from within max_cost */

typedef struct svh_grid_plan_params {
    int32_t neutral;           /* 50: price of a cell of cost 0; 1..255 */
    int32_t unknown;           /* -1: cells of COST 255 are impassable; 0..252: they cost this much */
    int32_t max_cost;          /* 0x7FFFFFFE: horizon; 1..0x7FFFFFFE */
} svh_grid_plan_params;

void      svh_grid_plan_params_default(svh_grid_plan_params* p);
int32_t   svh_grid_set_plan(svh_grid* g, const svh_grid_plan_params* p);   /* SVH_ERR_BAD_ARG, nothing changed: out of range */
int32_t   svh_grid_get_plan(svh_grid* g, svh_grid_plan_params* p);
/* n >= 0 goals as global cells (ga, gb), |ga|, |gb| < 2^20, n <= 65536; copied; n = 0 forgets them */
int32_t   svh_grid_plan_set_goals(svh_grid* g, const int32_t* cells, int32_t n);
/* one goal from a map-frame position, through svh_grid_cell_of */
int32_t   svh_grid_plan_set_goal(svh_grid* g, const double xyz[3]);
/* planes of svh_grid_get_plan_plane, laid out as those of svh_grid_get */
#define SVH_GRID_PLAN_POT 0   /* int32; a device array is 4-byte aligned */
#define SVH_GRID_PLAN_DIR 1   /* uint8 */
int32_t   svh_grid_get_plan_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device);
/* out[0] goals given, out[1] of them inside the window and passable now (a duplicate once), out[2] cells with POT != FAR,
 * out[3] relaxation rounds of the last field (the only figure here that may differ from run to run: how many rounds the
 * device needed depends on its scheduling, the field does not) */
int32_t   svh_grid_get_plan_stats(svh_grid* g, int64_t out[4]);
#define SVH_GRID_PATH_FOUND        0
#define SVH_GRID_PATH_UNREACHABLE  1   /* the start is passable, POT is FAR (no goals included) */
#define SVH_GRID_PATH_BLOCKED      2   /* the start cell is impassable */
#define SVH_GRID_PATH_OUTSIDE      3   /* the start cell is not in the window */
/* returns a status above or a negative error; *len = cells of the whole path (0 unless FOUND), the first min(*len, cap) of
 * them written to cells[2 * i], cells[2 * i + 1] (host memory); *cost = POT(start) or SVH_GRID_PLAN_FAR; cells may be NULL
 * with cap 0 */
int32_t   svh_grid_plan_path(svh_grid* g, const double start_xyz[3], int32_t* cells, int64_t cap, int64_t* len, int32_t* cost);
/* svh_grid_render_cost with the goals that count drawn (255, 255, 0) and the n given global cells (a path, host memory) drawn
 * (255, 255, 255) over them; cells outside the window are skipped; n may be 0 */
int32_t   svh_grid_render_plan(svh_grid* g, const int32_t* cells, int64_t n, uint8_t* rgb, int32_t on_device);


typedef struct svh_grid_front_params {
    int32_t  max_cell_cost;    /* 252: a frontier cell has a COST of at most this; 0..252 */
    int32_t  min_size;         /* 8: components of fewer cells are dropped; 1..2^26 */
    uint32_t unexplored;       /* SVH_GRID_LETHAL_UNSEEN: what counts as unexplored, a non-empty mask of SVH_GRID_LETHAL_UNSEEN |
                                  SVH_GRID_LETHAL_UNKNOWN_SEEN, no other bits */
    int32_t  border;           /* 0: positions outside the window are not unexplored; 1: they are */
} svh_grid_front_params;

void      svh_grid_front_params_default(svh_grid_front_params* p);
int32_t   svh_grid_set_frontier(svh_grid* g, const svh_grid_front_params* p);   /* SVH_ERR_BAD_ARG, nothing changed: out of range */
int32_t   svh_grid_get_frontier(svh_grid* g, svh_grid_front_params* p);
/* planes of svh_grid_get_front_plane, laid out as those of svh_grid_get */
#define SVH_GRID_FRONT_FLAGS 0   /* uint8: bit 0 frontier, bit 1 in a kept component, bit 2 representative */
#define SVH_GRID_FRONT_LABEL 1   /* int32: -1 off the frontier, else the lowest index of the component; a device array is 4-byte aligned */
int32_t   svh_grid_get_front_plane(svh_grid* g, int32_t plane, void* out, int32_t on_device);
#define SVH_GRID_FRONT_RECORD 10 /* int32 per record: label, size, ga_min, gb_min, ga_max, gb_max, cen_ga, cen_gb, rep_ga, rep_gb */
/* *n = the kept components; the first min(*n, cap) records, ascending by label, to recs (host memory); recs may be NULL with cap 0 */
int32_t   svh_grid_get_frontiers(svh_grid* g, int32_t* recs, int64_t cap, int64_t* n);
/* out[0] frontier cells, out[1] components, out[2] kept components, out[3] cells in kept components, out[4] kernel launches
 * of the last computation (a constant of the build: it does not depend on the scene) */
int32_t   svh_grid_get_frontier_stats(svh_grid* g, int64_t out[5]);
/* the representatives of the kept components become the planner's goals (svh_grid_plan_set_goals), the first 65536 by label;
 * returns how many, or a negative error.  A snapshot: the goals are global cells and do not follow a changing frontier */
int32_t   svh_grid_plan_set_goals_frontiers(svh_grid* g);
/* svh_grid_render_cost with the frontier cells over it: of a kept component (0, 255, 255), of a dropped one (0, 96, 128),
 * representatives (255, 255, 0) */
int32_t   svh_grid_render_frontiers(svh_grid* g, uint8_t* rgb, int32_t on_device);


typedef struct svh_grid_roll_params {
    float   front, rear, half_width;   /* 3.5, 1.0, 0.9: metres from the reference point to the front, the rear and either side; finite, >= 0 */
    int32_t headings_m;                /* 8: 64 headings; 1..32 */
    int32_t stop_cost;                 /* 253: a pose whose F is at least this cuts its candidate; 1..255, 255 never cuts */
    int32_t unknown_cost;              /* 254: what a cell of COST 255 counts as under a footprint; 0..254 */
    int32_t w_pot, w_cost, w_cut;      /* 1, 1, 0: the weights of the score; 0..65535 */
} svh_grid_roll_params;

#define SVH_GRID_ROLL_RECORD 5         /* int32 per record: L, status, maxF, sumF, pot_end */
#define SVH_GRID_ROLL_COMPLETE    0
#define SVH_GRID_ROLL_CUT_COST    1
#define SVH_GRID_ROLL_CUT_WINDOW  2
#define SVH_GRID_ROLL_EMPTY       3    /* a candidate of no poses */

void      svh_grid_roll_params_default(svh_grid_roll_params* p);
/* checks the parameters, fills the footprint table for the grid's cell and uploads it.  SVH_ERR_BAD_ARG, nothing changed: a
 * parameter out of its range, or R outside 1..128.  A grid is created with the defaults; if their R does not fit the grid's cell the
 * object exists, and svh_grid_roll_footprint, svh_grid_footprint_cost and svh_grid_roll_score return SVH_ERR_BAD_ARG until this call
 * succeeds.  After SVH_ERR_HIP the parameters are set and the next call that needs the table uploads it again. */
int32_t   svh_grid_set_roll(svh_grid* g, const svh_grid_roll_params* p);
/* the parameters in force, their R (0 while the defaults do not fit) and the cells of all lists; any output may be NULL, not all */
int32_t   svh_grid_get_roll(svh_grid* g, svh_grid_roll_params* p, int32_t* reach_R, int64_t* footprint_cells_total);
/* the heading of a map-frame direction: rows a and b of T without the translation, the direction rounded to float once.
 * SVH_ERR_BAD_ARG: it has none */
int32_t   svh_grid_heading_of(svh_grid* g, const double dir_xyz[3], int32_t* k);
/* the list of heading k: *n its cells, the first min(*n, cap) pairs (da, db) to offsets (host memory); offsets may be NULL with cap 0 */
int32_t   svh_grid_roll_footprint(svh_grid* g, int32_t k, int32_t* offsets, int64_t cap, int64_t* n);
/* F of n poses (ga, gb, k), n <= 2^26: poses and out both on the host or (on_device) both in device memory, 4-byte aligned there.  A
 * heading outside 0..8 m - 1 is SVH_ERR_BAD_ARG on the host path and gives F = -1 on the device path */
int32_t   svh_grid_footprint_cost(svh_grid* g, const int32_t* poses, int64_t n, int32_t on_device, int32_t* out);
/* the table of S x K x T poses (host memory), copied, and to the device once.  After SVH_ERR_HIP the table is set and the next
 * svh_grid_roll_score uploads it again */
int32_t   svh_grid_roll_set_candidates(svh_grid* g, const int32_t* table, int32_t S, int32_t K, int32_t T);
/* S, K and T of the table in force, (0, 0, 0) while there is none: what sizes the outputs of svh_grid_roll_score */
int32_t   svh_grid_roll_get_candidates(svh_grid* g, int32_t skt[3]);
/* scores set `set` at the cell of the map-frame position anchor_xyz: recs (5 K int32) and scores (K int64) on the host or
 * (on_device) in device memory, 4- and 8-byte aligned there; each may be NULL; *best (host memory) = index or -1.  An anchor outside
 * the window is no error: every candidate is cut at pose 0.  SVH_ERR_BAD_ARG: no candidates, no such set, an anchor with no cell */
int32_t   svh_grid_roll_score(svh_grid* g, const double anchor_xyz[3], int32_t set, int32_t* recs, int64_t* scores, int32_t on_device, int32_t* best);
/* svh_grid_render_cost with the reference cells of the poses before the cut of every candidate of the last svh_grid_roll_score drawn
 * (0, 192, 255) and those of its best (255, 255, 255) over them; they are global cells, those outside the window now are skipped.
 * SVH_ERR_BAD_ARG: nothing was scored since the tables were set, or the last scoring failed */
int32_t   svh_grid_render_roll(svh_grid* g, uint8_t* rgb, int32_t on_device);


typedef struct svh_grid_explore_params {
    float   range;             /* 10.0: metres a viewpoint sees; finite, > 0, R = floor(range / cell) in 1..128 */
    int32_t min_gain;          /* 1: a record with a smaller gain is infeasible; 0..2^26 */
    int32_t w_gain;            /* 500: weight of the gain in the score; 0..65535 */
    int32_t w_reach;           /* 1: weight of the reach in the score; 0..65535 */
} svh_grid_explore_params;

#define SVH_GRID_EXPLORE_RECORD 5      /* int32 per record: label, rep_ga, rep_gb, gain, reach */
#define SVH_GRID_VIEW_NONE     0       /* bytes of a VIEW plane */
#define SVH_GRID_VIEW_VISITED  1
#define SVH_GRID_VIEW_COUNTED  2

void      svh_grid_explore_params_default(svh_grid_explore_params* p);
/* SVH_ERR_BAD_ARG, nothing changed: a parameter out of its range, or R outside 1..128.  A grid is created with the defaults; if
 * their R does not fit the grid's cell the object exists, and svh_grid_view_gain, svh_grid_view_mask, svh_grid_explore_rank,
 * svh_grid_plan_set_goal_explore and svh_grid_render_view return SVH_ERR_BAD_ARG until this call succeeds */
int32_t   svh_grid_set_explore(svh_grid* g, const svh_grid_explore_params* p);
/* the parameters in force and their R (0 while the defaults do not fit); either output may be NULL, not both */
int32_t   svh_grid_get_explore(svh_grid* g, svh_grid_explore_params* p, int32_t* range_R);
/* GAIN of n viewpoints, global cells (ga, gb), n <= 2^26: cells and out both on the host or (on_device) both in device memory,
 * 4-byte aligned there.  Computed per call */
int32_t   svh_grid_view_gain(svh_grid* g, const int32_t* cells, int64_t n, int32_t on_device, int32_t* out);
/* the VIEW plane of the viewpoint (ga, gb), a global cell: nx * nz bytes laid out as the planes of svh_grid_get.
 * SVH_ERR_BAD_ARG: the viewpoint is outside the window */
int32_t   svh_grid_view_mask(svh_grid* g, int32_t ga, int32_t gb, uint8_t* out, int32_t on_device);
/* ranks the kept frontier components from the cell of the map-frame position start_xyz: *n = the records (the kept components,
 * at most 65536), the first min(*n, cap) records (5 int32 each) to recs and scores to scores (host memory; either may be NULL),
 * *best = index or -1.  A start outside the window or on an impassable cell is no error: every reach is SVH_GRID_PLAN_FAR and
 * *best is -1.  The planner's goals and field are not touched.  SVH_ERR_BAD_ARG: a start with no cell */
int32_t   svh_grid_explore_rank(svh_grid* g, const double start_xyz[3], int32_t* recs, int64_t* scores, int64_t cap, int64_t* n, int32_t* best);
/* ranks as above and makes the best record's representative the planner's only goal (svh_grid_plan_set_goals): returns 1, or 0
 * when there is no best, and then leaves the goals alone; a negative error */
int32_t   svh_grid_plan_set_goal_explore(svh_grid* g, const double start_xyz[3]);
/* out[0] records of the last ranking, out[1] feasible records of it, out[2] reach fields computed since create, out[3] kernel
 * launches of the last gain computation (svh_grid_view_gain or a ranking) */
int32_t   svh_grid_get_explore_stats(svh_grid* g, int64_t out[4]);
/* svh_grid_render_frontiers with the VIEW plane of the viewpoint (ga, gb) over it: counted cells (255, 0, 255), visited cells
 * brightened (c + (255 - c) / 2 per byte), the viewpoint (255, 255, 255).  SVH_ERR_BAD_ARG: the viewpoint is outside the window */
int32_t   svh_grid_render_view(svh_grid* g, int32_t ga, int32_t gb, uint8_t* rgb, int32_t on_device);

typedef struct svh_grid_align_params {
    float   reach;      /* 0.6: metres; the field is 0 beyond; ceil(reach / cell) in 1..32 */
    float   range;      /* 25.6: metres; half side of the box of scan subs about the pivot; floor(range / cell) in 1..256 */
    int32_t rot_den;    /* 256: D, 16..4096; rotation k is the direction (D, k) */
    int32_t rot_n;      /* 8: K, 0..32 */
    int32_t trans_n;    /* 8: W in subs (quarter cells), 0..32 */
    int32_t min_scan;   /* 32: fewer distinct scan subs than this -> SVH_GRID_ALIGN_FEW; >= 1 */
} svh_grid_align_params;

#define SVH_GRID_ALIGN_RECORD 8        /* int32 per record: status, k, ta, tb, score, identity score, n_scan, ties */
#define SVH_GRID_ALIGN_OK     0
#define SVH_GRID_ALIGN_FEW    1
#define SVH_GRID_ALIGN_FLAT   2

void      svh_grid_align_params_default(svh_grid_align_params* p);
/* SVH_ERR_BAD_ARG, nothing changed: a parameter out of its range for this grid's cell.  A grid is created WITHOUT align parameters:
 * every other align entry returns SVH_ERR_BAD_ARG until this call succeeds.  A success forgets the last alignment */
int32_t   svh_grid_set_align(svh_grid* g, const svh_grid_align_params* p);
/* the field F: nx * nz bytes laid out as the planes of svh_grid_get */
int32_t   svh_grid_get_align_field(svh_grid* g, uint8_t* out, int32_t on_device);
/* aligns n >= 0 points (x, y, z, val), on the host or (on_device, 16-byte aligned) in device memory, about the map-frame position
 * `pivot`: the record to rec (host memory).  Nothing is added to the grid */
int32_t   svh_grid_align_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device, const double pivot[3], int32_t rec[8]);
/* ... the points of n_lists lists of the view, from first_list on, as svh_grid_add_view_lists_from takes them */
int32_t   svh_grid_align_view_lists(svh_grid* g, svh_view* v, int32_t first_list, int32_t n_lists, const double pivot[3], int32_t rec[8]);
/* the volume of the last alignment, (2 K + 1) (2 W + 1)^2 int32 as [k + K][tb + W][ta + W]; SVH_ERR_BAD_ARG if there is none: no
 * alignment since svh_grid_set_align, the last one failed or was SVH_GRID_ALIGN_FEW */
int32_t   svh_grid_get_align_volume(svh_grid* g, int32_t* out, int32_t on_device);
/* the scan of the last alignment: *n = n_scan, the first min(*n, cap) pairs (ua, ub), ascending by (ub, ua), to subs (host memory) */
int32_t   svh_grid_get_align_scan(svh_grid* g, int32_t* subs, int64_t cap, int64_t* n);
/* M, 4 x 4 row major, of the candidate (k, ta, tb) of the parameters in force about `pivot` (CORRECTION above).  Needs no device */
int32_t   svh_grid_align_correction(svh_grid* g, int32_t k, int32_t ta, int32_t tb, const double pivot[3], double M[16]);
/* svh_grid_render_local with the last alignment over it: the cells of the scan at the identity (255, 224, 0), then the cells of the
 * scan placed at the best (0, 224, 255), then the pivot's cell (255, 255, 255); the later primitive wins */
int32_t   svh_grid_render_align(svh_grid* g, uint8_t* rgb, int32_t on_device);


typedef struct svh_grid_dyn_params {
    int32_t clear_frames;      /* 2: contradicting observations in a row that clear a cell; 0..65535, 0 = never */
    int32_t min_through;       /* 3: weight of through-lines that makes an observation contradict a cell; >= 1 */
    float   margin;            /* 0.1: how far below the stored top a line must pass; finite, 0 <= margin < 2^20 */
    int32_t max_age;           /* 0: observations without a point after which a cell is emptied; >= 0, 0 = never */
} svh_grid_dyn_params;

void      svh_grid_dyn_params_default(svh_grid_dyn_params* p);
/* sets the layer and allocates its planes.  SVH_ERR_BAD_ARG, nothing changed: a parameter out of its range.  A grid is created
 * WITHOUT the layer: the observe entries, svh_grid_get_dynamics, svh_grid_get_dyn and svh_grid_render_dyn return SVH_ERR_BAD_ARG until
 * this call succeeds.  New parameters keep CONTRA and LAST.  p == NULL drops the layer and frees its planes; setting it again
 * starts from empty planes (the stamp goes on).  After SVH_ERR_HIP the parameters are set and the planes are empty */
int32_t   svh_grid_set_dynamics(svh_grid* g, const svh_grid_dyn_params* p);
int32_t   svh_grid_get_dynamics(svh_grid* g, svh_grid_dyn_params* p);
/* one observation: the arguments and the origin rule of svh_grid_add_points_from.  n may be 0: a frame without points still
 * advances the stamp and ages.  SVH_ERR_BAD_ARG, before anything is read or changed: the origin is not a low point of the window,
 * the dynamics are not set, or the stamp has reached 2^31 - 1.  One host wait per call (a host array: one more per 2^22 points) */
int32_t   svh_grid_observe_points(svh_grid* g, const float* xyzv, int64_t n, int32_t on_device, const double origin[3]);
/* ... the points of n_lists lists of the view, from first_list on, as svh_grid_add_view_lists_from takes them */
int32_t   svh_grid_observe_view_lists(svh_grid* g, svh_view* v, int32_t first_list, int32_t n_lists, const double origin[3]);
/* planes of svh_grid_get_dyn, int32, laid out as those of svh_grid_get; a device array is 4-byte aligned */
#define SVH_GRID_DYN_AGE     0   /* stamp - LAST: observations since the cell last had a point of a frame; -1 where LAST is 0 */
#define SVH_GRID_DYN_CONTRA  1   /* contradicting observations in a row */
#define SVH_GRID_DYN_THROUGH 2   /* THROUGH of the last observation; 0 in strips that entered since */
int32_t   svh_grid_get_dyn(svh_grid* g, int32_t plane, void* out, int32_t on_device);
/* since the last clear: out[0] observations (the stamp), out[1] cells cleared, out[2] cells aged, out[3] frames x cells confirmed */
int32_t   svh_grid_get_dyn_stats(svh_grid* g, int64_t out[4]);
/* svh_grid_render_local; a cell with CONTRA > 0 is tinted (red and green bytes c + (255 - c) / 2), a cell that the last
 * observation cleared or aged is (255, 0, 255) */
int32_t   svh_grid_render_dyn(svh_grid* g, uint8_t* rgb, int32_t on_device);

#ifdef __cplusplus
}
#endif

#include "svh_grid_obj.h"   /* OBJECTS: obstacle components as things and their tracks from frame to frame */
#include "svh_grid_pred.h"  /* PREDICTION: the tracks carried ahead in time slots, and the rollouts scored against them */
#include "svh_grid_pose.h"  /* POSE PLANNING: cost-to-go and paths over cell x heading under the vehicle's footprint */
#include "svh_grid_archive.h"   /* ARCHIVE: cells that scroll out are kept and restored on return; planes over any box of global cells */
#include "svh_grid_time.h"  /* TIME: cost-to-go and paths over cell x time that wait for the predicted objects */
#endif

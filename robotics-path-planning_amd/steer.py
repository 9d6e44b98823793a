"""Batched Dubins / Reeds-Shepp curves between pose pairs, and LQR rollouts between point pairs, on the GPU, without a
planner around them.

    bs = BatchSteer("dubins")                       # or "rs"
    res = bs.plan(starts, goals, curvature)         # (n, 3) poses each; res.path(i) = the reference's five-tuple
    cost = bs.plan(starts, goals, 1.0, points=False, product=True).length_matrix()   # (ns, ng) lengths
    res = bs.plan(starts, goals, 1.0, points=False, product=True, obstacle_list=circles, robot_radius=0.3)
    cost = res.length_matrix(free_only=True)        # +inf where the curve touches a circle; res.hit says which one

obstacle_list: rows (x, y, size), any number of them; the test is the pose planners' check_collision (rrt_05 :1625,
rrt_06 :1749) on the curve's own points, made in the kernel that computes them.

Every double is what the reference's plan_dubins_path (10_path_planning_00_dubins_path.py :109) /
reeds_shepp_path_planning (10_path_planning_00_reeds_shepp_path.py :506) returns for that pair, bit for bit.  There is no
CPU fallback: without a device the call raises RrtxError.

    cands = bs.candidates(starts, goals, curvature, obstacle_list=circles)   # "dubins" / "rs": EVERY candidate curve of
                                                    # every pair, CSR: cands.of(i), cands.paths(i) = calc_paths' list
    res = bs.plan_free(starts, goals, curvature, obstacle_list=circles)      # plan(), but the shortest candidate that
                                                    # touches no circle (plan()'s row where none is free); res.rank, res.n_free

    bs = BatchSteer("lqr")                          # rows (x, y); no curvature
    res = bs.plan(starts, goals)                    # rrt_09's edges: res.path(i) = sample_path's (px, py, course_lens),
                                                    # res.end[i] = (px[-1], py[-1]), res.length[i] = sum(course_lens)
    rx, ry = bs.plan(starts, goals, resample=False).path(i)    # LQRPlanner.lqr_planning's rollout itself
    cost = bs.plan(starts, goals, points=False, product=True, obstacle_list=circles).length_matrix(free_only=True)

    bs = BatchSteer("bezier")                       # rows (x, y, yaw); no curvature argument: a Bezier curve has no bound
    res = bs.plan(starts, goals, offset=3.0)        # res.path(i) = calc_4points_bezier_path's (path, control_points)
    x, y, yaw, k = res.course(i)                    # res.kmax[i] = max |k|; BatchTrack().run(res) drives the courses
    cost = bs.plan(starts, goals, points=False, product=True, obstacle_list=circles).length_matrix(
        free_only=True, max_curvature=0.5)          # +inf where the curve touches a circle or bends harder than 0.5
    res = bs.plan_control_points(cps, n_points=50)  # calc_bezier_path for (n, m, 2) control points, 3 <= m <= 16

"bezier" is 10_path_planning_00_bazier_path.py: control points, points, bezier() on the derivative control points and
curvature() are the script's doubles, bit for bit.  yaw (atan2 of the first derivative), length (the left-to-right sum of
math.hypot over consecutive points) and kmax are this package's own definitions: the script returns none of them.

"lqr" is LQRPlanner.lqr_planning (10_path_planning_00_lqr_path.py :24-66 = rrt_09 :944-986) for the reference's model
(DT = 0.1, Q = R = I), with rrt_09's sample_path :1157-1172, edge cost (steer :1189, calc_new_cost :1432-1442) and
check_collision :1292-1305 around it; max_time and goal_dist are the planner's MAX_TIME and GOAL_DIST.
"""
import math

import numpy as np

from . import _abi

KINDS = {"dubins": _abi.STEER_DUBINS, "rs": _abi.STEER_RS, "reeds_shepp": _abi.STEER_RS, "lqr": _abi.STEER_LQR,
         "bezier": _abi.STEER_BEZIER}
DEFAULT_STEP = {_abi.STEER_DUBINS: 0.1, _abi.STEER_RS: 0.2, _abi.STEER_LQR: 0.2}   # LQR: rrt_09's step_size (:1063)


def word_order(selected_types):
    """plan_dubins_path's selected_types (names, in order) as word indices; a repeated name cannot change the result
    (the first of equal lengths wins), so only its first occurrence is kept.  KeyError for an unknown name, as
    _PATH_TYPE_MAP[ptype] raises it."""
    if selected_types is None:
        return None
    idx = []
    for name in selected_types:
        if name not in _abi.DUBINS_WORDS:
            raise KeyError(name)
        k = _abi.DUBINS_WORDS.index(name)
        if k not in idx:
            idx.append(k)
    return idx


def word_list(selected_types):
    """selected_types as word indices with every entry kept: in BatchSteer.candidates a repeated name is a candidate of its
    own.  None: the six words in DUBINS_WORDS order."""
    if selected_types is None:
        return None
    for name in selected_types:
        if name not in _abi.DUBINS_WORDS:
            raise KeyError(name)
    return [_abi.DUBINS_WORDS.index(name) for name in selected_types]


class Path:
    """The reeds_shepp_path script's Path container (10_path_planning_00_reeds_shepp_path.py :101-115), as calc_paths
    leaves it: lengths and L divided by the curvature."""

    def __init__(self):
        self.lengths = []
        self.ctypes = []
        self.L = 0.0
        self.x = []
        self.y = []
        self.yaw = []
        self.directions = []


class SteerCandidates:
    """Every candidate curve of a batch, CSR twice.  Per pair: status (n,) STEER_*, n_candidates (n,), cand_offsets
    (n + 1,) int64 -- of(i) is pair i's candidate range; a pair whose status is not STEER_OK has none.  Per candidate, in
    the reference's list order: pair; variant ("rs": 4 * word family + symmetry of generate_path, 0..47; "dubins": the
    position in the word list); modes (list of strings), n_seg, seg_len (m, 5), length (the column SteerResult.length
    holds); key, what the kind's planner minimises ("rs": Path.L; "dubins": the cost plan_dubins_path compares, in
    curvature units); hit (m,) int32 with an obstacle list (-1 free, else the lowest obstacle index touched), else None.
    Per point, with points=True: offsets (m + 1,) int64 over candidates, x, y, yaw and directions (int8, +1 / -1: "rs"
    Path.directions, "dubins" all +1); else None."""

    def __init__(self, kind, summary, pts, shape, rc, kernel_ms):
        self.kind = kind
        for k in ("status", "cand_offsets", "pair", "variant", "n_seg", "seg_len", "length", "key", "hit", "offsets"):
            setattr(self, k, summary[k])
        self.n_candidates = np.diff(self.cand_offsets).astype(np.int32)
        self.modes = [m.decode() for m in summary["modes"]]
        self.x, self.y, self.yaw, self.directions = pts if pts is not None else (None,) * 4
        self.shape = shape
        self.rc = rc
        self.kernel_ms = kernel_ms
        self.obstacle_index = None   # with an obstacle list: what tested it (BatchSteer's obstacle_index), a dict

    def __len__(self):
        return len(self.status)

    def of(self, i):
        """range of the candidate indices of pair i"""
        return range(int(self.cand_offsets[i]), int(self.cand_offsets[i + 1]))

    @property
    def free(self):
        """Boolean mask over candidates: the curve touches no obstacle."""
        if self.hit is None:
            raise _abi.RrtxError("free: these candidates were solved without an obstacle list")
        return self.hit == -1

    def paths(self, i):
        """"rs": what calc_paths returns for pair i -- a list of Path objects (lengths, ctypes, L, x, y, yaw, directions as
        Python lists and floats), [] where it returns []; raises where it raises.  "dubins": the list of
        plan_dubins_path(..., selected_types=[w]) five-tuples of the feasible list entries."""
        st = int(self.status[i])
        if st == _abi.STEER_RAISES_ZERODIV:
            raise ZeroDivisionError("float division by zero")
        if st == _abi.STEER_RAISES_VALUE:
            raise ValueError("math domain error")
        if self.x is None:
            raise _abi.RrtxError("paths(): these candidates were solved with points=False")
        out = []
        for c in self.of(i):
            a, b = int(self.offsets[c]), int(self.offsets[c + 1])
            modes = list(self.modes[c])
            lengths = [float(v) for v in self.seg_len[c, :self.n_seg[c]]]
            if self.kind == _abi.STEER_DUBINS:
                out.append((self.x[a:b].copy(), self.y[a:b].copy(), self.yaw[a:b].copy(), modes, lengths))
                continue
            p = Path()
            p.lengths, p.ctypes, p.L = lengths, modes, float(self.key[c])
            p.x, p.y, p.yaw = self.x[a:b].tolist(), self.y[a:b].tolist(), self.yaw[a:b].tolist()
            p.directions = self.directions[a:b].tolist()
            out.append(p)
        return out


class SteerResult:
    """One solved batch.  status (n,) STEER_*; length (n,): the absolute segment lengths added up; modes: list of n strings; lengths: list of n arrays of segment
    lengths; offsets (n + 1,) and the flat x, y, yaw when points were asked for, else None; hit (n,) int32 when the batch
    was planned with an obstacle list (-1 free, j >= 0 the first obstacle of the list the curve touches, -2 no curve),
    else None.
    An "lqr" batch: n_seg is the number of rollout points len(rx), end (n, 2) the last point, length the sum of
    math.hypot over consecutive points, left to right -- of the resampled points (rrt_09's edge cost), or with
    resample=False of the rollout points (the lqr_path script returns no length: this one is this package's definition);
    yaw is None, modes and lengths are empty.
    A "bezier" batch: every status is STEER_OK and every curve has n_points points; n_seg is the number of control points,
    control_points (n, m, 2) what the device computed from the poses (or was given); k the flat curvature per point and
    kmax (n,) the largest |k| per curve (NaN if any k is NaN) when curvature was asked for, else None.  yaw, length and
    kmax are this package's definitions (the bazier_path script returns none of them): yaw = atan2(dy, dx) of the first
    derivative, length the left-to-right sum of math.hypot over consecutive points.  modes and lengths are empty.
    A batch of BatchSteer.plan_free has three more (n,) int32 columns (None otherwise): rank, the position of the chosen
    candidate among the pair's candidates ordered by the kind's ranking key (0: plan()'s curve); n_candidates; n_free."""

    def __init__(self, kind, status, length, nseg, seglen, modes, offsets, xyz, shape, rc, kernel_ms, hit=None, end=None,
                 resampled=True, k=None, kmax=None, control_points=None):
        self.kind = kind
        self.status = status
        self.length = length
        self.n_seg = nseg
        self.seg_len = seglen
        if kind == _abi.STEER_BEZIER:   # neither modes nor segment lengths: no loop over what can be 2^20 curves
            self.modes = [""] * len(nseg)
            self.lengths = [seglen[:0, 0]] * len(nseg)
        else:
            self.modes = [m.decode() for m in modes]
            nl = np.zeros_like(nseg) if kind == _abi.STEER_LQR else nseg   # a rollout has no segment lengths
            self.lengths = [seglen[i, :nl[i]].copy() for i in range(len(nseg))]
        self.offsets = offsets
        self.x, self.y, self.yaw = xyz if xyz is not None else (None, None, None)
        self.shape = shape          # (ns, ng) in product mode, else None
        self.rc = rc                # 0 or RRTX_PARTIAL
        self.kernel_ms = kernel_ms
        self.hit = hit
        self.end = end              # "lqr": (n, 2); else None
        self.resampled = resampled  # "lqr": path(i) is sample_path's triple, not the rollout
        self.k = k                  # "bezier": flat curvature per point, or None
        self.kmax = kmax            # "bezier": (n,), or None
        self.control_points = control_points   # "bezier": (n, m, 2)
        self.rank = self.n_candidates = self.n_free = None   # plan_free()
        self.device_courses = None   # points="device": an _abi.DeviceCourses, and x, y, yaw are None
        self.obstacle_index = None   # with an obstacle list: what tested it (BatchSteer's obstacle_index), a dict

    @property
    def free(self):
        """Boolean mask of the pairs whose curve touches no obstacle (hit == -1); a pair without a curve is not free."""
        if self.hit is None:
            raise _abi.RrtxError("free: this batch was planned without an obstacle list")
        return self.hit == -1

    def is_free(self, i):
        """What the reference's check_collision(node, obstacle_list, robot_radius) returns for pair i's curve; raises what
        path(i) raises where the pair has no curve."""
        if self.hit is None:
            raise _abi.RrtxError("is_free(): this batch was planned without an obstacle list")
        st = int(self.status[i])
        if st == _abi.STEER_RAISES_ZERODIV:
            raise ZeroDivisionError("float division by zero")
        if st == _abi.STEER_RAISES_VALUE:
            raise ValueError("math domain error")
        if st == _abi.STEER_NO_PATH:
            if self.kind == _abi.STEER_DUBINS:
                raise TypeError("'NoneType' object is not iterable")
            if self.kind == _abi.STEER_LQR:   # rrt_09's steer fails at px[-1] (:1185) before any check
                raise IndexError("list index out of range")
            return False   # Reeds-Shepp: path(i) is (None,) * 5, and check_collision(None, ...) is False (:1751)
        return bool(self.hit[i] == -1)

    def __len__(self):
        return len(self.status)

    def path(self, i):
        """What the reference function returns for pair i: (x, y, yaw, modes, lengths) -- numpy arrays and lists for
        Dubins, lists for Reeds-Shepp, (None,) * 5 where Reeds-Shepp finds no path; raises where the reference raises.
        "lqr": sample_path's (px, py, course_lens) as lists, or with resample=False lqr_planning's (rx, ry); empty lists
        where the rollout never arrives.
        "bezier": calc_4points_bezier_path's (path (n_points, 2) array, control_points (m, 2) array)."""
        st = int(self.status[i])
        if self.kind == _abi.STEER_LQR:
            return self._lqr_path(i, st)
        if self.kind == _abi.STEER_BEZIER:
            if self.x is None:
                raise _abi.RrtxError("path(): this batch was solved with points=False")
            a, b = int(self.offsets[i]), int(self.offsets[i + 1])
            return np.stack([self.x[a:b], self.y[a:b]], axis=1), self.control_points[i].copy()
        if st == _abi.STEER_RAISES_ZERODIV:
            raise ZeroDivisionError("float division by zero")
        if st == _abi.STEER_RAISES_VALUE:
            raise ValueError("math domain error")
        if st == _abi.STEER_NO_PATH:
            if self.kind == _abi.STEER_DUBINS:   # b_mode stays None and _generate_local_course zips over it
                raise TypeError("'NoneType' object is not iterable")
            return None, None, None, None, None
        if self.x is None:
            raise _abi.RrtxError("path(): this batch was solved with points=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        modes = list(self.modes[i])
        lengths = [float(v) for v in self.lengths[i]]
        if self.kind == _abi.STEER_DUBINS:
            return self.x[a:b].copy(), self.y[a:b].copy(), self.yaw[a:b].copy(), modes, lengths
        return self.x[a:b].tolist(), self.y[a:b].tolist(), self.yaw[a:b].tolist(), modes, lengths

    def _lqr_path(self, i, st):
        if st == _abi.STEER_NO_PATH:
            return ([], [], []) if self.resampled else ([], [])
        if self.x is None:
            raise _abi.RrtxError("path(): this batch was solved with points=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        px, py = self.x[a:b].tolist(), self.y[a:b].tolist()
        if not self.resampled:
            return px, py
        dx, dy = np.diff(px), np.diff(py)   # :1167-1170, on the host as the reference does it
        return px, py, [math.hypot(idx, idy) for (idx, idy) in zip(dx, dy)]

    def course(self, i):
        """"bezier": (x, y, yaw, k) arrays of curve i; k is None when curvature was not asked for."""
        if self.kind != _abi.STEER_BEZIER:
            raise _abi.RrtxError("course(): a Bezier batch has courses; use path(i)")
        if self.x is None:
            raise _abi.RrtxError("course(): this batch was solved with points=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return (self.x[a:b].copy(), self.y[a:b].copy(), self.yaw[a:b].copy(),
                None if self.k is None else self.k[a:b].copy())

    def length_matrix(self, free_only=False, max_curvature=None):
        """The (ns, ng) lengths of a product-mode batch; free_only: +inf where the pair is not free; max_curvature
        ("bezier"): +inf where kmax > max_curvature or kmax is NaN."""
        if self.shape is None:
            raise _abi.RrtxError("length_matrix(): this batch was not solved in product mode")
        cost = self.length
        if free_only:
            cost = np.where(self.free, cost, np.inf)
        if max_curvature is not None:
            if self.kmax is None:
                raise _abi.RrtxError("length_matrix(): max_curvature needs a Bezier batch planned with curvature=True")
            cost = np.where(self.kmax <= max_curvature, cost, np.inf)   # a NaN compares False
        return cost.reshape(self.shape)


class BatchSteer:
    """Shortest Dubins ("dubins") or Reeds-Shepp ("rs") curves or Bezier curves ("bezier") for batches of pose pairs, or
    LQR rollouts ("lqr") for batches of point pairs; device buffers are kept between calls of plan()."""

    def __init__(self, kind, device=0, obstacle_index=None):
        """obstacle_index: how a list of circles is tested -- None: through the obstacle index (a grid over the list, a
        point reads its own cell) when the list has more than 256 circles, True: always, False: never (every point against
        every circle).  hit is the same either way; also a settable attribute.  result.obstacle_index says what served a
        batch: {"mode", "used", "reason", and the grid's fields}, or None without a list."""
        if kind not in KINDS:
            raise ValueError("BatchSteer: kind is 'dubins', 'rs', 'lqr' or 'bezier', not %r" % (kind,))
        _abi.obstacle_index_mode(obstacle_index)   # a ValueError comes before any device call
        self.kind = KINDS[kind]
        self._steer = _abi.Steer(device)
        self.obstacle_index = obstacle_index

    @property
    def obstacle_index(self):
        return self._obstacle_index

    @obstacle_index.setter
    def obstacle_index(self, v):
        _abi.obstacle_index_mode(v)
        self._steer.set_obstacle_index(v)
        self._obstacle_index = v

    def close(self):
        self._steer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def plan(self, starts, goals, curvature=None, step_size=None, selected_types=None, points=True, product=False,
             obstacle_list=None, robot_radius=0.0, resample=True, max_time=100.0, goal_dist=0.1, offset=3.0, n_points=100):
        """starts, goals: (n, 3) rows of (x, y, yaw) -- with product=True (ns, 3) and (ng, 3), pair p = (p // ng, p % ng).
        curvature: a float or one per pair.  step_size: Reeds-Shepp any value > 0 (default 0.2); Dubins 0.1 only.
        selected_types (Dubins): word names in the order to try them.  obstacle_list: rows (x, y, size) every curve is
        tested against with robot_radius (result.hit / .free); None or empty: no check.
        "lqr": rows are (x, y); curvature and selected_types must stay None; step_size >= 1e-3 (default rrt_09's 0.2) is
        sample_path's step, resample=False gives the rollout itself; max_time <= 100.0 and goal_dist are the planner's
        MAX_TIME and GOAL_DIST (these three keywords belong to this kind alone).
        "bezier": plan(starts, goals, offset=3.0, n_points=100, curvature=True, points=True, product=False,
        obstacle_list=None, robot_radius=0.0) -- offset is calc_4points_bezier_path's, a float or one per pair; n_points
        (2..4096) the points per curve; curvature is a flag here (default True): k per point and kmax per curve."""
        if _abi.on_device(points) and self.kind == _abi.STEER_LQR:
            raise ValueError("BatchSteer('lqr').plan: points='device' is for courses of (x, y, yaw), a rollout has no yaw")
        if self.kind == _abi.STEER_BEZIER:
            if step_size is not None or selected_types is not None or resample is not True or max_time != 100.0 \
                    or goal_dist != 0.1:
                raise ValueError("BatchSteer('bezier').plan: takes offset, n_points, curvature, points, product, "
                                 "obstacle_list and robot_radius")
            if curvature is not None and not isinstance(curvature, (bool, np.bool_)):
                if offset != 3.0:   # the third positional argument of this kind is the offset
                    raise ValueError("BatchSteer('bezier').plan: two offsets (curvature is a flag for this kind)")
                offset, curvature = curvature, True
            return self._plan_bezier(starts, goals, None, offset, n_points, True if curvature is None else curvature,
                                     points, product, obstacle_list, robot_radius)
        if offset != 3.0 or n_points != 100:
            raise ValueError("BatchSteer.plan: offset and n_points belong to kind 'bezier'")
        if step_size is None:
            step_size = DEFAULT_STEP[self.kind]
        if self.kind == _abi.STEER_LQR:
            return self._plan_lqr(starts, goals, curvature, step_size, selected_types, points, product, obstacle_list,
                                  robot_radius, resample, max_time, goal_dist)
        if curvature is None:
            raise TypeError("BatchSteer.plan: curvature is required for Dubins and Reeds-Shepp curves")
        if resample is not True or max_time != 100.0 or goal_dist != 0.1:
            raise ValueError("BatchSteer.plan: resample, max_time and goal_dist belong to kind 'lqr'")
        wo = word_order(selected_types)
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        S = self._steer
        ob = self._set_obstacles(obstacle_list, robot_radius)   # (nothing to clear when no list was ever set)
        rc = S.solve(self.kind, st, go, curvature, step_size, word_order=wo, points=points, product=product)
        status, length, nseg, seglen, modes, off = S.summary(offsets=bool(points))
        xyz = S.points() if points and not _abi.on_device(points) else None
        res = SteerResult(self.kind, status, length, nseg, seglen, modes, off, xyz,
                          (len(st), len(go)) if product else None, rc, S.kernel_ms(), hit=S.hits() if len(ob) else None)
        if _abi.on_device(points):
            res.device_courses = _abi.DeviceCourses(_abi.SRC_STEER, S)
        return self._served(res, ob)

    def _solve_all(self, what, starts, goals, curvature, step_size, selected_types, points, product, obstacle_list,
                   robot_radius):
        """plan()'s checks and defaults for the two curve kinds, then rrtx_steer_solve_all: (rc, shape, obstacle rows)."""
        if self.kind not in (_abi.STEER_DUBINS, _abi.STEER_RS):
            raise ValueError("BatchSteer.%s belongs to the kinds 'dubins' and 'rs'" % what)
        if curvature is None:
            raise TypeError("BatchSteer.%s: curvature is required" % what)
        if step_size is None:
            step_size = DEFAULT_STEP[self.kind]
        wl = word_list(selected_types)
        if wl is not None and len(wl) > 16:
            raise ValueError("BatchSteer.%s: at most 16 entries in selected_types" % what)
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        ob = self._set_obstacles(obstacle_list, robot_radius)
        rc = self._steer.solve_all(self.kind, st, go, curvature, step_size, word_order=wl, points=points, product=product)
        return rc, ((len(st), len(go)) if product else None), ob

    def candidates(self, starts, goals, curvature, step_size=None, selected_types=None, points=True, product=False,
                   obstacle_list=None, robot_radius=0.0):
        """Every candidate curve of every pair ("rs": calc_paths' list; "dubins": one per feasible entry of the word list,
        a repeated word repeated), arguments as plan(): a SteerCandidates."""
        if _abi.on_device(points):
            raise ValueError("BatchSteer.candidates: points='device' is not supported, only the chosen curves of plan_free "
                             "are a source of courses")
        rc, shape, ob = self._solve_all("candidates", starts, goals, curvature, step_size, selected_types, points, product,
                                        obstacle_list, robot_radius)
        S = self._steer
        summary = S.cand_summary(hits=len(ob) > 0, offsets=bool(points))
        return self._served(SteerCandidates(self.kind, summary, S.cand_points() if points else None, shape, rc,
                                            S.cand_counts()[3]), ob)

    def plan_free(self, starts, goals, curvature, step_size=None, selected_types=None, points=True, product=False,
                  obstacle_list=None, robot_radius=0.0):
        """As plan(obstacle_list=...), but every row is the shortest candidate curve that touches no obstacle -- smallest
        by the key plan() minimises, the first in list order among equal keys; where no candidate is free (or the pair has
        none) the row is plan()'s.  The SteerResult has rank, n_candidates and n_free beside plan()'s columns."""
        if obstacle_list is None or len(np.asarray(obstacle_list).reshape(-1)) == 0:
            raise ValueError("BatchSteer.plan_free: an obstacle list is required")
        rc, shape, ob = self._solve_all("plan_free", starts, goals, curvature, step_size, selected_types, points, product,
                                       obstacle_list, robot_radius)
        S = self._steer
        rc, _, rank, n_free = S.select_free()
        status, length, nseg, seglen, modes, off = S.summary(offsets=bool(points))
        res = SteerResult(self.kind, status, length, nseg, seglen, modes, off,
                          S.points() if points and not _abi.on_device(points) else None, shape, rc, S.kernel_ms(), hit=S.hits())
        if _abi.on_device(points):
            res.device_courses = _abi.DeviceCourses(_abi.SRC_STEER, S)
        res.rank, res.n_free = rank, n_free
        res.n_candidates = np.diff(S.cand_offsets()).astype(np.int32)
        return self._served(res, ob)

    def plan_control_points(self, control_points, n_points=100, curvature=True, points=True, obstacle_list=None,
                            robot_radius=0.0):
        """"bezier": calc_bezier_path for a batch of control-point sets (n, m, 2) -- or one (m, 2) -- with 3 <= m <= 16."""
        if self.kind != _abi.STEER_BEZIER:
            raise ValueError("BatchSteer.plan_control_points belongs to kind 'bezier'")
        return self._plan_bezier(None, None, control_points, None, n_points, curvature, points, False, obstacle_list,
                                 robot_radius)

    def _plan_bezier(self, starts, goals, cps, offset, n_points, curvature, points, product, obstacle_list, robot_radius):
        S = self._steer
        ob = self._set_obstacles(obstacle_list, robot_radius)
        shape = None
        if cps is not None:
            rc = S.solve_bezier_cp(cps, n_points, points=points, curvature=curvature)
        else:
            st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
            go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
            rc = S.solve_bezier(st, go, offset, n_points, points=points, curvature=curvature, product=product)
            shape = (len(st), len(go)) if product else None
        status, length, nseg, seglen, modes, off = S.summary(offsets=bool(points))
        fetch = points and not _abi.on_device(points)
        xyz = S.points() if fetch else None
        res = SteerResult(self.kind, status, length, nseg, seglen, modes, off, xyz, shape, rc, S.kernel_ms(),
                          hit=S.hits() if len(ob) else None, k=S.curvature() if fetch and curvature else None,
                          kmax=S.kmax() if curvature else None, control_points=S.control_points())
        if _abi.on_device(points):
            res.device_courses = _abi.DeviceCourses(_abi.SRC_STEER, S)
        return self._served(res, ob)

    def _set_obstacles(self, obstacle_list, robot_radius):
        S = self._steer
        ob = np.zeros((0, 3)) if obstacle_list is None else np.asarray(obstacle_list, dtype=np.float64).reshape(-1, 3)
        if len(ob) or S.n_obstacles:
            S.set_obstacles(ob, robot_radius)
        return ob

    def _served(self, res, ob):
        """res with the obstacle index info of the list it was tested against"""
        info = getattr(self._steer, "obstacle_index_info", None)   # (a stand-in for _abi.Steer may have none)
        res.obstacle_index = info() if len(ob) and info else None
        return res

    def _plan_lqr(self, starts, goals, curvature, step_size, selected_types, points, product, obstacle_list, robot_radius,
                  resample, max_time, goal_dist):
        if curvature is not None or selected_types is not None:
            raise ValueError("BatchSteer('lqr').plan: an LQR rollout has no curvature and no selected_types")
        if resample and not float(step_size) > 0.0:
            raise ValueError("BatchSteer('lqr').plan: step_size must be > 0 (resample=False gives the raw rollout)")
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        go = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        S = self._steer
        ob = self._set_obstacles(obstacle_list, robot_radius)
        rc = S.solve_lqr(st, go, step_size if resample else 0.0, max_time, goal_dist, points=points, product=product)
        status, length, nseg, seglen, modes, off = S.summary(offsets=bool(points))
        xyz = S.points(yaw=False) if points else None
        return self._served(SteerResult(self.kind, status, length, nseg, seglen, modes, off, xyz,
                                        (len(st), len(go)) if product else None, rc, S.kernel_ms(),
                                        hit=S.hits() if len(ob) else None, end=S.ends(), resampled=bool(resample)), ob)

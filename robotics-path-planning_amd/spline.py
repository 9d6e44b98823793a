"""Batched cubic-spline courses through waypoints on the GPU: the step between a path and a course.

    bs = BatchSpline()
    res = bs.run(paths, ds=0.1)                 # paths: planner paths, path_smoothing's output, any (x, y) polylines
    rx, ry, ryaw, rk, s = res.course(i)         # what calc_spline_course(x_i, y_i, ds) returns
    tracked = BatchTrack().run(res)             # a SplineResult is a batch of (x, y, yaw) courses

For every course: what the reference's calc_spline_course (10_path_planning_00_cubic_spline_path.py :313-325) returns -- a
natural cubic spline over the chord length, sampled every ds.  Point counts, offsets and s are the reference's bit for bit
in every mode.  The spline coefficient c, which the reference takes from np.linalg.solve, comes from one of three places:

    solve="device"  (default) the Thomas recurrence of csrc/rpp_spline.h on the device: this package's own definition of c,
                    bit-identical to tests/spline_oracle.py; x, y, yaw, k agree with the reference to rounding
    solve="numpy"   the host builds A and B and calls np.linalg.solve per course exactly as the reference does, and hands c
                    down: bit-identical to the reference running on this host.  Slow (one dense solve per course and axis).
    c=(cx, cy)      c as data, flat over all waypoints (e.g. a recorded sx.c, sy.c): x, y, yaw, k are the reference's doubles

The fitted splines stay on the device and answer at parameters of the caller's choosing -- the pointwise methods of the
reference's classes (CubicSpline2D.calc_position / calc_yaw / calc_curvature :248-310, CubicSpline1D.calc_position /
calc_first_derivative / calc_second_derivative :75-140), one kernel lane per query:

    bs.fit(paths)                               # or run(...): the splines of the last of them answer
    q = bs.query(s_of_my_controller)            # one array for every course, a list per course, or CSR (offsets, t)
    q.x, q.y, q.yaw, q.k, q.status              # flat over the queries; q.of(i): the slices of course i
    bs.fit1d(knots, values)                     # CubicSpline1D over the caller's knots; query() then gives y (dy, ddy)

A query outside the knots (the reference returns None), on the last knot or NaN (the reference raises IndexError) or of a
course without a spline is NaN in every plane and says so in status (SPLINE_Q_*).

There is no CPU fallback: without a device BatchSpline raises RrtxError.
"""
import numpy as np

from . import _abi


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _csr(waypoints):
    """(offsets, x, y) of `waypoints`: a CSR tuple (offsets, x, y), a list of (n_i, 2) arrays, or a list of (x, y) pairs of
    sequences.  In a list, a two-dimensional ndarray is taken as rows (x, y); anything else as a pair (x, y)."""
    if (isinstance(waypoints, tuple) and len(waypoints) == 3 and all(np.ndim(w) == 1 for w in waypoints)
            and np.issubdtype(np.asarray(waypoints[0]).dtype, np.integer)):
        off = np.ascontiguousarray(waypoints[0], dtype=np.int64)
        x, y = _f64(waypoints[1]).reshape(-1), _f64(waypoints[2]).reshape(-1)
    else:
        xs, ys = [], []
        for i, w in enumerate(waypoints):
            if isinstance(w, np.ndarray) and w.ndim == 2:
                if w.shape[1] != 2:
                    raise ValueError("BatchSpline: course %d is an array of shape %s, expected (n, 2)" % (i, w.shape))
                cx, cy = _f64(w[:, 0]), _f64(w[:, 1])
            else:
                if len(w) != 2:
                    raise ValueError("BatchSpline: course %d is neither an (n, 2) array nor a pair (x, y)" % i)
                cx, cy = _f64(w[0]).reshape(-1), _f64(w[1]).reshape(-1)
            if len(cx) != len(cy):
                raise ValueError("BatchSpline: x and y of course %d differ in length" % i)
            xs.append(cx)
            ys.append(cy)
        off = np.zeros(len(xs) + 1, dtype=np.int64)
        if xs:
            off[1:] = np.cumsum([len(c) for c in xs])
        x = _f64(np.concatenate(xs)) if xs else np.zeros(0)
        y = _f64(np.concatenate(ys)) if ys else np.zeros(0)
    if len(off) < 1 or len(x) != len(y) or off[-1] != len(x):
        raise ValueError("BatchSpline: the offsets do not describe the waypoint arrays")
    return off, x, y


def _csr1(seqs):
    """(offsets, flat) of `seqs`: a CSR tuple (offsets, flat), a list of one sequence per spline, or one sequence of
    numbers (a batch of one)."""
    if (isinstance(seqs, tuple) and len(seqs) == 2 and np.ndim(seqs[0]) == 1 and np.ndim(seqs[1]) == 1
            and np.issubdtype(np.asarray(seqs[0]).dtype, np.integer) and len(seqs[0]) >= 1
            and int(np.asarray(seqs[0])[-1]) == len(seqs[1])):
        return np.ascontiguousarray(seqs[0], dtype=np.int64), _f64(seqs[1]).reshape(-1)
    if len(seqs) and all(np.ndim(v) == 0 for v in seqs):
        seqs = [seqs]
    rows = [_f64(v).reshape(-1) for v in seqs]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    return off, (_f64(np.concatenate(rows)) if rows else np.zeros(0))


def solve_numpy_1d(knots, values):
    """c of one CubicSpline1D(knots, values) as the reference makes it on this host: h = np.diff(x) (:50), A and B
    (:148-173), np.linalg.solve (:65)."""
    return _solve_numpy(np.diff(knots), [[float(v) for v in values]])[0]


def solve_numpy(x, y):
    """(cx, cy) of one course as the reference makes them on this host: s of CubicSpline2D.__calc_s (:240-246), A and B of
    CubicSpline1D (:148-173), np.linalg.solve (:65)."""
    s = [0]
    s.extend(np.cumsum(np.hypot(np.diff(x), np.diff(y))))
    out = _solve_numpy(np.diff(s), ([float(v) for v in x], [float(v) for v in y]))
    return out[0], out[1]


def _solve_numpy(h, axes):
    nx = len(h) + 1
    A = np.zeros((nx, nx))
    A[0, 0] = 1.0
    for i in range(nx - 1):
        if i != (nx - 2):
            A[i + 1, i + 1] = 2.0 * (h[i] + h[i + 1])
        A[i + 1, i] = h[i]
        A[i, i + 1] = h[i]
    A[0, 1] = 0.0
    A[nx - 1, nx - 2] = 0.0
    A[nx - 1, nx - 1] = 1.0
    out = []
    for a in axes:
        B = np.zeros(nx)
        for i in range(nx - 2):
            B[i + 1] = 3.0 * (a[i + 2] - a[i + 1]) / h[i + 1] - 3.0 * (a[i + 1] - a[i]) / h[i]
        out.append(np.linalg.solve(A, B))
    return out


def pack_batch(waypoints, ds=0.1, c=None, obstacle_list=None, robot_radius=0.0, arrays=True):
    """The rrtx_spline_batch of one run: (batch, keep).  `keep` names the arrays the batch points into (they must outlive
    the call)."""
    off, x, y = _csr(waypoints)
    n = len(off) - 1
    if np.ndim(ds) == 0:
        dsa, per = _f64([float(ds)]), False
    else:
        dsa, per = _f64(ds).reshape(-1), True
        if len(dsa) != n:
            raise ValueError("BatchSpline: %d values of ds for %d courses" % (len(dsa), n))
    cx = cy = None
    if c is not None:
        cx, cy = _f64(c[0]).reshape(-1), _f64(c[1]).reshape(-1)
        if len(cx) != len(cy):
            raise ValueError("BatchSpline: cx and cy differ in length")
    obs = _f64([list(o) for o in obstacle_list]).reshape(-1, 3) if obstacle_list is not None and len(obstacle_list) else None
    keep = dict(offsets=off, x=x, y=y, ds=dsa, cx=cx, cy=cy, obstacles=obs)

    def ptr(a):
        return None if a is None else a.ctypes.data
    b = _abi.SplineBatch(n=n, offsets=ptr(off), x=ptr(x), y=ptr(y), ds=ptr(dsa), ds_per_course=int(per),
                         want_arrays=int(bool(arrays)), cx=ptr(cx), cy=ptr(cy), n_c=0 if cx is None else len(cx),
                         obstacles=ptr(obs), n_obstacles=0 if obs is None else len(obs), robot_radius=float(robot_radius))
    return b, keep


class SplineResult:
    """One batch of spline courses.  Per course: status (SPLINE_OK, SPLINE_DEGENERATE coinciding waypoints,
    SPLINE_REF_RAISES the reference raises IndexError), n_points, total_length (s[-1]); offsets (n + 1,) into the flat x, y,
    yaw, k, s (None when the run was made with arrays=False); c = (cx, cy) as used, flat over the waypoints (wp_offsets);
    hit (n,) int32 when the batch was run with an obstacle list (-1 free, j >= 0 the first circle of the list the course
    touches, -2 no points), else None; rc 0 or RRTX_PARTIAL; kernel_ms.
    offsets / x / y / yaw are what BatchTrack.run takes as a batch of courses."""

    def __init__(self, records, offsets, arrays, c, wp_offsets, hit=None, rc=0, kernel_ms=0.0):
        self.status = records["status"].copy()
        self.n_points = records["n_points"].copy()
        self.total_length = records["length"].copy()
        self.offsets = offsets
        self.x, self.y, self.yaw, self.k, self.s = arrays if arrays is not None else (None,) * 5
        self.device_courses = None   # arrays="device": an _abi.DeviceCourses, and the five arrays are None
        self.c = c
        self.wp_offsets = wp_offsets
        self.hit = hit
        self.obstacle_index = None   # with an obstacle list: what tested it (the obstacle_index keyword), a dict
        self.rc = rc
        self.kernel_ms = kernel_ms

    def __len__(self):
        return len(self.status)

    def _raise_for(self, i, who):
        st = int(self.status[i])
        if st == _abi.SPLINE_DEGENERATE:
            raise _abi.RrtxError("%s: course %d has two consecutive waypoints that coincide (the reference divides by zero)"
                                 % (who, i))
        if st == _abi.SPLINE_REF_RAISES:
            raise IndexError("list index out of range")   # self.b[i] at the last knot (:93)

    def course(self, i):
        """What calc_spline_course returns for course i: (rx, ry, ryaw, rk, s) as lists."""
        self._raise_for(i, "course()")
        if self.x is None:
            raise _abi.RrtxError("course(): this batch was run with arrays=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return tuple(q[a:b].tolist() for q in (self.x, self.y, self.yaw, self.k, self.s))

    @property
    def free(self):
        """Boolean mask of the courses that touch no obstacle (hit == -1); a course without points is not free."""
        if self.hit is None:
            raise _abi.RrtxError("free: this batch was run without an obstacle list")
        return self.hit == -1

    def is_free(self, i):
        """What the pose planners' check_collision returns for course i's points."""
        if self.hit is None:
            raise _abi.RrtxError("is_free(): this batch was run without an obstacle list")
        self._raise_for(i, "is_free()")
        return bool(self.hit[i] == -1)


class SplineQueryResult:
    """The answers of one BatchSpline.query, flat over the queries in the order given.  offsets (n + 1,) into them, one row
    per spline; s the parameters; status (Q,) int32 SPLINE_Q_OK / _OUTSIDE / _REF_RAISES / _NO_SPLINE.  After run() or fit():
    x, y, yaw, k and, with derivatives=True, dx, dy, ddx, ddy.  After fit1d(): y and, with derivatives=True, dy, ddy.  A plane
    that was not made is None; every value of a query whose status is not SPLINE_Q_OK is NaN.  rc 0 or RRTX_PARTIAL;
    kernel_ms the HIP-event time of the query kernel."""
    PLANES = ("x", "y", "yaw", "k", "dx", "dy", "ddx", "ddy")

    def __init__(self, offsets, s, status, planes, rc=0, kernel_ms=0.0):
        self.offsets = offsets
        self.s = s
        self.status = status
        for key in self.PLANES:
            setattr(self, key, planes.get(key))
        self.rc = rc
        self.kernel_ms = kernel_ms

    def __len__(self):
        return len(self.offsets) - 1

    @property
    def valid(self):
        """Boolean mask of the queries that were answered (status == SPLINE_Q_OK)"""
        return self.status == _abi.SPLINE_Q_OK

    def of(self, i):
        """The slices of spline i: a dict of s, status and every plane that was made"""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        out = dict(s=self.s[a:b], status=self.status[a:b])
        for key in self.PLANES:
            if getattr(self, key) is not None:
                out[key] = getattr(self, key)[a:b]
        return out


class BatchSpline:
    """Natural cubic splines through batches of waypoint lists, sampled every ds; device buffers are kept between calls of
    run().  The splines of the last run(), fit() or fit1d() answer query()."""

    def __init__(self, device=0, obstacle_index=None):
        """obstacle_index: None, True or False, as BatchSteer's (also a settable attribute); result.obstacle_index says what
        tested a run's obstacle list."""
        _abi.obstacle_index_mode(obstacle_index)   # a ValueError comes before any device call
        self._spline = _abi.Spline(device)
        self._n = None   # splines of the last completed run / fit / fit1d
        self.obstacle_index = obstacle_index

    @property
    def obstacle_index(self):
        return self._obstacle_index

    @obstacle_index.setter
    def obstacle_index(self, v):
        _abi.obstacle_index_mode(v)
        self._spline.set_obstacle_index(v)
        self._obstacle_index = v

    def close(self):
        self._spline.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def run(self, waypoints, ds=0.1, solve="device", c=None, obstacle_list=None, robot_radius=0.0, arrays=True):
        """waypoints: a list of (x, y) pairs of sequences, a CSR tuple (offsets, x, y), or a list of (n_i, 2) arrays such as
        planner paths (2 .. 4096 waypoints per course).  ds: a scalar or one value per course.  solve: "device" or "numpy"
        (see the module docstring); c=(cx, cy), flat over all waypoints, overrides it.  obstacle_list: rows (x, y, size)
        every point is tested against with robot_radius (result.hit / .free).  arrays=False: records and hits only;
        arrays="device": the points stay on the device for BatchTrack.run (result.device_courses), none is fetched."""
        if solve not in ("device", "numpy"):
            raise ValueError("BatchSpline: solve is 'device' or 'numpy'")
        if c is None and solve == "numpy":
            off, x, y = _csr(waypoints)
            if len(off) > 1 and np.min(np.diff(off)) < 2:
                raise _abi.RrtxError("rrtx_spline_run: RRTX_E_INVALID a course of fewer than 2 waypoints")
            cs = []
            with np.errstate(all="ignore"):   # coinciding waypoints: the device reports them, whatever the solve made of them
                for i in range(len(off) - 1):
                    try:
                        cs.append(solve_numpy(x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]))
                    except np.linalg.LinAlgError:
                        cs.append((np.zeros(off[i + 1] - off[i]),) * 2)
            c = (np.nan_to_num(np.concatenate([q[0] for q in cs])) if cs else np.zeros(0),
                 np.nan_to_num(np.concatenate([q[1] for q in cs])) if cs else np.zeros(0))
            waypoints = (off, x, y)
        b, keep = pack_batch(waypoints, ds, c, obstacle_list, robot_radius, arrays)
        S = self._spline
        self._n = None
        rc = S.run(b)
        rec, off, ms = S.records()
        self._n = len(rec)
        w = int(keep["offsets"][-1])
        res = SplineResult(rec, off, S.points(int(off[-1])) if arrays and not _abi.on_device(arrays) else None, S.c(w),
                           keep["offsets"], S.hits(len(rec)) if keep["obstacles"] is not None else None, rc, ms)
        if _abi.on_device(arrays):
            res.device_courses = _abi.DeviceCourses(_abi.SRC_SPLINE, S)
        res.obstacle_index = S.obstacle_index_info() if keep["obstacles"] is not None else None
        return res

    def fit(self, waypoints, solve="device", c=None):
        """The splines of run() without a sample: fits every course and keeps it on the device for query().  Returns the
        SplineResult (status, total_length, c; no arrays)."""
        return self.run(waypoints, ds=1.0, solve=solve, c=c, arrays=False)

    def fit1d(self, knots, values, solve="device", c=None):
        """One-dimensional splines CubicSpline1D(knots_i, values_i): knots (ascending; integers become float64) and values
        as lists of one sequence per spline, CSR tuples (offsets, flat), or one sequence each (a batch of one); 2 .. 4096
        knots per spline.  solve and c as run() takes them, c flat over all knots.  Returns a SplineResult whose c is
        (c, None); n_points is 0 and total_length the last knot."""
        if solve not in ("device", "numpy"):
            raise ValueError("BatchSpline: solve is 'device' or 'numpy'")
        off, kn = _csr1(knots)
        off_v, va = _csr1(values)
        if not np.array_equal(off, off_v):
            raise ValueError("BatchSpline: knots and values differ in shape")
        n = len(off) - 1
        if c is None and solve == "numpy":
            if n and np.min(np.diff(off)) < 2:
                raise _abi.RrtxError("rrtx_spline_fit1d: RRTX_E_INVALID a spline of fewer than 2 knots")
            cs = []
            with np.errstate(all="ignore"):   # equal knots: the device reports them, whatever the solve made of them
                for i in range(n):
                    try:
                        cs.append(solve_numpy_1d(kn[off[i]:off[i + 1]], va[off[i]:off[i + 1]]))
                    except np.linalg.LinAlgError:
                        cs.append(np.zeros(off[i + 1] - off[i]))
            c = np.nan_to_num(np.concatenate(cs)) if cs else np.zeros(0)
        ca = None if c is None else _f64(c).reshape(-1)
        b = _abi.SplineFit1dBatch(n=n, offsets=off.ctypes.data, knots=kn.ctypes.data, values=va.ctypes.data,
                                  c=None if ca is None else ca.ctypes.data, n_c=0 if ca is None else len(ca))
        S = self._spline
        self._n = None
        rc = S.fit1d(b)
        rec, _, ms = S.records()
        self._n = len(rec)
        return SplineResult(rec, np.zeros(n + 1, dtype=np.int64), None, (S.c1d(int(off[-1])), None), off, None, rc, ms)

    def query(self, s, derivatives=False):
        """The splines of the last run(), fit() or fit1d() at the caller's parameters.  s: a list of one sequence per spline, a
        CSR tuple (offsets, t), or one 1-D array applied to every spline; any double is taken.  Returns a
        SplineQueryResult."""
        if self._n is None:
            raise _abi.RrtxError("rrtx_spline_query: RRTX_E_STATE no completed run or fit1d")
        n = self._n
        is_csr = (isinstance(s, tuple) and len(s) == 2 and np.ndim(s[0]) == 1 and np.ndim(s[1]) == 1
                  and np.issubdtype(np.asarray(s[0]).dtype, np.integer) and len(s[0]) == n + 1)
        if is_csr:
            off, t = np.ascontiguousarray(s[0], dtype=np.int64), _f64(s[1]).reshape(-1)
            if off[-1] != len(t):
                raise ValueError("BatchSpline: the offsets do not describe the parameters")
        elif isinstance(s, np.ndarray) and s.ndim == 1 or (len(s) and all(np.ndim(v) == 0 for v in s)):
            one = _f64(s).reshape(-1)
            off, t = np.arange(n + 1, dtype=np.int64) * len(one), np.tile(one, n)
        else:
            if len(s) != n:
                raise ValueError("BatchSpline: %d lists of parameters for %d splines" % (len(s), n))
            off, t = _csr1(list(s))
        b = _abi.SplineQueryBatch(n=n, q_offsets=off.ctypes.data, t=t.ctypes.data if len(t) else None,
                                  want_derivatives=int(bool(derivatives)), reserved=0)
        S = self._spline
        rc = S.query(b)
        planes, status, ms = S.query_planes()
        return SplineQueryResult(off, t, status, planes, rc, ms)

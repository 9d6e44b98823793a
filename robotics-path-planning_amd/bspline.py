"""Batched interpolating B-spline courses of degree 1 .. 5 through waypoints on the GPU: the reference's two scipy scripts.

    bb = BatchBSpline()
    res = bb.interpolate(paths, 50, degree=3)       # interpolate_b_spline_path(x_i, y_i, 50, 3) for every course
    rx, ry, heading, curvature = res.course(i)
    res = bb.spline2d(paths, ds=0.1, kind="cubic")  # the driver loop of spline_2d over Spline2D(x_i, y_i, kind)
    tracked = BatchTrack().run(res)                  # a BSplineResult is a batch of (x, y, yaw) courses

Both scripts are one object: B-spline interpolation on a knot vector known in closed form (clamped ends; the data sites for
odd degree, their midpoints for even degree -- what FITPACK with s = 0 and make_interp_spline's not-a-knot default choose).
The reference's bit for bit: the waypoint parameter, the knots, the sample parameters (np.linspace, np.arange), counts and
offsets, and x and y of spline2d's linear kind.  This package's own definition, bit-identical to tests/bspline_oracle.py: the
B-spline coefficients (banded elimination without pivoting) and the evaluation (Cox-de Boor recurrences in a stated order);
they agree with scipy to a measured tolerance.  scipy is not imported.

The smoothing fit, approximate_b_spline_path with s other than 0 (s=None included), is approximate():

    res = bb.approximate(paths, 50, degree=3, s=0.5)   # approximate_b_spline_path(x_i, y_i, 50, 3, s=0.5) for every course

FITPACK's adaptive knot insertion and its root search on the smoothing parameter, restated: the knot vectors are
scipy's, the coefficients this package's own arithmetic, bit-identical to tests/bspline_smooth_oracle.py and within a measured
tolerance of scipy.  The drop-in module rrt_amd.bspline_path_smoothing calls it; rrt_amd.bspline_path still refuses s != 0.
There is no CPU fallback: without a device BatchBSpline raises RrtxError.
"""
import warnings

import numpy as np

from . import _abi
from .spline import _csr, _f64

KINDS = {"linear": 1, "quadratic": 2, "cubic": 3}


def _samples(u, n):
    """(u_offsets, values) of explicit sample parameters: a CSR tuple (offsets, values) or one sequence per course"""
    if (isinstance(u, tuple) and len(u) == 2 and np.ndim(u[0]) == 1 and np.ndim(u[1]) == 1
            and np.issubdtype(np.asarray(u[0]).dtype, np.integer) and len(u[0]) == n + 1):
        off, val = np.ascontiguousarray(u[0], dtype=np.int64), _f64(u[1]).reshape(-1)
    else:
        if len(u) != n:
            raise ValueError("BatchBSpline: %d sample lists for %d courses" % (len(u), n))
        parts = [_f64(q).reshape(-1) for q in u]
        off = np.zeros(n + 1, dtype=np.int64)
        if parts:
            off[1:] = np.cumsum([len(q) for q in parts])
        val = _f64(np.concatenate(parts)) if parts else np.zeros(0)
    if off[-1] != len(val):
        raise ValueError("BatchBSpline: the sample offsets do not describe the sample array")
    return off, val


def pack_batch(waypoints, degree=3, param=_abi.BSPLINE_PARAM_NORMALISED, n_path_points=None, ds=None, u=None,
               obstacle_list=None, robot_radius=0.0, arrays=True):
    """The rrtx_bspline_batch of one run: (batch, keep).  n_path_points (np.linspace) or ds (np.arange) selects the sampling
    mode; u alone gives every course its sample parameters as data; u beside one of the two is a list with a sample list for
    the courses sampled explicitly and None for the others.  `keep` names the arrays the batch points into (they must
    outlive the call)."""
    off, x, y = _csr(waypoints)
    n = len(off) - 1
    if n_path_points is not None and ds is not None or all(v is None for v in (n_path_points, ds, u)):
        raise ValueError("BatchBSpline: one of n_path_points and ds, or u alone, is given")

    def per_course(v, dtype, what):
        if np.ndim(v) == 0:
            return np.ascontiguousarray([v], dtype=dtype), False
        a = np.ascontiguousarray(v, dtype=dtype).reshape(-1)
        if len(a) != n:
            raise ValueError("BatchBSpline: %d values of %s for %d courses" % (len(a), what, n))
        return a, True
    if np.ndim(degree) == 0 and int(degree) != degree:
        raise ValueError("BatchBSpline: degree is an integer")
    deg, deg_per = per_course(degree, np.int32, "degree")
    cnt = dsa = uoff = uval = modes = None
    smp_per = False
    sample = _abi.BSPLINE_SAMPLE_EXPLICIT
    if n_path_points is not None:
        sample = _abi.BSPLINE_SAMPLE_LINSPACE
        cnt, smp_per = per_course(n_path_points, np.int64, "n_path_points")
    elif ds is not None:
        sample = _abi.BSPLINE_SAMPLE_ARANGE
        dsa, smp_per = per_course(ds, np.float64, "ds")
    if u is not None:
        if sample != _abi.BSPLINE_SAMPLE_EXPLICIT:   # a mode per course: explicit where a sample list is given
            if isinstance(u, tuple) or len(u) != n:
                raise ValueError("BatchBSpline: with n_path_points or ds, u is one sample list or None per course")
            modes = np.ascontiguousarray([sample if q is None else _abi.BSPLINE_SAMPLE_EXPLICIT for q in u], dtype=np.int32)
            u = [np.zeros(0) if q is None else q for q in u]
        elif not isinstance(u, tuple) and any(q is None for q in u):
            raise ValueError("BatchBSpline: a course without sample list needs n_path_points or ds")
        uoff, uval = _samples(u, n)
    obs = _f64([list(o) for o in obstacle_list]).reshape(-1, 3) if obstacle_list is not None and len(obstacle_list) else None
    keep = dict(offsets=off, x=x, y=y, degree=deg, sample_of=modes, count=cnt, ds=dsa, u_offsets=uoff, u=uval, obstacles=obs)

    def ptr(a):
        return None if a is None else a.ctypes.data
    b = _abi.BSplineBatch(n=n, offsets=ptr(off), x=ptr(x), y=ptr(y), degree=ptr(deg), degree_per_course=int(deg_per),
                          param=int(param), sample=sample, sample_per_course=int(smp_per), sample_of=ptr(modes),
                          count=ptr(cnt), ds=ptr(dsa), u_offsets=ptr(uoff), u=ptr(uval), want_arrays=int(bool(arrays)),
                          reserved=0, obstacles=ptr(obs), n_obstacles=0 if obs is None else len(obs),
                          robot_radius=float(robot_radius))
    return b, keep


def pack_smooth_batch(waypoints, s=None, **kw):
    """The rrtx_bspline_smooth_batch of one approximate run: (batch, keep); kw as pack_batch without param.  s: a scalar, one
    value per course, or None (an entry None likewise): the course's waypoint count."""
    b, keep = pack_batch(waypoints, param=_abi.BSPLINE_PARAM_NORMALISED, **kw)
    n = int(b.n)
    m = np.diff(keep["offsets"]).astype(np.float64)
    if s is None:
        sv, s_per = m, True
    elif np.ndim(s) == 0:
        sv, s_per = [float(s)], False
    else:
        if len(s) != n:
            raise ValueError("BatchBSpline: %d values of s for %d courses" % (len(s), n))
        sv, s_per = [m[i] if q is None else float(q) for i, q in enumerate(s)], True
    keep["s"] = np.ascontiguousarray(sv, dtype=np.float64).reshape(-1)
    if s_per and n == 0:
        keep["s"] = np.zeros(1)
    return _abi.BSplineSmoothBatch(run=b, s=keep["s"].ctypes.data, s_per_course=int(s_per), reserved=0), keep


class BSplineResult:
    """One batch of B-spline courses.  Per course: status (BSPLINE_OK, BSPLINE_DEGENERATE coinciding waypoints, BSPLINE_TOO_FEW
    no more waypoints than the degree), n_points, degree, length (the last waypoint parameter: 1.0 from interpolate(), s[-1]
    from spline2d()); offsets (n + 1,) into the flat x, y, yaw, k, u (None when the run was made with arrays=False), u being
    the sample parameter; knots with knot_offsets (n + 1,), and coefficients = (cx, cy) flat over the waypoints (wp_offsets);
    hit (n,) int32 when the batch was run with an obstacle list (-1 free, j >= 0 the first circle of the list the course
    touches, -2 no points), else None; rc 0 or RRTX_PARTIAL; kernel_ms.
    offsets / x / y / yaw are what BatchTrack.run takes as a batch of courses."""

    def __init__(self, records, offsets, arrays, knots, knot_offsets, coefficients, wp_offsets, hit=None, rc=0, kernel_ms=0.0):
        self.status = records["status"].copy()
        self.n_points = records["n_points"].copy()
        self.degree = records["degree"].copy()
        self.length = records["length"].copy()
        self.offsets = offsets
        self.x, self.y, self.yaw, self.k, self.u = arrays if arrays is not None else (None,) * 5
        self.device_courses = None   # arrays="device": an _abi.DeviceCourses, and the five arrays are None
        self.knots = knots
        self.knot_offsets = knot_offsets
        self.coefficients = coefficients
        self.wp_offsets = wp_offsets
        self.hit = hit
        self.obstacle_index = None   # with an obstacle list: what tested it (the obstacle_index keyword), a dict
        self.rc = rc
        self.kernel_ms = kernel_ms

    def __len__(self):
        return len(self.status)

    def _raise_for(self, i, who):
        st = int(self.status[i])
        if st == _abi.BSPLINE_DEGENERATE:
            raise _abi.RrtxError("%s: course %d has two consecutive waypoints that coincide (scipy raises on such input)" % (who, i))
        if st == _abi.BSPLINE_TOO_FEW:
            raise _abi.RrtxError("%s: course %d has no more waypoints than its degree %d (scipy raises on such input)"
                                 % (who, i, int(self.degree[i])))

    def course(self, i):
        """What interpolate_b_spline_path returns for course i: (x, y, heading, curvature) as arrays."""
        self._raise_for(i, "course()")
        if self.x is None:
            raise _abi.RrtxError("course(): this batch was run with arrays=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return tuple(q[a:b].copy() for q in (self.x, self.y, self.yaw, self.k))

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


class BSplineSmoothResult(BSplineResult):
    """One batch of smoothing B-spline courses (BatchBSpline.approximate).  status, n_points, degree, length, offsets, x, y,
    yaw, k, u, hit / free / is_free(i), course(i), rc and kernel_ms as BSplineResult (status may also be BSPLINE_SINGULAR: a
    coefficient is not finite; such a course owns no points).  The two axes of a course have splines of their own, so these
    are pairs (x axis, y axis): knots with knot_offsets (n + 1,), coefficients with coef_offsets (n + 1,), and per course
    ier (FITPACK's: 0 smoothing spline, -1 interpolating, -2 least-squares polynomial, 2 / 3 the root search stopped early
    and the last approximation is kept; 1 no knot could be added, the least-squares spline on the knots so far), fp (the sum of squared residuals), p (the smoothing parameter, +inf without a root
    search), rounds (knot rounds) and iters (root-search steps).  wp_offsets: the waypoint CSR of the batch."""

    def __init__(self, records, offsets, arrays, axes, axis_records, wp_offsets, hit=None, rc=0, kernel_ms=0.0):
        BSplineResult.__init__(self, records, offsets, arrays, tuple(a[1] for a in axes), tuple(a[0] for a in axes),
                               tuple(a[3] for a in axes), wp_offsets, hit, rc, kernel_ms)
        self.coef_offsets = tuple(a[2] for a in axes)
        for key in ("ier", "fp", "p", "rounds", "iters"):
            setattr(self, key, tuple(axis_records[a][key].copy() for a in (0, 1)))

    def _raise_for(self, i, who):
        if int(self.status[i]) == _abi.BSPLINE_SINGULAR:
            raise _abi.RrtxError("%s: the smoothing fit of course %d has a coefficient that is not finite" % (who, i))
        BSplineResult._raise_for(self, i, who)


def _check_range(u_offsets, u, status, length):
    """interp1d's bounds check for explicit samples: ValueError outside [0, length] of a course that has a spline"""
    for i in np.nonzero(status == _abi.BSPLINE_OK)[0]:
        q = u[u_offsets[i]:u_offsets[i + 1]]
        if len(q) and np.min(q) < 0.0:
            raise ValueError("A value (%r) in the samples of course %d is below the interpolation range's minimum value (0.0)."
                             % (float(np.min(q)), i))
        if len(q) and np.max(q) > length[i]:
            raise ValueError("A value (%r) in the samples of course %d is above the interpolation range's maximum value (%r)."
                             % (float(np.max(q)), i, float(length[i])))


class BatchBSpline:
    """Interpolating and smoothing B-splines of degree 1 .. 5 through batches of waypoint lists; device buffers are kept
    between calls."""

    def __init__(self, device=0, obstacle_index=None):
        """obstacle_index: None, True or False, as BatchSteer's (also a settable attribute); result.obstacle_index says what
        tested a run's obstacle list."""
        _abi.obstacle_index_mode(obstacle_index)   # a ValueError comes before any device call
        self._bs = _abi.BSpline(device)
        self.obstacle_index = obstacle_index

    @property
    def obstacle_index(self):
        return self._obstacle_index

    @obstacle_index.setter
    def obstacle_index(self, v):
        _abi.obstacle_index_mode(v)
        self._bs.set_obstacle_index(v)
        self._obstacle_index = v

    def close(self):
        self._bs.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _run(self, waypoints, arrays, **kw):
        b, keep = pack_batch(waypoints, arrays=arrays, **kw)
        S = self._bs
        rc = S.run(b)
        rec, off, n_knots, ms = S.records()
        if keep["u"] is not None:
            _check_range(keep["u_offsets"], keep["u"], rec["status"], rec["length"])
        koff, knots, cx, cy = S.coefficients(len(rec), n_knots, int(keep["offsets"][-1]))
        res = BSplineResult(rec, off, S.points(int(off[-1])) if arrays and not _abi.on_device(arrays) else None, knots, koff,
                            (cx, cy), keep["offsets"], S.hits(len(rec)) if keep["obstacles"] is not None else None, rc, ms)
        if _abi.on_device(arrays):
            res.device_courses = _abi.DeviceCourses(_abi.SRC_BSPLINE, S)
        res.obstacle_index = S.obstacle_index_info() if keep["obstacles"] is not None else None
        return res

    def interpolate(self, waypoints, n_path_points=None, degree=3, obstacle_list=None, robot_radius=0.0, arrays=True, u=None):
        """interpolate_b_spline_path(x, y, n_path_points, degree) (10_path_planning_00_bspline_path.py :59-108) for every
        course: the parameter of _calc_distance_vector, samples np.linspace(0.0, u[-1], n_path_points), and per point x, y,
        heading and curvature.  The curvature keeps the script's own exponent, (ddy * dx - ddx * dy) / np.power(dx * dx +
        dy * dy, 2.0 / 3.0): 2 / 3, not the geometric 3 / 2, and it is not corrected here.  Degree 1 has a zero second
        derivative, hence zero curvature (the script itself raises there, in derivative(2)).
        waypoints: a list of (x, y) pairs of sequences, a CSR tuple (offsets, x, y), or a list of (n_i, 2) arrays, 2 .. 4096
        waypoints per course.  n_path_points and degree (1 .. 5): a scalar or one value per course; courses of different
        degree run side by side.  u=: explicit sample parameters in [0, 1], one sequence per course or a CSR tuple (offsets,
        values), instead of n_path_points -- or beside it, as a list with None for the courses that keep n_path_points;
        ValueError outside the range, as scipy's interp1d raises.  obstacle_list: rows
        (x, y, size) every point is tested against with robot_radius (result.hit / .free).  arrays=False: records, splines
        and hits only; arrays="device" (here, in spline2d and in approximate): the points stay on the device for
        BatchTrack.run (result.device_courses), none is fetched."""
        return self._run(waypoints, arrays, degree=degree, param=_abi.BSPLINE_PARAM_NORMALISED, n_path_points=n_path_points,
                         u=u, obstacle_list=obstacle_list, robot_radius=robot_radius)

    def approximate(self, waypoints, n_path_points=None, degree=3, s=None, u=None, obstacle_list=None, robot_radius=0.0,
                    arrays=True):
        """approximate_b_spline_path(x, y, n_path_points, degree, s) (10_path_planning_00_bspline_path.py :12-56) for every
        course: UnivariateSpline(distances, x, k=degree, s=s) and the same for y, then _evaluate_spline at
        np.linspace(0.0, 1.0, n_path_points).  s: a scalar, one value per course, or None -- the script's default, each
        course's waypoint count (an entry None of a list means the same); finite and >= 0.  A course with s == 0 is
        interpolate()'s, bit for bit.  The knot vectors are scipy's; the coefficients agree with scipy to a measured
        tolerance.  Where FITPACK's root search stops early (ier 2 or 3) the last approximation is kept, as
        scipy keeps it, and one RuntimeWarning per call names how many axes.  The other arguments as interpolate().
        Returns a BSplineSmoothResult."""
        sb, keep = pack_smooth_batch(waypoints, s, arrays=arrays, degree=degree, n_path_points=n_path_points, u=u,
                                     obstacle_list=obstacle_list, robot_radius=robot_radius)
        S = self._bs
        rc = S.approximate(sb)
        rec, off, _, ms = S.records()
        if keep["u"] is not None:
            _check_range(keep["u_offsets"], keep["u"], rec["status"], rec["length"])
        arec = S.axis_records(len(rec))
        axes = [S.axis_splines(a, len(rec)) for a in (0, 1)]
        early = int(np.sum((arec["ier"] > 0) & (rec["status"] == _abi.BSPLINE_OK)[None, :]))
        if early:
            warnings.warn("BatchBSpline.approximate: the fit stopped early on %d axes (ier 2 or 3: the root search on the "
                          "smoothing parameter; ier 1: no knot could be added); their last approximation is kept" % early,
                          RuntimeWarning, stacklevel=2)
        res = BSplineSmoothResult(rec, off, S.points(int(off[-1])) if arrays and not _abi.on_device(arrays) else None, axes,
                                  arec, keep["offsets"], S.hits(len(rec)) if keep["obstacles"] is not None else None, rc, ms)
        if _abi.on_device(arrays):
            res.device_courses = _abi.DeviceCourses(_abi.SRC_BSPLINE, S)
        res.obstacle_index = S.obstacle_index_info() if keep["obstacles"] is not None else None
        return res

    def spline2d(self, waypoints, ds=0.1, kind="cubic", obstacle_list=None, robot_radius=0.0, arrays=True, u=None):
        """The driver loop of 10_path_planning_00_spline_2d.py (:45-54) for every course: Spline2D(x, y, kind), s of
        Spline2D.__calc_s, samples np.arange(0, s[-1], ds), and calc_position at each.  kind: "linear", "quadratic" or
        "cubic" (degree 1, 2, 3), one name or one per course; ds: a scalar or one per course.  The linear kind's x and y are
        interp1d's own arithmetic bit for bit.  The script returns only (x, y): yaw -- atan2 of the first derivative -- and k
        -- the same form as interpolate(), exponent 2 / 3 included -- are this package's additions.  u=: explicit sample
        parameters in [0, s[-1]], with ds=None for all courses or beside ds as in interpolate().  The other keywords as interpolate()."""
        def deg(name):
            if name not in KINDS:
                raise ValueError("BatchBSpline: kind is 'linear', 'quadratic' or 'cubic', not %r" % (name,))
            return KINDS[name]
        degree = deg(kind) if isinstance(kind, str) else [deg(q) for q in kind]
        return self._run(waypoints, arrays, degree=degree, param=_abi.BSPLINE_PARAM_CHORD, ds=ds, u=u,
                         obstacle_list=obstacle_list, robot_radius=robot_radius)

"""Batched closed-loop tracking of courses on the GPU, without a planner around it.

    bt = BatchTrack()                                   # the model globals of rrt_10:1592-1607 as keywords
    res = bt.run(courses, obstacle_list, robot_radius=0.3)
    find_goal, x, y, yaw, v, t, a, d = res.feasible(i)  # what check_tracking_path_is_feasible returns for course i
    flag, x, y, yaw, v, t, a, d = res.best()            # search_best_feasible_path over the batch

A producer can leave its courses on the device and the tracker reads them there (rrtx_tracker_run_from): no point crosses
to the host and back.

    plan = BatchSteer("rs").plan_free(starts, goals, 1.0, product=True, obstacle_list=circles, points="device")
    res = bt.run(plan, circles, robot_radius=0.3, select="free", group=True, arrays="best")
    res.winner[j]; flag, x, y, yaw, v, t, a, d, goal = res.best_of(j)     # one start against all goals, picked on the device

For every course: what the reference's ClosedLoopRRTStar.check_tracking_path_is_feasible(path)
(10_path_planning_01_rrt_10_closed_loop_rrt_star.py :1526-1564) returns, every double the reference's.  A course is given
in driving order (start ... goal; the reference receives it reversed), its goal is its last point, and the roll-out starts
at the reference's State(-0.0, -0.0, 0.0, 0.0) unless start_state is given.  There is no CPU fallback: without a device
BatchTrack raises RrtxError.
"""
import numpy as np

from . import _abi

OOD_DOMAIN, OOD_RAISES, OOD_OVERFLOW = 1, 2, 3   # rrtx_track_record.ood
OOD_NOT_FINITE, OOD_SKIPPED = _abi.OOD_NOT_FINITE, _abi.OOD_SKIPPED   # device-resident courses only


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _csr(courses):
    """(offsets, x, y, yaw) of `courses`: a SteerResult (or anything with its offsets / x / y / yaw), a CSR tuple, or a list
    of (cx, cy, cyaw) triples."""
    if hasattr(courses, "offsets") and hasattr(courses, "yaw"):
        if getattr(courses, "kind", None) == _abi.STEER_LQR:
            raise ValueError("BatchTrack: an LQR SteerResult has no yaw, the tracker needs courses of (x, y, yaw)")
        if courses.offsets is None or courses.x is None:
            raise ValueError("BatchTrack: the SteerResult was solved with points=False, it holds no courses")
        if courses.yaw is None:
            raise ValueError("BatchTrack: these courses have no yaw, the tracker needs courses of (x, y, yaw)")
        if getattr(courses, "order", "driving") != "driving":
            raise ValueError("BatchTrack: the courses are in planning order, the tracker drives them: order='driving'")
        courses = (courses.offsets, courses.x, courses.y, courses.yaw)
    if isinstance(courses, tuple) and len(courses) == 4 and np.ndim(courses[0]) == 1 and np.ndim(courses[1]) == 1:
        off = np.ascontiguousarray(courses[0], dtype=np.int64)
        x, y, yaw = (_f64(c).reshape(-1) for c in courses[1:])
    else:
        trip = [tuple(_f64(c).reshape(-1) for c in t) for t in courses]
        for cx, cy, cw in trip:
            if not len(cx) == len(cy) == len(cw):
                raise ValueError("BatchTrack: cx, cy and cyaw of a course differ in length")
        off = np.zeros(len(trip) + 1, dtype=np.int64)
        if trip:
            off[1:] = np.cumsum([len(t[0]) for t in trip])
        x, y, yaw = (_f64(np.concatenate([t[k] for t in trip])) if trip else np.zeros(0) for k in range(3))
    if len(off) < 1 or not len(x) == len(y) == len(yaw) or (len(off) and off[-1] != len(x)):
        raise ValueError("BatchTrack: the offsets do not describe the point arrays")
    return off, x, y, yaw


def _per_course(v, n, name):
    """(array, is_per_course): a scalar stays one value, a sequence must hold one value per course."""
    if np.ndim(v) == 0:
        return _f64([float(v)]), False
    a = _f64(v).reshape(-1)
    if len(a) != n:
        raise ValueError("BatchTrack: %d values of %s for %d courses" % (len(a), name, n))
    return a, True


def pack_source(dc, n, select=None, group=None, arrays=True):
    """The rrtx_track_source of one run over the device-resident courses `dc` (an _abi.DeviceCourses) of n courses:
    (source, keep).  `keep` holds the mask the source points into."""
    mask, sel = None, _abi.SELECT_ALL
    if isinstance(select, str):
        if select != "free":
            raise ValueError("BatchTrack: select is None, 'free' or a boolean array")
        sel = _abi.SELECT_FREE
    elif select is not None:
        mask = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8)
        if len(mask) != n:
            raise ValueError("BatchTrack: a mask of %d entries for %d courses" % (len(mask), n))
        sel = _abi.SELECT_MASK
    g = 0 if group is None else int(group)
    if group is not None and g < 1:
        raise ValueError("BatchTrack: group is a size >= 1")
    best = isinstance(arrays, str) and arrays == "best"
    if best and not g:
        raise ValueError("BatchTrack: arrays='best' needs a group")
    src = _abi.TrackSource(kind=dc.kind, select=sel, object=dc.owner._s, generation=dc.generation,
                           mask=None if mask is None else mask.ctypes.data, group=g, arrays_of=int(best))
    return src, dict(mask=mask)


def pack_batch(courses, obstacle_list=(), course_obstacles=None, robot_radius=0.0, target_speed=10.0 / 3.6,
               yaw_th=float(np.deg2rad(3.0)), invalid_travel_ratio=5.0, start_state=None, arrays=True):
    """The rrtx_track_batch of one run and the three scalars that go into rrtx_track_params: (batch, scalars, keep).
    `keep` names the arrays the batch points into (they must outlive the call); goals (n, 3) is each course's last point."""
    off, x, y, yaw = _csr(courses)
    n = len(off) - 1
    if course_obstacles is not None and len(obstacle_list):
        raise ValueError("BatchTrack: give obstacle_list or course_obstacles, not both")
    if course_obstacles is not None:
        if len(course_obstacles) != n:
            raise ValueError("BatchTrack: %d obstacle lists for %d courses" % (len(course_obstacles), n))
        obs_off, obs = _abi.pack_instance_obstacles(course_obstacles)
        obs_off = np.ascontiguousarray(obs_off, dtype=np.int64)
        obs = _f64(obs).reshape(-1, 3)
    else:
        obs_off = None
        obs = _f64([list(o) for o in obstacle_list]).reshape(-1, 3)
    rr, rr_per = _per_course(robot_radius, n, "robot_radius")
    cols = [_per_course(v, n, k) for k, v in (("target_speed", target_speed), ("yaw_th", yaw_th),
                                              ("invalid_travel_ratio", invalid_travel_ratio))]
    per = None
    if any(p for _, p in cols):
        per = _f64(np.stack([np.broadcast_to(a, (n,)) for a, _ in cols], axis=1))
    scalars = {k: float(a[0]) for k, (a, _) in zip(("target_speed", "yaw_th", "invalid_travel_ratio"), cols)}
    st = None
    if start_state is not None:
        st = _f64(start_state)
        st = _f64(np.broadcast_to(st, (n, 4))) if st.ndim == 1 else st.reshape(-1, 4)
        if len(st) != n:
            raise ValueError("BatchTrack: %d start states for %d courses" % (len(st), n))
    keep = dict(offsets=off, x=x, y=y, yaw=yaw, per_course=per, start_state=st, obstacles=obs, obs_offsets=obs_off,
                robot_radius=rr)

    def ptr(a):
        return None if a is None else a.ctypes.data
    b = _abi.TrackBatch(n=n, offsets=ptr(off), x=ptr(x), y=ptr(y), yaw=ptr(yaw), per_course=ptr(per), start_state=ptr(st),
                        obstacles=ptr(obs), obs_offsets=ptr(obs_off), n_obstacles=len(obs), robot_radius=ptr(rr),
                        robot_radius_per_course=int(rr_per), want_arrays=int(bool(arrays)))
    goals = np.full((n, 3), np.nan)
    full = np.nonzero(np.diff(off) > 0)[0]
    last = off[1:][full] - 1
    goals[full] = np.stack([x[last], y[last], yaw[last]], axis=1)
    keep["goals"] = goals
    return b, scalars, keep


class TrackResult:
    """One tracked batch.  Per course: find_goal, length (len(t)), fail (TRACK_FAIL_* bits), t_last (t[-1]) and status (0,
    or 1 tan outside the replica's domain, 2 the reference raises, 3 longer than 960 points; of device-resident courses
    also 4 a pose component is not finite, 5 left out by `select`); offsets (n + 1,) into the flat x, y, yaw, v, t, a, d
    (None when the run was made with arrays=False); steps: their length.  A run with a group: winner (n / group,), the
    course the device picked in each group (-1 none), else None.
    goals (n, 3) is each course's last point.  Of device-resident courses the tracker keeps the goals on the device: with a
    group only the winners' rows are fetched (best() raises RrtxError for another course of such a run), without one
    all rows on first use -- which must come before the tracker's next run, or goals, best() and best_of() raise
    RrtxError.  A result of host courses holds everything it needs."""

    def __init__(self, records, offsets, arrays, goals, rc=0, kernel_ms=0.0, course_len=None, winner=None, group=0,
                 obstacle_index=None):
        self.find_goal = records["find_goal"].copy()
        self.length = records["len"].copy()
        self.fail = records["fail"].copy()
        self.t_last = records["t_last"].copy()
        self.status = records["ood"].copy()
        self.offsets = offsets
        self.x, self.y, self.yaw, self.v, self.t, self.a, self.d = arrays if arrays is not None else (None,) * 7
        self._goals = goals         # (n, 3): each course's last point; device-resident courses: a callable that fetches
        self.winner = winner        # them on first use, or with a group the winners' rows, NaN elsewhere
        self.group = group
        self.course_len = np.zeros(len(records), dtype=np.int64) if course_len is None else course_len
        self.rc = rc                # 0 or RRTX_PARTIAL
        self.kernel_ms = kernel_ms
        self.steps = int(offsets[-1])
        self.obstacle_index = obstacle_index   # with an obstacle list: what tested it (BatchTrack's obstacle_index), a dict

    def __len__(self):
        return len(self.status)

    @property
    def goals(self):
        if callable(self._goals):
            self._goals = self._goals()
        return self._goals

    def feasible(self, i):
        """What check_tracking_path_is_feasible returns for course i: (find_goal, x, y, yaw, v, t, a, d) with lists;
        IndexError where the reference raises it (a course of fewer than 3 points, rrt_10:1435)."""
        st = int(self.status[i])
        if st == OOD_RAISES:
            raise IndexError("index -3 is out of bounds for axis 0 with size %d" % int(self.course_len[i]))
        if st == OOD_OVERFLOW:
            raise _abi.RrtxError("feasible(): course %d is longer than 960 points" % i)
        if st == OOD_NOT_FINITE:
            raise _abi.RrtxError("feasible(): course %d holds an x, y or yaw that is not finite" % i)
        if st == OOD_SKIPPED:
            raise _abi.RrtxError("feasible(): course %d was left out by select, it was not tracked" % i)
        if self.winner is not None and self.x is not None and self.offsets[i] == self.offsets[i + 1] and self.length[i]:
            raise _abi.RrtxError("feasible(): this batch was run with arrays='best' and course %d is no winner" % i)
        if st:
            raise _abi.RrtxError("feasible(): course %d left the domain of the tan replica (steer_max above 0.79)" % i)
        if self.x is None:
            raise _abi.RrtxError("feasible(): this batch was run with arrays=False")
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return (bool(self.find_goal[i]),) + tuple(q[a:b].tolist() for q in (self.x, self.y, self.yaw, self.v, self.t,
                                                                             self.a, self.d))

    def best(self, indices=None):
        """search_best_feasible_path (rrt_10:1495-1524) over the courses `indices` (default: all) in that order: the
        feasible one with the smallest t[-1], the later one of equal times; its goal pose is appended to x, y, yaw."""
        best_time, win = float("inf"), None
        for i in (range(len(self)) if indices is None else indices):
            out = self.feasible(i)
            if out[0] and best_time >= out[5][-1]:   # :1510
                best_time, win = out[5][-1], (i, out)
        if win is None:
            return False, None, None, None, None, None, None, None
        i, (_, x, y, yaw, v, t, a, d) = win
        gx, gy, gyaw = (float(q) for q in self.goals[i])
        if gx != gx:      # a grouped run fetched the winners' goal poses only
            raise _abi.RrtxError("best(): course %d is not the winner of its group, its goal pose was not fetched "
                                 "(use best_of(j), or run without a group)" % i)
        return True, x + [gx], y + [gy], yaw + [gyaw], v, t, a, d

    def best_of(self, j):
        """best() for group j of a run with a group, from the pick made on the device, with the goal pose appended:
        (flag, x, y, yaw, v, t, a, d, (gx, gy, gyaw)).  Unlike best(indices), which raises at the first course of the
        group that is not complete, the device passes over courses with status != 0."""
        if self.winner is None:
            raise _abi.RrtxError("best_of(): this batch was run without a group")
        w = int(self.winner[j])
        if w < 0:
            return False, None, None, None, None, None, None, None, None
        return self.best([w]) + (tuple(float(q) for q in self.goals[w]),)


class BatchTrack:
    """Pure-pursuit / PID tracking of batches of courses on the unicycle model and the four feasibility tests of
    check_tracking_path_is_feasible; device buffers are kept between calls of run()."""

    _obstacle_index = False   # the state of a new tracker (rrtx_tracker_set_obstacle_index: RRTX_OBSIDX_OFF)

    def __init__(self, device=0, dt=0.05, L=0.9, steer_max=np.deg2rad(40.0), accel_max=5.0, Kp=2.0, Lf=0.5, T=100.0,
                 goal_dis=0.5, stop_speed=0.5, obstacle_index=False):
        """obstacle_index: False -- lane k of a wave tests obstacle k, at most 64 rows in a list; True -- the shared
        obstacle_list goes through the obstacle index (a grid over the list, a trajectory point reads its own cell) and may
        hold up to 2**20 rows; course_obstacles and a per-course robot_radius with a list are then refused.  Records and
        arrays are the same either way; also a settable attribute.  result.obstacle_index says what served a batch:
        {"mode", "used", "reason", and the grid's fields}, or None without a list."""
        _abi.tracker_obstacle_index_mode(obstacle_index)   # a ValueError comes before any device call
        self.model = dict(dt=dt, L=L, steer_max=steer_max, accel_max=accel_max, Kp=Kp, Lf=Lf, T=T, goal_dis=goal_dis,
                          stop_speed=stop_speed)
        self._tracker = _abi.Tracker(device)
        self._runs_from = 0   # runs over device-resident courses so far: a result's unfetched goals are its own run's only
        if obstacle_index:
            self.obstacle_index = True

    @property
    def obstacle_index(self):
        return self._obstacle_index

    @obstacle_index.setter
    def obstacle_index(self, v):
        _abi.tracker_obstacle_index_mode(v)
        self._tracker.set_obstacle_index(v)
        self._obstacle_index = v

    def _index_checks(self, obstacle_list, course_obstacles, robot_radius):
        """With the obstacle index on: what it cannot take, before any device call."""
        if not self._obstacle_index:
            return
        if course_obstacles is not None:
            raise ValueError("BatchTrack: the obstacle index serves the shared obstacle_list only, not course_obstacles")
        if np.ndim(robot_radius) != 0 and len(obstacle_list):
            raise ValueError("BatchTrack: the obstacle index takes one robot_radius for the obstacle_list, not one per course")

    def _served(self, n_obstacles):
        """The obstacle index info of the run just made, None without a list"""
        info = getattr(self._tracker, "obstacle_index_info", None)   # (a stand-in for _abi.Tracker may have none)
        return info() if n_obstacles and info else None

    def close(self):
        self._tracker.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def run(self, courses, obstacle_list=(), course_obstacles=None, robot_radius=0.0, target_speed=10.0 / 3.6,
            yaw_th=np.deg2rad(3.0), invalid_travel_ratio=5.0, start_state=None, arrays=True, select=None, group=None):
        """courses: a list of (cx, cy, cyaw) triples, a CSR tuple (offsets, x, y, yaw), or a SteerResult solved with
        points (a pair without a path is an empty course: status 2).  obstacle_list: rows (x, y, radius) for every
        course, or course_obstacles: one such list per course (at most 64 rows in a list; with obstacle_index=True the shared
        obstacle_list may hold up to 2**20 rows).  robot_radius, target_speed,
        yaw_th, invalid_travel_ratio: a scalar or one value per course.  start_state: None, one (x, y, yaw, v) or one
        row per course.
        courses may also be a PlannerCourses (BatchPlanner.courses(order="driving")): with host arrays it is tracked like
        any CSR tuple (leave out the instances without a course yourself), with arrays="device" as below, where
        select=courses.found leaves them out on the device.
        courses may also be a SteerResult, SplineResult or BSplineResult made with points="device" / arrays="device": the
        tracker then reads the points where the producer left them (a result whose producer has solved again since raises
        RrtxError).  For those alone: select -- None, "free" (the courses with hit == -1) or a boolean array; the others
        get status 5 and are not read.  group -- an int g: courses [j g, (j + 1) g) form group j and the device picks each
        group's best (TrackResult.winner, best_of); True: ng of a product-mode steer result.  arrays="best": only the
        winners' seven arrays are produced.  The goal poses of such a result are fetched from the tracker on first use
        (with a group: the winners' at once), so use best() or goals before this tracker runs again."""
        self._index_checks(obstacle_list, course_obstacles, robot_radius)
        dc = getattr(courses, "device_courses", None)
        if dc is not None:
            return self._run_from(courses, dc, obstacle_list, course_obstacles, robot_radius, target_speed, yaw_th,
                                  invalid_travel_ratio, start_state, arrays, select, group)
        if select is not None or group is not None or (isinstance(arrays, str) and arrays == "best"):
            raise ValueError("BatchTrack: select, group and arrays='best' need courses left on the device "
                             "(points='device' / arrays='device')")
        b, scalars, keep = pack_batch(courses, obstacle_list, course_obstacles, robot_radius, target_speed, yaw_th,
                                      invalid_travel_ratio, start_state, arrays)
        p = dict(_abi.TRACK_DEFAULTS)
        p.update({k: float(v) for k, v in self.model.items()})
        p.update(scalars)
        T = self._tracker
        rc = T.run(_abi.TrackParams(**p), b)
        rec, off = T.records()
        return TrackResult(rec, off, T.arrays() if arrays else None, keep["goals"], rc, T.kernel_ms(),
                           np.diff(keep["offsets"]), obstacle_index=self._served(b.n_obstacles))

    def _run_from(self, result, dc, obstacle_list, course_obstacles, robot_radius, target_speed, yaw_th,
                  invalid_travel_ratio, start_state, arrays, select, group):
        n = len(result.status)
        if group is True:
            if getattr(result, "shape", None) is None:
                raise ValueError("BatchTrack: group=True needs a steer result planned with product=True")
            group = result.shape[1]
        empty = (np.zeros(n + 1, dtype=np.int64), np.zeros(0), np.zeros(0), np.zeros(0))   # for the per-course checks only
        b, scalars, keep = pack_batch(empty, obstacle_list, course_obstacles, robot_radius, target_speed, yaw_th,
                                      invalid_travel_ratio, start_state, arrays)
        b.offsets = b.x = b.y = b.yaw = None
        src, keep_src = pack_source(dc, n, select, group, arrays)
        p = dict(_abi.TRACK_DEFAULTS)
        p.update({k: float(v) for k, v in self.model.items()})
        p.update(scalars)
        T = self._tracker
        rc = T.run_from(_abi.TrackParams(**p), src, b)
        del keep_src
        rec, off = T.records()
        self._runs_from += 1
        winner = None
        if src.group:
            winner = T.winners()
            goals = np.full((n, 3), np.nan)
            goals[winner[winner >= 0]] = T.goals(len(winner))[winner >= 0]
        else:
            run = self._runs_from

            def goals():   # on first use; the tracker keeps them on the device until its next run (after a run of host
                if self._runs_from != run:   # courses the native getter refuses)
                    raise _abi.RrtxError("goals: the tracker has run again, the goal poses of this run were not fetched")
                return T.goals(n)
        return TrackResult(rec, off, T.arrays() if arrays else None, goals, rc, T.kernel_ms(), np.diff(result.offsets),
                           winner, int(src.group), self._served(b.n_obstacles))

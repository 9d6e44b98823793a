"""Names of /root/reference/src_path_planning/10_path_planning_00_lqr_path.py as its driver cell uses them: LQRPlanner
:15-114.  The MI355X mirror: lqr_planning is a batch of one on robotics-path-planning_amd/steer.py (same keywords, same
return shapes and types); no CPU fallback.  The device holds the gain of the reference's model (DT = 0.1, Q = R = I) as a
constant, so another DT raises RrtxError; MAX_ITER and EPS (solve_dare's) are kept as attributes and not read."""
from . import _abi
from . import steer as _s

_steer = None


class LQRPlanner:

    def __init__(self):
        self.MAX_TIME = 100.0  # Maximum simulation time
        self.DT = 0.1  # Time tick
        self.GOAL_DIST = 0.1
        self.MAX_ITER = 150
        self.EPS = 0.01

    def lqr_planning(self, sx, sy, gx, gy, show_animation=True):
        global _steer
        if self.DT != 0.1:
            raise _abi.RrtxError("LQRPlanner: the device holds the gain of the model DT = 0.1 only, not DT = %r" % (self.DT,))
        if _steer is None:
            _steer = _s.BatchSteer("lqr")
        res = _steer.plan([[sx, sy]], [[gx, gy]], resample=False, max_time=self.MAX_TIME, goal_dist=self.GOAL_DIST)
        rx, ry = res.path(0)
        if not rx:
            print("Cannot found path")
            return [], []
        return rx, ry


__all__ = ['LQRPlanner']

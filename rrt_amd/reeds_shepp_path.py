"""Names of /root/reference/src_path_planning/10_path_planning_00_reeds_shepp_path.py as its driver cell uses them:
reeds_shepp_path_planning :506-515.  The MI355X mirror: a batch of one on robotics-path-planning_amd/steer.py (same
keywords and defaults, same return shapes and types); no CPU fallback."""
from . import steer as _s

_steer = None


def reeds_shepp_path_planning(sx, sy, syaw, gx, gy, gyaw, maxc, step_size=0.2):
    global _steer
    if _steer is None:
        _steer = _s.BatchSteer("rs")
    res = _steer.plan([[sx, sy, syaw]], [[gx, gy, gyaw]], float(maxc), step_size=step_size)
    return res.path(0)


__all__ = ['reeds_shepp_path_planning']

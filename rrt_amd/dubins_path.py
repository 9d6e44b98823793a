"""Names of /root/reference/src_path_planning/10_path_planning_00_dubins_path.py as its driver cell uses them:
plan_dubins_path :109-197.  The MI355X mirror: a batch of one on robotics-path-planning_amd/steer.py (same keywords and
defaults, same return shapes and types); no CPU fallback."""
from . import steer as _s

_steer = None


def plan_dubins_path(s_x, s_y, s_yaw, g_x, g_y, g_yaw, curvature, step_size=0.1, selected_types=None):
    global _steer
    _s.word_order(selected_types)   # KeyError for an unknown word, before anything else (:177)
    if _steer is None:
        _steer = _s.BatchSteer("dubins")
    res = _steer.plan([[s_x, s_y, s_yaw]], [[g_x, g_y, g_yaw]], float(curvature), step_size=step_size,
                      selected_types=selected_types)
    return res.path(0)


__all__ = ['plan_dubins_path']

"""Names of the reference's 10_path_planning_00_reeds_shepp_path.py beyond its driver cell: calc_paths
:483-503, every Reeds-Shepp curve between two poses as the list of Path objects (:101-115) set_path kept, of which
reeds_shepp_path_planning (rrt_amd.reeds_shepp_path) is the shortest.  The MI355X mirror: a batch of one on
BatchSteer("rs").candidates (same arguments, same list, the same Python lists and floats); no CPU fallback.
generate_path is not offered: its lengths in curvature units cannot be recovered bit for bit from the divided ones."""
from . import steer as _s

Path = _s.Path
_steer = None


def calc_paths(sx, sy, syaw, gx, gy, gyaw, maxc, step_size):
    global _steer
    if _steer is None:
        _steer = _s.BatchSteer("rs")
    res = _steer.candidates([[sx, sy, syaw]], [[gx, gy, gyaw]], float(maxc), step_size=step_size)
    return res.paths(0)


__all__ = ['calc_paths', 'Path']

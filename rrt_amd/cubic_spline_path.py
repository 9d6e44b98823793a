"""Names of the reference's 10_path_planning_00_cubic_spline_path.py as its driver cell uses them: calc_spline_course :313-325.
The MI355X mirror: a batch of one on robotics-path-planning_amd/spline.py with solve="numpy" -- the host makes the spline
coefficient c with np.linalg.solve exactly as the reference does, the device does the rest -- so a driver cell sees the
reference's values on its own host; no CPU fallback.  Coinciding consecutive waypoints, where the reference divides by zero and
returns inf / nan, raise RrtxError instead.  The classes' pointwise methods (CubicSpline1D / CubicSpline2D.calc_position(s) at a
caller's s) are not carried."""
from . import spline as _sp

_spline = None


def calc_spline_course(x, y, ds=0.1):
    global _spline
    if _spline is None:
        _spline = _sp.BatchSpline()
    return _spline.run([(x, y)], ds=ds, solve="numpy").course(0)


__all__ = ['calc_spline_course']

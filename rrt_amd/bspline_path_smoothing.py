"""Names of the reference's 10_path_planning_00_bspline_path.py as its driver cell uses them, the smoothing fit included:
approximate_b_spline_path :12-56 for any s -- s=None (the script's default, s = len(x)), the driver's s=0.5, s=0.0 --,
interpolate_b_spline_path :59-88, plot_curvature :115-148.
The MI355X mirror: every call is a batch of one on robotics-path-planning_amd/bspline.py (BatchBSpline.approximate: FITPACK's
adaptive knot insertion and root search on the smoothing parameter, restated on the device); no CPU fallback, no
scipy, no matplotlib.

Which module does what: rrt_amd.bspline_path is the interpolating half and raises NotImplementedError for s other than 0.0;
this module is the whole script.  interpolate_b_spline_path and plot_curvature here are that module's own.  Where scipy warns
that the root search stopped early, this module warns too (RuntimeWarning) and returns the same last approximation."""
from . import bspline_path as _bp
from .bspline_path import interpolate_b_spline_path, plot_curvature


def approximate_b_spline_path(x, y, n_path_points, degree=3, s=None):
    return _bp._batch().approximate([(x, y)], int(n_path_points), degree=int(degree), s=None if s is None else float(s)).course(0)


__all__ = ['approximate_b_spline_path', 'interpolate_b_spline_path', 'plot_curvature']

"""Names of the reference's 10_path_planning_00_bspline_path.py as its driver cell uses them: approximate_b_spline_path :12-56,
interpolate_b_spline_path :59-88, _calc_distance_vector :91-96, _evaluate_spline :99-108, plot_curvature :115-148.
The MI355X mirror: every call is a batch of one on robotics-path-planning_amd/bspline.py; no CPU fallback, no scipy.

Interpolation only.  The smoothing fit -- approximate_b_spline_path with s other than 0.0, s=None (the script's default, meaning
s = len(x)) included -- is FITPACK's adaptive knot insertion with a root search on the smoothing parameter; this module does not
serve it: such a call raises NotImplementedError here.
s=0.0 is the interpolation.  The curvature keeps the script's exponent 2.0 / 3.0 (:107).  Degree 1, where the script raises in
derivative(2), returns a zero curvature.  plot_curvature is refused: nothing is drawn, and no matplotlib is imported.

Which module does what: this module is the interpolating half and keeps refusing s other than 0.0; rrt_amd.bspline_path_smoothing
is the whole script, its approximate_b_spline_path running the smoothing fit on the device (BatchBSpline.approximate)."""
import numpy as np

from . import bspline as _bs

_handle = None


def _batch():
    global _handle
    if _handle is None:
        _handle = _bs.BatchBSpline()
    return _handle


class _Axis:
    """What stands in for the script's UnivariateSpline objects spl_i_x / spl_i_y: one axis of an interpolating course"""

    def __init__(self, x, y, degree, axis):
        self.x, self.y, self.degree, self.axis = x, y, degree, axis


def _calc_distance_vector(x, y):
    chords = [np.hypot(a, b) for a, b in zip(np.diff(x), np.diff(y))]
    total = np.concatenate(([0.0], np.cumsum(chords)))
    total /= total[-1]
    return total


def _evaluate_spline(sampled, spl_i_x, spl_i_y):
    """(x, y, heading, curvature) at the parameters `sampled` of the course the two axes belong to"""
    if spl_i_x.x is not spl_i_y.x or spl_i_x.degree != spl_i_y.degree:
        raise ValueError("_evaluate_spline: the two axes belong to different courses")
    res = _batch().interpolate([(spl_i_x.x, spl_i_x.y)], degree=spl_i_x.degree, u=[np.asarray(sampled, dtype=np.float64)])
    return res.course(0)


def approximate_b_spline_path(x, y, n_path_points, degree=3, s=None):
    if s is None or float(s) != 0.0:
        raise NotImplementedError("approximate_b_spline_path: the smoothing fit (s != 0.0; s=None means s = len(x)) is FITPACK's "
                                  "adaptive knot insertion and has no device counterpart; only s=0.0, the interpolation, is provided")
    return _batch().interpolate([(x, y)], int(n_path_points), degree=int(degree)).course(0)


def interpolate_b_spline_path(x, y, n_path_points, degree=3):
    return approximate_b_spline_path(x, y, n_path_points, degree, s=0.0)


def plot_curvature(x_list, y_list, heading_list, curvature, k=0.01, c="-c", label="Curvature"):
    raise ValueError("plot_curvature: nothing is drawn here; draw the arrays interpolate_b_spline_path returns")


__all__ = ['approximate_b_spline_path', 'interpolate_b_spline_path', 'plot_curvature']

"""Names of the reference's 10_path_planning_00_spline_2d.py as its driver cell uses them: Spline2D :12-28 with .s, .ds and
calc_position(s).  The MI355X mirror: every calc_position call is a batch of one on robotics-path-planning_amd/bspline.py with
the sample parameters handed over as data; no CPU fallback, no scipy.  .s and .ds are numpy's own statements of the script, made
on the host when the object is built.  The linear kind returns interp1d's doubles bit for bit, the quadratic and cubic kinds
agree with scipy to rounding.  Outside [0, s[-1]] calc_position raises ValueError, as interp1d does.  The
attributes sx / sy (scipy's interp1d objects) are not carried."""
import numpy as np

from . import bspline as _bs

_handle = None


class Spline2D:

    def __init__(self, x, y, kind="cubic"):
        if kind not in _bs.KINDS:
            raise NotImplementedError("Spline2D: kind is 'linear', 'quadratic' or 'cubic', not %r" % (kind,))
        self.kind = kind
        self._x, self._y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self.ds = np.hypot(np.diff(x), np.diff(y))          # the chords, and their running sum from 0.0 as a list
        self.s = [0.0] + list(np.cumsum(self.ds))
        if len(self._x) <= _bs.KINDS[kind]:
            raise ValueError("Spline2D: kind %r needs more than %d waypoints" % (kind, _bs.KINDS[kind]))
        if not np.all(np.diff(self.s) > 0.0):
            raise ValueError("Spline2D: two consecutive waypoints coincide")

    def calc_position(self, s):
        """(x, y) at s, a scalar or an array: arrays of s's shape"""
        global _handle
        q = np.asarray(s, dtype=np.float64)
        flat = q.reshape(-1)
        if len(flat) and np.min(flat) < self.s[0]:
            raise ValueError("A value (%r) in x_new is below the interpolation range's minimum value (%r)."
                             % (float(np.min(flat)), float(self.s[0])))
        if len(flat) and np.max(flat) > self.s[-1]:
            raise ValueError("A value (%r) in x_new is above the interpolation range's maximum value (%r)."
                             % (float(np.max(flat)), float(self.s[-1])))
        if _handle is None:
            _handle = _bs.BatchBSpline()
        res = _handle.spline2d([(self._x, self._y)], ds=None, kind=self.kind, u=[flat])
        res._raise_for(0, "Spline2D.calc_position")
        return res.x.reshape(q.shape), res.y.reshape(q.shape)


__all__ = ['Spline2D']

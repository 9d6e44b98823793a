"""Names of the reference's 10_path_planning_00_cubic_spline_path.py as its driver cells use them: CubicSpline1D :14-173,
CubicSpline2D :176-310, calc_spline_course :313-325.
The MI355X mirror: batches of one on robotics-path-planning_amd/spline.py with solve="numpy" -- the host makes the spline
coefficient c with np.linalg.solve exactly as the reference does, the device does the rest -- so a driver cell sees the
reference's values on its own host; no CPU fallback.  Coinciding consecutive waypoints (equal consecutive knots), where the
reference divides by zero and returns inf / nan, raise RrtxError instead.

The classes' pointwise methods take a scalar and return what the reference returns: None (CubicSpline2D.calc_position: (None,
None)) outside the knots, IndexError("list index out of range") on the last knot and for NaN, TypeError from calc_yaw /
calc_curvature outside the knots (the reference does arithmetic on None there).  They also take an array of parameters,
answered by one kernel launch; there the three failure cases come back as NaN and nothing is raised.  Every scalar call is a
device call: a loop over many parameters is what the array form (or BatchSpline.query) is for."""
import numpy as np

from . import _abi
from . import spline as _sp

_spline = None
_owner = None   # the object whose fit the shared handle holds


def _handle():
    global _spline
    if _spline is None:
        _spline = _sp.BatchSpline()
    return _spline


def calc_spline_course(x, y, ds=0.1):
    global _owner
    _owner = None
    return _handle().run([(x, y)], ds=ds, solve="numpy").course(0)


def _coefficients(h, a, c):
    """b and d of CubicSpline1D.__init__ :68-73"""
    b, d = [], []
    for i in range(len(a) - 1):
        d.append((c[i + 1] - c[i]) / (3.0 * h[i]))
        b.append(1.0 / h[i] * (a[i + 1] - a[i]) - h[i] / 3.0 * (2.0 * c[i] + c[i + 1]))
    return b, d


class _Fitted:
    """A batch of one on the module's handle: fitted again when another object has used the handle since."""

    def _fit(self):
        raise NotImplementedError

    def _claim(self):
        global _owner
        if _owner is not self:
            _owner = None
            res = self._fit()
            if int(res.status[0]) == _abi.SPLINE_DEGENERATE:
                raise _abi.RrtxError("%s: two consecutive knots coincide (the reference divides by zero)" % type(self).__name__)
            _owner = self
            self._last = None
            return res
        return None

    def _ask(self, t):
        """(the SplineQueryResult of t with derivatives, scalar?)"""
        scalar = np.ndim(t) == 0
        ta = np.ascontiguousarray([t] if scalar else t, dtype=np.float64).reshape(-1)
        self._claim()
        key = ta.tobytes() if scalar else None
        if scalar and self._last is not None and self._last[0] == key:
            return self._last[1], True   # calc_position, calc_yaw and calc_curvature of one parameter: one device call
        res = _handle().query([ta], derivatives=True)
        self._last = (key, res) if scalar else None
        return res, scalar

    @staticmethod
    def _scalar(res, planes):
        """What the reference returns or raises for one parameter: the planes' values, None outside, IndexError"""
        st = int(res.status[0])
        if st == _abi.SPLINE_Q_REF_RAISES:
            raise IndexError("list index out of range")   # self.b[i] at the last knot (:93)
        if st != _abi.SPLINE_Q_OK:
            return None
        return tuple(getattr(res, p)[0] for p in planes)


class CubicSpline1D(_Fitted):
    """CubicSpline1D(x, y) of the reference: x ascending.  Attributes x, y, nx, a, b, c, d as the reference keeps them."""

    def __init__(self, x, y):
        h = np.diff(x)
        if np.any(h < 0):
            raise ValueError("x coordinates must be sorted in ascending order")
        self.x = x
        self.y = y
        self.nx = len(x)
        self.a = [iy for iy in y]
        self._last = None
        self.c = self._claim().c[0]
        self.b, self.d = _coefficients(h, self.a, self.c)

    def _fit(self):
        return _handle().fit1d([self.x], [self.y], solve="numpy")

    def _method(self, x, plane):
        res, scalar = self._ask(x)
        if not scalar:
            return getattr(res, plane).reshape(np.shape(x))
        v = self._scalar(res, (plane,))
        return None if v is None else v[0]

    def calc_position(self, x):
        return self._method(x, "y")

    def calc_first_derivative(self, x):
        return self._method(x, "dy")

    def calc_second_derivative(self, x):
        return self._method(x, "ddy")


class _Axis:
    """sx / sy of a CubicSpline2D: CubicSpline1D(s, x) / CubicSpline1D(s, y) answered from the 2-D fit on the device"""

    def __init__(self, parent, knots, values, c, planes):
        self._parent = parent
        self._planes = planes
        self.x = knots
        self.y = values
        self.nx = len(knots)
        self.a = [v for v in values]
        self.c = c
        self.b, self.d = _coefficients(np.diff(knots), self.a, c)

    def _method(self, s, plane):
        res, scalar = self._parent._ask(s)
        if not scalar:
            return getattr(res, plane).reshape(np.shape(s))
        v = _Fitted._scalar(res, (plane,))
        return None if v is None else v[0]

    def calc_position(self, x):
        return self._method(x, self._planes[0])

    def calc_first_derivative(self, x):
        return self._method(x, self._planes[1])

    def calc_second_derivative(self, x):
        return self._method(x, self._planes[2])


class CubicSpline2D(_Fitted):
    """CubicSpline2D(x, y) of the reference.  Attributes s, ds, sx, sy as the reference keeps them; sx and sy are views
    over the one 2-D fit on the device."""

    def __init__(self, x, y):
        self._x, self._y = x, y
        self.ds = np.hypot(np.diff(x), np.diff(y))   # __calc_s :240-246
        self.s = [0]
        self.s.extend(np.cumsum(self.ds))
        self._last = None
        cx, cy = self._claim().c
        self.sx = _Axis(self, self.s, x, cx, ("x", "dx", "ddx"))
        self.sy = _Axis(self, self.s, y, cy, ("y", "dy", "ddy"))

    def _fit(self):
        return _handle().fit([(self._x, self._y)], solve="numpy")

    def calc_position(self, s):
        res, scalar = self._ask(s)
        if not scalar:
            return res.x.reshape(np.shape(s)), res.y.reshape(np.shape(s))
        v = self._scalar(res, ("x", "y"))
        return (None, None) if v is None else v

    def calc_curvature(self, s):
        res, scalar = self._ask(s)
        if not scalar:
            return res.k.reshape(np.shape(s))
        v = self._scalar(res, ("k",))
        if v is None:   # ddy * dx on two None (:289)
            raise TypeError("unsupported operand type(s) for *: 'NoneType' and 'NoneType'")
        return v[0]

    def calc_yaw(self, s):
        res, scalar = self._ask(s)
        if not scalar:
            return res.yaw.reshape(np.shape(s))
        v = self._scalar(res, ("yaw",))
        if v is None:   # math.atan2(None, None) (:309)
            raise TypeError("must be real number, not NoneType")
        return v[0]


# tests/test_spline_host.py pins this list; the two classes are imported by name
__all__ = ['calc_spline_course']

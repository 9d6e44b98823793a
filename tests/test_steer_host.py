"""Batched Dubins / Reeds-Shepp steer (rrtx_steer_*, BatchSteer, the two drop-in modules): everything that can be checked
without a device -- the ABI surface, the argument checks made before any HIP call, the reference's signatures, and that
there is no CPU fallback."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import util

STEER_FUNCS = ("rrtx_steer_create", "rrtx_steer_destroy", "rrtx_steer_last_error", "rrtx_steer_solve",
               "rrtx_steer_get_counts", "rrtx_steer_get_summary", "rrtx_steer_get_points", "rrtx_steer_get_kernel_ms")


def test_steer_entry_points_declared_exported_and_bound():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION == 6
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    assert L.rrtx_abi_version() == 6
    for fn in STEER_FUNCS:
        assert re.search(r"\b%s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None, fn
    vals = dict(re.findall(r"#define (RRTX_STEER_[A-Z_]+) (\d+)", hdr))
    assert {k: int(v) for k, v in vals.items()} == {
        "RRTX_STEER_DUBINS": A.STEER_DUBINS, "RRTX_STEER_RS": A.STEER_RS, "RRTX_STEER_OK": A.STEER_OK,
        "RRTX_STEER_NO_PATH": A.STEER_NO_PATH, "RRTX_STEER_RAISES_ZERODIV": A.STEER_RAISES_ZERODIV,
        "RRTX_STEER_RAISES_VALUE": A.STEER_RAISES_VALUE}
    assert A.DUBINS_WORDS == ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")


@pytest.fixture()
def steer_obj():
    """A raw rrtx_steer*: handed out with or without a device, so that the argument checks can be reached."""
    import rrt_amd
    L = rrt_amd._abi.load()
    s = C.c_void_p()
    rc = L.rrtx_steer_create(0, C.byref(s))
    assert rc in (0, -2) and s.value
    if rc == -2:
        assert L.rrtx_steer_last_error(s)
    yield L, s
    L.rrtx_steer_destroy(s)


P2 = np.zeros((2, 3))
G2 = np.ones((2, 3))
CV = np.ones(1)
BASE = dict(kind=0, product=0, n=2, ng=0, starts=P2, goals=G2, curv=CV, per_pair=0, step=0.1, order=None, n_words=0, points=1)
INVALID = {
    "null_object": dict(obj=None),
    "null_starts": dict(starts=None),
    "null_goals": dict(goals=None),
    "null_curvature": dict(curv=None),
    "negative_n": dict(n=-1),
    "negative_ng_in_product": dict(product=1, ng=-1),
    "unknown_kind": dict(kind=2),
    "negative_kind": dict(kind=-1),
    "dubins_step_zero": dict(step=0.0),
    "rs_step_zero": dict(kind=1, step=0.0),
    "rs_step_negative": dict(kind=1, step=-0.2),
    "rs_step_nan": dict(kind=1, step=float("nan")),
    "dubins_step_not_default": dict(step=0.2),
    "word_index_6": dict(order=np.array([0, 6], dtype=np.int32), n_words=2),
    "word_index_negative": dict(order=np.array([-1], dtype=np.int32), n_words=1),
    "seven_words": dict(order=np.zeros(7, dtype=np.int32), n_words=7),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_call(steer_obj, case):
    L, s = steer_obj
    kw = dict(BASE)
    kw.update(INVALID[case])
    obj = kw.pop("obj", s)

    def ptr(a):
        return None if a is None else a.ctypes.data
    rc = L.rrtx_steer_solve(obj, kw["kind"], kw["product"], kw["n"], kw["ng"], ptr(kw["starts"]), ptr(kw["goals"]),
                            ptr(kw["curv"]), kw["per_pair"], kw["step"], ptr(kw["order"]), kw["n_words"], kw["points"])
    assert rc == -1, (case, rc)   # RRTX_E_INVALID
    assert len(L.rrtx_steer_last_error(obj)) > 0, case


def test_dropin_modules_have_the_reference_signatures():
    import rrt_amd.dubins_path as dp
    import rrt_amd.reeds_shepp_path as rp
    assert dp.__all__ == ["plan_dubins_path"] and rp.__all__ == ["reeds_shepp_path_planning"]
    assert str(inspect.signature(dp.plan_dubins_path)) == \
        "(s_x, s_y, s_yaw, g_x, g_y, g_yaw, curvature, step_size=0.1, selected_types=None)"
    assert str(inspect.signature(rp.reeds_shepp_path_planning)) == "(sx, sy, syaw, gx, gy, gyaw, maxc, step_size=0.2)"


def test_unknown_dubins_word_is_a_key_error():
    import rrt_amd.dubins_path as dp
    with pytest.raises(KeyError):
        dp.plan_dubins_path(0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, selected_types=["LSL", "XYZ"])


def test_no_cpu_fallback_for_the_curves():
    """Without a device the drop-in calls raise RrtxError and return no path."""
    import rrt_amd
    import rrt_amd.dubins_path as dp
    import rrt_amd.reeds_shepp_path as rp
    if rrt_amd._abi.load().rrtx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(rrt_amd._abi.RrtxError):
        dp.plan_dubins_path(1.0, 1.0, 0.7, -3.0, -3.0, -0.7, 1.0)
    with pytest.raises(rrt_amd._abi.RrtxError):
        rp.reeds_shepp_path_planning(-1.0, -4.0, -0.3, 5.0, 5.0, 0.4, 0.1, 0.05)
    with pytest.raises(rrt_amd._abi.RrtxError):
        rrt_amd.BatchSteer("rs")

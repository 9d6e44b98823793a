"""BatchSteer's obstacle check (rrtx_steer_set_obstacles / rrtx_steer_get_hits, BatchSteer.plan(obstacle_list=...)):
everything that can be checked without a device -- the ABI surface, the argument checks made before any HIP call, the call
order, that an empty list changes nothing, and the scalar piece of the kernel's check (csrc/rpp_collide.h) compiled for
the host, under AddressSanitizer and UndefinedBehaviorSanitizer, against the reference's own answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import util
import steer_collide_util as scu

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
NEW_FUNCS = ("rrtx_steer_set_obstacles", "rrtx_steer_get_hits")
E_INVALID, E_STATE = -1, -5


def test_entry_points_declared_exported_and_bound():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    assert L.rrtx_abi_version() == A.RRTX_ABI_VERSION == int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1))
    for fn in NEW_FUNCS:
        assert re.search(r"\bint %s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None and getattr(L, fn).restype is C.c_int, fn
    assert len(L.rrtx_steer_set_obstacles.argtypes) == 4 and L.rrtx_steer_set_obstacles.argtypes[2] is C.c_int64
    assert L.rrtx_steer_set_obstacles.argtypes[3] is C.c_double and len(L.rrtx_steer_get_hits.argtypes) == 2
    assert callable(A.Steer.set_obstacles) and callable(A.Steer.hits)


@pytest.fixture()
def steer_obj():
    """A raw rrtx_steer*: handed out with or without a device, so that the argument checks can be reached."""
    import rrt_amd
    L = rrt_amd._abi.load()
    s = C.c_void_p()
    rc = L.rrtx_steer_create(0, C.byref(s))
    assert rc in (0, -2) and s.value
    yield L, s
    L.rrtx_steer_destroy(s)


OB2 = np.array([[1.0, 2.0, 0.5], [3.0, 4.0, 0.25]])


def with_entry(i, v):
    a = OB2.copy()
    a.reshape(-1)[i] = v
    return a


INVALID = {
    "null_object": dict(obj=None),
    "negative_m": dict(m=-1),
    "m_above_2_20": dict(ob=np.zeros(((1 << 20) + 1, 3)), m=(1 << 20) + 1),
    "null_array": dict(ob=None, m=2),
    "nan_x": dict(ob=with_entry(0, float("nan"))),
    "inf_y": dict(ob=with_entry(4, float("inf"))),
    "nan_size": dict(ob=with_entry(5, float("nan"))),
    "minus_inf_size": dict(ob=with_entry(2, float("-inf"))),
    "nan_radius": dict(rr=float("nan")),
    "inf_radius": dict(rr=float("inf")),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_obstacles_are_refused_before_any_device_call(steer_obj, case):
    L, s = steer_obj
    kw = dict(obj=s, ob=OB2, m=2, rr=0.0)
    kw.update(INVALID[case])
    rc = L.rrtx_steer_set_obstacles(kw["obj"], None if kw["ob"] is None else kw["ob"].ctypes.data, kw["m"], kw["rr"])
    assert rc == E_INVALID, (case, rc)
    assert len(L.rrtx_steer_last_error(kw["obj"])) > 0, case


def test_valid_lists_are_accepted_without_a_device(steer_obj):
    """A negative size (the reference squares it), a NULL array with m == 0, and 2^20 rows: all taken, copied, no HIP call."""
    L, s = steer_obj
    neg = np.array([[1.0, 2.0, -0.5]])
    assert L.rrtx_steer_set_obstacles(s, neg.ctypes.data, 1, 0.25) == 0
    assert L.rrtx_steer_set_obstacles(s, None, 0, 0.0) == 0
    big = np.zeros((1 << 20, 3))
    assert L.rrtx_steer_set_obstacles(s, big.ctypes.data, 1 << 20, 0.0) == 0
    del big
    assert L.rrtx_steer_set_obstacles(s, OB2.ctypes.data, 2, 0.0) == 0


def test_get_hits_before_any_solve_is_a_state_error(steer_obj):
    L, s = steer_obj
    hit = np.zeros(4, dtype=np.int32)
    assert L.rrtx_steer_get_hits(s, hit.ctypes.data) == E_STATE and len(L.rrtx_steer_last_error(s)) > 0
    assert L.rrtx_steer_set_obstacles(s, OB2.ctypes.data, 2, 0.0) == 0
    assert L.rrtx_steer_get_hits(s, hit.ctypes.data) == E_STATE      # a list alone is no solve
    assert L.rrtx_steer_get_hits(None, hit.ctypes.data) == E_INVALID


class FakeSteer:
    """Stands in for _abi.Steer: records what BatchSteer.plan asks of it."""

    def __init__(self):
        self.calls = []
        self.n_obstacles = 0

    def set_obstacles(self, ob, rr=0.0):
        self.calls.append(("set_obstacles", len(ob), rr))
        self.n_obstacles = len(ob)

    def solve(self, *a, **kw):
        self.calls.append(("solve",))
        return 0

    def summary(self, offsets=True):
        self.calls.append(("summary",))
        z = np.zeros(2)
        return (np.zeros(2, dtype=np.int32), z, np.full(2, 3, dtype=np.int32), np.ones((2, 5)), np.array([b"LSL", b"RSR"]),
                np.array([0, 1, 2], dtype=np.int64) if offsets else None)

    def points(self):
        self.calls.append(("points",))
        return np.zeros(2), np.zeros(2), np.zeros(2)

    def hits(self):
        self.calls.append(("hits",))
        return np.array([-1, 0], dtype=np.int32)

    def kernel_ms(self):
        return 0.0


def fake_batch_steer():
    import rrt_amd
    bs = object.__new__(rrt_amd.BatchSteer)
    bs.kind = rrt_amd._abi.STEER_DUBINS
    bs._steer = FakeSteer()
    return bs


@pytest.mark.parametrize("empty", [None, [], (), np.zeros((0, 3))], ids=["none", "list", "tuple", "array"])
def test_plan_with_an_empty_list_takes_the_path_without_a_check(empty):
    import rrt_amd
    bs = fake_batch_steer()
    st, go = np.zeros((2, 3)), np.ones((2, 3))
    res = bs.plan(st, go, 1.0, obstacle_list=empty, robot_radius=0.4)
    assert [c[0] for c in bs._steer.calls] == ["solve", "summary", "points"]      # what plan() did before the check existed
    assert res.hit is None
    with pytest.raises(rrt_amd._abi.RrtxError):
        res.free
    with pytest.raises(rrt_amd._abi.RrtxError):
        res.is_free(0)
    with pytest.raises(rrt_amd._abi.RrtxError):
        bs.plan(st, go, 1.0, obstacle_list=empty, product=True).length_matrix(free_only=True)


def test_plan_with_a_list_sets_it_reads_hits_and_clears_it_again():
    bs = fake_batch_steer()
    st, go = np.zeros((2, 3)), np.ones((2, 3))
    res = bs.plan(st, go, 1.0, points=False, obstacle_list=[(1, 2, 0.5)], robot_radius=0.25)
    assert bs._steer.calls == [("set_obstacles", 1, 0.25), ("solve",), ("summary",), ("hits",)]
    assert res.hit.tolist() == [-1, 0] and res.free.tolist() == [True, False]
    assert res.is_free(0) is True and res.is_free(1) is False
    bs._steer.calls.clear()
    res = bs.plan(st, go, 1.0, points=False)
    assert bs._steer.calls == [("set_obstacles", 0, 0.0), ("solve",), ("summary",)] and res.hit is None   # the list is cleared
    bs._steer.calls.clear()
    bs.plan(st, go, 1.0, points=False)
    assert bs._steer.calls == [("solve",), ("summary",)]


def test_steer_result_keeps_its_positional_constructor_and_masks_the_matrix():
    import rrt_amd
    from importlib import import_module
    SR = import_module("robotics-path-planning_amd.steer").SteerResult
    args = (0, np.array([0, 0, 1, 0], dtype=np.int32), np.array([1.0, 2.0, 0.0, 4.0]), np.array([3, 3, 0, 3], dtype=np.int32),
            np.ones((4, 5)), np.array([b"LSL", b"RSR", b"", b"LSR"]), None, None, (2, 2), 1, 0.0)
    old = SR(*args)
    assert old.hit is None and np.array_equal(old.length_matrix(), [[1.0, 2.0], [0.0, 4.0]])
    new = SR(*args, hit=np.array([-1, 3, -2, -1], dtype=np.int32))
    assert new.free.tolist() == [True, False, False, True]
    assert np.array_equal(new.length_matrix(), old.length_matrix())
    assert np.array_equal(new.length_matrix(free_only=True), [[1.0, np.inf], [np.inf, 4.0]])
    with pytest.raises(TypeError):       # Dubins, no feasible word: what path(i) raises
        new.is_free(2)
    rs = SR(1, *args[1:], hit=np.array([-1, 3, -2, -1], dtype=np.int32))
    assert rs.is_free(2) is False and rs.is_free(1) is False and rs.is_free(3) is True   # check_collision(None, ...) is False
    assert rrt_amd.BatchSteer is not None


def test_first_hit_compiled_for_the_host_matches_the_reference(tmp_path):
    """csrc/rpp_collide.h in a program of its own (-ffp-contract=off, ASan + UBSan) over every golden row: the points are
    the C oracle's (bit-identical to the reference's curves), the thresholds Python's (size + robot_radius) ** 2."""
    g = scu.load_kat()
    exe = str(tmp_path / "steer_collide_host_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "steer_collide_host_check.cpp"), "-o", exe], check=True)
    want, recs = [], []
    for kind in ("d", "r"):
        for i, inp in enumerate(g[kind + "_inp"]):
            no_curve = kind == "d" and g["d_nsel"][i] >= 0     # the Dubins row whose word list has no feasible word
            xy = None if no_curve else scu.oracle_curve(kind, inp)
            obs = scu.thresholds(scu.obstacle_list(g, int(g[kind + "_list"][i])), g[kind + "_rr"][i])
            n = -1 if xy is None else len(xy[0])
            recs.append(np.concatenate([[float(len(obs)), float(n)], obs.reshape(-1)] + ([] if xy is None else [xy[0], xy[1]])))
            want.append(int(g[kind + "_hit"][i]))
            if no_curve:
                assert want[-1] == -2
    np.concatenate(recs).astype(np.float64).tofile(str(tmp_path / "records.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")   # (the leak pass at exit needs ptrace, which a container may forbid)
    out = subprocess.run([exe, str(tmp_path / "records.bin")], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert out.stderr == b"", out.stderr.decode()      # a sanitizer report goes there
    got = [int(v) for v in out.stdout.split()]
    assert got == want
    assert want.count(-1) > 10 and want.count(-2) == 2 and want.count(999) == 2 and sum(1 for v in want if v > 0) > 10
    tags = g["d_tag"].tolist() + g["r_tag"].tolist()
    assert tags.count("graze_free") == tags.count("graze_hit") == 8

"""Every candidate curve of a pair and the shortest free one (rrtx_steer_solve_all / _select_free, BatchSteer.candidates /
plan_free, rrt_amd.reeds_shepp_calc_paths): everything that can be checked without a device -- the scalar core compiled for
the host against the reference's calc_paths lists (tests/golden/steer_all_kat.npz, bit for bit), the selection rule on forged
hit vectors, the ABI surface, the argument checks made before any HIP call, and the drop-in module's signatures."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import util

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("RRTX_TEST_SANITIZE") else []
ALL_FUNCS = ("rrtx_steer_solve_all", "rrtx_steer_get_cand_counts", "rrtx_steer_get_cand_summary", "rrtx_steer_get_cand_points",
             "rrtx_steer_select_free")
STATUS = {"": 0, "ZeroDivisionError": 2, "ValueError": 3}   # RRTX_STEER_*; an empty list is RRTX_STEER_NO_PATH


def build_check(builddir):
    exe = os.path.join(builddir, "steer_all_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"] + SAN + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "steer_all_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check(str(tmp_path_factory.mktemp("native")))


@pytest.fixture(scope="module")
def kat():
    g = np.load(os.path.join(util.GOLDEN, "steer_all_kat.npz"))
    return {f: g[f] for f in g.files}


def test_the_golden_set_holds_what_it_must(kat):
    n_cand, off, L = kat["n_cand"], kat["cand_off"], kat["c_L"]
    assert len(n_cand) == len(kat["inp"]) == 77 and off[-1] == len(L) == len(kat["c_mode"]) == 390
    assert np.sum(n_cand == 0) >= 3                                         # pairs with []
    assert {"ZeroDivisionError", "ValueError"} <= set(kat["err"].tolist())  # both exception kinds
    assert np.array_equal(n_cand == -1, kat["err"] != "")
    assert np.sum(kat["too_large"]) >= 1 and np.all(n_cand[kat["too_large"]] == 0)   # "Step size too large" hides the list
    assert np.sum(n_cand >= 10) >= 5
    ties = 0
    for i in range(len(n_cand)):
        ls = sorted(L[off[i]:off[i + 1]].tolist())
        ties += any(a == b for a, b in zip(ls, ls[1:]))
    assert ties >= 10                                                       # two candidates of exactly equal L
    assert set(kat["inp"][:, 6].tolist()) >= {0.1, 0.5, 1.0, 2.0}
    assert kat["c_off"][-1] == len(kat["x"]) == len(kat["y"]) == len(kat["yaw"]) == len(kat["directions"])
    assert kat["directions"].dtype == np.int8 and set(kat["directions"].tolist()) == {1, -1}
    assert os.path.getsize(os.path.join(util.GOLDEN, "steer_all_kat.npz")) < 1000000


def test_scalar_core_against_the_reference_lists(kat, check_exe, tmp_path):
    """Candidate lists in list order, words, lengths, L, every point, yaw and direction -- bit for bit."""
    blob = str(tmp_path / "steer_all_kat.bin")
    with open(blob, "wb") as f:
        for i in range(len(kat["inp"])):
            n = int(kat["n_cand"][i])
            f.write(np.asarray(kat["inp"][i], dtype=np.float64).tobytes())
            f.write(struct.pack("<ii", n, STATUS[str(kat["err"][i])] if n != 0 else 1))
            for c in range(int(kat["cand_off"][i]), int(kat["cand_off"][i + 1])):
                a, b = int(kat["c_off"][c]), int(kat["c_off"][c + 1])
                f.write(str(kat["c_mode"][c]).encode().ljust(8, b"\0"))
                f.write(struct.pack("<ii", int(kat["c_nlen"][c]), b - a))
                f.write(np.asarray(kat["c_lengths"][c], dtype=np.float64).tobytes())
                f.write(np.asarray(kat["c_L"][c], dtype=np.float64).tobytes())
                for key in ("x", "y", "yaw"):
                    f.write(np.asarray(kat[key][a:b], dtype=np.float64).tobytes())
                f.write(np.asarray(kat["directions"][a:b], dtype=np.int8).tobytes())
    r = subprocess.run([check_exe, "kat", blob], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases 77 candidates 390 mismatches 0" in r.stdout


def test_selection_rule_on_forged_hit_vectors(check_exe):
    """Ties, none free, the first free not being the first candidate (the cases are in the native program)."""
    r = subprocess.run([check_exe, "pick"], capture_output=True, text=True)
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout + r.stderr


def test_entry_points_declared_exported_and_bound():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    raw = C.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    L = A.load()
    assert L.rrtx_abi_version() == A.RRTX_ABI_VERSION == 6
    for fn in ALL_FUNCS:
        assert re.search(r"\b%s\(" % fn, hdr), fn
        assert hasattr(raw, fn), fn
        assert fn in A.EXPORTS and getattr(L, fn).argtypes is not None and getattr(L, fn).restype is C.c_int, fn
    assert "10_path_planning_00_reeds_shepp_path.py :483-503" in hdr      # the lines the entry points restate
    assert len(re.findall(r"#define (RRTX_STEER_[A-Z_]+) (\d+)", hdr)) == 6   # no new value under that prefix
    for name in ("solve_all", "cand_counts", "cand_summary", "cand_points", "select_free"):
        assert callable(getattr(A.Steer, name)), name


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


P2 = np.zeros((2, 3))
G2 = np.ones((2, 3))
CV = np.ones(1)
BASE = dict(kind=1, product=0, n=2, ng=0, starts=P2, goals=G2, curv=CV, per_pair=0, step=0.2, order=None, n_words=0, points=1)
FAR = np.array([[0.0, 0.0, 0.0], [1e7, 0.0, 0.0]])
INVALID = {
    "null_object": dict(obj=None),
    "null_starts": dict(starts=None),
    "null_goals": dict(goals=None),
    "null_curvature": dict(curv=None),
    "negative_n": dict(n=-1),
    "negative_ng_in_product": dict(product=1, ng=-1),
    "unknown_kind": dict(kind=2),
    "rs_step_zero": dict(step=0.0),
    "rs_step_nan": dict(step=float("nan")),
    "rs_with_a_word_list": dict(order=np.zeros(1, dtype=np.int32), n_words=1),
    "dubins_step_not_default": dict(kind=0, step=0.2),
    "word_index_6": dict(kind=0, step=0.1, order=np.array([0, 6], dtype=np.int32), n_words=2),
    "word_index_negative": dict(kind=0, step=0.1, order=np.array([-1], dtype=np.int32), n_words=1),
    "seventeen_words": dict(kind=0, step=0.1, order=np.zeros(17, dtype=np.int32), n_words=17),
    "curvature_zero": dict(curv=np.zeros(1)),
    "pose_beyond_1e6": dict(goals=FAR),
    "pose_nan": dict(starts=np.full((2, 3), np.nan)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_refused_before_any_device_call(steer_obj, case):
    L, s = steer_obj
    kw = dict(BASE)
    kw.update(INVALID[case])
    obj = kw.pop("obj", s)

    def ptr(a):
        return None if a is None else a.ctypes.data
    rc = L.rrtx_steer_solve_all(obj, kw["kind"], kw["product"], kw["n"], kw["ng"], ptr(kw["starts"]), ptr(kw["goals"]),
                                ptr(kw["curv"]), kw["per_pair"], kw["step"], ptr(kw["order"]), kw["n_words"], kw["points"])
    assert rc == -1, (case, rc)   # RRTX_E_INVALID
    assert len(L.rrtx_steer_last_error(obj)) > 0, case


def test_sixteen_words_pass_the_checks_and_getters_need_a_solve(steer_obj):
    L, s = steer_obj
    order = np.zeros(16, dtype=np.int32)
    # an empty batch: the checks are made, and no kernel runs with or without a device
    rc = L.rrtx_steer_solve_all(s, 0, 0, 0, 0, P2.ctypes.data, G2.ctypes.data, CV.ctypes.data, 0, 0.1, order.ctypes.data, 16, 0)
    assert rc in (0, -2), rc   # solved, or no device: never RRTX_E_INVALID
    s2 = C.c_void_p()
    assert L.rrtx_steer_create(0, C.byref(s2)) in (0, -2)
    try:   # a fresh object: nothing solved
        n = C.c_int64()
        assert L.rrtx_steer_get_cand_counts(s2, C.byref(n), None, None, None) == -5   # RRTX_E_STATE
        assert L.rrtx_steer_get_cand_summary(s2, *([None] * 11)) == -5
        assert L.rrtx_steer_get_cand_points(s2, None, None, None, None, 0) == -5
        assert L.rrtx_steer_select_free(s2, None, None, None) == -5
        for fn, args in (("rrtx_steer_get_cand_counts", [None] * 4), ("rrtx_steer_get_cand_summary", [None] * 11),
                         ("rrtx_steer_get_cand_points", [None] * 4 + [0]), ("rrtx_steer_select_free", [None] * 3)):
            assert getattr(L, fn)(None, *args) == -1, fn
    finally:
        L.rrtx_steer_destroy(s2)
    assert L.rrtx_steer_select_free(s, None, None, None) == -5   # solved without an obstacle list (or not at all): no hits


def test_python_surface_checks_its_arguments_first():
    """The word list of candidates() keeps repeats; candidates and plan_free take plan()'s arguments for the curve kinds."""
    import rrt_amd
    S = rrt_amd.steer
    assert S.word_list(None) is None and S.word_list(["LSL", "LSL", "RLR"]) == [0, 0, 4]
    assert S.word_order(["LSL", "LSL", "RLR"]) == [0, 4]   # plan() goes on dropping the repeats
    with pytest.raises(KeyError):
        S.word_list(["LSL", "XYZ"])
    names = list(inspect.signature(S.BatchSteer.candidates).parameters)
    assert names == ["self", "starts", "goals", "curvature", "step_size", "selected_types", "points", "product",
                     "obstacle_list", "robot_radius"]
    assert list(inspect.signature(S.BatchSteer.plan_free).parameters) == names
    assert rrt_amd.SteerCandidates is S.SteerCandidates


def test_dropin_module_has_the_reference_signatures():
    import rrt_amd.reeds_shepp_calc_paths as cp
    import rrt_amd.reeds_shepp_path as rp
    assert rp.__all__ == ["reeds_shepp_path_planning"]              # unchanged
    assert cp.__all__ == ["calc_paths", "Path"] and not hasattr(cp, "generate_path")
    assert str(inspect.signature(cp.calc_paths)) == "(sx, sy, syaw, gx, gy, gyaw, maxc, step_size)"
    assert str(inspect.signature(cp.Path.__init__)) == "(self)"
    p = cp.Path()
    assert (p.lengths, p.ctypes, p.L, p.x, p.y, p.yaw, p.directions) == ([], [], 0.0, [], [], [], [])
    import ref_loader
    ref = os.path.join(ref_loader.REF_DIR, "10_path_planning_00_reeds_shepp_path.py")
    if os.path.exists(ref):   # the build host: against the reference's own text
        import ast
        tree = ast.parse(open(ref).read())
        fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "calc_paths"][0]
        assert [a.arg for a in fn.args.args] == list(inspect.signature(cp.calc_paths).parameters) and not fn.args.defaults
        cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Path"][0]
        init = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
        assert [a.arg for a in init.args.args] == ["self"]
        attrs = [t.attr for st in init.body if isinstance(st, ast.Assign) for t in st.targets]
        assert attrs == list(vars(p))


def test_no_cpu_fallback_for_the_candidates():
    import rrt_amd
    import rrt_amd.reeds_shepp_calc_paths as cp
    if rrt_amd._abi.load().rrtx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(rrt_amd._abi.RrtxError):
        cp.calc_paths(-1.0, -4.0, -0.3, 5.0, 5.0, 0.4, 0.1, 0.05)

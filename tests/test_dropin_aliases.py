"""Per-script drop-in modules: `rrt_amd.rrt_01` ... `rrt_amd.rrt_08` expose exactly the names the
reference script of that number defines for its driver cell, bound to the right mirror class, with the script's
constructor keywords and defaults.  CPU only: nothing here touches a device."""
import importlib
import inspect
import json
import math
import os

import pytest

import util

DEG1 = math.radians(1.0)

# (module, reference file, name -> mirror class name, positional ctor args, keyword defaults in order) -- the reference's
# signatures (rrt_01:32, rrt_02:948, rrt_03:1371, rrt_04:951, rrt_05:1358, rrt_06:1467, rrt_07:1029, rrt_08:140)
CASES = [
    ("rrt_01", "10_path_planning_01_rrt_01_simple.py", {"RRT": "RRT"}, ["start", "goal", "obstacle_list", "rand_area"],
     [("expand_dis", 3.0), ("path_resolution", 0.5), ("goal_sample_rate", 5), ("max_iter", 500), ("play_area", None),
      ("robot_radius", 0.0)]),
    ("rrt_02", "10_path_planning_01_rrt_02_sobol_sampler.py", {"RRT": "RRTSobol"},
     ["start", "goal", "obstacle_list", "rand_area"],
     [("expand_dis", 3.0), ("path_resolution", 0.5), ("goal_sample_rate", 5), ("max_iter", 500), ("play_area", None),
      ("robot_radius", 0.0)]),
    ("rrt_03", "10_path_planning_01_rrt_03_dubins_path.py", {"RRT": "RRTDubins"},
     ["start", "goal", "obstacle_list", "rand_area"],
     [("goal_sample_rate", 10), ("max_iter", 200), ("play_area", None), ("robot_radius", 0.0), ("sobol_sampler", False),
      ("curvature", 1.0), ("goal_yaw_th", DEG1), ("goal_xy_th", 0.5)]),
    ("rrt_04", "10_path_planning_01_rrt_04_rrt_star.py", {"RRT": "RRTStar"},
     ["start", "goal", "obstacle_list", "rand_area"],
     [("expand_dis", 3.0), ("path_resolution", 0.5), ("goal_sample_rate", 5), ("max_iter", 500), ("play_area", None),
      ("robot_radius", 0.0), ("sobol_sampler", True), ("connect_circle_dist", 50.0), ("search_until_max_iter", False)]),
    ("rrt_05", "10_path_planning_01_rrt_05_rrt_star_dubins_path.py", {"RRT": "RRTStarDubins"},
     ["start", "goal", "obstacle_list", "rand_area"],
     [("expand_dis", 3.0), ("path_resolution", 0.5), ("goal_sample_rate", 5), ("max_iter", 500), ("play_area", None),
      ("robot_radius", 0.0), ("sobol_sampler", True), ("connect_circle_dist", 50.0), ("search_until_max_iter", False),
      ("curvature", 1.0), ("goal_yaw_th", DEG1), ("goal_xy_th", 0.5)]),
    ("rrt_06", "10_path_planning_01_rrt_06_rrt_star_reeds_shepp_path.py", {"RRT": "RRTStarReedsShepp"},
     ["start", "goal", "obstacle_list", "rand_area"],
     [("expand_dis", 3.0), ("path_resolution", 0.5), ("goal_sample_rate", 5), ("max_iter", 500), ("play_area", None),
      ("robot_radius", 0.0), ("sobol_sampler", True), ("connect_circle_dist", 50.0), ("search_until_max_iter", False),
      ("curvature", 1.0), ("goal_yaw_th", DEG1), ("goal_xy_th", 0.5), ("step_size", 0.2)]),
    ("rrt_07", "10_path_planning_01_rrt_07_informed_rrt_star.py", {"RRT": "InformedRRTStar", "Node": "InformedNode"},
     ["start", "goal", "obstacle_list", "rand_area"],
     [("expand_dis", 0.5), ("goal_sample_rate", 10), ("max_iter", 200), ("sobol_sampler", False)]),
    ("rrt_08", "10_path_planning_01_rrt_08_batch_informed_rrt_star.py", {"BITStar": "BITStar"},
     ["start", "goal", "obstacleList", "randArea"],
     [("eta", 2.0), ("maxIter", 80), ("lowerLimit", None), ("upperLimit", None), ("resolution", 0.01)]),
]
ENTRY = {"rrt_01": "planning", "rrt_02": "planning", "rrt_03": "planning", "rrt_04": "planning", "rrt_05": "planning",
         "rrt_06": "planning", "rrt_07": "informed_rrt_star_search", "rrt_08": "plan"}
FUNCS = {"rrt_01": ["get_path_length", "path_smoothing"], "rrt_02": ["get_path_length", "path_smoothing"],
         "rrt_04": ["get_path_length", "path_smoothing"]}


def _sig(cls):
    ps = list(inspect.signature(cls.__init__).parameters.values())[1:]
    pos = [p.name for p in ps if p.default is inspect.Parameter.empty]
    kw = [(p.name, p.default) for p in ps if p.default is not inspect.Parameter.empty]
    return pos, kw


@pytest.mark.parametrize("mod,ref_file,names,pos,kw", CASES, ids=[c[0] for c in CASES])
def test_alias_module_names_classes_and_defaults(mod, ref_file, names, pos, kw):
    import rrt_amd
    m = importlib.import_module("rrt_amd." + mod)
    for name, mirror in names.items():
        assert getattr(m, name) is getattr(rrt_amd.planner, mirror), (mod, name)
        assert name in m.__all__
    main = getattr(m, "BITStar" if mod == "rrt_08" else "RRT")
    got_pos, got_kw = _sig(main)
    assert got_pos == pos
    # the mirror may add trailing keywords of its own (`device`); the reference's come first, in order, same defaults
    assert [k for k, _ in got_kw[:len(kw)]] == [k for k, _ in kw]
    for (k, v), (_, g) in zip(kw, got_kw):
        assert (g is None and v is None) or g == pytest.approx(v, rel=0, abs=0), (mod, k, g, v)
    assert all(k in ("device",) for k, _ in got_kw[len(kw):])
    assert callable(getattr(main, ENTRY[mod]))
    for f in FUNCS.get(mod, []):
        assert callable(getattr(m, f)) and f in m.__all__


@pytest.mark.parametrize("mod,ref_file,names,pos,kw", CASES, ids=[c[0] for c in CASES])
def test_alias_signatures_equal_the_reference_sources(mod, ref_file, names, pos, kw):
    """The expected table above is itself checked against the reference scripts' interface as recorded from their
    source text (tests/golden/ref_signatures.json, made by oracle/gen_golden_signatures.py: parsed, never imported)."""
    with open(os.path.join(util.GOLDEN, "ref_signatures.json")) as f:
        ref = json.load(f)[mod]
    assert ref["file"] == ref_file
    assert ref["class"] == ("BITStar" if mod == "rrt_08" else "RRT")
    for name in list(names) + FUNCS.get(mod, []):
        assert name in ref["defines"], (mod, name)
    assert ref["init_positional"] == pos
    assert [k for k, _ in ref["init_keywords"]] == [k for k, _ in kw]
    for (k, val), (_, v) in zip(ref["init_keywords"], kw):
        assert val == v, (mod, k, val, v)
    assert ENTRY[mod] in ref["entry_points"]


@pytest.mark.gpu
def test_reference_driver_cell_runs_through_the_alias_modules(gpu):
    """The driver cell of rrt_04 (:1532-1559) with nothing changed but the import: `RRT`, `path_smoothing` and
    `get_path_length` from rrt_amd.rrt_04 reproduce the reference-generated golden; rrt_07's and rrt_08's cells likewise."""
    import random

    import numpy as np
    import util
    from rrt_amd.rrt_04 import RRT, get_path_length, path_smoothing
    obstacleList = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
    g = util.load_golden(util.GOLDEN + "/smooth_drv_s1234.npz")
    random.seed(1234)
    rrt = RRT(start=[0, 0], goal=[6.0, 10.0], rand_area=[-2, 15], obstacle_list=obstacleList, expand_dis=1.0,
              path_resolution=0.1, goal_sample_rate=5, max_iter=500, play_area=[0, 10, 0, 14], robot_radius=0.6,
              sobol_sampler=False, connect_circle_dist=50.0, search_until_max_iter=True)
    path = rrt.planning(animation=False)
    assert np.array_equal(np.array(path), g["path_in"])
    smoothedPath = path_smoothing(path, 1000, obstacleList)
    assert np.array_equal(np.array(smoothedPath), g["smoothed"])
    assert get_path_length(smoothedPath) <= get_path_length(path)

    from rrt_amd.rrt_07 import RRT as RRT7
    g7 = util.load_golden(util.GOLDEN + "/rrt07_drv_mt_s42_it2000.npz")
    kw = util.informed_kwargs_from_golden(g7)
    random.seed(42)
    r7 = RRT7(start=kw["start"], goal=kw["goal"], rand_area=kw["rand_area"], obstacle_list=kw["obstacles"],
              max_iter=2000)                       # expand_dis 0.5, goal_sample_rate 10, sobol_sampler False: the defaults
    p7 = r7.informed_rrt_star_search(animation=False)
    assert (p7 is None) == (len(g7["path"]) == 0)
    if p7 is not None:
        assert np.array_equal(np.array(p7), g7["path"])
    assert [nd.parent for nd in r7.node_list[1:]] == [int(v) for v in g7["parent"][1:]]

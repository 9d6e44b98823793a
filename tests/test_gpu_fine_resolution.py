"""GPU (-m gpu): rrt_04 / rrt_01 at fine path resolutions and away from the origin -- where the libm-free snap decision of
the iteration kernel (rpp::snap_certain) has to know how far n sequential additions drift.

At path_resolution 0.001 an extension walks 3000 steps; the edge back from the nearest node to the new one then measures
3.0 give or take that walk's drift (~4e-11 on a 100 x 100 map), i.e. it sits at the snap limit with more play than the
1e-9 res = 1e-12 the rule allowed itself before it grew with n and the coordinates.  tests/test_snap_rule_host.py counts,
on the CPU, that every seed of the "fine" scene holds at least 3 edges that margin misjudged, at choose_parent and at rewire.
Every case: trees (x, y, cost, parent), paths, result records, RNG state and the decision counters equal the oracle's bit
for bit; the goldens equal the reference's."""
import os

import numpy as np
import pytest

import snap_util as S
import test_gpu_obstacle_map as TM
import util

pytestmark = pytest.mark.gpu

# (RRTX_TPB, RRTX_OBS_CULL): the shapes of the iteration kernel, as tests/test_gpu_graze.py lists them
SHAPES = (("64", "1"), ("64", "0"), ("128", None), ("256", None))


def _check(kw, seeds, what, use_map=False, shape=None):
    out = TM.plan(kw, list(seeds), use_map=use_map)
    if shape is not None:
        assert out["stats"]["main_shape"] == shape, what
    TM.equals_oracle(kw, list(seeds), out, what)
    return out


@pytest.mark.parametrize("tpb,cull", SHAPES)
def test_gpu_fine_scene_on_every_kernel_shape(gpu, monkeypatch, tpb, cull):
    kw, seeds, _ = S.SCENES["fine"]
    monkeypatch.setenv("RRTX_TPB", tpb)
    if cull is None:
        monkeypatch.delenv("RRTX_OBS_CULL", raising=False)
    else:
        monkeypatch.setenv("RRTX_OBS_CULL", cull)
    _check(kw, seeds, "fine, RRTX_TPB=%s RRTX_OBS_CULL=%s" % (tpb, cull), shape=int(tpb))


def test_gpu_fine_scene_without_speculation_and_grid(gpu, monkeypatch):
    kw, seeds, _ = S.SCENES["fine"]
    monkeypatch.setenv("RRTX_TPB", "64")
    monkeypatch.setenv("RRTX_SPEC2", "0")
    monkeypatch.setenv("RRTX_GRID", "0")
    _check(kw, seeds, "fine, RRTX_TPB=64 RRTX_SPEC2=0 RRTX_GRID=0", shape=64)


def test_gpu_fine_scene_on_the_general_kernel(gpu, monkeypatch):
    kw, seeds, _ = S.SCENES["fine"]
    monkeypatch.setenv("RRTX_KERNEL", "v1")
    _check(kw, seeds, "fine, RRTX_KERNEL=v1", shape=256)


@pytest.mark.parametrize("name", ["fineres_rrt04_s5", "fineres_rrt04_s7", "fineres_rrt01_s5", "fineres_rrt04_off1000_s6"])
def test_gpu_fine_goldens_bit_for_bit(gpu, name):
    g = util.load_golden(os.path.join(util.GOLDEN, name + ".npz"))
    kw = util.kwargs_from_golden(g)
    seed = int(g["seed"])
    out = _check(kw, [seed], name)
    util.assert_tree_equal(out["trees"][0], (g["x"], g["y"], g["cost"] if kw["algo"] == "rrt_star" else None, g["parent"]), name)
    assert (out["paths"][0] is None) == (len(g["path"]) == 0)
    if len(g["path"]):
        assert np.array_equal(out["paths"][0], g["path"])
    st = out["rng"][0]
    assert st[1][624] == int(g["rng_pos_after"]) and st[1][0] == int(g["rng_word0_after"])
    assert out["results"][1][0] == len(g["x"])


def test_gpu_fine_scene_through_the_obstacle_map(gpu):
    kw, seeds, _ = S.SCENES["fine"]
    _check(kw, seeds, "fine, obstacle map", use_map=True)


def test_gpu_fine_scene_rrt(gpu):
    kw, seeds, _ = S.SCENES["fine_rrt"]
    out = _check(kw, seeds, "fine, rrt")
    assert all(p is not None for p in out["paths"])


@pytest.mark.parametrize("name", ["offset_1000", "offset_-10100"])
def test_gpu_offset_scenes(gpu, monkeypatch, name):
    """The 16-bit coordinate mirror, the grid index and the collision band's tol at an origin the suite never used."""
    kw, seeds, _ = S.SCENES[name]
    dflt = _check(kw, seeds, name)
    monkeypatch.setenv("RRTX_TPB", "64")
    TM.same(_check(kw, seeds, name + ", RRTX_TPB=64", shape=64), dflt, name + ": 64-thread shape vs default")


def test_gpu_moved_nodes_at_fine_resolution(gpu, monkeypatch):
    """rewire moves nodes on these seeds (tests/test_snap_rule_host.py counts how often), so the back edges are evaluated
    again from the winner's end point -- under the snap rule, 1500 steps to an edge."""
    kw, seeds, _ = S.SCENES["moved"]
    dflt = _check(kw, seeds, "moved nodes, res 0.002")
    monkeypatch.setenv("RRTX_TPB", "64")
    TM.same(_check(kw, seeds, "moved nodes, res 0.002, RRTX_TPB=64", shape=64), dflt, "moved nodes: 64 vs default")

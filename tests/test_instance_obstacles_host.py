"""CPU: per-instance obstacle maps (rrtx_set_instance_obstacles) -- the ABI symbol, the CSR packing of the Python
binding and BatchPlanner's argument checks, none of which needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import util


def test_set_instance_obstacles_is_declared_exported_and_mirrored():
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert re.search(r"int rrtx_set_instance_obstacles\(rrtx_handle\* h, const int32_t\* offsets, const double\* oxyr\);",
                     hdr)
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION == 6
    lib = ctypes.CDLL(os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so"))
    assert hasattr(lib, "rrtx_set_instance_obstacles")
    assert lib.rrtx_abi_version() == 6
    assert "rrtx_set_instance_obstacles" in A.EXPORTS
    assert A.load().rrtx_set_instance_obstacles.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def test_csr_packing_round_trips():
    import rrt_amd
    A = rrt_amd._abi
    lists = [[], util.synth_map(3, 5), [], [(1.5, -2.0, 0.25)], util.synth_map(4, 40), []]
    offsets, oxyr = A.pack_instance_obstacles(lists)
    assert offsets.dtype == np.int32 and oxyr.dtype == np.float64 and oxyr.flags["C_CONTIGUOUS"]
    assert list(offsets) == [0, 0, 5, 5, 6, 46, 46]
    assert oxyr.shape == (46, 3)
    assert A.unpack_instance_obstacles(offsets, oxyr) == [[tuple(map(float, o)) for o in lst] for lst in lists]
    offsets, oxyr = A.pack_instance_obstacles([[], []])
    assert list(offsets) == [0, 0, 0] and oxyr.shape == (0, 3)
    assert A.unpack_instance_obstacles(offsets, oxyr) == [[], []]


def _batch(**kw):
    import rrt_amd
    args = dict(algo="rrt_star", seeds=[1, 2, 3], start=[2, 2], goal=[98, 98], obstacle_list=None, rand_area=[0, 100],
                max_iter=100, search_until_max_iter=True)
    args.update(kw)
    return rrt_amd.BatchPlanner(**args)


def test_batch_planner_rejects_wrong_length_instance_obstacles():
    with pytest.raises(ValueError, match="3 instances"):
        _batch(instance_obstacles=[[], []])
    with pytest.raises(ValueError, match="3 instances"):
        _batch(instance_obstacles=[[], [], [], []], devices=[0, 0])


def test_batch_planner_rejects_both_obstacle_keywords():
    with pytest.raises(ValueError, match="not both"):
        _batch(obstacle_list=[(5, 5, 1)], instance_obstacles=[[], [], []])
    with pytest.raises(ValueError, match="not both"):
        _batch(obstacle_list=[], instance_obstacles=[[], [], []])


def test_csr_packing_rejects_rows_that_are_not_triples():
    import rrt_amd
    A = rrt_amd._abi
    with pytest.raises(ValueError, match="instance 1"):
        A.pack_instance_obstacles([[(1, 2, 3)], [(1, 2), (3, 4), (5, 6)]])
    with pytest.raises(ValueError, match="instance 0"):
        A.pack_instance_obstacles([[(1, 2, 3, 4)]])

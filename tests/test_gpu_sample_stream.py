"""GPU (-m gpu): the sample stream of the rrt_04 iteration kernel (rrt_samples.hip.h).  Every sample of a plan is drawn
before the first iteration launch; the iteration kernel reads sample `it` in iteration `it` and holds no generator.  The
stream equals the host's serial stream bit for bit (rrtx_get_sample_stream), and every path of the kernel that used to draw
-- the three shapes, passes that serve several iterations, forced streaming, resumed launches, a reused handle, the
re-plans -- still equals the oracle.  Scenes and helpers are those of test_gpu_kid_records.py."""
import subprocess

import numpy as np
import pytest

import test_gpu_kid_records as kid
import test_sample_stream_host as host
import util

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(51, 63))   # 12
ITERS = 2000
KNOBS = ("RRTX_TPB", "RRTX_SPEC2", "RRTX_GRID", "RRTX_GRID_MIN", "RRTX_CHUNK_ITERS", "RRTX_PROP_VEC", "RRTX_PROP_CAP")


def _env(monkeypatch, **env):
    for var in KNOBS:
        if env.get(var) is not None:
            monkeypatch.setenv(var, env[var])
        else:
            monkeypatch.delenv(var, raising=False)


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    """The host's serial stream (tests/native/sample_stream_check.cpp, dump mode) of `seeds`: (len(seeds), count, 2) bit patterns."""
    exe = host.build_check(str(tmp_path_factory.mktemp("stream")))

    def run(seeds, rate, sampler, count, lo, hi, gx, gy):
        r = subprocess.run([exe, "dump", ",".join(str(s) for s in seeds), str(rate), str(sampler), str(count), repr(float(lo)),
                            repr(float(hi)), repr(float(gx)), repr(float(gy))], capture_output=True, text=True, check=True)
        v = np.array([int(t, 16) for t in r.stdout.split()], dtype=np.uint64)
        return v.reshape(len(seeds), count, 2)
    return run


def _handle(kw, n, sampler=0):
    import rrt_amd
    A = rrt_amd._abi
    h = A.Handle(A.ALGO_RRT_STAR, kw["start"], kw["goal"], kw["rand_area"], kw["expand_dis"], kw["path_resolution"],
                 kw["goal_sample_rate"], kw["max_iter"], play_area=kw["play_area"], robot_radius=kw["robot_radius"],
                 sampler=sampler, connect_circle_dist=kw["connect_circle_dist"],
                 search_until_max_iter=kw["search_until_max_iter"], n_instances=n)
    h.set_obstacles(kw["obstacles"])
    return h


def _stream_bits(h, n, count):
    return np.stack([h.get_sample_stream(i, 0, count).view(np.uint64) for i in range(n)])


@pytest.mark.parametrize("sampler", [0, 1], ids=["mt", "sobol"])
@pytest.mark.parametrize("rate", [0, 5, 100])
def test_gpu_sample_stream_equals_host_serial_stream(gpu, monkeypatch, serial, sampler, rate):
    """12 instances x 2 000 samples: rrtx_get_sample_stream against the serial generator, bit for bit; a window in the
    middle of the stream reads the same values."""
    _env(monkeypatch, RRTX_TPB="64")
    kw = util.c2_kwargs(ITERS)
    kw["goal_sample_rate"] = rate
    want = serial(SEEDS, rate, sampler, ITERS, kw["rand_area"][0], kw["rand_area"][1], kw["goal"][0], kw["goal"][1])
    h = _handle(kw, len(SEEDS), sampler)
    try:
        h.seed_instances(list(SEEDS))
        h.plan()
        got = _stream_bits(h, len(SEEDS), ITERS)
        mid = h.get_sample_stream(7, 613, 40).view(np.uint64)
        it = h.get_stats()["iterations"]
    finally:
        h.close()
    assert it == len(SEEDS) * ITERS
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "first difference at (instance, sample, coordinate) %s" % (bad[0],)
    assert np.array_equal(mid, want[7, 613:653])


@pytest.mark.parametrize("tpb", ["64", "128", "256"])
def test_gpu_sample_stream_shapes_equal_oracle(gpu, monkeypatch, tpb):
    """C2 at 2 000 iterations, 12 seeds, on each of the three shapes: trees, paths and counters are the oracle's."""
    _env(monkeypatch, RRTX_TPB=tpb, RRTX_GRID_MIN="256")
    out, _, _ = kid._plan(util.c2_kwargs(ITERS), SEEDS)
    kid._equals_oracle(out, [kid._oracle_c2(ITERS, s) for s in SEEDS], "RRTX_TPB=" + tpb)
    if tpb == "64":
        assert out["stats"]["passes_shared"] > 0   # iterations rode on passes that read the samples ahead


@pytest.mark.parametrize("knob", [dict(RRTX_SPEC2="0"), dict(RRTX_GRID="0"), dict(RRTX_GRID_MIN="1000000")],
                         ids=["spec2_off", "grid_off", "grid_min_above_tree"])
def test_gpu_sample_stream_forced_streaming_equals_oracle(gpu, monkeypatch, knob):
    """The same problem with one pass per iteration, without the index, and with the index never reached: the streaming
    passes read their look-ahead samples from the stream too."""
    _env(monkeypatch, RRTX_TPB="64", **knob)
    out, _, _ = kid._plan(util.c2_kwargs(ITERS), SEEDS)
    kid._equals_oracle(out, [kid._oracle_c2(ITERS, s) for s in SEEDS], str(knob))
    if "RRTX_SPEC2" in knob:
        assert out["stats"]["passes_shared"] == 0


def test_gpu_sample_stream_resume_across_launches(gpu, monkeypatch):
    """Launches of 97 iterations equal one launch: the stream is drawn once per plan and indexed by the iteration number
    across launches; the generators' state after the plan is the same."""
    kw = util.c2_kwargs(ITERS)
    res = {}
    for name, chunk in (("one", None), ("chunked", "97")):
        _env(monkeypatch, RRTX_TPB="64", RRTX_GRID_MIN="256", RRTX_CHUNK_ITERS=chunk)
        h = _handle(kw, len(SEEDS))
        try:
            h.seed_instances(list(SEEDS))
            h.plan(strict=True)
            res[name] = dict(stats=h.get_stats(), trees=[h.get_tree(i) for i in range(len(SEEDS))],
                             paths=[h.get_path(i) for i in range(len(SEEDS))], stream=_stream_bits(h, len(SEEDS), ITERS),
                             rng=[h.get_rng_state(i) for i in range(len(SEEDS))])
        finally:
            h.close()
    assert res["chunked"]["stats"]["launches"] >= res["one"]["stats"]["launches"] + 20
    kid._same(res["chunked"], res["one"], "launches of 97 vs one launch", skip=("passes_shared",))
    assert np.array_equal(res["chunked"]["stream"], res["one"]["stream"])
    assert res["chunked"]["rng"] == res["one"]["rng"]   # random.getstate() tuples: 624 words and the position
    kid._equals_oracle(res["chunked"], [kid._oracle_c2(ITERS, s) for s in SEEDS], "launches of 97")


def test_gpu_sample_stream_is_regenerated_on_a_reused_handle(gpu, monkeypatch, serial):
    """Plan, change the seeds, plan, stage the first seeds again, plan: each plan's stream is its own seeds' stream, and
    each plan equals the oracle."""
    _env(monkeypatch, RRTX_TPB="64", RRTX_GRID_MIN="256")
    kw = util.c2_kwargs(ITERS)
    s1, s2 = list(SEEDS), [s + 20 for s in SEEDS]
    n = len(s1)
    want = {tuple(s): serial(s, kw["goal_sample_rate"], 0, ITERS, kw["rand_area"][0], kw["rand_area"][1], kw["goal"][0],
                             kw["goal"][1]) for s in (s1, s2)}
    assert not np.array_equal(want[tuple(s1)], want[tuple(s2)])
    h = _handle(kw, n)
    try:
        for k, seeds in enumerate((s1, s2, s1)):
            h.seed_instances(seeds)
            h.plan(strict=True)
            out = dict(stats=h.get_stats(), trees=[h.get_tree(i) for i in range(n)], paths=[h.get_path(i) for i in range(n)])
            assert np.array_equal(_stream_bits(h, n, ITERS), want[tuple(seeds)]), "plan %d" % k
            kid._equals_oracle(out, [kid._oracle_c2(ITERS, s) for s in seeds], "plan %d" % k)
    finally:
        h.close()


def test_gpu_sample_stream_overflow_replan_equals_oracle(gpu, monkeypatch):
    """The scene of test_gpu_kid_general_kernel_on_the_same_records: near sets outgrow the 64-thread shape, the instances
    are planned again from their staged state on the next shape, which reads a stream drawn again from the same seeds."""
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 10], rand_area=[-2, 15], expand_dis=3.0, path_resolution=0.5, max_iter=700,
              obstacles=kid.DRV_OBSTACLES, robot_radius=0.8)
    _env(monkeypatch, RRTX_TPB="64")
    seeds = list(range(1, 9))
    out, _, _ = kid._plan(kw, seeds)
    assert out["stats"]["near_unique_max"] > 44
    for i, s in enumerate(seeds):
        r = util.run_oracle(kw, s, exact_pow=True)
        util.assert_tree_equal(out["trees"][i], (r["x"], r["y"], r["cost"], r["parent"]), "seed %d" % s)


def test_gpu_sample_stream_moved_node_equals_oracle(gpu, monkeypatch):
    """One moved-node problem of test_gpu_kid_moved_node_equals_oracle (path_resolution 0.05, goal_sample_rate 60): a
    moved node voids the speculated sets in mid-stream; an instance handed to the general kernel draws its own samples."""
    kw = dict(util.C2)
    kw.update(start=[0, 0], goal=[6, 8], rand_area=[-2, 12], obstacles=[(3, 3, 1)], expand_dis=3.0, path_resolution=0.05,
              goal_sample_rate=60, connect_circle_dist=50.0, max_iter=400, robot_radius=0.0)
    r = util.run_oracle(kw, 5, exact_pow=True)
    _env(monkeypatch, RRTX_TPB="64", RRTX_PROP_VEC="0", RRTX_GRID_MIN="0")
    out, _, _ = kid._plan(kw, [5, 1005])
    util.assert_tree_equal(out["trees"][0], (r["x"], r["y"], r["cost"], r["parent"]), "moved-node problem")
    assert (out["paths"][0] is None) == (r["path"] is None)
    if r["path"] is not None:
        assert np.array_equal(out["paths"][0], r["path"])
    assert not (out["results"][2] & 16).any()   # no instance left as UNSUPPORTED

"""Golden generator of LQR-RRT* (rrt_09): runs the reference class itself (loaded through oracle/ref_loader.py, the
rrt_09 file added to ref_loader.FILES at run time) and writes tests/golden/rrt09_*.npz, tests/golden/lqr_kat.npz and
tests/golden/rrt09_signatures.json.  Build host only (needs the reference checkout).

    python tools/gen_golden_lqr.py            # every configuration below
"""
import inspect
import io
import json
import math
import os
import random
import sys
import contextlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_loader  # noqa: E402

ref_loader.FILES["rrt_09"] = "10_path_planning_01_rrt_09_lqr_rrt_star.py"
GOLD = os.path.join(ROOT, "tests", "golden")

DRIVER_OBS = [(5, 5, 1), (3, 6, 2), (3, 8, 2), (3, 10, 2), (7, 5, 2), (9, 5, 2), (8, 10, 1)]
DRIVER = dict(start=[0, 0], goal=[6.0, 10.0], obstacle_list=DRIVER_OBS, rand_area=[-2, 15], expand_dis=3.0,
              path_resolution=0.5, goal_sample_rate=10, max_iter=500, play_area=None, robot_radius=0.0,
              sobol_sampler=True, connect_circle_dist=50.0, search_until_max_iter=False, curvature=1.0,
              goal_xy_th=0.5, step_size=0.2)


def bits(v):
    return np.array(v, dtype=np.float64).view(np.uint64)


def run_plan(mod, kw, seed, until_max=True, smooth_iter=1000):
    ref_loader.reset_sobol(mod)
    random.seed(seed)
    rrt = mod.LQRRRTStar(**kw)
    trace = []
    orig_nearest = rrt.get_nearest_node_index

    def nearest(node_list, rnd):
        i = orig_nearest(node_list, rnd)
        trace.append([float(rnd.x), float(rnd.y), i, -1])
        return i
    orig_near = rrt.find_near_nodes

    def near(new_node):
        r = orig_near(new_node)
        trace[-1][3] = len(r)
        return r
    rrt.get_nearest_node_index = nearest
    rrt.find_near_nodes = near
    with contextlib.redirect_stdout(io.StringIO()):
        path = rrt.planning(animation=False, search_until_max_iter=until_max)
    st = random.getstate()
    nodes = rrt.node_list
    idx = {id(nd): i for i, nd in enumerate(nodes)}
    out = dict(seed=seed, until_max=int(until_max), x=np.array([float(n.x) for n in nodes]),
               y=np.array([float(n.y) for n in nodes]), cost=np.array([float(n.cost) for n in nodes]),
               parent=np.array([idx[id(n.parent)] if n.parent is not None else -1 for n in nodes], dtype=np.int32),
               plen=np.array([len(n.path_x) for n in nodes], dtype=np.int32),
               px=np.array([float(v) for n in nodes for v in n.path_x]),
               py=np.array([float(v) for n in nodes for v in n.path_y]),
               mt_after=np.array(st[1][:624], dtype=np.uint32), mt_pos_after=st[1][624],
               sobol_index=rrt.sobol_inter_,
               tr_rx=np.array([t[0] for t in trace]), tr_ry=np.array([t[1] for t in trace]),
               tr_nearest=np.array([t[2] for t in trace], dtype=np.int32),
               tr_nnear=np.array([t[3] for t in trace], dtype=np.int32))
    out["path"] = np.zeros((0, 2)) if path is None else np.array(path, dtype=np.float64)
    if path is not None:
        sp = mod.path_smoothing(path, smooth_iter, kw["obstacle_list"])
        st2 = random.getstate()
        out["smoothed"] = np.array(sp, dtype=np.float64)
        out["mt_after_smooth"] = np.array(st2[1][:624], dtype=np.uint32)
        out["mt_pos_after_smooth"] = st2[1][624]
        out["smooth_iter"] = smooth_iter
    return out


def save_plan(name, kw, res):
    d = dict(res)
    d["kwargs"] = json.dumps(kw)
    np.savez_compressed(os.path.join(GOLD, "rrt09_%s.npz" % name), **d)


def kat(mod, n=300):
    lqr = mod.LQRPlanner()
    A, B = lqr.get_system_model()
    K, X, _ = lqr.dlqr(A, B, np.eye(2), np.eye(1))
    rs = np.random.RandomState(9)
    obj = mod.LQRRRTStar([0, 0], [1, 1], [], [-2, 15])
    rows, wxs, wys, pxs, pys, cls, nw, npt, ends = [], [], [], [], [], [], [], [], []
    for i in range(n):
        f = rs.uniform(-3, 18, 2)
        t = f + rs.uniform(-4, 4, 2) * (10.0 ** rs.randint(-3, 1))
        step = [0.2, 0.1, 0.15, 0.3, 0.25, 0.07][i % 6]
        wx, wy = lqr.lqr_planning(float(f[0]), float(f[1]), float(t[0]), float(t[1]), show_animation=False)
        px, py, cl = obj.sample_path(wx, wy, step)
        rows.append([f[0], f[1], t[0], t[1], step])
        wxs += [float(v) for v in wx]
        wys += [float(v) for v in wy]
        pxs += [float(v) for v in px]
        pys += [float(v) for v in py]
        cls += [float(v) for v in cl]
        nw.append(len(wx))
        npt.append(len(px))
        ends.append([float(px[-1]), float(py[-1]), float(sum(cl))])
    np.savez_compressed(os.path.join(GOLD, "lqr_kat.npz"), rows=np.array(rows), wx=np.array(wxs), wy=np.array(wys),
                        px=np.array(pxs), py=np.array(pys), clen=np.array(cls), nw=np.array(nw, dtype=np.int32),
                        np=np.array(npt, dtype=np.int32), ends=np.array(ends), K=np.array(K, dtype=np.float64),
                        X=np.array(X, dtype=np.float64))


def signatures(mod):
    rec = {}
    for name in ("LQRRRTStar", "path_smoothing", "get_path_length"):
        obj = getattr(mod, name)
        sig = inspect.signature(obj.__init__ if inspect.isclass(obj) else obj)
        rec[name] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                     for p in sig.parameters.values() if p.name != "self"]
    rec["LQRRRTStar.planning"] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                                  for p in inspect.signature(mod.LQRRRTStar.planning).parameters.values()
                                  if p.name != "self"]
    with open(os.path.join(GOLD, "rrt09_signatures.json"), "w") as f:
        json.dump(rec, f, indent=1)


CONFIGS = [
    ("drv_s1", {}, 1, True), ("drv_s2", {}, 2, True), ("drv_s42", {}, 42, True),
    ("mt_s3", dict(sobol_sampler=False), 3, True),
    ("early_s5", {}, 5, False), ("early_mt_s6", dict(sobol_sampler=False), 6, False),
    ("play_s7", dict(play_area=[-1, 12, -1, 13]), 7, True),
    ("robot_s8", dict(robot_radius=0.3, max_iter=300), 8, True),
    ("step01_s9", dict(step_size=0.1, max_iter=200), 9, True),
    ("step015_s10", dict(step_size=0.15, max_iter=200), 10, True),
    ("step03_s11", dict(step_size=0.3, max_iter=300), 11, True),
    ("exp1_s12", dict(expand_dis=1.0, max_iter=300), 12, True),
    ("rate50_s13", dict(goal_sample_rate=50, max_iter=300), 13, True),
    ("long_s14", dict(max_iter=2500), 14, True),
]


def main():
    os.makedirs(GOLD, exist_ok=True)
    mod = ref_loader.load("rrt_09")
    kat(mod)
    signatures(mod)
    only = sys.argv[1:]
    for name, over, seed, until in CONFIGS:
        if only and name not in only:
            continue
        kw = dict(DRIVER)
        kw.update(over)
        res = run_plan(mod, kw, seed, until)
        save_plan(name, kw, res)
        print(name, len(res["x"]), "nodes, path", len(res["path"]), flush=True)


if __name__ == "__main__":
    main()

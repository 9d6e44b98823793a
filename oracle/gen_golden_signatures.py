#!/usr/bin/env python3
"""Golden record of the reference scripts' driver-facing interface (build container only): for every rrt_0N script,
which of the names a driver cell uses it defines at top level, the constructor of its planner class and which planning
entry points that class has, read from the parsed source text (never imported or executed).  Constructor defaults are
stored as their values.  Data only; written to tests/golden/ref_signatures.json, which tests/test_dropin_aliases.py
checks the drop-in modules' table against.
Usage: python oracle/gen_golden_signatures.py"""
import ast
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_loader  # noqa: E402
from gen_golden import OUT  # noqa: E402

PLANNER_CLASS = {"rrt_08": "BITStar"}     # every other script's planner class is RRT
DRIVER_NAMES = ("RRT", "BITStar", "Node", "get_path_length", "path_smoothing")
ENTRY_POINTS = ("planning", "informed_rrt_star_search", "plan")


def default_value(node):
    src = ast.unparse(node)
    if src == "np.deg2rad(1.0)":
        return math.radians(1.0)
    return ast.literal_eval(src)


def record(short):
    path = os.path.join(ref_loader.REF_DIR, ref_loader.FILES[short])
    tree = ast.parse(open(path).read(), filename=path)
    top = {n.name: n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef))}
    cls = PLANNER_CLASS.get(short, "RRT")
    methods = [f for f in top[cls].body if isinstance(f, ast.FunctionDef)]
    init = [f for f in methods if f.name == "__init__"][0]
    args = [a.arg for a in init.args.args][1:]
    nd = len(init.args.defaults)
    return {"file": ref_loader.FILES[short], "defines": [n for n in DRIVER_NAMES if n in top], "class": cls,
            "entry_points": [f.name for f in methods if f.name in ENTRY_POINTS],
            "init_positional": args[:len(args) - nd],
            "init_keywords": [[k, default_value(d)] for k, d in zip(args[len(args) - nd:], init.args.defaults)]}


if __name__ == "__main__":
    out = {short: record(short) for short in sorted(ref_loader.FILES)}
    dst = os.path.join(OUT, "ref_signatures.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(dst, len(out), "scripts")

"""CPU: the product's scalar core (rpp_core.h + the generated glibc replicas), compiled for the host,
agrees bit-for-bit with the live libm / the oracle; the C ABI library loads and exports every symbol."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import util

CSRC = os.path.join(util.ROOT, "robotics-path-planning_amd", "csrc")
# RRTX_TEST_SANITIZE=1: build the host checks with AddressSanitizer + UndefinedBehaviorSanitizer (run pytest with
# LD_PRELOAD=$(gcc -print-file-name=libasan.so) so that the shared-object check loads too); CPU only
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("RRTX_TEST_SANITIZE") else []


@pytest.fixture(scope="module")
def builddir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("native"))


def test_core_against_oracle(builddir):
    import oracle
    oracle.lib()
    exe = os.path.join(builddir, "core_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"] + SAN + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "core_host_check.cpp"), "-o", exe, "-ldl"], check=True)
    r = subprocess.run([exe, os.path.join(util.ROOT, "oracle", "liboracle.so"), "200000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_snap_rule_against_oracle(builddir):
    """rpp::snap_certain, the libm-free snap decision of the rrt_04 iteration kernel: wherever it answers "certainly
    snapped" the oracle's steer snaps after the same number of steps -- path resolutions 0.25 to 1e-4, offsets to 1e6,
    walk-made and forged lengths at the limit (on which the fixed 1e-9 res it replaces must be caught misjudging) -- and at
    C2 scale it leaves no more edges in doubt than that did (tests/native/snap_rule_check.cpp)."""
    import oracle
    oracle.lib()
    exe = os.path.join(builddir, "snap_rule_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"] + SAN + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "snap_rule_check.cpp"), "-o", exe, "-ldl"], check=True)
    r = subprocess.run([exe, os.path.join(util.ROOT, "oracle", "liboracle.so"), "1000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_glibc_replicas_against_live_libm(builddir):
    src = os.path.join(util.ROOT, "tests", "native", "glibc_replica_check.c")
    exe = os.path.join(builddir, "glibc_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-fno-builtin"] + SAN + ["-I", CSRC, src, "-o", exe, "-lm"],
                   check=True)
    r = subprocess.run([exe, "5000000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_abi_library_exports_every_declared_symbol():
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    declared = set(re.findall(r"\b(rrtx_[a-z_0-9]+)\s*\(", hdr))
    declared -= {"rrtx_handle", "rrtx_params", "rrtx_stats"}
    so = os.path.join(util.ROOT, "robotics-path-planning_amd", "librrtx.so")
    assert os.path.exists(so), "librrtx.so not built"
    lib = ctypes.CDLL(so)
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.rrtx_abi_version() == int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1))
    import rrt_amd
    assert set(rrt_amd._abi.EXPORTS) <= declared


def test_python_binding_mirrors_the_header():
    """The ctypes mirror (robotics-path-planning_amd/_abi.py) against include/rrtx.h: ABI version, algorithm ids, the
    size of rrtx_params as the C compiler lays it out, and every binding has argtypes (a missing one truncates the
    64-bit handle)."""
    import subprocess
    import tempfile
    import rrt_amd
    A = rrt_amd._abi
    hdr = open(os.path.join(util.ROOT, "include", "rrtx.h")).read()
    assert int(re.search(r"#define RRTX_ABI_VERSION (\d+)", hdr).group(1)) == A.RRTX_ABI_VERSION
    ids = dict((k, int(v)) for k, v in re.findall(r"(RRTX_ALGO_[A-Z_]+) = (\d+)", hdr))
    assert ids == {"RRTX_ALGO_RRT": A.ALGO_RRT, "RRTX_ALGO_RRT_STAR": A.ALGO_RRT_STAR, "RRTX_ALGO_INFORMED": A.ALGO_INFORMED,
                   "RRTX_ALGO_DUBINS": A.ALGO_DUBINS, "RRTX_ALGO_BITSTAR": A.ALGO_BITSTAR,
                   "RRTX_ALGO_RRT_DUBINS": A.ALGO_RRT_DUBINS, "RRTX_ALGO_RS": A.ALGO_RS}
    # per-instance status bits and return codes: every one the header defines has a mirror of the same value
    st = dict((k, int(v)) for k, v in re.findall(r"(RRTX_ST_[A-Z_]+) = (\d+)", hdr))
    assert st == {"RRTX_ST_DONE": A.ST_DONE, "RRTX_ST_PATH": A.ST_PATH, "RRTX_ST_OVERFLOW": A.ST_OVERFLOW,
                  "RRTX_ST_PATH_TRUNC": A.ST_PATH_TRUNC, "RRTX_ST_UNSUPPORTED": A.ST_UNSUPPORTED,
                  "RRTX_ST_REF_RAISES": A.ST_REF_RAISES, "RRTX_ST_REF_HANGS": A.ST_REF_HANGS}
    rcs = dict((k, int(v)) for k, v in re.findall(r"(RRTX_(?:OK|PARTIAL|E_[A-Z_]+)) = (-?\d+)", hdr))
    assert rcs["RRTX_PARTIAL"] == A.RRTX_PARTIAL == 1 and rcs["RRTX_OK"] == 0
    assert {v: k for k, v in rcs.items()} == {k: (v if v != "OK" else "RRTX_OK") for k, v in A.ERRORS.items()}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "rrtx.h"\nint main(void) { printf("%zu %zu %zu", '
                             'sizeof(rrtx_params), offsetof(rrtx_params, step_size), sizeof(rrtx_stats)); return 0; }\n')
        exe = os.path.join(d, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(util.ROOT, "include"), "-o", exe, src])
        sz, off, ssz = (int(v) for v in subprocess.check_output([exe]).split())
    assert sz == ctypes.sizeof(A.Params) and off == A.Params.step_size.offset and ssz == ctypes.sizeof(A.Stats)
    L = A.load()
    for name in A.EXPORTS:
        if name not in ("rrtx_abi_version", "rrtx_device_count"):
            assert getattr(L, name).argtypes is not None, name


def test_no_cpu_fallback_without_device():
    """Without a GPU the product path must fail loudly, not plan on the CPU."""
    import rrt_amd
    if rrt_amd._abi.load().rrtx_device_count() > 0:
        pytest.skip("a GPU is present")
    rrt = rrt_amd.RRTStar([0, 0], [6, 10], [(5, 5, 1)], [-2, 15])
    with pytest.raises(rrt_amd._abi.RrtxError):
        rrt.planning(animation=False)


def test_python_hypot_matches_oracle_hypot():
    import math
    import oracle
    L = oracle.lib()
    rng = np.random.default_rng(1)
    a = (rng.random(200000) * 2 - 1) * 120
    b = (rng.random(200000) * 2 - 1) * 120
    b[::7] *= 1e-6
    for i in range(len(a)):
        assert L.orc_hypot(a[i], b[i]) == math.hypot(a[i], b[i])


def test_bitstar_core_against_goldens_and_oracle(builddir):
    """The product's BIT* core (rpp_bitstar.h), compiled for the host, reproduces the reference goldens and agrees
    with the oracle on further seeds (vertex order, g-scores, parents, path, popped-edge sequence, RNG state)."""
    import ctypes as C
    import oracle
    so = os.path.join(builddir, "libbitstar_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-mfma"] + SAN + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "bitstar_host.cpp"), "-o", so], check=True)
    L = C.CDLL(so)

    def run(start, goal, obst, rand_area, max_iter, seed):
        c_min, c = oracle.bitstar_rotation([float(v) for v in start], [float(v) for v in goal])
        st = np.array(start, dtype=np.float64); gl = np.array(goal, dtype=np.float64)
        ob = np.ascontiguousarray(np.array(obst, dtype=np.float64).reshape(-1, 3))
        rot = np.array([c[0, 0], c[0, 1], c[1, 0], c[1, 1]])
        rng = oracle.mt_from_seed(seed)
        mt = np.array(list(rng.mt), dtype=np.uint32); pos = C.c_int(rng.pos)
        path = np.zeros((4096, 2)); vid = np.zeros(1024); vg = np.zeros(1024); vp = np.zeros(1024)
        ta = np.zeros(1 << 16); tb = np.zeros(1 << 16)
        pn = C.c_int(); nv = C.c_int(); tn = C.c_int(); ne = C.c_int(); ns = C.c_int(); er = C.c_int()
        L.host_bitstar(st.ctypes.data_as(C.c_void_p), gl.ctypes.data_as(C.c_void_p), C.c_double(rand_area[0]),
                       C.c_double(rand_area[1]), C.c_int(max_iter), ob.ctypes.data_as(C.c_void_p), C.c_int(len(ob)),
                       rot.ctypes.data_as(C.c_void_p), C.c_double(c_min), mt.ctypes.data_as(C.c_void_p), C.byref(pos),
                       path.ctypes.data_as(C.c_void_p), C.c_int(4096), C.byref(pn), vid.ctypes.data_as(C.c_void_p),
                       vg.ctypes.data_as(C.c_void_p), vp.ctypes.data_as(C.c_void_p), C.c_int(1024), C.byref(nv),
                       ta.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p), C.c_int(1 << 16), C.byref(tn),
                       C.byref(ne), C.byref(ns), C.byref(er))
        return dict(path=path[:pn.value].copy(), vertex_ids=vid[:nv.value].copy(), g_scores=vg[:nv.value].copy(),
                    parent_ids=vp[:nv.value].copy(), tr_e0=ta[:tn.value].copy(), tr_e1=tb[:tn.value].copy(),
                    n_edges=ne.value, n_samples=ns.value, error=er.value, pos=pos.value, w0=int(mt[0]))

    for f in util.golden_files("rrt08"):
        g = util.load_golden(f)
        r = run(g["start"], g["goal"], g["obstacles"], [float(v) for v in g["rand_area"]], int(g["max_iter"]), int(g["seed"]))
        assert np.array_equal(r["vertex_ids"], g["vertex_ids"]) and np.array_equal(r["g_scores"], g["g_scores"]), f
        assert np.array_equal(r["parent_ids"], g["parent_ids"]) and np.array_equal(r["path"], g["path"]), f
        assert np.array_equal(r["tr_e0"], g["tr_e0"]) and np.array_equal(r["tr_e1"], g["tr_e1"]), f
        assert r["n_edges"] == int(g["n_edges"]) and r["n_samples"] == int(g["n_samples"])
        assert r["pos"] == int(g["rng_pos_after"]) and r["w0"] == int(g["rng_word0_after"])
    g = util.load_golden(util.GOLDEN + "/rrt08_s42_it80.npz")
    for seed in range(100, 112):
        r = run(g["start"], g["goal"], g["obstacles"], [-2.0, 15.0], 60, seed)
        o = oracle.plan_bitstar(g["start"], g["goal"], g["obstacles"], [-2, 15], 60, seed=seed)
        assert r["error"] == o["error"]
        assert np.array_equal(r["vertex_ids"], o["vertex_ids"]) and np.array_equal(r["g_scores"], o["g_scores"])
        assert np.array_equal(r["path"], o["path"]) and np.array_equal(r["tr_e0"], o["tr_e0"])


def test_reeds_shepp_core_against_reference_kat(builddir):
    """rpp_rs.h (host + device source of the Reeds-Shepp steer of the rrt_06 kernel) against the reference's 600
    known-answer vectors: word, lengths, every point and yaw, None and raising cases -- bit for bit."""
    import struct
    import numpy as np
    g = np.load(os.path.join(util.GOLDEN, "rs_kat.npz"))
    blob = os.path.join(builddir, "rs_kat.bin")
    off = 0
    with open(blob, "wb") as f:
        for k in range(len(g["inp"])):
            n = int(g["n"][k])
            f.write(np.asarray(g["inp"][k], dtype=np.float64).tobytes())
            f.write(struct.pack("<ii", n, int(g["n_len"][k])))
            f.write(str(g["mode"][k]).encode()[:7].ljust(8, b"\0"))
            f.write(np.asarray(g["lengths"][k][:5], dtype=np.float64).tobytes())
            if n > 0:
                for key in ("poly_x", "poly_y", "poly_yaw"):
                    f.write(np.asarray(g[key][off:off + n], dtype=np.float64).tobytes())
                off += n
    exe = os.path.join(builddir, "rs_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"] + SAN + ["-I", CSRC,
                    os.path.join(util.ROOT, "tests", "native", "rs_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

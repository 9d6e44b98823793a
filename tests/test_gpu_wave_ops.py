"""The cross-lane integer helpers of the one-wave RRT* kernel (csrc/rrt_star_v2_shapes.inc: wave_prefix_sum, wave_total,
wave_argmin, wave_umin), driven through op 13 of rrtx_selftest_math and compared per 64-lane group with numpy.  They are
built from DPP row shifts (16-lane rows, 4-lane banks) and row broadcasts, so the inputs put the answer on the borders
those forms have: lanes 15/16, 31/32, 0 and 63."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 0xffffffff


def _cases(n):
    """(name, values uint32 [n], indices int32 [n]); every 64-lane group of a 256-element input gets its own variant"""
    lane = np.arange(n) % 64
    grp = np.arange(n) // 64
    ident = np.arange(n, dtype=np.int64)          # indices ascending with the lane
    rev = (n - 1 - np.arange(n)).astype(np.int64)   # ... and descending: the lowest index is then in the highest lane
    out = []
    for iname, idx in (("asc", ident), ("desc", rev)):
        out.append(("all_equal_" + iname, np.full(n, 7 + 0 * grp, dtype=np.int64), idx))
        out.append(("descending_" + iname, (1000 - lane - grp).astype(np.int64), idx))
        v = np.full(n, 500, dtype=np.int64)
        v[lane == 63] = 3
        out.append(("min_in_lane_63_" + iname, v, idx))
        v = np.full(n, 500, dtype=np.int64)
        v[lane == 0] = 3
        out.append(("min_in_lane_0_" + iname, v, idx))
        v = (600 + lane).astype(np.int64)
        v[(lane == 31) | (lane == 32)] = 5
        out.append(("dup_min_31_32_" + iname, v, idx))
        v = (600 + lane).astype(np.int64)
        v[(lane == 15) | (lane == 16)] = 5
        out.append(("dup_min_15_16_" + iname, v, idx))
        v = np.full(n, U32, dtype=np.int64)
        out.append(("all_ffffffff_" + iname, v, idx))
        v = np.full(n, U32, dtype=np.int64)
        v[lane == (17 + 13 * grp) % 64] = U32 - 1
        out.append(("ffffffff_but_one_" + iname, v, idx))
    for pos in (0, 15, 16, 31, 32, 47, 48, 63):
        v = np.zeros(n, dtype=np.int64)
        v[lane == (pos + grp) % 64] = 1
        out.append(("zeros_single_one_%d" % pos, v, ident))
    rng = np.random.default_rng(20261021)
    out.append(("random_small", rng.integers(0, 40, n).astype(np.int64), rng.permutation(n).astype(np.int64)))
    out.append(("random_u32", rng.integers(0, 1 << 32, n, dtype=np.int64), rng.permutation(n).astype(np.int64)))
    # the empty slot of a grid pass: value 0xffffffff with index 0x7fffffff
    v = rng.integers(0, 1 << 20, n).astype(np.int64)
    idx = rng.permutation(n).astype(np.int64)
    hole = rng.random(n) < 0.5
    v[hole] = U32
    idx[hole] = 0x7fffffff
    out.append(("random_with_empty_slots", v, idx))
    return out


def _expect(v, idx):
    n = v.size
    e = np.zeros((5, n))
    for g in range(0, n, 64):
        a, b = v[g:g + 64], idx[g:g + 64]
        pre = np.cumsum(a) & U32
        pre = np.where(pre >= 1 << 31, pre - (1 << 32), pre)   # the kernel sums in int32
        e[0, g:g + 64] = pre
        e[1, g:g + 64] = pre[63]
        m = a.min()
        e[2, g:g + 64] = m
        e[3, g:g + 64] = b[a == m].min()
        e[4, g:g + 64] = m
    return e


@pytest.mark.parametrize("n", [256, 64])
def test_wave_ops_match_numpy(n):
    import rrt_amd
    for name, v, idx in _cases(n):
        got = rrt_amd._abi.selftest_math(13, v.astype(np.float64), idx.astype(np.float64))
        want = _expect(v, idx)
        for k, what in enumerate(("prefix", "total", "argmin value", "argmin index", "minimum")):
            bad = np.nonzero(got[k] != want[k])[0]
            assert bad.size == 0, "%s, n = %d: %s differs at element %d: got %r, want %r" % (
                name, n, what, bad[0], got[k][bad[0]], want[k][bad[0]])


def test_wave_ops_reject_partial_wave():
    import rrt_amd
    with pytest.raises(rrt_amd._abi.RrtxError):
        rrt_amd._abi.selftest_math(13, np.zeros(65), np.zeros(65))

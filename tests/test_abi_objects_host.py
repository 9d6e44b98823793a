"""The ctypes wrappers of the seven device objects besides the planner handle (Steer, Tracker, Spline, BSpline, ArmNav, ArmIK,
ArmDH in _abi.py): what they share lives in one base class, and what load() declares for every exported entry point.  Runs
with or without a device."""
import ctypes as C

import pytest

import rrt_amd

A = rrt_amd._abi
CLASSES = [(A.Steer, "steer"), (A.Tracker, "tracker"), (A.Spline, "spline"), (A.BSpline, "bspline"), (A.ArmNav, "armnav"),
           (A.ArmIK, "armik"), (A.ArmDH, "armdh")]
IDS = [p for _, p in CLASSES]
SHARED = ("close", "__del__", "__enter__", "__exit__", "_chk")


def have_device():
    return A.load().rrtx_device_count() > 0


def test_the_seven_classes_are_the_declared_objects():
    assert tuple(IDS) == tuple(A.DEVICE_OBJECTS)
    assert [cls._prefix for cls, _ in CLASSES] == IDS


@pytest.mark.parametrize("cls,prefix", CLASSES, ids=IDS)
def test_a_negative_ordinal_is_refused(cls, prefix):
    with pytest.raises(A.RrtxError) as e:
        cls(device=-1)
    assert str(e.value).startswith("rrtx_%s_create: RRTX_E_INVALID" % prefix), str(e.value)
    assert "negative device ordinal" in str(e.value)


@pytest.mark.parametrize("cls,prefix", CLASSES, ids=IDS)
def test_lifecycle_with_or_without_a_device(cls, prefix):
    if not have_device():
        with pytest.raises(A.RrtxError) as e:
            cls()
        assert str(e.value).startswith("rrtx_%s_create: RRTX_E_NO_DEVICE" % prefix), str(e.value)
        assert "no CPU fallback" in str(e.value)
        return
    with cls() as o:
        assert isinstance(o, cls) and o._s.value
    assert not o._s
    o.close()   # a second close is harmless
    assert not o._s


@pytest.mark.parametrize("cls,prefix", CLASSES, ids=IDS)
def test_no_subclass_carries_the_shared_part(cls, prefix):
    assert issubclass(cls, A._DevObject)
    for name in SHARED:
        assert name not in vars(cls), (cls.__name__, name)
        assert name in vars(A._DevObject)
    assert not any(hasattr(cls, old) for old in ("_t", "_a"))


def test_every_export_resolves_with_its_return_type():
    L = A.load()
    assert len(set(A.EXPORTS)) == len(A.EXPORTS)
    for prefix in IDS:
        for f in ("create", "destroy", "last_error"):
            assert "rrtx_%s_%s" % (prefix, f) in A.EXPORTS
    for name in A.EXPORTS:
        fn = getattr(L, name)   # AttributeError when the library does not export it
        if name.endswith("_destroy"):
            want = None
        elif name.endswith("_last_error"):
            want = C.c_char_p
        else:
            want = C.c_int
        assert fn.restype is want, (name, fn.restype)

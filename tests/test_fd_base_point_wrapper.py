"""MIR_LSQ_FD_BASE_POINT on the Python side: the constants are the header's, and DeviceProblem.options() sets the flag exactly
when it hands over a fbRowMajorDiff callback of a problem class that declares p = 2n + 1 support. No GPU needed."""
import ctypes as C
import os
import re
import types

from mir_optim_amd import api, workloads as W

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mir_optim_amd.h")


def header_value(name):
    text = open(HEADER).read()
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)u(?:\s*<<\s*(\d+))?", text)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


def test_constants_are_the_headers():
    assert api.FD_BASE_POINT == header_value("MIR_LSQ_FD_BASE_POINT") == 4
    assert api.VARIANT_NO_FD_BASE_POINT == header_value("MIR_LSQ_VARIANT_NO_FD_BASE_POINT") == 1 << 14
    assert api.DEVICE_CALLBACKS == header_value("MIR_LSQ_DEVICE_CALLBACKS") and api.TIME_KERNELS == header_value("MIR_LSQ_TIME_KERNELS")
    taken = [getattr(api, k) for k in dir(api) if k.startswith("VARIANT_") and k != "VARIANT_NO_FD_BASE_POINT"]
    assert all(v & api.VARIANT_NO_FD_BASE_POINT == 0 for v in taken)
    assert C.sizeof(api.GpuOptions) == 96           # a bit, not a member


def fake(cls, fbd=3):
    p = cls.__new__(cls)
    p.stream = types.SimpleNamespace(handle=None)
    p.ctx = W._TanhCtx()
    p.fb, p.fbr, p.fbd = 1, 2, fbd
    return p


def test_options_set_the_flag_with_the_difference_callback_only():
    for cls in (W.TanhLinear, W.TanhLinearView):
        assert cls.fbd_base_point
        o = fake(cls).options(batched=True)
        assert o.fbRowMajorDiff == 3 and o.flags & api.FD_BASE_POINT and o.flags & api.DEVICE_CALLBACKS
        for batched in (False, "rowmajor", "pointmajor"):
            o = fake(cls).options(batched=batched)
            assert not o.fbRowMajorDiff and not o.flags & api.FD_BASE_POINT
        assert not fake(cls, fbd=None).options(batched=True).flags & api.FD_BASE_POINT      # the float problem has no fbd
    assert not W.DeviceProblem.fbd_base_point and not W.Curve.fbd_base_point
    assert not fake(W.Curve).options(batched=True).flags & api.FD_BASE_POINT                # a class that does not declare it

"""The argument precedence of the three plain level-0 entries: dvo_amd_pyramid_create, _create_from_device, _create_raw.

Every bad argument, one at a time, is DVO_AMD_ERR_INVALID_ARGUMENT with *out left NULL -- with or without a GPU, so an argument
error is reported before the missing device is -- and valid arguments on a machine without a device are DVO_AMD_ERR_NO_DEVICE.
(The remapped and the registered entry have their own: tests/test_rectify.py, tests/test_register.py.)"""
import ctypes as C

import numpy as np
import pytest

F = np.float32
INVALID, NO_DEVICE = 1, 2
W, H = 8, 4
NAN = float("nan")


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


@pytest.fixture(scope="module")
def frame():
    """host arrays large enough for every case below (no case that passes the checks reads them on a machine without a GPU)"""
    return dict(I=np.zeros((16, 32), F), Z=np.ones((16, 32), F), image=np.zeros((16, 32 * 3), np.uint8), depth=np.ones((16, 32), np.uint16))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _planes(capi, frame, name, h, **kw):
    a = dict(device=0, intensity=frame["I"], depth=frame["Z"], width=W, height=H, stride=W, levels=1, out=C.byref(h))
    a.update(kw)
    if name == "dvo_amd_pyramid_create":
        ptr = lambda v: None if v is None else _fp(v)
    else:  # (a host address stands in for the device pointer: the entry must refuse the call before it reads one)
        ptr = lambda v: None if v is None else v.ctypes.data
    return getattr(capi.lib(), name)(a["device"], ptr(a["intensity"]), ptr(a["depth"]), a["width"], a["height"], a["stride"], 8.0, 8.0,
                                     4.0, 2.0, a["levels"], 0.0, a["out"])


def _raw(capi, frame, h, **kw):
    a = dict(device=0, image=frame["image"], channels=3, istride=None, depth=frame["depth"], zstride=None, scale=1.0 / 5000.0,
             on_device=0, width=W, height=H, levels=1, out=C.byref(h))
    a.update(kw)
    istride = a["width"] * a["channels"] if a["istride"] is None else a["istride"]
    zstride = a["width"] if a["zstride"] is None else a["zstride"]
    ptr = lambda v: None if v is None else v.ctypes.data
    return capi.lib().dvo_amd_pyramid_create_raw(a["device"], ptr(a["image"]), a["channels"], istride, ptr(a["depth"]), zstride, a["scale"],
                                                 a["on_device"], a["width"], a["height"], 8.0, 8.0, 4.0, 2.0, a["levels"], 0.0, a["out"])


SIZE_CASES = [dict(width=3, stride=8), dict(height=1), dict(levels=0), dict(levels=9), dict(width=12, height=8, stride=12, levels=3)]


@pytest.mark.parametrize("name", ["dvo_amd_pyramid_create", "dvo_amd_pyramid_create_from_device"])
def test_float_plane_entries_refuse_each_bad_argument(capi, frame, name):
    assert capi.MAX_LEVELS + 1 == 9
    h = C.c_void_p()
    bad = [dict(out=None), dict(intensity=None), dict(depth=None), dict(stride=W - 1)] + SIZE_CASES
    for kw in bad:
        assert _planes(capi, frame, name, h, **kw) == INVALID, kw
        assert not h.value, kw


@pytest.mark.parametrize("on_device", [0, 1])
def test_raw_entry_refuses_each_bad_argument(capi, frame, on_device):
    h = C.c_void_p()
    bad = [dict(out=None), dict(image=None), dict(depth=None), dict(channels=2), dict(scale=0.0), dict(scale=-1.0), dict(scale=NAN),
           dict(istride=W * 3 - 1), dict(channels=1, istride=W - 1), dict(zstride=W - 1)]
    bad += [{k: v for k, v in kw.items() if k != "stride"} for kw in SIZE_CASES]
    for kw in bad:
        assert _raw(capi, frame, h, on_device=on_device, **kw) == INVALID, kw
        assert not h.value, kw


def test_valid_arguments_without_a_device_are_no_device(capi, frame):
    if capi.lib().dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    for name in ("dvo_amd_pyramid_create", "dvo_amd_pyramid_create_from_device"):
        assert _planes(capi, frame, name, h) == NO_DEVICE and not h.value
        assert _planes(capi, frame, name, h, width=16, height=8, stride=19, levels=3) == NO_DEVICE and not h.value
    for channels in (1, 3):
        assert _raw(capi, frame, h, channels=channels) == NO_DEVICE and not h.value
        assert _raw(capi, frame, h, channels=channels, on_device=1, istride=W * channels + 5, zstride=W + 3) == NO_DEVICE and not h.value

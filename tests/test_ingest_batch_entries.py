"""The argument checks of dvo_amd_pyramid_create_raw_batch (include/dvo_amd.h) and the two examples above it, on any host.

Every bad argument, one at a time, is DVO_AMD_ERR_INVALID_ARGUMENT with its sentence in dvo_amd_last_error() and every entry of
`out` NULL -- with or without a GPU, so an argument error is reported before the missing device is --, and well-formed arguments on
a machine without a device are DVO_AMD_ERR_NO_DEVICE, again with every entry NULL.  examples/batch_ingest_example.c (C99) and
examples/batch_ingest_adaptor_example.cpp (RgbdImagePyramid::createRawBatch) compile against the headers with -Werror.
(What the entry builds is tests/test_ingest_batch.py's business, on the GPU.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_batch_cases import compile_example  # noqa: E402

INVALID, NO_DEVICE = 1, 2
W, H, N = 8, 4, 3
NAN, INF = float("nan"), float("inf")
STALE = 0xDEAD0  # what every entry of `out` holds before a call: the entry must overwrite it with NULL


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


@pytest.fixture(scope="module")
def frames():
    """host frames large enough for every case below (no case that passes the checks reads them on a machine without a GPU)"""
    return [(np.zeros((16, 32 * 3), np.uint8), np.ones((16, 32), np.uint16)) for _ in range(N)]


def _call(capi, frames, **kw):
    """(status, out array) of one call whose arguments are well formed except for what `kw` replaces"""
    a = dict(device=0, count=N, images="all", depths="all", timestamps=None, channels=3, istride=None, zstride=None, scale=1.0 / 5000.0,
             on_device=0, width=W, height=H, levels=1, build_selection=0, ti=0.0, td=0.0, batch=True, out=True, null_image=None,
             null_depth=None)
    a.update(kw)
    n = max(a["count"], 1)
    b = capi.CRawBatch()
    b.count = a["count"]
    img = [frames[f % N][0].ctypes.data for f in range(n)]
    z = [frames[f % N][1].ctypes.data for f in range(n)]
    if a["null_image"] is not None:
        img[a["null_image"]] = None
    if a["null_depth"] is not None:
        z[a["null_depth"]] = None
    b.images = None if a["images"] is None else (C.c_void_p * n)(*img)
    b.depths = None if a["depths"] is None else (C.c_void_p * n)(*z)
    b.timestamps = None if a["timestamps"] is None else (C.c_double * n)(*a["timestamps"])
    b.channels = a["channels"]
    b.image_stride_bytes = a["width"] * a["channels"] if a["istride"] is None else a["istride"]
    b.depth_stride = a["width"] if a["zstride"] is None else a["zstride"]
    b.depth_scale, b.on_device, b.width, b.height = a["scale"], a["on_device"], a["width"], a["height"]
    b.fx, b.fy, b.ox, b.oy, b.levels = 8.0, 8.0, 4.0, 2.0, a["levels"]
    b.build_selection, b.intensity_threshold, b.depth_threshold = a["build_selection"], a["ti"], a["td"]
    out = (C.c_void_p * n)(*([STALE] * n))
    rc = capi.lib().dvo_amd_pyramid_create_raw_batch(a["device"], C.byref(b) if a["batch"] else None, out if a["out"] else None)
    return rc, out


def _last_error(capi):
    return capi.lib().dvo_amd_last_error().decode()


# (what is wrong, the sentence's distinguishing words)
BAD = [
    (dict(count=0), "count must be >= 1"), (dict(count=-3), "count must be >= 1"),
    (dict(images=None), "NULL"), (dict(depths=None), "NULL"),
    (dict(null_image=0), "NULL pointer at frame 0"), (dict(null_image=N - 1), "NULL pointer at frame %d" % (N - 1)),
    (dict(null_depth=1), "NULL pointer at frame 1"),
    (dict(channels=2), "channels must be 1 or 3"),
    (dict(scale=0.0), "depth_scale must be > 0"), (dict(scale=-1.0), "depth_scale must be > 0"), (dict(scale=NAN), "depth_scale must be > 0"),
    (dict(istride=W * 3 - 1), "image stride"), (dict(channels=1, istride=W - 1), "image stride"), (dict(zstride=W - 1), "depth_stride < width"),
    (dict(build_selection=2), "build_selection must be 0 or 1"), (dict(build_selection=-1), "build_selection must be 0 or 1"),
    (dict(build_selection=1, ti=NAN), "non-finite"), (dict(build_selection=1, td=INF), "non-finite"),
    (dict(build_selection=1, ti=-INF), "non-finite"),
    (dict(width=3), "level 0"), (dict(height=1), "level 0"), (dict(levels=0), "levels must be"), (dict(levels=9), "levels must be"),
    (dict(width=12, height=8, levels=3), "level 1"),
]


@pytest.mark.parametrize("on_device", [0, 1])
def test_batch_entry_refuses_each_bad_argument_with_its_sentence(capi, frames, on_device):
    for kw, words in BAD:
        rc, out = _call(capi, frames, on_device=on_device, **kw)
        assert rc == INVALID, kw
        text = _last_error(capi)
        assert text.startswith("dvo_amd_pyramid_create_raw_batch: ") and words in text, (kw, text)
        if kw.get("count", N) >= 1:  # (with count < 1 there is no entry to clear)
            assert not any(out[f] for f in range(N)), kw
    for kw in (dict(batch=False), dict(out=False)):
        assert _call(capi, frames, on_device=on_device, **kw)[0] == INVALID, kw
        assert "NULL" in _last_error(capi)


def test_the_checks_come_in_the_raw_entries_order_and_before_the_device(capi, frames):
    """NULL pointers, then the frame's format (check_raw), then the selection's arguments, then the levels, then the device: of two
    bad arguments the earlier one's sentence is reported, and a device that cannot exist does not hide either"""
    for kw, words in [(dict(null_depth=2, channels=2), "NULL"), (dict(channels=2, build_selection=7), "channels"),
                      (dict(zstride=W - 1, levels=0), "depth_stride"), (dict(build_selection=7, levels=0), "build_selection"),
                      (dict(levels=0, device=-1), "levels must be"), (dict(levels=0, device=10 ** 6), "levels must be")]:
        rc, out = _call(capi, frames, **kw)
        assert rc == INVALID and words in _last_error(capi), (kw, _last_error(capi))
        assert not any(out[f] for f in range(N)), kw


def test_thresholds_are_only_looked_at_when_a_selection_is_asked_for(capi, frames):
    rc, out = _call(capi, frames, build_selection=0, ti=NAN, td=INF)
    have_gpu = capi.lib().dvo_amd_device_count() > 0
    assert rc == (0 if have_gpu else NO_DEVICE)
    for f in range(N):
        if out[f]:
            capi.lib().dvo_amd_pyramid_release(out[f])


def test_valid_arguments_without_a_device_are_no_device(capi, frames):
    if capi.lib().dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    cases = [dict(), dict(count=1), dict(channels=1), dict(on_device=1, istride=W * 3 + 5, zstride=W + 3),
             dict(width=16, height=8, levels=3, timestamps=[0.5, 1.5, 2.5]), dict(build_selection=1, ti=2.0, td=0.01)]
    for kw in cases:
        rc, out = _call(capi, frames, **kw)
        assert rc == NO_DEVICE, kw
        assert not any(out[f] for f in range(kw.get("count", N))), kw
    with pytest.raises(capi.DvoAmdError) as e:
        capi.RgbdImagePyramid.from_raw_batch([f[0].reshape(16, 32, 3) for f in frames], [f[1] for f in frames], (8.0, 8.0, 4.0, 2.0), 1,
                                             selection=(0.0, 0.0))
    assert e.value.status == NO_DEVICE


def test_binding_refuses_frames_of_different_shapes(capi):
    a, z = np.zeros((4, 8), np.uint8), np.ones((4, 8), np.uint16)
    for images, depths, stamps in [([a, a[:, :4]], [z, z], None), ([a, a], [z], None), ([], [], None), ([a, a], [z, z], [0.0]),
                                   ([a, a], [z, z[:2]], None)]:
        with pytest.raises(ValueError):
            capi.RgbdImagePyramid.from_raw_batch(images, depths, (8.0, 8.0, 4.0, 2.0), 1, timestamps=stamps)
    with pytest.raises(ValueError):  # device pointers say nothing about their frames: size and channels must come with them
        capi.RgbdImagePyramid.from_raw_batch([4096], [8192], (8.0, 8.0, 4.0, 2.0), 1)


@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_batch_ingest_examples_compile(kind):
    assert os.path.exists(compile_example(kind))


def test_abi_version_stays_and_the_two_names_are_exported(capi):
    for n in ("dvo_amd_pyramid_create_raw_batch", "dvo_amd_debug_batch_build_stats"):
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
    assert capi.lib().dvo_amd_abi_version() == 3  # purely additive
    if capi.lib().dvo_amd_device_count() == 0:  # no batched build yet: the probe reports nothing
        assert capi.batch_build_stats() == dict(kernel_launches=0, copies=0, synchronisations=0)
    assert capi.lib().dvo_amd_debug_batch_build_stats(-1, None, None, None) == INVALID

"""Share placement (DVO_AMD_SHARE_PLACEMENT) decides on which XCD and when a block of k_tick runs, never what it computes.

A batch in which several pairs share keyframes and current frames -- three keyframes under four current frames, every
combination resident several times at once -- must return, pair for pair and bit for bit, what single match() calls return
(a single pair goes out behind the small argument block, which has no sets), under each value of the knob: 0 = every item
placed on its own, 1 = the pairs of a keyframe level next to each other with one XCD rotation, 2 = ... dispatched interleaved.
The knob is read when a tracker is created.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    if c.lib().dvo_amd_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return c


@pytest.fixture(scope="module")
def frames(capi, synth):
    """three keyframes and four current frames of one 640x480 trajectory"""
    K = synth.intrinsics_for(640, 480)
    poses = synth.stream_poses(7, synth.XI_STEP_STREAM * 1.5)
    return [capi.RgbdImagePyramid(*synth.render(640, 480, poses[t], frame_id=t), K, 4) for t in range(7)]


@pytest.fixture(scope="module")
def singles(capi, frames):
    one = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    out = {(i, j): one.match(frames[i], frames[j]) for i in range(3) for j in range(3, 7)}
    assert not any(r.isNaN() for r in out.values())
    return out


def assert_same_bytes(a, b, what):
    assert a.isNaN() == b.isNaN(), what
    assert np.asarray(a.Transformation).tobytes() == np.asarray(b.Transformation).tobytes(), what
    assert np.asarray(a.Information).tobytes() == np.asarray(b.Information).tobytes(), what
    assert np.float64(a.LogLikelihood).tobytes() == np.float64(b.LogLikelihood).tobytes(), what
    assert len(a.Levels) == len(b.Levels), what
    for la, lb in zip(a.Levels, b.Levels):
        assert (la["Id"], la["ValidPixels"], la["TerminationCriterion"], len(la["Iterations"])) == \
               (lb["Id"], lb["ValidPixels"], lb["TerminationCriterion"], len(lb["Iterations"])), what
        for ia, ib in zip(la["Iterations"], lb["Iterations"]):
            assert ia["ValidConstraints"] == ib["ValidConstraints"], what
            assert np.float64(ia["TDistributionLogLikelihood"]).tobytes() == np.float64(ib["TDistributionLogLikelihood"]).tobytes(), what
            for key in ("TDistributionPrecision", "EstimateIncrement", "EstimateInformation", "estimate", "initial"):
                assert np.asarray(ia[key]).tobytes() == np.asarray(ib[key]).tobytes(), (what, key)


@pytest.mark.parametrize("residency", [24, 62])
@pytest.mark.parametrize("share", [0, 1, 2])
def test_batch_with_shared_keyframes_and_frames_equals_single_matches(capi, frames, singles, monkeypatch, share, residency):
    """pair k: keyframe k % 3, current frame 3 + (k // 3) % 4.  62 resident pairs fill one launch (every keyframe level's set has
    up to ~20 members), 24 turn every slot over several times and go out on the same large argument block"""
    monkeypatch.setenv("DVO_AMD_SHARE_PLACEMENT", str(share))
    pairs = [(k % 3, 3 + (k // 3) % 4) for k in range(96)]
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    out = trk.match_batch([frames[i] for i, _ in pairs], [frames[j] for _, j in pairs], in_flight=residency)
    assert len(out) == len(pairs)
    for k, (ij, r) in enumerate(zip(pairs, out)):
        assert_same_bytes(singles[ij], r, f"pair {k} = {ij}, share placement {share}, {residency} resident")

"""The cache policy of k_tick's streams changes where bytes are kept, never which bytes a pair gets.

The residual spill, its re-read by the likelihood pass and the per-block records go through non-temporal stores and loads
(csrc/dvo_kernels.hip: st_once / ld_once); the pyramids keep the default policy.  A streaming store is still an ordinary
write-back store to the launch that reads it, so a batch in which pairs of two references share current frames -- the sharing
the policy is there to protect -- must give, pair for pair, the bytes of the same pairs run one at a time with match().  The
batch runs twice on the same tracker: the second one reuses, slot by slot, residual buffers and record areas that the first
one wrote with streaming stores.
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
    """two references and four current frames of one 640x480 trajectory"""
    K = synth.intrinsics_for(640, 480)
    poses = synth.stream_poses(6, synth.XI_STEP_STREAM * 1.5)
    return [capi.RgbdImagePyramid(*synth.render(640, 480, poses[t], frame_id=t), K, 4) for t in range(6)]


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


@pytest.mark.parametrize("residency", [12, 62])
def test_shared_frames_batch_equals_single_matches_twice(capi, frames, residency):
    """pair k: reference k % 2 (frames 0 and 1 alternate), current frame 2 + (k // 2) % 4: every current frame is resident under
    both references at once, every reference under all four current frames; 12 resident pairs turn every slot over several
    times within a batch, 62 fill one launch"""
    cfg = capi.Config(FirstLevel=3, LastLevel=0)
    pairs = [(k % 2, 2 + (k // 2) % 4) for k in range(72)]
    one = capi.DenseTracker(cfg)
    singles = {ij: one.match(frames[ij[0]], frames[ij[1]]) for ij in sorted(set(pairs))}
    assert len(singles) == 8 and not any(r.isNaN() for r in singles.values())
    trk = capi.DenseTracker(cfg)
    for run in (1, 2):
        out = trk.match_batch([frames[i] for i, _ in pairs], [frames[j] for _, j in pairs], in_flight=residency)
        assert len(out) == len(pairs)
        for k, (ij, r) in enumerate(zip(pairs, out)):
            assert_same_bytes(singles[ij], r, f"pair {k} = {ij}, batch {run}, {residency} resident")

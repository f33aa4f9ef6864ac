"""GPU: the fixed-seed slices of tools/fuzz_map.py — every map-side family's generator with its own parameters drawn at random, on the device, bit for
bit against the family's reference — and the exhaustive spaces of the two association replays through the HIP kernels.

  * one test per family: the seed and case count committed in fuzz_map.FAMILIES (tests/test_fuzz_map_cases.py proves on the CPU that they reach every
    tag); every case is good, and the union of the reached tags is the family's tag list
  * hs_frame_associate_device and hs_frame_associate_views_device over EVERY state and op set of the n x L spaces that tests/test_track_ref.py and
    tests/test_refkf_ref.py enumerate in numpy (all but 4 x 4, which the tool runs): cases with disjoint view and landmark ranges are independent
    under both replays, so up to 2^20 of them are one state and one call; ops in a seeded shuffled array order; kp_lm and kp_outl case by case
    against seq_batch, n_matches against the start value plus the twins' fresh counts
  * the six key-frame stages cannot be concatenated (the depth walk is per frame): a fixed stride over the three exhaustive spaces of
    tests/test_keyframe_ref.py; the tool runs all of them
Measured durations on the MI355X: profiles/README.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_map as FM                           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    return FM.Context()


def test_constants_are_the_library_s(ctx):
    from hyslam_amd import _native as N
    assert (FM.HS_KF_LDS_SLOTS, FM.HS_KF_SORT_PASS) == (N.HS_KF_LDS_SLOTS, N.HS_KF_SORT_PASS)


@pytest.mark.parametrize("name", list(FM.FAMILIES))
def test_family_slice(ctx, name):
    fam = FM.FAMILIES[name]
    ctx.seed = fam.seed
    rng, reached = np.random.default_rng(fam.seed), set()
    for i in range(fam.cases):
        msg, good, tags = fam.one_case(rng, i, ctx)
        assert good, msg
        reached |= tags
    assert reached == set(fam.tags), (sorted(set(fam.tags) - reached), sorted(reached - set(fam.tags)))


@pytest.mark.parametrize("n,L", FM.EXHAUSTIVE_SIZES)
@pytest.mark.parametrize("which", ["lm", "vw"])
def test_replay_exhaustive_on_the_device(ctx, which, n, L):
    """lm: hs_frame_associate_device over (L + 1)^n x 3^n x (n + 1)^L cases (2.6 million at 4 x 3); vw: hs_frame_associate_views_device over the
    valid op sets (a view in at most one op, a landmark in at most one)"""
    count, msg = FM.exhaustive_check(which, n, L, FM.device_runner(ctx, which), seed=1000 * n + L)
    assert msg is None, msg
    mod = FM.LR if which == "lm" else FM.VR
    kp, fl, op = mod.state_tables(n, L)
    assert count == len(kp) * len(fl) * len(op)


KEYFRAME_STRIDE = 47


def test_keyframe_stages_over_a_stride_of_the_exhaustive_spaces(ctx):
    """every 47th of the 22 576 cases of tests/test_keyframe_ref.py's three spaces (481 cases; 47 shares no factor with the spaces' periods 4, 8, 12 and
    64, so every residue of their cycling tables comes up), each through the six stage entry points against ref_keyframe.dense stage by stage.
    Measured on the MI355X: a case takes 8.2 ms (all 22 576 from the tool: 185 s), almost all of it the ~30 guarded buffers a case allocates and the
    six read-backs; at the committed stride 47 the test takes 4.6 s (8.4 s at stride 23)."""
    count, msg = FM.keyframe_exhaustive(ctx, KEYFRAME_STRIDE)
    assert msg is None, msg
    assert count == -(-22576 // KEYFRAME_STRIDE)

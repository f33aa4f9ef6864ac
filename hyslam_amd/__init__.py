"""hyslam_amd — MI355X-native ORB extraction + Hamming matching for hySLAM's per-frame hot path.

The compute lives in libhyslam_amd.so (hand-written HIP for gfx950) behind the C ABI of include/hyslam_amd.h;
this package is the thin host-side mirror of the reference's FeatureExtractor / Stereomatcher interfaces.
"""
from .features import (Camera, FeatureExtractorSettings, FeatureMatcher, FeatureMatcherSettings, FrameTracker, HsError, KP_DTYPE, MonoEstimator,  # noqa: F401
                       ORBExtractor, ORBFactory, ORBVocabulary, Optimizer, PlaceRecognizer, PnPsolver, Sim3Solver, Stereomatcher, stereo_params)
from ._native import FrameView, LM_DTYPE, MONOINIT_PARAMS_DTYPE, MONOINIT_RESULT_DTYPE, PNP_CORR_DTYPE, PNP_PARAMS_DTYPE, PNP_RESULT_DTYPE, PNP_STATE_DTYPE, POSE_EDGE_DTYPE, POSE_PROBLEM_DTYPE, POSE_RESULT_DTYPE, POSE_VIEW_DTYPE, ProjParams, SIM3_CORR_DTYPE, SIM3_PARAMS_DTYPE, SIM3_RESULT_DTYPE, SIM3_STATE_DTYPE, TRACK_RESULT_DTYPE, TrackParams, VocabTree  # noqa: F401

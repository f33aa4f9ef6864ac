#!/usr/bin/env python3
"""Cost of the quadtree launch per pyramid level on the benchmark's scene: one stereo-front-end call of `pairs` pairs (default 64 = 128 frames,
no FAST keys at that batch), then the quadtree launch replayed for every single level alone (hs_orb_debug_quadtree_replay, HIP events), for the
ranges [0, k) / [k, L) and for all levels.  Prints the candidates per level of the first frames beside the times.

Under `rocprofv3 --pmc SQ_INSTS_VALU SQ_BUSY_CU_CYCLES -- python tools/quadtree_level_times.py 64 1` (a counter pass of its own, no trace
domains) the k_quadtree dispatches appear in this order: the front-end call's own launch, then ONE launch per line printed below; the grid's x
extent is the number of levels of the dispatch."""
import json
import sys
sys.path.insert(0, ".")
import numpy as np
import torch
import hyslam_amd as HS
from hyslam_amd import _native as N
from hyslam_amd.synth import synth_stereo_pair

W, H, NFEAT = 1920, 1080, 2000
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
nd = min(4, B)
pairs = [synth_stereo_pair(1000 + i, W, H, max(40, (W * H) // 800)) for i in range(nd)]
left = torch.from_numpy(np.stack([pairs[i % nd][0] for i in range(B)])).to(dev)
right = torch.from_numpy(np.stack([pairs[i % nd][1] for i in range(B)])).to(dev)
ex = HS.ORBExtractor(HS.FeatureExtractorSettings(nFeatures=NFEAT), device=0)
cap = ex.max_keypoints()
sp = HS.stereo_params(HS.Camera(fx=1050.0, mbf=1050.0 * 0.12, mnMaxY=float(H)))
kpb = N.KP_DTYPE.itemsize
kL = torch.empty(B * cap * kpb, dtype=torch.uint8, device=dev); kR = torch.empty_like(kL)
dL = torch.empty(B * cap * 32, dtype=torch.uint8, device=dev); dR = torch.empty_like(dL)
nL = torch.zeros(B, dtype=torch.int32, device=dev); nR = torch.zeros(B, dtype=torch.int32, device=dev)
uR = torch.empty(B * cap, dtype=torch.float32, device=dev); depth = torch.empty_like(uR)
ex.reserve(W, H, 2 * B)
ex.stereo_frontend_batch_device(left.data_ptr(), right.data_ptr(), B, W, H, W, W * H, kL.data_ptr(), dL.data_ptr(), nL.data_ptr(),
                                kR.data_ptr(), dR.data_ptr(), nR.data_ptr(), cap, sp, uR.data_ptr(), depth.data_ptr(), 0)
ex.synchronize()
L = 8
cands = [[int(len(ex.debug_candidates(img, lv))) for img in range(min(2 * B, 8))] for lv in range(L)]
rows = []
for lv in range(L):
    rows.append({"levels": [lv, lv + 1], "ms": round(ex.debug_quadtree_replay(lv, 1, REPS), 5), "candidates_first_frames": cands[lv]})
for k in range(1, L):
    rows.append({"levels": [0, k], "ms": round(ex.debug_quadtree_replay(0, k, REPS), 5)})
    rows.append({"levels": [k, L], "ms": round(ex.debug_quadtree_replay(k, L - k, REPS), 5)})
rows.append({"levels": [0, L], "ms": round(ex.debug_quadtree_replay(0, L, REPS), 5)})
# the four- / eight-wave level instance for the levels [k, L) the plan allows (1080p: k >= 2), and how many of its workgroups leave the count domain
lib = N.lib()
for threads in (256, 512):
    for k in range(2, L):
        lib.hs_debug_quadtree_level_fallbacks(1)
        ms1 = ex.debug_quadtree_replay(k, L - k, 1, threads)
        fb = int(lib.hs_debug_quadtree_level_fallbacks(1))
        rows.append({"levels": [k, L], "threads": threads, "ms": round(ex.debug_quadtree_replay(k, L - k, REPS, threads), 5), "ms_first": round(ms1, 5),
                     "fallback_workgroups": fb, "of": (L - k) * 2 * B})
    for lv in range(2, L):
        rows.append({"levels": [lv, lv + 1], "threads": threads, "ms": round(ex.debug_quadtree_replay(lv, 1, REPS, threads), 5)})
for r in rows:
    print(json.dumps(r))

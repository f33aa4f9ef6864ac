"""Host-side mirror of the reference's feature interfaces for the ORB hot path, on top of the C ABI.

Names, argument meaning and error behaviour follow bmhopkinson/hyslam:
  FeatureExtractorSettings  src/core/FeatureExtractorSettings.h:19-32
  FeatureMatcherSettings    src/features/FeatureMatcher.h:98-103
  ORBExtractor              src/features/ORBExtractor.h:62-130 (FeatureExtractor ABC: FeatureExtractor.h:25-37)
  Stereomatcher             src/features/Stereomatcher.h:25-51
  ORBFactory                src/features/ORBFactory.h / FeatureFactory.h:21-33
All compute happens in libhyslam_amd.so (HIP, gfx950).  Nothing here falls back to a CPU path.
"""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import KP_DTYPE, HsError  # noqa: F401


class FeatureExtractorSettings:
    def __init__(self, nFeatures=1000, fScaleFactor=1.2, nLevels=8, init_threshold=20, min_threshold=4, N_CELLS=30,
                 size_ref=31.0, sigma_ref=1.0):
        # defaults of ORBFactory::ORBFactory(), src/features/ORBFactory.cpp:13-25
        self.nFeatures, self.fScaleFactor, self.nLevels = nFeatures, fScaleFactor, nLevels
        self.init_threshold, self.min_threshold, self.N_CELLS = init_threshold, min_threshold, N_CELLS
        self.size_ref, self.sigma_ref = size_ref, sigma_ref


class FeatureMatcherSettings:
    def __init__(self, nnratio=0.6, TH_HIGH=100.0, TH_LOW=50.0, checkOri=True):
        self.nnratio, self.TH_HIGH, self.TH_LOW, self.checkOri = nnratio, TH_HIGH, TH_LOW, checkOri


class Camera:
    """The fields of HYSLAM::Camera the stereo matcher reads (src/features/Stereomatcher.cpp:7-24,44)."""

    def __init__(self, fx=1050.0, mbf=1050.0 * 0.12, mnMaxY=1080.0):
        self._fx, self.mbf, self.mnMaxY = fx, mbf, mnMaxY

    def fx(self):
        return self._fx


def _params(settings, blur_taps=None, fast_threshold=20):
    p = N.OrbParams()
    N.lib().hs_orb_default_params(C.byref(p))
    p.nfeatures, p.scale_factor, p.nlevels = settings.nFeatures, settings.fScaleFactor, settings.nLevels
    p.cell_px, p.ini_th_fast, p.min_th_fast = settings.N_CELLS, settings.init_threshold, settings.min_threshold
    p.fast_threshold = fast_threshold
    if blur_taps is not None:
        for i in range(7):
            p.blur_taps[i] = int(blur_taps[i])
    return p


class ORBExtractor:
    """HYSLAM::ORBExtractor.  `extractor(image)` returns (keypoints[KP_DTYPE], descriptors[n,32] uint8)."""

    def __init__(self, settings=None, device=0, blur_taps=None, fast_threshold=20):
        """fast_threshold: hs_orb_params::fast_threshold (the reference always runs 20: ORBFinder.cpp:58-60; other values are for tests and other callers)"""
        self.settings = settings or FeatureExtractorSettings()
        self._lib = N.lib()
        self._h = C.c_void_p()
        self._p = _params(self.settings, blur_taps, fast_threshold)
        st = self._lib.hs_orb_create(C.byref(self._p), device, C.byref(self._h))
        if st != N.HS_OK:
            self._h = C.c_void_p()
            raise HsError(st, self._lib.hs_status_string(st).decode())
        self.device = device
        self.last_frame_tokens = []                        # of the last extract_batch(..., publish=True)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.hs_orb_destroy(self._h)
            self._h = C.c_void_p()
            for ptr in getattr(self, "_pinned", []):
                self._lib.hs_host_free(ptr)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- FeatureExtractor interface (FeatureExtractor.h:25-37)
    def GetLevels(self):
        return self._lib.hs_orb_get_levels(self._h)

    def GetScaleFactor(self):
        return self._lib.hs_orb_get_scale_factor(self._h)

    def _tables(self):
        n = self.GetLevels()
        arrs = [np.zeros(n, np.float32) for _ in range(4)] + [np.zeros(n, np.int32)]
        N.check(self._h, self._lib.hs_orb_get_scale_tables(self._h, *(a.ctypes.data_as(C.c_void_p) for a in arrs)))
        return arrs

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def GetFeaturesPerLevel(self):
        return self._tables()[4]

    def max_keypoints(self):
        return self._lib.hs_orb_max_keypoints(self._h)

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors), ORBExtractor.cpp:496-562 (mask ignored, as in the reference)."""
        if image is None or image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)     # silent return, ORBExtractor.cpp:499-500
        k, d = self.extract_batch([image])
        return k[0], d[0]

    def extract_batch(self, images, publish=False):
        """publish=True: every extracted frame also stays on the device (include/hyslam_amd.h "device-resident frames"); the tokens of the call are in
        `last_frame_tokens` — what the C++ extractor adaptor does for hySLAM's FeatureViews (host/HipORBExtractor.h)."""
        # row-strided views (a cv::Mat ROI: unit pixel stride, row stride >= width) go to the C ABI as they are
        strided = lambda im: isinstance(im, np.ndarray) and im.ndim == 2 and im.dtype == np.uint8 and im.strides[1] == 1 and im.strides[0] >= im.shape[1]
        imgs = [im if strided(im) else np.ascontiguousarray(im) for im in images]
        if len({im.strides[0] for im in imgs if im.ndim == 2}) > 1:           # one row stride per call
            imgs = [np.ascontiguousarray(im) for im in imgs]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 2:
                raise TypeError("image must be CV_8UC1 (2-D uint8)")          # assert(image.type() == CV_8UC1), :503
            if im.shape != imgs[0].shape:
                raise ValueError("batched frames must have equal size")
        b = len(imgs)
        h, w = imgs[0].shape
        self.reserve(w, h, b)                                   # max_keypoints() depends on the frame's aspect ratio (root nodes per level)
        cap = self.max_keypoints()
        kps = np.zeros((b, cap), KP_DTYPE)
        desc = np.zeros((b, cap, 32), np.uint8)
        n = np.zeros(b, np.int32)
        ptrs = (C.c_void_p * b)(*[im.ctypes.data for im in imgs])
        N.check(self._h, self._lib.hs_orb_extract_batch(self._h, ptrs, b, w, h, imgs[0].strides[0],
                                                        kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), cap,
                                                        n.ctypes.data_as(C.c_void_p)))
        self.last_frame_tokens = []
        if publish:
            for i in range(b):
                tok = C.c_uint64(0)
                if n[i] > 0:
                    N.check(self._h, self._lib.hs_frame_publish(self._h, i, kps[i].ctypes.data_as(C.c_void_p), int(n[i]), C.byref(tok)))
                self.last_frame_tokens.append(tok.value)
        return [kps[i, :n[i]].copy() for i in range(b)], [desc[i, :n[i]].copy() for i in range(b)]

    def extract_camera_batch(self, frames, rgb, scale, want_grey=False):
        """ImageProcessing::PreProcessImg + the extractor call in one (src/main/ImageProcessing.cpp:44,55 / :76-77,82-83; hs_orb_extract_camera_batch): `frames`
        as the camera delivers them — (h, w) or (h, w, 3 | 4) uint8, equal sizes — cross PCIe as they are, are scaled by the camera's `scale` and turned to grey on
        the device (`rgb`: the camera's RGB key) and extracted.  Returns (keypoints per frame, descriptors per frame[, grey frames])."""
        imgs = [np.ascontiguousarray(f, np.uint8) for f in frames]
        for im in imgs:
            if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] not in (3, 4)) or im.shape != imgs[0].shape:
                raise TypeError("camera frames must be equal-sized (h, w) or (h, w, 3 | 4) uint8 arrays")
        b = len(imgs)
        h, w = imgs[0].shape[:2]
        cn = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
        pp = N.PreprocessParams(cn, int(bool(rgb)), float(scale), 0)
        ow, oh = C.c_int32(), C.c_int32()
        self._lib.hs_preprocess_size(w, h, C.c_float(scale), C.byref(ow), C.byref(oh))
        if ow.value < 1 or oh.value < 1:
            raise N.HsError(N.HS_ERR_INVALID, "the camera scale reduces the frame to nothing")
        self.reserve(ow.value, oh.value, b)
        cap = self.max_keypoints()
        kps = np.zeros((b, cap), KP_DTYPE)
        desc = np.zeros((b, cap, 32), np.uint8)
        n = np.zeros(b, np.int32)
        grey = np.zeros((b, oh.value, ow.value), np.uint8) if want_grey else None
        ptrs = (C.c_void_p * b)(*[im.ctypes.data for im in imgs])
        N.check(self._h, self._lib.hs_orb_extract_camera_batch(self._h, ptrs, b, w, h, imgs[0].strides[0], C.byref(pp),
                                                               kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), cap, n.ctypes.data_as(C.c_void_p),
                                                               grey.ctypes.data_as(C.c_void_p) if want_grey else None))
        out = ([kps[i, :n[i]].copy() for i in range(b)], [desc[i, :n[i]].copy() for i in range(b)])
        return out + ([grey[i] for i in range(b)],) if want_grey else out

    def preprocess_device(self, d_src, w, h, row_stride, image_stride, batch, channels, rgb, scale, d_grey, grey_row_stride, grey_image_stride, stream=0):
        """hs_preprocess_device: device frames -> device grey frames of the scaled size (asynchronous)"""
        pp = N.PreprocessParams(int(channels), int(bool(rgb)), float(scale), 0)
        N.check(self._h, self._lib.hs_preprocess_device(self._h, d_src, w, h, row_stride, image_stride, batch, C.byref(pp), d_grey, grey_row_stride, grey_image_stride, stream or None))

    def find_frame(self, keypoints):
        """token of the cached frame whose keypoint array equals `keypoints` bit for bit (0: none) — hs_frame_find, what the matcher adaptors do with a FeatureViews"""
        k = np.ascontiguousarray(keypoints, KP_DTYPE)
        tok = C.c_uint64(0)
        if len(k) == 0 or self._lib.hs_frame_find(self.device, k.ctypes.data_as(C.c_void_p), len(k), C.byref(tok)) != N.HS_OK:
            return 0
        return tok.value

    def release_frame(self, token):
        return self._lib.hs_frame_release(self.device, C.c_uint64(token)) == N.HS_OK

    # ---- pipelined host ingest (hs_orb_submit_batch / hs_orb_wait): at most two tickets in flight, like the reference's frame queue
    # (System.cc:194-196).  The H2D copy of a submitted batch overlaps the kernels of the batch before it.
    def submit_batch(self, images, sp=None):
        """images: same-sized 2-D uint8 arrays with one common row stride (pinned_frames() gives page-locked ones); with `sp` (a StereoParams)
        the first half are the left frames and the second half the right ones and the stereo matcher runs too.  Returns a ticket.
        The arrays must stay alive and unchanged until wait(ticket) returns."""
        b = len(images)
        h, w = images[0].shape
        for im in images:
            if im.dtype != np.uint8 or im.ndim != 2 or im.shape != (h, w) or im.strides != images[0].strides or im.strides[1] != 1:
                raise TypeError("frames must be 2-D uint8 of one size and one row stride")
        ptrs = (C.c_void_p * b)(*[im.ctypes.data for im in images])
        t = C.c_int32()
        N.check(self._h, self._lib.hs_orb_submit_batch(self._h, ptrs, b, w, h, images[0].strides[0], C.byref(sp) if sp is not None else None, C.byref(t)))
        self._tickets = getattr(self, "_tickets", {})
        # the ticket remembers ITS output capacity (the geometry may change with a later submit) and keeps the frames alive: the C side reads
        # them asynchronously until wait() / cancel() returns (include/hyslam_amd.h: lifetime of the frames)
        self._tickets[t.value] = (b, sp is not None, images, self.max_keypoints())
        return t.value

    def submit_camera_batch(self, frames, rgb, scale, sp=None):
        """the same with the camera's own frames (hs_orb_submit_camera_batch): equal-sized (h, w) or (h, w, 3 | 4) uint8 arrays, C-contiguous; PreProcessImg (camera
        scale + grey) runs on the device in front of the pyramid; with `sp` the first half are the left frames, the second half the right ones."""
        b = len(frames)
        for im in frames:
            if im.dtype != np.uint8 or im.ndim not in (2, 3) or im.shape != frames[0].shape or not im.flags["C_CONTIGUOUS"] or (im.ndim == 3 and im.shape[2] not in (3, 4)):
                raise TypeError("camera frames must be equal-sized C-contiguous (h, w) or (h, w, 3 | 4) uint8 arrays")
        h, w = frames[0].shape[:2]
        cn = 1 if frames[0].ndim == 2 else frames[0].shape[2]
        pp = N.PreprocessParams(cn, int(bool(rgb)), float(scale), 0)
        ptrs = (C.c_void_p * b)(*[im.ctypes.data for im in frames])
        t = C.c_int32()
        N.check(self._h, self._lib.hs_orb_submit_camera_batch(self._h, ptrs, b, w, h, frames[0].strides[0], C.byref(pp), C.byref(sp) if sp is not None else None, C.byref(t)))
        self._tickets = getattr(self, "_tickets", {})
        self._tickets[t.value] = (b, sp is not None, frames, self.max_keypoints())
        return t.value

    def wait(self, ticket, out=None):
        """-> (n[b], kps[b, cap], desc[b, cap, 32], uRight[b/2, cap] | None, depth[b/2, cap] | None); entries beyond n[i] are undefined.
        `out` = a tuple of arrays from a previous call to reuse."""
        b, stereo, _, cap = self._tickets[ticket]          # looked up, NOT removed: a wait that fails (capacity, arguments) can be repeated
        if out is None:
            out = (np.zeros(b, np.int32), np.zeros((b, cap), KP_DTYPE), np.zeros((b, cap, 32), np.uint8),
                   np.zeros((b // 2, cap), np.float32) if stereo else None, np.zeros((b // 2, cap), np.float32) if stereo else None)
        n, kps, desc, uR, depth = out
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        # hs_orb_wait writes all five arrays in ONE [batch][c] layout: every reused array must have exactly that shape and dtype, or the C side
        # would write out of bounds
        c = kps.shape[1] if (isinstance(kps, np.ndarray) and kps.ndim == 2) else -1
        want = [(n, (b,), np.int32), (kps, (b, c), KP_DTYPE), (desc, (b, c, 32), np.uint8)]
        if stereo:
            want += [(uR, (b // 2, c), np.float32), (depth, (b // 2, c), np.float32)]
        for a, shape, dt in want:
            if not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable:
                raise ValueError("wait(): a reused output array does not have the ticket's layout (need %s %s, C-contiguous)" % (shape, np.dtype(dt).name))
        if c < cap:
            raise ValueError("wait(): the reused output arrays hold %d keypoints per frame, the ticket needs %d" % (c, cap))
        try:
            N.check(self._h, self._lib.hs_orb_wait(self._h, ticket, p(kps), p(desc), p(n), kps.shape[1], p(uR), p(depth)))
        except HsError as e:
            if e.status == N.HS_ERR_HIP:                    # the C side has released the slot: the ticket is gone
                self._tickets.pop(ticket, None)
            raise
        del self._tickets[ticket]                           # only now: the results are out and the frames may go
        return out

    def cancel(self, ticket):
        """give up a ticket: waits until its batch has drained, drops the results"""
        N.check(self._h, self._lib.hs_orb_cancel(self._h, ticket))
        self._tickets.pop(ticket, None)

    def frames_copied(self, ticket):
        """True once the copy-in of `ticket` is complete (its frame buffers may be recycled)"""
        return self._lib.hs_ticket_frames_copied(self._h, ticket) == 1

    def pinned_frames(self, count, h, w):
        """`count` h x w uint8 frames in page-locked host memory (hs_host_alloc): H2D copies from them are plain DMA, no staging.
        The memory is released when the extractor is closed."""
        ptr = C.c_void_p()
        st = self._lib.hs_host_alloc(count * h * w, C.byref(ptr))
        if st != N.HS_OK:
            raise HsError(st, "hs_host_alloc")
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(ptr)
        buf = (C.c_uint8 * (count * h * w)).from_address(ptr.value)
        return np.frombuffer(buf, np.uint8).reshape(count, h, w)

    # ---- device-resident entry points (pointers are plain integers, e.g. torch.Tensor.data_ptr())
    def reserve(self, w, h, batch):
        N.check(self._h, self._lib.hs_orb_reserve(self._h, w, h, batch))

    def extract_batch_device(self, d_imgs, batch, w, h, row_stride, image_stride, d_kps, d_desc, d_n, cap, stream=0):
        N.check(self._h, self._lib.hs_orb_extract_batch_device(self._h, d_imgs, batch, w, h, row_stride, image_stride,
                                                               d_kps, d_desc, d_n, cap, stream or None))

    def landmark_best_descriptors_device(self, d_offsets, L, d_desc, d_best, d_median, stream=0):
        """hs_landmark_best_descriptors_device: d_offsets int64 [L+1], d_desc uint8 [total][32] (16-byte aligned), d_best / d_median int32 [L]"""
        N.check(self._h, self._lib.hs_landmark_best_descriptors_device(self._h, d_offsets, d_desc, L, d_best, d_median, stream or None))

    def landmark_update_entries_device(self, L, d_entries, d_obs_offsets, d_obs, d_desc_offsets, d_desc, d_normal, d_min_dist, d_max_dist,
                                       d_mean_dist, d_size, d_best, d_median, d_flags, d_lms=None, d_lm_index=None, n_lms=0, params=None, stream=0):
        """hs_landmark_update_entries_device: d_entries hs_lm_entry_in [L], d_obs_offsets / d_desc_offsets int64 [L+1], d_obs hs_lm_obs [..],
        d_desc uint8 [..][32] (16-byte aligned); outputs d_normal float [L][3], d_min_dist .. d_size float [L], d_best / d_median / d_flags int32 [L].
        d_lms (hs_landmark [n_lms]) + d_lm_index (int32 [L]): optional scatter target.  `params`: _native.LmEntryParams (default 2.0 / 0.5)."""
        prm = params or N.LmEntryParams()
        N.check(self._h, self._lib.hs_landmark_update_entries_device(self._h, C.byref(prm), L, d_entries, d_obs_offsets, d_obs, d_desc_offsets, d_desc,
                                                                     d_normal, d_min_dist, d_max_dist, d_mean_dist, d_size, d_best, d_median, d_flags,
                                                                     d_lms, d_lm_index, n_lms, stream or None))

    # ---- the local map on device-resident tables (include/hyslam_amd.h): raw device addresses, asynchronous, nothing checked
    def local_points_work_bytes(self, L):
        return int(self._lib.hs_local_points_work_bytes(int(L)))

    def local_map_work_bytes(self, L):
        return int(self._lib.hs_local_map_work_bytes(int(L)))

    def local_keyframes_device(self, n_kf, d_weights, d_kf_bad, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, d_local,
                               d_n_local, stream=0):
        """hs_local_keyframes_device: d_weights int32 [n_kf], d_kf_bad u8 [n_kf], d_neigh int32 [n_kf][neigh_cap], d_parent int32 [n_kf];
        d_local u8 [n_kf], d_n_local int32 [1]"""
        N.check(self._h, self._lib.hs_local_keyframes_device(self._h, n_kf, d_weights, d_kf_bad, d_neigh, neigh_cap, d_parent, n_max_local_keyframes,
                                                             n_neighbor_keyframes, d_local, d_n_local, stream or None))

    def local_points_device(self, table, d_local, d_frame_lm, n_assoc, d_frame_remove, d_sel, cap, d_n_sel, d_work, stream=0):
        """hs_local_points_device: `table` a _native.KfTable of device pointers; d_work: local_points_work_bytes(table.L) bytes"""
        N.check(self._h, self._lib.hs_local_points_device(self._h, C.byref(table), d_local, d_frame_lm, n_assoc, d_frame_remove, d_sel, cap, d_n_sel,
                                                          d_work, stream or None))

    def landmark_gather_device(self, d_lms, L, d_sel, d_n_sel, cap, d_out, stream=0):
        """hs_landmark_gather_device: d_out[j] = d_lms[d_sel[j]] (hs_landmark, 16-byte aligned), skip = 1 past *d_n_sel; exactly cap records"""
        N.check(self._h, self._lib.hs_landmark_gather_device(self._h, d_lms, L, d_sel, d_n_sel, cap, d_out, stream or None))

    def local_map_search_device(self, table, d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, frame,
                                d_lms, proj_params, cap, out, d_work, stream=0):
        """hs_local_map_search_device: vote, key-frame expansion, landmark selection, gather and projection search on one stream.  `table`:
        _native.KfTable, `frame`: _native.FrameView, both of device pointers; `out`: _native.LocalMapOut; d_work: local_map_work_bytes(table.L)"""
        N.check(self._h, self._lib.hs_local_map_search_device(self._h, C.byref(table), d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent,
                                                              n_max_local_keyframes, n_neighbor_keyframes, C.byref(frame), d_lms, C.byref(proj_params),
                                                              cap, C.byref(out), d_work, stream or None))

    # ---- pose-only optimisation on device-resident data (include/hyslam_amd.h): raw device addresses, asynchronous, nothing checked
    def pose_work_bytes(self, Q, n_edges_total):
        return int(self._lib.hs_pose_work_bytes(int(Q), int(n_edges_total)))

    def pose_optimize_device(self, Q, d_problems, d_edges, d_outlier, d_results, d_edge_offsets=None, d_n_edges=None, edge_cap=0, d_work=None, stream=0):
        """hs_pose_optimize_device: d_problems hs_pose_problem [Q], d_edges hs_pose_edge [..] (16-byte aligned), d_outlier u8 [..], d_results
        hs_pose_result [Q]; exactly one of d_edge_offsets (int64 [Q + 1]) and d_n_edges (int32 [1], Q == 1, with edge_cap)"""
        N.check(self._h, self._lib.hs_pose_optimize_device(self._h, Q, d_problems, d_edge_offsets, d_n_edges, edge_cap, d_edges, d_outlier, d_results,
                                                           d_work, stream or None))

    def pose_edges_device(self, frame, d_lms, L, d_kp_lm, d_edges, cap, d_n_edges, sigma_ref=1.0, d_work=None, stream=0):
        """hs_pose_edges_device: `frame` a _native.FrameView of device pointers (kps, uR, n, size_ref are read); d_lms hs_landmark [L]; d_kp_lm int32
        [frame.n]; d_edges hs_pose_edge [cap] in ascending keypoint index, d_n_edges int32 [1] the full count"""
        N.check(self._h, self._lib.hs_pose_edges_device(self._h, C.byref(frame), d_lms, L, d_kp_lm, sigma_ref, d_edges, cap, d_n_edges, d_work,
                                                        stream or None))

    def stereo_match_batch_device(self, d_kpsL, d_descL, d_nL, d_kpsR, d_descR, d_nR, pairs, cap, sp, d_uRight, d_depth, stream=0):
        N.check(self._h, self._lib.hs_stereo_match_batch_device(self._h, d_kpsL, d_descL, d_nL, d_kpsR, d_descR, d_nR, pairs, cap,
                                                                C.byref(sp), d_uRight, d_depth, stream or None))

    def stereo_frontend_batch_device(self, d_left, d_right, pairs, w, h, row_stride, image_stride,
                                     d_kpsL, d_descL, d_nL, d_kpsR, d_descR, d_nR, cap, sp, d_uRight, d_depth, stream=0):
        N.check(self._h, self._lib.hs_stereo_frontend_batch_device(self._h, d_left, d_right, pairs, w, h, row_stride, image_stride,
                                                                   d_kpsL, d_descL, d_nL, d_kpsR, d_descR, d_nR, cap,
                                                                   C.byref(sp), d_uRight, d_depth, stream or None))

    def debug_stream_copy(self, d_dst, d_src, nbytes, width=16, stream=0):
        """measurement utility (hs_debug_stream_copy): a grid-stride copy kernel of `width` (4 or 16) bytes per lane — known HBM traffic"""
        N.check(self._h, self._lib.hs_debug_stream_copy(self._h, d_dst, d_src, nbytes, width, stream or None))

    def set_lanes(self, lanes):
        """1 or 2 internal launch sequences for the batched device entry points (hs_orb_set_lanes)."""
        N.check(self._h, self._lib.hs_orb_set_lanes(self._h, int(lanes)))

    def set_split(self, mode):
        """-1 auto, 0 never, 1 always: level 0's FAST + quadtree on a second stream beside the pyramid (hs_orb_set_split)"""
        N.check(self._h, self._lib.hs_orb_set_split(self._h, int(mode)))

    def synchronize(self, stream=0):
        N.check(self._h, self._lib.hs_orb_synchronize(self._h, stream or None))

    STAGES = ("pyramid", "fast_cells", "quadtree", "describe", "stereo_match", "stereo_median")

    def pyramid_launches(self):
        """kernel launches of the pyramid stage per call (hs_orb_stage_launches)"""
        return max(1, self._lib.hs_orb_stage_launches(self._h, 0))

    def profile_begin(self):
        N.check(self._h, self._lib.hs_orb_profile_begin(self._h))

    def profile_pause(self):
        """stop recording stage events; what was recorded stays for profile_end()"""
        N.check(self._h, self._lib.hs_orb_profile_pause(self._h))

    def profile_end(self):
        """-> {stage: (total_ms, launches)} measured with HIP events on the launch stream."""
        ms = np.zeros(6, np.float64)
        cnt = np.zeros(6, np.int32)
        N.check(self._h, self._lib.hs_orb_profile_end(self._h, ms.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
        return {s: (float(ms[i]), int(cnt[i])) for i, s in enumerate(self.STAGES)}

    # ---- stage taps (parity tests)
    def debug_level(self, image, level):
        buf = np.zeros(1 << 26, np.uint8)
        lw, lh = C.c_int32(), C.c_int32()
        N.check(self._h, self._lib.hs_orb_debug_level(self._h, image, level, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(lw), C.byref(lh)))
        return buf[:lw.value * lh.value].reshape(lh.value, lw.value).copy()

    def set_debug(self, on=True):
        """debug mode: the quadtree stage also gathers the FAST candidates into dense per-level lists (debug_candidates reads them)"""
        N.check(self._h, self._lib.hs_orb_set_debug(self._h, 1 if on else 0))

    def debug_candidates(self, image, level, cap=1 << 20):
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int32()
        N.check(self._h, self._lib.hs_orb_debug_candidates(self._h, image, level, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def debug_selected(self, image, level, cap=1 << 16):
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int32()
        N.check(self._h, self._lib.hs_orb_debug_selected(self._h, image, level, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def debug_quadtree_replay(self, level_first, level_count, reps=20, threads=0):
        """mean milliseconds of the last call's quadtree launch restricted to the given levels (hs_orb_debug_quadtree_replay)"""
        ms = C.c_float()
        N.check(self._h, self._lib.hs_orb_debug_quadtree_replay(self._h, level_first, level_count, threads, reps, C.byref(ms)))
        return float(ms.value)


def stereo_params(camera, settings=None, size_ref=31.0):
    settings = settings or FeatureMatcherSettings()
    return N.StereoParams(camera.fx(), camera.mbf, int(camera.mnMaxY), settings.TH_HIGH, settings.TH_LOW, size_ref)


class Stereomatcher:
    """HYSLAM::Stereomatcher (src/features/Stereomatcher.h:25-51): construct from the left/right views, the camera and the
    matcher settings, call computeStereoMatches(), read uRight/depth with getData()."""

    def __init__(self, keys, keysR, descriptors, descriptorsR, camera, settings=None, extractor=None, size_ref=31.0):
        self.mvKeys = np.ascontiguousarray(keys, KP_DTYPE)
        self.mvKeysRight = np.ascontiguousarray(keysR, KP_DTYPE)
        self.mDescriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        self.mDescriptorsRight = np.ascontiguousarray(descriptorsR, np.uint8).reshape(-1, 32)
        self.sp = stereo_params(camera, settings, size_ref)
        self._ex = extractor or ORBExtractor()
        self.mvuRight = np.full(len(self.mvKeys), -1.0, np.float32)
        self.mvDepth = np.full(len(self.mvKeys), -1.0, np.float32)

    def computeStereoMatches(self):
        ex = self._ex
        nL, nR = len(self.mvKeys), len(self.mvKeysRight)
        self.mvuRight = np.full(nL, -1.0, np.float32)
        self.mvDepth = np.full(nL, -1.0, np.float32)
        # both views still on the device (published by the extractor)?  Then only the results cross the bus (hs_stereo_match_frames).
        self.frames_on_device = False
        tl, tr = (ex.find_frame(self.mvKeys), ex.find_frame(self.mvKeysRight)) if nL > 0 and nR > 0 else (0, 0)
        if tl and tr:
            st = ex._lib.hs_stereo_match_frames(ex._h, C.c_uint64(tl), C.c_uint64(tr), C.byref(self.sp), self.mvuRight.ctypes.data_as(C.c_void_p), self.mvDepth.ctypes.data_as(C.c_void_p))
            if st == N.HS_OK:
                self.frames_on_device = True
                return
            if st != N.HS_ERR_INVALID:                       # (INVALID: a slot was reused between find and use — fall back to the host arrays)
                N.check(ex._h, st)
        N.check(ex._h, ex._lib.hs_stereo_match(ex._h, self.mvKeys.ctypes.data_as(C.c_void_p), self.mDescriptors.ctypes.data_as(C.c_void_p), nL,
                                               self.mvKeysRight.ctypes.data_as(C.c_void_p), self.mDescriptorsRight.ctypes.data_as(C.c_void_p), nR,
                                               C.byref(self.sp), self.mvuRight.ctypes.data_as(C.c_void_p),
                                               self.mvDepth.ctypes.data_as(C.c_void_p)))

    def getData(self):
        return self.mvuRight, self.mvDepth


class FeatureMatcher:
    """HYSLAM::FeatureMatcher (src/features/FeatureMatcher.h:105-176) on flat arrays.  `frame` is a _native.FrameView,
    `landmarks` a numpy array of _native.LM_DTYPE (one record per MapPoint, in the order the reference would iterate them)."""

    def __init__(self, settings=None, extractor=None):
        s = settings or FeatureMatcherSettings()
        self.mfNNratio, self.mbCheckOrientation, self.TH_LOW, self.TH_HIGH = s.nnratio, s.checkOri, s.TH_LOW, s.TH_HIGH
        self._ex = extractor or ORBExtractor()

    def _project(self, frame, landmarks, pp):
        ex = self._ex
        lms = np.ascontiguousarray(landmarks, N.LM_DTYPE)
        L = len(lms)
        midx = np.full(L, -1, np.int32)
        mdist = np.full(L, -1, np.float32)
        n = C.c_int32()
        self.frame_on_device = False
        if frame.n > 0 and frame.kps:                          # the frame's keypoints / descriptors still on the device?  (hs_frame_find + hs_search_by_projection_frame)
            tok = C.c_uint64(0)
            if ex._lib.hs_frame_find(ex.device, frame.kps, frame.n, C.byref(tok)) == N.HS_OK and tok.value:
                st = ex._lib.hs_search_by_projection_frame(ex._h, tok, C.byref(frame), lms.ctypes.data_as(C.c_void_p), L, C.byref(pp),
                                                           midx.ctypes.data_as(C.c_void_p), mdist.ctypes.data_as(C.c_void_p), C.byref(n))
                if st == N.HS_OK:
                    self.frame_on_device = True
                    return midx, mdist, n.value
                if st != N.HS_ERR_INVALID:
                    N.check(ex._h, st)
        N.check(ex._h, ex._lib.hs_search_by_projection(ex._h, C.byref(frame), lms.ctypes.data_as(C.c_void_p), L, C.byref(pp),
                                                       midx.ctypes.data_as(C.c_void_p), mdist.ctypes.data_as(C.c_void_p), C.byref(n)))
        return midx, mdist, n.value

    def SearchByProjection(self, frame, landmarks, th=3.0):
        """SearchByProjection(Frame&, vector<MapPoint*>&, th) — track the local map (FeatureMatcher.cc:123-143)."""
        return self._project(frame, landmarks, N.ProjParams(th, self.TH_HIGH, self.mfNNratio, 0.5, 1.5, 1, 1, 0))

    def SearchByProjectionLastFrame(self, frame, landmarks, th):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (FeatureMatcher.cc:145-176): landmarks = LastFrame's map points,
        prev_angle = angle of each one's keypoint in LastFrame."""
        return self._project(frame, landmarks, N.ProjParams(th, self.TH_HIGH, self.mfNNratio, 0.5, 1.5, 0, 1, 1))

    def SearchByProjectionKeyFrame(self, frame, landmarks, th, ORBdist):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) — relocalisation (FeatureMatcher.cc:180-212);
        landmarks = pKF's map points minus sAlreadyFound.  Its rotation criterion is a no-op in the reference (no previous frame)."""
        return self._project(frame, landmarks, N.ProjParams(th, float(ORBdist), 1.0, 0.5, 1.5, 1, 0, 0))

    def SearchForInitialization(self, kps1, desc1, frame2, vbPrevMatched, windowSize=10):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (FeatureMatcher.cc:404-462).  frame2 is a FrameView (grid
        bounds + keypoints + descriptors).  Returns (vnMatches12, updated vbPrevMatched, number of matches)."""
        ex = self._ex
        k1 = np.ascontiguousarray(kps1, KP_DTYPE); d1 = np.ascontiguousarray(desc1, np.uint8)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2).copy()
        m = np.full(len(k1), -1, np.int32)
        n = C.c_int32()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_search_for_initialization(ex._h, p(k1), p(d1), len(k1), C.byref(frame2), p(prev), int(windowSize),
                                                            self.TH_LOW, self.mfNNratio, p(m), C.byref(n)))
        return m, prev, n.value

    def Fuse(self, keyframe, landmarks, th=3.0, reprojection_err=5.99):
        """Fuse(pKF, vpMapPoints, fuse_matches, th, reprojection_err) (FeatureMatcher.cc:464-521).  The caller sets skip = 1 on landmarks
        that are bad, already observed in pKF or protected (:480-485).  Returns per-landmark keypoint indices (first landmark per keypoint)."""
        return self._project(keyframe, landmarks, N.ProjParams(th, self.TH_LOW, 1.0, 0.5, 1.5, use_distance=1, use_stereo=0, check_rotation=0,
                                                               use_prev_matched=0, use_viewing_angle=1, max_view_angle=1.047,
                                                               use_reprojection=1, reproj_threshold=reprojection_err, sigma_ref=1.0, first_wins=1))

    def SearchByProjectionSim3(self, keyframe, Scw, landmarks, vpMatched, th):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) — loop detection, legacy (FeatureMatcher.cc:628-737).  landmarks: min_dist / max_dist =
        the invariance range, skip = bad or already found; vpMatched: uint8[n] (keypoint already has a loop match).  Returns (match per landmark,
        updated vpMatched flags, nmatches)."""
        ex = self._ex
        lms = np.ascontiguousarray(landmarks, N.LM_DTYPE)
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        taken = np.ascontiguousarray(vpMatched, np.uint8).copy()
        midx = np.full(len(lms), -1, np.int32)
        n = C.c_int32()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_search_by_projection_sim3(ex._h, C.byref(keyframe), p(S), p(lms), len(lms), int(th), self.TH_LOW, p(taken), p(midx), C.byref(n)))
        return midx, taken, n.value

    def SearchBySim3(self, kf1, landmarks1, kf2, landmarks2, s12, R12, t12, th):
        """SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) — loop closing, legacy (FeatureMatcher.cc:739-934).  landmarks1[n1] / landmarks2[n2]:
        the landmark of every keypoint (skip = none / bad / already matched).  Returns (match12[n1], nFound)."""
        ex = self._ex
        l1 = np.ascontiguousarray(landmarks1, N.LM_DTYPE); l2 = np.ascontiguousarray(landmarks2, N.LM_DTYPE)
        R = np.ascontiguousarray(R12, np.float32).reshape(9); t = np.ascontiguousarray(t12, np.float32).reshape(3)
        m = np.full(kf1.n, -1, np.int32)
        n = C.c_int32()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_search_by_sim3(ex._h, C.byref(kf1), p(l1), C.byref(kf2), p(l2), float(s12), p(R), p(t), float(th), self.TH_HIGH, p(m), C.byref(n)))
        return m, n.value

    def SearchForTriangulation(self, kps1, desc1, featvec1, kps2, desc2, featvec2, F12, keep1=None, keep2=None, size_ref=31.0, sigma_ref=1.0):
        """The matching core of SearchForTriangulation (FeatureMatcher.cc:373-402): keep1/keep2 = keypoints WITHOUT a landmark (and with a
        stereo observation when bOnlyStereo), epipolar gate with F12, best match under TH_LOW with ratio 1.0, rotation check."""
        return self.SearchByBoW(kps1, desc1, featvec1, kps2, desc2, featvec2, keep1, True, keep2=keep2, F12=F12, ratio=1.0,
                                size_ref=size_ref, sigma_ref=sigma_ref)

    def SearchByBoWLegacy(self, kps1, desc1, featvec1, kps2, desc2, featvec2, keep1=None, keep2=None):
        """the legacy SearchByBoW(pKF1, pKF2, vpMatches12) (FeatureMatcher.cc:938-1077): a key-frame-2 feature is matched at most once, the
        orientation histogram takes angle1 - angle2.  keep1 / keep2 = views with a good landmark.  Returns (match12, nmatches)."""
        ex = self._ex
        k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        a = [np.ascontiguousarray(x, np.int32) for x in featvec1]; b = [np.ascontiguousarray(x, np.int32) for x in featvec2]
        kp1 = None if keep1 is None else np.ascontiguousarray(keep1, np.uint8)
        kp2 = None if keep2 is None else np.ascontiguousarray(keep2, np.uint8)
        m = np.full(len(k1), -1, np.int32)
        n = C.c_int32()
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_search_by_bow_legacy(ex._h, p(k1), p(d1), len(k1), p(a[0]), p(a[1]), p(a[2]), len(a[0]),
                                                       p(k2), p(d2), len(k2), p(b[0]), p(b[1]), p(b[2]), len(b[0]),
                                                       p(kp1), p(kp2), self.TH_LOW, self.mfNNratio, int(self.mbCheckOrientation), p(m), C.byref(n)))
        return m, n.value

    def SearchByBoW(self, kps1, desc1, featvec1, kps2, desc2, featvec2, keep1=None, check_rotation=True, keep2=None, F12=None, ratio=None,
                    size_ref=31.0, sigma_ref=1.0):
        """The matching core of SearchByBoW / SearchByBoW2 (FeatureMatcher.cc:216-371).  featvec = (node_id, node_ptr, idx) CSR arrays."""
        ex = self._ex
        k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        a = [np.ascontiguousarray(x, np.int32) for x in featvec1]
        b = [np.ascontiguousarray(x, np.int32) for x in featvec2]
        keep = None if keep1 is None else np.ascontiguousarray(keep1, np.uint8)
        kp2 = None if keep2 is None else np.ascontiguousarray(keep2, np.uint8)
        Fm = None if F12 is None else np.ascontiguousarray(F12, np.float32).reshape(9)
        m = np.full(len(k1), -1, np.int32)
        n = C.c_int32()
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_search_by_bow_ex(ex._h, p(k1), p(d1), len(k1), p(a[0]), p(a[1]), p(a[2]), len(a[0]),
                                                   p(k2), p(d2), len(k2), p(b[0]), p(b[1]), p(b[2]), len(b[0]),
                                                   p(keep), p(kp2), p(Fm), size_ref, sigma_ref, self.TH_LOW,
                                                   self.mfNNratio if ratio is None else ratio, int(check_rotation), p(m), C.byref(n)))
        return m, n.value

    def HammingKnn2(self, query, train):
        ex = self._ex
        q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
        bi, bd, sd = (np.zeros(len(q), np.int32) for _ in range(3))
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_hamming_knn2(ex._h, p(q), len(q), p(t), len(t), p(bi), p(bd), p(sd)))
        return bi, bd, sd


    def ComputeDistinctiveDescriptors(self, descriptors=None, offsets=None, desc=None):
        """MapPointDBEntry::_computeDistinctiveDescriptor_ (src/core/MapPointDB.cpp:128-175) for a batch of landmarks, in one call.
        Either `descriptors`, a list of (N_i, 32) uint8 arrays (one per landmark, observations in the order the reference's std::map would
        walk them), or CSR arrays `offsets` [L+1] and `desc` [offsets[L]][32].  Returns (best, median), int32 [L]: the index within the
        landmark of its representative descriptor and that row's median Hamming distance; -1 / -1 for a landmark without descriptors."""
        if descriptors is not None:
            if offsets is not None or desc is not None:
                raise ValueError("pass either descriptors or offsets + desc")
            rows = [np.asarray(d, np.uint8).reshape(-1, 32) for d in descriptors]
            off = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=off[1:])
            d = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 32), np.uint8))
        else:
            if offsets is None or desc is None:
                raise ValueError("pass either descriptors or offsets + desc")
            off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
            d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
            if len(off) < 1 or off[-1] > len(d):
                raise ValueError("offsets[L] exceeds the number of descriptors")
        L = len(off) - 1
        best, median = np.zeros(L, np.int32), np.zeros(L, np.int32)
        ex = self._ex
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_landmark_best_descriptors(ex._h, p(off), p(d), L, p(best), p(median)))
        return best, median

    @staticmethod
    def _csr(parts, offsets, flat, dtype, row, what):
        """a list of per-landmark arrays, or CSR `offsets` [L+1] + `flat` -> (int64 offsets, contiguous rows of shape `row`)"""
        if parts is not None and offsets is None and flat is None:
            rows = [np.ascontiguousarray(x, dtype).reshape((-1,) + row) for x in parts]
            off = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=off[1:])
            return off, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0,) + row, dtype))
        if parts is None and offsets is not None and flat is not None:
            off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
            f = np.ascontiguousarray(flat, dtype).reshape((-1,) + row)
            if len(off) < 1 or off[-1] > len(f):
                raise ValueError("%s offsets[L] exceeds the number of rows" % what)
            return off, f
        raise ValueError("pass either the %s list or its offsets + flat array" % what)

    def UpdateLandmarkEntries(self, entries, observations=None, descriptors=None, obs_offsets=None, obs=None, desc_offsets=None, desc=None,
                              max_dist_factor=2.0, min_dist_factor=0.5):
        """MapPointDBEntry::_updateEntry_ (src/core/MapPointDB.cpp:223-310) for a batch of landmarks, in one call: normal and depth range,
        representative descriptor, mean distance and size.  `entries`: _native.LM_ENTRY_DTYPE [L] (world position, reference key frame's camera
        centre).  Observations: either `observations`, a list of _native.LM_OBS_DTYPE arrays (one per landmark, in the reference's std::map order),
        or CSR `obs_offsets` [L+1] + `obs`.  Descriptor sets (isBad() key frames left out): `descriptors`, a list of (N_i, 32) uint8 arrays, or
        `desc_offsets` [L+1] + `desc`.  Returns a dict of normal (L, 3), min_dist, max_dist, mean_dist, size (float32 [L]), best, median, flags
        (int32 [L]).  Where the reference leaves an output unchanged (flags without HS_LM_SET_NORMAL_DEPTH / HS_LM_SET_MEAN) it holds NaN here."""
        ent = np.ascontiguousarray(entries, N.LM_ENTRY_DTYPE).reshape(-1)
        ooff, ob = self._csr(observations, obs_offsets, obs, N.LM_OBS_DTYPE, (), "observation")
        doff, d = self._csr(descriptors, desc_offsets, desc, np.uint8, (32,), "descriptor")
        L = len(ent)
        if len(ooff) != L + 1 or len(doff) != L + 1:
            raise ValueError("entries, observations and descriptors must describe the same number of landmarks")
        out = dict(normal=np.full((L, 3), np.nan, np.float32), min_dist=np.full(L, np.nan, np.float32), max_dist=np.full(L, np.nan, np.float32),
                   mean_dist=np.full(L, np.nan, np.float32), size=np.full(L, np.nan, np.float32), best=np.zeros(L, np.int32),
                   median=np.zeros(L, np.int32), flags=np.zeros(L, np.int32))
        ex = self._ex
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        prm = N.LmEntryParams(max_dist_factor, min_dist_factor)
        N.check(ex._h, ex._lib.hs_landmark_update_entries(ex._h, C.byref(prm), L, p(ent), p(ooff), p(ob), p(doff), p(d),
                                                          *[p(out[k]) for k in ("normal", "min_dist", "max_dist", "mean_dist", "size", "best", "median", "flags")]))
        return out

    @staticmethod
    def _kf_table(table):
        """the observation table of the key-frame graph calls -> (_native.KfTable, the arrays it points into).  `table`: a dict with kf_bad, kf_id
        [n_kf], lm_bad, lm_nobs [L] (each optional: zeros / the CSR lengths) and the landmarks' observations either as `observations`, a list per
        landmark of (slot, octave) rows in ascending slot order, or as CSR lm_obs_offsets [L+1] + lm_obs_kf + lm_obs_octave (octave optional)."""
        if "observations" in table:
            rows = [np.asarray(o, np.int32).reshape(-1, 2) for o in table["observations"]]
            off = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=off[1:])
            flat = np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)
            kf, octv = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
        else:
            off = np.ascontiguousarray(table["lm_obs_offsets"], np.int64).reshape(-1)
            kf = np.ascontiguousarray(table["lm_obs_kf"], np.int32).reshape(-1)
            octv = np.ascontiguousarray(table["lm_obs_octave"], np.int32).reshape(-1) if table.get("lm_obs_octave") is not None else np.zeros(len(kf), np.int32)
            if len(off) < 1 or off[-1] > len(kf) or len(octv) != len(kf):
                raise ValueError("lm_obs_offsets[L] exceeds the number of observations")
        L = len(off) - 1
        lm_bad = np.ascontiguousarray(table["lm_bad"], np.uint8).reshape(-1) if table.get("lm_bad") is not None else np.zeros(L, np.uint8)
        lm_nobs = np.ascontiguousarray(table["lm_nobs"], np.int32).reshape(-1) if table.get("lm_nobs") is not None else np.diff(off).astype(np.int32)
        if table.get("kf_id") is not None:
            kf_id = np.ascontiguousarray(table["kf_id"], np.int64).reshape(-1)
        else:
            kf_id = np.arange(int(table["n_kf"]) if "n_kf" in table else (int(kf.max()) + 1 if len(kf) else 0), dtype=np.int64)
        kf_bad = np.ascontiguousarray(table["kf_bad"], np.uint8).reshape(-1) if table.get("kf_bad") is not None else np.zeros(len(kf_id), np.uint8)
        if len(lm_bad) != L or len(lm_nobs) != L or len(kf_bad) != len(kf_id):
            raise ValueError("the per-landmark / per-key-frame arrays do not match the table")
        keep = (off, kf, octv, lm_bad, lm_nobs, kf_bad, kf_id)
        return N.KfTable(L, len(kf_id), *[a.ctypes.data for a in keep]), keep

    def KeyFrameVotes(self, table, queries=None, q_offsets=None, q_lm=None, self_id=None, count_bad_kf=False, th=15, cap=10, weights=True):
        """The key-frame counter of CovisNode::UpdateConnections (src/core/CovisibilityGraph.cpp:42-124; count_bad_kf=False, self_id = the node's
        mnId) or TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:80-123; count_bad_kf=True) for a batch of queries, and what
        the reference derives from it.  `table`: see _kf_table.  Queries: either `queries`, a list of landmark-index arrays, or CSR `q_offsets`
        [Q+1] + `q_lm`.  `self_id` [Q] (None: nothing excluded).  Returns a dict: weights (Q, n_kf) (None with weights=False), max_slot, max_count,
        n_ordered [Q], ordered_slot, ordered_weight (Q, cap): the entries with count >= th (or the single maximum) by descending weight, then
        descending slot; rows padded with -1 / 0; n_ordered holds the full length.  With cap=10 a row is a `neigh` row of PlaceRecognizer."""
        T, keep = self._kf_table(table)
        qoff, ql = self._csr(queries, q_offsets, q_lm, np.int32, (), "query")
        Q = len(qoff) - 1
        sid = None if self_id is None else np.ascontiguousarray(self_id, np.int64).reshape(-1)
        if sid is not None and len(sid) != Q:
            raise ValueError("self_id must have one entry per query")
        out = dict(weights=np.zeros((Q, T.n_kf), np.int32) if weights else None, max_slot=np.zeros(Q, np.int32), max_count=np.zeros(Q, np.int32),
                   ordered_slot=np.zeros((Q, cap), np.int32), ordered_weight=np.zeros((Q, cap), np.int32), n_ordered=np.zeros(Q, np.int32))
        ex = self._ex
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_kf_votes(ex._h, C.byref(T), Q, p(qoff), p(ql), p(sid), int(bool(count_bad_kf)), int(th), p(out["weights"]),
                                           p(out["max_slot"]), p(out["max_count"]), p(out["ordered_slot"]), p(out["ordered_weight"]), int(cap),
                                           p(out["n_ordered"])))
        return out

    def KeyFrameRedundancy(self, table, cand_slot, cand_th_depth, items=None, cand_offsets=None, item_lm=None, item_octave=None, item_depth=None,
                           is_mono=False, th_obs=3, frac_redundant=0.9):
        """KeyFrameCuller::run's verdict (src/slam/mapping/KeyFrameCuller.cpp:33-86) for every candidate against ONE snapshot of the map (`table`,
        see _kf_table): a pure function of the snapshot — SetBadKeyFrame on a culled candidate changes the map, so cull the first candidate with
        cull = 1, regather and ask again for those behind it.  Candidates: slot and mThDepth, and their keypoints that hold a landmark either as
        `items`, a list per candidate of (landmark, octave, depth) rows, or as CSR `cand_offsets` [C+1] + item_lm + item_octave + item_depth.
        Returns a dict of n_mps, n_redundant (int32 [C]) and cull (uint8 [C])."""
        T, keep = self._kf_table(table)
        slot = np.ascontiguousarray(cand_slot, np.int32).reshape(-1)
        thd = np.ascontiguousarray(cand_th_depth, np.float32).reshape(-1)
        if items is not None:
            if cand_offsets is not None or item_lm is not None:
                raise ValueError("pass either the items list or cand_offsets + item arrays")
            rows = [np.asarray(r, np.float64).reshape(-1, 3) for r in items]
            coff = np.zeros(len(rows) + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=coff[1:])
            flat = np.concatenate(rows) if rows else np.zeros((0, 3))
            ilm, ioct, idep = (np.ascontiguousarray(flat[:, 0], np.int32), np.ascontiguousarray(flat[:, 1], np.int32), np.ascontiguousarray(flat[:, 2], np.float32))
        else:
            coff = np.ascontiguousarray(cand_offsets, np.int64).reshape(-1)
            ilm = np.ascontiguousarray(item_lm, np.int32).reshape(-1)
            ioct = np.ascontiguousarray(item_octave, np.int32).reshape(-1)
            idep = np.ascontiguousarray(item_depth, np.float32).reshape(-1) if item_depth is not None else np.zeros(len(ilm), np.float32)
            if len(coff) < 1 or coff[-1] > len(ilm) or len(ioct) != len(ilm) or len(idep) != len(ilm):
                raise ValueError("cand_offsets[C] exceeds the number of items")
        Cn = len(coff) - 1
        if len(slot) != Cn or len(thd) != Cn:
            raise ValueError("cand_slot, cand_th_depth and the items must describe the same number of candidates")
        out = dict(n_mps=np.zeros(Cn, np.int32), n_redundant=np.zeros(Cn, np.int32), cull=np.zeros(Cn, np.uint8))
        ex = self._ex
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_kf_redundancy(ex._h, C.byref(T), Cn, p(slot), p(thd), p(coff), p(ilm), p(ioct), p(idep), int(bool(is_mono)),
                                                int(th_obs), float(frac_redundant), p(out["n_mps"]), p(out["n_redundant"]), p(out["cull"])))
        return out

    def LocalKeyFrames(self, weights, kf_bad, neigh, parent, n_max_local_keyframes=80, n_neighbor_keyframes=10):
        """The key-frame expansion of TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:106-156).  weights [n_kf]: a row of
        KeyFrameVotes(count_bad_kf=True); kf_bad [n_kf]; neigh (n_kf, neigh_cap): each slot's ordered covisibility list padded with -1; parent
        [n_kf], -1 = none.  The live set is walked in ascending slot order as the reference walks its std::set while inserting; the walk ends at
        the first visited slot that has a parent.  Returns (local uint8 [n_kf], n_local)."""
        w = np.ascontiguousarray(weights, np.int32).reshape(-1)
        n_kf = len(w)
        bad = np.ascontiguousarray(kf_bad, np.uint8).reshape(-1)
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        ng = np.ascontiguousarray(neigh, np.int32).reshape(n_kf, -1) if n_kf else np.zeros((0, 0), np.int32)
        if len(bad) != n_kf or len(par) != n_kf:
            raise ValueError("weights, kf_bad, neigh and parent must describe the same number of key frames")
        local, n_local = np.zeros(n_kf, np.uint8), np.zeros(1, np.int32)
        ex = self._ex
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_local_keyframes(ex._h, n_kf, p(w), p(bad), p(ng), ng.shape[1], p(par), int(n_max_local_keyframes),
                                                  int(n_neighbor_keyframes), p(local), p(n_local)))
        return local, int(n_local[0])

    def LocalPoints(self, table, local, frame_lm, cap=None):
        """TrackLocalMap::UpdateLocalPoints (:166-184) with the filter at the head of SearchLocalPoints (:55-67).  `table`: see _kf_table; local
        [n_kf]: the set of LocalKeyFrames; frame_lm: the frame's associations as landmark indices, -1 = null.  Returns (frame_remove uint8
        [n_assoc], sel int32 [cap], n_sel): sel lists in ascending index the landmarks that are not bad, are observed by a local key frame and are
        not held by the frame through a good association, padded with -1; n_sel is the full count.  cap=None: room for every landmark."""
        T, keep = self._kf_table(table)
        loc = np.ascontiguousarray(local, np.uint8).reshape(-1)
        flm = np.ascontiguousarray(frame_lm, np.int32).reshape(-1)
        if len(loc) != T.n_kf:
            raise ValueError("local must have one entry per key frame")
        cap = T.L if cap is None else int(cap)
        rem, sel, n_sel = np.zeros(len(flm), np.uint8), np.zeros(cap, np.int32), np.zeros(1, np.int32)
        ex = self._ex
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_local_points(ex._h, C.byref(T), p(loc), p(flm), len(flm), p(rem), p(sel), cap, p(n_sel)))
        return rem, sel, int(n_sel[0])


class Optimizer:
    """HYSLAM::Optimizer::PoseOptimization (src/optimizers/Optimizer.cc:48-279) on flat arrays: the frame's pose against the landmarks its keypoints
    hold, four rounds of Levenberg-Marquardt with outlier classification, computed by one HIP launch (include/hyslam_amd.h)."""

    def __init__(self, extractor=None):
        self._ex = extractor or ORBExtractor()

    @staticmethod
    def pose_edges(kps, uR, kp_lm, landmarks, size_ref=31.0, sigma_ref=1.0):
        """The edge list the reference builds at Optimizer.cc:94-188: one _native.POSE_EDGE_DTYPE record per keypoint i with 0 <= kp_lm[i] <
        len(landmarks), in ascending i.  kps: KP_DTYPE; uR float32 [n] (< 0: monocular); landmarks: LM_DTYPE records or an (L, 3) position array."""
        kp_lm = np.asarray(kp_lm, np.int32).reshape(-1)
        pos = landmarks["pos"] if getattr(landmarks, "dtype", None) is not None and landmarks.dtype.names else np.asarray(landmarks, np.float32).reshape(-1, 3)
        idx = np.nonzero((kp_lm >= 0) & (kp_lm < len(pos)))[0]
        e = np.zeros(len(idx), N.POSE_EDGE_DTYPE)
        e["Xw"], e["u"], e["v"], e["kp"] = pos[kp_lm[idx]], kps["x"][idx], kps["y"][idx], idx
        e["ur"] = np.asarray(uR, np.float32).reshape(-1)[idx]
        with np.errstate(all="ignore"):
            s = kps["size"][idx].astype(np.float32) / np.float32(size_ref)             # determineSigma2, in float as the reference
            e["inv_sigma2"] = np.float32(1.0) / (np.float32(sigma_ref) * (s * s))
        return e

    def PoseOptimizationBatch(self, poses, cameras, edge_lists):
        """Q independent problems in one call.  poses: Q float32 4x4 (pFrame->mTcw); cameras: Q of (fx, fy, cx, cy, bf); edge_lists: Q arrays of
        POSE_EDGE_DTYPE.  Returns (results POSE_RESULT_DTYPE [Q], outlier uint8 arrays per problem — all zero for a problem with fewer than 3 edges,
        which is not optimised)."""
        Q = len(poses)
        prob = np.zeros(Q, N.POSE_PROBLEM_DTYPE)
        for q in range(Q):
            prob["Tcw"][q] = np.asarray(poses[q], np.float32).reshape(16)
            prob["fx"][q], prob["fy"][q], prob["cx"][q], prob["cy"][q], prob["bf"][q] = [np.float32(c) for c in cameras[q]]
        lists = [np.ascontiguousarray(e, N.POSE_EDGE_DTYPE).reshape(-1) for e in edge_lists]
        off = np.zeros(Q + 1, np.int64)
        off[1:] = np.cumsum([len(e) for e in lists])
        edges = np.concatenate(lists) if Q else np.zeros(0, N.POSE_EDGE_DTYPE)
        outlier, res = np.zeros(len(edges), np.uint8), np.zeros(Q, N.POSE_RESULT_DTYPE)
        ex = self._ex
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_pose_optimize(ex._h, Q, p(prob), p(off), p(edges), p(outlier), p(res)))
        return res, [outlier[off[q]:off[q + 1]] for q in range(Q)]

    def PoseOptimization(self, frame_pose, camera, edges=None, kps=None, uR=None, kp_lm=None, landmarks=None, size_ref=31.0, sigma_ref=1.0):
        """int Optimizer::PoseOptimization(Frame*).  frame_pose: pFrame->mTcw (4x4); camera: (fx, fy, cx, cy, bf); either `edges` (POSE_EDGE_DTYPE)
        or the frame's arrays (kps, uR, kp_lm, landmarks) from which pose_edges gathers them.  Returns (Tcw float32 4x4 — the pose handed to SetPose,
        the input pose when fewer than 3 keypoints hold a landmark; outlier uint8 per KEYPOINT INDEX — 1 where the reference calls
        setOutlier(i, true); n_good — the return value)."""
        if edges is None:
            edges = self.pose_edges(kps, uR, kp_lm, landmarks, size_ref, sigma_ref)
            n_kp = len(kps)
        else:
            edges = np.ascontiguousarray(edges, N.POSE_EDGE_DTYPE).reshape(-1)
            n_kp = int(edges["kp"].max()) + 1 if len(edges) else 0
        res, (flags,) = self.PoseOptimizationBatch([frame_pose], [camera], [edges])
        outlier = np.zeros(n_kp, np.uint8)
        outlier[edges["kp"]] = flags
        return res["Tcw"][0].reshape(4, 4).copy(), outlier, int(res["n_good"][0])


def _ransac_words(seed, cap, set, stride):
    """the words the generator of DESIGN.md D18 gives iterations 0 .. cap-1 of a solver that draws `set` per iteration, as rows of a draws table of
    `stride` words: SplitMix64's finaliser on the counters seed + it * set + k (the elements of synth.splitmix64(0, .) from index `seed` on, formed
    directly because a seed may be any 64-bit number)"""
    w = np.zeros((cap, stride), np.uint32)
    with np.errstate(over="ignore"):
        c = np.uint64(seed) + np.arange(cap * set, dtype=np.uint64)
        z = (c + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    w[:, :set] = (z >> np.uint64(32)).astype(np.uint32).reshape(cap, set)
    return w


def _ransac_iterate(solvers, nIterations, entry, stride, sets, result_dtype):
    """what PnPsolver.iterate_batch and Sim3Solver.iterate_batch share: ONE call of `entry` (hs_pnp_iterate / hs_sim3_iterate) for all solvers, whose
    draws tables have `stride` words a row and who draw sets[q] per iteration; every solver's state, best_mask and result are brought up to date.
    Returns (res, inl, off): the results, the concatenated inlier masks and the offsets of the solvers' correspondences in them."""
    ex, Q = solvers[0]._ex, len(solvers)
    par = np.concatenate([s.params() for s in solvers])
    off = np.zeros(Q + 1, np.int64)
    off[1:] = np.cumsum([len(s.corrs) for s in solvers])
    corrs = np.concatenate([s.corrs for s in solvers])
    cap = max([0] + [len(s.draws) for s in solvers if s.draws is not None])
    draws = np.zeros((Q, cap, stride), np.uint32)
    for q, s in enumerate(solvers):
        if cap and (s.draws is None or len(s.draws) < cap):        # a table shorter than the call's: the generator's own words fill it
            draws[q] = _ransac_words(s.seed, cap, sets[q], stride)
        if s.draws is not None:
            draws[q, :len(s.draws)] = s.draws
    states = np.concatenate([s.state for s in solvers])
    best = np.concatenate([s.best_mask for s in solvers])
    inl, res = np.zeros(len(corrs), np.uint8), np.zeros(Q, result_dtype)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    N.check(ex._h, getattr(ex._lib, entry)(ex._h, Q, p(par), p(off), p(corrs), int(nIterations), p(draws) if cap else None, cap, p(states), p(best), p(res), p(inl)))
    for q, s in enumerate(solvers):
        s.state, s.best_mask, s.result = states[q:q + 1].copy(), best[off[q]:off[q + 1]].copy(), res[q].copy()
    return res, inl, off


class PnPsolver:
    """HYSLAM::PnPsolver (src/estimators/PnPsolver.h:61-72) on flat arrays: EPnP inside RANSAC for one candidate key frame, computed by
    hs_pnp_iterate (include/hyslam_amd.h).  Built from the frame's arrays — kps (KP_DTYPE), the landmark positions and matches
    (matches[i] = landmark index of keypoint i, or < 0: no landmark / a bad one), in ascending keypoint index as the reference's constructor walks
    them — or from ready correspondences (PNP_CORR_DTYPE).  camera: (fx, fy, cx, cy).  `seed` replaces the process-wide rand() stream the
    reference's solvers share; `draws` (uint32 [cap, HS_PNP_MAX_SET]) directs the samples of the first cap iterations."""

    def __init__(self, camera, kps=None, landmarks=None, matches=None, corrs=None, n_keypoints=None, size_ref=31.0, sigma_ref=1.0, seed=0, draws=None,
                 extractor=None):
        self._ex = extractor or ORBExtractor()
        if corrs is None:
            corrs = self.correspondences(kps, landmarks, matches, size_ref, sigma_ref)
            n_keypoints = len(kps)
        self.corrs = np.ascontiguousarray(corrs, N.PNP_CORR_DTYPE).reshape(-1)
        self.n_keypoints = int(n_keypoints) if n_keypoints is not None else (int(self.corrs["kp"].max()) + 1 if len(self.corrs) else 0)
        self.camera = tuple(np.float32(c) for c in camera[:4])
        self.seed = int(seed)
        self.draws = None if draws is None else np.ascontiguousarray(draws, np.uint32).reshape(-1, N.HS_PNP_MAX_SET)
        self.state = np.zeros(1, N.PNP_STATE_DTYPE)
        self.best_mask = np.zeros(len(self.corrs), np.uint8)
        self.result = None
        self.SetRansacParameters()

    @staticmethod
    def correspondences(kps, landmarks, matches, size_ref=31.0, sigma_ref=1.0):
        """PnPsolver.cc:69-116: one record per keypoint i with 0 <= matches[i] < len(landmarks), in ascending i; sigma2 = determineSigma2(kp.size)
        in float, the quantity whose reciprocal hs_pose_edge::inv_sigma2 holds."""
        matches = np.asarray(matches, np.int64).reshape(-1)
        pos = landmarks["pos"] if getattr(landmarks, "dtype", None) is not None and landmarks.dtype.names else np.asarray(landmarks, np.float32).reshape(-1, 3)
        idx = np.nonzero((matches >= 0) & (matches < len(pos)))[0]
        c = np.zeros(len(idx), N.PNP_CORR_DTYPE)
        c["Xw"], c["u"], c["v"], c["kp"] = pos[matches[idx]], kps["x"][idx], kps["y"][idx], idx
        s = kps["size"][idx].astype(np.float32) / np.float32(size_ref)
        c["sigma2"] = np.float32(sigma_ref) * (s * s)
        return c

    def params(self):
        p = np.zeros(1, N.PNP_PARAMS_DTYPE)
        p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"], p["th2"] = self._ransac
        p["fx"], p["fy"], p["cx"], p["cy"] = self.camera
        p["seed"] = self.seed
        return p

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        """PnPsolver::SetRansacParameters with the header's defaults (PnPsolver.h:63); the effective values are in self.plan"""
        self._ransac = (probability, minInliers, maxIterations, minSet, epsilon, th2)
        plan, p = N.PnpPlan(), self.params()
        st = self._ex._lib.hs_pnp_plan(len(self.corrs), p.ctypes.data_as(C.POINTER(N.PnpParams)), C.byref(plan))
        if st != N.HS_OK:
            raise HsError(st, "hs_pnp_plan: bad RANSAC parameters")
        self.plan = (plan.min_inliers, plan.epsilon, plan.max_iterations)

    @staticmethod
    def iterate_batch(solvers, nIterations):
        """iterate(nIterations) of every solver in ONE call (the candidates of a relocalisation): a list of iterate's tuples.  A pose that holds a NaN or an
        infinity (HS_PNP_NONFINITE) is handed out as no pose with bNoMore true, also where Refine() produced it; solver.result keeps the record."""
        res, inl, off = _ransac_iterate(solvers, nIterations, "hs_pnp_iterate", N.HS_PNP_MAX_SET, [s._ransac[3] for s in solvers], N.PNP_RESULT_DTYPE)
        out = []
        for q, s in enumerate(solvers):
            status = int(res["status"][q])
            no_more = status != N.HS_PNP_REFINED
            if status in (N.HS_PNP_REFINED, N.HS_PNP_BEST):
                flags = np.zeros(s.n_keypoints, bool)
                flags[s.corrs["kp"][inl[off[q]:off[q + 1]] != 0]] = True
                out.append((res["Tcw"][q].reshape(4, 4).copy(), no_more, flags, int(res["n_inliers"][q])))
            else:
                out.append((None, no_more, np.zeros(0, bool), 0))
        return out

    def iterate(self, nIterations):
        """cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): (Tcw float32 4x4 or None, bNoMore, vbInliers by
        KEYPOINT INDEX — empty without a pose, as the reference clears it —, nInliers).  The state persists across calls as the reference's does."""
        return PnPsolver.iterate_batch([self], nIterations)[0]

    def find(self):
        """cv::Mat find(vector<bool> &vbInliers, int &nInliers): iterate(mRansacMaxIts) without the flag"""
        Tcw, _, flags, n = self.iterate(self.plan[2])
        return Tcw, flags, n


class Sim3Solver:
    """HYSLAM::Sim3Solver (src/estimators/Sim3Solver.h) on flat arrays: Horn's closed form inside RANSAC for one loop candidate, computed by
    hs_sim3_iterate (include/hyslam_amd.h).  Built from ready correspondences (SIM3_CORR_DTYPE; `correspondences` gathers them as the
    reference's constructor does) and the two cameras (fx, fy, cx, cy).  n_matches is mN1, the length of vpMatched12 and of the returned vbInliers.
    `seed` replaces the process-wide generator the reference's solvers share; `draws` (uint32 [cap, HS_SIM3_DRAW_STRIDE]) directs the samples of the
    first cap iterations."""

    def __init__(self, camera1, camera2, corrs, n_matches=None, fix_scale=True, seed=0, draws=None, extractor=None):
        self._ex = extractor or ORBExtractor()
        self.corrs = np.ascontiguousarray(corrs, N.SIM3_CORR_DTYPE).reshape(-1)
        self.n_matches = int(n_matches) if n_matches is not None else (int(self.corrs["idx1"].max()) + 1 if len(self.corrs) else 0)
        self.camera1, self.camera2 = tuple(np.float32(c) for c in camera1[:4]), tuple(np.float32(c) for c in camera2[:4])
        self.fix_scale, self.seed = bool(fix_scale), int(seed)
        self.draws = None if draws is None else np.ascontiguousarray(draws, np.uint32).reshape(-1, N.HS_SIM3_DRAW_STRIDE)
        self.state = np.zeros(1, N.SIM3_STATE_DTYPE)
        self.best_mask = np.zeros(len(self.corrs), np.uint8)
        self.result = None
        self.SetRansacParameters()

    @staticmethod
    def correspondences(matched12, points1, pos1, pos2, bad1, bad2, index1, index2, kps1, kps2, Tcw1, Tcw2, size_ref=31.0, sigma_ref=1.0):
        """Sim3Solver.cc:66-107.  matched12[i1]: the landmark of key frame 2 matched to keypoint i1 of key frame 1, or < 0 (a null match); points1[i1]:
        key frame 1's own landmark at i1, or < 0; pos1 / pos2 [L, 3]: world positions; bad1 / bad2 [L]: isBad(); index1 / index2 [L]:
        GetIndexInKeyFrame in the landmark's own key frame (< 0: not seen); kps1 / kps2: KP_DTYPE; Tcw1 / Tcw2: 4x4 poses.  Walks i1 in ascending order
        and skips a null match, a null own point, a bad point on either side and a negative index on either side.  X = Rcw Xw + tcw is one product
        (double accumulation in index order, one narrowing: DESIGN.md D19)."""
        matched12, points1 = np.asarray(matched12, np.int64).reshape(-1), np.asarray(points1, np.int64).reshape(-1)
        i1 = np.nonzero((matched12 >= 0) & (points1 >= 0))[0]
        m1, m2 = points1[i1], matched12[i1]
        keep = ~(np.asarray(bad1, bool)[m1] | np.asarray(bad2, bool)[m2])
        i1, m1, m2 = i1[keep], m1[keep], m2[keep]
        k1, k2 = np.asarray(index1, np.int64)[m1], np.asarray(index2, np.int64)[m2]
        keep = (k1 >= 0) & (k2 >= 0)
        i1, m1, m2, k1, k2 = i1[keep], m1[keep], m2[keep], k1[keep], k2[keep]
        c = np.zeros(len(i1), N.SIM3_CORR_DTYPE)

        def to_camera(T, X):
            T, X = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64), np.asarray(X, np.float32).reshape(-1, 3).astype(np.float64)
            return np.stack([(((T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]) + T[i, 2] * X[:, 2]) + T[i, 3]).astype(np.float32) for i in range(3)], 1)

        def sigma2(kps, k):
            s = kps["size"][k].astype(np.float32) / np.float32(size_ref)
            return np.float32(sigma_ref) * (s * s)
        c["X1c"], c["X2c"] = to_camera(Tcw1, np.asarray(pos1, np.float32).reshape(-1, 3)[m1]), to_camera(Tcw2, np.asarray(pos2, np.float32).reshape(-1, 3)[m2])
        c["sigma2_1"], c["sigma2_2"], c["idx1"] = sigma2(kps1, k1), sigma2(kps2, k2), i1
        return c

    def params(self):
        p = np.zeros(1, N.SIM3_PARAMS_DTYPE)
        p["probability"], p["min_inliers"], p["max_iterations"] = self._ransac
        p["fix_scale"], p["seed"] = int(self.fix_scale), self.seed
        p["fx1"], p["fy1"], p["cx1"], p["cy1"] = self.camera1
        p["fx2"], p["fy2"], p["cx2"], p["cy2"] = self.camera2
        return p

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        """Sim3Solver::SetRansacParameters with the header's defaults (Sim3Solver.h:41); the effective mRansacMaxIts is self.max_iterations.  Resets
        mnIterations, as the reference does, and nothing else."""
        self._ransac = (probability, minInliers, maxIterations)
        plan, p = N.Sim3Plan(), self.params()
        st = self._ex._lib.hs_sim3_plan(len(self.corrs), p.ctypes.data_as(C.POINTER(N.Sim3Params)), C.byref(plan))
        if st != N.HS_OK:
            raise HsError(st, "hs_sim3_plan: bad RANSAC parameters")
        self.max_iterations, self.epsilon = plan.max_iterations, plan.epsilon
        self.state["iterations"] = 0

    @staticmethod
    def iterate_batch(solvers, nIterations):
        """iterate(nIterations) of every solver in ONE call (the consistent candidates of LoopClosing::ComputeSim3): a list of iterate's tuples"""
        res, inl, off = _ransac_iterate(solvers, nIterations, "hs_sim3_iterate", N.HS_SIM3_DRAW_STRIDE, [3] * len(solvers), N.SIM3_RESULT_DTYPE)
        out = []
        for q, s in enumerate(solvers):
            status = int(res["status"][q])
            flags = np.zeros(s.n_matches, bool)                    # vbInliers: always mN1 long (:147)
            flags[s.corrs["idx1"][inl[off[q]:off[q + 1]] != 0]] = True
            no_more = status in (N.HS_SIM3_TOO_FEW, N.HS_SIM3_EXHAUSTED)
            T12 = res["T12"][q].reshape(4, 4).copy() if status in (N.HS_SIM3_FOUND, N.HS_SIM3_NONFINITE) else None
            out.append((T12, no_more, flags, int(res["n_inliers"][q])))
        return out

    @staticmethod
    def find_batch(solvers):
        """find() of every solver in ONE call: every solver runs to its own mRansacMaxIts (the loop's AND stops each at its plan)"""
        return [(T12, flags, n) for T12, _, flags, n in Sim3Solver.iterate_batch(solvers, max(s.max_iterations for s in solvers))]

    def iterate(self, nIterations):
        """cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): (T12 float32 4x4 or None, bNoMore, vbInliers by
        index into vpMatched12, nInliers).  The state persists across calls as the reference's does."""
        return Sim3Solver.iterate_batch([self], nIterations)[0]

    def find(self):
        """cv::Mat find(vector<bool> &vbInliers12, int &nInliers): iterate(mRansacMaxIts) without the flag"""
        return Sim3Solver.find_batch([self])[0]

    def GetEstimatedRotation(self):
        return self.state["R"][0].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self.state["t"][0].copy()

    def GetEstimatedScale(self):
        return float(self.state["s"][0])


class MonoEstimator:
    """HYSLAM::MonoEstimator (src/initializers/MonoEstimator.h) on flat arrays: homography and fundamental RANSAC on shared 8-point sets, the choice
    between the two models and the reconstruction of the first pose and points, computed by hs_monoinit_estimate (include/hyslam_amd.h; DESIGN.md
    5.21).  Built from the reference frame's key points (KP_DTYPE, or [n, 2] pixel coordinates), the camera (fx, fy, cx, cy) and
    MonoEstimatorParams.  `seed` replaces SeedRandOnce(0) + RandomInt; `draws` (uint32 [cap, HS_MONOINIT_DRAW_STRIDE]) directs the samples of the
    first cap iterations.  The call keeps no state: every Initialize starts afresh, as the reference's does."""

    def __init__(self, kps1, camera, sigma=1.0, MaxIterations=200, minTriangulated=50, minFracTriangulated=0.9, minParallax=1.0, seed=0, draws=None, extractor=None):
        self._ex = extractor or ORBExtractor()
        self.kps1 = self.keypoints(kps1)
        self.camera = tuple(np.float32(c) for c in camera[:4])
        self.sigma, self.MaxIterations, self.minTriangulated = float(sigma), int(MaxIterations), int(minTriangulated)
        self.minFracTriangulated, self.minParallax, self.seed = float(minFracTriangulated), float(minParallax), int(seed)
        self.draws = None if draws is None else np.ascontiguousarray(draws, np.uint32).reshape(-1, N.HS_MONOINIT_DRAW_STRIDE)
        self.result = None

    @staticmethod
    def keypoints(kps):
        """KP_DTYPE records from KP_DTYPE records or from [n, 2] pixel coordinates (only x and y are read)"""
        if getattr(kps, "dtype", None) is not None and kps.dtype.names:
            return np.ascontiguousarray(kps, N.KP_DTYPE).reshape(-1)
        xy = np.asarray(kps, np.float32).reshape(-1, 2)
        out = np.zeros(len(xy), N.KP_DTYPE)
        out["x"], out["y"] = xy[:, 0], xy[:, 1]
        return out

    def params(self):
        p = np.zeros(1, N.MONOINIT_PARAMS_DTYPE)
        p["fx"], p["fy"], p["cx"], p["cy"] = self.camera
        p["sigma"], p["max_iterations"], p["min_triangulated"] = self.sigma, self.MaxIterations, self.minTriangulated
        p["min_frac_triangulated"], p["min_parallax_deg"], p["seed"] = self.minFracTriangulated, self.minParallax, self.seed
        return p

    @staticmethod
    def _draws(estimators):
        """the call's draws table [Q, cap, stride] or None; a table shorter than the call's is continued with the generator's own words"""
        cap = max([0] + [len(e.draws) for e in estimators if e.draws is not None])
        if not cap:
            return None, 0
        draws = np.zeros((len(estimators), cap, N.HS_MONOINIT_DRAW_STRIDE), np.uint32)
        for q, e in enumerate(estimators):
            draws[q] = _ransac_words(e.seed, cap, 8, N.HS_MONOINIT_DRAW_STRIDE)
            if e.draws is not None:
                draws[q, :len(e.draws)] = e.draws
        return draws, cap

    @staticmethod
    def parallax_deg(result):
        """the reference's parallax of the motion that decided, in degrees, from the cosine the library reports"""
        import math
        c = float(result["cos_parallax"])
        return math.degrees(math.acos(max(-1.0, min(1.0, c)))) if c == c else float("nan")

    @staticmethod
    def initialize_batch(estimators, kps2_list, matches12_list):
        """Initialize of Q estimators (one per monocular camera) in ONE call: a list of Initialize's tuples"""
        ex, Q = estimators[0]._ex, len(estimators)
        k2 = [MonoEstimator.keypoints(k) for k in kps2_list]
        m12 = [np.ascontiguousarray(m, np.int32).reshape(-1) for m in matches12_list]
        for e, m in zip(estimators, m12):
            if len(m) != len(e.kps1):
                raise ValueError("matches12 holds one entry per key point of the reference frame")
        off1, off2 = np.zeros(Q + 1, np.int64), np.zeros(Q + 1, np.int64)
        off1[1:], off2[1:] = np.cumsum([len(e.kps1) for e in estimators]), np.cumsum([len(k) for k in k2])
        kps1, kps2, matches = np.concatenate([e.kps1 for e in estimators]), np.concatenate(k2), np.concatenate(m12)
        par = np.concatenate([e.params() for e in estimators])
        draws, cap = MonoEstimator._draws(estimators)
        n1 = int(off1[Q])
        res = np.zeros(Q, N.MONOINIT_RESULT_DTYPE)
        inl_h, inl_f, p3d, tri = np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_monoinit_estimate(ex._h, Q, p(par), p(off1), p(kps1), p(off2), p(kps2), p(matches), p(draws) if cap else None, cap, p(res), p(inl_h),
                                                    p(inl_f), p(p3d), p(tri)))
        out = []
        for q, e in enumerate(estimators):
            sl = slice(off1[q], off1[q + 1])
            e.result, e.inliers_h, e.inliers_f = res[q].copy(), inl_h[sl].copy(), inl_f[sl].copy()
            ok = int(res["status"][q]) in (N.HS_MONOINIT_OK_H, N.HS_MONOINIT_OK_F)
            out.append((ok, res["R21"][q].reshape(3, 3).copy() if ok else None, res["t21"][q].copy() if ok else None, p3d[sl].copy(), tri[sl].astype(bool), e.result))
        return out

    def Initialize(self, kps2, matches12):
        """bool Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated): (ok, R21 3x3 or None, t21 or None, vP3D [n1, 3], vbTriangulated
        [n1], the result record).  A pose that holds a NaN or an infinity (HS_MONOINIT_NONFINITE) is handed out as a failure."""
        return MonoEstimator.initialize_batch([self], [kps2], [matches12])[0]

    @staticmethod
    def draws_table(estimators):
        """(uint32 [Q, cap, HS_MONOINIT_DRAW_STRIDE] or None, cap): the call's draws table, for a caller of initialize_batch_device to put on the device"""
        return MonoEstimator._draws(estimators)

    @staticmethod
    def work_bytes(estimators, n1_total):
        ex = estimators[0]._ex
        return int(ex._lib.hs_monoinit_work_bytes(len(estimators), int(n1_total), max(e.MaxIterations for e in estimators)))

    @staticmethod
    def initialize_batch_device(estimators, d_kps1, key_offsets1, d_kps2, key_offsets2, d_matches12, d_results, d_inliers_h, d_inliers_f, d_p3d, d_triangulated,
                                d_work, d_draws=None, draw_cap=0, stream=None):
        """the enqueue-only form (hs_monoinit_estimate_device) on memory of the extractor's device that the CALLER owns, inputs, outputs and work area
        alike: every d_* is a raw address or an object that names one through data_ptr() (a torch tensor) or .ptr.  d_kps1 / d_kps2 hold hs_keypoint
        records, d_matches12 int32 [n1_total]; the offsets are host sequences of Q + 1; d_results takes Q records of MONOINIT_RESULT_DTYPE, d_inliers_h /
        d_inliers_f / d_triangulated n1_total bytes, d_p3d n1_total x 3 floats, d_work work_bytes(estimators, n1_total) bytes.  d_draws / draw_cap: the
        table of draws_table(estimators) on the device, where one is wanted.  Enqueues on `stream` (None: the handle's own) and synchronises
        nothing: the caller orders its reads behind the call on that stream and keeps every buffer alive until then."""
        ex, Q = estimators[0]._ex, len(estimators)
        off1, off2 = np.ascontiguousarray(key_offsets1, np.int64), np.ascontiguousarray(key_offsets2, np.int64)
        par = np.concatenate([e.params() for e in estimators])

        def ptr(x):
            if x is None:
                return None
            return C.c_void_p(int(x.data_ptr() if hasattr(x, "data_ptr") else x.ptr if hasattr(x, "ptr") else x))
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_monoinit_estimate_device(ex._h, Q, p(par), p(off1), ptr(d_kps1), p(off2), ptr(d_kps2), ptr(d_matches12),
                                                           ptr(d_draws) if draw_cap else None, int(draw_cap), ptr(d_results), ptr(d_inliers_h), ptr(d_inliers_f),
                                                           ptr(d_p3d), ptr(d_triangulated), ptr(d_work), ptr(stream)))


class _DevBuf:
    """a block of device memory on the extractor's device for FrameTracker's numpy calls (hs_device_alloc / hs_device_copy / hs_device_free)"""

    def __init__(self, ex, nbytes, src=None):
        self._ex, self.ptr, self.nbytes = ex, 0, int(max(nbytes, 16))
        p = C.c_void_p()
        N.check(ex._h, ex._lib.hs_device_alloc(ex._h, self.nbytes, C.byref(p)))
        self.ptr = p.value
        if src is not None:
            self.write(src)

    def write(self, src):
        src = np.ascontiguousarray(src)
        if src.nbytes > self.nbytes:
            raise ValueError("the array is larger than the device block")
        N.check(self._ex._h, self._ex._lib.hs_device_copy(self._ex._h, self.ptr, src.ctypes.data, src.nbytes, 1, None))

    def read(self, dtype, count, offset=0):
        out = np.empty(count, dtype)
        N.check(self._ex._h, self._ex._lib.hs_device_copy(self._ex._h, out.ctypes.data, self.ptr + offset, out.nbytes, 2, None))
        return out

    def free(self):
        if self.ptr:
            ptr, self.ptr = self.ptr, 0
            N.check(self._ex._h, self._ex._lib.hs_device_free(self._ex._h, ptr))

    def __del__(self):
        try:
            if self._ex._h.value:                                # an extractor that was closed first took its device context along
                self.free()
        except Exception:                                        # interpreter shutdown: nothing left to report to
            pass


class FrameTracker:
    """TrackMotionModel::track and TrackLocalMap::track (src/slam/tracking/) on resident tables: every stage — pose matrices, projection searches,
    the association replay, the edge list, the pose optimisation, the outlier removal — is enqueued on one stream and nothing comes back to the host
    in between (include/hyslam_amd.h, "frame tracking on resident tables").  The numpy methods upload their inputs, run the device
    chain, synchronise once and return the frame's associations, both poses and the counts; the `*_device` methods are the raw pass-throughs.
    Landmarks and key frames are indices in ascending address order."""

    def __init__(self, extractor=None):
        self._ex = extractor or ORBExtractor()

    # ---- raw device addresses, asynchronous, nothing checked
    def track_work_bytes(self, n, n_last, L, cap):
        return int(self._ex._lib.hs_track_work_bytes(int(n), int(n_last), int(L), int(cap)))

    def pose_views_device(self, d_Tcw, d_out, stream=0):
        """hs_pose_views_device: d_Tcw float [16] row-major -> d_out _native.POSE_VIEW_DTYPE [1]"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_pose_views_device(ex._h, d_Tcw, d_out, stream or None))

    def search_by_projection_posed_device(self, frame, d_pose, d_lms, L, proj_params, d_match_idx, d_match_dist, d_n_matches, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_search_by_projection_posed_device(ex._h, C.byref(frame), d_pose, d_lms, L, C.byref(proj_params), d_match_idx, d_match_dist,
                                                                    d_n_matches, stream or None))

    def local_map_search_posed_device(self, table, d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, n_max_local_keyframes, n_neighbor_keyframes, frame, d_pose,
                                      d_lms, proj_params, cap, out, d_work, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_local_map_search_posed_device(ex._h, C.byref(table), d_frame_lm, n_assoc, d_neigh, neigh_cap, d_parent, n_max_local_keyframes,
                                                                n_neighbor_keyframes, C.byref(frame), d_pose, d_lms, C.byref(proj_params), cap, C.byref(out),
                                                                d_work, stream or None))

    def frame_associate_device(self, n, L, d_kp_lm, d_kp_outl, d_n_matches, n_ops, d_op_view, d_op_lm, d_work, stream=0):
        """hs_frame_associate_device: the ops (d_op_view[j], d_op_lm[j]) applied in ascending landmark index to the dense state"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_frame_associate_device(ex._h, n, L, d_kp_lm, d_kp_outl, d_n_matches, n_ops, d_op_view, d_op_lm, d_work, stream or None))

    def frame_views_device(self, n, d_kp_lm, d_kp_outl, d_n_matches, table, drop_bad, d_kp_lm_obs, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_frame_views_device(ex._h, n, d_kp_lm, d_kp_outl, d_n_matches, C.byref(table), int(bool(drop_bad)), d_kp_lm_obs, stream or None))

    def track_discard_device(self, mode, d_edges, d_n_edges, edge_cap, d_outlier, d_result, table, sensor, d_kp_lm, d_kp_outl, d_n_matches, d_counts, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_discard_device(ex._h, mode, d_edges, d_n_edges, edge_cap, d_outlier, d_result, C.byref(table), sensor, d_kp_lm, d_kp_outl,
                                                       d_n_matches, d_counts, stream or None))

    def track_motion_model_device(self, frame, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, table, d_lms, params, state, out, d_work, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_motion_model_device(ex._h, C.byref(frame), d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, C.byref(table), d_lms,
                                                            C.byref(params), C.byref(state), C.byref(out), d_work, stream or None))

    def track_local_map_device(self, frame, d_Tcw_in, table, d_lms, d_neigh, neigh_cap, d_parent, cap, params, state, out, d_work, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_local_map_device(ex._h, C.byref(frame), d_Tcw_in, C.byref(table), d_lms, d_neigh, neigh_cap, d_parent, cap,
                                                         C.byref(params), C.byref(state), C.byref(out), d_work, stream or None))

    def track_frame_device(self, frame, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, table, d_lms, d_neigh, neigh_cap, d_parent, cap, params, state, out, d_work,
                           stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_frame_device(ex._h, C.byref(frame), d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, C.byref(table), d_lms, d_neigh, neigh_cap,
                                                     d_parent, cap, C.byref(params), C.byref(state), C.byref(out), d_work, stream or None))

    def track_refkf_work_bytes(self, n, kf_cap, L):
        return int(self._ex._lib.hs_track_refkf_work_bytes(int(n), int(kf_cap), int(L)))

    def search_by_bow_kf_device(self, keyframes, d_kf_slot, table, d_kps, d_desc, d_node, d_weight, n, th_low, nnratio, d_match_kf, kf_cap, d_op_view, d_op_lm,
                                d_n_matches, d_work=None, stream=0):
        """hs_search_by_bow_kf_device: SearchByBoW(KeyFrame*, Frame&) between key frame *d_kf_slot of `keyframes` (_native.KfFeatures) and the frame;
        d_node / d_weight: hs_bow_transform_device's outputs for the frame (d_weight 0 / None: every keypoint with a non-negative node takes part)"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_search_by_bow_kf_device(ex._h, C.byref(keyframes), d_kf_slot, C.byref(table), d_kps, d_desc, d_node, d_weight or None, n, th_low, nnratio,
                                                          d_match_kf, kf_cap, d_op_view, d_op_lm, d_n_matches, d_work, stream or None))

    def frame_associate_views_device(self, n, L, d_kp_lm, d_kp_outl, d_n_matches, d_op_view, d_op_lm, d_work, stream=0):
        """hs_frame_associate_views_device: the ops (d_op_view[j], d_op_lm[j]), j < n, applied in ascending view index to the dense state"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_frame_associate_views_device(ex._h, n, L, d_kp_lm, d_kp_outl, d_n_matches, d_op_view, d_op_lm, d_work, stream or None))

    def track_initial_work_bytes(self, n, n_last, L, cap, kf_cap):
        return int(self._ex._lib.hs_track_initial_work_bytes(int(n), int(n_last), int(L), int(cap), int(kf_cap)))

    def track_reference_keyframe_device(self, frame, vocab, keyframes, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry, d_motion_result, table, d_lms, params, refkf_params,
                                        state, iout, d_work, stream=0):
        """hs_track_reference_keyframe_device: the fall-back of initialPoseEstimation with both gates on the device.  vocab: the hs_vocab_dev handle
        (distributed.DeviceVocabulary._v); d_motion_result 0 / None: the stage always runs; iout: _native.TrackInitialOut"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_reference_keyframe_device(ex._h, C.byref(frame), vocab, C.byref(keyframes), d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry,
                                                                  d_motion_result or None, C.byref(table), d_lms, C.byref(params), C.byref(refkf_params),
                                                                  C.byref(state), C.byref(iout), d_work, stream or None))

    def track_initial_device(self, frame, velocity_valid, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, vocab, keyframes, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry,
                             table, d_lms, params, refkf_params, state, out, iout, d_work, stream=0):
        """hs_track_initial_device: TrackingStateNormal::initialPoseEstimation; out (_native.TrackOut) may be None when the velocity is not valid"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_initial_device(ex._h, C.byref(frame), int(bool(velocity_valid)), d_Tcw_pred or None, d_last_kps or None, d_last_kp_lm or None,
                                                       n_last, vocab, C.byref(keyframes), d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry or None, C.byref(table), d_lms,
                                                       C.byref(params), C.byref(refkf_params), C.byref(state), C.byref(out) if out is not None else None,
                                                       C.byref(iout), d_work, stream or None))

    def track_normal_device(self, frame, velocity_valid, d_Tcw_pred, d_last_kps, d_last_kp_lm, n_last, vocab, keyframes, d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry,
                            table, d_lms, d_neigh, neigh_cap, d_parent, cap, params, refkf_params, state, out, iout, d_work, stream=0):
        """hs_track_normal_device: hs_track_initial_device, the local-map stage from iout.Tcw_init, and iout.frame_result for the key-frame stage"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_normal_device(ex._h, C.byref(frame), int(bool(velocity_valid)), d_Tcw_pred or None, d_last_kps or None, d_last_kp_lm or None,
                                                      n_last, vocab, C.byref(keyframes), d_kf_slot, kf_cap, d_Tcw_last, d_Tcw_entry or None, C.byref(table), d_lms,
                                                      d_neigh, neigh_cap, d_parent, cap, C.byref(params), C.byref(refkf_params), C.byref(state), C.byref(out),
                                                      C.byref(iout), d_work, stream or None))

    def keyframe_work_bytes(self, n, kf_cap, new_cap):
        return int(self._ex._lib.hs_keyframe_work_bytes(int(n), int(kf_cap), int(new_cap)))

    def keyframe_reference_device(self, n, state, table, d_ref_slot, d_result, d_work, stream=0):
        """hs_keyframe_reference_device (stage 1): bad landmarks dropped, the vote, *d_ref_slot updated when there is a winner"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_keyframe_reference_device(ex._h, n, C.byref(state), C.byref(table), d_ref_slot, d_result, d_work, stream or None))

    def keyframe_gate_device(self, d_track_result, params, d_result, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_keyframe_gate_device(ex._h, d_track_result or None, C.byref(params), d_result, stream or None))

    def keyframe_clean_device(self, n, state, table, d_result, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_keyframe_clean_device(ex._h, n, C.byref(state), C.byref(table), d_result, stream or None))

    def keyframe_need_device(self, n, sensor, d_depth, state, table, keyframes, d_ref_slot, d_track_result, params, d_result, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_keyframe_need_device(ex._h, n, sensor, d_depth, C.byref(state), C.byref(table), C.byref(keyframes), d_ref_slot,
                                                       d_track_result or None, C.byref(params), d_result, stream or None))

    def keyframe_create_device(self, frame, d_depth, d_Tcw, state, table, params, new_cap, out, d_work, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_keyframe_create_device(ex._h, C.byref(frame), d_depth, d_Tcw, C.byref(state), C.byref(table), C.byref(params), new_cap,
                                                         C.byref(out), d_work, stream or None))

    def keyframe_discard_device(self, n, state, d_result, stream=0):
        ex = self._ex
        N.check(ex._h, ex._lib.hs_keyframe_discard_device(ex._h, n, C.byref(state), d_result, stream or None))

    def track_keyframe_device(self, frame, d_depth, d_Tcw, table, keyframes, d_track_result, params, state, d_ref_slot, new_cap, out, d_work, stream=0):
        """hs_track_keyframe_device: the six stages after hs_track_frame_device, enqueued in order; out: _native.KeyFrameOut"""
        ex = self._ex
        N.check(ex._h, ex._lib.hs_track_keyframe_device(ex._h, C.byref(frame), d_depth, d_Tcw, C.byref(table), C.byref(keyframes), d_track_result or None,
                                                        C.byref(params), C.byref(state), d_ref_slot, new_cap, C.byref(out), d_work, stream or None))

    # ---- numpy in, numpy out
    def device_keyframes(self, keyframes):
        """keyframes: a dict of n_kf, kf_off int64 [n_kf + 1], kps (KP_DTYPE), desc (total, 32) uint8, node int32 [total] (negative: in no feature-vector
        node), kp_lm int32 [total], optionally weight float32 [total] (the transform's word weights: not positive = in no node) -> (_native.KfFeatures of
        device pointers, the buffers)"""
        arrs = (np.ascontiguousarray(keyframes["kf_off"], np.int64), np.ascontiguousarray(keyframes["kps"], N.KP_DTYPE),
                np.ascontiguousarray(keyframes["desc"], np.uint8), np.ascontiguousarray(keyframes["node"], np.int32), np.ascontiguousarray(keyframes["kp_lm"], np.int32))
        if len(arrs[0]) != int(keyframes["n_kf"]) + 1 or any(len(a) != len(arrs[1]) for a in arrs[2:]) or (len(arrs[1]) and int(arrs[0][-1]) > len(arrs[1])):
            raise ValueError("kf_off has n_kf + 1 entries and every keypoint array one entry per keypoint")
        if keyframes.get("weight") is not None:
            arrs += (np.ascontiguousarray(keyframes["weight"], np.float32),)
            if len(arrs[-1]) != len(arrs[1]):
                raise ValueError("one weight per keypoint")
        bufs = [_DevBuf(self._ex, a.nbytes, a) for a in arrs]
        return N.KfFeatures(int(keyframes["n_kf"]), *[b.ptr for b in bufs], *([None] if len(arrs) == 5 else [])), bufs

    def SearchByBoWKeyFrame(self, keyframes, kf_slot, table, kps, desc, node, th_low=50.0, nnratio=0.7, kf_cap=None, weight=None):
        """FeatureMatcher::SearchByBoW(KeyFrame*, Frame&, map&) on the device (hs_search_by_bow_kf_device).  keyframes: see device_keyframes, kf_slot
        the key frame in it; table: see FeatureMatcher._kf_table (L and lm_bad are read); kps (KP_DTYPE), desc (n, 32) uint8 and node int32 [n]: the
        frame as the vocabulary transform left it, with `weight` float32 [n] its word weights (a keypoint whose weight is not positive is in no node;
        without `weight`, mark such a keypoint with a negative node).  Returns (matches {frame view: landmark}, match_kf int32 [kf_cap]: the
        view each key-frame keypoint took or -1, nmatches = matches_internal.size())."""
        ex = self._ex
        KF, kkeep = self.device_keyframes(keyframes)
        KT, tkeep = self.device_table(table)
        arrs = np.ascontiguousarray(kps, N.KP_DTYPE), np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(node, np.int32)
        n = len(arrs[0])
        if len(arrs[1]) != n or len(arrs[2]) != n:
            raise ValueError("one descriptor and one node per keypoint")
        off = np.asarray(keyframes["kf_off"], np.int64)
        kf_cap = int(kf_cap or max(1, int(np.diff(off).max()) if len(off) > 1 else 1))
        ins = [_DevBuf(ex, a.nbytes, a) for a in arrs] + [_DevBuf(ex, 4, np.array([kf_slot], np.int32))]
        d_w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, np.float32)
            if len(w) != n:
                raise ValueError("one weight per keypoint")
            d_w = _DevBuf(ex, w.nbytes, w)
        outs = _DevBuf(ex, kf_cap * 4), _DevBuf(ex, n * 4), _DevBuf(ex, n * 4), _DevBuf(ex, 4)
        self.search_by_bow_kf_device(KF, ins[3].ptr, KT, ins[0].ptr, ins[1].ptr, ins[2].ptr, d_w.ptr if d_w else None, n, th_low, nnratio, outs[0].ptr, kf_cap, outs[1].ptr, outs[2].ptr,
                                     outs[3].ptr)
        ex.synchronize()
        match_kf, op_view, op_lm = outs[0].read(np.int32, kf_cap), outs[1].read(np.int32, n), outs[2].read(np.int32, n)
        del kkeep, tkeep
        return {int(f): int(op_lm[f]) for f in np.nonzero(op_view >= 0)[0]}, match_kf, int(outs[3].read(np.int32, 1)[0])

    def AssociateLandMarks(self, kp_lm, kp_outl, n_matches, associations, L):
        """Frame::associateLandMarks(associations, true) on the dense state (hs_frame_associate_views_device).  associations: {view: landmark}, a
        landmark at most once.  Returns (kp_lm, kp_outl, n_matches) afterwards."""
        ex = self._ex
        st = np.ascontiguousarray(kp_lm, np.int32), np.ascontiguousarray(kp_outl, np.uint8), np.array([n_matches], np.int32)
        n = len(st[0])
        if len(set(associations.values())) != len(associations) or len(associations) > n:
            raise ValueError("a landmark occurs in at most one association, and there is at most one per view")
        op_view, op_lm = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        for j, (v, m) in enumerate(sorted(associations.items())):
            op_view[j], op_lm[j] = v, m
        bufs = [_DevBuf(ex, a.nbytes, a) for a in st + (op_view, op_lm)]
        work = _DevBuf(ex, self.track_refkf_work_bytes(n, 0, L))
        self.frame_associate_views_device(n, int(L), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, work.ptr)
        ex.synchronize()
        return bufs[0].read(np.int32, n), bufs[1].read(np.uint8, n), int(bufs[2].read(np.int32, 1)[0])

    def device_frame(self, frame):
        """frame: a dict of fx, fy, cx, cy, mbf, sensor, bounds (min_x, max_x, min_y, max_y), kps (KP_DTYPE), desc (n, 32) uint8, uR float32 [n]
        (optional size_ref, 31) -> (_native.FrameView of device pointers, the buffers).  The pose fields stay zero: the chain reads poses from HBM."""
        kps, desc = np.ascontiguousarray(frame["kps"], N.KP_DTYPE), np.ascontiguousarray(frame["desc"], np.uint8)
        uR = np.ascontiguousarray(frame["uR"], np.float32) if frame.get("uR") is not None else np.full(len(kps), -1, np.float32)
        F = N.FrameView()
        F.fx, F.fy, F.cx, F.cy, F.mbf, F.sensor = frame["fx"], frame["fy"], frame["cx"], frame["cy"], frame["mbf"], int(frame["sensor"])
        F.min_x, F.max_x, F.min_y, F.max_y = frame["bounds"]
        F.size_ref, F.n = frame.get("size_ref", 31.0), len(kps)
        bufs = [_DevBuf(self._ex, a.nbytes, a) for a in (kps, desc, uR)]
        F.kps, F.desc, F.uR = (b.ptr for b in bufs)
        return F, bufs

    def device_table(self, table):
        """`table`: see FeatureMatcher._kf_table -> (_native.KfTable of device pointers, the buffers)"""
        KT, keep = FeatureMatcher._kf_table(table)
        bufs = [_DevBuf(self._ex, a.nbytes, a) for a in keep]
        return N.KfTable(KT.L, KT.n_kf, *[b.ptr for b in bufs]), bufs

    def outputs(self, sizes):
        """device buffers for every field of _native.TrackOut; sizes: n, n_last, n_kf, cap -> (TrackOut, {field: (buffer, dtype, count)})"""
        bufs = {}

        def alloc(spec, prefix=""):
            ptrs = []
            for k, kind, cnt in spec:
                dt, cnt = N.track_out_dtype(kind), sizes.get(cnt, cnt)
                bufs[prefix + k] = (_DevBuf(self._ex, dt.itemsize * cnt), dt, cnt)
                ptrs.append(bufs[prefix + k][0].ptr)
            return ptrs
        head, local, tail = alloc(N.TRACK_OUT_HEAD), alloc(N.LOCAL_MAP_OUT_SPEC, "local."), alloc(N.TRACK_OUT_TAIL)
        return N.TrackOut(*head, N.LocalMapOut(*local), *tail), bufs

    def _run(self, which, frame, Tcw, table, landmarks, last_kps=None, last_kp_lm=None, neigh=None, parent=None, cap=None, params=None, state=None):
        ex = self._ex
        F, fkeep = self.device_frame(frame)
        KT, tkeep = self.device_table(table)
        lms = np.ascontiguousarray(landmarks, N.LM_DTYPE)
        if len(lms) != KT.L:
            raise ValueError("one hs_landmark record per landmark of the table")
        n, n_last = F.n, (len(last_kp_lm) if last_kp_lm is not None else 1)
        cap = int(cap or KT.L)
        prm = params or N.TrackParams()
        if state is None:
            state = (np.full(n, -1, np.int32), np.zeros(n, np.uint8), 0)
        st_in = (np.ascontiguousarray(state[0], np.int32), np.ascontiguousarray(state[1], np.uint8), np.array([state[2]], np.int32), np.full(n, -1, np.int32))
        if len(st_in[0]) != n or len(st_in[1]) != n:
            raise ValueError("the state has one entry per keypoint")
        st_bufs = [_DevBuf(ex, a.nbytes, a) for a in st_in]
        ST = N.TrackState(*[b.ptr for b in st_bufs])
        out, obufs = self.outputs(dict(n=n, n_last=n_last, n_kf=KT.n_kf, cap=cap))
        d_T, d_lms = _DevBuf(ex, 64, np.ascontiguousarray(Tcw, np.float32).reshape(16)), _DevBuf(ex, lms.nbytes, lms)
        work = _DevBuf(ex, self.track_work_bytes(n, n_last, KT.L, cap))
        keep = [fkeep, tkeep]
        if which != "local":
            lk, ll = np.ascontiguousarray(last_kps, N.KP_DTYPE), np.ascontiguousarray(last_kp_lm, np.int32)
            if len(lk) != len(ll) or len(ll) < 1:
                raise ValueError("last_kps and last_kp_lm have one entry per keypoint of the last frame")
            d_lk, d_ll = _DevBuf(ex, lk.nbytes, lk), _DevBuf(ex, ll.nbytes, ll)
        if which != "motion":
            ng, pa = np.ascontiguousarray(neigh, np.int32).reshape(KT.n_kf, -1), np.ascontiguousarray(parent, np.int32)
            d_ng, d_pa = _DevBuf(ex, ng.nbytes, ng), _DevBuf(ex, pa.nbytes, pa)
        if which == "motion":
            self.track_motion_model_device(F, d_T.ptr, d_lk.ptr, d_ll.ptr, n_last, KT, d_lms.ptr, prm, ST, out, work.ptr)
        elif which == "local":
            self.track_local_map_device(F, d_T.ptr, KT, d_lms.ptr, d_ng.ptr, ng.shape[1], d_pa.ptr, cap, prm, ST, out, work.ptr)
        else:
            self.track_frame_device(F, d_T.ptr, d_lk.ptr, d_ll.ptr, n_last, KT, d_lms.ptr, d_ng.ptr, ng.shape[1], d_pa.ptr, cap, prm, ST, out, work.ptr)
        ex.synchronize()
        raw = {k: b.read(dt, cnt) for k, (b, dt, cnt) in obufs.items()}
        res = dict(kp_lm=st_bufs[0].read(np.int32, n), kp_outl=st_bufs[1].read(np.uint8, n), n_matches=int(st_bufs[2].read(np.int32, 1)[0]),
                   kp_lm_obs=st_bufs[3].read(np.int32, n), raw=raw)
        del keep
        return res

    @staticmethod
    def _summary(res, motion, local):
        raw, r = res["raw"], res["raw"]["result"][0]
        if motion:
            res.update(pose_motion=raw["pose_motion"][0], status=int(r["status"]), used_wide=bool(r["used_wide"]), n_narrow=int(r["n_narrow"]),
                       n_wide=int(r["n_wide"]), n_matches_map=int(r["n_matches_map"]))
        if local:
            res.update(pose_local=raw["pose_local"][0], n_inliers=int(r["n_inliers"]))
        return res

    def TrackMotionModel(self, frame, Tcw_pred, last_kps, last_kp_lm, table, landmarks, params=None):
        """TrackMotionModel::track from SetPose(Tcw_pred) on.  frame: see device_frame; last_kps (KP_DTYPE; the angle is read) and last_kp_lm int32: the
        last frame's keypoints and the landmark each holds (-1 = none); table: see FeatureMatcher._kf_table (lm_nobs is read); landmarks: LM_DTYPE
        [L]; params: _native.TrackParams (the radii already truncated as the reference's `int th`).  Returns a dict: kp_lm, kp_outl (0 none / 1 inlier
        / 2 outlier), n_matches, pose_motion (POSE_RESULT_DTYPE record), status (_native.HS_TRACK_*), used_wide, n_narrow, n_wide, n_matches_map, and
        `raw`: every device output of the call by field name."""
        return self._summary(self._run("motion", frame, Tcw_pred, table, landmarks, last_kps, last_kp_lm, params=params), True, False)

    def TrackLocalMap(self, frame, Tcw_in, table, landmarks, neigh, parent, kp_lm, kp_outl, n_matches, params=None, cap=None):
        """TrackLocalMap::track from the pose Tcw_in and the associations (kp_lm, kp_outl, n_matches).  neigh (n_kf, neigh_cap) / parent [n_kf]: as
        FeatureMatcher.LocalKeyFrames; cap: the local map's capacity (default: every landmark).  Returns kp_lm, kp_outl, n_matches, pose_local,
        n_inliers and `raw`."""
        return self._summary(self._run("local", frame, Tcw_in, table, landmarks, neigh=neigh, parent=parent, cap=cap, params=params,
                                       state=(kp_lm, kp_outl, n_matches)), False, True)

    def TrackFrame(self, frame, Tcw_pred, last_kps, last_kp_lm, table, landmarks, neigh, parent, params=None, cap=None):
        """the two, one after the other on the device (hs_track_frame_device): the local map starts from the motion model's pose whatever its status;
        the caller reads `status` and decides what TrackingStateNormal decides.  Returns the union of the two calls' results."""
        return self._summary(self._run("frame", frame, Tcw_pred, table, landmarks, last_kps, last_kp_lm, neigh, parent, cap, params), True, True)

    def initial_outputs(self, n, kf_cap, alloc=None):
        """device buffers for every field of _native.TrackInitialOut -> (TrackInitialOut, {field: (buffer, dtype, count)})"""
        sizes, bufs = dict(n=n, kf_cap=kf_cap), {}
        alloc = alloc or (lambda nbytes: _DevBuf(self._ex, nbytes))
        for k, kind, cnt in N.TRACK_INITIAL_OUT_SPEC:
            dt, cnt = N.track_out_dtype(kind), sizes.get(cnt, cnt)
            bufs[k] = (alloc(dt.itemsize * cnt), dt, cnt)
        return N.TrackInitialOut(*[bufs[k][0].ptr for k, _, _ in N.TRACK_INITIAL_OUT_SPEC]), bufs

    def _run_initial(self, local, frame, vocab, keyframes, kf_slot, Tcw_last, table, landmarks, velocity_valid, Tcw_pred, last_kps, last_kp_lm, Tcw_entry, state,
                     neigh, parent, cap, params, refkf_params, kf_cap):
        ex = self._ex
        F, fkeep = self.device_frame(frame)
        KT, tkeep = self.device_table(table)
        KF, kkeep = self.device_keyframes(keyframes)
        lms = np.ascontiguousarray(landmarks, N.LM_DTYPE)
        if len(lms) != KT.L:
            raise ValueError("one hs_landmark record per landmark of the table")
        n = F.n
        off = np.asarray(keyframes["kf_off"], np.int64)
        kf_cap = int(kf_cap or max(1, int(np.diff(off).max()) if len(off) > 1 else 1))
        cap = int(cap or KT.L)
        prm, rprm = params or N.TrackParams(), refkf_params or N.TrackRefkfParams()
        if state is None:
            state = (np.full(n, -1, np.int32), np.zeros(n, np.uint8), 0)
        st_in = (np.ascontiguousarray(state[0], np.int32), np.ascontiguousarray(state[1], np.uint8), np.array([state[2]], np.int32), np.full(n, -1, np.int32))
        if len(st_in[0]) != n or len(st_in[1]) != n:
            raise ValueError("the state has one entry per keypoint")
        st_bufs = [_DevBuf(ex, a.nbytes, a) for a in st_in]
        ST = N.TrackState(*[b.ptr for b in st_bufs])
        pose = lambda T: _DevBuf(ex, 64, np.ascontiguousarray(T, np.float32).reshape(16))
        d_last, d_lms, d_slot = pose(Tcw_last), _DevBuf(ex, lms.nbytes, lms), _DevBuf(ex, 4, np.array([kf_slot], np.int32))
        d_pred = d_entry = d_lk = d_ll = None
        n_last = 1
        if velocity_valid:
            lk, ll = np.ascontiguousarray(last_kps, N.KP_DTYPE), np.ascontiguousarray(last_kp_lm, np.int32)
            if len(lk) != len(ll) or len(ll) < 1:
                raise ValueError("last_kps and last_kp_lm have one entry per keypoint of the last frame")
            d_pred, d_lk, d_ll, n_last = pose(Tcw_pred), _DevBuf(ex, lk.nbytes, lk), _DevBuf(ex, ll.nbytes, ll), len(ll)
        else:
            d_entry = pose(Tcw_entry)
        out, obufs = self.outputs(dict(n=n, n_last=n_last, n_kf=KT.n_kf, cap=cap))
        iout, ibufs = self.initial_outputs(n, kf_cap)
        work = _DevBuf(ex, self.track_initial_work_bytes(n, n_last, KT.L, cap, kf_cap))
        ptr = lambda b: b.ptr if b is not None else None
        head = (F, velocity_valid, ptr(d_pred), ptr(d_lk), ptr(d_ll), n_last, vocab._v, KF, d_slot.ptr, kf_cap, d_last.ptr, ptr(d_entry), KT, d_lms.ptr)
        if local:
            ng, pa = np.ascontiguousarray(neigh, np.int32).reshape(KT.n_kf, -1), np.ascontiguousarray(parent, np.int32)
            d_ng, d_pa = _DevBuf(ex, ng.nbytes, ng), _DevBuf(ex, pa.nbytes, pa)
            self.track_normal_device(*head, d_ng.ptr, ng.shape[1], d_pa.ptr, cap, prm, rprm, ST, out, iout, work.ptr)
        else:
            self.track_initial_device(*head, prm, rprm, ST, out, iout, work.ptr)
        ex.synchronize()
        raw = {k: b.read(dt, cnt) for k, (b, dt, cnt) in obufs.items()}
        raw.update({"initial." + k: b.read(dt, cnt) for k, (b, dt, cnt) in ibufs.items()})
        r = raw["initial.result"][0]
        res = dict(kp_lm=st_bufs[0].read(np.int32, n), kp_outl=st_bufs[1].read(np.uint8, n), n_matches=int(st_bufs[2].read(np.int32, 1)[0]),
                   kp_lm_obs=st_bufs[3].read(np.int32, n), raw=raw, Tcw_init=raw["initial.Tcw_init"].reshape(4, 4).copy(), pose_refkf=raw["initial.pose"][0])
        res.update({k: int(r[k]) for k in N.TRACK_INITIAL_RESULT_DTYPE.names if k != "_pad"})
        if velocity_valid:
            m = raw["result"][0]
            res.update(pose_motion=raw["pose_motion"][0], status=int(m["status"]), used_wide=bool(m["used_wide"]), n_narrow=int(m["n_narrow"]), n_wide=int(m["n_wide"]),
                       n_matches_map=int(m["n_matches_map"]))
        if local:
            res.update(pose_local=raw["pose_local"][0], n_inliers=int(raw["result"][0]["n_inliers"]), frame_result=raw["initial.frame_result"][0])
        del fkeep, tkeep, kkeep
        return res

    def InitialPoseEstimation(self, frame, vocab, keyframes, kf_slot, Tcw_last, table, landmarks, velocity_valid, Tcw_pred=None, last_kps=None, last_kp_lm=None,
                              Tcw_entry=None, state=None, params=None, refkf_params=None, kf_cap=None):
        """TrackingStateNormal::initialPoseEstimation on the device (hs_track_initial_device): the motion model when `velocity_valid` (Tcw_pred, last_kps,
        last_kp_lm as TrackMotionModel), then TrackReferenceKeyFrame::track when the motion model found fewer than thresh_init matches, both decisions
        taken on the device.  vocab: a distributed.DeviceVocabulary; keyframes: see device_keyframes, kf_slot the reference key frame in it; Tcw_last: the
        last frame's pose; without a valid velocity the fall-back always runs, on `state` (kp_lm, kp_outl, n_matches; default: empty) and with Tcw_entry
        the pose the frame holds.  params: _native.TrackParams, refkf_params: _native.TrackRefkfParams.  Returns a dict: kp_lm, kp_outl, n_matches, the
        fields of hs_track_initial_result (refkf_status, n_bow, n_matches_map_refkf, n_init, success), Tcw_init (4, 4), pose_refkf, with a valid velocity
        the motion model's fields as TrackMotionModel returns them, and `raw`: every device output by field name (the initial stage's as "initial.<field>")."""
        return self._run_initial(False, frame, vocab, keyframes, kf_slot, Tcw_last, table, landmarks, velocity_valid, Tcw_pred, last_kps, last_kp_lm, Tcw_entry, state,
                                 None, None, None, params, refkf_params, kf_cap)

    def TrackNormal(self, frame, vocab, keyframes, kf_slot, Tcw_last, table, landmarks, neigh, parent, velocity_valid, Tcw_pred=None, last_kps=None, last_kp_lm=None,
                    Tcw_entry=None, state=None, params=None, refkf_params=None, kf_cap=None, cap=None):
        """InitialPoseEstimation, then TrackLocalMap::track from Tcw_init (hs_track_normal_device); the local map runs whatever `success` says, and the
        caller decides.  Adds pose_local, n_inliers and frame_result: the hs_track_result record KeyFrameDecision takes as track_result."""
        return self._run_initial(True, frame, vocab, keyframes, kf_slot, Tcw_last, table, landmarks, velocity_valid, Tcw_pred, last_kps, last_kp_lm, Tcw_entry, state,
                                 neigh, parent, cap, params, refkf_params, kf_cap)

    def keyframe_outputs(self, new_cap, alloc=None):
        """device buffers for every field of _native.KeyFrameOut -> (KeyFrameOut with lms = NULL, {field: (buffer, dtype, count)})"""
        sizes = dict(new_cap=new_cap, new_cap1=new_cap + 1, new_cap3=3 * new_cap, new_cap32=32 * new_cap)
        alloc = alloc or (lambda nbytes: _DevBuf(self._ex, nbytes))
        bufs = {}
        for k, kind, cnt in N.KEYFRAME_OUT_SPEC:
            dt, cnt = N.track_out_dtype(kind), sizes.get(cnt, cnt)
            bufs[k] = (alloc(dt.itemsize * cnt), dt, cnt)
        return N.KeyFrameOut(*[bufs[k][0].ptr for k, _, _ in N.KEYFRAME_OUT_SPEC], None, 0), bufs

    def KeyFrameDecision(self, frame, depth, Tcw, table, keyframes, kp_lm, kp_outl, n_matches, ref_slot, track_result=None, params=None, new_cap=None):
        """What Tracking::_Track_ does after the two track functions, on the device (hs_track_keyframe_device): the reference key-frame vote, bOK,
        HandlePostTrackingSuccess, needNewKeyFrame, createNewKeyFrame's stereo landmarks and the final outlier removal.  frame: see device_frame; depth
        float32 [n]; Tcw: the final pose; table: see FeatureMatcher._kf_table; keyframes: see device_keyframes (only n_kf, kf_off and kp_lm are read:
        the other arrays may be left out); (kp_lm, kp_outl, n_matches): the frame's associations; ref_slot: the current reference key frame's slot or
        -1; track_result: a dict of status, n_matches_map, n_inliers (TrackFrame's result has them) or None with params.ok_override set; params:
        _native.KeyFrameParams; new_cap: room for creation records (default n).  Returns a dict: the fields of hs_keyframe_result, kp_lm, kp_outl,
        n_matches, kp_lm_obs, pose_view, and for the min(n_new, new_cap) created points new_view, new_pos, entries, obs, desc, lm_index and the
        offsets — the arrays FeatureMatcher.UpdateLandmarkEntries / hs_landmark_update_entries_device take."""
        ex = self._ex
        prm = params or N.KeyFrameParams()
        F, fkeep = self.device_frame(frame)
        KT, tkeep = self.device_table(table)
        n = F.n
        new_cap = n if new_cap is None else int(new_cap)
        kf = dict(keyframes)
        total = len(np.asarray(kf["kp_lm"]))
        for k, filler in (("kps", np.zeros(total, N.KP_DTYPE)), ("desc", np.zeros((total, 32), np.uint8)), ("node", np.full(total, -1, np.int32))):
            kf.setdefault(k, filler)
        KF, kkeep = self.device_keyframes(kf)
        st_in = (np.ascontiguousarray(kp_lm, np.int32), np.ascontiguousarray(kp_outl, np.uint8), np.array([n_matches], np.int32), np.full(n, -1, np.int32))
        d_depth = np.ascontiguousarray(depth, np.float32)
        if len(st_in[0]) != n or len(st_in[1]) != n or len(d_depth) != n:
            raise ValueError("the state and the depths have one entry per keypoint")
        st_bufs = [_DevBuf(ex, a.nbytes, a) for a in st_in]
        ST = N.TrackState(*[b.ptr for b in st_bufs])
        d_depth, d_T = _DevBuf(ex, d_depth.nbytes, d_depth), _DevBuf(ex, 64, np.ascontiguousarray(Tcw, np.float32).reshape(16))
        d_ref = _DevBuf(ex, 4, np.array([ref_slot], np.int32))
        d_tr = None
        if track_result is not None:
            tr = np.zeros(1, N.TRACK_RESULT_DTYPE)
            for k in ("status", "n_matches_map", "n_inliers"):
                tr[k] = int(track_result[k])
            d_tr = _DevBuf(ex, tr.nbytes, tr)
        elif prm.ok_override < 0:
            raise ValueError("without a track result the gate needs params.ok_override")
        out, obufs = self.keyframe_outputs(new_cap)
        work = _DevBuf(ex, self.keyframe_work_bytes(n, KT.n_kf, new_cap))
        self.track_keyframe_device(F, d_depth.ptr, d_T.ptr, KT, KF, d_tr.ptr if d_tr else None, prm, ST, d_ref.ptr, new_cap, out, work.ptr)
        ex.synchronize()
        r = obufs["result"][0].read(N.KEYFRAME_RESULT_DTYPE, 1)[0]
        res = {k: int(r[k]) for k in N.KEYFRAME_RESULT_DTYPE.names if k != "_pad"}
        m = min(res["n_new"], new_cap)
        res.update(kp_lm=st_bufs[0].read(np.int32, n), kp_outl=st_bufs[1].read(np.uint8, n), n_matches=int(st_bufs[2].read(np.int32, 1)[0]),
                   kp_lm_obs=st_bufs[3].read(np.int32, n), pose_view=obufs["pose_view"][0].read(N.POSE_VIEW_DTYPE, 1)[0])
        for k in ("new_view", "entries", "obs"):
            res[k] = obufs[k][0].read(obufs[k][1], new_cap)[:m]
        res["new_pos"] = obufs["new_pos"][0].read(np.float32, 3 * new_cap).reshape(-1, 3)[:m]
        res["desc"] = obufs["desc"][0].read(np.uint8, 32 * new_cap).reshape(-1, 32)[:m]
        res["lm_index"] = obufs["lm_index"][0].read(np.int32, new_cap)
        res["offsets"] = obufs["obs_offsets"][0].read(np.int64, new_cap + 1)
        del fkeep, tkeep, kkeep
        return res


class ORBVocabulary:
    """HYSLAM::ORBVocabulary::transform (src/features/low_level/ORBVocabulary.cpp:31-42) over a flat vocabulary tree
    (_native.VocabTree; DBoW2 and ORBvoc are external to the reference).  `transform` returns the two containers Frame::ComputeBoW fills:
    the BoW vector {word id: L1-normalised tf-idf weight} and the feature vector as CSR (node ids ascending, node_ptr, indices ascending)."""

    def __init__(self, tree, extractor=None):
        """tree: a _native.VocabTree, or the path of a DBoW2 vocabulary file (".txt" = text format, else binary; ORBVocabulary.cpp:14-29)"""
        self._vocab = None
        if isinstance(tree, (str, bytes)):
            L = N.lib()
            v = C.c_void_p()
            st = L.hs_vocab_load(tree.encode() if isinstance(tree, str) else tree, C.byref(v))
            if st != N.HS_OK:
                raise HsError(st, "Wrong path to vocabulary. Failed to open at: %s" % tree)       # the reference prints this and exits (ORBVocabulary.cpp:22-27)
            self._vocab = v
            tree = N.VocabTree()
            L.hs_vocab_get_tree(v, C.byref(tree))
        self.tree = tree
        self._ex = extractor or ORBExtractor()

    def size(self):
        """ORBVocabulary::size(): number of words"""
        if self._vocab is not None:
            n = C.c_int32()
            N.lib().hs_vocab_info(self._vocab, None, None, None, C.byref(n), None, None)
            return n.value
        cc = np.ctypeslib.as_array(C.cast(self.tree.child_count, C.POINTER(C.c_int32)), shape=(self.tree.n_nodes,))
        return int((cc[1:] == 0).sum())

    def __del__(self):
        try:
            if self._vocab is not None:
                N.lib().hs_vocab_destroy(self._vocab)
                self._vocab = None
        except Exception:
            pass

    def transform(self, descriptors, levelsup=4):
        ex = self._ex
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        w = np.zeros(n, np.int32); wt = np.zeros(n, np.float32); nd = np.zeros(n, np.int32)
        N.check(ex._h, ex._lib.hs_bow_transform(ex._h, C.byref(self.tree), d.ctypes.data_as(C.c_void_p), n, levelsup,
                                                w.ctypes.data_as(C.c_void_p), wt.ctypes.data_as(C.c_void_p), nd.ctypes.data_as(C.c_void_p)))
        return self.containers(w, wt, nd)

    @staticmethod
    def containers(word, weight, node):
        """DBoW2: `if (w > 0) { bow.addWeight(id, w); fv.addFeature(nid, i); }`, then L1 normalisation of the BoW vector."""
        use = weight > 0
        bow = {}
        for wid, wv in zip(word[use].tolist(), weight[use].tolist()):
            bow[wid] = bow.get(wid, 0.0) + wv
        tot = sum(abs(v) for _, v in sorted(bow.items()))
        if tot > 0:
            bow = {k: v / tot for k, v in bow.items()}
        idx = np.nonzero(use)[0]
        order = np.lexsort((idx, node[idx]))
        ids, counts = np.unique(node[idx], return_counts=True)
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        return bow, (ids.astype(np.int32), ptr, idx[order].astype(np.int32)), (word, weight, node)

    def bow_vector(self, word, weight):
        """The BoW vector of `containers`, built on the device (hs_bow_vector) from a transform's per-feature (word, weight): (words int32 [m]
        ascending and unique, values float64 [m], L1-normalised) — what DBoW2's transform leaves in Frame::mBowVec (Frame.cc:472-479)."""
        ex = self._ex
        w = np.ascontiguousarray(word, np.int32).reshape(-1)
        wt = np.ascontiguousarray(weight, np.float32).reshape(-1)
        if len(w) != len(wt):
            raise ValueError("word and weight must have one entry per feature")
        ow, ov, m = np.zeros(len(w), np.int32), np.zeros(len(w), np.float64), C.c_int32()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        N.check(ex._h, ex._lib.hs_bow_vector(ex._h, p(w), p(wt), len(w), p(ow), p(ov), C.byref(m)))
        return ow[:m.value].copy(), ov[:m.value].copy()

    def score(self, a, b):
        """FeatureVocabulary::score(a, b) (ORBVocabulary.cpp:44-46): DBoW2's L1 score of two BoW vectors, as a double rounded to the `float` every
        caller in the reference assigns it to.  a, b: {word: value} or (words, values).  0.0 when they share no word.
        A convenience for single comparisons: every call builds and destroys a one-entry database (device allocations of n_words * 8 bytes and
        several synchronisations).  To score one vector against many, add them to a PlaceRecognizer and read `score` of a query with details=True."""
        rec = PlaceRecognizer(self.size(), self._ex)
        try:
            rec.add(0, b)
            return float(rec.detectRelocalizationCandidates(a, details=True)[1]["score"][0])
        finally:
            rec.close()


def _bow_arrays(bow):
    """{word: value} or (words, values) -> (int32 [m] ascending, float64 [m])"""
    if isinstance(bow, dict):
        ks = sorted(bow)
        return np.asarray(ks, np.int32), np.asarray([bow[k] for k in ks], np.float64)
    w, v = bow
    return np.ascontiguousarray(w, np.int32).reshape(-1), np.ascontiguousarray(v, np.float64).reshape(-1)


class PlaceRecognizer:
    """HYSLAM::PlaceRecognizer (src/core/PlaceRecognizer.cpp:43-311) over a key-frame BoW database resident on the device (hs_place_db).  A key
    frame is named by a caller-chosen integer `key` (< 2^64, unique among live entries): it stands for the KeyFrame* and orders the results where
    the reference orders by address.  Covisibility is the caller's: `neighbours` maps a key to the keys of GetBestCovisibilityKeyFrames(10) in
    that call's order (a dict, or a callable key -> list); unknown or erased keys in a list are ignored."""

    def __init__(self, n_words, extractor=None, scoring=0):
        self._ex = extractor or ORBExtractor()
        self._lib = self._ex._lib
        self._db = C.c_void_p()
        N.check(self._ex._h, self._lib.hs_place_db_create(self._ex._h, int(n_words), int(scoring), C.byref(self._db)))
        self._slot = {}                                    # key -> slot (live entries)
        self._keys = []                                    # slot -> key

    def close(self):
        if getattr(self, "_db", None) and self._db.value:
            self._lib.hs_place_db_destroy(self._db)
            self._db = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        live, slots = C.c_int32(), C.c_int32()
        self._lib.hs_place_db_size(self._db, C.byref(live), C.byref(slots))
        return live.value, slots.value

    def add(self, key, bow):
        if key in self._slot:
            raise ValueError("key %r is already in the database" % (key,))
        w, v = _bow_arrays(bow)
        slot = C.c_int32()
        N.check(self._ex._h, self._lib.hs_place_db_add(self._db, int(key), w.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), len(w), C.byref(slot)))
        self._slot[key] = slot.value
        self._keys.append(key)
        return slot.value

    def add_device(self, key, d_word, d_value, d_m, m_max, stream=None):
        """the outputs of hs_bow_vector_device, without a host round trip"""
        if key in self._slot:
            raise ValueError("key %r is already in the database" % (key,))
        slot = C.c_int32()
        N.check(self._ex._h, self._lib.hs_place_db_add_device(self._db, int(key), C.c_void_p(d_word), C.c_void_p(d_value), C.c_void_p(d_m), int(m_max),
                                                              C.byref(slot), C.c_void_p(stream)))
        self._slot[key] = slot.value
        self._keys.append(key)
        return slot.value

    def erase(self, key):
        N.check(self._ex._h, self._lib.hs_place_db_erase(self._db, self._slot[key]))
        del self._slot[key]

    def clear(self):
        N.check(self._ex._h, self._lib.hs_place_db_clear(self._db))
        self._slot, self._keys = {}, []

    def neighbour_table(self, neighbours):
        """[slots][10] int32 for the C ABI"""
        t = np.full((len(self._keys), 10), -1, np.int32)
        if neighbours is None:
            return t
        get = neighbours if callable(neighbours) else (lambda k: neighbours.get(k, ()))
        for key, slot in self._slot.items():
            row = [self._slot[k] for k in list(get(key))[:10] if k in self._slot]      # an erased key frame is no longer in the inverted file
            t[slot, :len(row)] = row
        return t

    def _query(self, loop, bow, neighbours, connected, min_score, details):
        w, v = _bow_arrays(bow)
        slots = len(self._keys)
        neigh = self.neighbour_table(neighbours)
        cand, n = np.zeros(max(slots, 1), np.int32), C.c_int32()
        out = dict(words=np.zeros(slots, np.int32), score=np.zeros(slots, np.float32), acc=np.zeros(slots, np.float32), best=np.zeros(slots, np.int32))
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        opt = [p(out[k]) if details else None for k in ("words", "score", "acc", "best")]
        if loop:
            excl = np.zeros(max(slots, 1), np.uint8)
            for k in connected or ():
                if k in self._slot:
                    excl[self._slot[k]] = 1
            st = self._lib.hs_place_query_loop(self._db, p(w), p(v), len(w), p(excl), float(min_score), p(neigh), p(cand), slots, C.byref(n), *opt)
        else:
            st = self._lib.hs_place_query_reloc(self._db, p(w), p(v), len(w), p(neigh), p(cand), slots, C.byref(n), *opt)
        N.check(self._ex._h, st)
        keys = [self._keys[s] for s in cand[:n.value]]
        return (keys, out) if details else keys

    def detectRelocalizationCandidates(self, bow, neighbours=None, details=False):
        """(:201-311) the candidate keys in ascending key order; details=True also returns the per-slot words / score / acc / best arrays"""
        return self._query(False, bow, neighbours, None, 0.0, details)

    def detectLoopCandidates(self, bow, minScore, connected=(), neighbours=None, details=False):
        """(:81-199) `connected`: the keys of the query key frame's GetConnectedKeyFrames(), left out of the search"""
        return self._query(True, bow, neighbours, connected, minScore, details)


class ORBFactory:
    """HYSLAM::ORBFactory: hands out extractors and matcher settings (FeatureFactory.h:21-33, ORBFactory.cpp:13-45)."""

    def __init__(self, extractor_settings=None, matcher_settings=None, device=0):
        self.extractor_settings = extractor_settings or FeatureExtractorSettings()
        self.matcher_settings = matcher_settings or FeatureMatcherSettings()
        self.device = device

    def getExtractor(self, settings=None):
        return ORBExtractor(settings or self.extractor_settings, self.device)

    def getFeatureMatcher(self, extractor=None):
        return FeatureMatcher(self.matcher_settings, extractor)

    def getFeatureExtractorSettings(self):
        return self.extractor_settings

    def getFeatureMatcherSettings(self):
        return self.matcher_settings

    def setFeatureMatcherSettings(self, s):
        self.matcher_settings = s

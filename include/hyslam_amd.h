/* hyslam_amd.h — C ABI of the MI355X-native ORB extract + Hamming match path for hySLAM.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch/OpenCV
 * types, int status codes, caller-allocated outputs.  A hySLAM maintainer binds it from a
 * `HipORBExtractor : FeatureExtractor` / `HipORBFactory : FeatureFactory` adaptor (see
 * INTEGRATION.md and hyslam_amd/host/).  File:line citations are relative to the reference
 * repository (bmhopkinson/hyslam).
 *
 * Threading: a handle is thread-compatible (one thread at a time); distinct handles are fully
 * concurrent — this matches the reference, which runs two separate extractor instances for the
 * left and right image (src/main/ImageProcessing.cpp:31-32,82-84).  What a handle reaches that is NOT its own (DESIGN.md 5.17 names the test that
 * holds each line under concurrent handles):
 *   - the frame cache (hs_frame_*): one per device and process, 16 slots, guarded by one mutex.  Any thread may publish, find, read by token,
 *     release and clear at the same time.  A reader of a token gets that frame's exact data, or HS_ERR_INVALID when the slot was pushed out,
 *     released or cleared meanwhile (the caller then passes host pointers); a slot is never refilled or freed under a reader (publish skips it,
 *     hs_frame_cache_clear answers HS_ERR_INVALID);
 *   - the poison mode (hs_debug_poison) and its violation counter: two process-wide atomics.  Setting the mode while other threads are inside
 *     calls is allowed and takes effect per call; which calls see it is not defined, so a test sets it while nothing else runs;
 *   - per-device kernel attributes (the raised dynamic-LDS limits of k_resize_chain, once per device, and of k_bow_vector, on every long call):
 *     idempotent; several threads may race through the first use;
 *   - the tuning variables (HS_*): read from the environment when a handle is created, a few once per process at their first use.  Creating
 *     handles on several threads is fine; changing the environment while another thread creates one is the caller's race (getenv);
 *   - hs_vocab_last_error: per calling thread.  hs_comm_available: loads the collective library once, under std::call_once.
 * An object made from a handle follows its own rule, stated where it is declared: an hs_vocab_dev may serve hs_bow_transform_device calls of several
 * handles at once but hs_records_bow_match_device of one caller at a time; an hs_place_db takes one caller at a time (add and erase also wait for
 * the whole device: other handles' work is waited for, never disturbed).
 *
 * Device pointers: every `*_device` entry point takes pointers into HBM of the handle's device
 * and enqueues work on `stream` (a hipStream_t passed as void*; NULL = the handle's own stream)
 * without synchronising.  The plain entry points take host pointers, stage through pinned
 * buffers and synchronise before returning.
 */
#ifndef HYSLAM_AMD_H
#define HYSLAM_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HS_DESC_BYTES 32          /* ORBFinder::descriptor_cols(), src/features/low_level/ORBFinder.h:88 */

enum hs_status {
    HS_OK = 0,
    HS_ERR_INVALID = 1,           /* bad argument / unsupported parameter combination            */
    HS_ERR_HIP = 2,               /* a HIP runtime call failed; see hs_*_last_error               */
    HS_ERR_CAPACITY = 3,          /* caller's output capacity too small (nothing partial written) */
    HS_ERR_NO_DEVICE = 4,         /* no usable gfx950 device                                       */
    HS_ERR_POISON = 5             /* hs_debug_poison: a kernel wrote past a staged piece            */
};

/* The cv::KeyPoint fields the reference sets (ORBExtractor.cpp:478-487,546-552; class_id stays -1). */
typedef struct hs_keypoint {
    float x, y;                   /* level-0 pixel coordinates (level coords * scale[octave])     */
    float size;                   /* (int)(31 * scale[octave])                                     */
    float angle;                  /* degrees [0,360), intensity centroid on the blurred level      */
    float response;               /* FAST corner score                                             */
    int32_t octave;
} hs_keypoint;

/* HYSLAM::FeatureExtractorSettings (src/core/FeatureExtractorSettings.h:19-32) + the two knobs the
 * reference hard-wires. */
typedef struct hs_orb_params {
    int32_t nfeatures;            /* nFeatures                                                     */
    float   scale_factor;         /* fScaleFactor                                                  */
    int32_t nlevels;              /* nLevels (1..16)                                               */
    int32_t cell_px;              /* N_CELLS: FAST cell edge in pixels (ORBExtractor.cpp:409)      */
    int32_t ini_th_fast;          /* init_threshold: accepted, unused — reference quirk, ORBFinder.cpp:58-60 */
    int32_t min_th_fast;          /* min_threshold:  accepted, unused — idem                       */
    int32_t fast_threshold;       /* effective FAST threshold; the reference always runs 20        */
    uint16_t blur_taps[7];        /* 7-tap Gaussian, unsigned 8.8 fixed point; all 0 => 18,34,49,55,49,34,18 */
    uint16_t _pad;
} hs_orb_params;

/* What Stereomatcher reads from Camera and FeatureMatcherSettings (src/features/Stereomatcher.cpp:7-24). */
typedef struct hs_stereo_params {
    float   fx;                   /* Camera::fx()                                                   */
    float   mbf;                  /* Camera::mbf                                                    */
    int32_t n_rows;               /* (int)Camera::mnMaxY                                            */
    float   th_high, th_low;      /* FeatureMatcherSettings::TH_HIGH / TH_LOW (FeatureMatcher.h:98-103) */
    float   size_ref;             /* FeatureExtractorSettings::size_ref (31)                        */
} hs_stereo_params;

typedef struct hs_orb hs_orb;     /* one FeatureExtractor instance (+ its device workspace and stream) */

/* ---- library ---- */
const char* hs_version(void);
const char* hs_status_string(int status);
int hs_device_count(int* count);

/* ---- extractor: replaces HYSLAM::ORBExtractor behind FeatureExtractor (src/features/FeatureExtractor.h:25-37) ---- */
/* defaults of ORBFactory::ORBFactory(), src/features/ORBFactory.cpp:13-25 */
void hs_orb_default_params(hs_orb_params* p);
/* ORBFactory::getExtractor(settings) -> ORBExtractor ctor, src/features/ORBFactory.cpp:37-40, ORBExtractor.cpp:76-119 */
int  hs_orb_create(const hs_orb_params* p, int device, hs_orb** out);
void hs_orb_destroy(hs_orb* h);
const char* hs_orb_last_error(const hs_orb* h);
/* GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares,
 * FeatureExtractor.h:31-36.  Any output pointer may be NULL; arrays hold nlevels entries. */
int  hs_orb_get_levels(const hs_orb* h);
int  hs_orb_get_device(const hs_orb* h);          /* the device index given to hs_orb_create (-1 for a NULL handle) */
float hs_orb_get_scale_factor(const hs_orb* h);
int  hs_orb_get_scale_tables(const hs_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                             int32_t* features_per_level);
/* smallest `cap` that can never overflow: nfeatures + per-level overshoot of DistributeOctTree.  Frames wider than 8:1 start the
 * quadtree with more than 8 root nodes per level and need more: call hs_orb_reserve() for the frame size first, the value then covers it. */
int  hs_orb_max_keypoints(const hs_orb* h);
/* optional: size the device workspace up front for `batch` images of w x h (grows lazily otherwise) */
int  hs_orb_reserve(hs_orb* h, int w, int h_px, int batch);

/* ORBExtractor::operator()(image, mask, keypoints, descriptors), ORBExtractor.cpp:496-562.
 * img: CV_8UC1 rows of `stride` bytes (host).  Writes *n keypoints (<= cap) and n*32 descriptor bytes.
 * An empty image (w==0||h==0||!img) returns HS_OK with *n = 0, like the reference's silent return (:499-500). */
int  hs_orb_extract(hs_orb* h, const uint8_t* img, int w, int h_px, int stride,
                    hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n);
/* `batch` same-sized host images; outputs are [batch][cap] / [batch][cap][32] / [batch]. */
int  hs_orb_extract_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, int stride,
                          hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n);
/* ---- the camera frame as it arrives: ImageProcessing::PreProcessImg on the device (src/main/ImageProcessing.cpp:118-138; it sits inside the
 * reference's timing bracket, :70 / :112, in front of both extractor calls, :76-77).  cv::resize(img, img, Size(), scale, scale) on the 1-, 3- or
 * 4-channel 8-bit frame — a copy at scale 1, the rounded 2x2 mean INTER_LINEAR silently becomes at exactly 0.5 (the reference's "Imaging" camera:
 * 2704 x 2028 x 3 -> 1352 x 1014), OpenCV's 11-bit fixed-point bilinear otherwise — then cvtColor to grey with its 14-bit weights (R 4899, G 9617,
 * B 1868); `rgb` = the camera's `RGB:` key (1: channel 0 is red: CV_RGB(A)2GRAY, 0: CV_BGR(A)2GRAY).  The scaled size is cvRound(w * scale). */
typedef struct hs_preprocess_params { int32_t channels; int32_t rgb; float scale; int32_t _pad; } hs_preprocess_params;
void hs_preprocess_size(int w, int h_px, float scale, int32_t* ow, int32_t* oh);
/* device frames (image i at d_src + i * image_stride, rows `row_stride` bytes apart, channels interleaved) -> device grey frames of the scaled size;
 * asynchronous on `stream` (the handle's own when 0).  Only the ow x oh pixels of every grey frame are written.
 * Layout: d_src, d_grey and all four strides may have ANY alignment (a source whose base and strides are multiples of 4 is read with dword loads, any
 * other with byte loads; grey rows are stored as dwords where they fall on one and as bytes elsewhere, never past column ow, so grey_row_stride == ow
 * is allowed).  Rows and images must not overlap.
 * Refused with HS_ERR_INVALID, nothing enqueued and nothing written, the handle stays usable — here and in the two camera-batch calls below:
 * pp->channels other than 1, 3 and 4; pp->scale outside (0, 16]; a scaled size (hs_preprocess_size) that is empty; row_stride < w * pp->channels;
 * w or h_px above 32768.  hs_preprocess_device also refuses a scaled size above 16384 either way, grey_row_stride < ow, w or h_px < 1 and batch < 1. */
int  hs_preprocess_device(hs_orb* h, const uint8_t* d_src, int w, int h_px, size_t row_stride, size_t image_stride, int batch, const hs_preprocess_params* pp,
                          uint8_t* d_grey, size_t grey_row_stride, size_t grey_image_stride, void* stream);
/* ProcessMonoImage / ProcessStereoImage's `PreProcessImg(...)` + `(*extractor)(mImGray, ...)` in one call (ImageProcessing.cpp:44,55 / :76-77,82-83): `batch`
 * host frames of w x h_px x pp->channels cross PCIe as they are, are reduced to grey level-0 frames on the device and extracted; outputs as
 * hs_orb_extract_batch ([batch][cap] ...; cap >= hs_orb_max_keypoints after hs_orb_reserve(h, ow, oh, batch) with (ow, oh) = hs_preprocess_size).
 * grey_out (may be NULL): the grey frames, batch x oh x ow tight — what the reference keeps as track_data.image (:60,108). */
int  hs_orb_extract_camera_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, size_t row_stride, const hs_preprocess_params* pp,
                                 hs_keypoint* kps, uint8_t* desc, int cap, int32_t* n, uint8_t* grey_out);
/* the same through the pipelined ingest (hs_orb_submit_batch's ticket machinery, two tickets in flight): the camera's frames are copied in on the copy-in
 * stream, PreProcessImg runs on the compute stream in front of the pyramid; with `sp` the batch is [left frames | right frames] of batch / 2 stereo pairs and the
 * ticket also carries uRight / depth — ProcessStereoImage's PreProcessImg x 2 + extractors + Stereomatcher (ImageProcessing.cpp:76-103) as ONE ticket.
 * Results by hs_orb_wait as for any ticket (cap >= hs_orb_max_keypoints for the SCALED size). */
int  hs_orb_submit_camera_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, size_t row_stride, const hs_preprocess_params* pp,
                                const hs_stereo_params* sp, int32_t* ticket);

/* Device-resident batch: image i starts at d_imgs + i*image_stride, rows `row_stride` bytes apart.
 * d_kps [batch][cap], d_desc [batch][cap][32] (16-byte aligned), d_n [batch]; all device memory.  Asynchronous.
 * ONE STREAM AT A TIME PER HANDLE: the *_device entry points take a caller stream, but a handle's workspace, the FAST kernel's work-queue counter
 * rotation and its spill halves assume that every call on the handle is ordered after the previous one — drive a handle from one stream (or order the
 * streams yourself); use separate handles for concurrent streams. */
int  hs_orb_extract_batch_device(hs_orb* h, const uint8_t* d_imgs, int batch, int w, int h_px,
                                 size_t row_stride, size_t image_stride,
                                 hs_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, void* stream);

/* ---- pipelined host ingest: the reference's bounded frame queue (System::TrackStereo throttles the producer at more than two waiting frames,
 * src/main/System.cc:194-196; ImageProcessing pops, extracts, matches: src/main/ImageProcessing.cpp:69-116) ----
 * hs_orb_submit_batch enqueues `batch` same-sized host frames and returns a ticket at once: the frames are copied in on a copy stream while the
 * kernels of the previously submitted batch still run, the results leave on a third stream into page-locked memory of the handle.  With `sp`
 * != NULL the batch is batch/2 stereo pairs — images [0, batch/2) left, [batch/2, batch) right — and the stereo matcher runs too.
 * hs_orb_wait blocks until that ticket's results are on the host and copies them out: kps [batch][cap], desc [batch][cap][32], n [batch],
 * uRight / depth [batch/2][cap] (stereo tickets only; NULL otherwise); cap >= hs_orb_max_keypoints().
 * At most TWO tickets may be in flight (two staging slots): a third submit returns HS_ERR_INVALID until the oldest was waited for.
 * Frames in page-locked memory (hs_host_alloc, or the caller's own hipHostMalloc / hipHostRegister) are DMA'd at link speed; pageable frames
 * work too and go through the runtime's staging path.
 * LIFETIME OF THE FRAMES: hs_orb_submit_batch returns BEFORE the frames have been read (page-locked frames are DMA'd asynchronously) — they must stay
 * valid and UNCHANGED until hs_orb_wait (or hs_orb_cancel) for that ticket returns, or until hs_ticket_frames_copied(h, ticket) returns 1 (the
 * copy-in of that ticket is complete: a capture buffer may be recycled from then on; 0 = not yet, -1 = unknown ticket).  A capture loop that reuses
 * its buffer right after submit gets silently corrupted features.
 * hs_orb_cancel(h, ticket): give up a ticket — waits until its batch has drained, drops the results, frees the slot.
 * A failed hs_orb_submit_batch leaves no ticket and no work behind (the streams are drained before it returns); a hs_orb_wait that fails with
 * HS_ERR_CAPACITY / HS_ERR_INVALID keeps the ticket (call again with valid arguments), one that fails with HS_ERR_HIP releases it. */
int  hs_host_alloc(size_t bytes, void** out);
void hs_host_free(void* p);
int  hs_orb_submit_batch(hs_orb* h, const uint8_t* const* imgs, int batch, int w, int h_px, int stride, const hs_stereo_params* sp, int32_t* ticket);
int  hs_orb_wait(hs_orb* h, int32_t ticket, hs_keypoint* kps, uint8_t* desc, int32_t* n, int cap, float* uRight, float* depth);
int  hs_orb_cancel(hs_orb* h, int32_t ticket);
int  hs_ticket_frames_copied(hs_orb* h, int32_t ticket);

/* ---- stereo: replaces Stereomatcher::computeStereoMatches + getData, src/features/Stereomatcher.cpp:26-156 ---- */
/* uRight[nL], depth[nL]: -1 where there is no stereo match (Stereomatcher.h:44-47). */
int  hs_stereo_match(hs_orb* h, const hs_keypoint* kpsL, const uint8_t* descL, int nL,
                     const hs_keypoint* kpsR, const uint8_t* descR, int nR,
                     const hs_stereo_params* sp, float* uRight, float* depth);
/* Device batch of `pairs` stereo pairs laid out like the extractor's outputs (stride `cap` per frame).
 * d_uRight / d_depth: [pairs][cap].  Asynchronous. */
int  hs_stereo_match_batch_device(hs_orb* h, const hs_keypoint* d_kpsL, const uint8_t* d_descL, const int32_t* d_nL,
                                  const hs_keypoint* d_kpsR, const uint8_t* d_descR, const int32_t* d_nR,
                                  int pairs, int cap, const hs_stereo_params* sp,
                                  float* d_uRight, float* d_depth, void* stream);

/* ImageProcessing::ProcessStereoImage's compute (src/main/ImageProcessing.cpp:82-84,100-103) for a
 * device-resident batch: extract left and right frames, then stereo-match each pair.  Asynchronous. */
int  hs_stereo_frontend_batch_device(hs_orb* h, const uint8_t* d_left, const uint8_t* d_right, int pairs,
                                     int w, int h_px, size_t row_stride, size_t image_stride,
                                     hs_keypoint* d_kpsL, uint8_t* d_descL, int32_t* d_nL,
                                     hs_keypoint* d_kpsR, uint8_t* d_descR, int32_t* d_nR, int cap,
                                     const hs_stereo_params* sp, float* d_uRight, float* d_depth, void* stream);

/* Concurrency inside one handle: with lanes = 2 the batched device entry points (hs_orb_extract_batch_device,
 * hs_stereo_frontend_batch_device) split their batch in two halves that run on two streams with separate workspaces (the second lane
 * is an internal child handle).  The kernels of this path are latency-bound rather than bandwidth-bound, so two interleaved launch
 * sequences fill each other's stalls (+15 % pairs/s measured).  Ordering towards the caller is unchanged: all work is complete when the
 * caller's stream reaches the point after the call.  Default 1. */
int  hs_orb_set_lanes(hs_orb* h, int lanes);

/* The launch sequence of an extraction can be SPLIT: level 0 needs no pyramid, so its FAST + quadtree can run on a second stream of the handle
 * beside the pyramid and the other levels' FAST + quadtree (joined before the describe stage; same kernels, same results).  mode -1 (default): split
 * one or two large frames (>= 6 Mpx per call); 0: never; 1: always.  Measured (profiles/README.md, row "C4"; profiles/r03_bench_lines.json -> c4): the
 * 4000 x 3000 "Imaging" extraction 0.413 ms unsplit (round 2) -> 0.207 ms split; for an isolated 1080p pair the fork / join between the streams costs
 * more than the overlap saves (0.132 -> 0.160 ms in round 3), but when several handles share the GPU (hySLAM's SLAM stereo camera + Imaging camera,
 * BASELINE config 4) splitting BOTH lets their kernels interleave: 2 592 -> 4 068 steps/s.  Ignored while stage events are on.
 * The two concurrent FAST launches of a split call rely on every earlier launch of the handle having completed — one more reason for the
 * one-stream-at-a-time rule of the *_device entry points (see hs_orb_extract_batch_device). */
int  hs_orb_set_split(hs_orb* h, int mode);

/* block until everything enqueued on the handle's own stream (or `stream`) has finished */
int  hs_orb_synchronize(hs_orb* h, void* stream);

/* ================= matchers on flat arrays: the cores of HYSLAM::FeatureMatcher (src/features/FeatureMatcher.h:105-176) =================
 * The C++ adaptor gathers Frame / KeyFrame / MapPoint fields into these arrays and replays associations
 * (Frame::associateLandMark) from the returned per-landmark results, in the reference's order.  Containers the
 * reference orders by MapPoint* address are replaced by landmark ARRAY ORDER (pass landmarks sorted by address to
 * reproduce its iteration order).  Host pointers; synchronous. */

/* what _SearchByProjection_ reads from Frame / Camera / FeatureViews / LandMarkMatches
 * (src/core/Frame.cc:45-72,137-180,416-469; src/core/Camera.cpp:116-153) */
typedef struct hs_frame_view {
    float Rcw[9], tcw[3], Ow[3];       /* mRcw (row-major), mtcw, mOw                                  */
    float fx, fy, cx, cy, mbf;         /* K, Camera::mbf                                                */
    int32_t sensor;                    /* Camera::sensor: 0 mono, 1 stereo, 2 RGBD                      */
    float min_x, max_x, min_y, max_y;  /* mnMinX .. mnMaxY                                              */
    float size_ref;                    /* views.orbParams().size_ref (31)                               */
    int32_t n;                         /* number of keypoints                                           */
    const hs_keypoint* kps;            /* [n]                                                           */
    const uint8_t* desc;               /* [n][32]                                                       */
    const float* uR;                   /* [n], < 0 = no stereo correspondence                           */
    const int32_t* kp_lm_obs;          /* [n]: -1 = keypoint has no landmark, else Observations() of it */
} hs_frame_view;

/* the MapPoint fields the matchers read (src/core/MapPoint.h:54-169) */
typedef struct hs_landmark {
    float pos[3];                      /* GetWorldPos()                                                 */
    float size;                        /* getSize(), world units                                        */
    float min_dist, max_dist;          /* mfMinDistance, mfMaxDistance (before the 0.8 / 1.2 factors, MapPoint.cc:139-149) */
    float normal[3];                   /* GetNormal()                                                   */
    int32_t assoc_kp;                  /* Frame::hasAssociation(lm) in THIS frame, -1 if none (Frame.cc:296-300) */
    float prev_angle;                  /* angle of its keypoint in the previous frame (rotation check)  */
    int32_t skip;                      /* 1 = nullptr entry                                             */
    uint8_t desc[32];                  /* GetDescriptor()                                               */
} hs_landmark;

typedef struct hs_proj_params {
    float th;                          /* search radius factor                                          */
    float score_threshold;             /* BestScoreCriterion threshold: TH_HIGH or ORBdist              */
    float second_best_ratio;           /* mfNNratio or 1.0                                              */
    float frac_smaller, frac_larger;   /* FeatureSizeCriterion(0.5, 1.5)                                */
    int32_t use_distance;              /* DistanceCriterion among the landmark criteria                 */
    int32_t use_stereo;                /* StereoConsistencyCriterion(th)                                */
    int32_t check_rotation;            /* RotationConsistencyCriterion (uses prev_angle)                */
    int32_t use_prev_matched;          /* PreviouslyMatchedCriterion (all Frame variants; not Fuse)     */
    int32_t use_viewing_angle;         /* ViewingAngleCriterion(max_view_angle): Fuse, FeatureMatcher.cc:469 */
    float   max_view_angle;            /* radians (1.047)                                               */
    int32_t use_reprojection;          /* ProjectionViewCriterion(reproj_threshold): Fuse, :473         */
    float   reproj_threshold;          /* 5.99                                                          */
    float   sigma_ref;                 /* FeatureExtractorSettings::sigma_ref (1.0), determineSigma2    */
    int32_t first_wins;                /* Fuse: the first landmark that matched a keypoint keeps it (:515) */
    int32_t dist_is_invariance_range;  /* 1: hs_landmark::min_dist / max_dist already hold GetMinDistanceInvariance() / GetMaxDistanceInvariance()
                                          (= 0.8f*mfMinDistance, 1.2f*mfMaxDistance, MapPoint.cc:139-149) — what a hySLAM adaptor can read */
} hs_proj_params;

/* FeatureMatcher::_SearchByProjection_ (FeatureMatcher.cc:57-121) with the criteria of SearchByProjection(Frame, MapPoints, th)
 * (:123-143: use_distance=1,use_stereo=1,check_rotation=0), (CurrentFrame, LastFrame, th, bMono) (:145-176: 0,1,1) and
 * (CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:180-212: 1,0,0, ratio 1.0), and of Fuse(pKF, MapPoints, matches, th, err)
 * (:464-521: distance + viewing angle, size + reprojection + best score TH_LOW/1.0, first landmark per keypoint wins; the caller
 * marks bad / already-observed / protected landmarks with skip = 1).  match_idx[L] = keypoint index or -1,
 * match_dist[L] = Hamming distance of the match, *n_matches = matches.size(). */
int  hs_search_by_projection(hs_orb* h, const hs_frame_view* F, const hs_landmark* lms, int L, const hs_proj_params* pp,
                             int32_t* match_idx, float* match_dist, int32_t* n_matches);

/* Frame::AssignFeaturesToGrid / PosInGrid (src/core/Frame.cc:137-153,459-469): the 64 x 48 grid cell of every keypoint, cell = round((x - mnMinX) *
 * 64 / (mnMaxX - mnMinX)) (nearest, not floor), -1 when outside.  cell_xy [n][2] int8 (column, row).  The matchers build this grid on the device
 * themselves; the entry point exposes it for Frame construction on the host side and for tests.  Host pointers; synchronous. */
int  hs_frame_grid(hs_orb* h, const hs_frame_view* F, int8_t* cell_xy);

/* the same on device-resident data (FeatureViews stay in HBM between extraction and tracking): every pointer inside *F and
 * d_lms / d_match_idx / d_match_dist / d_n_matches are device pointers (F->kps / F->desc can be the extractor's own outputs).  Asynchronous. */
int  hs_search_by_projection_device(hs_orb* h, const hs_frame_view* F, const hs_landmark* d_lms, int L, const hs_proj_params* pp,
                                    int32_t* d_match_idx, float* d_match_dist, int32_t* d_n_matches, void* stream);

/* ---- device-resident frames: a frame's keypoints and descriptors stay in HBM between ImageProcessing and Tracking ----
 * The reference copies them into FeatureViews (src/core/FeatureViews.h:20-81, built in ImageProcessing.cpp:85,100 and stored by the Frame
 * constructor, src/core/Frame.cc:45-72), and every matcher call reads them back out of those host objects.  Here the extractor can keep what it
 * just produced on the device, and the matchers take it from there:
 *   hs_frame_publish   right after a host-pointer extraction (hs_orb_extract / hs_orb_extract_batch / hs_orb_wait) on `h`: keeps image `image` of
 *                      that call — device-to-device, on the handle's stream, no host round trip — in a per-device cache of 16 slots (oldest reused
 *                      first).  kps[n] = the keypoints the call returned for that image (kept beside the slot to recognise the frame later).
 *   hs_frame_find      hySLAM has no field that could carry a token through FeatureViews / Frame: a frame is recognised by its keypoint array
 *                      (exact comparison of all n records).  HS_ERR_INVALID when no live slot of `device` holds it.
 *   hs_frame_release   optional: give a slot back early.      hs_frame_info: its keypoint count.      hs_frame_cache_clear: free a device's cache.
 *   hs_search_by_projection_frame   hs_search_by_projection with F->kps / F->desc taken from the cache (both may be NULL in *F; F->n must equal the
 *                      published count; F->uR / F->kp_lm_obs are host arrays as before: they change between calls).
 *   hs_stereo_match_frames          hs_stereo_match on two published frames (left, right).
 * A token whose slot has been reused is unknown again: the call returns HS_ERR_INVALID and the caller uses the host-pointer entry point (the C++
 * adaptors do).  Tokens are per device; the calls are thread-safe against each other; a slot that a call is reading is never refilled. */
typedef uint64_t hs_frame_token;    /* 0 = none */
int  hs_frame_publish(hs_orb* h, int image, const hs_keypoint* kps, int n, hs_frame_token* token);
int  hs_frame_find(int device, const hs_keypoint* kps, int n, hs_frame_token* token);
int  hs_frame_release(int device, hs_frame_token token);
int  hs_frame_info(int device, hs_frame_token token, int32_t* n);
int  hs_frame_cache_clear(int device);  /* frees a device's cache (every token of it becomes unknown); HS_ERR_INVALID while a call is reading a slot.  The cache
                                            otherwise lives as long as the process: call this before unloading the library or resetting the device */
int  hs_search_by_projection_frame(hs_orb* h, hs_frame_token frame, const hs_frame_view* F, const hs_landmark* lms, int L, const hs_proj_params* pp,
                                   int32_t* match_idx, float* match_dist, int32_t* n_matches);
int  hs_stereo_match_frames(hs_orb* h, hs_frame_token left, hs_frame_token right, const hs_stereo_params* sp, float* uRight, float* depth);

/* ---- legacy loop-closing matchers (the reference keeps them for LoopClosing, which is a stub: src/main/System.cc:149) ----
 * FeatureMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (FeatureMatcher.cc:628-737).  KF = the keyframe (its OWN pose is used by
 * landMarkSizePixels, KeyFrame.cc:258-279 — reference quirk), Scw = the caller's Sim3 as a row-major 4x4.  lms[L] in vpPoints order with
 * min_dist / max_dist = GetMin/MaxDistanceInvariance() and skip = pMP->isBad() || already in vpMatched.  kp_matched[KF->n] (in/out) =
 * vpMatched[idx] != NULL.  The search is sequential by definition: a landmark cannot take a keypoint that an earlier landmark took (:713,731);
 * everything that does not depend on vpMatched runs in parallel first, the assignment walks the landmarks in order on one wavefront.
 * match_idx[L] = keypoint taken by landmark i or -1; *n_matches = nmatches.  Host pointers; synchronous. */
int  hs_search_by_projection_sim3(hs_orb* h, const hs_frame_view* KF, const float* Scw, const hs_landmark* lms, int L, int th, float th_low,
                                  uint8_t* kp_matched, int32_t* match_idx, int32_t* n_matches);
/* FeatureMatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (FeatureMatcher.cc:739-934): lms1[KF1->n] / lms2[KF2->n] = the landmark
 * of each keypoint (skip = none, bad or already matched; assoc_kp = its view in the OTHER keyframe; min_dist / max_dist = the invariance range).
 * Both directions run in parallel, then the agreement check.  match12[KF1->n] = KF2 keypoint index or -1; *n_found = nFound. */
int  hs_search_by_sim3(hs_orb* h, const hs_frame_view* KF1, const hs_landmark* lms1, const hs_frame_view* KF2, const hs_landmark* lms2,
                       float s12, const float* R12, const float* t12, float th, float th_high, int32_t* match12, int32_t* n_found);

/* the inner loops of SearchByBoW / SearchByBoW2 / _SearchByBoW_ (FeatureMatcher.cc:216-371): for every vocabulary node present in
 * both feature vectors, best / second-best Hamming of each side-1 index over the node's side-2 indices (BestMatchBoWCriterion,
 * MatchCriteria.cpp:601-635: d < threshold and d < ratio*d2, both strict), then RotationConsistencyBoW (:679-726).
 * Feature vectors (DBoW2::FeatureVector) as CSR: node ids ascending, node_ptr[n_nodes+1] (non-negative, non-decreasing), idx[] with
 * node_ptr[n_nodes] entries inside [0, n).  node_ptr is always checked on the host, idx whenever both sides have features and nodes
 * (HS_ERR_INVALID); the length of idx[] and the order of the node ids are the caller's.  keep1[n1] (may be NULL) = 1 for
 * side-1 indices that pass the index criteria (PreviouslyMatchedIndexCriterion).  match12[n1] = side-2 index or -1.  A side-1 feature
 * without any candidate is never matched, whatever the thresholds. */
int  hs_search_by_bow(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                      const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int n_nodes1,
                      const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                      const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int n_nodes2,
                      const uint8_t* keep1, float score_threshold, float second_best_ratio, int check_rotation,
                      int32_t* match12, int32_t* n_matches);
/* the same with the index criteria on BOTH sides (keep2, may be NULL: _SearchByBoW_, FeatureMatcher.cc:306-309) and, when F12 (row-major
 * 3x3, may be NULL) is given, EpipolarConsistencyBoWCriterion (MatchCriteria.cpp:641-676: dsqr < 3.84*sigma2(kp2.size)) ahead of the
 * best-match criterion — the core of SearchForTriangulation (FeatureMatcher.cc:373-402; threshold TH_LOW, ratio 1.0). */
int  hs_search_by_bow_ex(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                         const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int n_nodes1,
                         const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                         const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int n_nodes2,
                         const uint8_t* keep1, const uint8_t* keep2, const float* F12, float size_ref, float sigma_ref,
                         float score_threshold, float second_best_ratio, int check_rotation,
                         int32_t* match12, int32_t* n_matches);

/* The legacy FeatureMatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (FeatureMatcher.cc:938-1077; hySLAM never calls it — "aim to replace this with
 * SearchByBoW2" — bound for completeness of the FeatureMatcher surface): as hs_search_by_bow_ex without the epipolar gate, but a side-2 feature
 * can be matched only once (vbMatched2: the side-1 features of a node are processed in list order, one wavefront per shared node) and the
 * orientation histogram takes angle1 - angle2.  keep1 / keep2 = the view has a landmark that is not bad. */
int  hs_search_by_bow_legacy(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1,
                             const int32_t* node_id1, const int32_t* node_ptr1, const int32_t* idx1, int n_nodes1,
                             const hs_keypoint* kps2, const uint8_t* desc2, int n2,
                             const int32_t* node_id2, const int32_t* node_ptr2, const int32_t* idx2, int n_nodes2,
                             const uint8_t* keep1, const uint8_t* keep2, float th_low, float nnratio, int check_orientation,
                             int32_t* match12, int32_t* n_matches);

/* FeatureMatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (FeatureMatcher.cc:404-462; monocular map
 * initialisation, MonoInitializer.cpp:83).  Inherently sequential over F1's keypoints — a later keypoint takes over an F2 keypoint only
 * with a strictly smaller distance (MatchCriteria.cpp:525-549) — so one workgroup walks F1 in order and parallelises the window search
 * and the best / second-best reduction of each step.  F2 supplies the grid bounds, keypoints and descriptors (pose fields unused).
 * prev_matched_xy [n1][2] is vbPrevMatched (in/out), matches12 [n1] is vnMatches12.  Host pointers; synchronous. */
int  hs_search_for_initialization(hs_orb* h, const hs_keypoint* kps1, const uint8_t* desc1, int n1, const hs_frame_view* F2,
                                  float* prev_matched_xy, int window, float th_low, float nnratio,
                                  int32_t* matches12, int32_t* n_matches);

/* Vocabulary transform: what Frame::ComputeBoW / KeyFrame::ComputeBoW obtain from ORBVocabulary::transform -> DBoW2::TemplatedVocabulary<FORB>
 * ::transform(features, bow, fv, levelsup=4) (src/core/Frame.cc:472-479, src/features/low_level/ORBVocabulary.cpp:31-42).  DBoW2 and the
 * ORBvoc data are not part of the reference tree; the tree descent follows DBoW2's published algorithm (first minimum wins at every level).
 * Flat tree: node 0 = root, the children of a node are contiguous, child_count == 0 marks a leaf (word).  Outputs per descriptor: word id,
 * word weight and the id of the node passed at level (levels - levelsup), which keys DBoW2::FeatureVector.  Host pointers; synchronous. */
typedef struct hs_vocab_tree {
    int32_t n_nodes, levels;
    const int32_t* child_begin;        /* [n_nodes] */
    const int32_t* child_count;        /* [n_nodes] */
    const uint8_t* desc;               /* [n_nodes][32] */
    const int32_t* word_id;            /* [n_nodes], valid at leaves */
    const float* weight;               /* [n_nodes], valid at leaves */
    const int32_t* orig_id;            /* [n_nodes] or NULL: the DBoW2 NodeId of every flat node (reported as the feature-vector key) when a loader
                                          had to renumber a vocabulary; NULL = the flat index IS the DBoW2 id */
} hs_vocab_tree;
/* Vocabulary files: what ORBVocabulary::ORBVocabulary(vocab_file) loads through DBoW2 (src/features/low_level/ORBVocabulary.cpp:14-29): a path ending
 * in ".txt" is DBoW2's text format (loadFromTextFile, ORBvoc.txt), anything else the binary format (loadFromBinaryFile, the output of
 * tools/bin_vocabulary.cc).  DBoW2 and the vocabulary file are external to the reference; the formats are restated from the published ORB-SLAM2
 * DBoW2 sources (hs_vocab.hip).  Host only, no device needed.  hs_vocab_get_tree's arrays stay valid until hs_vocab_destroy. */
typedef struct hs_vocab hs_vocab;
/* text of the last failed hs_vocab_load on the calling thread ("" after a success): the loaders print nothing */
const char* hs_vocab_last_error(void);
int  hs_vocab_load(const char* path, hs_vocab** out);
int  hs_vocab_from_tree(const hs_vocab_tree* tree, int k, hs_vocab** out);      /* deep copy of a caller-built flat tree (synthetic vocabularies) */
int  hs_vocab_save(const hs_vocab* v, const char* path);                        /* ".txt" -> text, else binary: tools/bin_vocabulary.cc's conversion */
void hs_vocab_destroy(hs_vocab* v);
int  hs_vocab_get_tree(const hs_vocab* v, hs_vocab_tree* out);
int  hs_vocab_info(const hs_vocab* v, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words, int32_t* scoring, int32_t* weighting);

/* A vocabulary resident in HBM of h's device, prepared for feature vectors `levelsup` levels above the leaves (Frame::ComputeBoW uses 4,
 * src/core/Frame.cc:477).  Uploaded once; hs_vocab_dev_groups = number of distinct feature-vector nodes. */
typedef struct hs_vocab_dev hs_vocab_dev;
int  hs_vocab_upload(hs_orb* h, const hs_vocab_tree* tree, int levelsup, hs_vocab_dev** out);
void hs_vocab_dev_destroy(hs_vocab_dev* v);
int  hs_vocab_dev_groups(const hs_vocab_dev* v);
/* hs_bow_transform on descriptors that already live in HBM (the extractor's outputs): d_n (may be NULL) = device count clamped to n_max.
 * Asynchronous. */
int  hs_bow_transform_device(hs_orb* h, const hs_vocab_dev* v, const uint8_t* d_desc, const int32_t* d_n, int n_max,
                             int32_t* d_word, float* d_weight, int32_t* d_node, void* stream);
/* Cross-camera BoW matching over `world` gathered frame records (BASELINE config 5): for every peer p != rank the matching core of SearchByBoW /
 * _SearchByBoW_ (FeatureMatcher.cc:216-345: per shared vocabulary node, best / second-best Hamming of every side-1 feature over the node's side-2
 * features, `d < score_threshold && d < ratio * d2`, then RotationConsistencyBoW) between record `rank` (side 1) and record p (side 2), with the
 * vocabulary transform of all records done on the device.  d_match12 [world][cap] = side-2 index or -1 (row `rank`: all -1), d_n_matches [world].
 * No host synchronisation.  Asynchronous.  The matcher's scratch (feature groups, bucket lists) lives INSIDE `v`: one hs_vocab_dev serves one
 * caller stream at a time and is not thread-safe for this entry point (hs_bow_transform_device only reads `v` and may run concurrently); give
 * every handle / stream that matches concurrently its own hs_vocab_upload. */
int  hs_records_bow_match_device(hs_orb* h, hs_vocab_dev* v, const uint8_t* d_records, size_t record_stride, int world, int rank, int cap,
                                 float score_threshold, float second_best_ratio, int check_rotation,
                                 int32_t* d_match12, int32_t* d_n_matches, void* stream);

int  hs_bow_transform(hs_orb* h, const hs_vocab_tree* tree, const uint8_t* desc, int n, int levelsup,
                      int32_t* word_id, float* weight, int32_t* node_id);

/* ---- place recognition: the BoW vector, DBoW2's L1 score and HYSLAM::PlaceRecognizer (src/core/PlaceRecognizer.cpp:43-311), which KeyFrameDB::
 * DetectRelocalizationCandidates / DetectLoopCandidates (KeyFrameDB.cc:392-419) and Map::detectRelocalizationCandidates (Map.cc:552-559) reach ---- */
/* The BoW vector DBoW2::TemplatedVocabulary::transform leaves in Frame::mBowVec (Frame.cc:472-479), from the (word, weight) arrays of
 * hs_bow_transform(_device): `if (w > 0) v.addWeight(word, w)` per feature in feature order (double sums of the float weights), then
 * v.normalize(L1): norm = sum of |v| in ascending word order, every value divided by it when norm > 0.  out_word [m] ascending and unique,
 * out_value [m], *m <= n; outputs hold room for n (n_max) entries; n (n_max) <= 16384.  d_n (may be NULL) = device count clamped to n_max.
 * hs_bow_vector_device is asynchronous on `stream`; hs_bow_vector takes host pointers and returns when done. */
int  hs_bow_vector_device(hs_orb* h, const int32_t* d_word, const float* d_weight, const int32_t* d_n, int n_max,
                          int32_t* d_out_word, double* d_out_value, int32_t* d_m, void* stream);
int  hs_bow_vector(hs_orb* h, const int32_t* word, const float* weight, int n, int32_t* out_word, double* out_value, int32_t* m);

/* The key frames' BoW vectors resident in HBM of h's device (h lends its stream and error text and must outlive the database): what
 * PlaceRecognizer keeps as an inverted file (:43-78), here a CSR of (int32 word, double value) per slot.  `scoring`: DBoW2::ScoringType as
 * hs_vocab_info reports it; only 0 (L1_NORM, the one hySLAM's vocabulary uses) is accepted, anything else is HS_ERR_INVALID.
 * One caller at a time.  The dense query table, the maximum count and the default per-slot arrays exist ONCE per database: all work on one database
 * — queries included — must be ordered on a single stream or otherwise serialised by the caller; two queries in flight on different streams, or an
 * add / erase / clear next to a query in flight, corrupt each other silently. */
typedef struct hs_place_db hs_place_db;
int  hs_place_db_create(hs_orb* h, int n_words, int scoring, hs_place_db** out);
void hs_place_db_destroy(hs_place_db* db);
/* PlaceRecognizer::add (:43-51): stores a copy of the vector.  `key`: caller-chosen, unique among live entries; it takes the place of the
 * KeyFrame* address wherever the reference orders by address (the C++ adaptor passes the pointer value).  *slot is stable until
 * erase.  Words ascending, unique and < n_words, values finite and > 0 (checked by the host form: HS_ERR_INVALID); no limit on m below n_words,
 * HS_ERR_CAPACITY beyond 2^20 slots.  Storage grows by doubling (reallocate + copy, which drains the device); the host form returns when the copy
 * is done.  hs_place_db_add_device takes the outputs of hs_bow_vector_device without a host round trip: it reserves m_max entries, the length is
 * *d_m clamped to m_max (d_m NULL: m_max), nothing is checked; asynchronous on `stream` unless the storage has to grow. */
int  hs_place_db_add(hs_place_db* db, uint64_t key, const int32_t* word, const double* value, int m, int32_t* slot);
int  hs_place_db_add_device(hs_place_db* db, uint64_t key, const int32_t* d_word, const double* d_value, const int32_t* d_m, int m_max, int32_t* slot, void* stream);
/* PlaceRecognizer::erase (:53-72): leaves a tombstone; slots are reused only after hs_place_db_clear (PlaceRecognizer::clear, :74-78), which keeps
 * the allocations.  Both wait for the device. */
int  hs_place_db_erase(hs_place_db* db, int32_t slot);
int  hs_place_db_clear(hs_place_db* db);
int  hs_place_db_size(const hs_place_db* db, int32_t* live, int32_t* slots);     /* either pointer may be NULL */
/* PlaceRecognizer::detectRelocalizationCandidates (:201-311) / detectLoopCandidates (:81-199) for the query vector (qword, qvalue, qm).
 *   neigh    [slots][10] int32: the slots of GetBestCovisibilityKeyFrames(10) of every key frame, in that call's order (:153,267); -1 pads a row,
 *            a tombstoned or out-of-range slot is ignored; NULL = no key frame has neighbours
 *   exclude  [slots] u8 (loop; may be NULL): spConnectedKeyFrames (:83,97) — nothing else is excluded, not even the query key frame itself
 * Score pass: per slot the shared-word count and float si = (float)L1Scoring::score(query, key frame) — `fabs(vi - wi) - fabs(vi) - fabs(wi)` added
 * per shared word in ascending word order in double, -s / 2.0.  Then `int minCommonWords = maxCommonWords * 0.8f`; reloc: scored = words >
 * minCommonWords, every neighbour that shares a word adds its score (the score it HAS, also when it was not scored) and replaces
 * pBestKF on a strictly greater one, bestAccScore from 0, retained = acc > 0.75f * bestAccScore, result = the SET of retained pBestKF in ascending
 * key order (KeyFrameDB's std::set<KeyFrame*>).  loop: the count is the number of shared words MINUS ONE (`insert({pKFi, 0})` on the first hit,
 * :98-102), listed = scored and si >= min_score, a neighbour contributes only when it is scored, bestAccScore from min_score, entries walked in
 * ascending key order (std::map<KeyFrame*, int>), result = pBestKF of every retained entry in walk order, first occurrence only.
 * Outputs: cand_slot [cap], *n_cand; optional (NULL = not wanted) per-slot arrays [slots]: words (the reference's count; -1 = the key frame is not
 * in lKFsSharingWords / shared_words), score (si; 0 without a shared word), acc and best (accScore and pBestKF's slot of a listed key frame; 0 / -1
 * otherwise) — the scores KeyFrameDB.cc:393's note asks for.  Host forms: synchronous; HS_ERR_CAPACITY when cap is too small (*n_cand = the
 * required count, no candidate written).  Device forms: every pointer in HBM, d_qm (may be NULL) = device count clamped to qm_max, asynchronous on
 * `stream`; they cannot return a capacity status: *d_n_cand ALWAYS holds the required count and NO candidate is written when it exceeds cap.  The
 * first query after an add / erase / clear uploads the key order and waits for `stream`; steady-state queries allocate and wait for nothing. */
int  hs_place_query_reloc(hs_place_db* db, const int32_t* qword, const double* qvalue, int qm, const int32_t* neigh,
                          int32_t* cand_slot, int cap, int32_t* n_cand, int32_t* words, float* score, float* acc, int32_t* best);
int  hs_place_query_loop(hs_place_db* db, const int32_t* qword, const double* qvalue, int qm, const uint8_t* exclude, float min_score, const int32_t* neigh,
                         int32_t* cand_slot, int cap, int32_t* n_cand, int32_t* words, float* score, float* acc, int32_t* best);
int  hs_place_query_reloc_device(hs_place_db* db, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qm, int qm_max, const int32_t* d_neigh,
                                 int32_t* d_cand_slot, int cap, int32_t* d_n_cand, int32_t* d_words, float* d_score, float* d_acc, int32_t* d_best, void* stream);
int  hs_place_query_loop_device(hs_place_db* db, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qm, int qm_max, const uint8_t* d_exclude,
                                float min_score, const int32_t* d_neigh, int32_t* d_cand_slot, int cap, int32_t* d_n_cand,
                                int32_t* d_words, float* d_score, float* d_acc, int32_t* d_best, void* stream);

/* brute-force Hamming 2-NN (cross-camera matching without a vocabulary): for each of nq query descriptors the first-minimum
 * train index, its distance and the second-smallest distance (-1 when absent). */
int  hs_hamming_knn2(hs_orb* h, const uint8_t* q, int nq, const uint8_t* t, int nt,
                     int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
/* same on device pointers, asynchronous */
int  hs_hamming_knn2_device(hs_orb* h, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                            int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist, void* stream);

/* ---- landmark representative descriptors: MapPointDBEntry::_computeDistinctiveDescriptor_ (src/core/MapPointDB.cpp:128-175) for a batch.
 * CSR input: landmark i has N_i = offsets[i+1] - offsets[i] observation descriptors desc[offsets[i] .. offsets[i+1])[32], offsets non-decreasing,
 * offsets[0] >= 0.  Container order is the caller's ARRAY ORDER: the reference walks its std::map<KeyFrame*, FeatureDescriptor>, so pass each
 * landmark's observations sorted by KeyFrame address, with the isBad() key frames left out (MapPointDB.cpp:131-135).  Per landmark: the N x N
 * Hamming matrix (0 on the diagonal), every row's median = element (size_t)(0.5*(N-1)) of the ascending row, and the FIRST row with the strictly
 * smallest median (MapPointDB.cpp:160-171).  best[i] = that row's index within the landmark (0 for N = 1), median[i] = its median; both -1 for
 * N_i = 0, where the reference returns without changing the landmark.  Duplicate descriptors are allowed; N_i < 2^31, otherwise unbounded.
 * Host pointers; synchronous. */
int  hs_landmark_best_descriptors(hs_orb* h, const int64_t* offsets, const uint8_t* desc, int L, int32_t* best, int32_t* median);
/* the same on device pointers (d_offsets [L+1] 8-byte aligned, d_desc 16-byte aligned, d_best / d_median [L]), enqueued on `stream` (NULL = the
 * handle's own stream) without synchronising; the offsets are not checked on the host.  The handle's one-stream-at-a-time rule applies
 * (see hs_orb_extract_batch_device).  Asynchronous. */
int  hs_landmark_best_descriptors_device(hs_orb* h, const int64_t* d_offsets, const uint8_t* d_desc, int L, int32_t* d_best, int32_t* d_median,
                                         void* stream);

/* ---- landmark entry update: MapPointDBEntry::_updateEntry_ (src/core/MapPointDB.cpp:223-228) for a batch — all four steps in one call:
 * _updateNormalAndDepth_ (:230-265), _computeDistinctiveDescriptor_ (:128-175, exactly as hs_landmark_best_descriptors), _updateMeanDistance_
 * (:267-289) and _updateSize_ (:291-310, with KeyFrame::featureSizeMetric, KeyFrame.cc:234-255, and Camera::Unproject, Camera.cpp:155-159).
 * The float / double rounding of every step is DESIGN.md D8 (OpenCV 3.4's cv::norm, scaleAdd and convertTo restated). */
typedef struct hs_lm_entry_in {
    float pos[3];                      /* pMP_entry->GetWorldPos() (MapPointDB.cpp:238,272)                               */
    float ref_Ow[3];                   /* pKF_ref->GetCameraCenter() (:255); pKF_ref need not be among the observations   */
} hs_lm_entry_in;

/* one entry of the landmark's `observations` map (KeyFrame*, keypoint index), in the map's order = sorted by KeyFrame address */
typedef struct hs_lm_obs {
    float Ow[3];                       /* pKF->GetCameraCenter() (:247,280; KeyFrame.cc:241)                              */
    float fx, fy, cx, cy;              /* pKF's camera, Camera::Unproject (Camera.cpp:155-159)                            */
    float u, v, kp_size;               /* views.keypt(idx).pt.x, .pt.y, .size (KeyFrame.cc:245-247)                       */
    float assoc_pos[3];                /* hasAssociation(idx)->GetWorldPos() (KeyFrame.cc:235-240), normally = pos        */
    int32_t assoc;                     /* 0: hasAssociation(idx) is NULL, featureSizeMetric returns -1 (KeyFrame.cc:236-238) */
} hs_lm_obs;

typedef struct hs_lm_entry_params {
    float max_dist_factor;             /* max_dist_invariance_factor (2.0f, MapPointDB.h:99)                              */
    float min_dist_factor;             /* min_dist_invariance_factor (0.5f, MapPointDB.h:100)                             */
} hs_lm_entry_params;

/* out_flags bits: which outputs the reference sets for that landmark */
#define HS_LM_SET_NORMAL_DEPTH 1       /* normal, min_dist, max_dist: N > 0 (:241-242)                                    */
#define HS_LM_SET_DESC         2       /* best / median >= 0: the descriptor set is not empty (:139-141)                  */
#define HS_LM_SET_MEAN         4       /* mean distance: N > 0 (:275-276)                                                 */
#define HS_LM_SET_SIZE         8       /* size: always (:291-310 does not return early; 0.0f / 0.0f = NaN without a positive size) */

/* Landmark i has N_i = obs_offsets[i+1] - obs_offsets[i] observations obs[obs_offsets[i] ..) and, separately, the descriptor set
 * desc[desc_offsets[i] ..)[32] of hs_landmark_best_descriptors (isBad() key frames left out, :131-135 — the observation loops keep them).
 * Both CSRs: non-decreasing, offsets[0] >= 0, checked here.  Per landmark:
 *   out_normal[i][3], out_min_dist[i], out_max_dist[i], out_mean_dist[i]   written only when N_i > 0 (left unchanged otherwise, as the reference)
 *   out_size[i]                                                            always written (NaN when no observation has a positive size)
 *   out_best[i], out_median[i]                                             as hs_landmark_best_descriptors (-1 / -1 for an empty descriptor set)
 *   out_flags[i]                                                           HS_LM_SET_* bits
 * Host pointers; synchronous. */
int  hs_landmark_update_entries(hs_orb* h, const hs_lm_entry_params* params, int L, const hs_lm_entry_in* entries,
                                const int64_t* obs_offsets, const hs_lm_obs* obs, const int64_t* desc_offsets, const uint8_t* desc,
                                float* out_normal, float* out_min_dist, float* out_max_dist, float* out_mean_dist, float* out_size,
                                int32_t* out_best, int32_t* out_median, int32_t* out_flags);
/* The same on device pointers (offsets 8-byte aligned, d_desc 16-byte aligned, d_obs / d_entries 4-byte aligned; the offsets are not checked on
 * the host), enqueued on `stream` (NULL = the handle's own stream) without synchronising.  Every output array is required and written as above.
 * Scatter (optional, both or neither): for each i with 0 <= d_lm_index[i] < n_lms, record d_lms[d_lm_index[i]] receives normal, min_dist and
 * max_dist when N_i > 0, size always, and desc = the chosen descriptor's 32 bytes when the descriptor set is not empty; pos, assoc_kp,
 * prev_angle and skip are never written, nor is any record no index names.  Indices must be distinct.  The handle's one-stream-at-a-time rule
 * applies (see hs_orb_extract_batch_device).  Asynchronous. */
int  hs_landmark_update_entries_device(hs_orb* h, const hs_lm_entry_params* params, int L, const hs_lm_entry_in* d_entries,
                                       const int64_t* d_obs_offsets, const hs_lm_obs* d_obs, const int64_t* d_desc_offsets, const uint8_t* d_desc,
                                       float* d_normal, float* d_min_dist, float* d_max_dist, float* d_mean_dist, float* d_size,
                                       int32_t* d_best, int32_t* d_median, int32_t* d_flags,
                                       hs_landmark* d_lms, const int32_t* d_lm_index, int n_lms, void* stream);

/* ---- key-frame graph: everything the reference answers by walking "which key frames see these landmarks?" — CovisNode::UpdateConnections
 * (src/core/CovisibilityGraph.cpp:42-124), TrackLocalMap::UpdateLocalKeyFrames (src/slam/tracking/TrackLocalMap.cpp:80-123) and KeyFrameCuller::run
 * (src/slam/mapping/KeyFrameCuller.cpp:21-93) — over ONE observation table, for a batch.  Integer arithmetic only: every output is identical to the
 * reference's, not merely close.
 * Containers the reference orders by KeyFrame* address become ARRAY ORDER: key frames are numbered by slot 0 .. n_kf-1, passed in
 * ascending address order.  The table (host pointers for the host forms, device pointers for the `_device` forms; the struct itself is host memory):
 *   lm_obs_offsets [L+1] int64   CSR over the landmarks' observations: non-decreasing, [0] >= 0 (the host forms check: HS_ERR_INVALID)
 *   lm_obs_kf      []    int32   slot of each observation, ascending within a landmark (the order of its std::map<KeyFrame*, size_t>)
 *   lm_obs_octave  []    int32   views.keypt(idx).octave of that observation          (hs_kf_redundancy only; hs_kf_votes ignores it)
 *   lm_bad         [L]   u8      MapPoint::isBad()
 *   lm_nobs        [L]   int32   MapPoint::Observations() — counts a stereo observation twice, so it is NOT the CSR length (hs_kf_redundancy only)
 *   kf_bad         [n_kf] u8     KeyFrame::isBad()                                    (hs_kf_votes only)
 *   kf_id          [n_kf] int64  KeyFrame::mnId                                       (hs_kf_votes only)
 * The host forms also refuse a landmark index or slot outside the table (HS_ERR_INVALID, no output touched); the device forms check nothing, their
 * kernels skip such an entry. */
typedef struct hs_kf_table {
    int32_t L, n_kf;
    const int64_t* lm_obs_offsets;
    const int32_t* lm_obs_kf;
    const int32_t* lm_obs_octave;
    const uint8_t* lm_bad;
    const int32_t* lm_nobs;
    const uint8_t* kf_bad;
    const int64_t* kf_id;
} hs_kf_table;

/* hs_kf_votes keeps a query's counters in LDS while n_kf <= HS_KF_LDS_SLOTS; beyond it they are a row of global memory updated with device atomics
 * (integer adds: both paths are exact).  An ordered list of up to HS_KF_SORT_PASS entries is sorted from LDS in one pass; a longer one is ranked
 * straight from the counters: correct for any length up to n_kf, at n_ordered * n_kf counter reads per query (with all of 12 288 key frames
 * listed about 12 ms on an MI355X, with 12 289 about 23 ms; profiles/README.md). */
#define HS_KF_LDS_SLOTS 12288
#define HS_KF_SORT_PASS 1024

/* The counter of UpdateConnections / UpdateLocalKeyFrames and what the reference derives from it, for Q queries.  Query q votes with the landmarks
 * q_lm[q_offsets[q] .. q_offsets[q+1]) (a CSR like the table's; pKF->GetMapPoints() for covisibility, the frame's matched landmarks for the local
 * map; a landmark listed twice counts twice — a std::set caller never lists one twice).  A bad landmark contributes nothing (:55,
 * TrackLocalMap.cpp:88).  q_self_id [Q] (may be NULL = none): observations by a key frame whose kf_id equals it are not counted (:63 compares mnId,
 * not the address, so EVERY slot carrying that id is left out); -1 excludes none.  count_bad_kf = 0 is covisibility (:65-68): a bad key frame is
 * not counted and never appears.  count_bad_kf = 1 is UpdateLocalKeyFrames: a bad key frame is counted into `weights`, but skipped when the maximum
 * is chosen (TrackLocalMap.cpp:113) and left out of the ordered list.  th: the connection threshold (15, :82).  Per query:
 *   weights [Q][n_kf] int32 (may be NULL)   the counter, 0 = not in the map: mConnectedKeyFrameWeights.  For local_key_frames the caller tests
 *                                           `> 0` AND !isBad(): with count_bad_kf = 1 a bad key frame carries its count here, and the reference skips it
 *                                           before local_key_frames.insert (TrackLocalMap.cpp:113-122)
 *   max_slot [Q], max_count [Q]             pKFmax / nmax of `if (count > nmax)` on the walk over ascending slots: the LOWEST slot among equal
 *                                           maxima; -1 / 0 when nothing (that is not bad) was counted — the reference returns without touching the node
 *   ordered_slot [Q][cap], ordered_weight [Q][cap], n_ordered [Q]
 *                                           the entries with count >= th or, when there is none, the single (nmax, pKFmax) entry (:100-104), in the
 *                                           order of sort(vPairs) + push_front (:106-113): descending weight and, among equal weights, DESCENDING
 *                                           slot.  n_ordered always holds the full length; the first min(n_ordered, cap) entries are written and the
 *                                           rest of the row is filled with -1 / 0.  Truncation is not an error: GetBestCovisibilityKeyFrames(N) is the
 *                                           first N entries, and with cap = 10 a row is a `neigh` row of hs_place_query_*.  cap = 0: no list wanted.
 * The symmetric_updates of :96,103 — what the CovisGraph applies to the OTHER nodes — are exactly the ordered entries (slot, weight).
 * hs_kf_votes: host pointers, staged through the handle's scratch, synchronous.  hs_kf_votes_device: `T` holds device pointers, every array is in HBM
 * of the handle's device, enqueued on `stream` (NULL = the handle's own) without synchronising, nothing checked; beyond HS_KF_LDS_SLOTS key frames
 * the d_weights rows ARE the counters and d_weights must not be NULL.  The handle's one-stream-at-a-time rule applies (see
 * hs_orb_extract_batch_device). */
int  hs_kf_votes(hs_orb* h, const hs_kf_table* T, int Q, const int64_t* q_offsets, const int32_t* q_lm, const int64_t* q_self_id,
                 int count_bad_kf, int th, int32_t* weights, int32_t* max_slot, int32_t* max_count,
                 int32_t* ordered_slot, int32_t* ordered_weight, int cap, int32_t* n_ordered);
int  hs_kf_votes_device(hs_orb* h, const hs_kf_table* T, int Q, const int64_t* d_q_offsets, const int32_t* d_q_lm, const int64_t* d_q_self_id,
                        int count_bad_kf, int th, int32_t* d_weights, int32_t* d_max_slot, int32_t* d_max_count,
                        int32_t* d_ordered_slot, int32_t* d_ordered_weight, int cap, int32_t* d_n_ordered, void* stream);

/* KeyFrameCuller::run's verdict (:33-86) for C candidate key frames, each against the SAME snapshot of the map.  Candidate c is the key frame in
 * slot cand_slot[c] with mThDepth cand_th_depth[c]; its keypoints that hold a landmark are the items [cand_offsets[c] .. cand_offsets[c+1]):
 * item_lm (landmark index), item_octave (KFviews.keypt(i).octave), item_depth (KFviews.depth(i); read only when is_mono = 0).  Per item, as :39-81:
 * a bad landmark is skipped; when not mono an item with depth > th_depth || depth < 0 is skipped; nMPs counts the rest; when lm_nobs > th_obs the
 * landmark's observations with slot != cand_slot and octave <= item octave + 1 are counted, and the landmark is redundant when they reach th_obs
 * (the reference's early `break` changes nothing).  n_mps [C], n_redundant [C], cull [C] u8 = n_redundant > frac_redundant * n_mps evaluated as C++
 * does (:86): the int converted to float, one float product.  th_obs = 3 and frac_redundant = 0.9f are KeyFrameCullerParameters' defaults.
 * The call is a PURE FUNCTION OF THE SNAPSHOT.  The sequential part of the reference is not in it: SetBadKeyFrame on a culled candidate erases its
 * observations, can turn landmarks bad (MapPointDB.cpp:39-75) and may be refused (Map.cc:153-159), all of which changes the verdict of the candidates
 * after it.  The caller culls the first candidate with cull = 1, regathers the table and asks again for the candidates behind it
 * (hyslam_amd/host/HipKeyFrameGraph.h does).  Host / device forms as hs_kf_votes. */
int  hs_kf_redundancy(hs_orb* h, const hs_kf_table* T, int C, const int32_t* cand_slot, const float* cand_th_depth, const int64_t* cand_offsets,
                      const int32_t* item_lm, const int32_t* item_octave, const float* item_depth, int is_mono, int th_obs, float frac_redundant,
                      int32_t* n_mps, int32_t* n_redundant, uint8_t* cull);
int  hs_kf_redundancy_device(hs_orb* h, const hs_kf_table* T, int C, const int32_t* d_cand_slot, const float* d_cand_th_depth,
                             const int64_t* d_cand_offsets, const int32_t* d_item_lm, const int32_t* d_item_octave, const float* d_item_depth,
                             int is_mono, int th_obs, float frac_redundant, int32_t* d_n_mps, int32_t* d_n_redundant, uint8_t* d_cull, void* stream);

/* ---- the local map: what TrackLocalMap::track (src/slam/tracking/TrackLocalMap.cpp) does between the vote (hs_kf_votes, count_bad_kf = 1) and the
 * projection search (hs_search_by_projection): the key-frame expansion of UpdateLocalKeyFrames (:126-156), the landmark selection of
 * UpdateLocalPoints (:166-184) with the filter at the head of SearchLocalPoints (:55-67), and the gather of the selected hs_landmark records.  Over
 * the same hs_kf_table, in ARRAY ORDER: key frames are slots 0 .. n_kf-1 and landmarks indices 0 .. L-1, both in ascending
 * address.  Integer and index work: every output is identical to the reference's.  Each stage has a host form (host pointers, staged through the
 * handle's scratch, synchronous, arguments checked: HS_ERR_INVALID, no output touched) and a `_device` form (device pointers, enqueued on `stream`
 * (NULL = the handle's own) without synchronising, nothing checked; its kernels skip a slot or index outside the table).  The `_device` forms take
 * their temporaries from the caller (`d_work`), not from the handle, so a chain of them never waits for the host.  The handle's
 * one-stream-at-a-time rule applies (see hs_orb_extract_batch_device). */

/* The expansion (:106-156).  weights [n_kf]: a row of hs_kf_votes with count_bad_kf = 1;  kf_bad [n_kf];  neigh [n_kf][neigh_cap]: each slot's
 * ordered covisibility list = Map::getBestCovisibilityKeyFrames, i.e. the ordered rows of hs_kf_votes, padded with -1;  parent [n_kf]: GetParent(),
 * -1 = none.  n_max_local_keyframes, n_neighbor_keyframes: TrackLocalMapParameters (80, 10).  The host form refuses n_neighbor_keyframes > neigh_cap
 * or < 0, and a neigh / parent entry outside [-1, n_kf).  local [n_kf] u8, n_local [1]: the set and its size.  Literally as the reference:
 *   the set starts as weights > 0 && !kf_bad (:109-123);
 *   the reference iterates the std::set while inserting into it: the live set is walked in ascending slot order, a slot inserted above the cursor is
 *   visited later, one inserted below it never;
 *   at each visited slot: stop if the size of the set is > n_max (strict, the current size; the int is converted to size_t as C++ does, so a
 *   negative n_max never stops the walk) (:130); among the first n_neighbor entries of the slot's row insert the first that is not bad and look no
 *   further in that row (:139-147); if the slot has a parent insert it — bad or not — and END THE WHOLE WALK (the `break` at :153 leaves the
 *   outer loop);
 *   nothing counted: the set stays empty.
 * One wave; the next member is found with a ballot over 64-slot words. */
int  hs_local_keyframes(hs_orb* h, int n_kf, const int32_t* weights, const uint8_t* kf_bad, const int32_t* neigh, int neigh_cap, const int32_t* parent,
                        int n_max_local_keyframes, int n_neighbor_keyframes, uint8_t* local, int32_t* n_local);
int  hs_local_keyframes_device(hs_orb* h, int n_kf, const int32_t* d_weights, const uint8_t* d_kf_bad, const int32_t* d_neigh, int neigh_cap,
                               const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, uint8_t* d_local, int32_t* d_n_local,
                               void* stream);

/* The landmarks of the local map (:166-184 and :55-67).  Of the table only lm_obs_offsets, lm_obs_kf and lm_bad are read.  local [n_kf]: the set of
 * hs_local_keyframes.  frame_lm [n_assoc]: the frame's associations (getLandMarkMatches()) as landmark indices, -1 = a null entry.
 *   frame_remove [n_assoc] u8   1 where the associated landmark is bad: the caller calls removeLandMarkAssociation on it (:62)
 *   sel [cap] int32, n_sel [1]  in ASCENDING landmark index every landmark that is not bad, has at least one observation by a local key frame, and
 *                               is not held by the frame through an association that is not bad (the erase at :65).  n_sel always holds the full
 *                               count; the first min(n_sel, cap) indices are written and the rest of sel is -1.  Truncation is not an error.
 * A landmark with an empty observation range is never selected.  The reference collects KeyFrame::GetMapPointMatches() of the local key frames; the
 * table lists the MapPoints' observations.  The two are the same relation as long as associations are symmetric (a key frame holds a landmark
 * exactly when the landmark lists that key frame as an observer), which Map's association calls maintain.
 * The compaction is deterministic: counts per block of HS_LOCAL_POINTS_BLOCK landmarks, a scan, a scatter; no atomic counter decides a position.
 * d_work: hs_local_points_work_bytes(L) bytes of device memory, 16-byte aligned, contents irrelevant before and after. */
#define HS_LOCAL_POINTS_BLOCK 1024
size_t hs_local_points_work_bytes(int L);
int  hs_local_points(hs_orb* h, const hs_kf_table* T, const uint8_t* local, const int32_t* frame_lm, int n_assoc, uint8_t* frame_remove,
                     int32_t* sel, int cap, int32_t* n_sel);
int  hs_local_points_device(hs_orb* h, const hs_kf_table* T, const uint8_t* d_local, const int32_t* d_frame_lm, int n_assoc, uint8_t* d_frame_remove,
                            int32_t* d_sel, int cap, int32_t* d_n_sel, void* d_work, void* stream);

/* d_out[j] = d_lms[d_sel[j]] for j < min(*d_n_sel, cap), with assoc_kp = -1 (no selected landmark is held by the frame) and skip = 0.  The records
 * j in [*d_n_sel, cap) — and one whose index is outside [0, L) — are all zero but for assoc_kp = -1 and skip = 1, so hs_search_by_projection_device
 * can be enqueued with L = cap and the host never needs to know n_sel, which is read from device memory.  Exactly cap records are written.  d_lms and
 * d_out are 16-byte aligned (hipMalloc's are): a record moves as five 16-byte loads and stores.  No host form: the gather has no reference semantics
 * of its own. */
int  hs_landmark_gather_device(hs_orb* h, const hs_landmark* d_lms, int L, const int32_t* d_sel, const int32_t* d_n_sel, int cap, hs_landmark* d_out,
                               void* stream);

/* UpdateLocalMap + SearchLocalPoints in one call: hs_kf_votes_device (one query = frame_lm, count_bad_kf = 1), hs_local_keyframes_device,
 * hs_local_points_device, hs_landmark_gather_device and hs_search_by_projection_device with L = cap, enqueued on one stream, no synchronisation in
 * between; the result equals making those five calls one after another (it IS those five calls).  T: the map's table;  d_lms [T->L]: its resident
 * hs_landmark records (hs_landmark_update_entries_device keeps them current);  F, pp: as hs_search_by_projection_device.  cap >= 1.
 * Every pointer of `out` is device memory and required: */
typedef struct hs_local_map_out {
    int32_t* weights;              /* [n_kf]   keyframeCounter, the bad key frames included                                  */
    int32_t* max_slot;             /* [1]      pKFmax (the reference key frame), -1 = none                                   */
    int32_t* max_count;            /* [1]                                                                                    */
    uint8_t* local;                /* [n_kf]   local_key_frames                                                              */
    int32_t* n_local;              /* [1]                                                                                    */
    uint8_t* frame_remove;         /* [n_assoc]                                                                              */
    int32_t* sel;                  /* [cap]    local_map_points as landmark indices, ascending; -1 past n_sel                */
    int32_t* n_sel;                /* [1]      the full count (may exceed cap)                                               */
    hs_landmark* lms;              /* [cap]    the gathered records, 16-byte aligned                                         */
    int32_t* match_idx;            /* [cap]    keypoint matched by landmark sel[j], or -1                                    */
    float*   match_dist;           /* [cap]                                                                                  */
    int32_t* n_matches;            /* [1]                                                                                    */
} hs_local_map_out;
size_t hs_local_map_work_bytes(int L);
int  hs_local_map_search_device(hs_orb* h, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap,
                                const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F,
                                const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out, void* d_work, void* stream);

/* ================= pose-only optimisation: Optimizer::PoseOptimization (src/optimizers/Optimizer.cc:48-279) =================
 * One 6-DoF vertex (the frame's pose), one unary reprojection edge per keypoint that holds a landmark, Huber kernels, g2o's Levenberg-Marquardt
 * (at most 10 iterations of at most 10 trials) in four rounds; after every round each edge is classified against chi2 5.991 (mono) / 7.815 (stereo),
 * the next round optimises the inliers only and starts again from the INPUT pose, and the kernels come off after the third round.  DESIGN.md 5.11
 * lists the behaviour item by item.  A call takes Q independent problems (the cameras of a rig, the candidates of a relocalisation): one launch, one
 * workgroup per problem.  fp64 but for what the reference computes in float; no floating-point atomics: the same call gives the same bytes.
 *
 * hs_pose_edge: what Optimizer.cc:105-187 reads for keypoint `kp`.  ur < 0 makes the monocular edge, anything else (NaN included) the stereo edge.
 * Arrays of edges are 16-byte aligned (hipMalloc's are; the host form stages them). */
typedef struct hs_pose_edge {
    float Xw[3];                       /* pMP->GetWorldPos()                                            */
    float u, v, ur;                    /* kpUn.pt.x, kpUn.pt.y, views.uR(i)                             */
    float inv_sigma2;                  /* 1 / orbParams().determineSigma2(kpUn.size), computed in float */
    int32_t kp;                        /* the keypoint index i; carried, not read                       */
} hs_pose_edge;                        /* 32 bytes */
typedef struct hs_pose_problem {
    float Tcw[16];                     /* pFrame->mTcw, row-major 4x4                                   */
    float fx, fy, cx, cy, bf;          /* Camera::fx() .. cy(), Camera::mbf                             */
} hs_pose_problem;
#define HS_POSE_OK 0                   /* hs_pose_result::status: optimised                                                        */
#define HS_POSE_TOO_FEW 1              /* fewer than 3 edges: nothing ran (the reference returns 0 and leaves pose and flags alone) */
#define HS_POSE_NONFINITE 2            /* optimised, and the resulting pose holds a NaN or an infinity                              */
typedef struct hs_pose_result {
    double Tcw_d[16];                  /* SE3Quat::to_homogeneous_matrix() of the estimate, row-major                  */
    float  Tcw[16];                    /* the same converted to float: what Converter::toCvMat hands to SetPose        */
    int32_t n_edges;                   /* nInitialCorrespondences                                                     */
    int32_t n_good;                    /* the return value: nInitialCorrespondences - nBad of the last round run       */
    int32_t rounds;                    /* rounds run: 4, or 1 with fewer than 10 edges, or 0                           */
    int32_t lm_iterations, lm_trials;  /* calls of OptimizationAlgorithmLevenberg::solve / passes of its trial loop    */
    int32_t status;                    /* HS_POSE_*                                                                    */
} hs_pose_result;
/* Problem q owns edges [edge_offsets[q], edge_offsets[q + 1]) and the same range of `outlier` (u8, 1 = outlier: what the reference passes to
 * pFrame->setOutlier(kp, ...)).  outlier is written for every edge of a problem that ran and NOT TOUCHED for a problem with fewer than 3 edges; for
 * such a problem status = HS_POSE_TOO_FEW, n_good = 0 and Tcw / Tcw_d carry the input pose (Tcw_d its floats widened), so the next search of a chain
 * can always read results[q].Tcw:  Rcw = its upper-left 3x3, tcw = its last column, Ow = -Rcw^T tcw (Frame::UpdatePoseMatrices).
 * Host form: host pointers, synchronous; edge_offsets must be non-negative and non-decreasing, else HS_ERR_INVALID and no output is touched. */
int  hs_pose_optimize(hs_orb* h, int Q, const hs_pose_problem* problems, const int64_t* edge_offsets, const hs_pose_edge* edges, uint8_t* outlier,
                      hs_pose_result* results);
/* Device pointers, enqueued on `stream` (NULL = the handle's own); nothing that lives on the device is checked (the arguments themselves are: NULL
 * problems / results, both or neither of the two count sources, d_n_edges with Q != 1, a misaligned d_edges give HS_ERR_INVALID), nothing synchronises.  Exactly one of d_edge_offsets
 * [Q + 1] and d_n_edges [1] is non-NULL; d_n_edges needs Q == 1 and makes the problem's edges d_edges[0, min(*d_n_edges, edge_cap)) — the count
 * hs_pose_edges_device left on the device, so the host never needs it (edge_cap is not read with d_edge_offsets).  d_work: hs_pose_work_bytes(Q,
 * n_edges_total) bytes, which is 0 today: both kernels keep their temporaries in registers and LDS, and d_work may then be NULL.  The parameter is
 * there so that a chain never waits for the handle's scratch, whatever a later version needs. */
size_t hs_pose_work_bytes(int Q, int64_t n_edges_total);
int  hs_pose_optimize_device(hs_orb* h, int Q, const hs_pose_problem* d_problems, const int64_t* d_edge_offsets, const int32_t* d_n_edges, int edge_cap,
                             const hs_pose_edge* d_edges, uint8_t* d_outlier, hs_pose_result* d_results, void* d_work, void* stream);
/* The loop at Optimizer.cc:94-188 on resident data: for every keypoint i of F (device pointers; kps, uR and n, size_ref are read; uR == NULL: all
 * monocular) with 0 <= d_kp_lm[i] < L, in ASCENDING i, one edge: Xw = d_lms[d_kp_lm[i]].pos, u, v = kps[i].x, .y, ur = uR[i], inv_sigma2 =
 * 1 / (sigma_ref * (kps[i].size / F->size_ref)^2) in float, kp = i.  The compaction is deterministic (one workgroup: a scan per chunk of 1024
 * keypoints and a running base; no atomic counter decides a position).  d_n_edges [1] receives the full count; only the first min(count, cap)
 * edges are written and truncation is not an error.  d_work as above. */
int  hs_pose_edges_device(hs_orb* h, const hs_frame_view* F, const hs_landmark* d_lms, int L, const int32_t* d_kp_lm, float sigma_ref,
                          hs_pose_edge* d_edges, int cap, int32_t* d_n_edges, void* d_work, void* stream);

/* ================= relocalisation: PnPsolver, EPnP inside RANSAC (src/estimators/PnPsolver.cc) =================
 * A call takes Q independent problems (the candidate key frames of TrackPlaceRecognition::track) and runs, for each, what PnPsolver::iterate(n)
 * runs: every hypothesis of the call at once (one wave each: EPnP on min_set sampled correspondences, then the inlier count over all N), then, one
 * workgroup per problem, the walk over the counts in order with Refine() on every new best set until one refines.  DESIGN.md 5.18 lists the
 * behaviour item by item.  fp64 but for what the reference narrows to float; no floating-point atomics: the same call gives the same bytes.
 * Two stated deviations from the reference:
 *   - every decomposition (the PCA 3x3, the inverse 3x3, MtM 12x12, the 6x4 / 6x3 / 6x5 least squares, ABt 3x3) is ONE routine: a one-sided cyclic
 *     Jacobi SVD in double, pairs (p, q) in the order p = 0 .. n-2, q = p+1 .. n-1, at most 30 sweeps, the rotation from sqrt and division only, a
 *     pair skipped when |<p,q>| <= DBL_EPSILON sqrt(<p,p><q,q>) or when a column's squared norm is <= (n DBL_EPSILON)^2 ||A||_F^2, singular values sorted
 *     descending by a stable sort; the symmetric uses (PCA, MtM) take the RIGHT singular vectors, which are defined for sigma = 0 too; the
 *     pseudo-inverse drops singular values <= 2 DBL_EPSILON (sum of sigma); a PCA axis is oriented so that its component of largest magnitude is
 *     positive (EPnP's answer depends on the control points' signs under pixel noise);
 *   - draw k of absolute iteration `it` is r = mix(0x9E3779B97F4A7C15 * (seed + it * min_set + k + 1)), mix being SplitMix64's finaliser (element
 *     seed + it * min_set + k of hyslam_amd.synth.splitmix64(0, .)), and randi = (hi32(r) * avail) >> 32.  A table draws[q][it][k] (uint32, stride
 *     HS_PNP_MAX_SET per iteration, draw_cap iterations per problem; same reduction with the entry in place of hi32(r)) overrides it for it < draw_cap. */
/* largest min_set a call accepts, and the stride of a draws row */
#define HS_PNP_MAX_SET 16
typedef struct hs_pnp_corr {
    float Xw[3];                       /* pMP->GetWorldPos()                                                          */
    float u, v;                        /* kp.pt                                                                       */
    float sigma2;                      /* orbParams().determineSigma2(kp.size), in float: 1 / hs_pose_edge::inv_sigma2 */
    int32_t kp;                        /* the keypoint index i; carried, not read                                     */
    int32_t _pad;
} hs_pnp_corr;                         /* 32 bytes; arrays are 16-byte aligned */
typedef struct hs_pnp_params {
    double probability;                /* SetRansacParameters' arguments (Tracking_datastructs.cc:53-58: 0.99, 10, 300, 4, 0.5, 5.991) */
    int32_t min_inliers, max_iterations, min_set;
    float epsilon, th2;
    float fx, fy, cx, cy;              /* Camera::fx() .. cy()                                                        */
    int32_t _pad;
    uint64_t seed;                     /* replaces the process-wide rand() stream                                     */
} hs_pnp_params;                       /* 56 bytes */
typedef struct hs_pnp_plan_t {         /* (hs_pnp_plan is the function: C has one name space for both)                */
    int32_t min_inliers;               /* mRansacMinInliers after SetRansacParameters                                 */
    float epsilon;                     /* mRansacEpsilon                                                              */
    int32_t max_iterations;            /* mRansacMaxIts                                                               */
    int32_t _pad;
} hs_pnp_plan_t;
typedef struct hs_pnp_state {          /* what persists between two calls of iterate; the best mask is a u8 [N] array of the caller's */
    int32_t iterations;                /* mnIterations                                                                */
    int32_t best_inliers;              /* mnBestInliers                                                               */
    float best_Tcw[16];                /* mBestTcw, row-major 4x4                                                     */
} hs_pnp_state;                        /* 72 bytes */
#define HS_PNP_TOO_FEW 0               /* N below the effective min_inliers: nothing ran (bNoMore true, no pose)      */
#define HS_PNP_REFINED 1               /* Refine() succeeded: its pose and inliers, bNoMore false                     */
#define HS_PNP_BEST 2                  /* the loop ran out: the best hypothesis' pose and inliers, bNoMore true       */
#define HS_PNP_NONE 3                  /* the loop ran out with no best: bNoMore true, no pose                        */
#define HS_PNP_NONFINITE 4             /* a pose would be returned and holds a NaN or an infinity                     */
/* HS_PNP_NONFINITE hands out no usable pose: the Python and C++ mirrors give it as "no pose, bNoMore true" also where it replaces HS_PNP_REFINED
 * (the reference would hand the non-finite matrix back with bNoMore false); hs_pnp_result::at_iteration > 0 tells that case apart. */
typedef struct hs_pnp_result {
    double Tcw_d[16];                  /* R and t before the narrowing, row-major 4x4 (for a best carried over from an earlier call: its floats widened) */
    float  Tcw[16];                    /* what iterate returns                                                        */
    int32_t status;                    /* HS_PNP_*                                                                    */
    int32_t n_inliers;                 /* nInliers                                                                    */
    int32_t at_iteration;              /* mnIterations at the return out of the loop (REFINED), else 0                */
    int32_t iterations;                /* mnIterations after the call                                                 */
    int32_t hypotheses_run;            /* hypotheses the call evaluated (all of its range, also past an early return)  */
    int32_t refines_run;               /* evaluations of Refine(): one per distinct best set                          */
} hs_pnp_result;                       /* 216 bytes */
/* SetRansacParameters (:127-163) for N correspondences: pure host arithmetic (glibc's log and pow).  HS_ERR_INVALID for NULL, N < 0, min_set < 4. */
int  hs_pnp_plan(int N, const hs_pnp_params* params, hs_pnp_plan_t* plan);
void hs_pnp_state_init(hs_pnp_state* state);     /* iterations = best_inliers = 0, best_Tcw = 0 */
/* bytes of d_work for a call of Q problems over n_corr_total correspondences that runs at most max_hypotheses hypotheses per problem:
 * max_hypotheses >= max(n_iterations, every problem's planned max_iterations); max(n_iterations, the largest params.max_iterations) always serves. */
size_t hs_pnp_work_bytes(int Q, int64_t n_corr_total, int max_hypotheses);
/* PnPsolver::iterate(n_iterations) for Q problems.  Problem q owns corrs [corr_offsets[q], corr_offsets[q + 1]) and the same range of best_masks
 * (state, read and written) and inlier_masks (output, u8, 1 = inlier; NOT TOUCHED for HS_PNP_TOO_FEW and HS_PNP_NONE).  draws may be NULL with
 * draw_cap = 0.  Host form: host pointers, synchronous, staged through the handle's scratch.  HS_ERR_INVALID, nothing enqueued and no output touched:
 * NULL pointers, Q < 1, min_set outside [4, HS_PNP_MAX_SET], negative or decreasing offsets, n_iterations < 1, a state with a negative count (a
 * state starts from hs_pnp_state_init; the device form cannot see it and reads a negative `iterations` as 0). */
int  hs_pnp_iterate(hs_orb* h, int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* corrs, int n_iterations,
                    const uint32_t* draws, int draw_cap, hs_pnp_state* states, uint8_t* best_masks, hs_pnp_result* results, uint8_t* inlier_masks);
/* The same with device pointers, enqueued on `stream` (NULL = the handle's own), nothing synchronises; params and corr_offsets stay host arrays
 * (the plan is host arithmetic) and are read before the call returns.  d_work: hs_pnp_work_bytes bytes, 16-byte aligned. */
int  hs_pnp_iterate_device(hs_orb* h, int Q, const hs_pnp_params* params, const int64_t* corr_offsets, const hs_pnp_corr* d_corrs, int n_iterations,
                           const uint32_t* d_draws, int draw_cap, hs_pnp_state* d_states, uint8_t* d_best_masks, hs_pnp_result* d_results,
                           uint8_t* d_inlier_masks, void* d_work, void* stream);

/* ================= loop closing: Sim3Solver, Horn's closed form inside RANSAC (src/estimators/Sim3Solver.cc) =================
 * A call takes Q independent problems (the consistent candidates of LoopClosing::ComputeSim3) and runs, for each, what Sim3Solver::iterate(n) runs:
 * every hypothesis of the call at once (one LANE each: three sampled correspondences, Horn's closed form, the inlier count over all N in both
 * directions), then, one wave per problem, the walk over the counts in order.  DESIGN.md 5.19 lists the behaviour item by item.  No atomics and no
 * sum shared between lanes: the same call gives the same bytes.  Two stated rules for what cannot be reproduced:
 *   - DESIGN.md D19 defines what OpenCV does inside ComputeSim3: every matrix-product entry accumulated in double in index order and narrowed once,
 *     the eigenvector by a cyclic Jacobi in double (HS_SIM3_EIG_SWEEPS sweeps, + - x / sqrt only), R directly from the quaternion;
 *   - draws follow D18 with a set of 3: draw k of absolute iteration `it` is element seed + 3 it + k of the SplitMix64 sequence, randi =
 *     (hi32(r) * avail) >> 32.  A table draws[q][it][k] (uint32, HS_SIM3_DRAW_STRIDE words per iteration, draw_cap iterations per problem)
 *     overrides it for it < draw_cap. */
#define HS_SIM3_DRAW_STRIDE 4
#define HS_SIM3_EIG_SWEEPS 10
typedef struct hs_sim3_corr {
    float X1c[3];                      /* Rcw1 * pMP1->GetWorldPos() + tcw1, formed by the caller (:98-99)            */
    float sigma2_1;                    /* orb_params_KF1.determineSigma2(kp1.size)                                    */
    float X2c[3];                      /* Rcw2 * pMP2->GetWorldPos() + tcw2 (:101-102)                                */
    float sigma2_2;
    int32_t idx1;                      /* mvnIndices1: i1; carried, not read                                          */
    int32_t _pad[3];
} hs_sim3_corr;                        /* 48 bytes; arrays are 16-byte aligned */
typedef struct hs_sim3_params {
    double probability;                /* SetRansacParameters' arguments (LoopClosing.cc: 0.99, 20, 300)              */
    int32_t min_inliers, max_iterations;
    int32_t fix_scale;                 /* mbFixScale: ms12i = 1.0f                                                    */
    int32_t _pad;
    float fx1, fy1, cx1, cy1;          /* mK1                                                                         */
    float fx2, fy2, cx2, cy2;          /* mK2                                                                         */
    uint64_t seed;                     /* replaces the process-wide generator                                         */
} hs_sim3_params;                      /* 64 bytes */
typedef struct hs_sim3_plan_t {        /* (hs_sim3_plan is the function)                                              */
    int32_t max_iterations;            /* mRansacMaxIts after SetRansacParameters                                     */
    float epsilon;                     /* (float)minInliers / N                                                       */
} hs_sim3_plan_t;
typedef struct hs_sim3_state {         /* what persists between two calls of iterate; the best mask is a u8 [N] array of the caller's */
    int32_t iterations;                /* mnIterations                                                                */
    int32_t best_inliers;              /* mnBestInliers                                                               */
    float R[9], t[3], s;               /* mBestRotation, mBestTranslation, mBestScale                                 */
    float T12[16];                     /* mBestT12, row-major 4x4                                                     */
    int32_t _pad;
} hs_sim3_state;                       /* 128 bytes */
#define HS_SIM3_TOO_FEW 0              /* N below min_inliers, or below 3: nothing ran (bNoMore true, no pose)        */
#define HS_SIM3_FOUND 1                /* a hypothesis with more than min_inliers inliers: its pose, bNoMore false    */
#define HS_SIM3_CONTINUE 2             /* the call's iterations ran out, the plan's did not: no pose, bNoMore false   */
#define HS_SIM3_EXHAUSTED 3            /* mnIterations reached mRansacMaxIts: no pose, bNoMore true                   */
#define HS_SIM3_NONFINITE 4            /* HS_SIM3_FOUND whose pose holds a NaN or an infinity                         */
typedef struct hs_sim3_result {
    float T12[16];                     /* what iterate returns (zeros without a pose)                                 */
    float R[9], t[3], s;
    int32_t status;                    /* HS_SIM3_*                                                                   */
    int32_t n_inliers;                 /* nInliers (0 without a pose)                                                 */
    int32_t at_iteration;              /* mnIterations at the return out of the loop (FOUND), else 0                  */
    int32_t iterations;                /* mnIterations after the call                                                 */
    int32_t hypotheses_run;            /* hypotheses the call evaluated (all of its range, also past an early return)  */
} hs_sim3_result;                      /* 136 bytes */
/* SetRansacParameters (:118-142) for N correspondences: pure host arithmetic (glibc's log and pow).  HS_ERR_INVALID for NULL, N < 0. */
int  hs_sim3_plan(int N, const hs_sim3_params* params, hs_sim3_plan_t* plan);
void hs_sim3_state_init(hs_sim3_state* state);   /* everything 0 */
/* bytes of d_work for a call of Q problems over n_corr_total correspondences that runs at most max_hypotheses hypotheses per problem:
 * min(n_iterations, the largest params.max_iterations) always serves (the loop's AND). */
size_t hs_sim3_work_bytes(int Q, int64_t n_corr_total, int max_hypotheses);
/* Sim3Solver::iterate(n_iterations) for Q problems.  Problem q owns corrs [corr_offsets[q], corr_offsets[q + 1]) and the same range of best_masks
 * (state, read and written) and inlier_masks (output, u8, 1 = inlier by correspondence; ALWAYS written: all 0 but for HS_SIM3_FOUND / NONFINITE).
 * draws may be NULL with draw_cap = 0.  Host form: host pointers, synchronous, staged through the handle's scratch.  HS_ERR_INVALID, nothing enqueued
 * and no output touched: NULL pointers, Q < 1, n_iterations < 1, negative or decreasing offsets, a problem above 2^31 - 1 correspondences,
 * min_inliers < 0, a state with a negative count (host form only: the device form cannot see it and reads a negative count as 0). */
int  hs_sim3_iterate(hs_orb* h, int Q, const hs_sim3_params* params, const int64_t* corr_offsets, const hs_sim3_corr* corrs, int n_iterations,
                     const uint32_t* draws, int draw_cap, hs_sim3_state* states, uint8_t* best_masks, hs_sim3_result* results, uint8_t* inlier_masks);
/* The same with device pointers, enqueued on `stream` (NULL = the handle's own), nothing synchronises; params and corr_offsets stay host arrays
 * (the plan is host arithmetic) and are read before the call returns.  d_corrs and d_work (hs_sim3_work_bytes bytes) are 16-byte aligned. */
int  hs_sim3_iterate_device(hs_orb* h, int Q, const hs_sim3_params* params, const int64_t* corr_offsets, const hs_sim3_corr* d_corrs, int n_iterations,
                            const uint32_t* d_draws, int draw_cap, hs_sim3_state* d_states, uint8_t* d_best_masks, hs_sim3_result* d_results,
                            uint8_t* d_inlier_masks, void* d_work, void* stream);

/* ================= monocular initialisation: MonoEstimator, homography and fundamental RANSAC, then reconstruction =================
 * (src/initializers/MonoEstimator.cpp.)  A call takes Q independent problems (one per monocular camera) and runs, for each, what
 * MonoEstimator::Initialize runs: the compaction of matches12 into mvMatches12, Normalize of both frames, max_iterations homography and as many
 * fundamental hypotheses on the SAME 8-point sets, each scored over all N matches, the choice between the two models by RH = SH / (SH + SF), and
 * ReconstructH (8 motions) or ReconstructF (4 motions) with CheckRT over the model's inliers.  One call, no state between calls.  N is known only
 * on the device: nothing of a call depends on a host read.  DESIGN.md 5.21 lists the behaviour item by item.  No float atomics, every float sum is
 * one lane's in the reference's order: the same call gives the same bytes.  Three stated rules for what cannot be reproduced:
 *   - DESIGN.md D20 defines the linear algebra OpenCV does inside (SVDecomp, inv, determinant, norm): float operands widened, D17's Jacobi in
 *     double, one narrowing where the reference holds a float Mat; 3x3 products by D19;
 *   - DESIGN.md D21: no transcendental on the device.  The parallax is reported and compared as a COSINE, against the float nearest
 *     cos(min_parallax_deg * pi / 180), formed on the host;
 *   - draws follow D18 with a set of 8: draw k of iteration `it` is element seed + 8 it + k of the SplitMix64 sequence, randi =
 *     (hi32(r) * avail) >> 32, swap-with-back.  A table draws[q][it][k] (uint32, HS_MONOINIT_DRAW_STRIDE words per iteration, draw_cap iterations
 *     per problem) overrides it for it < draw_cap. */
#define HS_MONOINIT_DRAW_STRIDE 8
typedef struct hs_monoinit_params {
    float fx, fy, cx, cy;              /* mK                                                                          */
    float sigma;                       /* MonoEstimatorParams::sigma (1.0)                                            */
    int32_t max_iterations;            /* MaxIterations (200): hypotheses per model; 1 .. HS_MONOINIT_MAX_ITERATIONS   */
    int32_t min_triangulated;          /* minTriangulated (50)                                                        */
    float min_frac_triangulated;       /* minFracTriangulated (0.9f)                                                  */
    float min_parallax_deg;            /* the 1.0 Initialize passes to ReconstructH / ReconstructF; must be > 0       */
    int32_t _pad;
    uint64_t seed;                     /* replaces SeedRandOnce(0) + RandomInt                                        */
} hs_monoinit_params;                  /* 48 bytes */
#define HS_MONOINIT_MAX_ITERATIONS 65535
#define HS_MONOINIT_TOO_FEW 0          /* N < 8: nothing ran, every output zero                                       */
#define HS_MONOINIT_FAILED 1           /* Initialize returns false: R21, t21, p3d and triangulated are zero           */
#define HS_MONOINIT_OK_H 2             /* true, reconstructed from the homography                                     */
#define HS_MONOINIT_OK_F 3             /* true, reconstructed from the fundamental matrix                             */
#define HS_MONOINIT_NONFINITE 4        /* true, yet R21 or t21 holds a NaN or an infinity                             */
#define HS_MONOINIT_MODEL_NONE 0
#define HS_MONOINIT_MODEL_H 1
#define HS_MONOINIT_MODEL_F 2
typedef struct hs_monoinit_result {
    int32_t status;                    /* HS_MONOINIT_*                                                               */
    int32_t n_matches;                 /* N = mvMatches12.size()                                                      */
    int32_t model;                     /* HS_MONOINIT_MODEL_*: the one handed to reconstruction (NONE: TOO_FEW, or both scores 0) */
    int32_t best_solution;             /* the motion that decided (H: bestSolutionIdx; F: the first with maxGood), -1: none */
    int32_t best_it_h, best_it_f;      /* the iteration whose model won; -1: no hypothesis scored above 0             */
    int32_t n_triangulated;            /* true entries of `triangulated`                                              */
    int32_t _pad;
    float score_h, score_f, rh;        /* SH, SF, RH = SH / (SH + SF)                                                 */
    float cos_parallax;                /* the selected cosine of best_solution (1 where it has no good point or there is none) */
    float H21[9], F21[9];              /* the winning models, row-major (zeros where best_it is -1)                   */
    int32_t n_good[8];                 /* nGood of every motion (H: 8, F: the first 4)                                */
    float R21[9], t21[3];
} hs_monoinit_result;                  /* 200 bytes */
/* bytes of d_work for a call of Q problems whose frames 1 hold n1_total key points, with at most max_iterations hypotheses per model */
size_t hs_monoinit_work_bytes(int Q, int64_t n1_total, int max_iterations);
/* The predicate of both forms below: pure host code over the by-value arguments and the three host arrays (params, key_offsets1, key_offsets2);
 * the pointers are only compared with NULL and, for device != 0, with their alignment.  Returns NULL where the call would be accepted, else
 * the refusal's text: NULL pointers, Q < 1, negative or decreasing offsets, a frame above 2^31 - 1 key points, max_iterations outside
 * [1, HS_MONOINIT_MAX_ITERATIONS], sigma or a focal length that is not positive and finite, min_parallax_deg outside (0, 180),
 * min_frac_triangulated not finite, draw_cap < 0 or a table without words; device form: d_kps1, d_kps2 or d_work not 16-byte aligned. */
const char* hs_monoinit_check(int Q, const hs_monoinit_params* params, const int64_t* key_offsets1, const hs_keypoint* kps1, const int64_t* key_offsets2,
                              const hs_keypoint* kps2, const int32_t* matches12, const uint32_t* draws, int draw_cap, const hs_monoinit_result* results,
                              const uint8_t* inliers_h, const uint8_t* inliers_f, const float* p3d, const uint8_t* triangulated, int device, const void* d_work);
/* MonoEstimator::Initialize for Q problems.  Problem q owns kps1 [key_offsets1[q], key_offsets1[q + 1]) (n1 key points of the reference frame),
 * the same range of matches12 (matches12[i] = key point of frame 2 matched to key point i, a value outside [0, n2): none), of inliers_h and
 * inliers_f (u8 per COMPACTED match: entry j < N belongs to the j-th match in ascending i; entries from N on are 0), of p3d ([n1][3] float) and of
 * triangulated (u8 [n1], by key point of frame 1 like vP3D / vbTriangulated), and kps2 [key_offsets2[q], key_offsets2[q + 1]).  Every output is
 * ALWAYS written.  draws may be NULL with draw_cap = 0.  Host form: host pointers, synchronous, staged through the handle's scratch.
 * HS_ERR_INVALID, nothing enqueued and no output touched: what hs_monoinit_check refuses. */
int  hs_monoinit_estimate(hs_orb* h, int Q, const hs_monoinit_params* params, const int64_t* key_offsets1, const hs_keypoint* kps1, const int64_t* key_offsets2,
                          const hs_keypoint* kps2, const int32_t* matches12, const uint32_t* draws, int draw_cap, hs_monoinit_result* results,
                          uint8_t* inliers_h, uint8_t* inliers_f, float* p3d, uint8_t* triangulated);
/* The same with device pointers, enqueued on `stream` (NULL = the handle's own), nothing synchronises; params and the two offset arrays stay host
 * arrays and are read before the call returns.  d_kps1, d_kps2 and d_work (hs_monoinit_work_bytes bytes) are 16-byte aligned. */
int  hs_monoinit_estimate_device(hs_orb* h, int Q, const hs_monoinit_params* params, const int64_t* key_offsets1, const hs_keypoint* d_kps1,
                                 const int64_t* key_offsets2, const hs_keypoint* d_kps2, const int32_t* d_matches12, const uint32_t* d_draws, int draw_cap,
                                 hs_monoinit_result* d_results, uint8_t* d_inliers_h, uint8_t* d_inliers_f, float* d_p3d, uint8_t* d_triangulated,
                                 void* d_work, void* stream);

/* Measurement and parity tests: which of the two layouts of stage 2 the next calls launch, 0 (the default: one wave per hypothesis and model,
 * k_mono_hypotheses) or 1 (one lane per hypothesis, k_mono_hypotheses_lane).  Both give the same bytes.  Returns the previous value; any other
 * argument changes nothing.  Process-wide. */
int  hs_debug_monoinit_layout(int layout);

/* ================= frame tracking on resident tables: TrackMotionModel::track + TrackLocalMap::track =================
 * (src/slam/tracking/TrackMotionModel.cpp:14-83, TrackLocalMap.cpp:9-78, src/core/LandMarkMatches.cpp:26-64, Frame::UpdatePoseMatrices,
 * FeatureMatcher.cc:57-176.)  The glue between the device entry points above, as kernels: a pose that a kernel left in HBM feeds the next search,
 * a search's matches become the frame's associations, the optimiser's outlier flags come back onto them, and the two tracking strategies are one
 * enqueue-only call each.  Every `_device` entry point of this section enqueues on `stream` (NULL = the handle's own), synchronises nothing and
 * checks nothing that lives on the device; temporaries come from the caller's d_work (hs_track_work_bytes), except for the projection search's own
 * grid lists, which hs_search_by_projection_posed_device takes from the handle's scratch exactly as hs_search_by_projection_device does.  The
 * handle's one-stream-at-a-time rule applies (see hs_orb_extract_batch_device).
 *
 * The frame's LandMarkMatches as dense arrays by view (keypoint) index — the model of hyslam_amd/host/HipAssociationReplay.h:
 *   kp_lm   [n] int32   views_to_landmarks: the landmark index at view i, -1 = none.  Entries lie in [-1, L).
 *   kp_outl [n] u8      outliers: 0 = no entry, 1 = false, 2 = true
 *   n_matches [1] int32 LandMarkMatches::n_matches (path dependent: a landmark that moves does not decrement it) */

/* Frame::UpdatePoseMatrices on a pose in device memory: Rcw / tcw copied from the row-major 4x4 d_Tcw, Ow = -Rcw^T tcw as ONE cv::gemm (float
 * inputs, double accumulation left to right, alpha = -1 applied in double, one rounding to float). */
typedef struct hs_pose_view { float Rcw[9], tcw[3], Ow[3]; float _pad; } hs_pose_view;     /* 64 bytes */
int  hs_pose_views_device(hs_orb* h, const float* d_Tcw, hs_pose_view* d_out, void* stream);
/* hs_search_by_projection_device / hs_local_map_search_device in every output, with F->Rcw / tcw / Ow IGNORED and read from *d_pose by the kernels
 * (projection, landMarkSizePixels, the distance and viewing-angle criteria). */
int  hs_search_by_projection_posed_device(hs_orb* h, const hs_frame_view* F, const hs_pose_view* d_pose, const hs_landmark* d_lms, int L,
                                          const hs_proj_params* pp, int32_t* d_match_idx, float* d_match_dist, int32_t* d_n_matches, void* stream);
int  hs_local_map_search_posed_device(hs_orb* h, const hs_kf_table* T, const int32_t* d_frame_lm, int n_assoc, const int32_t* d_neigh, int neigh_cap,
                                      const int32_t* d_parent, int n_max_local_keyframes, int n_neighbor_keyframes, const hs_frame_view* F,
                                      const hs_pose_view* d_pose, const hs_landmark* d_lms, const hs_proj_params* pp, int cap, const hs_local_map_out* out,
                                      void* d_work, void* stream);

/* d_work of every entry point of this section: n = keypoints of the frame, n_last = keypoints of the last frame, L = landmarks of the map, cap = the
 * local map's capacity.  16-byte aligned, contents irrelevant before and after. */
size_t hs_track_work_bytes(int n, int n_last, int L, int cap);

/* The association loop at the end of _SearchByProjection_ (FeatureMatcher.cc:113-118) on the dense state: op j is associateLandMark(d_op_view[j],
 * d_op_lm[j], true); an op with a negative view or landmark (or one outside [0, n) / [0, L)) is skipped.  The ops are applied in ASCENDING LANDMARK
 * INDEX (the std::map<MapPoint*, ...> order), whatever their array order, each one literally as LandMarkMatches::associateLandMark
 * (stale outliers entries and the path-dependent n_matches included).  PRECONDITION: a landmark occurs in at most one op.  The initial state may hold
 * one landmark on several views.  Parallel closed form, integer atomicMin / atomicMax only: the same call gives the same bytes.
 * d_work: hs_track_work_bytes(n, 0, L, 0). */
int  hs_frame_associate_device(hs_orb* h, int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, int n_ops, const int32_t* d_op_view,
                               const int32_t* d_op_lm, void* d_work, void* stream);
/* d_kp_lm_obs[i] = -1 without a landmark, else T->lm_nobs[kp_lm[i]]: the array hs_frame_view wants.  drop_bad = 1 first removes the association of
 * every view whose landmark is T->lm_bad (removeLandMarkAssociation, TrackLocalMap.cpp:62: kp_lm = -1, kp_outl = 0, --n_matches).  Of T only L,
 * lm_nobs and (drop_bad) lm_bad are read.  d_kp_outl / d_n_matches may be NULL with drop_bad = 0. */
int  hs_frame_views_device(hs_orb* h, int n, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const hs_kf_table* T, int drop_bad,
                           int32_t* d_kp_lm_obs, void* stream);

/* What the two track functions do after Optimizer::PoseOptimization.  For every edge k < min(*d_n_edges, edge_cap), i = d_edges[k].kp: when the
 * problem ran (d_result->status != HS_POSE_TOO_FEW) kp_outl[i] = d_outlier[k] ? 2 : 1 (setOutlier); then, with isOutlier(i) = (kp_outl[i] == 2):
 *   HS_TRACK_MOTION (TrackMotionModel.cpp:62-79)  an outlier loses its association (kp_lm = -1, kp_outl = 0, --n_matches); an inlier whose landmark
 *                                                 has T->lm_nobs > 0 counts
 *   HS_TRACK_LOCAL  (TrackLocalMap.cpp:25-38)     an inlier with lm_nobs > 0 counts; an outlier is removed only when sensor == 1, else it stays
 *                                                 associated with its flag at 2
 * As in the reference, setOutlier does nothing on a view without an `outliers` entry (kp_outl == 0), and the loop passes over a view that holds no
 * landmark (kp_lm < 0): neither occurs inside the chain, where every edge is a held view with an entry.  edges[k].kp must be a valid view index.
 * d_counts [1] = the count: nmatchesMap / mnMatchesInliers.  One workgroup; integer sums. */
#define HS_TRACK_MOTION 0
#define HS_TRACK_LOCAL  1
int  hs_track_discard_device(hs_orb* h, int mode, const hs_pose_edge* d_edges, const int32_t* d_n_edges, int edge_cap, const uint8_t* d_outlier,
                             const hs_pose_result* d_result, const hs_kf_table* T, int sensor, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches,
                             int32_t* d_counts, void* stream);

/* th_motion / th_motion_wide: the search radii of TrackMotionModel.cpp:38-50 AS THE REFERENCE'S `int th` HOLDS THEM — the caller truncates
 * (th = (int)match_radius_threshold_x; th_wide = (int)(match_theshold_inflation_factor * th)) and picks the parameter by the reference's inverted
 * naming (:39-42: sensor != 1 selects match_radius_threshold_stereo).  The product Vcw * Tcw_last and ScaleVelocity stay with the caller too. */
typedef struct hs_track_params {
    float   th_motion, th_motion_wide;
    int32_t n_min_matches;             /* TrackMotionModelParameters::N_min_matches                      */
    float   th_local;                  /* TrackLocalMapParameters::match_radius_threshold                */
    float   nnratio_motion, nnratio_local;
    float   th_high;                   /* FeatureMatcherSettings::TH_HIGH                                */
    float   sigma_ref;
    int32_t n_max_local_keyframes, n_neighbor_keyframes;
} hs_track_params;
typedef struct hs_track_state {        /* the frame's associations, device memory, in / out              */
    int32_t* kp_lm;                    /* [n]                                                            */
    uint8_t* kp_outl;                  /* [n]                                                            */
    int32_t* n_matches;                /* [1]                                                            */
    int32_t* kp_lm_obs;                /* [n]  maintained by the calls; F->kp_lm_obs is ignored          */
} hs_track_state;
#define HS_TRACK_OK 0
#define HS_TRACK_MOTION_FAILED 1       /* fewer than n_min_matches matches also in the wide window: TrackMotionModel::track returned -1 */
/* hs_track_motion_model_device writes status, used_wide, n_narrow, n_wide, n_matches_map and zeroes the rest; hs_track_local_map_device writes
 * n_inliers ONLY (called on its own it leaves the other fields as the caller's memory had them); hs_track_frame_device therefore defines all. */
typedef struct hs_track_result {
    int32_t status;                    /* HS_TRACK_*                                                     */
    int32_t used_wide;                 /* 1: the associations are the wide search's                      */
    int32_t n_narrow, n_wide;          /* nmatches of the two searches                                   */
    int32_t n_matches_map;             /* TrackMotionModel::track's return value (0 when it failed)      */
    int32_t n_inliers;                 /* TrackLocalMap::track's return value                            */
    int32_t _pad[2];
} hs_track_result;                     /* 32 bytes */
/* every pointer is device memory and required; n = F->n, n_last = the last frame's keypoints, cap = the local map's capacity */
typedef struct hs_track_out {
    hs_pose_view* pose_view;           /* [2]      the pose views of the two stages (predicted, motion-optimised)                    */
    hs_pose_problem* problem;          /* [2]      the optimiser's problems                                                          */
    hs_landmark* last_lms;             /* [n_last] the last frame's landmark records, 16-byte aligned                                */
    int32_t* narrow_idx;  float* narrow_dist;  int32_t* narrow_n;      /* [n_last] [n_last] [1]  the search with th_motion           */
    int32_t* wide_idx;    float* wide_dist;    int32_t* wide_n;        /* the search with th_motion_wide                             */
    int32_t* op_view;                  /* [n_last] the chosen search's match_idx: the ops (op_view[j], last_kp_lm[j])                */
    hs_pose_edge* edges_motion;        /* [n]      16-byte aligned                                                                   */
    uint8_t* outlier_motion;           /* [n]                                                                                        */
    int32_t* n_edges_motion;           /* [2]      [0] nInitialCorrespondences, [1] what the optimiser sees: 0 when the stage failed */
    hs_pose_result* pose_motion;       /* [1]                                                                                        */
    hs_local_map_out local;            /* the local map's outputs (frame_remove is all 0: stage 2 drops bad landmarks first)         */
    hs_pose_edge* edges_local;         /* [n]                                                                                        */
    uint8_t* outlier_local;            /* [n]                                                                                        */
    int32_t* n_edges_local;            /* [1]                                                                                        */
    hs_pose_result* pose_local;        /* [1]                                                                                        */
    hs_track_result* result;           /* [1]                                                                                        */
} hs_track_out;

/* The three calls below are sequences of launches.  Arguments are checked before the first one; a HIP error from a stage in the middle (a failed
 * launch, a scratch regrow that fails) is returned after the earlier stages were already enqueued: the outputs and the state are then undefined and
 * the caller drains the stream (hs_orb_synchronize) before reusing the buffers.
 * The searches use frac_smaller / frac_larger = 0.5 / 1.5 (FeatureSizeCriterion(0.5, 1.5)) and dist_is_invariance_range = 0: d_lms[].min_dist / max_dist
 * hold mfMinDistance / mfMaxDistance, the kernel applies 0.8 / 1.2.  Records that hold the invariance range already (what an adaptor reads through
 * GetMin / MaxDistanceInvariance) are converted once when they are made resident: min_dist / 0.8f, max_dist / 1.2f are NOT exact inverses, so such an
 * integration keeps the raw distances in its resident records. */
/* TrackMotionModel::track from current_frame.SetPose(Tcw_cur) on (:33).  d_Tcw_pred float[16]: the predicted pose.  Last frame: d_last_kps [n_last]
 * (the angle is read) and d_last_kp_lm [n_last], its associations as landmark indices (a landmark at most once).  d_lms [L]: the map's records; T:
 * lm_nobs is read.  F: the current frame with device pointers; its Rcw / tcw / Ow / kp_lm_obs are ignored.  Enqueued, in this order: pose view;
 * gather of the last frame's landmarks (record j = last keypoint j: skip = 1 where it holds none or the index is outside [0, L), assoc_kp = -1,
 * prev_angle = d_last_kps[j].angle); clearAssociations; BOTH searches (use_stereo, check_rotation, use_prev_matched, th_high, nnratio_motion) from
 * the cleared frame; the select (narrow iff n_narrow >= n_min_matches, else wide; HS_TRACK_MOTION_FAILED when the chosen count is < n_min_matches);
 * hs_frame_associate_device; hs_pose_edges_device; the gate; hs_pose_optimize_device; hs_track_discard_device.  When the stage fails the optimiser
 * sees 0 edges, reports HS_POSE_TOO_FEW and hands back the predicted pose, nothing is discarded, and the wide search's associations stay on the
 * frame — the state in which the reference returns -1. */
int  hs_track_motion_model_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm,
                                  int n_last, const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_state* st,
                                  const hs_track_out* out, void* d_work, void* stream);
/* TrackLocalMap::track from the pose d_Tcw_in float[16] and the associations in *st: pose view; hs_frame_views_device with drop_bad = 1;
 * hs_local_map_search_posed_device with d_frame_lm = kp_lm, n_assoc = n (use_distance, use_stereo, use_prev_matched, th_high, nnratio_local);
 * hs_frame_associate_device with the ops (match_idx[j], sel[j]); hs_pose_edges_device; hs_pose_optimize_device from d_Tcw_in;
 * hs_track_discard_device (HS_TRACK_LOCAL, F->sensor).  mnLastFrameSeen and SetReferenceMapPoints are not modelled: nothing here reads them. */
int  hs_track_local_map_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_in, const hs_kf_table* T, const hs_landmark* d_lms,
                               const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent, int cap, const hs_track_params* tp, const hs_track_state* st,
                               const hs_track_out* out, void* d_work, void* stream);
/* the two, enqueued back to back: stage 2 starts from out->pose_motion->Tcw and runs whatever stage 1 reports (its input state is defined in every
 * case); the caller reads *out->result once at the end and decides what TrackingStateNormal.cpp:34-41,71 decides.  It IS the two calls. */
int  hs_track_frame_device(hs_orb* h, const hs_frame_view* F, const float* d_Tcw_pred, const hs_keypoint* d_last_kps, const int32_t* d_last_kp_lm,
                           int n_last, const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh, int neigh_cap, const int32_t* d_parent,
                           int cap, const hs_track_params* tp, const hs_track_state* st, const hs_track_out* out, void* d_work, void* stream);

/* ================= TrackReferenceKeyFrame::track on resident tables: the BoW search and the association replay =================
 * (src/slam/tracking/TrackReferenceKeyFrame.cpp:22-30, FeatureMatcher.cc:216-278, Frame.cc:221-232)  The two steps
 * of the tracker's fall-back that had no resident form; with hs_bow_transform_device before them and hs_pose_edges_device, hs_pose_optimize_device and
 * hs_track_discard_device (HS_TRACK_MOTION) after them they make TrackReferenceKeyFrame::track without a host pointer.  Both are enqueue-only under
 * the rules of the section above; temporaries come from the caller's d_work (hs_track_refkf_work_bytes), nothing takes the handle's scratch, nothing
 * synchronises.
 *
 * The key frames' features, resident (every pointer device memory).  Key frame s owns keypoints [kf_off[s], kf_off[s + 1]).  node / weight: the
 * d_node and d_weight hs_bow_transform_device wrote for the key frame's descriptors, unchanged.  A keypoint is in the feature vector when its weight is
 * positive (DBoW2: `if (w > 0) fv.addFeature(nid, i)`) and its node is not negative; weight == NULL puts every keypoint with a non-negative node in.
 * kp_lm: KeyFrame::hasAssociation(idx) as a landmark index, -1 = none. */
typedef struct hs_kf_features {
    int32_t n_kf;
    const int64_t* kf_off;             /* [n_kf + 1]                                                     */
    const hs_keypoint* kps;            /* [total]   the angle is read                                    */
    const uint8_t* desc;               /* [total][32]                                                    */
    const int32_t* node;               /* [total]                                                        */
    const int32_t* kp_lm;              /* [total]                                                        */
    const float* weight;               /* [total]   may be NULL                                          */
} hs_kf_features;
/* FeatureMatcher::SearchByBoW(KeyFrame*, Frame&, map&) between key frame *d_kf_slot (read on the device: in a chain it is the local.max_slot the
 * previous frame's local-map stage left) and the frame: d_kps, d_desc [n] and d_node, d_weight [n] as hs_bow_transform_device left them (d_weight may be
 * NULL: every keypoint with a non-negative node is in; otherwise as above), so the transform's outputs feed the search with no step in between.  Side 1:
 * the key frame's keypoints with 0 <= kp_lm < T->L and !T->lm_bad[kp_lm] (PreviouslyMatchedIndexCriterion(true)); each takes the first minimum over the
 * frame's keypoints of its node in ascending index, accepted when d < th_low && d < nnratio * d2 (d2 = FLT_MAX with one candidate);
 * then RotationConsistencyBoW, always (rot = frame angle - key-frame angle; the reference does not read checkOri on this path).  Outputs: d_match_kf
 * [kf_cap]: the frame view key-frame keypoint j took, -1 = none, every entry written; *d_n_matches = matches_internal.size(), counted before the
 * collapse; d_op_view / d_op_lm [n]: `matches[idx_f] = lm` as ops for hs_frame_associate_views_device: d_op_view[f] = f and d_op_lm[f] = the landmark
 * of the LARGEST key-frame index that took view f, both -1 for a view nobody took.  A slot outside [0, K->n_kf) or an empty key frame gives 0
 * matches; a key frame with more than kf_cap keypoints is truncated in ascending index.  kf_cap >= 1, 1 <= n <= 65535.  Of T only L and lm_bad are
 * read.  Integer atomics only: the same call gives the same bytes.  d_work is not used today and may be NULL. */
int  hs_search_by_bow_kf_device(hs_orb* h, const hs_kf_features* K, const int32_t* d_kf_slot, const hs_kf_table* T, const hs_keypoint* d_kps,
                                const uint8_t* d_desc, const int32_t* d_node, const float* d_weight, int n, float th_low, float nnratio, int32_t* d_match_kf,
                                int kf_cap, int32_t* d_op_view, int32_t* d_op_lm, int32_t* d_n_matches, void* d_work, void* stream);
/* Frame::associateLandMarks(matches, true) on the dense state: op j is associateLandMark(d_op_view[j], d_op_lm[j], true), j < n; an op with a view
 * outside [0, n) or a landmark outside [0, L) is skipped.  The ops are applied in ASCENDING VIEW INDEX (the std::map<size_t, MapPoint*> order),
 * whatever their array order, each literally as LandMarkMatches::associateLandMark.  PRECONDITIONS: a view occurs in at most one op and a landmark in
 * at most one (hs_search_by_bow_kf_device's output satisfies both when a key frame holds a landmark on one view).  The frame is not cleared first and
 * may hold one landmark on several views.  Parallel closed form, integer atomicMin only: the same call gives the same bytes.
 * d_work: hs_track_refkf_work_bytes(n, 0, L), 16-byte aligned, contents irrelevant before and after. */
size_t hs_track_refkf_work_bytes(int n, int kf_cap, int L);
int  hs_frame_associate_views_device(hs_orb* h, int n, int L, int32_t* d_kp_lm, uint8_t* d_kp_outl, int32_t* d_n_matches, const int32_t* d_op_view,
                                     const int32_t* d_op_lm, void* d_work, void* stream);

/* ================= initial pose estimation as one resident call: both gates on the device =================
 * (src/slam/tracking/TrackingStateNormal.cpp:21-58, TrackReferenceKeyFrame.cpp:10-58; DESIGN.md 5.13 "the chain")
 * TrackingStateNormal::initialPoseEstimation decides twice on a count: the motion model's return value decides whether the fall-back runs (:34), and
 * the BoW search's count decides whether the fall-back optimises (TrackReferenceKeyFrame.cpp:27).  The three calls below take both decisions on the
 * device: every step is enqueued whatever the counts are, and a step that is switched off reads its gate from device memory and changes nothing.
 * They are enqueue-only under the rules of the tracking section: the arguments are checked on the host before the first launch (a vocabulary that
 * lives on another device than h among them: what hs_bow_transform_device refuses, these refuse), nothing synchronises, nothing reads device memory
 * on the host, and nothing takes the handle's scratch beyond what the reused calls take (the projection searches' grid lists).
 *
 * The gate, evaluated by every thread of k_init_gate from the same two words:
 *   motion_return = motion status == HS_TRACK_MOTION_FAILED ? -1 : n_matches_map      (0 for a stage that is not predicated)
 *   run           = not predicated || motion_return < thresh_init
 *   refkf_status  = !run ? HS_REFKF_SKIPPED : n_bow < n_min_matches_bow ? HS_REFKF_BOW_FAILED : HS_REFKF_OK
 * A stage that is not HS_REFKF_OK leaves the state (kp_lm, kp_outl, n_matches) byte for byte as it found it, hands the optimiser 0 edges
 * (n_edges[1] = 0, pose->status = HS_POSE_TOO_FEW, pose->Tcw = d_Tcw_last) and copies d_Tcw_entry to Tcw_init bit for bit.  The transform and the
 * search run in every case: bow_*, match_kf, op_view / op_lm, n_bow and n_edges[0] are what they are for a stage that runs. */
typedef struct hs_track_refkf_params {
    float   th_low, nnratio;           /* FeatureMatcherSettings::TH_LOW; TrackReferenceKeyFrame's matcher ratio                       */
    int32_t n_min_matches_bow;         /* TrackReferenceKeyFrameParameters::N_min_matches_BoW                                          */
    int32_t thresh_init;               /* StateNormalParameters::thresh_init                                                           */
} hs_track_refkf_params;
#define HS_REFKF_OK 0
#define HS_REFKF_BOW_FAILED 1          /* fewer than n_min_matches_bow matches: TrackReferenceKeyFrame::track returned -1               */
#define HS_REFKF_SKIPPED 2             /* the motion model's return value was at least thresh_init: the fall-back did not run           */
typedef struct hs_track_initial_result {
    int32_t refkf_status;              /* HS_REFKF_*                                                                                   */
    int32_t n_bow;                     /* the search's nmatches, also for a skipped stage                                              */
    int32_t n_matches_map_refkf;       /* TrackReferenceKeyFrame::track's nmatchesMap; 0 unless HS_REFKF_OK                            */
    int32_t n_init;                    /* initialPoseEstimation's nmatches: OK: the line above; BOW_FAILED: -1; SKIPPED: motion_return */
    int32_t success;                   /* n_init > thresh_init (:41)                                                                   */
    int32_t _pad[3];                   /* written as 0                                                                                 */
} hs_track_initial_result;             /* 32 bytes */
typedef struct hs_track_initial_out {  /* all device memory, all required; n = F->n                                                    */
    int32_t* bow_word; float* bow_weight; int32_t* bow_node;      /* [n]  hs_bow_transform_device's outputs for the frame              */
    int32_t* match_kf;                 /* [kf_cap] hs_search_by_bow_kf_device's                                                        */
    int32_t* op_view; int32_t* op_lm;  /* [n]  as the search leaves them: never masked                                                 */
    hs_pose_view* pose_view; hs_pose_problem* problem;            /* [1]  from d_Tcw_last                                              */
    hs_pose_edge* edges;               /* [n]  16-byte aligned                                                                         */
    uint8_t* outlier;                  /* [n]                                                                                          */
    int32_t* n_edges;                  /* [2]  [0] nInitialCorrespondences, [1] what the optimiser sees: 0 unless HS_REFKF_OK          */
    hs_pose_result* pose;              /* [1]                                                                                          */
    float* Tcw_init;                   /* [16] the pose the frame holds after the stage: pose->Tcw when OK, else d_Tcw_entry           */
    hs_track_initial_result* result;   /* [1]                                                                                          */
    hs_track_result* frame_result;     /* [1]  written by hs_track_normal_device only; not the record hs_track_out.result points to    */
} hs_track_initial_out;
/* d_work of the three calls: hs_track_work_bytes's area, hs_track_refkf_work_bytes's, the masked ops.  16-byte aligned, contents irrelevant before
 * and after. */
size_t hs_track_initial_work_bytes(int n, int n_last, int L, int cap, int kf_cap);
/* TrackReferenceKeyFrame::track as the fall-back of initialPoseEstimation.  F: the frame with device pointers (n, sensor, the camera, kps, desc, uR,
 * size_ref are read).  vocab: the resident vocabulary; K, d_kf_slot, kf_cap: as hs_search_by_bow_kf_device.  d_Tcw_last float[16]: the last frame's
 * pose, from which the optimiser starts (SetPose(last_frame.mTcw), :32).  d_Tcw_entry float[16]: the pose the frame holds on entry.
 * d_motion_result: the motion stage's record, on which the stage is predicated, or NULL for a stage that always runs.  tp: sigma_ref is read.
 * Enqueued, in this order: hs_bow_transform_device on F->desc; hs_search_by_bow_kf_device (always: n_bow is reported for a skipped stage too); the
 * gate; hs_frame_associate_views_device on the masked ops; pose view and problem from d_Tcw_last; hs_pose_edges_device; the edge gate;
 * hs_pose_optimize_device; hs_track_discard_device (HS_TRACK_MOTION) on &n_edges[1]; the finish (n_init, success, Tcw_init).
 * iout->frame_result is not touched.  1 <= F->n <= 65535, kf_cap >= 1, T->L >= 1. */
int  hs_track_reference_keyframe_device(hs_orb* h, const hs_frame_view* F, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap,
                                        const float* d_Tcw_last, const float* d_Tcw_entry, const hs_track_result* d_motion_result, const hs_kf_table* T,
                                        const hs_landmark* d_lms, const hs_track_params* tp, const hs_track_refkf_params* rp, const hs_track_state* st,
                                        const hs_track_initial_out* iout, void* d_work, void* stream);
/* TrackingStateNormal::initialPoseEstimation.  The validity of the trajectory's velocity stays a host fact.  velocity_valid != 0:
 * hs_track_motion_model_device (its arguments as there), then the call above predicated on out->result with d_Tcw_entry = out->pose_motion->Tcw (the
 * caller's d_Tcw_entry is not read).  velocity_valid == 0: the call above alone, not predicated, on the caller's d_Tcw_entry and on the state as it
 * is; d_Tcw_pred, the last frame and `out` are not read and may be NULL.  It IS these calls. */
int  hs_track_initial_device(hs_orb* h, const hs_frame_view* F, int velocity_valid, const float* d_Tcw_pred, const hs_keypoint* d_last_kps,
                             const int32_t* d_last_kp_lm, int n_last, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap,
                             const float* d_Tcw_last, const float* d_Tcw_entry, const hs_kf_table* T, const hs_landmark* d_lms, const hs_track_params* tp,
                             const hs_track_refkf_params* rp, const hs_track_state* st, const hs_track_out* out, const hs_track_initial_out* iout, void* d_work,
                             void* stream);
/* TrackingStateNormal's two stages: hs_track_initial_device, then hs_track_local_map_device from iout->Tcw_init, then one record for the key-frame
 * stage: iout->frame_result = { status = HS_TRACK_OK, used_wide / n_narrow / n_wide of the motion stage (0 when it did not run), n_matches_map =
 * n_init, n_inliers of the local stage }.  With that record and ok_override = -1, hs_keyframe_gate_device computes n_init > thresh_init && n_inliers
 * > thresh_refine && !force_loss: TrackingStateNormal.cpp:41,71 for every path, the fall-back included.  `out` is required in both modes (the local
 * stage writes into it).  It is these calls and nothing else: the local-map stage runs whatever the initial stage reports, exactly as in
 * hs_track_frame_device; gating it on `success` is NOT done here and stays with the caller, who reads iout->result / iout->frame_result once. */
int  hs_track_normal_device(hs_orb* h, const hs_frame_view* F, int velocity_valid, const float* d_Tcw_pred, const hs_keypoint* d_last_kps,
                            const int32_t* d_last_kp_lm, int n_last, const hs_vocab_dev* vocab, const hs_kf_features* K, const int32_t* d_kf_slot, int kf_cap,
                            const float* d_Tcw_last, const float* d_Tcw_entry, const hs_kf_table* T, const hs_landmark* d_lms, const int32_t* d_neigh,
                            int neigh_cap, const int32_t* d_parent, int cap, const hs_track_params* tp, const hs_track_refkf_params* rp,
                            const hs_track_state* st, const hs_track_out* out, const hs_track_initial_out* iout, void* d_work, void* stream);

/* ================= after the two track functions: reference key frame, key-frame decision, stereo landmark creation =================
 * (src/main/Tracking.cpp:179-227,273-317,375-388, src/slam/tracking/TrackingStateNormal.cpp:87-170, src/slam/tracking/TrackingState.cpp:20-93;
 * DESIGN.md 5.14)  What Tracking::_Track_ does with the frame once hs_track_frame_device has run, on the same dense state (kp_lm,
 * kp_outl, n_matches, kp_lm_obs) and the same tables: six stages, one enqueue-only entry point each under the rules of the tracking section
 * (nothing synchronises, nothing on the device is checked, temporaries come from the caller's d_work = hs_keyframe_work_bytes), and one composite
 * that IS these calls in this order.  Integer and flag work equals the reference exactly; the one float computation (UnprojectStereo) is stated
 * at stage 5.  Every kernel is bounded by n, the reference key frame's keypoint count or new_cap; the kernel boundary is the only synchronisation.
 *
 * A stage that is switched off (ok == 0, insert == 0, sensor == 0) is still launched: its kernels read the flag from *d_result at entry and write
 * zeros to their outputs — the mechanism of hs_track_motion_model_device's gate.
 *
 * PROVISIONAL LANDMARKS.  Stage 5 leaves the index T->L + k on the view that created point k.  Until the caller has appended the new landmarks to
 * its tables (and calls with the larger L), every existing kernel tests `(unsigned)kp_lm < (unsigned)L` before it reads a table through the index:
 * k_frame_views (kp_lm_obs = -1, never dropped), the replays' k_assoc_* / k_vassoc_* (the view counts as held, no jk / lm_view slot is touched),
 * k_pose_edges (no edge), k_kf_votes and k_lp_mark (no vote, frame_remove = 0), k_last_gather (skip = 1), k_track_discard (an outlier is
 * still removed, an inlier does not count).  So the state may be handed to the next hs_track_frame_device call before or after the append.
 * The append must have happened before the next frame that INSERTS: stage 5 numbers from T->L again, and an index a view still holds would name two points.
 * kp_lm_obs of a provisional view is 0 when stage 5 has just made it and -1 once a later k_frame_views (stage 1 of the next call, TrackLocalMap)
 * has rewritten it; the searches test `> 0`, so both read "not yet matched to an observed landmark".
 *
 * Integer widths of the decision (read from the declarations): Frame::mnId is `long unsigned int` (Frame.h:195) = frame_id uint64;
 * Tracking::mnLastKeyFrameId and the last_keyframe_id parameter are `unsigned int` (Tracking.h:195) = uint32; min / max_KF_interval and every
 * other threshold are `int`.  `last_keyframe_id + max_KF_interval` is therefore evaluated in 32-bit unsigned arithmetic (wrapping) and widened to
 * 64 bits for the comparison with mnId; getQueueLength() is `int`. */
typedef struct hs_keyframe_params {
    uint64_t frame_id;                 /* current_frame.mnId                                                                          */
    uint32_t last_keyframe_id;         /* mnLastKeyFrameId                                                                            */
    int32_t force;                     /* the `force` argument of newKeyFrame (Tracking.cpp:193: false)                               */
    int32_t mapping_stopped;           /* thread_status->mapping.isStopped() || isStopRequested()                                     */
    int32_t mapping_idle;              /* thread_status->mapping.isAcceptingInput()                                                   */
    int32_t mapping_queue_length;      /* thread_status->mapping.getQueueLength()                                                     */
    int32_t n_kfs_in_map;              /* pMap->KeyFramesInMap(): nMinObs = n_kfs_in_map <= 2 ? 2 : 3                                 */
    int32_t min_N_tracked_close, thresh_N_nontracked_close, min_KF_interval, max_KF_interval, N_tracked_target, N_tracked_variance;
    float   th_depth;                  /* camera.thDepth                                                                              */
    int32_t n_min_points;              /* the literal 100 of TrackingState.cpp:85                                                     */
    int32_t thresh_init, thresh_refine;/* StateNormalParameters (TrackingStateNormal.cpp:41,71)                                       */
    int32_t force_loss;                /* 1: the reset_interval branch fired (:78-82); n_frames_tracked_consecutively stays a host counter */
    int32_t ok_override;               /* -1: compute ok from *d_track_result; 0 / 1: take this (a fall-back driven step by step; hs_track_normal_device's frame_result needs none) */
} hs_keyframe_params;
typedef struct hs_keyframe_result {
    int32_t ok;                        /* stage 2: bOK                                                                                */
    int32_t ref_slot;                  /* stage 1: *d_ref_slot afterwards                                                             */
    int32_t n_valid;                   /* stage 3: numValidMatches() = held views with kp_outl != 2                                   */
    int32_t n_ref_matches, n_tracked_close, n_nontracked_close, insert;       /* stage 4                                              */
    int32_t n_new, n_candidates, n_processed;                                  /* stage 5: points created, vDepthIdx.size(), loop trips */
    int32_t _pad[6];
} hs_keyframe_result;                  /* 64 bytes */
/* every pointer is device memory; all but lms are required.  Arrays are [new_cap] unless said otherwise. */
typedef struct hs_keyframe_out {
    hs_keyframe_result* result;        /* [1]                                                                                         */
    hs_pose_view* pose_view;           /* [1]  UpdatePoseMatrices on the final pose (TrackingState.cpp:32)                            */
    int32_t* new_view;                 /* the view that created point k                                                               */
    float* new_pos;                    /* [new_cap][3]  its world position                                                            */
    hs_lm_entry_in* entries;           /* the creation records, as hs_landmark_update_entries_device reads them: pos, ref_Ow = frame Ow */
    hs_lm_obs* obs;                    /* one observation each: Ow, the frame's camera, u, v, kp_size, assoc_pos = pos, assoc = 1     */
    int64_t* obs_offsets;              /* [new_cap + 1]  = k, every entry written                                                     */
    int64_t* desc_offsets;             /* [new_cap + 1]  = k, every entry written                                                     */
    uint8_t* desc;                     /* [new_cap][32]  the keypoint's descriptor, 16-byte aligned                                   */
    int32_t* lm_index;                 /* T->L + k for k < min(n_new, new_cap), -1 behind: every entry written                        */
    hs_landmark* lms;                  /* optional [lms_cap], 16-byte aligned: record T->L + k (when below lms_cap) receives pos, assoc_kp = -1,
                                          prev_angle = 0 and skip = 0 — the fields the entry update's scatter never writes             */
    int32_t lms_cap;
} hs_keyframe_out;
/* d_work of every entry point of this section.  n: keypoints of the frame; kf_cap: at least T->n_kf (the vote's counter row); new_cap as above.
 * 16-byte aligned, contents irrelevant before and after. */
size_t hs_keyframe_work_bytes(int n, int kf_cap, int new_cap);

/* Stage 1, Tracking::determineReferenceKeyFrame (:273-317) and `if (mpReferenceKF) ...` (:181-183, :229-230); runs whether or not tracking
 * succeeded.  It is hs_frame_views_device(drop_bad = 1) followed by hs_kf_votes_device with Q = 1, q_lm = kp_lm [0, n), count_bad_kf = 1, cap = 0:
 * a landmark held on two views votes twice; the maximum is over key frames that are not bad, the lowest slot among equals.  d_ref_slot [1] in / out
 * receives max_slot when that is >= 0 and keeps its value otherwise; d_result->ref_slot = the value afterwards.  Two one-thread kernels of its own:
 * the query's offsets {0, n} before the vote, the update after it. */
int  hs_keyframe_reference_device(hs_orb* h, int n, const hs_track_state* st, const hs_kf_table* T, int32_t* d_ref_slot, hs_keyframe_result* d_result,
                                  void* d_work, void* stream);
/* Stage 2, the gate: d_result->ok = prm->ok_override >= 0 ? prm->ok_override != 0 : (status == HS_TRACK_OK && n_matches_map > thresh_init &&
 * n_inliers > thresh_refine && !force_loss), read from *d_track_result on the device (TrackingStateNormal.cpp:41,71,78-82).  d_track_result may be
 * NULL with an override.  With ok == 0 stages 3-6 leave the state untouched and write zeros to their fields of *d_result. */
int  hs_keyframe_gate_device(hs_orb* h, const hs_track_result* d_track_result, const hs_keyframe_params* prm, hs_keyframe_result* d_result, void* stream);
/* Stage 3, HandlePostTrackingSuccess (:375-388): every held view whose landmark (an index in [0, T->L)) has T->lm_nobs < 1 loses its association
 * (kp_lm = -1, kp_outl = 0, kp_lm_obs = -1, --n_matches; the setOutlier(false) before it is invisible after the erase); n_valid is counted after. */
int  hs_keyframe_clean_device(hs_orb* h, int n, const hs_track_state* st, const hs_kf_table* T, hs_keyframe_result* d_result, void* stream);
/* Stage 4, needNewKeyFrame (:87-170), literally and in the widths above.  n_ref_matches = TrackedMapPoints(nMinObs) (KeyFrame.cc:201-222) of key
 * frame *d_ref_slot: its keypoints K->kp_lm[kf_off[s] .. kf_off[s+1]) with an index in [0, T->L), !T->lm_bad and T->lm_nobs >= nMinObs; a slot
 * outside [0, K->n_kf) gives 0 (the reference dereferences a null mpReferenceKF there).  n_tracked_close / n_nontracked_close: over
 * the views with d_depth > 0 && d_depth < th_depth, held && kp_outl != 2 / everything else; both 0 when sensor == 0.  mnMatchesInliers is
 * d_track_result->n_inliers (0 when d_track_result is NULL).  The counts are written also when the decision returns early on mapping_stopped
 * (the reference does not compute them there; nothing reads them).  thRefRatio is dead code in the reference and is not modelled. */
int  hs_keyframe_need_device(hs_orb* h, int n, int sensor, const float* d_depth, const hs_track_state* st, const hs_kf_table* T, const hs_kf_features* K,
                             const int32_t* d_ref_slot, const hs_track_result* d_track_result, const hs_keyframe_params* prm, hs_keyframe_result* d_result,
                             void* stream);
/* Stage 5, createNewKeyFrame (:20-93); does something when d_result->insert != 0 and F->sensor != 0.  hs_pose_views_device(d_Tcw) -> out->pose_view
 * first (always).  Candidates: views with d_depth > 0 (NaN and <= 0 out, +inf in), in the order of std::sort on pair<float, int>: ascending depth,
 * then ascending index — ranked by counting on the key (depth bits << 32 | index << 1 | creates: the low bit says whether the view would create a point, so the
 * same count numbers the points), no atomic decides a position.  Closed form of the walk (DESIGN.md
 * 5.14): with n_cand candidates and f = the number of them with !(depth > th_depth), the loop runs positions 0 .. j* where j* = max(n_min_points, f)
 * when f < n_cand and that maximum is < n_cand, and the whole list otherwise (so always with a NaN th_depth).  A processed view creates a point when
 * it is empty or when its landmark (an index in [0, T->L)) has lm_nobs < 1, whose association is removed first.  Points are numbered k = 0, 1, ...
 * in sorted order (creation order, not address order); view i then holds T->L + k by the fresh insert of associateLandMark(i, p,
 * false): kp_outl keeps a stale 1 or 2 on a view that was empty and becomes 1 otherwise; n_matches grows by one per view that was empty;
 * kp_lm_obs = 0.  Position = Frame::UnprojectStereo (Frame.cc:481-494, Camera.cpp:155-159): x = (u - cx) * (z / fx), y likewise, in float as
 * written, no contraction; then mRwc * x3Dc + mOw as one cv::gemm — float inputs, double products summed left to right from 0, + Ow in double, one
 * rounding; mRwc = the transpose of pose_view->Rcw.  d_result->n_new holds the full count; records k >= new_cap are not written and truncation is
 * not an error (the state is complete either way).  F: n, sensor, fx, fy, cx, cy, kps, desc are read. */
int  hs_keyframe_create_device(hs_orb* h, const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_track_state* st, const hs_kf_table* T,
                               const hs_keyframe_params* prm, int new_cap, const hs_keyframe_out* out, void* d_work, void* stream);
/* Stage 6, the final outlier removal (:219-225): every held view with kp_outl == 2 loses its association (kp_lm_obs = -1, --n_matches). */
int  hs_keyframe_discard_device(hs_orb* h, int n, const hs_track_state* st, hs_keyframe_result* d_result, void* stream);
/* The six, in this order.  d_Tcw float[16]: the final pose, in a chain &track_out.pose_local->Tcw[0].  d_ref_slot [1] in / out.  The caller reads
 * *out->result once; after an insert it appends n_new landmarks and one key frame to its tables. */
int  hs_track_keyframe_device(hs_orb* h, const hs_frame_view* F, const float* d_depth, const float* d_Tcw, const hs_kf_table* T, const hs_kf_features* K,
                              const hs_track_result* d_track_result, const hs_keyframe_params* prm, const hs_track_state* st, int32_t* d_ref_slot,
                              int new_cap, const hs_keyframe_out* out, void* d_work, void* stream);

/* Device memory of the handle's device for callers without a HIP binding of their own (the Python FrameTracker): plain hipMalloc / hipFree /
 * hipMemcpy after hipSetDevice(handle's device).  hs_device_copy: kind 1 = host to device, 2 = device to host; it first waits for `stream` (NULL =
 * the handle's own), so a read after an enqueue-only call sees its results; synchronous. */
int  hs_device_alloc(hs_orb* h, size_t bytes, void** out);
int  hs_device_free(hs_orb* h, void* d_ptr);
int  hs_device_copy(hs_orb* h, void* dst, const void* src, size_t bytes, int kind, void* stream);

/* ---- frame records: the fixed-size unit of the cross-camera exchange (BASELINE config 5; new — the reference has no
 * multi-camera exchange).  record = { int32 count; 12 bytes pad; hs_keypoint kps[cap]; pad to a 16-byte boundary; uint8 desc[cap][32] }: the
 * extractor's three outputs laid out in one buffer, so hs_orb_extract_batch_device writes a frame straight into the all-gather message (the
 * device entry points want the descriptor block 16-byte aligned — it is written with 16-byte vector stores — hence the padding for odd cap;
 * put the records themselves at 16-byte aligned addresses with a stride that is a multiple of 16: hs_record_bytes is). */
#define HS_RECORD_HEADER 16
size_t hs_record_bytes(int cap);
void   hs_record_offsets(int cap, size_t* off_count, size_t* off_kps, size_t* off_desc);
/* Cross-camera brute-force 2-NN over `world` gathered records (device memory, `record_stride` bytes apart): for every peer p != rank the
 * descriptors of record `rank` are matched against record p's.  The counts are read from the record headers ON THE DEVICE (clamped to
 * [0, cap]) — no host synchronisation between the all-gather and the matcher.  Outputs are [world][cap]; row `rank` and the entries beyond
 * the query count are left untouched.  One launch.  Asynchronous. */
int  hs_records_knn2_device(hs_orb* h, const uint8_t* d_records, size_t record_stride, int world, int rank, int cap,
                            int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist, void* stream);

/* ---- the exchange itself in C: an RCCL all-gather of the frame records (north_star: "RCCL all-gather over xGMI of per-frame keypoints /
 * descriptors"; hs_comm.hip).  hs_comm_get_unique_id on ONE rank; the caller carries the 128 bytes to the other ranks over its own channel
 * (file, socket, MPI, ...); every rank then calls hs_comm_create(handle of its GPU, id, world, rank), which blocks until all ranks arrived
 * (ncclCommInitRank).  One process per GPU.  hs_comm_allgather_records enqueues ncclAllGather of `record_bytes` bytes per rank on `stream`
 * (NULL = the handle's stream): d_gathered [world][record_bytes]; in place when d_record == d_gathered + rank * record_bytes.  With the
 * extraction before it and the matcher after it on the same stream a config-5 step needs no event and no host synchronisation.
 * librccl is loaded on first use (dlopen): HS_ERR_NO_DEVICE when it or a GPU is missing.  Asynchronous.
 * hs_comm_available(): non-collective probe (HS_OK / HS_ERR_NO_DEVICE, reason in hs_comm_unavailable_reason()) — ask it on every rank before
 * the first hs_comm_create, which blocks until all ranks arrive, and fall back together when any rank cannot.
 * Lifetime: a communicator BORROWS its handle (device, stream).  The handle is reference-counted (the owner + one per communicator):
 * hs_orb_destroy on a handle that still has communicators only drops the owner's reference and the last hs_comm_destroy frees it, so the two
 * destroy calls are safe in either order and from two threads; the handle must not be used for anything else after its hs_orb_destroy.
 * hs_orb_borrowers() = communicators alive on the handle.  librccl is taken from the directory of the HIP runtime the process runs on (a
 * process may hold two ROCm stacks: PyTorch ships its own libamdhip64 + librccl, and RCCL must match the runtime whose streams it is handed),
 * then by its usual names, and loaded RTLD_LOCAL so that a second copy in the process is left alone. */
#define HS_COMM_ID_BYTES 128
typedef struct hs_comm hs_comm;
int  hs_comm_available(void);
const char* hs_comm_unavailable_reason(void);
int  hs_orb_borrowers(const hs_orb* h);
int  hs_comm_get_unique_id(uint8_t* id /* [HS_COMM_ID_BYTES] */);
int  hs_comm_create(hs_orb* h, const uint8_t* id, int world, int rank, hs_comm** out);
void hs_comm_destroy(hs_comm* c);
int  hs_comm_rccl_ranks(const hs_comm* c);     /* ncclCommCount of the live communicator: what RCCL itself says, -1 = unknown */
int  hs_comm_rccl_rank(const hs_comm* c);      /* ncclCommUserRank, -1 = unknown */
int  hs_comm_rccl_version(void);               /* ncclGetVersion of the librccl in use (e.g. 22203), -1 = not loaded */
int  hs_comm_world(const hs_comm* c);
int  hs_comm_rank(const hs_comm* c);
const char* hs_comm_last_error(const hs_comm* c);
int  hs_comm_allgather_records(hs_comm* c, const void* d_record, void* d_gathered, size_t record_bytes, void* stream);

/* ---- per-stage device timing (HIP events recorded on the stream the kernels run on) ----
 * Stages: 0 pyramid, 1 FAST+NMS cells, 2 quadtree distribution, 3 blur+orient+rBRIEF, 4 stereo match, 5 stereo median.
 * begin: start collecting (events are recorded around every stage of every later call on this handle);
 * pause: stop recording without collecting (later calls run un-instrumented; what was recorded stays for `end`).  A recorded event
 *        drains the stream between two stages (≈5 µs each on MI355X, 28 µs per call): measure on some calls, not on all;
 * end:   synchronise, write the summed milliseconds per stage into ms[6] and the number of launches of each
 *        stage into launches[6] (pyramid counts one launch per call although it is nlevels-1 kernels), stop collecting. */
#define HS_NUM_STAGES 6
/* kernel launches that stage `stage` issued in the last call on the handle (the pyramid is several launches, the stereo match two).  The figure
 * is PER LANE: with hs_orb_set_lanes(h, 2) the second lane enqueues as many again on its own stream.  Between a (re)configuration —
 * hs_orb_reserve, or a call with another frame size or a larger batch — and the next call, stage 0 reports the planned count of the
 * configured geometry's standard plan. */
int  hs_orb_stage_launches(const hs_orb* h, int stage);
int  hs_orb_profile_begin(hs_orb* h);
int  hs_orb_profile_pause(hs_orb* h);
int  hs_orb_profile_end(hs_orb* h, double* ms, int32_t* launches);

/* Measurement utility: streams `bytes` from d_src to d_dst with `width` (4 or 16; 64 = four 16-byte vectors in flight per lane, non-temporal) bytes per lane — a kernel of KNOWN HBM traffic
 * in this library's own access widths, used to calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE counters (tools/pmc_traffic.py). */
int  hs_debug_stream_copy(hs_orb* h, void* d_dst, const void* d_src, size_t bytes, int width, void* stream);

/* Workspace poisoning, a process-wide debug switch for tests (off by default; with it off no call does anything it did not do before).
 * byte in [0, 255] turns it on, -1 off; it may be flipped between calls.  While it is on
 *   - every device allocation the library makes for itself (handle workspaces, the scratch arena, the place database, vocabulary and record-matcher
 *     buffers, hs_device_alloc) is filled with the byte before its first use (synchronously); pinned host memory is not touched;
 *   - every host-pointer entry point fills the part of the handle's scratch arena it claims with the byte before its uploads, and checks after its
 *     kernels that the padding between its staged pieces and the slack behind the last one still hold it.  A changed byte makes the call return
 *     HS_ERR_POISON (the message names the piece and the arena offset of the first changed byte) after its host outputs were copied back as usual,
 *     and counts one violation.  The `_device` forms that take temporaries from the arena are filled too, but never checked: they do not wait.
 * A result that differs between two bytes depends on memory the call never wrote. */
int  hs_debug_poison(int byte);
long long hs_debug_poison_violations(void);      /* violations since the process started */
/* stages two 64-byte pieces and copies 16 bytes just past the end of the first, into its own padding inside the arena: *reported = 1 when the
 * check caught it (one violation is counted).  HS_ERR_INVALID while poisoning is off. */
int  hs_debug_poison_selftest(hs_orb* h, int* reported);

/* ---- stage taps for parity tests (host outputs; synchronous; valid after an extract call) ---- */
/* pyramid level `level` of image `image` of the last batch: tight w*h bytes; ORBExtractor::ComputePyramid :564-589 */
int  hs_orb_debug_level(hs_orb* h, int image, int level, uint8_t* out, size_t cap_bytes, int32_t* lw, int32_t* lh);
/* debug mode: the quadtree stage also gathers the FAST candidates into the dense per-level lists hs_orb_debug_candidates reads (the product path
 * works from the key histogram the FAST kernel leaves and never builds them).  Set before the extraction. */
int  hs_orb_set_debug(hs_orb* h, int on);
/* FAST candidates of that level before DistributeOctTree (unordered): (x,y,score) int32 triplets relative to
 * (16,16); ORBExtractor::ComputeKeyPointsOctTree :430-470 */
int  hs_orb_debug_candidates(hs_orb* h, int image, int level, int32_t* xys, int cap, int32_t* n);
/* keypoints kept by DistributeOctTree for that level, in list order: (x,y,score) level coords; :475-487 */
int  hs_orb_debug_selected(hs_orb* h, int image, int level, int32_t* xys, int cap, int32_t* n);
/* measurement: enqueues the quadtree launch of the last call again, for the levels [level_first, level_first + level_count) alone, `reps` times on
 * the handle's stream, and writes the mean milliseconds per launch (HIP events).  Same inputs, same outputs: the launch only reads what the FAST
 * stage left.  threads: 0 = the instance the call itself used for a single launch of all levels, 256 / 512 = the four- / eight-wave level instance (every
 * level of the range must fit it).  Only after a call that ran without the FAST keys (more frames than HS_FAST_KEYS_MAX_BATCH, or HS_FAST_KEYS=0); synchronous. */
/* (image, level) workgroups of the quadtree kernel's level instance that had to leave its count domain (a node deeper than its histogram pyramid) since
 * the process started or the last reset, on the current device; synchronises the device; -1 on a HIP error */
long long hs_debug_quadtree_level_fallbacks(int reset);
int  hs_orb_debug_quadtree_replay(hs_orb* h, int level_first, int level_count, int threads, int reps, float* ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif

/* orbx.h -- C ABI of the MI355X-native ORB-SLAM2 hot path (liborbx.so).
 *
 * This is the drop-in boundary.  The reference has no plugin
 * registry: its "operator interface" for this path is three C++ class surfaces,
 *   ORB_SLAM2::ORBextractor   /root/reference/include/ORBextractor.h:92-161
 *   ORB_SLAM2::ORBmatcher     /root/reference/include/ORBmatcher.h:57-215
 *   ORB_SLAM2::Optimizer      /root/reference/include/Optimizer.h:112
 * The header-compatible C++ classes in self_commit_orb-slam2_amd/shim/ keep those
 * surfaces and marshal to the functions declared here; INTEGRATION.md shows the
 * binding.  Plain pointers and sizes only; no C++ / torch types.
 *
 * Conventions: every function returns ORBX_OK (0) or a negative ORBX_ERR_* code and
 * never throws; orbx_last_error() returns a thread-local message for the last
 * failure.  There is NO CPU fallback: without a usable HIP device the create
 * functions fail with ORBX_ERR_NODEVICE.  A handle owns one HIP device + stream and
 * its scratch memory; a handle is not re-entrant (like an ORBextractor instance,
 * ORBextractor.h:161) but different handles may be used from different threads
 * (the stereo Frame constructor does exactly that, src/Frame.cc:159-167).
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_OK 0
#define ORBX_ERR_ARG (-1)      /* bad argument                                  */
#define ORBX_ERR_HIP (-2)      /* HIP runtime / kernel failure                  */
#define ORBX_ERR_CAPACITY (-3) /* an internal or caller buffer was too small    */
#define ORBX_ERR_NODEVICE (-4) /* no usable gfx950 device                       */
#define ORBX_ERR_STATE (-5)    /* call sequence error (e.g. results before run) */

const char *orbx_last_error(void);
/* Library/ABI version: major*10000 + minor*100 + patch. */
int orbx_version(void);
/* "<uuid>@<pci address>" of HIP device `device` into identity[capacity >= 64] and the NUMA node of its PCI function (-1 = unknown; may be
 * NULL): what a multi-process run uses to prove that its N ranks sit on N distinct GPUs (bench.py).  Creates no stream. */
int orbx_device_identity(int device, char *identity, int capacity, int *numa_node);

/* ------------------------------------------------------------------------------------
 * ORB extractor  ==  ORB_SLAM2::ORBextractor
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_extractor orbx_extractor;

/* == cv::KeyPoint, 28 bytes (pt.x, pt.y, size, angle, response, octave, class_id). */
typedef struct orbx_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbx_keypoint;

typedef struct orbx_extractor_config {
    /* the five ORBextractor constructor arguments, ORBextractor.h:92 /
     * src/ORBextractor.cc:492-496 (values come from the YAML, src/Tracking.cc:168-192) */
    int nfeatures;
    float scale_factor;
    int nlevels;
    int ini_th_fast;
    int min_th_fast;
    /* sizing of the handle's device buffers */
    int max_width, max_height; /* largest image accepted                          */
    int max_batch;             /* most frames per orbx_extract_batch* call (>=1)  */
    int device;                /* HIP device ordinal                              */
    /* 7-tap fixed-point Gaussian (sum 256) used for cv::GaussianBlur(7x7, sigma 2),
     * src/ORBextractor.cc:1629.  All zero selects the OpenCV 4.x taps
     * 18,34,48,56,48,34,18. */
    uint16_t gauss_taps[7];
    uint16_t reserved_;
} orbx_extractor_config;

/* ORBextractor::ORBextractor (src/ORBextractor.cc:492-609): scale tables, per-level
 * quotas, pattern and umax are built here, device buffers are allocated. */
int orbx_extractor_create(const orbx_extractor_config *cfg, orbx_extractor **out);
void orbx_extractor_destroy(orbx_extractor *h);

/* GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (ORBextractor.h:118-158) + mnFeaturesPerLevel.
 * Any pointer may be NULL; arrays hold nlevels entries. */
int orbx_extractor_tables(const orbx_extractor *h, int *nlevels, float *scale, float *inv_scale,
                          float *sigma2, float *inv_sigma2, int *features_per_level);
/* Upper bound of keypoints one frame can yield: sum over levels of quota+3
 * (octree exit conditions, src/ORBextractor.cc:910,1003). */
/* The same tables without a handle (and without a device): what ORBextractor::ORBextractor computes from
 * (nfeatures, scaleFactor, nlevels) alone (src/ORBextractor.cc:499-554).  Only cfg->nfeatures / scale_factor / nlevels are read.
 * The drop-in constructor uses it so that the getters are valid even when no HIP device can be opened (the reference's
 * constructor cannot fail). */
int orbx_extractor_tables_for(const orbx_extractor_config *cfg, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2,
                              int *features_per_level);
int orbx_extractor_capacity(const orbx_extractor *h);

/* ORBextractor::operator() for one host image WITHOUT the copy into caller arrays: *keypoints / *descriptors point into the
 * handle's pinned result buffer (count entries / count*32 bytes), valid until the next call on this handle.  The drop-in functor
 * (shim/ORBextractor.cc) converts to cv::KeyPoint / cv::Mat straight from there.  Empty image: ORBX_OK, *count = 0. */
int orbx_extract_view(orbx_extractor *h, const uint8_t *image, int width, int height, int stride, const orbx_keypoint **keypoints,
                      const uint8_t **descriptors, int *count);

/* The same call, plus the host copy of the image pyramid the reference keeps in the public member mvImagePyramid
 * (include/ORBextractor.h:161; read by Frame::ComputeStereoMatches, src/Frame.cc:1044,1248,1272,1281): `pyramid` (may be NULL = not
 * wanted) receives VIEWS into the handle's pinned memory - level 0 is the handle's staged copy of the caller's image, levels >= 1
 * arrive with the results of the same launch set (no second transfer, no second wait, no host copy) -, valid until the next call on
 * this handle.  Rows of level l are stride[l] bytes apart. */
#define ORBX_PYRAMID_MAX_LEVELS 12
typedef struct orbx_host_pyramid {
    const uint8_t *level[ORBX_PYRAMID_MAX_LEVELS];
    int width[ORBX_PYRAMID_MAX_LEVELS], height[ORBX_PYRAMID_MAX_LEVELS], stride[ORBX_PYRAMID_MAX_LEVELS];
    int nlevels;
} orbx_host_pyramid;
int orbx_extract_view_pyramid(orbx_extractor *h, const uint8_t *image, int width, int height, int stride, const orbx_keypoint **keypoints,
                              const uint8_t **descriptors, int *count, orbx_host_pyramid *pyramid);

/* Single-frame calls (orbx_extract_view*, orbx_extract, orbx_extract_batch with one frame on a max_batch = 1 handle) that are inside the
 * library at the same moment - from different handles on different threads, same device / configuration / image size - are COMBINED
 * into one launch set on a shared engine (csrc/orbx_extractor.hip: "the combiner"); each call returns exactly what it would have
 * returned alone.  A lone caller never waits for company.  ORBX_COMBINE=0 in the environment gives every handle its own graph instead;
 * ORBX_COMBINE_MAX (16) = most frames per set, ORBX_COMBINE_ENGINES (2) = sets in flight.
 * orbx_extractor_expect_partner: a one-shot hint for the NEXT call on `h` - `partner`'s call is about to arrive (the other extractor
 * thread of the stereo Frame constructor, src/Frame.cc:159-167): with ORBX_COMBINE_PARTNER_US=<us> in the environment the set waits that
 * long for it instead of leaving without it.  Off by default: measured on the reference's constructor, the 30-40 us between its two
 * thread starts cost more than the second launch set saves (the second call simply takes the other engine).
 * orbx_combiner_stats: launch sets and frames served so far for h's configuration (frames / batches = mean set size). */
int orbx_extractor_expect_partner(orbx_extractor *h, orbx_extractor *partner);
int orbx_combiner_stats(const orbx_extractor *h, int64_t *batches, int64_t *frames, int *engines);
/* Microseconds summed so far over h's configuration: us4[0] staging copies (per call), [1] leaders' wait for an engine / for company,
 * [2] graph launch calls, [3] device time + synchronisation (per launch set).  A measurement aid (tools/latency_shim.py). */
int orbx_combiner_profile(const orbx_extractor *h, double *us4);
int orbx_combiner_reset_stats(orbx_extractor *h);
int orbx_combiner_histogram(const orbx_extractor *h, int maxn, int64_t *sets, double *mean_us);   /* sets[n], mean_us[n] for n = 0..maxn frames per launch set */

/* ORBextractor::operator() (ORBextractor.h:110, src/ORBextractor.cc:1544-1668) for one
 * host image.  `keypoints` / `descriptors` hold `capacity` entries / capacity*32 bytes;
 * *count receives the real number (<= orbx_extractor_capacity()).  An empty image
 * (NULL / zero size) returns ORBX_OK with *count = 0 (reference: silent return). */
int orbx_extract(orbx_extractor *h, const uint8_t *image, int width, int height, int stride,
                 orbx_keypoint *keypoints, uint8_t *descriptors, int capacity, int *count);

/* Batched form: `batch` independent frames of identical size.  Frame f writes
 * keypoints[f*capacity ...], descriptors[f*capacity*32 ...], counts[f].
 * Equivalent to `batch` operator() calls; the frames are data-parallel on the GPU.
 * A batch of 2 x ORBX_HOST_BATCH_CHUNK frames (environment, default 64; 0 = never) or more runs as a pipeline over chunks (staging / upload of
 * chunk c+1 and read-back of chunk c-1 under the kernels of chunk c).  The caller's arrays receive the whole batch either way, but after a
 * CHUNKED call the handle's device buffers hold only its last chunk: every "last batch" device-side view below (orbx_batch_results_device,
 * orbx_batch_status_device, orbx_extractor_status, orbx_batch_download, orbx_download_pyramid*, the debug taps, and the matcher / frame-finish
 * entry points that read the extractor's last batch) then returns ORBX_ERR_STATE instead of indexing a chunk.  Callers that want the results on
 * the device use orbx_upload_frames + orbx_extract_batch_device (or set ORBX_HOST_BATCH_CHUNK=0). */
int orbx_extract_batch(orbx_extractor *h, const uint8_t *const *images, int batch, int width,
                       int height, int stride, orbx_keypoint *keypoints, uint8_t *descriptors,
                       int capacity, int *counts);

/* The same call as a two-deep pipeline (SURVEY.md 8b's batch entry point with host pointers; replaces a loop of operator() calls,
 * include/ORBextractor.h:110, src/Frame.cc:394).  _begin stages and uploads the frames (a batch whose frames ALL live in pinned or registered
 * host memory - every byte of every frame, checked per frame - is read in place; one pageable frame and the whole batch is staged), enqueues the batch's launch set and the read-back of its results, and returns without waiting; _end waits
 * for the OLDEST begun batch and fills the caller's arrays exactly like orbx_extract_batch.  Up to two batches may be begun before the first
 * _end: staging + upload of batch i+1 and the read-back of batch i-1 then run under the kernels of batch i.  The images of a batch must stay
 * valid until its _begin returns (pinned / registered images: until its _end returns).  A third _begin, or an _end with nothing begun,
 * returns ORBX_ERR_STATE.  orbx_extract_batch itself runs this pipeline over chunks of its batch (ORBX_HOST_BATCH_CHUNK frames, default 64). */
int orbx_extract_batch_begin(orbx_extractor *h, const uint8_t *const *images, int batch, int width, int height, int stride);
int orbx_extract_batch_end(orbx_extractor *h, orbx_keypoint *keypoints, uint8_t *descriptors, int capacity, int *counts);

/* Device-resident batch: images_dev points to DEVICE memory, frame f at
 * images_dev + f*frame_pitch (rows `stride` bytes apart); the buffer spans batch*frame_pitch
 * bytes.  Runs asynchronously on the handle's stream; results stay in handle-owned device
 * buffers until downloaded.  Rows padded to stride >= round_up(width,4)+12 (and frame_pitch >=
 * stride*height) let the pyramid kernel read aligned windows everywhere (faster); tight rows
 * are handled too. */
int orbx_extract_batch_device(orbx_extractor *h, const void *images_dev, int batch, int width,
                              int height, int stride, size_t frame_pitch);
/* Device pointers of the last batch's results: keypoints[f*cap + i], descriptors
 * [(f*cap + i)*32], counts[f]; *capacity = per-frame capacity of those arrays.  "Last batch" = the last orbx_extract_batch_device /
 * single-frame / un-chunked host call (ORBX_ERR_STATE after a chunked orbx_extract_batch, see there). */
int orbx_batch_results_device(orbx_extractor *h, const orbx_keypoint **keypoints_dev,
                              const uint8_t **descriptors_dev, const int32_t **counts_dev,
                              int *capacity);
/* Wait for the stream and copy the last batch's results to host arrays laid out as
 * in orbx_extract_batch. */
int orbx_batch_download(orbx_extractor *h, int batch, orbx_keypoint *keypoints, uint8_t *descriptors,
                        int capacity, int *counts);
/* Upload host frames into a handle-owned device staging area (returns its device
 * pointer, stride and frame pitch) so callers without their own device allocator
 * (bench.py, tests) can keep inputs resident in HBM. */
int orbx_upload_frames(orbx_extractor *h, const uint8_t *const *images, int batch, int width,
                       int height, int stride, const void **images_dev, int *dev_stride,
                       size_t *dev_frame_pitch);
int orbx_extractor_sync(orbx_extractor *h);
/* Capacity status of the last batch WITHOUT downloading it (a device-resident pipeline never calls orbx_batch_download, which is
 * where a host consumer learns about an overflow): waits for the stream, *bits = OR over the frames of
 *   2 = quadtree node list, 4 = level keypoint buffer (internal invariants: the list never exceeds the level's quota + 3; bit 1,
 *   the former per-level candidate limit, no longer exists - the quadtree's point arrays hold every candidate the detector can emit).
 * 0 = every frame is complete: always, unless an internal invariant is broken; a set bit means the results of that batch are NOT
 * the reference's.  orbx_batch_status_device: the same words on the device, status_dev[f] per frame and
 * status_dev[batch] for the whole batch.  Matcher / frame calls that are chained behind an extractor (`after` argument) pick
 * the batch word up on the device, and their own download calls return ORBX_ERR_CAPACITY when it is set. */
int orbx_extractor_status(orbx_extractor *h, int32_t *bits);
int orbx_batch_status_device(orbx_extractor *h, const int32_t **status_dev, int *batch);

/* std::vector<cv::Mat> mvImagePyramid (ORBextractor.h:161, read by
 * Frame::ComputeStereoMatches, src/Frame.cc:1044,1248,1272,1281): size and bytes of
 * pyramid level `level` of frame `frame` of the last call.  blurred=1 returns the
 * Gaussian-blurred copy the descriptors were sampled from (src/ORBextractor.cc:1626-1634). */
/* Every level of frame `frame` of the last call in one device->host transfer: dst[l] receives level l (rows dst_strides[l] bytes
 * apart), l = 0..nlevels-1.  This is what refills the public mvImagePyramid member in shim/ORBextractor.cc. */
int orbx_download_pyramid_all(orbx_extractor *h, int frame, uint8_t *const *dst, const int *dst_strides, int nlevels);
int orbx_pyramid_level_size(const orbx_extractor *h, int width, int height, int level, int *w, int *hgt);
int orbx_download_pyramid(orbx_extractor *h, int frame, int level, int blurred, uint8_t *dst, int dst_stride);

/* Stage taps for the parity tests: FAST score map of a level
 * (0 = not a corner at minThFAST), the per-level candidate list in vToDistributeKeys
 * order (src/ORBextractor.cc:1089-1157) packed as x | y<<12 | score<<24 relative to the
 * border window origin, and the per-level keypoints after DistributeOctTree + IC_Angle
 * in level coordinates (src/ORBextractor.cc:1167-1198). */
/* The fused detector keeps FAST scores on chip; enable the taps to also write the score map. */
int orbx_extractor_set_debug_taps(orbx_extractor *h, int enable);
int orbx_debug_download_scores(orbx_extractor *h, int frame, int level, uint8_t *dst, int dst_stride);
int orbx_debug_download_candidates(orbx_extractor *h, int frame, int level, uint32_t *packed, int cap, int *count);
int orbx_debug_download_level_keypoints(orbx_extractor *h, int frame, int level, orbx_keypoint *kps, int cap, int *count);

/* Kernel timing measured with HIP events on the handle's own stream: average milliseconds
 * per stage (order given by orbx_stage_name(i)) and their sum, over the batch calls issued
 * since profiling was enabled (at most the last 64).  Every call keeps its own event set,
 * so nothing is synchronised inside a timed region; reading waits for the stream. */
#define ORBX_MAX_STAGES 16
int orbx_extractor_set_profiling(orbx_extractor *h, int enable);
int orbx_extractor_last_timing(orbx_extractor *h, float *total_ms, float *stage_ms, int *nstages);
const char *orbx_stage_name(int stage);


/* ------------------------------------------------------------------------------------
 * ORB matcher  ==  the Hamming paths of ORB_SLAM2::ORBmatcher (+ the Hamming stage of
 * Frame::ComputeStereoMatches).  The reference walks KeyFrame / MapPoint / Frame objects;
 * the C ABI takes the same information as flat arrays (INTEGRATION.md shows the
 * marshalling the class shim does).
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_matcher orbx_matcher;

/* ORBmatcher::DescriptorDistance (ORBmatcher.h:65, src/ORBmatcher.cc:1913-1933): 256-bit
 * Hamming distance of two 32-byte descriptors (host helper, used by the class shim). */
int orbx_descriptor_distance(const uint8_t *a, const uint8_t *b);

/* Features of `nframes` frames, frame f at index f*capacity.  Device OR host pointers,
 * depending on the function. */
typedef struct orbx_feature_set {
    const orbx_keypoint *keypoints; /* angle/x/y/octave are read (mvKeys / mvKeysUn)             */
    const uint8_t *descriptors;     /* 32 bytes per feature (mDescriptors)                       */
    const int32_t *counts;          /* features per frame (N)                                    */
    const int32_t *groups;          /* DBoW2 node id per feature (FeatureVector, src/Frame.cc:889-892);
                                       negative = the feature is not filed in the FeatureVector and
                                       is never matched; NULL = every feature in one node = brute force */
    const uint8_t *valid;           /* 1 = feature has a non-bad MapPoint (src/ORBmatcher.cc:268-274);
                                       NULL = all valid                                          */
    int capacity;
    int nframes;
} orbx_feature_set;

typedef struct orbx_bow_params {
    float nn_ratio;        /* mfNNratio  (ORBmatcher.h:57; 0.7 at src/Tracking.cc:1189)          */
    int check_orientation; /* mbCheckOrientation                                                 */
    int mode;              /* 0: SearchByBoW(KeyFrame*,Frame&,...)     src/ORBmatcher.cc:230-382,
                                 result indexed by the Frame feature (value = KeyFrame feature)
                              1: SearchByBoW(KeyFrame*,KeyFrame*,...)  src/ORBmatcher.cc:656-799,
                                 result indexed by the KF1 feature (value = KF2 feature)         */
} orbx_bow_params;

int orbx_matcher_create(int device, int max_features, int max_pairs, orbx_matcher **out);
void orbx_matcher_destroy(orbx_matcher *m);

/* SearchByBoW for `npairs` independent (A frame, B frame) pairs; A plays the KeyFrame.
 * a/b hold DEVICE pointers; pairs_a/pairs_b are host arrays of frame indices.  Asynchronous
 * on the matcher's stream (which first waits for `after_stream_of`, an extractor whose
 * outputs are being consumed; may be NULL).
 * Chaining contract (every call that takes `after_stream_of`, and orbx_compute_stereo_matches_device
 * for its two extractors): the extractor double-buffers its results, so the batch extracted NEXT
 * leaves what this call reads alone and the one after that waits for this call before it
 * overwrites the buffer; a/b must be the pointers orbx_batch_results_device returned AFTER the
 * batch being consumed (they alternate from batch to batch).  Any number of matcher handles may
 * be chained behind the same batch, in any order: the extractor waits for every one of them, not
 * only for the last.  A call that is not chained (NULL) is ordered by the caller
 * (orbx_extractor_sync before it, orbx_matcher_sync before the extractor's next batch but one).
 * Results stay on the device:
 *   matches[p*stride + slot] = index of the matched feature in the other set or -1,
 *   dists[p*stride + slot]   = Hamming distance of that match,
 *   nmatches[p]              = return value of SearchByBoW.
 * The Hamming distances are XOR + population count on the vector ALUs (DescriptorDistance, src/ORBmatcher.cc:1913-1933).  Environment
 * ORBX_MATCH_MFMA=1 (read per call) takes the candidate lists of the unfiltered case - no node ids, no validity mask - from the matrix
 * cores instead (v_mfma_i32_32x32x32_i8 on +-1 / 0-1 bytes: bit-identical results); a measured alternative, not the default.            */
int orbx_search_by_bow_device(orbx_matcher *m, const orbx_feature_set *a, const orbx_feature_set *b,
                              const int32_t *pairs_a, const int32_t *pairs_b, int npairs,
                              const orbx_bow_params *params, orbx_extractor *after_stream_of);

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
 * (src/ORBmatcher.cc:810-1017; LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:332).  The
 * feature sets are the two KeyFrames: keypoints = mvKeysUn, groups = mFeatVec node ids,
 * valid = 1 where the feature may be matched: it has NO MapPoint and, when bOnlyStereo, mvuRight >= 0
 * (:845-855, 867-876).  Acceptance per KF1 feature, in FeatureVector order: among the still unmatched
 * KF2 features of its node with dist <= TH_LOW that pass the epipole gate (:888-895, both monocular)
 * and CheckDistEpipolarLine (:188-227), the smallest distance, the LAST one among equals (:880);
 * then the rotation histogram.  matches[p*stride + i] = KF2 feature of KF1 feature i or -1
 * (vMatchedPairs = the non-negative entries in ascending i), nmatches[p] = return value. */
typedef struct orbx_triangulation_params {
    const float *f12;           /* HOST [9*npairs]: F12 row-major as LocalMapping::ComputeF12 returns it   */
    const float *epipole;       /* HOST [2*npairs]: ex, ey = KF1's centre projected into KF2 (:817-826)    */
    const uint8_t *stereo_a;    /* pKF1->mvuRight[i] >= 0, laid out like set a (device pointer in the
                                   _device form, host pointer in the host form); NULL = monocular          */
    const uint8_t *stereo_b;    /* same for pKF2                                                           */
    const float *scale_factors; /* HOST pKF2->mvScaleFactors[nlevels]                                      */
    const float *level_sigma2;  /* HOST pKF2->mvLevelSigma2[nlevels]                                       */
    int nlevels;
    int check_orientation;      /* mbCheckOrientation                                                      */
} orbx_triangulation_params;
int orbx_search_for_triangulation_device(orbx_matcher *m, const orbx_feature_set *a, const orbx_feature_set *b,
                                         const int32_t *pairs_a, const int32_t *pairs_b, int npairs,
                                         const orbx_triangulation_params *params, orbx_extractor *after_stream_of);
/* Host-array form for one KeyFrame pair (upload, run, download): matches12[a->counts[0]]. */
int orbx_search_for_triangulation(orbx_matcher *m, const orbx_feature_set *a_host, const orbx_feature_set *b_host,
                                  const orbx_triangulation_params *params_host, int32_t *matches12, int32_t *nmatches);

/* Hamming stage of Frame::ComputeStereoMatches (src/Frame.cc:1041-1216) for `npairs`
 * (left frame, right frame) pairs: per left keypoint the right keypoint of minimum
 * descriptor distance among those in its row band (+-2*scale[octave]), within one octave and
 * with uR in [uL - max_disparity, uL].  dists = bestDist (TH_HIGH=100 when none),
 * matches = bestIdxR (0 when none), nmatches[p] = #left keypoints with bestDist < 75.       */
int orbx_stereo_match_device(orbx_matcher *m, const orbx_feature_set *left, const orbx_feature_set *right,
                             const int32_t *pairs_l, const int32_t *pairs_r, int npairs,
                             const float *scale_factors, int nlevels, float max_disparity,
                             orbx_extractor *after_stream_of);

/* Complete Frame::ComputeStereoMatches (src/Frame.cc:1026-1420) for `npairs` (left frame, right
 * frame) pairs taken from the LAST batches of two extractor handles (the reference's
 * mpORBextractorLeft / mpORBextractorRight; both may be the same handle when left and right
 * frames were extracted in one batch): Hamming stage as orbx_stereo_match_device, then the 11x11
 * SAD search over +-5 px on the keypoint's pyramid level (the extractor's device-resident
 * mvImagePyramid), parabola sub-pixel fit, disparity gate and the median*1.5*1.4 outlier cut.
 *   uright[p*stride + iL] = mvuRight[iL] (-1: no match), depth[...] = mvDepth[iL],
 *   nmatches[p] = number of left keypoints with a depth; matches/dists = bestIdxR/bestDist.
 * mbf = Frame::mbf, mb = Frame::mb AS IT IS when ComputeStereoMatches runs: 0 in this fork's
 * stereo constructor (src/Frame.cc:125, mb is assigned at :197 after the call) => maxD = +inf.
 * Asynchronous on the matcher's stream, ordered after both extractors; the extractors' next
 * batch waits for it before their pyramids are overwritten. */
int orbx_compute_stereo_matches_device(orbx_matcher *m, orbx_extractor *left, orbx_extractor *right,
                                       const int32_t *frames_l, const int32_t *frames_r, int npairs, float mbf,
                                       float mb);
int orbx_stereo_results_device(orbx_matcher *m, const float **uright_dev, const float **depth_dev, int *stride);
int orbx_stereo_download(orbx_matcher *m, int npairs, float *uright, float *depth, int stride);
/* Frame::ComputeStereoMatches (src/Frame.cc:1026-1420) for ONE stereo frame whose left / right image were extracted by the two
 * extractors' last single-frame calls (orbx_extract_view* / orbx_extract: the stereo Frame constructor, src/Frame.cc:159-168):
 * uright[i] / depth[i] = mvuRight / mvDepth of left keypoint i, i < n.  Synchronous; the latency form of
 * orbx_compute_stereo_matches_device + orbx_stereo_download (same kernels, three launches and one wait instead of ~22 runtime calls). */
int orbx_stereo_frame(orbx_matcher *m, orbx_extractor *left, orbx_extractor *right, float mbf, float mb, float *uright, float *depth, int n);
/* The same call in two halves: _begin launches and returns at once, _end waits and copies mvuRight / mvDepth out.  Neither extractor may
 * be called in between.  shim/Frame_hip.cc begins on the extractor thread that finishes last in the stereo constructor (src/Frame.cc:
 * 159-167), before that thread converts its keypoints, and ends in Frame::ComputeStereoMatches (:168): the match runs while the host
 * fills mvKeysRight and joins the threads. */
int orbx_stereo_frame_begin(orbx_matcher *m, orbx_extractor *left, orbx_extractor *right, float mbf, float mb);
int orbx_stereo_frame_end(orbx_matcher *m, float *uright, float *depth, int n);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th)
 * (ORBmatcher.h, src/ORBmatcher.cc:70-175; called by Tracking::SearchLocalPoints, src/Tracking.cc:1616)
 * including Frame::GetFeaturesInArea and the 64x48 feature grid (src/Frame.cc:741-877).
 * The Frame side is passed as arrays of the frame's members, the MapPoint side as what
 * Frame::isInFrustum left in every MapPoint.  Feature i of frame f at f*capacity + i. */
typedef struct orbx_projection_frame {
    const orbx_keypoint *keypoints_un; /* mvKeysUn                                                   */
    const uint8_t *descriptors;        /* mDescriptors                                               */
    const float *u_right;              /* mvuRight (<= 0: no stereo coordinate)                      */
    const uint8_t *occupied;           /* 1 = mvpMapPoints[i] holds a MapPoint with Observations()>0
                                          (src/ORBmatcher.cc:110-112); NULL = none                   */
    const int32_t *counts;             /* N per frame                                                */
    int capacity, nframes;
    float min_x, min_y;                /* Frame::mnMinX, mnMinY                                      */
    float grid_width_inv, grid_height_inv; /* Frame::mfGridElementWidthInv / HeightInv              */
} orbx_projection_frame;

typedef struct orbx_projection_points {
    const float *proj_x, *proj_y, *proj_xr; /* MapPoint::mTrackProjX / mTrackProjY / mTrackProjXR    */
    const int32_t *scale_level;        /* mnTrackScaleLevel                                          */
    const float *view_cos;             /* mTrackViewCos                                              */
    const uint8_t *in_view;            /* mbTrackInView && !isBad()                                  */
    const uint8_t *has_observations;   /* Observations()>0: the point blocks its feature for the
                                          points that follow; NULL = all                             */
    const uint8_t *descriptors;        /* GetDescriptor(), 32 bytes                                  */
    const int32_t *counts;             /* points per frame                                           */
    int capacity;
} orbx_projection_points;

/* Device-pointer form for `frame->nframes` independent (frame, point list) problems (the replay keeps 6 bytes of LDS
 * per feature slot: frame->capacity <= 27000, ORBX_ERR_CAPACITY beyond); results:
 * matches[f*stride + i] = index of the point written into F.mvpMapPoints[i] by the call or -1,
 * nmatches[f] = return value (orbx_matcher_results_device / orbx_matcher_download). */
int orbx_search_by_projection_device(orbx_matcher *m, const orbx_projection_frame *frame,
                                     const orbx_projection_points *points, const float *scale_factors, int nlevels,
                                     float th, float nn_ratio);
/* Host-array form for one frame (counts[0] entries each): upload, run, download. */
int orbx_search_by_projection(orbx_matcher *m, const orbx_projection_frame *frame_host,
                              const orbx_projection_points *points_host, const float *scale_factors, int nlevels,
                              float th, float nn_ratio, int32_t *assigned, int32_t *nmatches);

/* Frame::isInFrustum(pMP, viewingCosLimit) (reference src/Frame.cc:608-742) for a list of map points per frame: the
 * loop of Tracking::SearchLocalPoints (src/Tracking.cc:1580-1613) that prepares SearchByProjection(F, vpMapPoints, th).
 * Outputs are laid out like orbx_projection_points (point i of frame f at f*capacity + i), so that
 * orbx_frustum_results_device feeds orbx_search_by_projection_device without a host round trip:
 * in_view = mbTrackInView, proj_x / proj_y / proj_xr = mTrackProjX / Y / XR, scale_level = mnTrackScaleLevel,
 * view_cos = mTrackViewCos (only written where in_view). */
typedef struct orbx_frustum_frame {
    const float *tcw;                 /* [16] per frame: mTcw row-major (mRcw, mtcw, mOw follow as in Frame::UpdatePoseMatrices) */
    float fx, fy, cx, cy, mbf;        /* Frame statics                                                             */
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY                                                          */
    const float *ratio_thresholds;    /* HOST [nlevels-1] from orbx_predict_scale_thresholds(mfLogScaleFactor, ..) */
    int nlevels;                      /* mnScaleLevels                                                             */
    int nframes;
} orbx_frustum_frame;
typedef struct orbx_map_points {
    const float *world_pos;     /* [3] GetWorldPos()                                                                */
    const float *normal;        /* [3] GetNormal()                                                                  */
    const float *max_distance;  /* mfMaxDistance (GetMaxDistanceInvariance()/1.2f)                                  */
    const float *min_distance;  /* mfMinDistance                                                                    */
    const int32_t *counts;      /* points per frame                                                                 */
    int capacity;
} orbx_map_points;
/* MapPoint::PredictScale (src/MapPoint.cc:571-586) without a device logarithm: thresholds[k] = the largest float ratio
 * mfMaxDistance/dist that the reference's ceil(log(ratio)/mfLogScaleFactor) still maps to level <= k (k = 0..nlevels-2),
 * tabulated on the host with the libm log the reference itself calls. */
int orbx_predict_scale_thresholds(float log_scale_factor, int nlevels, float *thresholds);
int orbx_is_in_frustum_device(orbx_matcher *m, const orbx_frustum_frame *frame, const orbx_map_points *points,
                              float viewing_cos_limit);
int orbx_frustum_results_device(orbx_matcher *m, const float **proj_x, const float **proj_y, const float **proj_xr,
                                const int32_t **scale_level, const float **view_cos, const uint8_t **in_view);
/* Host-array form for one frame (points->counts[0] points). */
int orbx_is_in_frustum(orbx_matcher *m, const orbx_frustum_frame *frame_host, const orbx_map_points *points_host,
                       float viewing_cos_limit, float *proj_x, float *proj_y, float *proj_xr, int32_t *scale_level,
                       float *view_cos, uint8_t *in_view);

/* Tracking::SearchLocalPoints (src/Tracking.cc:1760-1830) as ONE device chain for one frame: Frame::isInFrustum over the local
 * map points (src/Frame.cc:608-742, the loop at src/Tracking.cc:1791-1811) feeding ORBmatcher::SearchByProjection(Frame&,
 * vector<MapPoint*>&, th) (src/ORBmatcher.cc:70-175; :1828) without the mTrack* fields ever visiting the host: one upload of the
 * frame side, the pose and the points' map data, k_is_in_frustum -> k_proj_topk -> k_proj_greedy, one read-back.
 * `points_host` lists the points the reference's loop would test (not yet seen in this frame, not bad), in list order.
 * Outputs: assigned[i] (frame->counts[0] entries) = index of the point written into F.mvpMapPoints[i] or -1, *nmatches = the
 * search's return value; per point the fields Frame::isInFrustum leaves in the MapPoint: in_view = mbTrackInView (= the function's
 * return value: IncreaseVisible() / nToMatch bookkeeping is the caller's), proj_x / proj_y / proj_xr / scale_level / view_cos
 * (written where in_view; any of the five may be NULL). */
typedef struct orbx_local_points {
    const float *world_pos;          /* [3] GetWorldPos()                                   */
    const float *normal;             /* [3] GetNormal()                                     */
    const float *max_distance;       /* mfMaxDistance                                       */
    const float *min_distance;       /* mfMinDistance                                       */
    const uint8_t *descriptors;      /* GetDescriptor(), 32 bytes                           */
    const uint8_t *has_observations; /* Observations()>0; NULL = all                        */
    int count;
} orbx_local_points;
int orbx_search_local_points(orbx_matcher *m, const orbx_projection_frame *frame_host, const orbx_frustum_frame *pose_host,
                             const orbx_local_points *points_host, const float *scale_factors, int nlevels,
                             float viewing_cos_limit, float th, float nn_ratio, int32_t *assigned, int32_t *nmatches,
                             uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr, int32_t *scale_level,
                             float *view_cos);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th,
 * const bool bMono) (src/ORBmatcher.cc:1569-1728; Tracking::TrackWithMotionModel,
 * src/Tracking.cc:1433-1441).  Last-frame side, feature i of frame f at f*capacity + i: */
typedef struct orbx_projection_last {
    const uint8_t *valid;            /* 1 = LastFrame.mvpMapPoints[i] != NULL && !mvbOutlier[i]             */
    const float *world_pos;          /* [3] MapPoint::GetWorldPos()                                         */
    const uint8_t *descriptors;      /* MapPoint::GetDescriptor(), 32 bytes                                 */
    const uint8_t *has_observations; /* Observations()>0; NULL = all                                        */
    const int32_t *octave;           /* LastFrame.mvKeys[i].octave                                          */
    const float *angle;              /* LastFrame.mvKeysUn[i].angle                                         */
    const int32_t *counts;           /* LastFrame.N per frame                                               */
    int capacity;
    const float *tcw_current;        /* [16] per frame: CurrentFrame.mTcw, row-major                        */
    const float *tcw_last;           /* [16] per frame: LastFrame.mTcw                                      */
    float fx, fy, cx, cy, mbf, mb;   /* CurrentFrame.fx .. mb                                               */
    float max_x, max_y;              /* Frame::mnMaxX, mnMaxY (min_x/min_y are in orbx_projection_frame)    */
} orbx_projection_last;
/* matches[f*stride + i2] = last-frame feature whose MapPoint ends up in CurrentFrame.mvpMapPoints[i2],
 * -1 = the call did not touch the feature, -2 = assigned and then cleared by the rotation-histogram
 * pruning (the reference stores NULL there, :1718); nmatches[f] = return value. */
int orbx_search_by_projection_last_device(orbx_matcher *m, const orbx_projection_frame *frame,
                                          const orbx_projection_last *last, const float *scale_factors, int nlevels,
                                          float th, int b_mono, int check_orientation);
int orbx_search_by_projection_last(orbx_matcher *m, const orbx_projection_frame *frame_host,
                                   const orbx_projection_last *last_host, const float *scale_factors, int nlevels,
                                   float th, int b_mono, int check_orientation, int32_t *assigned, int32_t *nmatches);

/* ------------------------------------------------------------------------------------
 * A tracked frame on the device: the two functions of the tracking thread that run on EVERY frame, each as one
 * launch chain with ONE host wait (inputs staged once through mapped pinned memory, results written by the chain's last
 * kernel into mapped pinned memory, a sequence word polled).  Both live on the matcher handle; host memory throughout.
 *
 * Limits of both: at most ORBX_TRACK_MAX_CORRESPONDENCES possible correspondences (the pose kernel keeps a frame's edges
 * in the registers of one workgroup) - for the motion model min(N, valid last-frame points), for the local map
 * min(N, held features + local points); N <= the matcher's max_features; the replays' LDS tiles (5 / 6 bytes per
 * feature: N <= 32000 / 27000).  ORBX_ERR_CAPACITY beyond, ORBX_ERR_ARG for NULL arguments or nlevels out of range;
 * neither launches anything.
 *
 * orbx_track_with_motion_model == Tracking::TrackWithMotionModel, src/Tracking.cc:1370-1421 (UpdateLastFrame, the
 * velocity product - last->tcw_current = mVelocity * mLastFrame.mTcw - and the final mbOnlyTracking decision stay the
 * caller's):
 *   SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1382); if it returns < 20, again with 2 * th from cleared
 *   matches (:1386-1390; enqueued unconditionally, its workgroups read the first pass' count on the device and leave
 *   unless it is < 20); if still < 20 the function fails (:1393): ran_pose = 0, pose = tcw_current unchanged, matches as
 *   the search left them, nmatches = nmatches_search, nmatches_map = 0.  Otherwise a gather kernel builds the pose
 *   problem on the device from the pass that counts (features i in ascending order with a match >= 0: the last-frame
 *   point's world_pos, keypoints_un[i].pt, u_right[i], inv_level_sigma2[keypoints_un[i].octave]), PoseOptimization
 *   (:1398) runs from tcw_current with camera fx, fy, cx, cy, mbf, and a discard kernel does :1403-1421.
 * Results (N = frame->counts[0] entries; any pointer may be NULL):
 *   matches[i]        last-frame feature whose MapPoint CurrentFrame.mvpMapPoints[i] holds on return, or -1
 *   search_matches[i] as orbx_search_by_projection_last reports the pass that counted (-2 = assigned, then pruned)
 *   discarded[i]      1 where :1409-1415 fired (the caller sets mbTrackInView = false, mnLastFrameSeen on that point)
 *   pose[16]          mTcw after PoseOptimization
 *   counts            nmatches_search (the search's return value), wide (1 = the 2 * th pass counted),
 *                     n_correspondences, pose_inliers (PoseOptimization's return value), nmatches (after the decrements
 *                     of :1415), nmatches_map (:1417-1419), ran_pose
 *   stats[8]          as orbx_pose_optimization
 * Contract: every field equals, bit for bit, orbx_search_by_projection_last (once or twice) followed by
 * orbx_pose_optimization on the problem a host loop builds from its result; against the CPU restatement the pose is
 * held to 1e-5 and everything else is equal (orbx_pose_optimization's own contract). */
#define ORBX_TRACK_MAX_CORRESPONDENCES 8192
typedef struct orbx_track_motion_result {
    int32_t *matches, *search_matches;
    uint8_t *discarded;
    float *pose;
    int32_t nmatches_search, wide, n_correspondences, pose_inliers, nmatches, nmatches_map, ran_pose;
    double stats[8];
} orbx_track_motion_result;
int orbx_track_with_motion_model(orbx_matcher *m, const orbx_projection_frame *frame_host, const orbx_projection_last *last_host,
                                 const float *scale_factors, int nlevels, const float *inv_level_sigma2, float th, int b_mono,
                                 int check_orientation, orbx_track_motion_result *result);

/* orbx_track_local_map == Tracking::TrackLocalMap, src/Tracking.cc:1454-1489 (UpdateLocalMap and the bookkeeping loop
 * of SearchLocalPoints over the points the frame already holds, :1770-1788, stay the caller's):
 *   orbx_search_local_points' chain (Frame::isInFrustum + SearchByProjection(F, vpMapPoints, th)), a gather kernel - the
 *   edges are the features in ascending order that are held (held[i] = 1: mvpMapPoints[i] != NULL on entry) or newly
 *   assigned; world position from the local point if assigned, else held_world_pos[i] -, PoseOptimization (:1459) from
 *   pose->tcw, and a statistics kernel for :1464-1489.
 * Inputs as orbx_search_local_points plus held[N], held_world_pos[N*3], inv_level_sigma2[nlevels], sensor_stereo
 * (mSensor == System::STEREO).  frame->occupied[i] = 1 where the held point has Observations() > 0 (NULL = none).
 * Results (any pointer may be NULL): assigned / nmatches / in_view / proj_x .. view_cos as orbx_search_local_points;
 *   pose[16]; outlier[N] = mvbOutlier of the features with an edge (0 elsewhere: the function does not touch those);
 *   found[N] = 1: IncreaseFound() is due (:1469-1471); cleared[N] = 1: outlier under sensor_stereo, mvpMapPoints[i]
 *   becomes NULL (:1485-1486); pose_inliers; inliers_map = non-outliers with Observations() > 0 (occupied for a held
 *   feature, the point's has_observations for a new one): mnMatchesInliers unless mbOnlyTracking; inliers_all =
 *   mnMatchesInliers under mbOnlyTracking; n_correspondences; stats[8].
 * Contract: as above, against orbx_search_local_points followed by orbx_pose_optimization. */
typedef struct orbx_track_local_result {
    int32_t *assigned;
    uint8_t *in_view;
    float *proj_x, *proj_y, *proj_xr;
    int32_t *scale_level;
    float *view_cos;
    float *pose;
    uint8_t *outlier, *found, *cleared;
    int32_t nmatches, n_correspondences, pose_inliers, inliers_map, inliers_all;
    double stats[8];
} orbx_track_local_result;
int orbx_track_local_map(orbx_matcher *m, const orbx_projection_frame *frame_host, const orbx_frustum_frame *pose_host,
                         const orbx_local_points *points_host, const float *scale_factors, int nlevels, float viewing_cos_limit,
                         float th, float nn_ratio, const uint8_t *held, const float *held_world_pos, const float *inv_level_sigma2,
                         int sensor_stereo, orbx_track_local_result *result);

/* orbx_track_reference_keyframe == Tracking::TrackReferenceKeyFrame, src/Tracking.cc:1189-1238, the third way to a first
 * pose (after initialisation, after a relocalisation, when the motion model fails).  ComputeBoW (:1185: the frame's
 * `groups` are an input, as for orbx_search_by_bow) and the pose handed to SetPose (mLastFrame.mTcw, :1206) stay the
 * caller's, as does the final nmatchesMap >= 10 (:1238).
 *   SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches) (:1195; ORBmatcher(0.7, true): nn_ratio and
 *   check_orientation are parameters) with the launches of orbx_search_by_bow's single-pair path; if it returns < 15 the
 *   function fails (:1201): ran_pose = 0, pose = tcw unchanged, matches as the search left them, nmatches =
 *   nmatches_search, nmatches_map = 0.  Otherwise a gather kernel builds the pose problem on the device (frame features i
 *   in ascending order with a match: the keyframe's world_pos at the matched slot, keypoints_un[i].pt, u_right[i],
 *   inv_level_sigma2[keypoints_un[i].octave]), PoseOptimization (:1209) runs from tcw with camera fx, fy, cx, cy, mbf, and
 *   the discard kernel does :1215-1236 (the keyframe's has_observations in the place of the last frame's).
 * keyframe->features: mvKeysUn, mDescriptors, groups = mFeatVec node ids, valid = the slot holds a non-bad MapPoint (NULL
 *   = all); frame->features: mvKeys (the angle is read, src/ORBmatcher.cc:320), mDescriptors, groups (NULL on both sides =
 *   brute force); its `valid` is not read.
 * Results (N = frame->features->counts[0] entries; any pointer may be NULL): the fields of orbx_track_motion_result
 *   without `wide`; matches / search_matches name KEYFRAME SLOTS (search_matches = what orbx_search_by_bow returns: a match
 *   pruned by the rotation histogram is -1 there).  discarded[i] = 1: the caller sets mbTrackInView = false and
 *   mnLastFrameSeen on that point (:1227-1228).
 * Limits: ORBX_TRACK_MAX_CORRESPONDENCES possible correspondences (min(N, valid keyframe slots)); N <= 4000 (the frame
 *   sits in the pair kernel's LDS, the bound orbx_search_by_bow tests before it takes its single-pair path) and both
 *   counts <= max_features; the replay's tile 4 N + 8 nA <= 160 KB.  ORBX_ERR_CAPACITY beyond, ORBX_ERR_ARG for NULL
 *   arguments or nlevels outside 1..64; neither stages or launches anything.  An empty frame or keyframe: the failure
 *   result, no launch.
 * Contract: every field equals, bit for bit, orbx_search_by_bow (mode 0) followed by orbx_pose_optimization on the
 * problem a host loop builds from its result and the host's discard loop; against the CPU restatement the pose is held
 * to 1e-5 and everything else is equal. */
typedef struct orbx_reference_keyframe {   /* host memory */
    const orbx_feature_set *features;
    const float *world_pos;                /* [nA*3] MapPoint::GetWorldPos of the slot's point (read where a match lands)  */
    const uint8_t *has_observations;       /* [nA] Observations() > 0 of the slot's point; NULL = all                      */
} orbx_reference_keyframe;
typedef struct orbx_reference_frame {      /* host memory */
    const orbx_feature_set *features;
    const orbx_keypoint *keypoints_un;     /* [N] mvKeysUn: pt and octave are read                                         */
    const float *u_right;                  /* [N] mvuRight                                                                 */
    const float *tcw;                      /* [16] the pose PoseOptimization starts from (mLastFrame.mTcw)                 */
    float fx, fy, cx, cy, mbf;
    const float *inv_level_sigma2;         /* mvInvLevelSigma2 [nlevels]                                                   */
    int nlevels;
} orbx_reference_frame;
typedef struct orbx_track_reference_result {
    int32_t *matches, *search_matches;
    uint8_t *discarded;
    float *pose;
    int32_t nmatches_search, n_correspondences, pose_inliers, nmatches, nmatches_map, ran_pose;
    double stats[8];
} orbx_track_reference_result;
int orbx_track_reference_keyframe(orbx_matcher *m, const orbx_reference_keyframe *keyframe_host, const orbx_reference_frame *frame_host,
                                  float nn_ratio, int check_orientation, orbx_track_reference_result *result);

/* orbx_reloc_match_candidates == the head of Tracking::Relocalization, src/Tracking.cc:2063-2095, without the
 * `new PnPsolver` itself: SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[k]) for ALL K candidate keyframes, the < 15
 * decision (:2075) and the arrays the PnPsolver constructor collects (src/PnPsolver.cc:120-167), as one launch chain with
 * ONE host wait.  It sits between orbx_kfdb_query and orbx_pnp_solve / orbx_relocalize_refine, which already take all
 * candidates in one call.  The frame is staged ONCE.
 *   A K-pair form of the single-pair distance kernel (candidate on the grid's y; a keyframe feature per wave, the frame
 *   split over 64 lanes and held in LDS; every candidate's processing order in the same launch), the greedy replay with K
 *   workgroups, and a gather kernel with one workgroup per candidate.  A bad keyframe (:2066) is staged with zero
 *   features: its workgroups leave at once.
 * frame: features as orbx_reference_frame (mvKeys, mDescriptors, groups), keypoints_un, level_sigma2 = mvLevelSigma2.
 * keyframes[k]: features (valid = the slot holds a non-bad MapPoint; groups on every keyframe or on none), world_pos,
 *   is_bad.
 * Results (host arrays, row k at k * N, N = the frame's features; any pointer may be NULL):
 *   matches[K][N]     keyframe slot or -1: the vvpMapPointMatches rows as the searches left them, also for a candidate
 *                     that is discarded for < 15 matches (all -1 for a bad keyframe)
 *   nmatches[K]       the searches' return values (0 for a bad keyframe)
 *   discarded[K]      vbDiscarded: bad, or nmatches < 15
 *   n[K]              kept matches of the PnP problem (= nmatches), 0 for a discarded candidate
 *   key_index[K][N], p2d[K][N][2], sigma2[K][N], p3dw[K][N][3]: the first n[k] entries of row k are mvKeyPointIndices,
 *                     mvP2D, mvSigma2 = level_sigma2[octave] and mvP3Dw in ascending feature order - the layout
 *                     orbx_pnp_problem takes; the rest of a row, and the whole row of a discarded candidate, is not
 *                     written.
 * The host still draws the RANSAC sets from n[k] and calls orbx_pnp_solve with these host arrays.  Handing the arrays to
 * the PnP handle in device memory is OUT OF SCOPE here: they cross to the host once and back.
 * Limits, per candidate, as orbx_track_reference_keyframe (N <= 4000, counts <= max_features, the replay's tile for the
 * largest candidate); K <= the handle's max_pairs.  ORBX_ERR_CAPACITY beyond; ORBX_ERR_ARG for NULL arguments, K < 1,
 * nlevels outside 1..64 or groups on some keyframes only; neither stages or launches anything.  An empty frame, or no
 * candidate with a feature: every candidate discarded, no launch.
 * Contract: every matches row and nmatches equals orbx_search_by_bow(kf_k, frame) (mode 0) and the arrays equal the
 * constructor's loop over that row, float bits included. */
typedef struct orbx_reloc_match_frame {    /* host memory */
    const orbx_feature_set *features;
    const orbx_keypoint *keypoints_un;     /* [N] mvKeysUn                                                                 */
    const float *level_sigma2;             /* mvLevelSigma2 [nlevels]                                                      */
    int nlevels;
} orbx_reloc_match_frame;
typedef struct orbx_reloc_match_keyframe { /* host memory */
    const orbx_feature_set *features;
    const float *world_pos;                /* [nA*3]                                                                       */
    int is_bad;                            /* pKF->isBad(): nothing else is read                                           */
} orbx_reloc_match_keyframe;
typedef struct orbx_reloc_match_result {
    int32_t *matches, *key_index;
    float *p2d, *sigma2, *p3dw;
    int32_t *n, *nmatches;
    uint8_t *discarded;
} orbx_reloc_match_result;
int orbx_reloc_match_candidates(orbx_matcher *m, const orbx_reloc_match_frame *frame_host, const orbx_reloc_match_keyframe *keyframes_host,
                                int ncandidates, float nn_ratio, int check_orientation, const orbx_reloc_match_result *result);

/* profile_kernels (developer tap of tools/latency_track_chain.py / latency_track_ref.py): on != 0 records an event between the
 * launches of the next chain calls; orbx_track_last_kernel_times returns the device milliseconds between them (at most
 * `capacity`, *count of them; motion model: stage, pass 1, pass 2, gather, pose, discard; local map: stage, search, gather,
 * pose, statistics; reference keyframe: stage, search, gather, pose, discard; relocalisation candidates: stage, search,
 * gather). */
int orbx_track_set_profiling(orbx_matcher *m, int on);
int orbx_track_last_kernel_times(orbx_matcher *m, float *ms, int capacity, int *count);

/* ------------------------------------------------------------------------------------
 * The refine loop of Tracking::Relocalization (src/Tracking.cc:2135-2223) for every pose that PnPsolver::iterate
 * returns, for ALL hypotheses of ALL candidates as one launch chain with ONE host wait.  Lives on the matcher handle;
 * host memory throughout; the handle keeps no state between calls.
 *
 * Per distinct hypothesis h = (candidate, Tcw, inlier mask), all H in parallel (one workgroup each):
 *   seed     mvpMapPoints[j] = bow_match[j] where inliers[j], else -1; sFound = those slots (:2137-2152)
 *   pose 1   PoseOptimization from Tcw over the features with a point, ascending (:2156) -> ngood[0]
 *            exit 0: ngood[0] < 10 (the outliers stay, :2159); then the outliers leave (:2162-2164)
 *            exit 1: ngood[0] >= 50, success
 *   search 1 SearchByProjection(CurrentFrame, pKF, sFound, 10, 100) (:2171; the whole of src/ORBmatcher.cc:1731-1863: Ow,
 *            projection, image bounds, dist3D in [0.8 min_distance, 1.2 max_distance], PredictScale, radius, levels
 *            [l-1, l+1], the greedy search in slot order with the features that hold a point blocked, the rotation
 *            histogram under check_orientation) -> nadditional[0]
 *            exit 2: nadditional[0] + ngood[0] < 50 (the additional matches stay)
 *   pose 2   (:2182) -> ngood[1]; its outliers are NOT dropped (the reference's quirk)
 *            exit 3: ngood[1] >= 50, success;  exit 4: ngood[1] <= 30
 *   search 2 sFound rebuilt from every feature that holds a point (:2191-2194); th 3, ORBdist 64 -> nadditional[1]
 *            exit 5: ngood[1] + nadditional[1] < 50
 *   pose 3   (:2205-2209) -> ngood[2], the outliers leave;  exit 6: ngood[2] >= 50, success;  exit 7: failure
 * Every stage is enqueued unconditionally; the workgroups of a hypothesis that has taken its exit leave at once.
 * A last kernel walks sequence[S] - indices into the H hypotheses in the order in which the reference's round-robin
 * loop (:2105-2226) would process the returned poses; one record may appear several times, its tail is computed once -
 * and reports winner = the first entry whose hypothesis succeeded, or -1.
 *
 * The identity of a map point is its keyframe slot: the same MapPoint in two slots of one keyframe would be two
 * points to sFound.  mvbOutlier starts as all zero for every hypothesis (the reference carries the flags of the
 * hypothesis before into features that hold no point; nothing reads them there).
 *
 * Results, per hypothesis (arrays of H entries; any pointer may be NULL): stage (the exit, 0..7), success, ngood[3],
 * nadditional[2], n_correspondences[3] (edges of each pose call; 0 = did not run), pose[16] (mTcw as the hypothesis
 * leaves it), stats[3][8] (as orbx_pose_optimization, per pose call; zeros = did not run).  For the winner - or, when
 * nothing won, for the LAST entry of sequence (what the reference leaves in mCurrentFrame): map_point[N] (keyframe
 * slot held by each feature or -1), outlier[N] (mvbOutlier), hypothesis, candidate.
 *
 * ORBX_ERR_ARG: NULL arguments, nlevels outside 1..12, an empty frame / candidate list / hypothesis list / sequence,
 * a bow_match outside -1..npoints-1, a hypothesis' candidate or a sequence entry out of range; in form (b) a PnP handle without
 * a solve or on another device, a candidate or record outside that solve, a keypoint_count that is not the solve's n, a
 * keypoint_index outside 0..N-1 or one feature named twice.  ORBX_ERR_CAPACITY: more than
 * ORBX_TRACK_MAX_CORRESPONDENCES possible correspondences (min(N, seeds + valid slots) of a hypothesis), N or npoints
 * beyond the matcher's max_features or 65535 or the replay's LDS tile (4 N + 6 npoints + 16 <= 160 KB), H beyond
 * ORBX_RELOC_MAX_HYPOTHESES, S beyond ORBX_RELOC_MAX_SEQUENCE.  Neither launches anything.
 *
 * Contract: every field equals, bit for bit, the composition per hypothesis of orbx_pose_optimization (one frame),
 * the projection restated on the host, orbx_area_search_greedy and the histogram / control flow on the host. */
#define ORBX_RELOC_MAX_HYPOTHESES 64
#define ORBX_RELOC_MAX_SEQUENCE 4096
typedef struct orbx_reloc_frame {
    orbx_projection_frame frame;      /* keypoints_un, descriptors, u_right, counts, grid statics (occupied is not read) */
    float fx, fy, cx, cy, mbf;
    float max_x, max_y;               /* Frame::mnMaxX, mnMaxY */
    const float *scale_factors;       /* mvScaleFactors [nlevels] */
    const float *ratio_thresholds;    /* [nlevels-1] from orbx_predict_scale_thresholds */
    const float *inv_level_sigma2;    /* mvInvLevelSigma2 [nlevels] */
    int nlevels;
    int check_orientation;
} orbx_reloc_frame;
typedef struct orbx_reloc_candidate {  /* pKF->GetMapPointMatches() as arrays over its npoints slots */
    int npoints;
    const uint8_t *valid;             /* pMP && !pMP->isBad() */
    const float *world_pos;           /* [3] */
    const float *max_distance;        /* mfMaxDistance (GetMaxDistanceInvariance() / 1.2f) */
    const float *min_distance;        /* mfMinDistance */
    const uint8_t *descriptors;       /* [32] */
    const float *kf_angle;            /* pKF->mvKeysUn[i].angle */
    const int32_t *bow_match;         /* [N] keyframe slot that vvpMapPointMatches[c][j] holds for frame feature j, or -1 */
} orbx_reloc_candidate;
typedef struct orbx_reloc_hypotheses {
    int count;                        /* H distinct hypotheses */
    const int32_t *candidate;         /* [H] */
    const float *tcw;                 /* form (a): [H*12] rows of [R | t] */
    const uint8_t *inliers;           /* form (a): [H*N] over the frame's features */
    const int32_t *sequence;          /* [S] indices into the H hypotheses */
    int sequence_length;
    /* form (b), pnp != NULL (tcw and inliers are then not read): hypothesis h is record record[h] of candidate candidate[h] of the LAST orbx_pnp_solve
     * of `pnp` (same device, same candidate order as `cands`).  Its pose is the record's mRefinedRi / mRefinedti narrowed to float (refined_tcw), its
     * mask the record's mvbRefinedInliers, both read where the PnP chain left them in device memory: no mask crosses to the host.
     * keypoint_index[c][i] (mvKeyPointIndices: compacted match i of candidate c -> frame feature), keypoint_count[c] entries = that solve's n. */
    struct orbx_pnp_solver *pnp;
    const int32_t *record;            /* [H] */
    const int32_t *const *keypoint_index;   /* [ncands] (entries of candidates no hypothesis names may be NULL) */
    const int32_t *keypoint_count;    /* [ncands] */
} orbx_reloc_hypotheses;
typedef struct orbx_reloc_result {
    int32_t *stage, *success, *ngood, *nadditional, *n_correspondences;   /* [H], [H], [H*3], [H*2], [H*3] */
    float *pose;                      /* [H*16] */
    double *stats;                    /* [H*24] */
    int32_t *map_point;               /* [N] */
    uint8_t *outlier;                 /* [N] */
    int32_t winner, hypothesis, candidate;
} orbx_reloc_result;
int orbx_relocalize_refine(orbx_matcher *m, const orbx_reloc_frame *frame, const orbx_reloc_candidate *cands, int ncands,
                           const orbx_reloc_hypotheses *hyp, orbx_reloc_result *result);
/* The chain's projection stage on explicit inputs (src/ORBmatcher.cc:1735-1790), from the chain's own kernel: per slot of
 * `candidate` (bow_match, descriptors and kf_angle are not read) u, v, radius, min_level, max_level of the query and
 * active = the slot reaches the search (valid, not in found[npoints] - NULL = none -, inside the image and the distance
 * range; the other values are 0 where it does not).  tcw: [12].  Only the scale tables, intrinsics and bounds of `frame`
 * are read. */
int orbx_reloc_project(orbx_matcher *m, const orbx_reloc_frame *frame, const orbx_reloc_candidate *candidate, const float *tcw,
                       const uint8_t *found, float th, float *u, float *v, float *radius, int32_t *min_level, int32_t *max_level,
                       uint8_t *active);

/* ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1020-1177; LocalMapping::SearchInNeighbors)
 * and ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1179-1312; LoopClosing): the search of
 * steps 2-3 for every map point - KeyFrame::GetFeaturesInArea(u, v, radius), the level gate, for the
 * first overload the chi-square gate on the reprojection error (:1111-1135, chi2_gate = 1) and the
 * feature of minimum Hamming distance (first minimum in GetFeaturesInArea order).  What couples the
 * map points in the reference's loop (isBad / IsInKeyFrame, Replace, AddObservation, :1036-1040,
 * 1150-1172) is sequential pointer surgery and stays with the caller, evaluated in order on the result.
 * kf: mvKeysUn, mDescriptors, mvuRight and the grid statics of the KeyFrame (`occupied` is not read). */
typedef struct orbx_fuse_points {
    const float *u, *v;          /* projection of the map point into the KeyFrame (:1056-1060)          */
    const float *ur;             /* u - bf*invz (:1066); read only with chi2_gate                       */
    const int32_t *level;        /* nPredictedLevel = pMP->PredictScale(dist3D, pKF) (:1090)            */
    const float *radius;         /* th*pKF->mvScaleFactors[nPredictedLevel] (:1093)                     */
    const uint8_t *active;       /* 1 = the point reached step 2 (gates :1036-1088); NULL = all         */
    const uint8_t *descriptors;  /* pMP->GetDescriptor(), 32 bytes                                      */
    const int32_t *counts;       /* points per KeyFrame                                                 */
    int capacity;
    float kf_min_x, kf_min_y;    /* (float)pKF->mnMinX / mnMinY: KeyFrame stores the bounds as int
                                    (include/KeyFrame.h), and its GetFeaturesInArea computes the cell window
                                    with them, while mGrid was filed with the Frame's float bounds
                                    (kf->min_x / min_y)                                                  */
} orbx_fuse_points;
/* Device-pointer form for kf->nframes independent (KeyFrame, point list) problems; results:
 * matches[f*stride + i] = bestIdx of point i or -1, dists[f*stride + i] = bestDist (256 when none)
 * (orbx_matcher_results_device / orbx_matcher_download); the caller fuses when bestDist <= TH_LOW (:1148).
 * inv_level_sigma2: HOST pKF->mvInvLevelSigma2[nlevels]. */
int orbx_fuse_search_device(orbx_matcher *m, const orbx_projection_frame *kf, const orbx_fuse_points *points,
                            const float *inv_level_sigma2, int nlevels, int chi2_gate);
/* Host-array form for one KeyFrame (counts[0] entries each): best_idx / best_dist per map point. */
int orbx_fuse_search(orbx_matcher *m, const orbx_projection_frame *kf_host, const orbx_fuse_points *points_host,
                     const float *inv_level_sigma2, int nlevels, int chi2_gate, int32_t *best_idx, int32_t *best_dist);

/* Greedy area search: the loops of ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
 * (loop closing, src/ORBmatcher.cc:388-513) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th,
 * ORBdist) (relocalisation, :1731-1864) after their per-point preparation (:410-452 / :1755-1790, cv::Mat
 * expressions and PredictScale, kept on the host by the shim).  Queries are processed in order; query i
 * takes the feature of minimum Hamming distance (first minimum in GetFeaturesInArea order) among the
 * features inside GetFeaturesInArea(u, v, radius[, min_level, max_level]) that are not blocked - blocked
 * from the start (frame->occupied: vpMatched[idx] / CurrentFrame.mvpMapPoints[i2] non-NULL) or taken by an
 * earlier query - provided that distance is <= max_dist (TH_LOW / ORBdist, < 256); the feature is then blocked.
 * Level gate: octave < min_level or (max_level >= 0 and octave > max_level) rejects (Frame::GetFeaturesInArea,
 * src/Frame.cc:741-850; the KeyFrame variants pass [level-1, level], :469-470). */
typedef struct orbx_area_queries {
    const float *u, *v, *radius;
    const int32_t *min_level, *max_level;
    const uint8_t *active;       /* 1 = the point reached the search; NULL = all                            */
    const uint8_t *descriptors;  /* pMP->GetDescriptor(), 32 bytes                                          */
    const int32_t *counts;       /* queries per frame                                                       */
    int capacity;
    float window_min_x, window_min_y; /* bounds used for the cell window: Frame::mnMinX/Y, or (float) of the
                                         KeyFrame's int mnMinX/Y (see orbx_fuse_points)                     */
} orbx_area_queries;
/* results: matches[f*stride + i] = feature taken by query i or -1, dists[...] its distance (256 when none),
 * nmatches[f] = number of queries that took a feature. */
int orbx_area_search_greedy_device(orbx_matcher *m, const orbx_projection_frame *frame, const orbx_area_queries *queries, int max_dist);
int orbx_area_search_greedy(orbx_matcher *m, const orbx_projection_frame *frame_host, const orbx_area_queries *queries_host, int max_dist,
                            int32_t *assigned, int32_t *dists, int32_t *nmatches);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * (src/ORBmatcher.cc:515-654; Tracking::MonocularInitialization, src/Tracking.cc:944).  f1: mvKeysUn and
 * descriptors of the reference frame; f2: the current frame with its grid statics; prev_matched_xy: vbPrevMatched
 * (x, y per F1 feature, laid out like f1).  matches[f*stride + i1] = vnMatches12[i1], nmatches[f] = return value;
 * the caller refreshes vbPrevMatched from the matches (:646-650). */
int orbx_search_for_initialization_device(orbx_matcher *m, const orbx_feature_set *f1, const orbx_projection_frame *f2,
                                          const float *prev_matched_xy, int window_size, float nn_ratio, int check_orientation);
int orbx_search_for_initialization(orbx_matcher *m, const orbx_feature_set *f1_host, const orbx_projection_frame *f2_host,
                                   const float *prev_matched_xy, int window_size, float nn_ratio, int check_orientation,
                                   int32_t *matches12, int32_t *nmatches);

int orbx_matcher_results_device(orbx_matcher *m, const int32_t **matches_dev, const int32_t **dists_dev,
                                const int32_t **nmatches_dev, int *stride);
int orbx_matcher_download(orbx_matcher *m, int npairs, int32_t *matches, int32_t *dists, int stride,
                          int32_t *nmatches);
int orbx_matcher_sync(orbx_matcher *m);

/* Host-array convenience forms for one pair (upload, run, download). */
int orbx_search_by_bow(orbx_matcher *m, const orbx_feature_set *a_host, const orbx_feature_set *b_host,
                       const orbx_bow_params *params, int32_t *matches, int32_t *nmatches);
int orbx_stereo_match(orbx_matcher *m, const orbx_feature_set *left_host, const orbx_feature_set *right_host,
                      const float *scale_factors, int nlevels, float max_disparity, int32_t *best_dist,
                      int32_t *best_idx);
/* Average kernel milliseconds (HIP events on the matcher's stream) per *_device call since
 * the previous orbx_matcher_last_timing (at most the last 64 calls). */
int orbx_matcher_last_timing(orbx_matcher *m, float *total_ms);
/* Split of the SearchByBoW calls averaged by the previous orbx_matcher_last_timing: the distance /
 * candidate-list kernel (k_bow_topk) and the greedy replay with its preparation (k_bow_order + k_bow_greedy). */
int orbx_matcher_last_kernel_timing(orbx_matcher *m, float *distance_ms, float *replay_ms);


/* ------------------------------------------------------------------------------------
 * Bag of words  ==  DBoW2::TemplatedVocabulary<FORB::TDescriptor,FORB>::transform, the work of
 * Frame::ComputeBoW / KeyFrame::ComputeBoW (reference src/Frame.cc:880-896,
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1262): per feature the word id, the word
 * weight and the node `levelsup` levels above the leaf - the FeatureVector key that gates
 * ORBmatcher::SearchByBoW, directly usable as orbx_feature_set.groups.
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_vocabulary orbx_vocabulary;

/* The tree as flat arrays, as ORBVocabulary::loadFromTextFile builds it
 * (TemplatedVocabulary.h:1338-1420): node 0 = root, parent[i] < i, the children of a node are
 * its child ids in ascending order, word ids count the leaves in node-id order.
 * descriptors: 32 bytes per node (root unused), weights: one double per node (leaves: word weight). */
int orbx_vocabulary_create(int device, int k, int L, int num_nodes, const int32_t *parent, const uint8_t *is_leaf,
                           const uint8_t *descriptors, const double *weights, orbx_vocabulary **out);
void orbx_vocabulary_destroy(orbx_vocabulary *v);
int orbx_vocabulary_words(const orbx_vocabulary *v);

/* ORBVocabulary::loadFromTextFile on the device (TemplatedVocabulary.h:1338-1420, what System::System runs before its first frame): the text
 * "k L scoring weighting" + one line "parent isLeaf d0 .. d31 weight" per node, node id = line number (:1385), to the SAME device tree
 * orbx_vocabulary_create builds from the same arrays - children in ascending node id for any line order with parent < id, word ids counting the
 * leaves in node-id order (:1408-1415).  The device indexes the lines, parses one line per lane and builds the child lists; the file form reads
 * the file in slices into pinned memory and uploads a slice while the next is read.  One host wait; a second one when the device flagged lines.
 *
 * Tokens are separated by what istream >> skips inside a line (space, tab, CR, VT, FF; CRLF files work); tokens behind the weight are ignored, as
 * in the reference.  The weight [+-]?(digits[.digits*]|.digits)([eE][+-]?digits)? becomes the correctly rounded double of the token, bit for
 * bit what istream >> double (glibc strtod) gives the reference (:1406): on the device by the Eisel-Lemire algorithm for up to 19 significant
 * digits, and every token whose rounding that algorithm cannot prove - more digits, a subnormal or overflowing value, a tie - flags its line for
 * the host statement (strtol / strtod, the body of orbx_voc_text_parse_host), as does a line of more than 1023 bytes.
 *
 * Stated differences (parity unpinned):
 *   - the reference loops on !f.eof() (:1378): a file that ends in '\n' - every file its own saveToTextFile writes - gives it one more node
 *     with parent 0 and an uninitialised descriptor.  Here the empty last line is dropped and final_newline = 1 says so;
 *   - malformed lines, which the reference stores as 0 or stale values: too few tokens, a non-numeric token, a descriptor value outside 0..255,
 *     a parent that is not a smaller node id (m_nodes[pid] out of bounds at :1392), an empty line in the middle, a child under a leaf, an
 *     inner node without children, inf / nan / hex-float weights.  Here: ORBX_ERR_ARG, the 1-based line in orbx_last_error and in error_line,
 *     *out NULL.  The header is held to the reference's range check (:1359) and to orbx_vocabulary_create's k >= 1 and two nodes.
 * Text of 2^31 bytes or more: ORBX_ERR_CAPACITY. */
typedef struct orbx_voc_text_info {
    int32_t k, L, scoring, weighting;      /* the header line */
    int32_t num_nodes, num_words;
    int32_t final_newline;                 /* the text ended in '\n': the empty last line was dropped */
    int32_t host_lines;                    /* lines the device flagged and the host statement re-parsed */
    int32_t error_line;                    /* 1-based line of the first format error, 0 = none */
    int32_t launches, waits;
    int64_t bytes;
    float read_ms, upload_ms, kernel_ms, host_ms, total_ms;
} orbx_voc_text_info;
int orbx_vocabulary_load_text(int device, const char *path, orbx_vocabulary **out, orbx_voc_text_info *info);
int orbx_vocabulary_load_text_buffer(int device, const void *text, size_t size, orbx_vocabulary **out, orbx_voc_text_info *info);
/* The tree of ANY orbx_vocabulary (loaded, created, trained) back as orbx_vocabulary_create's flat arrays; any pointer may be NULL.  The root's
 * descriptor (unused by create) comes back as zeros. */
int orbx_vocabulary_tree(orbx_vocabulary *v, int32_t *k, int32_t *L, int32_t *num_nodes, int32_t *parent, uint8_t *is_leaf,
                         uint8_t *descriptors, double *weights);
/* The literal host statement of the parse - split at '\n', tokens, strtol / strtod, then orbx_vocabulary_create's three checks: no device, no
 * handle.  Format errors are reported before structure errors, each kind at its first line.  With all four arrays NULL it only sizes
 * (info->num_nodes); ORBX_ERR_CAPACITY when capacity_nodes is too small. */
int orbx_voc_text_parse_host(const void *text, size_t size, orbx_voc_text_info *info, int32_t capacity_nodes, int32_t *parent,
                             uint8_t *is_leaf, uint8_t *descriptors, double *weights);
/* The device's accept rule for one weight token, run on the host (the same code): 1 and *value when the device proves the token's double itself,
 * 0 when it flags the line. */
int orbx_voc_text_weight_rule(const char *token, size_t size, double *value);

/* transform() of every feature of the extractor's LAST batch, on the extractor's stream (ordered
 * behind the extraction and ahead of any consumer that orders itself behind the extractor).
 * Results stay on the device, laid out like the extractor's results (feature i of frame f at
 * f*capacity + i): word id, FeatureVector node id (-1 when the word's weight is 0: the reference
 * does not file such a feature, :1160-1166) and the word weight. */
int orbx_bow_transform_device(orbx_vocabulary *v, orbx_extractor *ext, int levelsup);
int orbx_bow_results_device(orbx_vocabulary *v, const int32_t **word_dev, const int32_t **node_dev,
                            const double **weight_dev, int *capacity);
int orbx_bow_download(orbx_vocabulary *v, orbx_extractor *ext, int batch, int32_t *word, int32_t *node, double *weight);
/* Host-array form for n descriptors (upload, run, download). */
int orbx_bow_transform(orbx_vocabulary *v, const uint8_t *descriptors, int n, int levelsup, int32_t *word,
                       int32_t *node, double *weight);
/* The same call, plus the two orders in which transform() fills its std::map results (TemplatedVocabulary.h:1146-1196): by_word[k] / by_node[k] =
 * the feature that is k-th in ascending (word id, feature index) / (node id, feature index) order among the *filed features (word weight > 0).  A caller
 * that builds the BowVector / FeatureVector from them inserts every key at the end of the map (emplace_hint) and accumulates / appends in feature order,
 * i.e. gets the reference's maps bit for bit without ~2000 tree searches (shim/BoW_hip.cc: 66 -> 20 us per frame).  The orders are ranked on the device. */
int orbx_bow_transform_sorted(orbx_vocabulary *v, const uint8_t *descriptors, int n, int levelsup, int32_t *word, int32_t *node, double *weight,
                              int32_t *by_word, int32_t *by_node, int32_t *filed);
/* Latency form for the ONE frame that `ext`'s last single-frame call extracted (Frame::ComputeBoW of the frame the constructor has just built,
 * src/Frame.cc:880-896 behind :394-456): the descriptors are read where the extractor left them on the device - nothing is uploaded - and the call
 * can be begun the moment the extraction is complete, long before the tracking thread asks for the BowVector.  A job owns its stream, result
 * buffers and pinned memory and only READS the vocabulary: any number of jobs and orbx_bow_transform* calls may use one vocabulary concurrently
 * (the vocabulary must outlive its jobs).  _begin returns at once; _end waits and hands out pointers INTO the job's pinned memory, valid until the
 * next call on the job: word / node / weight per feature, the two orders of orbx_bow_transform_sorted, *filed and the feature count *n.
 * `ext` must not be called between _begin and the completion of the job's kernels (~20 us). */
typedef struct orbx_bow_job orbx_bow_job;
int orbx_bow_job_create(orbx_vocabulary *v, orbx_bow_job **out);
void orbx_bow_job_destroy(orbx_bow_job *j);
int orbx_bow_job_begin(orbx_bow_job *j, orbx_extractor *ext, int levelsup);
int orbx_bow_job_end(orbx_bow_job *j, const int32_t **word, const int32_t **node, const double **weight, const int32_t **by_word, const int32_t **by_node,
                     int32_t *filed, int32_t *n);


/* ------------------------------------------------------------------------------------
 * Rest of the Frame constructor  ==  Frame::UndistortKeyPoints (reference src/Frame.cc:899-947),
 * Frame::ComputeImageBounds (:950-1004) and Frame::AssignFeaturesToGrid / PosInGrid
 * (:460-491, 868-878); called from both Frame constructors (src/Frame.cc:181, 210, 234 and
 * 422-456).  One handle per camera (mK, mDistCoef).
 * ---------------------------------------------------------------------------------- */
#define ORBX_FRAME_GRID_COLS 64 /* FRAME_GRID_COLS, include/Frame.h:55-60 */
#define ORBX_FRAME_GRID_ROWS 48 /* FRAME_GRID_ROWS                         */
typedef struct orbx_frame_ops orbx_frame_ops;
typedef struct orbx_camera {
    float fx, fy, cx, cy; /* mK                                                                   */
    float dist[5];        /* mDistCoef: k1 k2 p1 p2 [k3]; dist[0] == 0 means "already rectified",
                             the reference's own test (src/Frame.cc:901, 953)                     */
    int ndist;            /* 4 or 5 (src/Tracking.cc:127-136 appends k3 only when non-zero)       */
} orbx_camera;
/* The statics PosInGrid reads (src/Frame.cc:868-878): Frame::mnMinX, mnMinY,
 * mfGridElementWidthInv = 64/(mnMaxX-mnMinX), mfGridElementHeightInv = 48/(mnMaxY-mnMinY) (:326-327). */
typedef struct orbx_frame_grid {
    float min_x, min_y, width_inv, height_inv;
} orbx_frame_grid;

int orbx_frame_ops_create(int device, const orbx_camera *camera, orbx_frame_ops **out);
void orbx_frame_ops_destroy(orbx_frame_ops *h);
/* Frame::ComputeImageBounds(imLeft): bounds = mnMinX, mnMaxX, mnMinY, mnMaxY for a cols x rows image. */
int orbx_frame_image_bounds(orbx_frame_ops *h, int cols, int rows, float *bounds);
/* Frame::UndistortKeyPoints on n host keypoints (upload, run, download): kp_un[i] = keypoints[i]
 * with pt replaced by the undistorted point. */
int orbx_frame_undistort(orbx_frame_ops *h, const orbx_keypoint *keypoints, int n, orbx_keypoint *kp_un);
/* Frame::AssignFeaturesToGrid on n host mvKeysUn: mGrid as CSR, cell = x*ORBX_FRAME_GRID_ROWS + y,
 * grid_offsets[cell .. cell+1] (64*48+1 entries) delimit the feature indices of mGrid[x][y] inside
 * grid_indices[n], in the reference's push_back (= ascending) order. */
int orbx_frame_assign_grid(orbx_frame_ops *h, const orbx_frame_grid *grid, const orbx_keypoint *kp_un, int n,
                           int32_t *grid_offsets, int32_t *grid_indices);
/* Both, fused, for every frame of the extractor's LAST batch on the extractor's stream.  Results stay
 * on the device: mvKeysUn laid out like the extractor's keypoints (feature i of frame f at
 * f*capacity + i), grid_offsets[f*(64*48+1) + ...], grid_indices[f*capacity + ...]. */
int orbx_frame_finish_device(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid);
int orbx_frame_results_device(orbx_frame_ops *h, const orbx_keypoint **kp_un_dev, const int32_t **grid_offsets_dev,
                              const int32_t **grid_indices_dev, int *capacity);
int orbx_frame_download(orbx_frame_ops *h, orbx_extractor *ext, int batch, orbx_keypoint *kp_un, int32_t *grid_offsets,
                        int32_t *grid_indices);
/* Latency form for ONE frame that `ext`'s last single-frame call extracted (the Frame constructors, src/Frame.cc:168-234, 394-456):
 * _begin launches the fused kernel on the handle's own stream, reading the keypoints where the extractor left them on the device and
 * writing mvKeysUn / the grid into the handle's pinned memory, and returns at once (grid == NULL: undistort only); _end waits and hands
 * out pointers INTO that pinned memory, valid until the next call on the handle: kp_un (NULL when the camera is not distorted: mvKeysUn
 * = mvKeys, src/Frame.cc:901-905), grid_offsets[64*48+1], grid_indices[n].  `ext` must not be called in between. */
int orbx_frame_finish_begin(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid);
int orbx_frame_finish_end(orbx_frame_ops *h, const orbx_keypoint **kp_un, const int32_t **grid_offsets, const int32_t **grid_indices, int *n);

/* ------------------------------------------------------------------------------------
 * The RGB-D Frame constructor  ==  Frame::Frame(imGray, imDepth, ...) (reference src/Frame.cc:238-348): the frame-finish work above plus
 * Frame::ComputeStereoFromRGBD (:1423-1461), fused into the same launch, and what the tracker derives from mvDepth on every RGB-D frame.
 * Per feature i of a frame, with (u, v) = mvKeys[i].pt converted float -> int by truncation (imDepth.at<float>(v, u), :1444):
 *     d = depth(v, u);   d > 0 (false for NaN):  mvDepth[i] = d,  mvuRight[i] = mvKeysUn[i].pt.x - bf / d;   otherwise both -1      (:1451-1458)
 *     xyz_cam[3i..] = ((uUn - cx) * d) * invfx, ((vUn - cy) * d) * invfy, d  with invfx = 1.0f / fx  (Frame::UnprojectStereo, :1478-1491,
 *                     before mRwc * x + mOw, which stays with the caller);  0 0 0 where mvDepth[i] <= 0
 * and per frame
 *     order[0 .. n_valid)  the features with mvDepth > 0, ascending by (mvDepth, i): the sorted vector<pair<float,int>> of
 *                          Tracking::UpdateLastFrame / CreateNewKeyFrame (src/Tracking.cc); order[n_valid .. n) = -1
 *     n_close              features with 0 < mvDepth < th_depth (Tracking::NeedNewKeyFrame)
 * All of it float32, one correctly rounded operation at a time (no contraction).  A keypoint outside the depth image (the extractor never
 * produces one) has no depth.
 * Depth formats: ORBX_DEPTH_F32 = the CV_32F image the constructor takes, used as is (`factor` is ignored);  ORBX_DEPTH_U16 = the raw 16-bit
 * image Tracking::GrabImageRGBD receives, d = (float)raw * factor with factor = mDepthMapFactor = 1 / DepthMapFactor (src/Tracking.cc:212-216,
 * 334-338: imDepth.convertTo(CV_32F, mDepthMapFactor)) - only the looked-up pixels are converted.
 * ---------------------------------------------------------------------------------- */
#define ORBX_DEPTH_F32 0
#define ORBX_DEPTH_U16 1
typedef struct orbx_depth_desc {
    const void *data;  /* batch form: DEVICE memory, frame f at data + f * stride_bytes * rows;  latency form: HOST memory, one image */
    int format;        /* ORBX_DEPTH_F32 | ORBX_DEPTH_U16                                                                          */
    int cols, rows;    /* must equal the size of the frames the extractor ran on                                                    */
    int stride_bytes;  /* bytes between rows: a multiple of the pixel size, >= cols * pixel size                                    */
    float factor;      /* ORBX_DEPTH_U16: mDepthMapFactor                                                                            */
} orbx_depth_desc;
typedef struct orbx_rgbd_params {
    float bf;       /* mbf                                                                     */
    float th_depth; /* mThDepth = mbf * ThDepth / fx (src/Tracking.cc:205)                     */
} orbx_rgbd_params;

/* Host depth images (one per frame, same size and format) into a handle-owned device area laid out as orbx_depth_desc asks for the batch
 * form; *depth_dev receives the descriptor to pass on.  Valid until the next orbx_upload_depth on `h`. */
int orbx_upload_depth(orbx_frame_ops *h, const void *const *images, int batch, int format, int cols, int rows, int stride_bytes, float factor,
                      orbx_depth_desc *depth_dev);
/* orbx_frame_finish_device + the RGB-D step for every frame of the extractor's LAST batch, in the same launch on the extractor's stream.
 * Results stay on the device next to those of orbx_frame_results_device: depth / u_right / order [f*capacity + i], xyz_cam[(f*capacity + i)*3],
 * n_valid[f], n_close[f]; entries at and behind a frame's keypoint count are undefined. */
int orbx_frame_rgbd_device(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid, const orbx_depth_desc *depth_dev,
                           const orbx_rgbd_params *params);
int orbx_frame_rgbd_results_device(orbx_frame_ops *h, const float **depth_dev, const float **u_right_dev, const int32_t **order_dev,
                                   const int32_t **n_valid_dev, const int32_t **n_close_dev, const float **xyz_cam_dev, int *capacity);
/* Waits for the extractor's stream; any pointer may be NULL.  Arrays as above with `batch` frames; orbx_frame_download brings the rest. */
int orbx_frame_rgbd_download(orbx_frame_ops *h, orbx_extractor *ext, int batch, float *depth, float *u_right, int32_t *order, int32_t *n_valid,
                             int32_t *n_close, float *xyz_cam);
/* Latency form for ONE frame, as orbx_frame_finish_begin / _end (same kernel, same pinned result area, `ext` must not be called in between):
 * `depth` is the caller's HOST image (pageable: the cv::Mat of the constructor).  _begin looks the n depth values up on the host - the
 * extractor's keypoints are in its pinned result arena already - and hands the kernel n floats; ORBX_RGBD_STAGE_IMAGE=1 in the environment
 * copies the whole image to pinned memory and lets the kernel gather instead (same bits; the two are compared in profiles/rgbd_latency.txt).  _end waits and hands
 * out pointers into the handle's pinned memory, valid until the next call on the handle. */
typedef struct orbx_rgbd_frame {
    const float *depth, *u_right; /* mvDepth, mvuRight [n]               */
    const int32_t *order;         /* [n], see above                      */
    const float *xyz_cam;         /* [3n]                                */
    int n_valid, n_close;
} orbx_rgbd_frame;
int orbx_frame_rgbd_begin(orbx_frame_ops *h, orbx_extractor *ext, const orbx_frame_grid *grid, const orbx_depth_desc *depth_host,
                          const orbx_rgbd_params *params);
int orbx_frame_rgbd_end(orbx_frame_ops *h, const orbx_keypoint **kp_un, const int32_t **grid_offsets, const int32_t **grid_indices, int *n,
                        orbx_rgbd_frame *rgbd);


/* ------------------------------------------------------------------------------------
 * Local bundle adjustment  ==  the numerical core of Optimizer::LocalBundleAdjustment
 * (reference include/Optimizer.h:112, src/Optimizer.cc:629-997): g2o BlockSolver_6_3 +
 * Levenberg-Marquardt with Schur complement, 5 robust (Huber) iterations, outlier
 * re-classification, 10 non-robust iterations.  The class shim collects the local window
 * from the KeyFrame/MapPoint graph (src/Optimizer.cc:634-853) into these flat arrays and
 * writes poses/points/outliers back under the map mutex (:961-996).
 * Precision at the boundary is float32 like the reference's cv::Mat (src/Converter.cc);
 * everything inside is FP64.  Contract vs the CPU oracle: |delta| <= 1e-5.
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_lba orbx_lba;

typedef struct orbx_lba_problem {
    int num_keyframes;            /* local + fixed keyframes                                      */
    const float *poses;           /* [K*16] Tcw, row-major 4x4 (KeyFrame::GetPose)                */
    const uint8_t *fixed;         /* [K] 1 = fixed vertex (lFixedCameras, or mnId==0)             */
    const float *intrinsics;      /* [K*5] fx, fy, cx, cy, mbf                                    */
    int num_points;
    const float *points;          /* [P*3] MapPoint::GetWorldPos                                  */
    int num_edges;                /* observations, in optimizer.addEdge order                     */
    const int32_t *edge_point;    /* [E]                                                          */
    const int32_t *edge_keyframe; /* [E]                                                          */
    const float *edge_obs;        /* [E*3] kpUn.pt.x, kpUn.pt.y, mvuRight (<0: monocular edge)    */
    const float *edge_inv_sigma2; /* [E] mvInvLevelSigma2[kpUn.octave]                            */
} orbx_lba_problem;

typedef struct orbx_lba_result {
    float *poses;           /* [K*16] optimised Tcw (fixed keyframes returned unchanged)          */
    float *points;          /* [P*3]                                                              */
    double *edge_chi2;      /* [E] e->chi2() as read at src/Optimizer.cc:921-958 (may be NULL)     */
    uint8_t *edge_outlier;  /* [E] 1 = goes to vToErase (chi2 > 5.991/7.815 or depth <= 0)          */
    double stats[8];        /* stage1 {iterations, LM trials, chi2 start, chi2 end}, stage2 idem    */
} orbx_lba_result;

int orbx_lba_create(int device, int max_keyframes, int max_points, int max_edges, orbx_lba **out);
void orbx_lba_destroy(orbx_lba *h);
/* stop_flag == pbStopFlag (mbAbortBA): polled before starting, between LM iterations and
 * between LM trials, like g2o's forceStopFlag; may be NULL. */
int orbx_lba_solve(orbx_lba *h, const orbx_lba_problem *problem, const volatile uint8_t *stop_flag,
                   orbx_lba_result *result);
/* Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (reference src/Optimizer.cc:55-84, 86-360; Tracking::
 * CreateInitialMapMonocular with 20 iterations, LoopClosing::RunGlobalBundleAdjustment with 10): the same graph
 * and solver as the local window, one optimize(iterations) with Huber kernels iff robust, no outlier pass.
 * problem: every non-bad KeyFrame (fixed[k] = mnId == 0) and MapPoint with its observations; result as
 * orbx_lba_solve (edge_outlier / edge_chi2 = the final classification, informative only here).
 * The reduced (keyframe) system is DENSE here: its lower triangle is factored by the blocked Cholesky of csrc/orbx_lba.hip, up to
 * 24576 unknowns = 4096 free keyframes (CHOL_DENSE_MAX_N), ORBX_ERR_CAPACITY beyond.  Up to ~530 free keyframes a block row of
 * the Schur complement is accumulated in LDS; larger windows take the global-memory path (tested at 560 keyframes). */
int orbx_bundle_adjustment(orbx_lba *h, const orbx_lba_problem *problem, int iterations, int robust,
                           const volatile uint8_t *stop_flag, orbx_lba_result *result);
/* Kernel milliseconds (HIP events) spent inside the last orbx_lba_solve and FP64 flop count. */
int orbx_lba_last_timing(orbx_lba *h, float *device_ms, double *flops);

/* Batched LocalBundleAdjustment: ONE handle solves N independent windows (several maps in one process: multi-session or
 * multi-agent SLAM, independent sequences on one device), and every kernel launch of the chain covers all N windows.
 * Capacities are PER WINDOW; max_keyframes <= 341 (6 * K <= 2048: every reduced system stays on the LDS paths), else
 * ORBX_ERR_ARG.  Without a device, create returns ORBX_ERR_NODEVICE after the argument checks, as orbx_lba_create does.
 * Only the two-stage 5 + 10 iteration form of orbx_lba_solve is batched (global BA windows come one at a time). */
typedef struct orbx_lba_batch orbx_lba_batch;
int orbx_lba_batch_create(int device, int max_windows, int max_keyframes, int max_points, int max_edges, orbx_lba_batch **out);
void orbx_lba_batch_destroy(orbx_lba_batch *h);
/* Optimizer::LocalBundleAdjustment on num_windows independent windows.  problems[w] / results[w] exactly as for orbx_lba_solve,
 * and results[w] is BIT-IDENTICAL to what orbx_lba_solve returns for problems[w] alone (poses, points, edge_chi2, edge_outlier,
 * all 8 stats), whatever the other windows of the batch are and in any order.
 * stop_flags: NULL, or num_windows pointers (each may be NULL) = each window's pbStopFlag, polled as orbx_lba_solve polls it; a
 * raised flag affects only its own window.  Bad input in any window (NULL array, edge id out of range, size over capacity,
 * num_windows outside 1..max_windows) fails the whole call before anything is launched: ORBX_ERR_ARG / ORBX_ERR_CAPACITY, the
 * window's index in orbx_last_error, no result written. */
int orbx_lba_solve_batch(orbx_lba_batch *h, int num_windows, const orbx_lba_problem *problems,
                         const volatile uint8_t *const *stop_flags, orbx_lba_result *results);
/* Kernel milliseconds (HIP events) of the last orbx_lba_solve_batch (all windows) and its FP64 flop count. */
int orbx_lba_batch_last_timing(orbx_lba_batch *h, float *device_ms, double *flops);


/* ------------------------------------------------------------------------------------
 * Motion-only bundle adjustment  ==  Optimizer::PoseOptimization(Frame *pFrame)
 * (reference include/Optimizer.h, src/Optimizer.cc:363-605; called by every Track* function of
 * Tracking): one SE3 vertex, unary EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
 * edges with Huber kernels, 4 rounds of 10 Levenberg iterations each restarted from the initial
 * pose, inlier re-classification between rounds (chi2 > 5.991 / 7.815).  A batch of independent
 * frames is solved by one kernel launch (one workgroup per frame, no host round trip).
 * Feature i of frame f at f*capacity + i; only features that have a MapPoint are passed. */
typedef struct orbx_pose_optimizer orbx_pose_optimizer;
typedef struct orbx_pose_problem {
    int num_frames, capacity;
    const float *poses;        /* [B*16] pFrame->mTcw, row-major                                  */
    const float *cameras;      /* [B*5]  fx, fy, cx, cy, mbf                                      */
    const int32_t *counts;     /* [B]    features with a MapPoint (nInitialCorrespondences)        */
    const float *world_points; /* [B*cap*3] MapPoint::GetWorldPos()                                */
    const float *observations; /* [B*cap*3] kpUn.pt.x, kpUn.pt.y, mvuRight (< 0: monocular edge)   */
    const float *inv_sigma2;   /* [B*cap]   mvInvLevelSigma2[kpUn.octave]                          */
} orbx_pose_problem;
int orbx_pose_optimizer_create(int device, int max_frames, int max_features, orbx_pose_optimizer **out);
void orbx_pose_optimizer_destroy(orbx_pose_optimizer *h);
/* poses_out [B*16] = pFrame->mTcw after SetPose; outlier [B*cap] = pFrame->mvbOutlier of the passed
 * features; inliers [B] = the return value (nInitialCorrespondences - nBad); stats [B*8] = per round
 * {LM iterations, final robustified chi2}.  Any output may be NULL.  Contract vs the CPU oracle:
 * |delta pose| <= 1e-5, identical outlier flags. */
int orbx_pose_optimization(orbx_pose_optimizer *h, const orbx_pose_problem *problem, float *poses_out, uint8_t *outlier,
                           int32_t *inliers, double *stats);


/* ------------------------------------------------------------------------------------
 * MapPoint refresh  ==  MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth
 * (reference src/MapPoint.cc:359-439, 477-521; the loops of LocalMapping::ProcessNewKeyFrame /
 * CreateNewMapPoints / SearchInNeighbors, Tracking::CreateNewKeyFrame, the bundle adjustments and
 * loop correction) for M points with ragged observation lists, in one launch chain.
 * Observations are CSR: those of point p at obs_offset[p] .. obs_offset[p+1], in the CALLER's
 * order (the order of std::map<KeyFrame*, size_t>, which the reference iterates); it is never
 * reordered.  desc_valid[t] == 0 marks an observer whose keyframe isBad(): skipped for the
 * descriptor choice (:384), still counted for the normal, as in the reference.
 *   best_obs / best_median: with N valid descriptors in list order and row i = the Hamming
 *     distances of descriptor i to all N (self-distance included), the median of a row is its
 *     element at sorted position (N-1)/2; best_obs = the position IN THE POINT'S FULL LIST of the
 *     lowest i with the smallest median, best_median that median (0..256).  N == 0: -1, INT_MAX
 *     (the caller keeps the old descriptor).
 *   normal / max_dist / min_dist: the reference's float / double steps on the project's OpenCV
 *     stand-in, bit for bit, the float sum of the unit vectors taken sequentially in list order.
 *     Stock OpenCV's Mat / double multiplies by a float reciprocal instead of dividing in double:
 *     parity unpinned for the quotient.
 *   updated[p] = 0 for a point without observations (the reference returns early: nothing of it
 *     is to be written back; its other outputs are unspecified), 1 otherwise.
 * At most 65535 observations per point (ORBX_ERR_CAPACITY beyond).  Synchronous: results are in
 * the caller's arrays on return. */
typedef struct orbx_mappoint_ops orbx_mappoint_ops;
typedef struct orbx_mappoint_batch {      /* host memory */
    int num_points, num_obs;
    const int32_t *obs_offset;            /* [M+1], obs_offset[0] == 0, non-decreasing, obs_offset[M] == num_obs */
    const uint8_t *desc, *desc_valid;     /* [T*32] pKF->mDescriptors.row(idx); [T] !pKF->isBad(), NULL = all valid */
    const float *cam_center;              /* [T*3] pKF->GetCameraCenter()                                         */
    const float *pos, *ref_center;        /* [M*3] mWorldPos; mpRefKF->GetCameraCenter()                          */
    const float *ref_scale, *top_scale;   /* [M]   mpRefKF->mvScaleFactors[level of the observation]; [nLevels-1] */
} orbx_mappoint_batch;
typedef struct orbx_mappoint_result {     /* any may be NULL */
    int32_t *best_obs, *best_median;      /* [M] */
    float *normal, *max_dist, *min_dist;  /* [M*3], [M], [M] */
    uint8_t *updated;                     /* [M] */
} orbx_mappoint_result;
int orbx_mappoint_ops_create(int device, int max_points, int max_obs_total, orbx_mappoint_ops **out);
void orbx_mappoint_ops_destroy(orbx_mappoint_ops *h);
int orbx_mappoint_refresh(orbx_mappoint_ops *h, const orbx_mappoint_batch *b, const orbx_mappoint_result *r);
/* device time of the last call's kernels and how many were launched (one per non-empty size class) */
int orbx_mappoint_last_timing(orbx_mappoint_ops *h, float *kernel_ms, int *launches);

/* ------------------------------------------------------------------------------------
 * New map points  ==  the per-match geometry of LocalMapping::CreateNewMapPoints
 * (src/LocalMapping.cc:423-596) and the chain over the neighbour keyframes around it (:350-624).
 *
 * Per match (KF1 feature idx1, KF2 feature idx2), in the reference's operation order: ray
 * parallax, stereo parallax, the three-way choice (linear triangulation / UnprojectStereo of
 * KF1 / of KF2), the two depth tests, the two chi2 reprojection tests, the scale test.  The
 * status byte says which `continue` was taken or which path accepted the point.
 *   float where the reference computes in float; double where the project's OpenCV stand-in
 *   does: Mat::dot and cv::norm accumulate in double, 1.0/z is a double quotient narrowed to
 *   float, the 3-term matrix products go left to right in float.
 *   The null vector of the 4x4 A comes from a one-sided Jacobi SVD in FP64 (the reference:
 *   cv::SVD in float), atan2f / cosf from the device library: PARITY UNPINNED AT THE OPENCV
 *   LEVEL for the SVD and the transcendental functions.  Contract: status equals the numpy
 *   restatement (tests/triangulate_ref.py) on every match that does not sit on a threshold;
 *   x3d of the stereo paths bit-equal; x3d of the triangulation path within a float32 SVD's
 *   own error of the float64 SVD's result.
 *   UnprojectStereo reads the RAW keypoint (mvKeys), not mvKeysUn (src/KeyFrame.cc:816), and the
 *   second keyframe's stereo reprojection uses the CURRENT keyframe's mbf (:562): kept.
 * ---------------------------------------------------------------------------------- */
#define ORBX_NP_NONE 0           /* the slot holds no match                                   */
#define ORBX_NP_TRIANGULATED 1   /* accepted, x3D from the SVD (:470-489)                     */
#define ORBX_NP_STEREO1 2        /* accepted, pKF1->UnprojectStereo (:490-493)                */
#define ORBX_NP_STEREO2 3        /* accepted, pKF2->UnprojectStereo (:494-497)                */
#define ORBX_NP_LOW_PARALLAX 4   /* no stereo and very low parallax (:499)                    */
#define ORBX_NP_W_ZERO 5         /* x3D.at<float>(3) == 0 (:485)                              */
#define ORBX_NP_DEPTH_INVALID 6  /* UnprojectStereo on mvDepth <= 0 (src/KeyFrame.cc:808)      */
#define ORBX_NP_BEHIND1 7        /* z1 <= 0 (:507)                                            */
#define ORBX_NP_BEHIND2 8        /* z2 <= 0 (:511)                                            */
#define ORBX_NP_REPROJ1 9        /* chi2 test in KF1 (:528 / :540)                            */
#define ORBX_NP_REPROJ2 10       /* chi2 test in KF2 (:556 / :568)                            */
#define ORBX_NP_DIST_ZERO 11     /* dist1 == 0 || dist2 == 0 (:582)                           */
#define ORBX_NP_SCALE 12         /* the two-sided ratio test (:595)                           */

typedef struct orbx_keyframe_geom {   /* host memory: pose and calibration of one KeyFrame */
    float tcw[12];              /* Rcw | tcw, 3x4 row-major (GetRotation / GetTranslation)     */
    float center[3];            /* GetCameraCenter() = Ow = Twc.col(3)                         */
    float fx, fy, cx, cy, invfx, invfy;
    float mb, mbf;
    float scale_factor;         /* mfScaleFactor (read of KF1 only: ratioFactor = 1.5f * it)   */
    const float *scale_factors; /* mvScaleFactors[nlevels]                                     */
    const float *level_sigma2;  /* mvLevelSigma2[nlevels]                                      */
    int nlevels;                /* 1..12                                                       */
} orbx_keyframe_geom;

typedef struct orbx_keyframe_obs {    /* host memory: the per-feature arrays of one KeyFrame */
    const orbx_keypoint *keys_un;     /* mvKeysUn[count]: x, y, octave are read                  */
    const float *keys_raw;            /* mvKeys[i].pt as x, y pairs [2*count]; NULL = identical  */
    const float *u_right, *depth;     /* mvuRight / mvDepth [count]; NULL = monocular            */
    int count;
} orbx_keyframe_obs;

/* The geometry alone, on K pairs of keyframes with explicit match lists (CSR over the pairs):
 * matches match_offset[p] .. match_offset[p+1] belong to pair p, match j is (idx1[j], idx2[j]).
 * status[j] and x3d[3*j..] per match (x3d is 0 where no point was computed).  No mask is kept:
 * the caller supplied the matches.  One launch per pair, one synchronisation. */
typedef struct orbx_triangulate_pairs {
    int npairs;
    const int32_t *match_offset;                 /* [npairs+1], match_offset[0] == 0, non-decreasing */
    const int32_t *idx1, *idx2;                  /* [match_offset[npairs]]                           */
    const orbx_keyframe_geom *geom1, *geom2;     /* [npairs]                                         */
    const orbx_keyframe_obs *obs1, *obs2;        /* [npairs]                                         */
} orbx_triangulate_pairs;
int orbx_triangulate_matches(orbx_matcher *m, const orbx_triangulate_pairs *pairs, uint8_t *status, float *x3d);

/* The chain: for neighbour k = 0..K-1 in order, SearchForTriangulation(KF1, neighbour k, bOnlyStereo = false) on
 * the CURRENT eligibility mask of KF1, the geometry above on its matches, and the mask bytes of the accepted KF1
 * features cleared (the reference: they now hold a MapPoint, src/ORBmatcher.cc:845-855) - all on the matcher's
 * stream without a host synchronisation between the neighbours; then the accepted slots of all neighbours are
 * compacted into the `created` list in the order the reference creates the points (neighbour ascending, then
 * KF1 feature ascending), and the host waits once.
 *   kf1_host: one frame (nframes = 1); `valid` initialises the mask (1 = the feature has no MapPoint).
 *   neighbours_host: one feature set, nframes = K, neighbour k at k*capacity; only the neighbours that passed the
 *     caller's baseline / median-depth gate (:358-384).  F12 and the epipole per neighbour come from the caller.
 *   stop_flag: NULL or CheckNewKeyFrames() as a byte, never written through; read before neighbour k > 0 is
 *     enqueued (:353); *pairs_done = how many neighbours ran (their results are complete).
 * Capacities and LDS sizes are checked before the first launch. */
typedef struct orbx_new_points_params {   /* host memory */
    const orbx_keyframe_geom *geom1;      /* KF1                                                       */
    const orbx_keyframe_geom *geom2;      /* [K]                                                       */
    const float *f12, *epipole;           /* [9*K], [2*K] as in orbx_triangulation_params              */
    const float *keys_raw1, *u_right1, *depth1;   /* KF1: [2*n1], [n1], [n1]; NULL as in orbx_keyframe_obs   */
    const float *keys_raw2, *u_right2, *depth2;   /* neighbours, laid out like the feature set: [2*K*capacity], [K*capacity] x 2 */
    int check_orientation;                /* mbCheckOrientation (false in CreateNewMapPoints, :323)    */
    int profile_kernels;                  /* 1: time every k_triangulate launch with events of its own */
} orbx_new_points_params;
typedef struct orbx_new_point {
    int32_t neighbour, idx1, idx2, path;  /* path = ORBX_NP_TRIANGULATED / _STEREO1 / _STEREO2 */
    float x, y, z;
} orbx_new_point;
typedef struct orbx_new_points_result {
    orbx_new_point *created;              /* [created_capacity]; a KF1 feature is created at most once: n1 suffices */
    int created_capacity;
    int32_t *count;                       /* entries written to `created`                               */
    int32_t *nmatches;                    /* [K] return value of each search (0 for neighbours not run) */
    int32_t *pairs_done;
    uint8_t *status;                      /* optional [K*kf1->capacity], slot k*capacity + idx1         */
    int32_t *matches;                     /* optional, same layout: the KF2 feature or -1               */
    float *x3d;                           /* optional [3*K*kf1->capacity]                               */
} orbx_new_points_result;
int orbx_create_new_map_points(orbx_matcher *m, const orbx_feature_set *kf1_host, const orbx_feature_set *neighbours_host,
                               const orbx_new_points_params *params, const volatile uint8_t *stop_flag,
                               const orbx_new_points_result *result);
/* device time of the last chain (first search to k_collect), its kernel launches, and the time inside k_triangulate
 * (0 unless the chain ran with profile_kernels) */
int orbx_new_points_last_timing(orbx_matcher *m, float *device_ms, int *launches, float *triangulate_ms);

/* ----------------------------------------------------------------------------------
 * LocalMapping::SearchInNeighbors, steps 2 and 3 (reference src/LocalMapping.cc:666-713): the T + 1 complete calls of
 * ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1020-1174) - one per target keyframe on the current
 * keyframe's points, then one of the current keyframe on the targets' points - as ONE chain on the matcher's stream.
 * The state that couples the calls (isBad, the observation maps and Observations(), mvpMapPoints of the searchable
 * keyframes, the descriptor that Replace -> ComputeDistinctiveDescriptors rewrites) lives on the device; the host
 * waits once.  Integers and bytes: every result equals the sequential loop.
 *
 * The slice (host arrays).  Keyframes are slots 0..num_keyframes-1: the current keyframe, the targets and every other
 * keyframe that observes a point of the slice; kf_rank = the iteration order of std::map<KeyFrame*, size_t> (distinct),
 * kf_bad = isBad().  The SEARCHABLE keyframes (the current keyframe and every target, each once) carry their
 * features, pose and calibration (orbx_fuse_keyframe).  Points 0..num_points-1: every point a searchable keyframe
 * holds; observations as CSR in ascending rank, each with the keyframe slot, the feature index, the stereo byte
 * (mvuRight[idx] >= 0) and the 32 descriptor bytes of that feature.  Observations() is derived: 1 per observation,
 * 2 where it is stereo.  For a searchable keyframe, kf_point[f] == p exactly when p has the observation
 * (that keyframe, f).
 *
 * One Fuse call (keyframe k, list of point ids, -1 = NULL):
 *   prepare  on the state at the start of the call, per entry: skip -1, bad points and points observed by k; the gates
 *            and values of :1040-1086 in the reference's precisions (3x3 * 3x1 left to right in float, cv::norm and
 *            Mat::dot in double, the viewing gate a double comparison, the level from the ratio thresholds of
 *            orbx_predict_scale_thresholds);
 *   search   the search of orbx_fuse_search with chi2_gate = 1 on the point's current descriptor;
 *   apply    strictly in list order; an entry whose point has meanwhile gone bad or entered k is skipped.  With
 *            bestDist <= TH_LOW (the entry counts for nFused) and q = kf_point[k][bestIdx]:
 *              q < 0             ORBX_FUSE_ADDED: the point gains the observation (k, bestIdx), kf_point[k][bestIdx] = p
 *              q bad             ORBX_FUSE_HOLDER_BAD: nothing changes
 *              Obs(q) > Obs(p)   ORBX_FUSE_REPLACED_BY_HOLDER: p->Replace(q)
 *              else              ORBX_FUSE_REPLACED_HOLDER: q->Replace(p)
 *            a->Replace(b) (src/MapPoint.cc:244-307): a goes bad, replaced[a] = b; a's observations in ascending rank
 *            move to b (kf_point of a searchable keyframe follows) or, where b is observed by that keyframe already,
 *            are dropped (kf_point = -1); found / visible of a are added to b's; b's descriptor is recomputed over
 *            its observations whose keyframe is not bad (median of the Hamming distances at sorted position
 *            (N - 1) / 2, first strictly smallest median; kept when N = 0).  Observations() of a is left as it was.
 * The chain: the forward list is kf_point of the current keyframe at the start (the same for every target), targets in
 * the caller's order (a slot may repeat); the candidates of the reverse pass are gathered on the device (targets in
 * order, features in order, every point held NOW that is not bad and not yet listed).
 * ---------------------------------------------------------------------------------- */
#define ORBX_FUSE_ADDED 0
#define ORBX_FUSE_REPLACED_BY_HOLDER 1   /* the list point went bad, replaced by the holder */
#define ORBX_FUSE_REPLACED_HOLDER 2      /* the holder went bad, replaced by the list point  */
#define ORBX_FUSE_HOLDER_BAD 3

typedef struct orbx_fuse_keyframe {      /* host memory: one searchable keyframe */
    int slot;                            /* its keyframe slot                                                         */
    int num_features;                    /* N, 0..65535                                                               */
    const orbx_keypoint *keys_un;        /* mvKeysUn                                                                  */
    const uint8_t *descriptors;          /* mDescriptors, 32 bytes each                                               */
    const float *u_right;                /* mvuRight                                                                  */
    const int32_t *kf_point;             /* mvpMapPoints: a point id or -1                                            */
    float tcw[12];                       /* the first three rows of Tcw: Rcw | tcw                                    */
    float ow[3];                         /* GetCameraCenter()                                                         */
    float fx, fy, cx, cy, mbf;
    float grid_min_x, grid_min_y;        /* Frame::mnMinX / mnMinY, the float bounds mGrid was filed with             */
    float grid_width_inv, grid_height_inv;
    int min_x, max_x, min_y, max_y;      /* KeyFrame::mnMinX .. mnMaxY (int): IsInImage and the cell window           */
    const float *scale_factors;          /* mvScaleFactors[nlevels]                                                   */
    const float *inv_level_sigma2;       /* mvInvLevelSigma2[nlevels]                                                 */
    float log_scale_factor;              /* mfLogScaleFactor                                                          */
    int nlevels;                         /* mnScaleLevels                                                             */
} orbx_fuse_keyframe;

typedef struct orbx_fuse_slice {         /* host memory */
    int num_keyframes;
    const int32_t *kf_rank;              /* [num_keyframes] distinct                                                  */
    const uint8_t *kf_bad;               /* [num_keyframes]                                                           */
    int num_searchable;
    const orbx_fuse_keyframe *searchable;/* [num_searchable], every slot at most once                                 */
    int num_points, num_obs;
    const float *pos, *normal;           /* [3*num_points] mWorldPos, mNormalVector                                   */
    const float *min_distance;           /* GetMinDistanceInvariance()                                                */
    const float *max_distance;           /* GetMaxDistanceInvariance()                                                */
    const float *raw_max_distance;       /* mfMaxDistance (PredictScale reads this one)                               */
    const uint8_t *descriptors;          /* [32*num_points] mDescriptor                                               */
    const uint8_t *point_bad;
    const int32_t *visible, *found;      /* mnVisible, mnFound                                                        */
    const int32_t *obs_offset;           /* [num_points + 1]                                                          */
    const int32_t *obs_kf, *obs_idx;     /* [num_obs] keyframe slot (ascending rank inside a point), feature index    */
    const uint8_t *obs_stereo;           /* [num_obs]                                                                 */
    const uint8_t *obs_descriptors;      /* [32*num_obs]                                                              */
    float th;                            /* 3.0 in SearchInNeighbors                                                  */
    int profile_kernels;                 /* 1: time every apply launch with events of its own                         */
} orbx_fuse_slice;

typedef struct orbx_fuse_decision {
    int32_t call;                        /* 0..T-1 the forward pass, T the reverse pass (orbx_fuse_apply: 0)           */
    int32_t position;                    /* index in that call's list                                                 */
    int32_t point, feature;              /* the list point and bestIdx                                                */
    int32_t kind;                        /* ORBX_FUSE_*                                                               */
    int32_t other;                       /* the holder, -1 for ORBX_FUSE_ADDED                                        */
} orbx_fuse_decision;

typedef struct orbx_fuse_result {        /* host memory; every pointer may be NULL */
    orbx_fuse_decision *log;             /* [log_capacity] in execution order                                         */
    int log_capacity;
    int32_t *log_count;
    int32_t *nfused;                     /* [T + 1] (orbx_fuse_apply: [1])                                             */
    int32_t *candidates;                 /* [candidates_capacity] the list of the reverse pass                        */
    int candidates_capacity;
    int32_t *candidates_count;
    int32_t *kf_point;                   /* the searchable keyframes' kf_point one behind the other, in their order   */
    uint8_t *point_bad;                  /* [num_points]                                                              */
    int32_t *replaced;                   /* [num_points] -1 = none                                                    */
    int32_t *point_obs;                  /* [num_points] Observations()                                               */
    int32_t *visible, *found;            /* [num_points]                                                              */
    uint8_t *descriptors;                /* [32*num_points]                                                           */
    int32_t *obs_offset;                 /* [num_points + 1] the observations after the call, ascending rank          */
    int32_t *obs_kf, *obs_idx;           /* [obs_capacity]                                                            */
    uint8_t *obs_stereo;                 /* [obs_capacity]                                                            */
    int obs_capacity;
    /* per call c and list position i at c*full_stride + i (orbx_search_in_neighbors only; positions behind a list's end
     * are not written): the prepare and search results */
    int full_stride;
    uint8_t *active;
    float *u, *v, *ur;
    int32_t *level;
    float *radius;
    int32_t *best_idx, *best_dist;
} orbx_fuse_result;

/* The chain.  current = the slot of the current keyframe, targets = vpTargetKFs as slots (searchable, not `current`).
 * ORBX_ERR_ARG before anything is launched: a NULL array, an index, offset or rank that the kernels would trip over,
 * observations of a point not in ascending rank, kf_point and the observations of a searchable keyframe that disagree,
 * a target that is not searchable.  ORBX_ERR_CAPACITY before anything is launched: more than 65535 features or more
 * than 12 levels in a keyframe; after the chain and before anything is written: log_capacity, candidates_capacity or
 * obs_capacity too small (every output is left untouched, the handle stays usable).
 * Launches: 2 (staging, state) + 3 per Fuse call + 2 (candidate gather) + 1 (final state). */
int orbx_search_in_neighbors(orbx_matcher *m, const orbx_fuse_slice *slice, int current, const int32_t *targets, int num_targets,
                             const orbx_fuse_result *result);
/* The apply stage alone for keyframe slot `kf` (searchable) on search results the caller supplies: list[n] (point id or
 * -1), active[n], best_idx[n], best_dist[n] as prepare and search would have left them. */
int orbx_fuse_apply(orbx_matcher *m, const orbx_fuse_slice *slice, int kf, const int32_t *list, const uint8_t *active,
                    const int32_t *best_idx, const int32_t *best_dist, int n, const orbx_fuse_result *result);
/* device time of the last chain, its kernel launches, and the time inside the apply kernels (0 unless profile_kernels) */
int orbx_search_in_neighbors_last_timing(orbx_matcher *m, float *device_ms, int *launches, float *apply_ms);

/* ----------------------------------------------------------------------------------
 * Monocular initialisation: Initializer::Initialize (reference src/Initializer.cc:68-230) and
 * everything below it - FindHomography / FindFundamental over the caller's RANSAC sets, the
 * choice between the two models, DecomposeE / ReconstructH's eight motions, CheckRT of all
 * twelve and the selection - in one chain of six launches on the handle's own stream; the
 * host waits once.  Inputs go through mapped pinned memory, the last kernel writes the
 * results into mapped pinned memory and raises a sequence word.
 *
 *   Host side of a call: vMatches12 is compacted in i1 order and Normalize (:1501-1575) runs
 *   over both frames' keypoints - sequential float sums, as the reference has them.
 *   Device side: k_init_models (one wave per hypothesis and model: the 16x9 / 8x9 system,
 *   its null vector by a one-sided Jacobi in FP64 with the columns in LDS, rank 2 for F,
 *   denormalisation, then CheckHomography / CheckFundamental over all matches with the
 *   score summed in match order), k_init_decompose (first argmax of the scores, the four
 *   motions of DecomposeE and the eight of ReconstructH - both families always),
 *   k_init_check_rt (12 x N triangulations), k_init_rank (nGood and the cosine at sorted
 *   index min(50, nGood-1) by rank counting), k_init_decide (ReconstructF's / ReconstructH's
 *   selection, the result block).
 *
 *   Arithmetic: float in the reference's operation order; 1.0/x a double quotient narrowed to
 *   float; Mat::dot / cv::norm in double; 3-term products left to right.  PARITY UNPINNED AT
 *   THE OPENCV LEVEL: cv::SVD in float (here: Jacobi in FP64, narrowed), Mat::inv (here:
 *   cofactors in FP64), cv::determinant (here: cofactors in FP64), the SIGN of null vectors and
 *   singular vectors and with it the ORDER of the motion hypotheses inside each family, and
 *   acos (the host's acosf turns the selected cosine into degrees; the device compares
 *   cosines against a bound the host derived from the same acosf).  ReconstructH's motions
 *   are declared invalid (hyp_valid = 0) when d1/d2 < 1.00001 || d2/d3 < 1.00001 (:1185) or
 *   when one of the quotients is not finite.
 *   Hypothesis order: 0..3 = (R1,t) (R2,t) (R1,-t) (R2,-t) of ReconstructF (:1050-1060),
 *   4..7 = the d' = d2 family, 8..11 = the d' = -d2 family of ReconstructH (:1230-1345).
 * ---------------------------------------------------------------------------------- */
#define ORBX_INIT_NOT_INLIER 0          /* !vbMatchesInliers[i] (:1652)                                */
#define ORBX_INIT_NONFINITE 1           /* the triangulated point is not finite (:1668)               */
#define ORBX_INIT_BEHIND1 2             /* z1 <= 0 && cosParallax < 0.99998 (:1697)                   */
#define ORBX_INIT_BEHIND2 3             /* z2 <= 0 && cosParallax < 0.99998 (:1707)                   */
#define ORBX_INIT_REPROJ1 4             /* squareError1 > th2 (:1722)                                 */
#define ORBX_INIT_REPROJ2 5             /* squareError2 > th2 (:1737)                                 */
#define ORBX_INIT_GOOD 6                /* counted, vbGood = true                                     */
#define ORBX_INIT_GOOD_LOW_PARALLAX 7   /* counted (nGood, vP3D, the cosine list), vbGood stays false */
#define ORBX_INIT_HYPOTHESES 12
#define ORBX_INIT_MAX_MATCHES 16000     /* k_init_rank keeps a hypothesis' cosines in LDS (64 KB)     */

typedef struct orbx_initializer orbx_initializer;
/* ORBX_ERR_ARG: max_matches outside 8..ORBX_INIT_MAX_MATCHES, max_iterations < 1; then ORBX_ERR_NODEVICE without a device */
int orbx_initializer_create(int device, int max_matches, int max_iterations, orbx_initializer **out);
void orbx_initializer_destroy(orbx_initializer *h);

typedef struct orbx_init_matches {     /* host memory */
    const float *keys1_xy, *keys2_xy;  /* mvKeysUn[i].pt of the reference / the current frame: [n1][2], [n2][2] */
    int n1, n2;
    const int32_t *matches12;          /* [n1]: index into frame 2 or -1, the reference's vMatches12            */
} orbx_init_matches;

typedef struct orbx_init_problem {     /* host memory */
    const float *keys1_xy, *keys2_xy;
    int n1, n2;
    const int32_t *matches12;
    const int32_t *sets;               /* [iterations][8]: mvSets, indices into the COMPACTED match list (:139-168) */
    int iterations;
    float sigma;
    float fx, fy, cx, cy;
    float min_parallax;                /* degrees; the reference passes 1.0 */
    int min_triangulated;              /* the reference passes 50           */
} orbx_init_problem;

typedef struct orbx_init_result {      /* host memory; every pointer may be NULL.  N = number of matches, it = iterations */
    int32_t *success, *model;          /* model: 0 = H, 1 = F (the branch taken on RH, also when it fails)  */
    int32_t *hyp;                      /* the selected hypothesis 0..11, -1 on failure                       */
    float *r21, *t21;                  /* [9], [3]; zeros on failure                                         */
    float *p3d;                        /* [n1][3] vP3D, zeros where nothing was stored                       */
    uint8_t *triangulated;             /* [n1] vbTriangulated                                                */
    /* diagnostics (copies of their own behind the call) */
    int32_t *n_matches;
    float *t1, *t2;                    /* [9] each: Normalize's T of frame 1 / 2                             */
    float *hn, *fpre, *fn;             /* [it][9]: unit null vectors of H and of F before / after the rank-2 step */
    float *h21, *h12, *f21;            /* [it][9] denormalised                                               */
    float *score_h, *score_f;          /* [it]                                                               */
    int32_t *best_h, *best_f;
    float *sh, *sf, *rh;
    uint8_t *inliers_h, *inliers_f;    /* [N] of the best iteration                                          */
    float *hyp_r, *hyp_t;              /* [12][9], [12][3]                                                   */
    uint8_t *hyp_valid;                /* [12]                                                               */
    int32_t *hyp_good;                 /* [12] nGood                                                         */
    float *hyp_cos_parallax;           /* [12] the cosine at sorted index min(50, nGood-1); 1.0 when nGood = 0 */
    float *hyp_parallax_deg;           /* [12] acos of it in degrees (host)                                  */
    uint8_t *hyp_status;               /* [12][N] ORBX_INIT_*                                                */
    float *hyp_p3d;                    /* [12][N][3] the triangulated point per MATCH (0 where none was computed) */
    float *hyp_cos;                    /* [12][N] cosParallax per MATCH (0 where none was computed)            */
} orbx_init_result;
/* ORBX_ERR_ARG: fewer than 8 matches, iterations < 1, a set index outside [0, N), a match outside [0, n2);
 * ORBX_ERR_CAPACITY: more matches or iterations than the handle was created for. */
int orbx_initialize(orbx_initializer *h, const orbx_init_problem *problem, const orbx_init_result *result);

/* CheckHomography (:616-810, kind 0; H12 = H21^-1 is computed inside as in FindHomography) or CheckFundamental
 * (:813-953, kind 1) of m explicit 3x3 models (m <= 2 * max_iterations) with the chain's kernel:
 * scores[m], inliers[m][N]. */
int orbx_init_score_models(orbx_initializer *h, const orbx_init_matches *matches, const float *models, int m, int kind, float sigma,
                           float *scores, uint8_t *inliers);
/* CheckRT (:1578-1797) of m <= 12 explicit motions r[m][9], t[m][3] over the matches whose inliers[N] byte is set, with the chain's
 * kernels: good[m], vb_good[m][n1], p3d[m][n1][3] (vP3D), cos_parallax[m], status[m][N].  Output pointers may be NULL. */
int orbx_init_check_rt(orbx_initializer *h, const orbx_init_matches *matches, const uint8_t *inliers, const float *r, const float *t, int m,
                       float fx, float fy, float cx, float cy, float th2, int32_t *good, uint8_t *vb_good, float *p3d, float *cos_parallax,
                       uint8_t *status);
/* device time of the last orbx_initialize chain (first to last kernel) and its kernel launches */
int orbx_initializer_last_timing(orbx_initializer *h, float *device_ms, int *launches);

/* ----------------------------------------------------------------------------------
 * Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc): Horn 1987 on RANSAC triples, for ALL loop candidates
 * of LoopClosing::ComputeSim3 (src/LoopClosing.cc:300-560) in one launch chain with one wait.
 *
 *   The host (the shim) walks the pointers: vpMatched12 compacted in i1 order, pairs with a missing or bad point or an
 *   index < 0 skipped; per kept pair the two world positions, the two mvLevelSigma2[octave] and mvnIndices1.  The device
 *   does the rest, every iteration of every candidate: iterations do not depend on the solver's state once the sets are
 *   drawn, so the running best of iterate (:199-285) is a scan over the per-iteration inlier counts.
 *     k_sim3_prepare  the constructor (:48-140): X3Dc = Rcw * Xw + tcw, FromCameraToImage (:526-545), the two error limits;
 *                     reads the call's inputs in mapped pinned memory once and leaves everything later kernels read
 *                     many times in device memory.
 *     k_sim3_models   one lane per (candidate, iteration): ComputeSim3 (:309-448).
 *     k_sim3_check    one wave per (candidate, iteration): CheckInliers / Project (:451-523), the ballot of 64 matches is
 *                     the mask word, its population count the count.  All masks stay on the device.
 *     k_sim3_decide   one workgroup per candidate: the running best (count >= best updates it), the RETURN EVENTS (an
 *                     update with count > min_inliers), the first event and its mask, the result block, the sequence word.
 *
 *   Arithmetic, in the reference's operation order (float where it is float; the library is built with -ffp-contract=off):
 *     constructor   X3Dc = (R[0]*x + R[1]*y) + R[2]*z, then + t; invz = 1 / z as a FLOAT quotient; fx * (x * invz) + cx;
 *                   the limits are std::vector<size_t> (Sim3Solver.h:156-157): 9.210 * sigma2 as a double product,
 *                   truncated to an unsigned integer, compared as that integer converted to float.
 *     centroids     the sum of the three columns in order, then Mat / int: a double quotient narrowed to float
 *     M             Pr2 * Pr1^T, 3-term float products left to right
 *     N             the ten entries as float sums left to right, widened to double, narrowed to float again
 *     eigenvector   of the largest eigenvalue (the first of equal ones): cyclic two-sided Jacobi in FP64 on the float N,
 *                   ORBX_SIM3_JACOBI_SWEEPS sweeps, narrowed to float.  q and -q give the same rotation.
 *     angle-axis    ang = atan2(norm(vec), q0) in double, norm accumulates in double; vec = float(((2 * ang) / norm) * vec)
 *     cv::Rodrigues in double on the float vec (theta = norm; R = c I + (1 - c) r r^T + s [r]x), narrowed to float
 *     scale         P3 = R * Pr2; nom = Pr1.dot(P3) accumulated in double, row-major; den = the double sum of the FLOAT
 *                   squares of P3, row-major; s = float(nom / den); 1.0f with fix_scale
 *     t, T12, T21   sR = float products s * R; t = O1 - sR * O2; sRinv = float((1.0 / s) * R^T) with the quotient and the
 *                   products in double; tinv = (-sRinv) * t
 *     CheckInliers  P = R * X + t of the 4x4's upper rows, invz = 1 / z as a float quotient, fx * (x * invz) + cx; the error
 *                   is Mat::dot: the two squares summed in double, narrowed to float; no depth test, z <= 0 and non-finite
 *                   values are not special-cased, a NaN error fails the <.  inlier = err1 < max1 && err2 < max2.
 *   PARITY UNPINNED AT THE OPENCV LEVEL: cv::eigen in float (here: Jacobi in FP64, narrowed), cv::Rodrigues, the
 *   accumulation inside cv::gemm (here: 3-term float products, scalar factors applied to the matrix first) and Mat / int.
 *   The device library's atan2, sin and cos are not pinned either.
 *
 *   RANSAC sets are the caller's, [iterations][3] indices into the compacted list, distinct inside a set, each drawn by
 *   the reference's draw, overwrite-with-back, pop scheme (:228-249).  The reference draws lazily, three numbers per
 *   iteration, interleaved between the candidates of the round-robin loop; a batched call has to draw ahead, so a caller's
 *   rand() sequence is consumed in ANOTHER ORDER than the reference's.  This is not a parity claim.
 *
 *   n < min_inliers (:206-210): no iterations are run whatever `iterations` says, no_more = 1.
 * ---------------------------------------------------------------------------------- */
/* Sweeps of the 4x4 Jacobi.  Chosen on the CPU with the same iteration restated in numpy float64 (tests/sim3_ref.py::jacobi_eig4) over the
 * 1843 RANSAC sets of the test scenes: no float32 bit of the eigenvector changes after 5 sweeps (after 4 on all but 3 sets); 8 are run, and
 * tests/test_sim3_solver.py::test_jacobi_sweeps_settled asserts that 6, 8 and 10 give the same bits. */
#define ORBX_SIM3_JACOBI_SWEEPS 8
#define ORBX_SIM3_MAX_MATCHES 65536

typedef struct orbx_sim3_solver orbx_sim3_solver;
/* ORBX_ERR_ARG: max_candidates < 1, max_matches outside 3..ORBX_SIM3_MAX_MATCHES, max_iterations < 1 (the three are PER
 * CANDIDATE limits except the first); then ORBX_ERR_NODEVICE without a device */
int orbx_sim3_solver_create(int device, int max_candidates, int max_matches, int max_iterations, orbx_sim3_solver **out);
void orbx_sim3_solver_destroy(orbx_sim3_solver *h);

typedef struct orbx_sim3_problem {     /* host memory: one candidate */
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];   /* GetRotation / GetTranslation of pKF1, pKF2                       */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    int n;                                      /* kept pairs                                                       */
    const float *world1, *world2;               /* [n][3] GetWorldPos of pMP1 / pMP2                                */
    const float *sigma2_1, *sigma2_2;           /* [n] mvLevelSigma2[octave]                                        */
    const int32_t *sets;                        /* [iterations][3]                                                  */
    int iterations;                             /* mRansacMaxIts (orbx_sim3_ransac_iterations)                      */
    int min_inliers;
    int fix_scale;
} orbx_sim3_problem;

typedef struct orbx_sim3_result {      /* host memory: one candidate; every pointer may be NULL.  it = iterations run */
    int32_t *count;                    /* [it] mnInliersi                                                            */
    float *r12, *t12, *s12;            /* [it][9], [it][3], [it]                                                     */
    uint8_t *is_event;                 /* [it] the iteration updates the best and count > min_inliers                */
    int32_t *first_event;              /* the first such iteration, -1 = none                                        */
    int32_t *best_iteration;           /* the last iteration that updated the best (mBest* after all), -1 = none run */
    int32_t *no_more;                  /* n < min_inliers, or no event in any iteration                              */
    uint8_t *inliers_first;            /* [n] mvbInliersi of the first event, COMPACTED indices; zeros without one   */
    /* diagnostics (copies of their own behind the call) */
    float *x3dc1, *x3dc2;              /* [n][3]                                                                     */
    float *p1im1, *p2im2;              /* [n][2]                                                                     */
    float *max_err1, *max_err2;        /* [n] the truncated limits as floats                                         */
    float *nmat, *quat;                /* [it][16], [it][4]                                                          */
    float *t12m, *t21m;                /* [it][16]                                                                   */
} orbx_sim3_result;
/* ORBX_ERR_ARG: ncandidates < 1, a NULL problem / array, n < 0, iterations < 0, n < 3 with iterations to run, a set index
 * outside [0, n), repeated indices inside a set; ORBX_ERR_CAPACITY: more candidates, matches or iterations than the handle
 * was created for.  Nothing is launched on an error and the handle stays usable. */
int orbx_sim3_solve(orbx_sim3_solver *h, const orbx_sim3_problem *problems, int ncandidates, const orbx_sim3_result *results);
/* mvbInliersi [n] of any iteration of any candidate of the last orbx_sim3_solve: one row of the device's masks, copied on
 * demand (a caller's second and later return events).  ORBX_ERR_STATE before a solve, ORBX_ERR_ARG outside it. */
int orbx_sim3_inliers(orbx_sim3_solver *h, int candidate, int iteration, uint8_t *inliers);
/* CheckInliers of m <= max_iterations explicit transformations t12[m][16], t21[m][16] (row-major 4x4) over the problem's
 * pairs with the chain's kernels: count[m], inliers[m][n] (may be NULL).  sets / iterations / min_inliers are not read. */
int orbx_sim3_check_models(orbx_sim3_solver *h, const orbx_sim3_problem *problem, const float *t12, const float *t21, int m,
                           int32_t *count, uint8_t *inliers);
/* mRansacMaxIts of SetRansacParameters (:143-196) with the reference's libm calls; n = number of kept pairs.  No device. */
int orbx_sim3_ransac_iterations(double probability, int min_inliers, int max_iterations, int n);
/* device time of the last orbx_sim3_solve chain (first to last kernel) and its kernel launches */
int orbx_sim3_last_timing(orbx_sim3_solver *h, float *device_ms, int *launches);

/* ----------------------------------------------------------------------------------
 * Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1364-1590 with the vendored g2o): the Sim3 refinement of
 * LoopClosing::ComputeSim3 for ALL of a call's problems (the Sim3Solver events of the loop candidates, each with
 * SearchBySim3's matches) in ONE launch on the handle's own stream with one wait.  The caller's loop is
 * orbx_sim3_solve -> SearchBySim3 -> orbx_optimize_sim3.
 *
 *   k_optsim3  one workgroup of 256 threads per problem; thread t owns pairs t, t + 256, ... and keeps their two camera
 *              points, observations, weights and errors in registers for the whole call.  Per linearisation lanes 0-13 of
 *              wave 0 form the 14 perturbed estimates Sim3(+-1e-9 e_d) * S and their inverses once, in LDS; every thread
 *              differences its edges through them; the 28 + 7 + 1 sums of H, b and the robust chi2 are block sums in a fixed
 *              order (no floating-point atomics: repeated calls, and a batch against single calls, give the same bits); one
 *              thread solves the 7x7 system and takes the Levenberg decision.  Inputs are read from mapped pinned memory,
 *              the result block is written to mapped pinned memory behind a sequence word, like orbx_sim3_solve's.
 *
 *   Arithmetic: FP64, every product / sum / quotient its own IEEE operation (-ffp-contract=off, no fused multiply-add),
 *   in the order tests/optsim3_ref.py restates:
 *     camera points  P3D1c = R1w * P3D1w + t1w in FLOAT, (R[0]*x + R[1]*y) + R[2]*z, then + t - k_sim3_prepare's arithmetic,
 *                    bit for bit - widened to double; observations, 1 / sigma2 and the intrinsics are floats widened;
 *                    Huber's delta is sqrtf(th2) widened, th2 is compared widened
 *     estimate       g2o::Sim3(Quaterniond(R), t, s) (Eigen's four branches); oplus = Sim3(update) * estimate with
 *                    update[6] = 0 under fix_scale; the exponential of sim3.h:70-142 with its four branches
 *                    (|sigma| < 1e-5, theta < 1e-5); quaternion products are never renormalised; inverse() as sim3.h:233-236
 *     edges          e12 = obs1 - cam_map1(project(S.map(X2))), e21 = obs2 - cam_map2(project(S.inverse().map(X1))),
 *                    project = two divisions by z
 *     Jacobians      g2o's central differences (base_binary_edge.hpp:147-200): delta = 1e-9, column d =
 *                    (1 / (2 delta)) * (e(+delta) - e(-delta)) through oplus; column 6 is exactly zero under fix_scale
 *     quadratic form chi2 = invSigma2 * (e0^2 + e1^2), Huber rho as robust_kernel_impl.cpp, H += J^T (rho1 Omega) J,
 *                    b -= J^T (rho1 Omega e)
 *     Levenberg      optimization_algorithm_levenberg.cpp:61-164: lambda0 = 1e-5 max|H_jj| at iteration 0 of EACH optimize(),
 *                    <= 10 trials, rho = (chi - chi_trial) / (x . (lambda x + b) + 1e-3), accepted: lambda *= max(1/3,
 *                    min(1 - (2 rho - 1)^3, 2/3)), rejected: lambda *= nu, nu *= 2; Terminate on 10 trials or rho == 0;
 *                    stop after three iterations with (iniChi - chi) * 1e3 < iniChi
 *     solve          dense 7x7 LDL^T, a non-positive factor makes the trial's chi DBL_MAX
 *     rounds         optimize(5) over all pairs; a pair is removed when either edge has chi2() > th2; fewer than 10 left:
 *                    return 0, the estimate stays as passed in; else optimize(nBad > 0 ? 10 : 5) on the kept pairs (the
 *                    estimate carries over, lambda0 is re-initialised), the same test counts the inliers
 *     QUIRK, KEPT    chi2() reads _error as the LAST trial left it, accepted or rejected: the reference does not call
 *                    computeError() before its tests, and neither does the kernel
 *   PARITY UNPINNED: the device library's sin / cos / exp; Eigen's Quaterniond(R) branch choice beyond rounding; LDL^T
 *   pivoting (Eigen's LDLT pivots, this factorisation does not); the order in which the edges' contributions are summed.
 *
 *   n < 10 is NOT an error: round one still runs (n >= 1), the call returns n_inliers = 0 and the input estimate.
 * ---------------------------------------------------------------------------------- */
#define ORBX_SIM3_OPT_MAX_PAIRS 1024

typedef struct orbx_sim3_optimizer orbx_sim3_optimizer;
/* ORBX_ERR_ARG: max_problems outside 1..4096, max_pairs outside 1..ORBX_SIM3_OPT_MAX_PAIRS (a PER PROBLEM limit); then
 * ORBX_ERR_NODEVICE without a device */
int orbx_sim3_optimizer_create(int device, int max_problems, int max_pairs, orbx_sim3_optimizer **out);
void orbx_sim3_optimizer_destroy(orbx_sim3_optimizer *h);

typedef struct orbx_sim3_opt_problem {  /* host memory: one (candidate, matches, Sim3) triple */
    float rcw1[9], tcw1[3], rcw2[9], tcw2[3];   /* GetRotation / GetTranslation of pKF1, pKF2                       */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    int n;                                      /* kept pairs (nCorrespondences)                                    */
    const float *world1, *world2;               /* [n][3] GetWorldPos of pMP1 / pMP2                                */
    const float *obs1, *obs2;                   /* [n][2] mvKeysUn[i].pt of KF1, mvKeysUn[i2].pt of KF2             */
    const float *inv_sigma2_1, *inv_sigma2_2;   /* [n] mvInvLevelSigma2[octave]                                     */
    double r12[9], t12[3], s12;                 /* g2oS12 as passed in: rotation matrix (row-major), t, s           */
    float th2;
    int fix_scale;
} orbx_sim3_opt_problem;

typedef struct orbx_sim3_opt_result {   /* host memory: one problem; every pointer may be NULL */
    int32_t *n_inliers;                 /* the return value: nIn, 0 when fewer than 10 pairs survive round one        */
    double *quat, *t, *s;               /* [4] (x, y, z, w), [3], [1]: g2oS12 afterwards (the input on a return 0)     */
    float *r12;                         /* [9] its rotation().toRotationMatrix(), narrowed                             */
    uint8_t *removed_first;             /* [n] pairs nulled by the test behind round one                               */
    uint8_t *removed_final;             /* [n] pairs nulled by the test behind round two (zeros when it did not run)    */
    int32_t *n_bad;                     /* nBad of round one                                                           */
    /* diagnostics */
    double *chi2_round1, *chi2_round2;  /* [2n] chi2() as tested, [2 i] = e12, [2 i + 1] = e21; -1 = not in the graph  */
    double *stats;                      /* [4] {Levenberg iterations, final robust chi2} of round one, of round two    */
    float *x3dc1, *x3dc2;               /* [n][3] the camera points                                                    */
} orbx_sim3_opt_result;
/* ORBX_ERR_ARG: nproblems < 1, a NULL problem / array, n < 0, non-finite intrinsics or th2; ORBX_ERR_CAPACITY: more
 * problems or pairs than the handle was created for.  Nothing is launched on an error and the handle stays usable. */
int orbx_optimize_sim3(orbx_sim3_optimizer *h, const orbx_sim3_opt_problem *problems, int nproblems, const orbx_sim3_opt_result *results);
/* ONE linearisation of the problem's edges at the explicit estimate (quat (x, y, z, w), t, s) with the chain's own device
 * functions: errors[2n][2], chi2[2n], jac[2n][2][7] (edge 2 i = e12, 2 i + 1 = e21 of pair i; zeros where active[i] == 0),
 * H[49], b[7].  active [n] may be NULL (= every pair), and so may every output.  r12 / t12 / s12 of the problem are not read. */
int orbx_optimize_sim3_linearize(orbx_sim3_optimizer *h, const orbx_sim3_opt_problem *problem, const double *quat, const double *t, double s,
                                 const uint8_t *active, double *errors, double *chi2, double *jac, double *H, double *b);
/* device time of the last orbx_optimize_sim3 launch chain and its kernel launches */
int orbx_sim3_optimizer_last_timing(orbx_sim3_optimizer *h, float *device_ms, int *launches);

/* ----------------------------------------------------------------------------------
 * The refine step of LoopClosing::ComputeSim3 (src/LoopClosing.cc:435-480) for EVERY event that Sim3Solver::iterate
 * returns, for all H events of all K candidates as one launch chain with ONE host wait (a caller that asks for the
 * diagnostic arrays of orbx_loop_refine_result pays a stream synchronisation and one blocking copy per array behind it).
 * Lives on the matcher handle;
 * host memory throughout; the handle keeps no state between calls.
 *
 * Per distinct hypothesis h = (candidate, R12, t12, s12, inlier mask), all H in parallel, one status word each:
 *   seed     vpMapPointMatches[i] = bow_match[i] where inliers[i], else -1 (:437-443); vbAlreadyMatched1 = those
 *            features, vbAlreadyMatched2 = the slots they name (src/ORBmatcher.cc:1347-1357)
 *   project  both directions of SearchBySim3 (:1367-1411 and its mirror :1430-1474), one thread per slot, float, in the
 *            reference's operation order: p3Dc1 = (R[0]*x + R[1]*y) + R[2]*z, then + t, from the keyframe's rcw / tcw;
 *            sR12 = s12 * R12; sR21 = float((1.0 / s12) * R12^T), quotient and products in double; t21 = (-sR21) * t12
 *            (k_sim3_models' arithmetic, see orbx_sim3_solve above); p3Dc2 = sR21 * p3Dc1 + t21 in the same 3-term
 *            form; z < 0 rejects; invz = 1 / z as a float quotient; u = fx * (x * invz) + cx with KF1's intrinsics in
 *            BOTH directions (as the reference); IsInImage (>= min, < max); dist3D = cv::norm (squares summed in
 *            double) in [0.8 min_distance, 1.2 max_distance]; PredictScale through ratio_thresholds of the SEARCHED
 *            keyframe; radius = th * scale_factors[level].  A slot whose u or v is NaN fails IsInImage and is turned away.
 *            Output: one orbx_fuse_points record per slot and direction, in device memory.
 *   search   k_fuse_best with chi2_gate = 0 for the 2 H (keyframe, list) problems in ONE launch: direction 1->2
 *            searches the hypothesis' candidate, 2->1 searches KF1; KF1 and the K candidates are staged once.
 *            Accepted up to TH_HIGH = 100 (:1444 / :1507).
 *   mutual   vpMatches12[i1] = idx2 where vnMatch2[vnMatch1[i1]] == i1 (:1507-1521) -> n_found; then the pairs of
 *            Optimizer::OptimizeSim3 (src/Optimizer.cc:1429-1520) in ascending i1 over every i1 with a match whose two
 *            slots are valid -> n_pairs; world1, world2, obs1 = mvKeysUn1[i1].pt, obs2 = mvKeysUn2[i2].pt and the two
 *            inv_level_sigma2[octave] in the layout of orbx_sim3_opt_problem, in device memory
 *   optimise k_optsim3 (orbx_optimize_sim3 above: same kernel, same arithmetic, same order of sums), th2, fix_scale,
 *            from g2o::Sim3(R12, t12, s12) with the floats widened
 *   decide   pairs removed by either chi2 test are nulled in vpMatches12 (src/Optimizer.cc:1541 / :1578);
 *            success = n_inliers >= 20 (:463); mg2oScw = gScm * gSmw in FP64 (sim3.h's operator*, gSmw from the
 *            candidate's rcw / tcw widened, scale 1, :469-471); mScw = Converter::toCvMat: float(s * R), float(t).
 *            The last workgroup to arrive walks the H status words in order - hypotheses are given in the order in which
 *            the reference's round-robin loop (:403-482) meets the events, every event once - and reports winner = the
 *            first success or -1.
 * Every stage is enqueued unconditionally.  Launches: stage copy, seed, project, search, mutual, optimise, decide = 7;
 * form (b) adds one in front = 8 (orbx_loop_sim3_last_timing reports the count of the last call).
 *
 * The identity of a map point is its keyframe slot: pMP->GetIndexInKeyFrame(pKF2) of a KF2 point is its slot, and the
 * same MapPoint in two slots of one keyframe counts as two points.  PARITY UNPINNED: that identity, and everything
 * orbx_optimize_sim3 lists.
 *
 * status: 0 = failed, 1 = success, 2 = overflow: the pair count is decided on the device and k_optsim3 holds
 * ORBX_SIM3_OPT_MAX_PAIRS; a hypothesis that gathers more runs no optimisation (n_inliers = n_bad = 0, the estimate as
 * passed in).  If the walk meets such a hypothesis before a winner the call returns ORBX_ERR_CAPACITY with the
 * per-hypothesis results filled, winner = -1; nothing is silently truncated.
 *
 * ORBX_ERR_ARG: NULL arguments or arrays, nlevels outside 1..12, an empty keyframe / candidate list / hypothesis list,
 * grid statics or image bounds of a candidate that differ from KF1's (they are statics of Frame in the reference), a
 * bow_match outside -1..N2-1, a hypothesis' candidate out of range, non-finite th / th2 or th2 < 0; in form (b) a solver
 * without a solve or on another device, a candidate or iteration outside that solve, an index1 count that is not that
 * solve's n, an index1 outside 0..N1-1 or one feature named twice.  ORBX_ERR_CAPACITY: N beyond the matcher's
 * max_features or 65535, H beyond ORBX_LOOP_SIM3_MAX_HYPOTHESES, K beyond max_pairs.  Neither launches anything.
 *
 * Contract: every field equals, bit for bit, the composition per hypothesis of the seed and the projection restated on
 * the host, orbx_fuse_search (chi2_gate = 0) twice, the mutual check and the gather on the host, orbx_optimize_sim3 (one
 * problem) and the decision on the host. */
#define ORBX_LOOP_SIM3_MAX_HYPOTHESES 64
typedef struct orbx_loop_sim3_keyframe {   /* host memory: one keyframe as arrays over its N = frame.counts[0] slots */
    orbx_projection_frame frame;      /* keypoints_un, descriptors, counts, grid statics (u_right and occupied are not read) */
    float rcw[9], tcw[3];             /* GetRotation / GetTranslation */
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y; /* (float) of KeyFrame::mnMinX .. mnMaxY: IsInImage and the cell window */
    const float *scale_factors;       /* mvScaleFactors [nlevels] */
    const float *ratio_thresholds;    /* [nlevels-1] from orbx_predict_scale_thresholds */
    const float *inv_level_sigma2;    /* mvInvLevelSigma2 [nlevels] */
    int nlevels;
    const uint8_t *valid;             /* pMP && !pMP->isBad() */
    const float *world_pos;           /* [3] */
    const float *max_distance;        /* mfMaxDistance, as orbx_reloc_candidate */
    const float *min_distance;        /* mfMinDistance */
    const uint8_t *descriptors;       /* the map point's GetDescriptor() [32] */
    const int32_t *bow_match;         /* candidates only: [N1] KF2 slot that vvpMapPointMatches[c][i1] holds, or -1 */
} orbx_loop_sim3_keyframe;
typedef struct orbx_loop_sim3_hypotheses {
    int count;                        /* H distinct events, in walk order */
    const int32_t *candidate;         /* [H] */
    const float *r12, *t12, *s12;     /* form (a): [H*9], [H*3], [H] */
    const uint8_t *inliers;           /* form (a): [H*N1] over KF1's features */
    /* form (b), solver != NULL (r12 .. inliers are then not read): hypothesis h is iteration iteration[h] of candidate candidate[h]
     * of the LAST orbx_sim3_solve of `solver` (same device, same candidate order as `cands`): R12 / t12 / s12 and the mask row are
     * read where that chain left them in device memory, the mask scattered through index1[c][i] (mvnIndices1: compacted pair i of
     * candidate c -> KF1 feature), index1_count[c] entries = that solve's n.  No mask crosses to the host. */
    struct orbx_sim3_solver *solver;
    const int32_t *iteration;         /* [H] */
    const int32_t *const *index1;     /* [ncands] (entries of candidates no hypothesis names may be NULL) */
    const int32_t *index1_count;      /* [ncands] */
} orbx_loop_sim3_hypotheses;
/* (orbx_loop_sim3_result is the result of orbx_loop_correct_sim3 below; this one is named after its entry point) */
typedef struct orbx_loop_refine_result {   /* any pointer may be NULL */
    int32_t *status, *n_found, *n_pairs, *n_inliers, *n_bad;   /* [H] each */
    double *quat, *t, *s;             /* [H*4] (x, y, z, w), [H*3], [H]: gScm afterwards */
    float *scw;                       /* [H*16] mScw (written for every hypothesis, meaningful where status == 1) */
    int32_t *matches12;               /* [N1] the winner's mvpCurrentMatchedPoints as KF2 slots, -1 = none (all -1 without a winner) */
    /* diagnostics (copies of their own behind the call); P = the largest slot count of the call's keyframes, NP = max(P, 1);
     * list 2 h is direction 1->2 of hypothesis h, list 2 h + 1 direction 2->1 */
    float *query_u, *query_v, *query_radius;   /* [2H*NP] */
    int32_t *query_level;             /* [2H*NP] */
    uint8_t *query_active;            /* [2H*NP] */
    int32_t *match1, *match2;         /* [H*NP] vnMatch1 / vnMatch2 */
    int32_t winner, hypothesis, candidate;   /* first successful hypothesis or -1 (every event occurs once: hypothesis == winner); its candidate or -1 */
} orbx_loop_refine_result;
int orbx_loop_refine_sim3(orbx_matcher *m, const orbx_loop_sim3_keyframe *kf1, const orbx_loop_sim3_keyframe *cands, int ncands,
                          const orbx_loop_sim3_hypotheses *hyp, float th, float th2, int fix_scale, orbx_loop_refine_result *result);
/* device time of the last orbx_loop_refine_sim3 chain (first to last kernel) and its kernel launches */
int orbx_loop_sim3_last_timing(orbx_matcher *m, float *device_ms, int *launches);

/* ----------------------------------------------------------------------------------
 * PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc): EPnP on RANSAC sets of four matches, for ALL relocalisation
 * candidates of Tracking::Relocalization (src/Tracking.cc) in one launch chain with one wait.
 *
 *   The host (the shim) walks the pointers (:120-168): per kept match the undistorted keypoint (mvP2D), mvLevelSigma2[octave]
 *   and the MapPoint's world position (mvP3Dw).  The device does the rest, every iteration of every candidate.  Iterations are
 *   independent once the sets are drawn, EXCEPT through Refine (:366-418), whose input is the running-best inlier mask: its
 *   result depends only on the current RECORD (an iteration at which the running best changes), so it is computed once per
 *   record, and iterate (:240-363) is a scan over counts, records and refined counts.
 *     k_pnp_prepare  mvMaxError[i] = sigma2 * th2 as a float product (:227-229); reads the call's inputs in mapped pinned memory
 *                    once and leaves everything later kernels read many times in device memory.
 *     k_pnp_models   a team of 16 lanes per (candidate, iteration): compute_pose (:684-759) with everything it calls.
 *     k_pnp_check    one wave per (candidate, iteration): CheckInliers (:421-458), the ballot of 64 matches is the mask word.
 *     k_pnp_records  one wave per candidate: the running best changes only on count >= minInliers && count > best (strictly
 *                    greater, unlike Sim3Solver); record_of[i] = the latest record at or before iteration i.
 *     k_pnp_refine   one workgroup per (candidate, record): compute_pose on the record's inlier mask (points in index order),
 *                    then k_pnp_check on the refined models.  Refine succeeds on refined count > minInliers (strict, :404).
 *     k_pnp_decide   one workgroup per candidate: the RETURN EVENTS (count_i >= minInliers, :301, and record_of[i] refined
 *                    successfully), the first event and its refined mask, mBestTcw and its mask, the result block.
 *   All masks, of iterations and of refines, stay on the device; orbx_pnp_inliers copies one row out.
 *
 *   SetRansacParameters (:181-223) is evaluated on the HOST with the reference's libm calls (orbx_pnp_ransac_parameters; the
 *   device library's log and pow are not pinned): int nMinInliers = N * epsilon is a truncated FLOAT product, raised to
 *   min_inliers and min_set; epsilon is raised to (float)minInliers / N; the iteration count uses pow(epsilon, 3) although a
 *   set has four points; minInliers == N gives one iteration; the result is clamped to [1, max_iterations].
 *   N < minInliers (:250-254): no iterations are run whatever `iterations` says, no_more = 1.
 *
 *   Arithmetic: FP64 where the reference is double, in its operation order (sums left to right; the library is built with
 *   -ffp-contract=off), float keypoints and positions widened on use.
 *     sums over a set's points    centroid, PW0^T PW0, M^T M, the camera-frame centroid, ABt and the reprojection sum are each ONE
 *                   lane's loop over the points in the set's order (Refine: ascending index); different entries run on
 *                   different lanes.  No atomics: every sum is bit-reproducible from run to run and from batch to single.
 *     alphas        a[1..3] = (ci[3j] * d0 + ci[3j+1] * d1) + ci[3j+2] * d2, a[0] = ((1 - a[1]) - a[2]) - a[3] (1.0f is exact)
 *     cvSVD of PW0^T PW0 and of M^T M: cyclic two-sided Jacobi in FP64 on the symmetric matrix (the rotation of (p, q) applied
 *                   to the off-diagonal entries of rows / columns p and q and to the columns of V, a_pp -= t a_pq,
 *                   a_qq += t a_pq, a_pq = 0; an entry <= 2^-60 (|a_pp| + |a_qq|) is set to zero unrotated), at most
 *                   ORBX_PNP_JACOBI_SWEEPS / ORBX_PNP_SMALL_SWEEPS sweeps, ended by a sweep without a rotation (the
 *                   later ones would be identities); singular values = |eigenvalues|, descending, the first of equal
 *                   ones first.
 *     cvSolve(CV_SVD) of find_betas_approx_1/2/3, cvInvert(CV_SVD) of the control-point matrix, cvSVD of ABt: one-sided
 *                   (Hestenes) Jacobi on the columns in FP64, ORBX_PNP_SMALL_SWEEPS sweeps, columns with
 *                   |a_p . a_q| <= 2^-49 |a_p| |a_q| left alone; x = V Sigma^-2 (A V)^T b with squared singular values below
 *                   2^-104 of the largest dropped; R = U V^T summed in the Jacobi's column order.
 *     qr_solve      (:1251-1385) restated operation by operation, including the column maximum that looks at rows k .. nr-2;
 *                   on its "A is singular" return the increment is zero (the reference adds an uninitialised one).
 *     CheckInliers  Xc, Yc, invZc are double expressions narrowed to float; ue = uc + (fu * Xc) * invZc and ve in double; distX,
 *                   distY (narrowed differences) and error2 = distX * distX + distY * distY in float; error2 < mvMaxError[i]
 *                   strictly; no depth test, z <= 0 is not special-cased; a NaN model counts zero inliers.
 *     Tcw           refined and best poses narrowed from double to float as :310-316 / :407-413.
 *   PARITY UNPINNED AT THE OPENCV LEVEL: cvSVD, cvSolve(CV_SVD) and cvInvert(CV_SVD) are replaced by the FP64 Jacobi
 *   routines above and least squares built on them; the signs of eigen- and singular vectors; the basis OpenCV picks inside
 *   the four-dimensional null space of M^T M for a minimal set (find_betas_approx_2/3 use individual vectors of it, so which
 *   of the three solutions wins may differ); planar or otherwise rank-deficient control-point sets, where cvInvert takes a
 *   pseudo-inverse; the accumulation order inside cvMulTransposed.
 *
 *   RANSAC sets are the caller's, [iterations][4] indices into the compacted list, distinct inside a set, each drawn by the
 *   reference's draw, overwrite-with-back, pop scheme (:274-290).  The reference draws lazily, four numbers per iteration,
 *   interleaved between the candidates of the round-robin loop; a batched call has to draw ahead, so a caller's rand()
 *   sequence is consumed in ANOTHER ORDER than the reference's.  This is not a parity claim.  `iterations` is the number of
 *   sets handed over; it may exceed mRansacMaxIts (iterate runs past it, :266).
 * ---------------------------------------------------------------------------------- */
/* Sweeps of the 12x12 two-sided Jacobi and of the small ones (3x3 two-sided; one-sided 6x3, 6x4, 6x5, 3x3).  Chosen on the CPU
 * with the same iterations restated in numpy float64 (tests/pnp_ref.py) over 135 sets of 4 to 130 matches of three scenes: both
 * iterations set the rotated entry to zero and stop touching entries that are negligible, so they reach a FIXED POINT - no bit of
 * any output changes after 10 sweeps of the 12x12 (after 9 on all but one set) and after 5 of the small ones; 12 and 8 are run, and
 * tests/test_pnp_solver.py::test_jacobi_sweeps_settled asserts that k, k + 2 and k + 4 sweeps give the same bits. */
#define ORBX_PNP_JACOBI_SWEEPS 12
#define ORBX_PNP_SMALL_SWEEPS 8
#define ORBX_PNP_MAX_MATCHES 65536
/* orbx_pnp_epnp(full): doubles per set and the offsets of the stage outputs inside them */
#define ORBX_PNP_FULL_DOUBLES 472
#define ORBX_PNP_F_CWS 0      /* [4][3] control points                                            */
#define ORBX_PNP_F_PCA 12     /* [3][3] PW0^T PW0                                                 */
#define ORBX_PNP_F_DC 21      /* [3] its singular values, descending                              */
#define ORBX_PNP_F_UCT 24     /* [3][3] rows = its vectors                                        */
#define ORBX_PNP_F_CI 33      /* [3][3] cc_inv                                                    */
#define ORBX_PNP_F_MTM 42     /* [12][12] M^T M                                                   */
#define ORBX_PNP_F_D 186      /* [12] its singular values, descending                             */
#define ORBX_PNP_F_UT 198     /* [12][12] rows = its vectors (the last four span the solution)    */
#define ORBX_PNP_F_L 342      /* [6][10]                                                          */
#define ORBX_PNP_F_RHO 402    /* [6]                                                              */
#define ORBX_PNP_F_B0 408     /* [3][4] betas of find_betas_approx_1, _2, _3                      */
#define ORBX_PNP_F_B1 420     /* [3][4] ... after gauss_newton                                    */
#define ORBX_PNP_F_RS 432     /* [3][3][3]                                                        */
#define ORBX_PNP_F_TS 459     /* [3][3]                                                           */
#define ORBX_PNP_F_ERR 468    /* [3] rep_errors                                                   */
#define ORBX_PNP_F_CHOICE 471 /* N of :750-752 (1, 2 or 3)                                        */

typedef struct orbx_pnp_solver orbx_pnp_solver;
/* ORBX_ERR_ARG: max_candidates < 1, max_matches outside 4..ORBX_PNP_MAX_MATCHES, max_iterations < 1 (the last two are PER
 * CANDIDATE limits); then ORBX_ERR_NODEVICE without a device */
int orbx_pnp_solver_create(int device, int max_candidates, int max_matches, int max_iterations, orbx_pnp_solver **out);
void orbx_pnp_solver_destroy(orbx_pnp_solver *h);

typedef struct orbx_pnp_problem {      /* host memory: one candidate */
    float fx, fy, cx, cy;
    int n;                             /* kept matches                                                               */
    const float *p2d;                  /* [n][2] mvP2D                                                               */
    const float *sigma2;               /* [n] mvLevelSigma2[octave]                                                  */
    const float *p3dw;                 /* [n][3] mvP3Dw                                                              */
    double probability;                /* the SetRansacParameters arguments                                          */
    int min_inliers, max_iterations, min_set;
    float epsilon, th2;
    const int32_t *sets;               /* [iterations][4]                                                            */
    int iterations;                    /* sets handed over (>= mRansacMaxIts for a caller that iterates past it)     */
} orbx_pnp_problem;

typedef struct orbx_pnp_result {       /* host memory: one candidate; every pointer may be NULL.  it = iterations run */
    int32_t *count;                    /* [it] mnInliersi                                                            */
    double *r, *t, *err;               /* [it][9], [it][3], [it]: mRi, mti and compute_pose's return value           */
    int32_t *record_of;                /* [it] index of the latest record at or before the iteration, -1 = none yet  */
    uint8_t *is_event;                 /* [it] iterate returns at this iteration                                     */
    int32_t *nrecords;
    int32_t *record_iteration;         /* [it], the first nrecords entries: the iteration of each record             */
    int32_t *refined_count;            /* [it], the first nrecords entries: mnRefinedInliers                         */
    double *refined_r, *refined_t;     /* [it][9], [it][3], the first nrecords entries                               */
    float *refined_tcw;                /* [it][12], the first nrecords entries: rows of [R | t] of mRefinedTcw       */
    float *best_tcw;                   /* [12] mBestTcw after all iterations (zeros without a record)                */
    int32_t *first_event;              /* the first returning iteration, -1 = none                                   */
    int32_t *best_iteration;           /* the last record's iteration, -1 = no iteration reached min_inliers         */
    int32_t *no_more;                  /* n < min_inliers: nothing was run                                           */
    int32_t *min_inliers;              /* mRansacMinInliers after SetRansacParameters                                */
    uint8_t *inliers_first;            /* [n] mvbRefinedInliers of the first event, COMPACTED indices; zeros without */
    uint8_t *inliers_best;             /* [n] mvbBestInliers after all iterations; zeros without a record            */
    float *max_error;                  /* [n] mvMaxError (diagnostic, a copy of its own behind the call)             */
} orbx_pnp_result;
/* ORBX_ERR_ARG: ncandidates < 1, a NULL problem / array, n < 0, iterations < 0, n < 4 with iterations to run, a set index
 * outside [0, n), a repeated index inside a set; ORBX_ERR_CAPACITY: more candidates, matches or iterations than the handle
 * was created for.  Nothing is launched on an error and the handle stays usable. */
int orbx_pnp_solve(orbx_pnp_solver *h, const orbx_pnp_problem *problems, int ncandidates, const orbx_pnp_result *results);
/* One row [n] of the device's masks of the last orbx_pnp_solve: refined = 0, mvbInliersi of iteration `index`; refined = 1,
 * mvbRefinedInliers of record `index`.  ORBX_ERR_STATE before a solve, ORBX_ERR_ARG outside it. */
int orbx_pnp_inliers(orbx_pnp_solver *h, int candidate, int index, int refined, uint8_t *inliers);
/* CheckInliers of m <= max_iterations explicit poses r[m][9], t[m][3] (double) over the problem's matches with the chain's
 * kernel: count[m], inliers[m][n] (may be NULL).  sets / iterations are not read. */
int orbx_pnp_check_models(orbx_pnp_solver *h, const orbx_pnp_problem *problem, const double *r, const double *t, int m,
                          int32_t *count, uint8_t *inliers);
/* compute_pose of m <= max_iterations explicit index sets sets[m][set_size], 4 <= set_size <= n, distinct inside a set, with
 * the chain's kernel: r[m][9], t[m][3], err[m]; full[m][ORBX_PNP_FULL_DOUBLES] (the stage outputs, ORBX_PNP_F_*) and
 * alphas[m][set_size][4] may be NULL.  ORBX_ERR_ARG: set_size < 4 or > n, a bad or repeated index. */
int orbx_pnp_epnp(orbx_pnp_solver *h, const orbx_pnp_problem *problem, const int32_t *sets, int m, int set_size, double *r,
                  double *t, double *err, double *full, double *alphas);
/* SetRansacParameters (:181-223) with the reference's libm calls; n = number of kept matches.  No device.  Outputs may be
 * NULL: mRansacMinInliers, mRansacMaxIts, mRansacEpsilon. */
int orbx_pnp_ransac_parameters(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                               int n, int *min_inliers_out, int *iterations_out, float *epsilon_out);
/* device time of the last orbx_pnp_solve chain (first to last kernel) and its kernel launches */
int orbx_pnp_last_timing(orbx_pnp_solver *h, float *device_ms, int *launches);

/* ----------------------------------------------------------------------------------
 * Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1017-1339 with the vendored g2o): the pose graph of
 * LoopClosing::CorrectLoop - every keyframe a 7-dof VertexSim3Expmap, every LoopConnections / spanning-tree / loop /
 * covisibility pair an EdgeSim3 with identity information and no robust kernel - under g2o's Levenberg driver with
 * setUserLambdaInit(1e-16), then the pose and map-point write-back.  The host (the shim) walks the pointers and selects the
 * edges; the device does the arithmetic.
 *
 *   k_eg_init       measurements Sji = Sjw * Swi (Sim3::inverse, operator*; kind 0 from `est`, kind 1 from `meas`)
 *   k_eg_linearize  16 threads per edge: 14 take one column each of g2o's central differences (delta = 1e-9, through oplus =
 *                   Sim3(update) * estimate, update[6] = 0 under fix_scale; a fixed vertex has no block), one the error
 *                   log(C * v1 * v2^-1) at the estimate (Sim3::log's four branches; W u = t by the adjugate)
 *   k_eg_assemble   one wave per block of H on the pattern of L: the edges' J^T J in edge order, each entry a sum over the
 *                   seven rows in row order; b += J^T (-e) likewise.  Every copy of a duplicated edge is added.  No atomics.
 *   k_eg_solve      (H + lambda I) x = b: block-sparse FP64 LDL^T on 7x7 blocks, right-looking, no pivoting, in ONE
 *                   workgroup (column steps are dependent; nothing waits across workgroups), then both substitutions,
 *                   x . (lambda x + b), and the trial estimates Sim3(x) * estimate.  A non-positive or non-finite pivot
 *                   makes the trial's chi2 DBL_MAX.  Under fix_scale the seventh pivot of every block is lambda itself and
 *                   the seventh component of x exactly 0.
 *   k_eg_error / k_eg_reduce   the trial's errors, chi2 = e^T e per edge, and their sum in a fixed order; one 32-byte record
 *                   per trial in mapped pinned memory behind a sequence word, from which the host takes the Levenberg
 *                   decision (optimization_algorithm_levenberg.cpp:61-164, as orbx_optimize_sim3's list above says, with
 *                   lambda0 = lambda_init).  No copy engine and no stream synchronisation inside the loop.
 *   k_eg_writeback  the estimates, their inverses (vCorrectedSwc), Tiw = [R | t / s] narrowed to float, and the map points
 *                   float(correctedSwr.map(Srw.map(double(p)))).
 *
 *   The symbolic phase runs on the host once per call: the elimination order (the free keyframes in the caller's order) and
 *   the exact block pattern of L.  Device memory is proportional to that pattern, never to n^2.  fill_blocks counts the blocks
 *   of L's lower triangle, diagonal blocks included.
 *   Arithmetic: FP64, every product / sum / quotient its own IEEE operation, in the order tests/essential_graph_ref.py
 *   restates; exp, sin, cos, log and acos are the kernels' own series of IEEE operations (a few ulps from libm's), restated too.
 *   PARITY UNPINNED against the reference: libm's last bits of those five; W.lu().solve (the adjugate here); the order of
 *   the block sums and Eigen's sparse LDL^T with its AMD ordering (natural order, no pivoting here).
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_essential_graph orbx_essential_graph;
/* ORBX_ERR_ARG: max_keyframes < 1, max_edges outside 0..2^26, max_points < 0, max_fill_blocks < 1; then ORBX_ERR_NODEVICE without a device */
int orbx_essential_graph_create(int device, int max_keyframes, int max_edges, int max_points, int max_fill_blocks,
                                orbx_essential_graph **out);
void orbx_essential_graph_destroy(orbx_essential_graph *h);

#define ORBX_EG_MAX_TRIALS 10      /* _maxTrialsAfterFailure */
#define ORBX_EG_END_ITERATIONS 0   /* why a run ended: every iteration ran, */
#define ORBX_EG_END_TRIALS 1       /* ten trials in one iteration,          */
#define ORBX_EG_END_RHO0 2         /* rho == 0,                             */
#define ORBX_EG_END_THREE 3        /* three iterations without progress     */

typedef struct orbx_essential_graph_problem {   /* host memory */
    int n;                          /* keyframes, in the caller's order (the shim: ascending mnId)                     */
    const double *est;              /* [n][8] q (x, y, z, w), t, s: vScw                                                */
    const double *meas;             /* [n][8] NonCorrectedSim3 where present, else est; NULL = est                      */
    int fixed;                      /* index of the loop keyframe                                                       */
    int fix_scale;
    int n_edges;
    const int32_t *edges;           /* [n_edges][3] i (vertex 0), j (vertex 1), kind (0: from est, 1: from meas)        */
    int n_points;
    const float *points;            /* [n_points][3]                                                                    */
    const int32_t *point_ref;       /* [n_points] vertex index of the reference keyframe, -1 = no vertex                */
    int iterations;                 /* <= 0: 20                                                                         */
    double lambda_init;             /* <= 0: 1e-16                                                                      */
} orbx_essential_graph_problem;

typedef struct orbx_essential_graph_result {    /* host memory; every pointer may be NULL */
    double *est;                    /* [n][8] the final estimates                                                       */
    float *tiw;                     /* [n][12] rows of [R | t / s]                                                      */
    double *inv;                    /* [n][8] their inverses (vCorrectedSwc)                                            */
    float *points;                  /* [n_points][3]                                                                    */
    double *chi2;                   /* [2] initial, final                                                               */
    int32_t *iterations;            /* [1] iterations run                                                               */
    int32_t *ended;                 /* [1] ORBX_EG_END_*                                                                */
    int32_t *iter_trials;           /* [iterations] trials of each iteration                                            */
    double *iter_chi2, *iter_lambda, *iter_rho;   /* [iterations] chi2 and lambda after it, rho of its last trial       */
    int32_t *order;                 /* [n - 1] the elimination order: vertex indices of the free keyframes              */
    int32_t *fill_blocks;           /* [1]                                                                              */
} orbx_essential_graph_result;
/* ORBX_ERR_ARG, before any launch: n < 1, fixed or an edge index or a point_ref outside its range, i == j, kind not 0 / 1,
 * s <= 0, a non-finite input; ORBX_ERR_CAPACITY: more keyframes, edges, points or fill blocks than the handle was created
 * for.  The handle stays usable.  n_edges == 0 is not an error: the estimates come back as passed in. */
int orbx_optimize_essential_graph(orbx_essential_graph *h, const orbx_essential_graph_problem *problem,
                                  const orbx_essential_graph_result *result);
/* ONE linearisation at the explicit estimates at[n][8] (NULL = problem->est) with the chain's kernels: meas[E][8] the edges'
 * measurements, errors[E][7], chi2[1], jac[E][2][7][7] (vertex 0 / 1, row, column; zeros for the fixed vertex), h_diag[n][49]
 * and b[n][7] by vertex (zeros for the fixed one), h_off[E][49] the assembled block H(i, j) of each edge's pair (zeros when
 * either end is fixed).  Every output may be NULL. */
int orbx_essential_graph_linearize(orbx_essential_graph *h, const orbx_essential_graph_problem *problem, const double *at,
                                   double *meas, double *errors, double *chi2, double *jac, double *h_diag, double *h_off, double *b);
/* (H + lambda I) x = b on the last orbx_essential_graph_linearize: x[n][7] by vertex (zeros for the fixed one), ok[1] = 0 on
 * a non-positive or non-finite pivot, and x is then all zeros.  ORBX_ERR_STATE without a linearisation. */
int orbx_essential_graph_solve(orbx_essential_graph *h, double lambda, double *x, int32_t *ok);
/* device time of the last orbx_optimize_essential_graph chain, its kernel launches, and the part of that time inside
 * k_eg_solve (factorisation and substitutions; the kernel's own clock: what tools/latency_essential_graph.py reports as the
 * factorisation's share).  Every output may be NULL. */
int orbx_essential_graph_last_timing(orbx_essential_graph *h, float *device_ms, int *launches, float *solve_ms);

/* ----------------------------------------------------------------------------------
 * KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:104-374) with
 * L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and the minimum-score loop of LoopClosing::DetectLoop
 * (src/LoopClosing.cc:160-176): place recognition for all queries of a call in one chain.  The database lives on the device:
 * an append-only pool of (word, value) entries and per keyframe id, `add` sequence number, offset, length, alive, the
 * up-to-ten best covisible ids and the persistent reloc_score.  There is no inverted file: the order of the reference's
 * lKFsSharingWords is the order by (smallest word shared with the query, `add` sequence number), which every keyframe finds
 * by intersecting its own sorted BowVector with the query (tests/test_kfdb.py proves the equivalence on a literal restatement
 * of the inverted-file walk).
 *
 *   k_kfdb_intersect  per (query, alive keyframe): shared words, first shared word; per query n_sharing and maxCommonWords
 *                     over the keyframes outside the connected set; minCommonWords = (int)((float)maxCommonWords * 0.8f)
 *   k_kfdb_score      the keyframes with words > minCommonWords and, loop mode, the connected ones: sum += fabs(v - w) -
 *                     fabs(v) - fabs(w) over the shared words in ascending order by one running double sum (no tree),
 *                     score = (float)(-sum / 2.0)
 *   k_kfdb_commit     the reloc_score state behind this call
 *   k_kfdb_select     the scored keyframes ranked by (first word, seq); minScore; lScoreAndMatch; the covisibility groups in
 *                     float with the strictly-greater best; bestAccScore; 0.75f; each group's best keyframe once, at its
 *                     first occurrence; results into mapped pinned memory
 *
 *   erase clears `alive`; an `add` that finds more dead entries than half of the entries in use (or that needs the room)
 *   compacts pool and slots first, keeping the sequence numbers.
 *   Loop mode: a covisible contributes only if THIS query scored it (:201).  minScore = min(min_score_in, the float scores of
 *   the listed connected keyframes that are in the database and have a count != 0).
 *   Relocalisation mode keeps the reference's quirk (:336-339): a covisible that shares at least one word with the query
 *   contributes its reloc_score even when this query did not score it.  Within one call a query reads its own score where it
 *   scored a keyframe and otherwise the value from before the call; after the call every keyframe holds the score of the
 *   highest-numbered relocalisation query that scored it (nq = 1: the reference exactly).
 *   PARITY UNPINNED against the reference: reloc_score is 0 from `add` until a query scores the keyframe (mRelocScore is
 *   uninitialised there); a query reads the covisibles as last pushed by orbx_kfdb_set_covisibles, not as of the query.
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_kf_database orbx_kf_database;
#define ORBX_KFDB_LOOP 0
#define ORBX_KFDB_RELOC 1
#define ORBX_KFDB_MAX_QUERY_WORDS 8192

typedef struct orbx_kfdb_query_t {      /* host memory */
    int mode;                        /* ORBX_KFDB_LOOP / ORBX_KFDB_RELOC                                                 */
    const int32_t *words;            /* [n] ascending, distinct, 0..n_words-1: the BowVector in map order                */
    const double *values;            /* [n]                                                                              */
    int n;
    const int64_t *connected;        /* [n_connected] loop mode: GetConnectedKeyFrames (ids need not be present)         */
    const int32_t *connected_counts; /* [n_connected] 0 = isBad(): excluded from the sharers, not part of minScore       */
    int n_connected;
    float min_score_in;              /* loop mode: what the caller scored itself (1.0f = nothing)                        */
    int capacity;                    /* entries of each list output of this query's result                               */
} orbx_kfdb_query_t;

typedef struct orbx_kfdb_result {       /* host memory; every pointer may be NULL */
    int32_t *n_sharing;              /* lKFsSharingWords.size()                                                          */
    int32_t *max_common_words, *min_common_words;
    float *min_score;                /* loop mode; 0 in relocalisation mode                                              */
    float *connected_score;          /* [n_connected] loop mode; -1 where the id is not in the database                  */
    int64_t *scored_id;              /* [n_scored] the keyframes with words > minCommonWords in the reference's order    */
    int32_t *scored_words;           /* ... mnLoopWords / mnRelocWords                                                   */
    float *scored_score;             /* ... mLoopScore / mRelocScore                                                     */
    int32_t *n_scored;
    int32_t *kept;                   /* [n_kept] lScoreAndMatch: index into the scored list                              */
    float *acc_score;                /* [n_kept] lAccScoreAndMatch: accScore                                             */
    int64_t *best_id;                /* [n_kept] ... pBestKF                                                             */
    int32_t *n_kept;
    float *best_acc_score;           /* bestAccScore (its start value, minScore or 0, where lScoreAndMatch is empty)     */
    int64_t *candidates;             /* [n_candidates]                                                                   */
    int32_t *n_candidates;
} orbx_kfdb_result;

/* ORBX_ERR_ARG: n_words, max_keyframes, max_entries, max_queries < 1, max_query_words outside 1..ORBX_KFDB_MAX_QUERY_WORDS,
 * max_queries * max_keyframes > 2^28; then ORBX_ERR_NODEVICE without a device */
int orbx_kfdb_create(int device, int n_words, int max_keyframes, int max_entries, int max_queries, int max_query_words,
                     orbx_kf_database **out);
void orbx_kfdb_destroy(orbx_kf_database *h);
/* ORBX_ERR_ARG: NULL handle, n < 0, a word outside 0..n_words-1, unsorted or repeated words; ORBX_ERR_STATE: the id is
 * present; ORBX_ERR_CAPACITY: no slot or no room in the pool even after compaction (the database is unchanged). */
int orbx_kfdb_add(orbx_kf_database *h, int64_t id, const int32_t *words, const double *values, int n);
int orbx_kfdb_erase(orbx_kf_database *h, int64_t id);          /* absent id: ORBX_OK, as the reference */
int orbx_kfdb_clear(orbx_kf_database *h);
/* n <= 10 ids in GetBestCovisibilityKeyFrames(10) order; they need not be present (an id added later counts from then on).
 * ORBX_ERR_ARG: n outside 0..10; ORBX_ERR_STATE: `id` is not in the database. */
int orbx_kfdb_set_covisibles(orbx_kf_database *h, int64_t id, const int64_t *ids, int n);
/* alive keyframes, pool entries in use (dead ones included), dead entries; every output may be NULL */
int orbx_kfdb_size(orbx_kf_database *h, int *keyframes, int *entries, int *dead_entries);
/* the persistent reloc_score of a keyframe; ORBX_ERR_STATE: not in the database */
int orbx_kfdb_reloc_score(orbx_kf_database *h, int64_t id, float *score);
/* ORBX_ERR_ARG: nq < 1, an unknown mode, bad words (as orbx_kfdb_add), n_connected < 0, capacity < 0; ORBX_ERR_CAPACITY: more
 * queries or query words than the handle was created for (nothing runs), or a list longer than its query's capacity (nothing
 * is written to any result; the queries HAVE run, so the reloc scores are those after the call).  An empty database, n = 0 and
 * a query that shares no word give empty lists and ORBX_OK. */
int orbx_kfdb_query(orbx_kf_database *h, const orbx_kfdb_query_t *queries, int nq, const orbx_kfdb_result *results);
/* device time of the last orbx_kfdb_query chain and its kernel launches (0, 0 when nothing was launched) */
int orbx_kfdb_last_timing(orbx_kf_database *h, float *device_ms, int *launches);
/* Measurement only: stage_ms[5] (may be NULL) = device time of the last query's staging, k_kfdb_intersect, k_kfdb_score,
 * k_kfdb_commit and k_kfdb_select, when that query ran with the events enabled (ORBX_ERR_STATE otherwise); then `enable`
 * switches the four extra event records per query on or off (off in a new handle). */
int orbx_kfdb_stage_timing(orbx_kf_database *h, int enable, float *stage_ms);

/* ----------------------------------------------------------------------------------
 * Covisibility: the counting inside KeyFrame::UpdateConnections (reference src/KeyFrame.cc:386-507), the vote that opens
 * Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1895-1955) and LocalMapping::KeyFrameCulling (src/LocalMapping.cc:873-956).
 * Integer counting over ragged observation lists: every result is exact.  Stateless and synchronous: a slice of the map in
 * host arrays goes in, host arrays come out, one wait per call (per culling round, see below).  AddConnection, the spanning
 * tree and the rest of SetBadFlag stay with the caller (shim/Covisibility_hip.cc).
 *
 * The slice.  num_keyframes slots: every keyframe the call names as a list owner or an observer.  kf_rank are distinct values
 * that give the iteration order of std::map<KeyFrame*, ...> (the rank of the pointer value); kf_flags bit 0: mnId == 0, bit 1:
 * mbNotErase, bit 2: isBad().  Points: CSR observation lists (obs_offset, obs_kf = the observer's slot, obs_octave =
 * mvKeysUn[idx].octave there, obs_stereo = mvuRight[idx] >= 0), a keyframe at most once per point; point_bad.  A point's
 * Observations() is the sum of 1 (2 where obs_stereo) over its observations: derived, not passed.  Lists: CSR (list_offset),
 * list_kf = the owner's slot or -1 for a Frame, list_point = the non-NULL mvpMapPoints in feature order (a point may repeat:
 * both entries count), list_octave = mvKeysUn[i].octave, list_close = 0 where the sensor is not monocular and mvDepth[i] is
 * beyond mThDepth or negative, else 1.  The octave, stereo and close arrays are read by the culling only and may be NULL for
 * orbx_covis_update_connections.
 *
 * orbx_covis_update_connections, all lists of the call in one launch.  Per list: KFcounter over the points that are not bad,
 * without the owner, as (slot, weight) in ascending rank; n_max / kf_max = the first slot in ascending rank with the strictly
 * greatest weight (a Frame's list, list_kf = -1: slots flagged bad are no candidates but stay in the counter; kf_max = -1
 * and n_max = 0 when no candidate is left); the connections = the slots with weight >= th by descending weight and, within a
 * weight, descending rank (sort + push_front of pair<int, KeyFrame*>), or the single (kf_max, n_max) when none reaches th.
 * An empty counter: n_counter = 0, kf_max = -1, no connection.  The histogram of a list lives in LDS up to
 * ORBX_COVIS_LDS_KEYFRAMES slots and in device memory beyond: the results are the same.
 *
 * orbx_covis_keyframe_culling: the lists are vpLocalKeyFrames in the caller's order, each owned by a different keyframe.
 * Equal to the sequential loop with its side effects: a keyframe with bit 0 is skipped; n_mps counts the entries that are not
 * bad and are close; n_redundant those of them with Observations() > 3 and at least 3 live observers other than the owner
 * with obs_octave <= list_octave + 1; culled = n_redundant > 0.9 * n_mps as the double product.  A culled keyframe without
 * bit 1 has its observations erased before the next list is looked at: each of its points loses 1 or 2 from Observations()
 * and goes bad (for good, with all its observations) when that leaves <= 2; only an erase makes a point bad.  A culled
 * keyframe with bit 1 is reported and changes nothing.  c erasing culls take c + 1 rounds: 2 c + 3 launches, c + 1 waits.
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_covis orbx_covis;
#define ORBX_COVIS_LDS_KEYFRAMES 4096

typedef struct orbx_covis_slice {       /* host memory */
    int num_keyframes;
    const int32_t *kf_rank;          /* [num_keyframes] distinct                                                         */
    const uint8_t *kf_flags;         /* [num_keyframes]                                                                  */
    int num_points, num_obs;
    const int32_t *obs_offset;       /* [num_points + 1]                                                                 */
    const int32_t *obs_kf;           /* [num_obs] 0..num_keyframes-1                                                     */
    const uint8_t *obs_octave;       /* [num_obs]                                                                        */
    const uint8_t *obs_stereo;       /* [num_obs]                                                                        */
    const uint8_t *point_bad;        /* [num_points]                                                                     */
    int num_lists, num_entries;
    const int32_t *list_offset;      /* [num_lists + 1]                                                                  */
    const int32_t *list_kf;          /* [num_lists] owner slot, -1 = a Frame (update_connections only)                   */
    const int32_t *list_point;       /* [num_entries] 0..num_points-1                                                    */
    const uint8_t *list_octave;      /* [num_entries]                                                                    */
    const uint8_t *list_close;       /* [num_entries]                                                                    */
} orbx_covis_slice;

typedef struct orbx_covis_connections {  /* host memory; every pointer may be NULL */
    int32_t *counter_offset;         /* [num_lists + 1] CSR of the counters: n_counter of list q = the difference        */
    int32_t *counter_kf, *counter_weight;   /* [counter_capacity]                                                        */
    int counter_capacity;
    int32_t *n_max, *kf_max;         /* [num_lists]                                                                      */
    int32_t *conn_offset;            /* [num_lists + 1] CSR of the ordered connections                                   */
    int32_t *conn_kf, *conn_weight;  /* [conn_capacity]                                                                  */
    int conn_capacity;
} orbx_covis_connections;

typedef struct orbx_covis_culling {      /* host memory; every pointer may be NULL */
    int32_t *n_mps, *n_redundant;    /* [num_lists]                                                                      */
    uint8_t *culled;                 /* [num_lists]                                                                      */
    uint8_t *point_bad;              /* [num_points] after the loop                                                      */
    int32_t *point_obs;              /* [num_points] Observations() after the loop                                       */
} orbx_covis_culling;

/* ORBX_ERR_ARG: NULL out, device out of range; ORBX_ERR_NODEVICE without a device */
int orbx_covis_create(int device, orbx_covis **out);
void orbx_covis_destroy(orbx_covis *h);
/* ORBX_ERR_ARG, before anything is launched: a NULL array, num_keyframes or num_lists < 1, an offset array that does not
 * start at 0, decreases or does not end at its total, a slot or point index out of range, two slots with one rank, a negative
 * capacity.  ORBX_ERR_CAPACITY: the counters (the connections) of all lists together exceed counter_capacity
 * (conn_capacity): nothing is written to any output; the handle stays usable. */
int orbx_covis_update_connections(orbx_covis *h, const orbx_covis_slice *slice, int th, const orbx_covis_connections *out);
/* ORBX_ERR_ARG as above, and: a list without an owner, two lists of one keyframe */
int orbx_covis_keyframe_culling(orbx_covis *h, const orbx_covis_slice *slice, const orbx_covis_culling *out);
/* device time of the last call's chain (the host's decisions between culling rounds included) and its kernel launches */
int orbx_covis_last_timing(orbx_covis *h, float *kernel_ms, int *launches);

/* ----------------------------------------------------------------------------------
 * Loop correction: the two passes of the loop closer that move the map.  orbx_loop_correct_sim3 is the Sim3 propagation of
 * LoopClosing::CorrectLoop (reference src/LoopClosing.cc:617-716), orbx_loop_propagate_gba the map update after global bundle
 * adjustment (:930-1003).  Stateless and synchronous: host arrays in, host arrays out, one launch chain and one wait per call;
 * the handle has no capacities, its buffers grow.  Keyframes are slot numbers 0..num_keyframes-1; a pose is the 12 floats of the
 * first three rows of the 4x4 Tcw, a Sim3 is 8 doubles q(x, y, z, w), t, s (the layout of orbx_essential_graph_problem.est).
 * Float results are bit for bit those of the reference on the project's OpenCV stand-in: every 4x4 and 3x3 product is a float
 * sum accumulated left to right over all its terms, the Sim3 arithmetic is g2o's in double, operation by operation.
 *
 * orbx_loop_correct_sim3.  The group = mvpCurrentConnectedKFs in the order in which the reference iterates CorrectedSim3 (a
 * std::map<KeyFrame*, ...>: ascending pointer; the caller's order here), `current` = the position of mpCurrentKF in it, scw =
 * mg2oScw.  Twc of the current keyframe is DERIVED on the device from its tcw by KeyFrame::SetPose's own steps (Rwc = Rcw^T,
 * Ow = (-Rwc) * tcw), so tcw must be what the keyframe's last SetPose was given; ow is GetCameraCenter() as stored.  Lists:
 * CSR over the group, list_point = GetMapPointMatches() with -1 for a NULL entry.  Points: point_done = mnCorrectedByKF ==
 * mpCurrentKF->mnId already, point_ref = the slot of mpRefKF, ref_scale / top_scale as in orbx_mappoint_batch; CSR observation
 * lists in the order of the observation map, never reordered.
 *   noncorrected[g] = Sim3(Riw, tiw, 1); corrected[g] = Sim3(Ric, tic, 1) * scw with Tic = Tiw * Twc, or scw itself at `current`;
 *   tiw[g] = [R | t / s] of corrected[g] (toRotationMatrix, t *= 1. / s, toCvSE3), ow_new[g] the centre SetPose derives from it;
 *   scw_mat[g] = Converter::toCvMat(corrected[g]) = [sR | t], what orbx_fuse_search takes for SearchAndFuse.
 *   A point is moved ONCE, by the first group position whose list holds it while it is neither bad nor done: pos =
 *   corrected.inverse().map(noncorrected.map(double(P))) narrowed to float, corrected_by = that position (mnCorrectedReference
 *   is that keyframe's id), -1 and the old position for an untouched point.  UpdateNormalAndDepth runs at that moment: group
 *   keyframes at EARLIER positions have had their SetPose, so their centre (as an observer and as the reference keyframe) is
 *   ow_new, every other centre is ow.  normal / max_dist / min_dist / updated as in orbx_mappoint_result (updated = moved and
 *   observed; the rest 0 otherwise).
 *
 * orbx_loop_propagate_gba.  parent[i] = the slot of the spanning-tree parent, -1 for a member of mvpKeyFrameOrigins, -2 for a
 * keyframe outside the tree (the walk never reaches it, nor its descendants).  in_gba = mnBAGlobalForKF == nLoopKF before the
 * walk; tcw_gba = mTcwGBA where in_gba (and of the origins), ignored elsewhere.
 *   tcw_gba, completed: a reached keyframe with in_gba == 0 and a parent gets (Tchild * Twc_parent) * TcwGBA_parent, both factors
 *   of the first product from the poses before the update; everything else is returned as it came.  reached[i] = the walk
 *   visits i (then mnBAGlobalForKF == nLoopKF, mTcwBefGBA = tcw and SetPose(tcw_gba) hold after it).
 *   moved[p]: 0 untouched (bad, point_ref -1, or the reference keyframe not reached), 1 copied from pos_gba (point_in_gba),
 *   2 re-projected: Rwc * (Rcw_bef * X + tcw_bef) + twc with Rwc, twc as SetPose(tcw_gba) stores them.
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_loop orbx_loop;

typedef struct orbx_loop_sim3_problem {  /* host memory */
    int num_keyframes;
    const float *tcw;                /* [num_keyframes][12]                                                              */
    const float *ow;                 /* [num_keyframes][3]                                                               */
    int num_group, current;
    const int32_t *group_kf;         /* [num_group] distinct slots                                                       */
    const double *scw;               /* [8]                                                                              */
    int num_entries;
    const int32_t *list_offset;      /* [num_group + 1]                                                                  */
    const int32_t *list_point;       /* [num_entries] 0..num_points-1, or -1                                             */
    int num_points, num_obs;
    const float *pos;                /* [num_points][3]                                                                  */
    const uint8_t *point_bad, *point_done;   /* [num_points]                                                             */
    const int32_t *point_ref;        /* [num_points] 0..num_keyframes-1                                                  */
    const float *ref_scale, *top_scale;      /* [num_points]                                                             */
    const int32_t *obs_offset;       /* [num_points + 1]                                                                 */
    const int32_t *obs_kf;           /* [num_obs] 0..num_keyframes-1                                                     */
} orbx_loop_sim3_problem;

typedef struct orbx_loop_sim3_result {   /* host memory; every pointer may be NULL */
    double *noncorrected, *corrected;        /* [num_group][8]                                                           */
    float *tiw;                      /* [num_group][12]                                                                  */
    float *ow_new;                   /* [num_group][3]                                                                   */
    float *scw_mat;                  /* [num_group][12]                                                                  */
    float *pos;                      /* [num_points][3]                                                                  */
    int32_t *corrected_by;           /* [num_points]                                                                     */
    float *normal;                   /* [num_points][3]                                                                  */
    float *max_dist, *min_dist;      /* [num_points]                                                                     */
    uint8_t *updated;                /* [num_points]                                                                     */
} orbx_loop_sim3_result;

typedef struct orbx_loop_gba_problem {   /* host memory */
    int num_keyframes;
    const int32_t *parent;           /* [num_keyframes] slot, -1 origin, -2 not in the tree                              */
    const float *tcw, *tcw_gba;      /* [num_keyframes][12]                                                              */
    const uint8_t *in_gba;           /* [num_keyframes]                                                                  */
    int num_points;
    const float *pos, *pos_gba;      /* [num_points][3]                                                                  */
    const uint8_t *point_in_gba, *point_bad; /* [num_points]                                                             */
    const int32_t *point_ref;        /* [num_points] slot, or -1                                                         */
} orbx_loop_gba_problem;

typedef struct orbx_loop_gba_result {    /* host memory; every pointer may be NULL */
    float *tcw_gba;                  /* [num_keyframes][12]                                                              */
    uint8_t *reached;                /* [num_keyframes]                                                                  */
    float *pos;                      /* [num_points][3]                                                                  */
    uint8_t *moved;                  /* [num_points]                                                                     */
} orbx_loop_gba_result;

/* ORBX_ERR_ARG: NULL out, device out of range; ORBX_ERR_NODEVICE without a device */
int orbx_loop_create(int device, orbx_loop **out);
void orbx_loop_destroy(orbx_loop *h);
/* ORBX_ERR_ARG, before the handle is looked at and before anything is launched: a NULL required array, an offset array that does
 * not start at 0, decreases or does not end at its total, a slot or point index out of range, two group entries with one slot,
 * `current` out of range, a scale of scw that is not positive, a pose, centre or point that is not finite.  `result` may be NULL. */
int orbx_loop_correct_sim3(orbx_loop *h, const orbx_loop_sim3_problem *problem, const orbx_loop_sim3_result *result);
/* ORBX_ERR_ARG likewise: a NULL required array, a parent or point_ref out of range, a keyframe that is its own ancestor, no
 * origin, a pose or point that is not finite */
int orbx_loop_propagate_gba(orbx_loop *h, const orbx_loop_gba_problem *problem, const orbx_loop_gba_result *result);
/* device time of the last call's launch chain and its kernel launches */
int orbx_loop_last_timing(orbx_loop *h, float *device_ms, int *launches);


/* ------------------------------------------------------------------------------------
 * Image front end  ==  what the reference does to a camera image BEFORE ORBextractor::operator():
 *   colour to grey     Tracking::GrabImageMonocular / GrabImageStereo / GrabImageRGBD (src/Tracking.cc:250-278, 311-326, 369-384):
 *                      cvtColor(RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY) by mbRGB
 *   rectification      Examples/Stereo/stereo_euroc.cc:124-134, 181-188: cv::initUndistortRectifyMap once, cv::remap(INTER_LINEAR) per image
 * A batch of frames in device memory goes in; grey, rectified frames come out in a handle-owned device buffer in the padded layout
 * orbx_extract_batch_device prefers (stride >= round_up(width, 4) + 12, frame_pitch = stride * height, every pad byte 0).
 *
 * Arithmetic (the project's pinned choice; PARITY WITH OpenCV IS UNPINNED - the OpenCV version and its SIMD path, the LU inverse of
 * initUndistortRectifyMap and remap's weight fix-up are not reproduced bit for bit; tests/imgprep_ref.py is the
 * restatement the device is held to, byte for byte):
 *   grey    (c[R] r + c[G] g + c[B] b + (1 << (shift - 1))) >> shift in 32-bit unsigned; the alpha byte of 4-channel input is ignored.
 *   maps    once per map: sx = rint(map_x * 32), sy = rint(map_y * 32) (half to even; |s| clamped to 2^30, which changes no result);
 *           ix = saturate_int16(sx >> 5) (arithmetic shift), fx = sx & 31; iy, fy likewise.
 *   remap   taps p00 = src(iy, ix), p01 = src(iy, ix + 1), p10 = src(iy + 1, ix), p11 = src(iy + 1, ix + 1), a tap outside the image
 *           reads 0 (BORDER_CONSTANT, value 0: cv::remap's default);
 *           out = ((32 - fx)(32 - fy) p00 + fx (32 - fy) p01 + (32 - fx) fy p10 + fx fy p11 + 512) >> 10.
 *   ORDER   colour input that is also rectified is converted to grey FIRST (per tap) and the grey image is remapped, in one launch:
 *           the reference's examples rectify grey images.  Remapping the colour planes and converting afterwards rounds differently
 *           and is not offered.
 * ---------------------------------------------------------------------------------- */
typedef struct orbx_image_prep orbx_image_prep;

typedef struct orbx_image_prep_config {
    int device;                 /* HIP device ordinal                                                             */
    int max_width, max_height;  /* largest image accepted (each 1..16384)                                         */
    int max_batch;              /* most frames per call (>= 1)                                                    */
    /* 8-bit fixed-point grey weights of R, G, B.  All zero selects OpenCV 4.x's 9798, 19235, 3735 with shift 15; OpenCV 3.x used
     * 4899, 9617, 1868 with shift 14.  The sum must be 1 << gray_shift and gray_shift must lie in 8..16 (ORBX_ERR_ARG otherwise). */
    uint16_t gray_coef[3];
    uint16_t gray_shift;
} orbx_image_prep_config;

/* ORBX_ERR_ARG: NULL argument, a size out of range, bad grey weights, device out of range; ORBX_ERR_NODEVICE without a device */
int orbx_image_prep_create(const orbx_image_prep_config *cfg, orbx_image_prep **out);
void orbx_image_prep_destroy(orbx_image_prep *h);

/* cv::initUndistortRectifyMap(K, D, R, Pnew(0:3, 0:3), (width, height), CV_32FC1): HOST code in double, no handle and no device.
 * K, R, Pnew row major; D = k1 k2 p1 p2 [k3] (num_d = 4 or 5); map_x / map_y hold width * height floats, rows `width` apart.
 *   iR = inverse(Pnew * R) by the cofactor formula (OpenCV: LU - the last bits are unpinned);
 *   row i: _x = i iR[1] + iR[2], _y = i iR[4] + iR[5], _w = i iR[7] + iR[8]; column j: w = 1 / _w, x = _x w, y = _y w, x2 = x x, y2 = y y,
 *   r2 = x2 + y2, _2xy = 2 x y, kr = 1 + ((k3 r2 + k2) r2 + k1) r2, u = fx (x kr + p1 _2xy + p2 (r2 + 2 x2)) + u0,
 *   v = fy (y kr + p1 (r2 + 2 y2) + p2 _2xy) + v0, stored as float; then _x += iR[0], _y += iR[3], _w += iR[6] (incremental, as OpenCV's loop).
 * ORBX_ERR_ARG: a NULL pointer, num_d not 4 or 5, an empty size, Pnew * R singular or not finite. */
int orbx_rectify_maps(const double K[9], const double *D, int num_d, const double R[9], const double Pnew[9], int width, int height,
                      float *map_x, float *map_y);

/* The two CV_32FC1 maps the reference hands to cv::remap, for `side` 0 (left) or 1 (right): uploaded and converted ONCE (k_maps_fixed) to
 * 6 bytes per pixel, ix | iy << 16 and fx | fy << 5.  Rows are map_stride_floats apart.  A value that is not finite is the caller's error:
 * ORBX_ERR_ARG, found in a host pass before anything is uploaded.  Returns when the maps are in place. */
int orbx_image_prep_set_maps(orbx_image_prep *h, int side, const float *map_x, const float *map_y, int map_stride_floats, int width, int height);

/* `batch` frames in DEVICE memory, frame f at src_dev + f * src_pitch, rows src_stride bytes apart, `channels` (1, 3 or 4) interleaved
 * bytes per pixel; rgb_order 1: the first byte is R, 0: B (ignored for one channel).  rectify_side -1: no rectification, 0 / 1: remap
 * through that side's maps, whose size must be width x height.  One channel without rectification is a plain copy into the padded
 * layout.  The work is enqueued on the stream of `consumer` (orbx_extractor_stream_internal, as orbx_frame_finish_device does), so an
 * orbx_extract_batch_device(consumer, <the results below>, ...) that follows is ordered behind it with no wait in between; consumer ==
 * NULL: the handle's own stream.  Nothing is waited for.  Sources whose pointer, stride and pitch are multiples of 4 take the dword
 * path, every other source the byte path - same results. */
int orbx_image_prep_batch_device(orbx_image_prep *h, orbx_extractor *consumer, const void *src_dev, int batch, int width, int height,
                                 int channels, int rgb_order, int src_stride, size_t src_pitch, int rectify_side);
/* The last call's output: frame f at *images_dev + f * *frame_pitch (ORBX_ERR_STATE before the first call). */
int orbx_image_prep_results_device(orbx_image_prep *h, const void **images_dev, int *stride, size_t *frame_pitch);
int orbx_image_prep_sync(orbx_image_prep *h);
/* Host frames (rows `stride` bytes apart) into a handle-owned device source buffer, for callers without a device allocator (tests, the
 * shim), like orbx_upload_frames.  dev_stride 0: rows padded to a multiple of 16 bytes; otherwise the row pitch to use (>= width *
 * channels).  dev_offset (0..15) shifts the whole buffer by that many bytes - a caller's own sources are not always aligned, and this
 * is how the byte path is reached through this entry point.  *src_pitch = *src_stride * height.  Returns when the copy is complete. */
int orbx_image_prep_upload(orbx_image_prep *h, const uint8_t *const *images, int batch, int width, int height, int channels, int stride,
                           int dev_stride, int dev_offset, const void **src_dev, int *src_stride, size_t *src_pitch);
/* Wait for the last batch and copy its first `batch` frames to the host: frame f at out + f * out_stride * height, width bytes per row. */
int orbx_image_prep_download(orbx_image_prep *h, int batch, int width, int height, uint8_t *out, int out_stride);
/* The synchronous form (upload + batch + download): host frames in, host frames out (frame f at out + f * out_stride * height, width bytes per row written). */
int orbx_image_prep_run(orbx_image_prep *h, const uint8_t *const *images, int batch, int width, int height, int channels, int rgb_order,
                        int stride, int rectify_side, uint8_t *out, int out_stride);
/* device time of the last call's kernel (HIP events on the stream it ran on) and its kernel launches */
int orbx_image_prep_last_timing(orbx_image_prep *h, float *device_ms, int *launches);


/* ------------------------------------------------------------------------------------
 * Vocabulary training  ==  DBoW2::TemplatedVocabulary<FORB::TDescriptor,FORB>::create(training_features, k, L, weighting, scoring)
 * (reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-587): HKmeansStep (:641-819), initiateClustersKMpp (:832-913),
 * FORB::meanValue / FORB::distance (FORB.cpp:28-101), createWords (:917-938) and setNodeWeights (:942-996) for 256-bit descriptors, one
 * level of the tree at a time for all its nodes.  Three stated differences:
 *   1. random draws: the reference consumes rand() lazily in depth-first order; here draw(seed, slot, j) is the top 53 bits r of
 *      splitmix64's output function chained over the caller's seed, the heap index of the node being split in the complete k-ary tree
 *      (root 0, child c of slot s is s * k + c + 1) and the draw number j inside the node.  The first centre of a node with n features is
 *      min(n - 1, floor((r * 2^-53) * n)); centre j >= 1 uses cut_d = ((r + 1) * 2^-53) * dist_sum;
 *   2. a cluster that receives no feature in an assignment pass keeps its previous centre (the reference reads a released cv::Mat there);
 *      its child node is still created, a word with Ni = 0 and weight 0;
 *   3. max_iterations (>= 2) caps the assignment passes per node (the reference has none); the summary counts the nodes that hit it.
 * Everything else is literal: stable feature order inside a node, min_dists against the last centre only, the first feature whose
 * running sum reaches cut_d, D(x) not D(x)^2, dist_sum == 0 ends the seeding early, one cluster per feature where n <= k, strict '<' in
 * the assignment, the mean's tie sets the bit, recursion only below level L into children with more than one feature, node ids in the
 * reference's depth-first order, word ids by node id, Ni from the real descent, log() from the host's libm on device-counted Ni.
 * ---------------------------------------------------------------------------------- */
#define ORBX_VOC_MAX_K 32
#define ORBX_VOC_MAX_L 10
typedef struct orbx_voc_trainer orbx_voc_trainer;
typedef struct orbx_voc_train_params {
    uint64_t seed;
    int weighting;        /* DBoW2::WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
    int max_iterations;   /* >= 2 */
} orbx_voc_train_params;
typedef struct orbx_voc_train_summary {
    int num_nodes, num_words;
    int unconverged_nodes;                       /* nodes whose association still changed in pass max_iterations */
    int passes_per_level[ORBX_VOC_MAX_L];        /* assignment passes run for level l + 1 (the most any of its nodes needed; 0: no node with n > k) */
} orbx_voc_train_summary;
/* ORBX_ERR_ARG, before a device is looked for: k outside 2..ORBX_VOC_MAX_K, L outside 1..ORBX_VOC_MAX_L, a complete tree of 2^31 nodes
 * or more, max_descriptors outside 1..2^26, max_images < 1; then ORBX_ERR_NODEVICE without a device. */
int orbx_voc_trainer_create(int device, int k, int L, int max_descriptors, int max_images, orbx_voc_trainer **out);
void orbx_voc_trainer_destroy(orbx_voc_trainer *h);
/* Appends num_images images from host arrays: counts[i] descriptors of 32 bytes each, image after image.  ORBX_ERR_CAPACITY (nothing
 * appended) beyond max_descriptors / max_images. */
int orbx_voc_trainer_add(orbx_voc_trainer *h, const uint8_t *descriptors, const int32_t *counts, int num_images);
/* Appends every frame of the extractor's last batch as one image each: the descriptors are read where the extractor left them on the
 * device, on its stream; nothing is downloaded and nothing is waited for.  ORBX_ERR_STATE where the extractor's "last batch" views are
 * (e.g. after a chunked host batch).  A batch that does not fit is dropped whole; the next call that reads the trainer's size
 * (_add, _size, orbx_voc_train) reports it once as ORBX_ERR_CAPACITY. */
int orbx_voc_trainer_add_extracted(orbx_voc_trainer *h, orbx_extractor *ext);
int orbx_voc_trainer_clear(orbx_voc_trainer *h);
int orbx_voc_trainer_size(orbx_voc_trainer *h, int *descriptors, int *images);
/* Trains on everything added.  ORBX_ERR_ARG: weighting outside 0..3, max_iterations < 2; ORBX_ERR_STATE: no descriptors.  Synchronous. */
int orbx_voc_train(orbx_voc_trainer *h, const orbx_voc_train_params *params, orbx_voc_train_summary *summary);
/* The trained tree as flat arrays in the layout of orbx_vocabulary_create (any pointer may be NULL), plus ni per node: the number of
 * training images with a feature on that word, 0 on inner nodes.  ORBX_ERR_STATE before a training, ORBX_ERR_CAPACITY when
 * capacity_nodes < summary.num_nodes. */
int orbx_voc_trainer_result(orbx_voc_trainer *h, int32_t *parent, uint8_t *is_leaf, uint8_t *descriptors, double *weights, int32_t *ni, int capacity_nodes);
/* The device vocabulary of the last training (the caller destroys it). */
int orbx_voc_trainer_vocabulary(orbx_voc_trainer *h, orbx_vocabulary **voc);
/* Host time of the last training and of each level (level_ms[ORBX_VOC_MAX_L]), its kernel launches, and - when the training ran with
 * profiling enabled - the device time of its stages from HIP events: stage_ms[5] = seeding, assignment, mean, partition, everything else. */
int orbx_voc_trainer_set_profiling(orbx_voc_trainer *h, int enable);
int orbx_voc_trainer_last_timing(orbx_voc_trainer *h, float *total_ms, float *level_ms, float *stage_ms, int *launches);
/* The two stages on explicit inputs (n <= max_descriptors descriptors in host memory; segment s = features seg_offsets[s] ..
 * seg_offsets[s + 1] - 1, offsets from 0 to n, no empty segment).
 * Seeding: slots[s] keys the draws of segment s.  chosen[s * k + j] = index inside the segment of the j-th centre, -1 where the seeding
 * ended early; a segment with n <= k features reports 0 .. n - 1. */
int orbx_voc_seed_segments(orbx_voc_trainer *h, const uint8_t *descriptors, int n, const int32_t *seg_offsets, const uint64_t *slots, int num_segments,
                           uint64_t seed, int32_t *chosen);
/* One Lloyd pass: centres[(s * k + c) * 32] for c < num_centres[s] (1..k).  With prev_assoc (cluster per feature, inside its segment's
 * centres) the centres are first replaced by the means of its groups (an empty group keeps its centre); then every feature is assigned.
 * changed_out[s] = 1 when an association of segment s differs from prev_assoc (0 without one).  Outputs may be NULL. */
int orbx_voc_lloyd_pass(orbx_voc_trainer *h, const uint8_t *descriptors, int n, const int32_t *seg_offsets, int num_segments, const uint8_t *centres,
                        const int32_t *num_centres, const int32_t *prev_assoc, uint8_t *centres_out, int32_t *assoc_out, uint8_t *changed_out);


#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */

/*
 * orbx.h — C ABI of the MI355X-native ORB front end + Hamming matchers (liborbx.so).
 *
 * Drop-in boundary for the ORB-SLAM2 hot path.  The reference has no
 * FFI; the seam is two C++ classes and one Frame method, so each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  INTEGRATION.md shows
 * the C++ adaptor a maintainer adds on the reference side (ORBextractor/ORBmatcher shims).
 *
 * Conventions: plain C, no exceptions; every function returns ORBX_OK (0) or a negative
 * ORBX_E_* code and records a message readable through orbx_last_error() (thread-local).
 * All buffers are caller-allocated with explicit capacities.  "host" entry points take host
 * pointers and synchronise; "*_device" entry points take device (HBM) pointers, enqueue on a
 * HIP stream and return without synchronising (the throughput path).
 * There is no CPU fallback: without a usable gfx950 device every compute call fails with
 * ORBX_E_NO_DEVICE.
 *
 * Threading (as the reference): one extractor handle is used by one thread
 * at a time; distinct handles may be used concurrently.
 *
 * Streams: a handle remembers the stream of its most recent "*_device" launches.  Whenever a call
 * has to rebuild the per-image-size tables (first call / a new image size) or to grow a workspace,
 * it first waits for that stream and for the handle's own stream, so tables and buffers are never
 * rewritten or freed under running kernels.  A call that launches on a DIFFERENT stream than the
 * previous one on the same handle is ordered behind the earlier work by an event (the handle's
 * pyramid and candidate workspaces are shared by all its launches), without a host synchronisation.
 * A caller stream must therefore stay valid until the handle has been used with another stream or
 * destroyed.  Steady state (same size, same batch, same stream) neither synchronises nor records events.  A kernel-side error (ORBX_E_CAPACITY from orbx_sync) belongs to the work
 * that orbx_sync has just waited for; the flag is cleared when it is reported.
 */
#ifndef ORBX_H
#define ORBX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_OK 0
#define ORBX_E_INVALID (-1)    /* bad argument */
#define ORBX_E_CAPACITY (-2)   /* an output capacity is too small */
#define ORBX_E_TOO_SMALL (-3)  /* image smaller than one 30-px FAST cell at some level (reference: div by 0) */
#define ORBX_E_NO_DEVICE (-4)  /* no gfx950 device / device index out of range */
#define ORBX_E_HIP (-5)        /* a HIP runtime call failed */

/* == cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id.
 * Output element type of ORBextractor::operator() (include/ORBextractor.h:74-76). */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbx_keypoint;

typedef struct orbx_extractor orbx_extractor; /* opaque; owns device pyramid + workspace */

const char *orbx_last_error(void);
int orbx_device_count(void);
/* "<pci bus id> <uuid hex> <gcn arch>" of one visible device: an N-process launch (one process per GPU) reports it
 * per rank so that the line shows every rank held its own card.  No reference counterpart (the reference is single-process CPU). */
int orbx_device_identity(int device, char *buf, int cap);

/* ---- ORBextractor (include/ORBextractor.h:58-139, src/ORBextractor.cc:429-534) ---------- */

/* replaces `new ORBextractor(nFeatures, fScaleFactor, nLevels, fIniThFAST, fMinThFAST)`
 * (src/Tracking.cc:124-130).  device = HIP device index; max_w/max_h/max_batch size the
 * workspace (images of any size <= max and batches <= max_batch are accepted later). */
int orbx_extractor_create(orbx_extractor **out, int nfeatures, float scale_factor, int nlevels,
                          int ini_th_fast, int min_th_fast, int device, int max_w, int max_h, int max_batch);
void orbx_extractor_destroy(orbx_extractor *e);

/* Which 7-tap table cv::GaussianBlur(7x7, sigma 2) (src/ORBextractor.cc:1311) is computed with.  OpenCV's 8-bit Gaussian has had two
 * fixed-point kernels over the releases the reference builds against ("OpenCV 2.4.3 or later, tested with 2.4.11 and 3.2", README.md:68):
 *   ORBX_CV_TAPS_257: every tap rounded by itself, cvRound(k * 256): 18 34 49 55 49 34 18 (sum 257)  -- default;
 *   ORBX_CV_TAPS_256: rounding error diffused so that the taps sum to exactly 256: 18 34 48 56 48 34 18.
 * Different taps give different blurred pixels and so different rBRIEF bits; the arithmetic around the taps (exact integer row pass,
 * (sum + 2^15) >> 16 column pass) is the same for both.  WHICH OpenCV RELEASE USES WHICH TABLE IS PARITY UNPINNED: the reference holds no
 * fixture and OpenCV is not installed here.  From memory: 3.2 (the tested version) has the 257 table; the fixed-point path that came with
 * 3.4.2 may still round tap by tap, the error-diffused table arrived with a later 3.4.x / 4.x release.  A deployment decides by comparing one
 * blurred image against its own OpenCV.  The *_PROFILE_* names are the older spelling of the same two values.
 * Call right after orbx_extractor_create; it applies to all later extractions. */
#define ORBX_CV_TAPS_257 0
#define ORBX_CV_TAPS_256 1
#define ORBX_CV_PROFILE_3_2 ORBX_CV_TAPS_257
#define ORBX_CV_PROFILE_3_4_2 ORBX_CV_TAPS_256
int orbx_extractor_set_cv_profile(orbx_extractor *e, int profile);
int orbx_gaussian_taps(int profile, int taps[7]);
/* inspection: the constant operand of the descriptor kernel's matrix-core row pass for a tap profile.  The row pass is the banded product
 * R[43 x 37] = Raw[43 x 43] . G, G[k][c] = taps[k - c] for 0 <= k - c <= 6; `out` (3 * 64 * 16 bytes) receives G cut into three column
 * tiles of 16 in the lane layout of the 16x16x64 int8 matrix instruction: byte j of lane l of tile t is G[16 (l / 16) + j][16 t + l % 16],
 * zero for k >= 43 and c >= 37.  *acc0 = 128 * sum(taps), where the accumulators start: the kernel multiplies pixel - 128. */
int orbx_desc_rowpass_matrix(int profile, uint8_t *out, int *acc0);

/* Tuning, no effect on results: extractions of at most `max_images` images per launch build the pyramid (ComputePyramid,
 * src/ORBextractor.cc:1347-1370) with two launches that each produce several levels (a single frame's time is its chain of dependent
 * launches); launches of up to 24 images still take the small levels (3 and up) in one launch; larger batches keep one launch per
 * level, which moves fewer bytes.  Default 8; 0 = always one launch per level. */
int orbx_extractor_set_pyramid_group_limit(orbx_extractor *e, int max_images);

/* getters: GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors /
 * GetScaleSigmaSquares / GetInverseScaleSigmaSquares (include/ORBextractor.h:78-98).
 * Each output array has nlevels entries; NULL pointers are skipped. */
int orbx_get_levels(const orbx_extractor *e);
float orbx_get_scale_factor(const orbx_extractor *e);
int orbx_get_scale_tables(const orbx_extractor *e, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2);
/* per-level feature quotas mnFeaturesPerLevel (src/ORBextractor.cc:468-493) */
int orbx_get_features_per_level(const orbx_extractor *e, int *quota);
/* smallest per-image keypoint capacity that can never overflow (quadtree may return up to
 * max(quota+2, 4*nIni) per level) */
int orbx_max_keypoints(const orbx_extractor *e, int w, int h);

/* replaces ORBextractor::operator()(image, mask, keypoints, descriptors)
 * (src/ORBextractor.cc:1261-1339; caller src/Frame.cc:285-292).  img: 8-bit grey, row stride in
 * bytes.  kps[cap], desc[cap*32].  An empty image (w==0||h==0) returns ORBX_OK with *n_out = 0
 * (reference :1264-1265 returns silently). */
int orbx_extract(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride,
                 orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out);

/* Same for a colour frame: the cvtColor(CV_RGB2GRAY | CV_BGR2GRAY | CV_RGBA2GRAY | CV_BGRA2GRAY) that
 * Tracking::GrabImageStereo/RGBD/Monocular apply first (src/Tracking.cc:177-202,:217-231,:254-268) runs on device into the
 * level-0 staging (first half).  channels 3 or 4; rgb_order 1 = R first (mbRGB), 0 = B first.
 * gray_out (optional, may be NULL; stride gray_stride) receives the grey image, i.e. what mImGray holds afterwards. */
int orbx_extract_color(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int channels, int rgb_order,
                       orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, uint8_t *gray_out, size_t gray_stride);

/* ---- RGB-D frames (Frame::Frame(imGray, imDepth, ...), src/Frame.cc:127-180) -------------------------
 * After ExtractORB (:146) the RGB-D constructor runs UndistortKeyPoints (:152) and ComputeStereoFromRGBD (:154, :754-774): per
 * keypoint i, with kp its extractor position (level-0 coordinates, distorted) and kpU = its undistorted position,
 *     d = imDepth.at<float>((int)kp.y, (int)kp.x)       -- the lookup uses the DISTORTED position, truncated (:764-767)
 *     d > 0:  mvDepth[i] = d, mvuRight[i] = kpU.x - mbf / d  (fp32, correctly rounded division);  else both -1.
 * imDepth is what Tracking::GrabImageRGBD (src/Tracking.cc:232-233) leaves: CV_16U depth is always converted to float as
 * d = (float)raw * depth_scale (one fp32 multiply); CV_32F depth is multiplied only when fabs(depth_scale - 1.0f) > 1e-5, else used as it is.
 * kpU is the arithmetic of orbx_undistort_keypoints, bit for bit; dist_coef[0] == 0 leaves it kp (src/Frame.cc:472-476).
 * Defined deviation: a keypoint whose truncated position lies outside the depth image gets -1 / -1 (the reference reads outside
 * the matrix; extraction never produces such a point, but orbx_rgbd_depth_batch_device accepts caller-supplied keypoints). */
#define ORBX_DEPTH_U16 0   /* CV_16U (the TUM PNG depth maps) */
#define ORBX_DEPTH_F32 1   /* CV_32F */
typedef struct {
    int depth_type;            /* ORBX_DEPTH_* */
    float depth_scale;         /* Tracking::mDepthMapFactor after src/Tracking.cc:147-151: 1.0f/DepthMapFactor, or 1 when |DepthMapFactor| < 1e-5 */
    float bf;                  /* mbf */
    float fx, fy, cx, cy;      /* mK */
    float dist_coef[5]; int ndist;   /* mDistCoef (k1 k2 p1 p2 [k3]), ndist 4 or 5; dist_coef[0] == 0: no undistortion */
} orbx_rgbd_params;

/* One RGB-D frame in one call (host pointers): the image preparation of Tracking::GrabImageRGBD (src/Tracking.cc:217-233: cvtColor,
 * depth convertTo) and lines :145-154 of the RGB-D constructor.  img: channels 1 (grey), 3 or 4 (colour through the cvtColor of
 * orbx_extract_color; rgb_order 1 = mbRGB); depth: h rows of w uint16 (ORBX_DEPTH_U16) or float (ORBX_DEPTH_F32) at depth_stride
 * bytes (at least a row, a multiple of the element size).  kps[cap] / desc[cap*32] / *n_out as orbx_extract; xy_un[cap][2]
 * (optional, may be NULL) = mvKeysUn positions, u_right[cap] = mvuRight, depth_out[cap] = mvDepth.  The depth is uploaded with the image
 * and everything comes back in one group of copies behind one synchronisation.  ORBX_E_INVALID: NULL / inconsistent arguments, unknown
 * depth_type, ndist not 4 or 5, bad depth_stride; ORBX_E_CAPACITY: cap < orbx_max_keypoints. */
int orbx_extract_rgbd(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int channels, int rgb_order,
                      const void *depth, size_t depth_stride, const orbx_rgbd_params *p,
                      orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                      float *xy_un, float *u_right, float *depth_out);
/* Pipelined form (the frame loop of Examples/RGB-D/rgbd_tum.cc:77-119): the third mode of the pipelined forms below.  RGB-D tickets share
 * the handle's slots and submission order with mono and stereo tickets; a ticket must be waited for through the form it was submitted
 * with.  The depth travels with the frame: gathered by the depth kernel straight from pinned host memory (default: only the values at the
 * keypoints cross PCIe) or, with ORBX_PIPE_RGBD_GATHER=0 in the environment when the handle is created, uploaded whole into the slot.  img and
 * depth lying in orbx_pinned_alloc memory with stride == row bytes are read in place (untouched until _wait returns); other input is
 * staged inside _submit.  The first RGB-D submit of a size makes and touches what the RGB-D mode adds to every slot and lane.  e must have
 * been created with max_batch >= 2 (as the other pipelined forms). */
int orbx_extract_rgbd_submit(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int channels, int rgb_order,
                             const void *depth, size_t depth_stride, const orbx_rgbd_params *p, int *ticket);
int orbx_extract_rgbd_wait(orbx_extractor *e, int ticket, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                           float *xy_un, float *u_right, float *depth_out);
/* Batched, device-resident (after orbx_extract_batch_device): image b has keypoints d_kps + b*cap (orbx_keypoint records), count d_n[b]
 * (int32, read on the device) and depth d_depth + b*depth_img_stride with row pitch depth_pitch bytes (w x h elements of p->depth_type).
 * Outputs are [batch*cap] rows in the layout of orbx_stereo_match_batch_device: d_u_right / d_depth_out floats, d_xy_un (may be NULL)
 * float pairs; a row goes straight into orbx_frame_create_from_extraction(..., d_u_right = row, K, dist_coef, ...).  Entries at or beyond
 * an image's count are left untouched.  Asynchronous on `stream` (a hipStream_t; NULL = the null stream). */
int orbx_rgbd_depth_batch_device(int device, const void *d_kps, const void *d_n, int cap, int batch,
                                 const void *d_depth, size_t depth_img_stride, size_t depth_pitch, int w, int h,
                                 const orbx_rgbd_params *p, void *d_xy_un, void *d_u_right, void *d_depth_out, void *stream);

/* ---- stereo rectification (second half) ----------------------------------
 * cv::remap(imLeft, imLeftRect, M1l, M2l, cv::INTER_LINEAR) of Examples/Stereo/stereo_euroc.cc:136-137 (8-bit grey,
 * BORDER_CONSTANT 0).  map_x / map_y = the CV_32FC1 pair cv::initUndistortRectifyMap returns (:103-104), dst_h x dst_w
 * floats each, dense; converted once to OpenCV's fixed-point form on the device. */
typedef struct orbx_rectifier orbx_rectifier;
int orbx_rectifier_create(int device, int src_w, int src_h, int dst_w, int dst_h, const float *map_x, const float *map_y,
                          orbx_rectifier **out);
void orbx_rectifier_destroy(orbx_rectifier *r);
int orbx_rectifier_size(const orbx_rectifier *r, int *dst_w, int *dst_h);
/* batch of device images -> rectified device images (d_dst, dst_pitch and dst_stride multiples of 4); asynchronous on `stream` */
int orbx_remap_batch_device(const orbx_rectifier *r, const void *d_src, size_t src_stride, size_t src_pitch, int batch,
                            void *d_dst, size_t dst_stride, size_t dst_pitch, void *stream);
/* raw grey frame (host) -> rectify on device -> extract; rect_out (optional) receives the rectified image */
int orbx_extract_rectified(orbx_extractor *e, const orbx_rectifier *r, const uint8_t *img, int w, int h, size_t stride,
                           orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out, uint8_t *rect_out, size_t rect_stride);

/* One stereo frame in one call (host pointers): both ORBextractor::operator() calls of Frame::Frame(imLeft, imRight, ...)
 * (src/Frame.cc:82-85, two threads in the reference) and Frame::ComputeStereoMatches (:97, :577-751).  e must have been
 * created with max_batch >= 2.  kps[2*cap] / desc[2*cap*32]: left eye at index 0, right eye at index cap; n_out[2];
 * u_right[cap], depth[cap] = mvuRight, mvDepth of the left keypoints.  bf = mbf, min_z = mb (see orbx_stereo_match). */
int orbx_extract_stereo(orbx_extractor *e, const uint8_t *img_left, const uint8_t *img_right, int w, int h, size_t stride,
                        float bf, float min_z, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                        float *u_right, float *depth);

/* Pipelined form of orbx_extract_stereo for a camera stream fed from host memory: _submit enqueues one stereo frame
 * (upload on a copy stream, both extractions + ComputeStereoMatches on the compute stream, download on a second copy
 * stream) and returns a ticket without waiting; _wait blocks until that frame's results are on the host and copies them
 * out (same output contract as orbx_extract_stereo).  Up to orbx_pipeline_depth() frames may be in flight per handle:
 * frame i+1 uploads and frame i-1 downloads while frame i computes.  Tickets must be waited for in submission order;
 * a submit with all slots in flight fails with ORBX_E_INVALID.  If img_left / img_right lie in memory obtained from
 * orbx_pinned_alloc and stride == w, the upload reads them in place (they must stay untouched until _wait returns);
 * otherwise they are copied to the handle's pinned staging inside _submit and may be reused at once.
 * Replaces the per-frame sequence of Frame::Frame(imLeft, imRight, ...) (src/Frame.cc:82-97) in the frame loop of
 * Examples/Stereo/stereo_kitti.cc:68-117. */
int orbx_pipeline_depth(void);
/* Makes and touches every pipeline slot and kernel lane of the pipelined forms for images of w x h by running one scratch frame through each
 * (tens of milliseconds, once).  orbx_extract_stereo_submit does this by itself on the first frame of a size; a camera loop that wants that
 * first frame on time as well (Examples/Stereo/stereo_kitti.cc:83-117 times every frame) calls it before the loop. */
int orbx_pipeline_warm(orbx_extractor *e, int w, int h);
int orbx_extract_stereo_submit(orbx_extractor *e, const uint8_t *img_left, const uint8_t *img_right, int w, int h, size_t stride,
                               float bf, float min_z, int *ticket);
int orbx_extract_stereo_wait(orbx_extractor *e, int ticket, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out,
                             float *u_right, float *depth);
/* the same pipeline for a monocular stream (Frame::Frame(imGray, ...), src/Frame.cc:176-215; frame loop of
 * Examples/Monocular/mono_tum.cc): one extraction per ticket, same output contract as orbx_extract.  Mono and stereo
 * tickets share the handle's slots and ordering. */
int orbx_extract_submit(orbx_extractor *e, const uint8_t *img, int w, int h, size_t stride, int *ticket);
int orbx_extract_wait(orbx_extractor *e, int ticket, orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out);
/* page-locked host memory for frame buffers (uploads from it need no staging copy) */
void *orbx_pinned_alloc(size_t bytes);
void orbx_pinned_free(void *p);

/* B images of one size in one pass (host pointers). kps[B*cap], desc[B*cap*32], n_out[B]. */
int orbx_extract_batch(orbx_extractor *e, const uint8_t *const *imgs, int batch, int w, int h, size_t stride,
                       orbx_keypoint *kps, uint8_t *desc, int cap, int *n_out);

/* Throughput path: images already resident in HBM.  Image b starts at d_imgs + b*img_stride and
 * has row pitch `pitch` bytes; outputs are device buffers d_kps[B*cap], d_desc[B*cap*32],
 * d_n_out[B].  Enqueued on `stream` (a hipStream_t; NULL = the handle's own stream); returns
 * before completion.  The input must stay valid until orbx_stereo_match*_device /
 * orbx_pyramid_level calls that read level 0 have completed (level 0 is read in place). */
int orbx_extract_batch_device(orbx_extractor *e, const void *d_imgs, size_t img_stride, size_t pitch,
                              int batch, int w, int h, void *d_kps, void *d_desc, int cap, void *d_n_out,
                              void *stream);
/* wait for everything enqueued on the handle's stream (or `stream`) */
int orbx_sync(orbx_extractor *e, void *stream);

/* backs the public member mvImagePyramid (include/ORBextractor.h:100): copy level `level` of
 * image `image_index` of the most recent extract call to host memory (no 19-px border: the
 * border is never read by the hot path). */
int orbx_pyramid_level(orbx_extractor *e, int image_index, int level, uint8_t *dst, size_t dst_stride, int *w, int *h);

/* ---- Frame::ComputeStereoMatches (src/Frame.cc:577-751) ---------------------------------- */

/* L and R have each run extract on the left/right image (their pyramids are read).
 * min_z replaces the `mb` member the reference reads uninitialised; maxD = bf/min_z.
 * u_right[nL], depth[nL]: -1 where unmatched (mvuRight / mvDepth). */
int orbx_stereo_match(orbx_extractor *L, orbx_extractor *R,
                      const orbx_keypoint *kL, const uint8_t *dL, int nL,
                      const orbx_keypoint *kR, const uint8_t *dR, int nR,
                      float bf, float min_z, float *u_right, float *depth);

/* Batched, device-resident: pair p uses image (imgL0+p) of handle L and (imgR0+p) of handle R
 * from their most recent extract_batch calls (L and R may be the same handle).  Keypoints /
 * descriptors / counts are the device outputs of orbx_extract_batch_device with capacity `cap`.
 * d_u_right, d_depth: [batch*cap] floats.
 * `row_table` states where the row table of src/Frame.cc:584-604 comes from -- never guessed from addresses:
 *   ORBX_ROWTAB_FROM_KEYPOINTS  built from the right keypoints handed in (d_kR, d_nR), whatever they are: always correct;
 *   ORBX_ROWTAB_OF_EXTRACTION   the by-product table R's most recent orbx_extract_batch_device left behind (one launch less).
 *                               The caller thereby asserts that d_kR still holds exactly what that extraction wrote; the call is
 *                               refused with ORBX_E_INVALID when d_kR / cap / the image range are not the ones of that extraction,
 *                               or when that extraction built no table (images taller than 600 rows). */
#define ORBX_ROWTAB_FROM_KEYPOINTS 0
#define ORBX_ROWTAB_OF_EXTRACTION 1
int orbx_stereo_match_batch_device(orbx_extractor *L, int imgL0, orbx_extractor *R, int imgR0, int batch,
                                   const void *d_kL, const void *d_dL, const void *d_nL,
                                   const void *d_kR, const void *d_dR, const void *d_nR, int cap,
                                   float bf, float min_z, void *d_u_right, void *d_depth, int row_table, void *stream);
/* 1 when R's most recent extraction left a row table behind that ORBX_ROWTAB_OF_EXTRACTION could use for (d_kR, imgR0, batch, cap) */
int orbx_stereo_row_table_available(const orbx_extractor *R, const void *d_kR, int imgR0, int batch, int cap);

/* ---- ORBmatcher (include/ORBmatcher.h:41-83) ---------------------------------------------- */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1733-1749), host inline popcount */
int orbx_hamming(const uint8_t *a, const uint8_t *b);

/* One side of a BoW search: descriptors + DBoW2::FeatureVector flattened to CSR
 * (Thirdparty/DBoW2/DBoW2/FeatureVector.h:21-22: node ids ascending, feature indices ascending
 * within a node, every feature in at most one node) + per-feature attributes.  Host pointers. */
typedef struct {
    int n;                   /* number of features */
    const uint8_t *desc;     /* [n][32] */
    int nnodes;
    const uint32_t *node_id; /* [nnodes] */
    const int32_t *node_off; /* [nnodes+1] */
    const uint32_t *feat;    /* [node_off[nnodes]] */
    const uint8_t *flag;     /* [n] per-search meaning, see below */
    const float *angle;      /* [n] keypoint angle, degrees */
    const float *x, *y;      /* [n] undistorted position (triangulation only, else may be NULL) */
    const int32_t *octave;   /* [n] (triangulation only) */
    const float *u_right;    /* [n] (triangulation only): <0 = monocular feature */
} orbx_featset;

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:171-303).
 * kf->flag[i] != 0 <=> KF feature i holds a non-bad MapPoint; f->flag unused.
 * match_f[f->n] = matched KF feature index or -1; *nmatches = return value of the reference. */
int orbx_search_by_bow_kf_f(int device, const orbx_featset *kf, const orbx_featset *f,
                            float nnratio, int check_orientation, int32_t *match_f, int *nmatches);
/* many keyframes against one frame in one launch (Tracking::Relocalization loop,
 * src/Tracking.cc:1661-1682): match_f[nkf][f->n], nmatches[nkf] */
int orbx_search_by_bow_kf_f_batch(int device, const orbx_featset *kfs, int nkf, const orbx_featset *f,
                                  float nnratio, int check_orientation, int32_t *match_f, int *nmatches);

/* Device-resident keyframe set for the relocalisation / place-recognition loops
 * (src/Tracking.cc:1661-1682 calls SearchByBoW once per candidate keyframe): the keyframes'
 * descriptors, CSR feature vectors, flags and angles are uploaded once; each search uploads only
 * the frame side.  match_f[nkf][f->n], nmatches[nkf] as in orbx_search_by_bow_kf_f_batch. */
typedef struct orbx_bowdb orbx_bowdb;
int orbx_bowdb_create(int device, const orbx_featset *kfs, int nkf, orbx_bowdb **out);
int orbx_bowdb_search(orbx_bowdb *db, const orbx_featset *f, float nnratio, int check_orientation,
                      int32_t *match_f, int *nmatches);
int orbx_bowdb_size(const orbx_bowdb *db);
void orbx_bowdb_destroy(orbx_bowdb *db);

/* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (src/ORBmatcher.cc:568-702).
 * flag != 0 <=> non-bad MapPoint (both sides).  match12[k1->n] = KF2 feature index or -1. */
int orbx_search_by_bow_kf_kf(int device, const orbx_featset *k1, const orbx_featset *k2,
                             float nnratio, int check_orientation, int32_t *match12, int *nmatches);

/* ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:704-871) incl. CheckDistEpipolarLine
 * (:147-164).  flag != 0 <=> the feature already has a MapPoint (skipped).  F12 row-major 3x3;
 * (ex,ey) = epipole of camera 1 in image 2 (:712-718, computed by the adaptor);
 * scale_factors2 / level_sigma2_2: KF2's per-level tables [nlevels2].
 * pairs[2*cap] receives (idx1, idx2) sorted by idx1; *npairs = number found (may exceed cap:
 * then ORBX_E_CAPACITY). */
int orbx_search_for_triangulation(int device, const orbx_featset *k1, const orbx_featset *k2,
                                  const float F12[9], float ex, float ey,
                                  const float *scale_factors2, const float *level_sigma2_2, int nlevels2,
                                  int only_stereo, int check_orientation, int32_t *pairs, int cap, int *npairs);

/* The loops the reference runs these searches in, as ONE call (one launch, one PCIe round trip):
 * LoopClosing::ComputeSim3 calls SearchByBoW(mpCurrentKF, pKF, ...) per loop candidate (src/LoopClosing.cc:293-323):
 * k1 against k2s[0..n2): match12[n2][k1->n], nmatches[n2]. */
int orbx_search_by_bow_kf_kf_batch(int device, const orbx_featset *k1, const orbx_featset *k2s, int n2,
                                   float nnratio, int check_orientation, int32_t *match12, int *nmatches);
/* LocalMapping::CreateNewMapPoints calls SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, ...) per neighbour keyframe
 * (src/LocalMapping.cc:241-309): k1 against k2s[0..n2), each with its own F12s[i][9] and epipole epipoles[i][2]; one set of
 * per-level tables (all keyframes of a map share one extractor).  pairs[n2][2*cap], npairs[n2]; ORBX_E_CAPACITY if any
 * list is longer than cap (the first cap entries of each are written). */
int orbx_search_for_triangulation_batch(int device, const orbx_featset *k1, const orbx_featset *k2s, int n2,
                                        const float *F12s, const float *epipoles,
                                        const float *scale_factors2, const float *level_sigma2_2, int nlevels2,
                                        int only_stereo, int check_orientation, int32_t *pairs, int cap, int *npairs);

/* ---- resident keyframes --------------------------------------------------------------------------
 * A keyframe's descriptors (KeyFrame::mDescriptors), FeatureVector (mFeatVec) and keypoint attributes (mvKeysUn, mvuRight)
 * never change once the keyframe exists (src/KeyFrame.cc:29-60); what changes is which features hold map points.  orbx_kf
 * keeps the immutable part in HBM in FeatureVector order (made once per keyframe, e.g. from the KeyFrame constructor; a
 * Frame can be uploaded the same way for the per-frame searches); the searches below then take the map-point flags per
 * call and move only those, the node intersection and the results over PCIe.  fs->flag is ignored by orbx_kf_create;
 * x / y / octave / u_right may be NULL for a set that is only used in SearchByBoW.
 * flag arrays are per FEATURE ([n] of that keyframe), with the meaning of the host-pointer call they mirror. */
typedef struct orbx_kf orbx_kf;
int orbx_kf_create(int device, const orbx_featset *fs, orbx_kf **out);
void orbx_kf_destroy(orbx_kf *k);
int orbx_kf_size(const orbx_kf *k);
/* Every per-call search keeps a small per-THREAD context per device: a stream plus pinned and device staging.  There are four families:
 * the per-call matchers (SearchByBoW, SearchForTriangulation and their orbx_kf_ forms), the legacy SearchByBoW kernels (a forced form or
 * an oversized node) with orbx_distinctive_descriptors, the projection searches with the orbx_frame_ calls, and
 * orbx_undistort_keypoints.  All of them are given back when the thread ends; a long-lived thread that is done searching (or a pool
 * worker between jobs) may give them back now.  The next call of the thread sets up what it needs again. */
void orbx_thread_release(void);
/* SearchByBoW(pKF, F): kf_flag as orbx_search_by_bow_kf_f's kf->flag; match_f[f's n] */
int orbx_kf_search_by_bow_kf_f(const orbx_kf *kf, const uint8_t *kf_flag, const orbx_kf *f,
                               float nnratio, int check_orientation, int32_t *match_f, int *nmatches);
/* Tracking::Relocalization's loop (src/Tracking.cc:1661-1682): SearchByBoW(pKF, mCurrentFrame) for nkf candidate RESIDENT keyframes against one
 * frame as ONE call; the frame lives one frame time and is given as host pointers (f->flag is not read): match_f[nkf][f->n], nmatches[nkf] */
int orbx_kf_search_by_bow_kfs_f(const orbx_kf *const *kfs, const uint8_t *const *kf_flags, int nkf, const orbx_featset *f,
                                float nnratio, int check_orientation, int32_t *match_f, int *nmatches);
/* SearchByBoW(pKF1, pKF2) for n2 candidates: match12[n2][k1's n], nmatches[n2] */
int orbx_kf_search_by_bow_kf_kf(const orbx_kf *k1, const uint8_t *flag1, const orbx_kf *const *k2s, const uint8_t *const *flags2, int n2,
                                float nnratio, int check_orientation, int32_t *match12, int *nmatches);
/* SearchForTriangulation for n2 neighbours; flag1 / flags2 (or flags2[i]) may be NULL = no feature has a map point */
int orbx_kf_search_for_triangulation(const orbx_kf *k1, const uint8_t *flag1, const orbx_kf *const *k2s, const uint8_t *const *flags2, int n2,
                                     const float *F12s, const float *epipoles,
                                     const float *scale_factors2, const float *level_sigma2_2, int nlevels2,
                                     int only_stereo, int check_orientation, int32_t *pairs, int cap, int *npairs);

/* ---- Frame::ComputeBoW (src/Frame.cc:459-466) --------------------------- */

/* DBoW2 vocabulary tree resident in HBM.  Arrays describe nodes 1..N in id order exactly as
 * TemplatedVocabulary::loadFromTextFile builds them (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:
 * 1358-1445): parent id (0 = root), leaf flag, 32-byte descriptor, weight; children are attached
 * to their parent in id order and word ids are given to leaves in id order.  k <= 20, L <= 10 as
 * in the reference loader.  Only TF_IDF weighting with L1_NORM scoring (ORBvoc.txt) is supported.
 * The leaf flag must say what the tree says (isLeaf() is children.empty(), :328): a childless node
 * without the flag, or a flagged node with children, is ORBX_E_INVALID here and in orbx_vocab_load_text. */
typedef struct orbx_vocab orbx_vocab;
int orbx_vocab_create(int device, int k, int L, int nnodes_minus_root, const int32_t *parent, const uint8_t *is_leaf,
                      const uint8_t *desc, const double *weight, orbx_vocab **out);
/* reads the ORBvoc.txt text format: header "k L scoring weighting", then one line per node
 * "parent isLeaf d0 .. d31 weight" */
int orbx_vocab_load_text(int device, const char *path, orbx_vocab **out);
int orbx_vocab_info(const orbx_vocab *v, int *k, int *L, int *nnodes, int *nwords);
void orbx_vocab_destroy(orbx_vocab *v);

/* TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) (:1127-1194, :1218-1259).
 * desc[n][32] (n <= 8192).  Per-feature outputs (may be NULL): word id, word weight (0 = stopped word:
 * the feature is in neither vector), node id at tree level L - levelsup.  BowVector: bow_id/bow_val[*nbow],
 * ascending word ids, values L1-normalised, bit-exact doubles (weights added in feature order, norm in
 * word order as std::map iteration gives).  FeatureVector as CSR ready for orbx_featset:
 * fv_node_id[*fv_nnodes], fv_node_off[*fv_nnodes + 1], fv_feat[].  Capacities: n (n + 1 for fv_node_off). */
int orbx_bow_transform(orbx_vocab *v, const uint8_t *desc, int n, int levelsup,
                       uint32_t *word_id, double *word_weight, uint32_t *node_id,
                       uint32_t *bow_id, double *bow_val, int *nbow,
                       uint32_t *fv_node_id, int32_t *fv_node_off, uint32_t *fv_feat, int *fv_nnodes);

/* ---- projection-guided tracking matchers -------------------------------- */

/* the current Frame: undistorted keypoints, right coordinates, descriptors, image bounds (the 64x48 feature
 * grid of Frame::AssignFeaturesToGrid / GetFeaturesInArea, src/Frame.cc:261-279,:386-457, is rebuilt on device by every
 * host-pointer call; orbx_frame below keeps frame and grid resident across the searches of one frame) */
/* ---- batched, device-resident ComputeBoW + relocalisation search (BASELINE config 3 at throughput) ----
 * orbx_bow_frames holds, in HBM, what Frame::ComputeBoW produces (mBowVec, mFeatVec) for a batch of frames whose
 * keypoints / descriptors / counts are the device outputs of orbx_extract_batch_device (same cap).  Nothing crosses
 * PCIe between extraction, transform and search; orbx_bow_frames_read copies one frame's vectors to the host.
 * stream = NULL: the transform runs on the vocabulary's own stream, read / search on the stream of the last transform. */
typedef struct orbx_bow_frames orbx_bow_frames;
int orbx_bow_frames_create(int device, int max_batch, int cap, orbx_bow_frames **out);
void orbx_bow_frames_destroy(orbx_bow_frames *f);
int orbx_bow_transform_batch_device(orbx_vocab *v, orbx_bow_frames *f, const void *d_kps, const void *d_desc, const void *d_n,
                                    int batch, int levelsup, void *stream);
int orbx_bow_frames_read(orbx_bow_frames *f, int index, void *stream, uint32_t *bow_id, double *bow_val, int *nbow,
                         uint32_t *fv_node_id, int32_t *fv_node_off, uint32_t *fv_feat, int *fv_nnodes);
/* every keyframe of db against frames 0..batch-1 of f (SearchByBoW(KF, F), src/ORBmatcher.cc:171-303, in the loop of
 * Tracking::Relocalization :1661-1682): d_match[batch][nkf][cap] (int32, KF feature per frame feature or -1) and
 * d_nmatches[batch][nkf], both device memory; asynchronous on `stream`. */
int orbx_bowdb_search_batch_device(orbx_bowdb *db, const orbx_bow_frames *f, int batch, float nnratio, int check_orientation,
                                   void *d_match, void *d_nmatches, void *stream);
/* The same search with compact results: d_pairs[batch][nkf][cap_pairs][2] int32 receives, per (frame, keyframe), the first
 * min(count, cap_pairs) matches as (frame feature, keyframe feature) in frame-feature order -- what Tracking::Relocalization hands to its PnP
 * solver next (src/Tracking.cc:1682-1693) -- and d_nmatches[batch][nkf] the counts (a count above cap_pairs says the list was cut). */
int orbx_bowdb_search_batch_device_compact(orbx_bowdb *db, const orbx_bow_frames *f, int batch, float nnratio, int check_orientation,
                                           void *d_pairs, int cap_pairs, void *d_nmatches, void *stream);
/* The search over the candidates only, as the loop of Tracking::Relocalization runs it (src/Tracking.cc:1661-1682): frame b of f against the
 * keyframes its candidate list names, all frames in one launch, the lists read on the device.  d_cand[batch][cand_stride] (int32 ids) and
 * d_ncand[batch] (int32 true counts: a count above cand_stride is cut to it, a negative one reads as 0) are device memory in the layout
 * orbx_kfdb_detect_relocalization_batch_device writes with cap == cand_stride; the call is legal on the same stream directly behind it, the host
 * never reads the lists and nothing synchronises.  d_kf_of_id (optional, device int32[n_ids]) joins an id to an index of db, -1 = not in this
 * set; NULL = an id is the index (keyframes added to orbx_kfdb in the order orbx_bowdb_create received them).  Slot j of frame b is searched
 * when j < min(max(d_ncand[b], 0), cand_stride) and its keyframe index lies in [0, orbx_bowdb_size(db)) (with a map: when also 0 <= id < n_ids);
 * every id is checked before anything is indexed by it.  A searched slot receives in d_match[batch][cand_stride][cap] and
 * d_nmatches[batch][cand_stride], at [b][j], what orbx_bowdb_search_batch_device writes at [b][kf] (entries at or beyond the frame's feature count
 * are left alone); any other slot receives d_nmatches[b][j] = -1 and its row is left alone.  Slots are independent: a keyframe named twice
 * is searched twice.  ORBX_E_INVALID: a NULL handle, list or output, batch outside [1, f's max_batch], another device, cand_stride < 1 or
 * >= 2^24, batch > 65535, d_kf_of_id with n_ids < 1, feature sets too large for LDS. */
int orbx_bowdb_search_candidates_device(orbx_bowdb *db, const orbx_bow_frames *f, int batch,
                                        const void *d_cand, int cand_stride, const void *d_ncand,
                                        const void *d_kf_of_id, int n_ids,
                                        float nnratio, int check_orientation, void *d_match, void *d_nmatches, void *stream);
/* The same with compact results, slot for slot what orbx_bowdb_search_batch_device_compact writes for the keyframe (src/Tracking.cc:1661-1682,
 * the lists the PnP solvers of :1682-1693 read): d_pairs[batch][cand_stride][cap_pairs][2] receives the first min(count, cap_pairs) pairs of a
 * searched slot (the rest of the list is left alone), d_nmatches[batch][cand_stride] the count, -1 for a slot that is not searched.
 * ORBX_E_INVALID also for cap_pairs < 1. */
int orbx_bowdb_search_candidates_device_compact(orbx_bowdb *db, const orbx_bow_frames *f, int batch,
                                                const void *d_cand, int cand_stride, const void *d_ncand,
                                                const void *d_kf_of_id, int n_ids,
                                                float nnratio, int check_orientation, void *d_pairs, int cap_pairs, void *d_nmatches, void *stream);

/* ---- a live orbx_bowdb: keyframes enter, leave and change their map-point flags while the set is searched ----
 * The set of orbx_bowdb_create is immutable: a map that gains or culls a keyframe (LocalMapping::ProcessNewKeyFrame, src/LocalMapping.cc:147-193;
 * KeyFrame::SetBadFlag, src/KeyFrame.cc:489), or whose map points are created and culled (src/LocalMapping.cc:195, :237), had to rebuild it from
 * every keyframe's host feature set.  A live set holds max_kf slots of `cap` features (1 <= cap <= 8192) in one device allocation made here;
 * nothing grows afterwards.  A keyframe is named by the caller's id in [0, max_ids) -- the id orbx_kfdb_add_from_frames returned, say -- and
 * takes the lowest free slot; orbx_bowdb_size is the number of slots ever used, and the all-keyframes searches report slot i at index i (an
 * empty slot as a keyframe without features: count 0).  Every search entry point above accepts a live set unchanged, except that the candidate
 * searches join ids to slots through the set's own map: d_kf_of_id must be NULL (an explicit map with a live set is ORBX_E_INVALID).
 * Streams: every call that enqueues work on the set -- the searches included -- first makes its stream wait for the previous such call when
 * that went to another stream, so a slot is never rewritten under a search in flight elsewhere; no call needs a host synchronisation between.
 * Refusals come before any device work and leave the set unchanged.  ORBX_E_INVALID: a NULL argument, a set of orbx_bowdb_create, frames of
 * another device or cap, an index outside the frames' batch, an id outside [0, max_ids), an id already in the set (add), an id not in the set
 * (erase, set_flags, read_keyframe), a feature set with more than cap features or nodes.  ORBX_E_CAPACITY: no free slot.  An erased id may be
 * added again. */
int orbx_bowdb_create_live(int device, int max_kf, int cap, int max_ids, orbx_bowdb **out);
/* Keyframe `id` from slot `index` of f (orbx_bow_transform_batch_device's output), device to device, asynchronous on `stream` (NULL: the stream
 * of f's last transform); the counts are read on the device.  Replaces the download, feat_pack and upload of orbx_bowdb_create for the
 * keyframe.  d_flag = device uint8[cap], != 0 <=> feature i holds a non-bad MapPoint (src/ORBmatcher.cc:205-210); NULL = every feature does. */
int orbx_bowdb_add_from_frames(orbx_bowdb *db, int id, const orbx_bow_frames *f, int index, const void *d_flag, void *stream);
/* The same from a host feature set, validated as orbx_bowdb_create validates it, kf->n and kf->nnodes <= cap.  Synchronises `stream`
 * (NULL: the set's own). */
int orbx_bowdb_add(orbx_bowdb *db, int id, const orbx_featset *kf, void *stream);
/* KeyFrameDatabase::erase (src/KeyFrameDatabase.cc:48-68) for the searched set: asynchronous, the slot is free for the next add. */
int orbx_bowdb_erase(orbx_bowdb *db, int id, void *stream);
/* New map-point flags for n distinct live keyframes in ONE launch: flags[i] = host uint8[that keyframe's feature count].  The searched form is
 * rebuilt on the device from the resident descriptors (replaces the rebuild of the set).  Synchronises `stream`. */
int orbx_bowdb_set_flags(orbx_bowdb *db, const int32_t *ids, int n, const uint8_t *const *flags, void *stream);
int orbx_bowdb_live_count(const orbx_bowdb *db);                                /* keyframes in the set (a negative code on error) */
/* id_of_slot[nslots >= orbx_bowdb_size(db)] = the id behind each slot, -1 = empty: the join orbx_bowdb_create's caller keeps by hand
 * (ORBX_E_CAPACITY: nslots too small). */
int orbx_bowdb_ids(const orbx_bowdb *db, int32_t *id_of_slot, int nslots);
/* Tests and debugging: the searched form of keyframe `id` as the kernels see it, through its device record.  node_id[nnodes],
 * node_off[nnodes + 1], feat / sdesc[32 x] / sflag over the filtered list of node_off[nnodes] entries, flag / angle / desc[32 x] over n; every
 * array has room for cap entries (node_off cap + 1).  NULL arguments are skipped.  Synchronises. */
int orbx_bowdb_read_keyframe(orbx_bowdb *db, int id, int *n, int *nnodes, uint32_t *node_id, int32_t *node_off,
                             uint32_t *feat, uint8_t *flag, float *angle, uint8_t *desc, uint8_t *sdesc, uint8_t *sflag);

/* ---- KeyFrameDatabase: the place-recognition query in front of the relocalisation / loop-closing searches ----
 * orbx_kfdb keeps the live keyframes' BowVectors (ascending uint32 word ids, the doubles orbx_bow_transform returns) in HBM, with up to
 * 10 covisibility neighbours and one persistent relocalisation score per keyframe; the host needs the vectors no more after add.
 * An id is the add sequence number: it grows monotonically and is not reused before orbx_kfdb_clear.  Candidates come back in the
 * reference's return order, which is ascending (smallest common word id, id) of the group that first names them.
 * Every call is a fresh query identity, and a keyframe's relocalisation score starts at 0.0f (the reference leaves it uninitialised).
 * Calls on one handle serialise inside it (the reference holds mMutex).  ORBX_E_INVALID: ids not ascending, a word id >= nwords,
 * a non-finite value, an unknown or erased id where a live one is required.  These checks read HOST vectors: a vector that is resident in an
 * orbx_bow_frames (add_from_frames, the _frame and batch forms) is taken as orbx_bow_transform_batch_device wrote it -- ascending ids below
 * the vocabulary's size, finite values -- and is not read back to be checked; no kernel indexes anything by a word id, so a malformed resident
 * vector gives wrong candidates, never an access out of bounds. */
typedef struct orbx_kfdb orbx_kfdb;
/* KeyFrameDatabase::KeyFrameDatabase / clear (src/KeyFrameDatabase.cc:33-37, :69-73); nwords = the vocabulary's size */
int orbx_kfdb_create(int device, int nwords, orbx_kfdb **out);
void orbx_kfdb_destroy(orbx_kfdb *db);
int orbx_kfdb_size(orbx_kfdb *db);       /* live keyframes */
int orbx_kfdb_next_id(orbx_kfdb *db);    /* ids issued since create / clear: the length of the per-id arrays below */
int orbx_kfdb_clear(orbx_kfdb *db);      /* ids restart at 0 */
/* KeyFrameDatabase::add (:40-46) from host arrays, or device to device from frame `index` of an orbx_bow_frames (only the word
 * count comes to the host; synchronises `stream`, NULL = the stream of the frames' last transform) */
int orbx_kfdb_add(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, int *id);
int orbx_kfdb_add_from_frames(orbx_kfdb *db, orbx_bow_frames *f, int index, void *stream, int *id);
/* KeyFrameDatabase::erase (:48-67); the arena storage is reclaimed when the arena next grows */
int orbx_kfdb_erase(orbx_kfdb *db, int id);
/* KeyFrame::GetBestCovisibilityKeyFrames(10) of keyframe id, in its order (n <= 10); neighbour ids that are unknown or erased at
 * query time are ignored (the reference's lists never hold an erased keyframe) */
int orbx_kfdb_set_covisibility(orbx_kfdb *db, int id, const int32_t *neigh_ids, int n);
/* ORBVocabulary::score(query, keyframe ids[i]) = L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), the loop of
 * src/LoopClosing.cc:143-162: bit-exact doubles (terms added in ascending word order); the caller rounds to float as the reference does */
int orbx_kfdb_score(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, const int32_t *ids, int n, double *scores);
int orbx_kfdb_score_frame(orbx_kfdb *db, orbx_bow_frames *f, int index, const int32_t *ids, int n, double *scores);
/* KeyFrameDatabase::DetectRelocalizationCandidates (:234-349) and DetectLoopCandidates (:80-229; connected_ids = pKF->GetConnectedKeyFrames(),
 * min_score = minScore).  cand[cap] receives *ncand ids; ORBX_E_CAPACITY with *ncand = the true count when the list is longer.
 * Optional stage outputs of orbx_kfdb_next_id entries each: words_out[id] = common words (mnRelocWords / mnLoopWords; 0 for erased and
 * connected keyframes), score_out[id] = the float score of the keyframes this query scored, 0 elsewhere.  The query is a host BowVector
 * or frame `index` of an orbx_bow_frames (the _frame forms).  A relocalisation query that ends in ORBX_E_CAPACITY has run like any other:
 * the keyframes it scored keep those scores as their persistent ones (the list is known only after the query), and asking again with a
 * larger cap returns the same list.  Cost note: the returned keyframes are ordered by a counting rank inside one workgroup, quadratic in the
 * length of the LIST (not of the database): a handful in place recognition; a query built to return thousands (thousands of identical
 * keyframes) spends milliseconds there. */
int orbx_kfdb_detect_relocalization(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, int32_t *cand, int cap,
                                    int *ncand, int32_t *words_out, float *score_out);
int orbx_kfdb_detect_relocalization_frame(orbx_kfdb *db, orbx_bow_frames *f, int index, int32_t *cand, int cap, int *ncand,
                                          int32_t *words_out, float *score_out);
int orbx_kfdb_detect_loop(orbx_kfdb *db, const uint32_t *bow_id, const double *bow_val, int nbow, const int32_t *connected_ids, int nconnected,
                          float min_score, int32_t *cand, int cap, int *ncand, int32_t *words_out, float *score_out);
int orbx_kfdb_detect_loop_frame(orbx_kfdb *db, orbx_bow_frames *f, int index, const int32_t *connected_ids, int nconnected, float min_score,
                                int32_t *cand, int cap, int *ncand, int32_t *words_out, float *score_out);
/* frames 0..batch-1 of f as relocalisation queries, asynchronous on `stream`, nothing crosses PCIe: d_cand[batch][cap] (int32; the first
 * min(count, cap) candidates) and d_ncand[batch] (true counts) are device memory.  Equals `batch` per-call queries issued in frame order,
 * the persistent scores included (batch <= 1024).  The handle's next call waits for the stream. */
int orbx_kfdb_detect_relocalization_batch_device(orbx_kfdb *db, orbx_bow_frames *f, int batch, void *d_cand, int cap, void *d_ncand, void *stream);
/* Test and tool utility: a BowVector computed elsewhere into slot `index` of an orbx_bow_frames, so that the forms above that take frames can be
 * driven with chosen vectors.  Checks nbow <= cap, ascending ids and finite values (it knows no vocabulary: word id < nwords is the caller's to
 * keep).  The slot's FeatureVector is NOT touched and no longer belongs to the slot's BowVector: do not hand such a slot to the SearchByBoW
 * forms.  stream = NULL: the stream of the frames' last transform (the default stream if there was none); synchronises it. */
int orbx_bow_frames_set_bow(orbx_bow_frames *f, int index, const uint32_t *bow_id, const double *bow_val, int nbow, void *stream);
/* the persistent relocalisation scores (mRelocScore, :289 / :315): scores[i] for ids 0..n-1, 0.0f past the ids issued */
int orbx_kfdb_reloc_scores(orbx_kfdb *db, float *scores, int n);

typedef struct {
    int n;
    const float *x, *y;        /* mvKeysUn[i].pt */
    const int32_t *octave;     /* mvKeysUn[i].octave */
    const float *angle;        /* mvKeysUn[i].angle */
    const float *u_right;      /* mvuRight */
    const uint8_t *desc;       /* mDescriptors [n][32] */
    const uint8_t *occupied;   /* 1: mvpMapPoints[i] is set and has Observations() > 0 before the call */
    float min_x, min_y, max_x, max_y; /* mnMinX, mnMinY, mnMaxX, mnMaxY */
} orbx_frame_feats;
/* the projected map points in the reference's iteration order; the adaptor (which has the poses) projects */
typedef struct {
    int n;
    const float *u, *v;        /* last-frame search: u, v of src/ORBmatcher.cc:1428-1429 ; map-point search: mTrackProjX/Y */
    const float *aux;          /* last-frame search: invzc (:1425)                   ; map-point search: mTrackProjXR */
    const int32_t *level;      /* last-frame search: LastFrame.mvKeys[i].octave      ; map-point search: mnTrackScaleLevel */
    const float *angle;        /* last-frame search only: LastFrame.mvKeysUn[i].angle */
    const float *view_cos;     /* map-point search only: mTrackViewCos */
    const uint8_t *desc;       /* pMP->GetDescriptor() [n][32] */
    const uint8_t *valid;      /* last-frame: pMP && !mvbOutlier[i] ; map-point: mbTrackInView && !isBad() */
    const uint8_t *has_obs;    /* pMP->Observations() > 0: a match by this point blocks the feature for later points */
} orbx_proj_points;

/* ---- resident current frame ------------------------------------------------------------------------
 * Tracking searches one Frame by projection two to four times (TrackWithMotionModel at th and again at 2*th,
 * src/Tracking.cc:1065,:1072; SearchLocalPoints :1463; Relocalization :1763,:1777), and the frame's keypoints, descriptors
 * and 64x48 grid (Frame::AssignFeaturesToGrid, src/Frame.cc:261-279) never change in between.  orbx_frame keeps that
 * immutable part in HBM -- undistorted x / y, octave, angle, u_right, descriptors, bounds and the grid, built once at
 * creation -- and the searches below move only the projected points, the per-call `occupied` bytes and the results.
 * One frame is used by one thread at a time (as the extractor handles); distinct frames may be used concurrently.  (The
 * keyframe searches further down -- orbx_frame_window_best, _window_best_batch, _search_by_sim3, _search_by_projection_sim3 --
 * only read the handle and may share one frame among threads; see there.) */
typedef struct orbx_frame orbx_frame;
/* from host pointers: one upload, then the grid build; synchronises.  f->occupied is ignored; f->angle may be NULL (then only
 * searches without the orientation check accept the frame).  Refused as the host-pointer searches refuse the frame: n >= 65536,
 * empty bounds, missing arrays. */
int orbx_frame_create(int device, const orbx_frame_feats *f, orbx_frame **out);
/* from the device outputs of orbx_extract_batch_device (image `index` of a launch with capacity `cap`): keypoints
 * d_kps + index*cap (orbx_keypoint records), descriptors d_desc + index*cap*32, count d_n[index] (int32).  d_u_right = that
 * image's [cap] row of orbx_stereo_match_batch_device's u_right output, or NULL for a monocular frame (every u_right = -1).
 * K = fx fy cx cy (may be NULL: positions are taken as they are); with K and dist_coef[0] != 0 (ndist 4 or 5) the positions are
 * undistorted on the device with the arithmetic of orbx_undistort_keypoints, bit for bit; dist_coef[0] == 0 copies them
 * (src/Frame.cc:472-476).  Bounds = mnMinX, mnMinY, mnMaxX, mnMaxY.  The work is enqueued on `stream` (the stream the
 * extraction ran on; NULL = the null stream) and nothing but the count passes through host memory: the call synchronises
 * `stream` ONCE to read those 4 bytes (the count sizes the frame), then enqueues the copy and the grid build and returns.  The
 * frame owns a copy: the extraction buffers may be overwritten afterwards.  Its first search waits for the creation through an
 * event, not a device synchronisation.  Refused: index < 0, cap < 1, a count outside [0, cap]. */
int orbx_frame_create_from_extraction(int device, const void *d_kps, const void *d_desc, const void *d_n, int cap, int index,
                                      const void *d_u_right, const float *K, const float *dist_coef, int ndist,
                                      float min_x, float min_y, float max_x, float max_y, void *stream, orbx_frame **out);
int orbx_frame_size(const orbx_frame *f);
/* tests and debugging: copies the frame's arrays to host memory ([n] each, desc [n][32]); NULL arguments are skipped */
int orbx_frame_read(const orbx_frame *f, float *x, float *y, int32_t *octave, float *angle, float *u_right, uint8_t *desc);
void orbx_frame_destroy(orbx_frame *f);
/* The three per-frame searches on a resident frame: arguments, semantics and results of orbx_search_by_projection_last_frame /
 * _map_points / _keyframe, with the frame given by handle and occupied[n] (the meaning each host-pointer twin gives
 * orbx_frame_feats::occupied) passed per call; occupied = NULL: no feature is occupied. */
int orbx_frame_search_by_projection_last_frame(orbx_frame *cur, const uint8_t *occupied, const orbx_proj_points *pts,
                                               const float *scale_factors, int nlevels, float th, int direction, float mbf,
                                               int check_orientation, int32_t *match_cur, int *nmatches);
int orbx_frame_search_by_projection_map_points(orbx_frame *cur, const uint8_t *occupied, const orbx_proj_points *pts,
                                               const float *scale_factors, int nlevels, float th, float nnratio,
                                               int32_t *match_cur, int *nmatches);
int orbx_frame_search_by_projection_keyframe(orbx_frame *cur, const uint8_t *occupied, const orbx_proj_points *pts,
                                             const float *scale_factors, int nlevels, float th, int orb_dist,
                                             int check_orientation, int32_t *match_cur, int *nmatches);

/* ---- resident keyframes for the projection searches of LocalMapping and LoopClosing ----------------------------------
 * A keyframe's keypoints and descriptors never change once it exists (src/KeyFrame.cc:29-60), and the same keyframes are
 * searched again and again (LocalMapping::SearchInNeighbors, src/LocalMapping.cc:515-599: Fuse into up to 60 / 120 neighbours
 * per new keyframe; LoopClosing::ComputeSim3 / SearchAndFuse).  An orbx_frame made once from the keyframe (mvKeysUn, mvuRight,
 * mDescriptors, the keyframe's image bounds) serves as the target: a call moves only the projected points and the results.
 * Arguments, results and refusals are those of the host-pointer twins named below, with the keyframe given by handle.
 * THREADS: unlike the three per-frame searches above, the four calls below take a const handle and only read it -- several
 * threads may search one keyframe at the same time (LocalMapping and LoopClosing do); the staging is the calling thread's.  A
 * frame whose creation is still pending (orbx_frame_create_from_extraction) is waited for through its event, the handle is
 * not written.  NULL and range refusals come before any device call. */
/* orbx_window_best on a resident keyframe: the search half of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:873-1038), of Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:1040-1164) and of each direction of
 * SearchBySim3 (:1218-1372).  One upload (the points), one launch, one download; nfound may be NULL. */
int orbx_frame_window_best(const orbx_frame *kf, const orbx_proj_points *pts, const float *scale_factors,
                           const float *inv_sigma2, int nlevels, float th, int chi2, int max_dist,
                           int32_t *best_idx, int32_t *best_dist, int *nfound);
/* one (keyframe, points) search of a batch: the arguments of orbx_frame_window_best */
typedef struct {
    const orbx_frame *kf; const orbx_proj_points *pts;
    const float *scale_factors, *inv_sigma2;     /* [nlevels] of kf; inv_sigma2 only when chi2 != 0 */
    int nlevels; float th; int chi2, max_dist;
    int32_t *best_idx, *best_dist;               /* [pts->n] out; best_dist may be NULL */
    int nfound;                                  /* out */
} orbx_window_job;
/* njobs searches (the loop `for each target keyframe: Fuse(pKFi, vpMapPointMatches)` of src/LocalMapping.cc:549-554, or the two
 * directions of SearchBySim3) as ONE upload, ONE launch, ONE download; every job's results equal its single call.  A keyframe may
 * be named by several jobs; jobs whose pts->desc is the same host array (and length) share one uploaded copy.  A job without
 * points or whose keyframe has no features gets -1 / 256 / nfound 0; if every job is empty nothing is launched.
 * ORBX_E_INVALID: njobs outside [1, 1024], a NULL handle / points / scale_factors / best_idx, keyframes on different devices, more
 * than 2^20 points in all, max_dist outside [0, 256], nlevels outside [1, 16], a valid point whose level is outside [0, nlevels),
 * missing point arrays (u, v, level, desc, valid; aux and inv_sigma2 when chi2). */
int orbx_frame_window_best_batch(orbx_window_job *jobs, int njobs);
/* orbx_search_by_projection_sim3 (ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th), src/ORBmatcher.cc:305-415)
 * on a resident keyframe; occupied[kf n] = vpMatched[idx] != NULL passed per call (NULL: none).  Matches claim their keypoint,
 * so this search keeps the list + resolve kernels of its twin. */
int orbx_frame_search_by_projection_sim3(const orbx_frame *kf, const uint8_t *occupied, const orbx_proj_points *pts,
                                         const float *scale_factors, int nlevels, float th, int32_t *match_kf, int *nmatches);
/* orbx_search_by_sim3 (ORBmatcher::SearchBySim3, src/ORBmatcher.cc:1166-1394) on two resident keyframes: both directions
 * (:1218-1292, :1295-1372) are two jobs of one batch launch, then the agreement check of :1375-1391 on the host. */
int orbx_frame_search_by_sim3(const orbx_frame *kf1, const orbx_frame *kf2, const orbx_proj_points *pts12,
                              const orbx_proj_points *pts21, const float *scale_factors1, const float *scale_factors2,
                              int nlevels, float th, int32_t *match12, int *nfound);

/* ---- resident map points: Frame::isInFrustum and Tracking::SearchLocalPoints from a pose -----------------------------
 * Tracking::SearchLocalPoints (src/Tracking.cc:1403-1466) runs on every tracked frame: Frame::isInFrustum (src/Frame.cc:310-380) on
 * each of the 2 000 - 8 000 local map points, then ORBmatcher::SearchByProjection(F, vpLocalMapPoints, th).  A map point's
 * position, normal, distance range and descriptor change rarely, and then one point at a time; the pose changes every frame and
 * is 15 floats.  orbx_mappoints keeps the points in HBM, a slot per point, and the searches below move a pose, one int32 slot
 * and one flag byte per local point, `occupied`, and the results.
 * The table has a fixed capacity and ONE device allocation made at creation; nothing grows: 64 bytes per slot, plus the staging of
 * one upload (68 bytes for each of min(capacity, 65536) records, and a pinned host buffer of that size).  THREADS: _set serialises against
 * every other call on the table; _frustum, _read and orbx_frame_search_local_points only read it and may run from several
 * threads at once.  A _set on one stream and a search on another are ordered through an event the table keeps (no device
 * synchronisation), and a slot is never rewritten under a search in flight. */
typedef struct orbx_mappoints orbx_mappoints;
/* ORBX_E_INVALID: out == NULL, capacity outside [1, 2^24] */
int orbx_mappoints_create(int device, int capacity, orbx_mappoints **out);
void orbx_mappoints_destroy(orbx_mappoints *m);
int orbx_mappoints_capacity(const orbx_mappoints *m);                          /* a negative code on error */
/* Writes n slots: geom[n][8] = X Y Z mfMinDistance nx ny nz mfMaxDistance (mWorldPos, mNormalVector and the RAW distances, not
 * GetMinDistanceInvariance's 0.8 / GetMaxDistanceInvariance's 1.2 products), desc[n][32] = mDescriptor.  Either array may be
 * NULL to leave that half of every named slot as it is (UpdateNormalAndDepth and bundle adjustment change only geom,
 * ComputeDistinctiveDescriptors only desc), provided each named slot has been given that half before.  A slot is "set" once it
 * has been given both halves; the host keeps that bitmap.  One upload -- packed by n: 4 + 32 bytes per record for one half, 4 + 64 for both, whatever the
 * capacity -- and one scatter kernel per 65536 records (a frame's changes are one of each), enqueued on `stream` (NULL: the
 * calling thread's own stream); the call does not wait for them -- later calls on the table are ordered behind them.
 * Refusals come before any device work and leave the table unchanged.  ORBX_E_CAPACITY: a slot >= capacity.  ORBX_E_INVALID: a
 * negative slot, a slot named twice in one call, both arrays NULL, a half left out that the slot never had. */
int orbx_mappoints_set(orbx_mappoints *m, const int32_t *slots, int n, const float *geom, const uint8_t *desc, void *stream);
/* tests and debugging: geom[n][8] / desc[n][32] of the named slots (NULL arguments are skipped; a half never given reads 0) */
int orbx_mappoints_read(const orbx_mappoints *m, const int32_t *slots, int n, float *geom, uint8_t *desc);
/* Frame::isInFrustum for points slots[0..n) of the table.  pose = Rcw[9] (row major) tcw[3] Ow[3]; cam = fx fy cx cy mbf mnMinX
 * mnMinY mnMaxX mnMaxY; log_scale_factor = mfLogScaleFactor, nlevels = mnScaleLevels.  eligible[i] == 0 (the caller's isBad() /
 * mnLastFrameSeen tests, src/Tracking.cc:1437-1440) gives in_view[i] = 0 without touching the table: its slot may be anything.
 * An eligible point whose slot is out of range or not set is refused, ORBX_E_INVALID, before any launch.  Outputs (in_view is
 * required, the others may be NULL): in_view = mbTrackInView, u / v / xr = mTrackProjX / Y / XR, level = mnTrackScaleLevel,
 * view_cos = mTrackViewCos; a point not in view reads 0 in all of them.
 * The arithmetic is fixed, in this order, in float unless a step says double, every operation rounded on its own (no fused
 * multiply-add), division and square root correctly rounded:
 *   1. Pc_k = ((R[k][0]*X + R[k][1]*Y) + R[k][2]*Z) + t[k]; out if Pc_z < 0
 *   2. invz = 1.0f / Pc_z; u = (fx*Pc_x)*invz + cx; v = (fy*Pc_y)*invz + cy; out if u < mnMinX, u > mnMaxX, v < mnMinY or
 *      v > mnMaxY (the bounds are inclusive), and out if u or v is not finite (a defined deviation: the reference would carry
 *      a NaN into GetFeaturesInArea, whose float-to-int conversion is undefined)
 *   3. PO = P - Ow per component; dist = (float)sqrt(((double)POx*POx + (double)POy*POy) + (double)POz*POz) (cv::norm
 *      accumulates CV_32F in double); out if dist < 0.8f*dmin or dist > 1.2f*dmax
 *   4. view_cos = (float)((((double)POx*nx + (double)POy*ny) + (double)POz*nz) / (double)dist) (Mat::dot in double); out if it
 *      is not finite or < view_cos_limit
 *   5. ratio = dmax / dist; level = clamp(ceilf(logf(ratio) / log_scale_factor), 0, nlevels - 1) with the C library's logf:
 *      the device evaluates no logarithm.  At call time the host finds, for k = 0 .. nlevels - 2, the smallest positive float
 *      r_k with ceilf(logf(r_k) / log_scale_factor) > k (bisection over float bit patterns, cached per (log_scale_factor,
 *      nlevels)), and the device counts the r_k <= ratio.  (A NaN ratio, from a NaN dmax, counts 0.)
 *   6. xr = u - mbf*invz
 * Against OpenCV's own cv::Mat arithmetic this restatement is unpinned. */
int orbx_mappoints_frustum(const orbx_mappoints *m, const int32_t *slots, const uint8_t *eligible, int n, const float *pose,
                           const float *cam, float view_cos_limit, float log_scale_factor, int nlevels, uint8_t *in_view,
                           float *u, float *v, float *xr, int32_t *level, float *view_cos);
/* The second loop of Tracking::SearchLocalPoints and its matcher call (src/Tracking.cc:1433-1463) in one call on a resident
 * frame: orbx_mappoints_frustum, then orbx_frame_search_by_projection_map_points on its outputs -- bit for bit that pair of
 * calls, without the points crossing PCIe.  flags[i] bit 0 = eligible, bit 1 = Observations() > 0 (orbx_proj_points::has_obs).
 * One upload (slots, flags, occupied), three launches (the frustum kernel, which writes the dense point set with each in-view
 * point's descriptor copied out of the table, then the list and resolve kernels of the map-point search), one group of
 * downloads behind one synchronisation: match_cur[cur n] (an index into slots[] / flags[], -1 none), *nmatches, in_view[n]
 * (for IncreaseVisible() and nToMatch).  n == 0 or a frame without features: ORBX_OK, no launch, match_cur = -1, in_view = 0.
 * Refusals as orbx_mappoints_frustum and the map-point search; also a frame and a table on different devices. */
int orbx_frame_search_local_points(orbx_frame *cur, const uint8_t *occupied, const orbx_mappoints *m, const int32_t *slots,
                                   const uint8_t *flags, int n, const float *pose, const float *cam, float view_cos_limit,
                                   float log_scale_factor, const float *scale_factors, int nlevels, float th, float nnratio,
                                   int32_t *match_cur, int *nmatches, uint8_t *in_view);

/* ---- resident observation graph: covisibility votes and LocalMapping::KeyFrameCulling -----------------------------------
 * Who observes what, in both views of the reference, kept independently because the reference lets them disagree:
 *   keyframe view, per keyframe slot and feature: the point slot or -1 (mvpMapPoints[i]), the octave (mvKeysUn[i].octave), a
 *     stereo bit (mvuRight[i] >= 0) and a close bit (0 <= mvDepth[i] <= mThDepth);
 *   point view, per point slot: up to max_obs (keyframe slot, feature index) entries (mObservations), nObs with the reference's
 *     weights (+2 stereo, +1 mono), a live bit and a bad bit.
 * The order of the entries within a row is unobservable (the reference's is the order of KeyFrame addresses); mpRefKF is not
 * modelled.  A point slot is free until its first observation makes it live; it goes bad through orbx_mapgraph_erase_points, or
 * when an erasure leaves it at nObs <= 2 (src/MapPoint.cc:137-144); nObs of a bad point stays what it was, as in the reference.  An
 * add_observations on a bad slot uses the slot again for a new point (nObs from 0, not bad): the caller's to do only once no match
 * names the slot.  A row entry may outlive its keyframe (an observation without a match survives erase_keyframe, as a pointer to a
 * bad KeyFrame does in the reference) and then still counts in the queries, with the attributes the slot last held; the slot is not
 * given to a new keyframe before those entries are erased.
 * Fixed capacities and ONE device allocation made at creation; nothing grows.  Bytes: 4 per keyframe slot, 5 per (keyframe slot,
 * feature), 4 + 4 * max_obs per point slot -- at most 2^32 - 1 words of 4 bytes in all, more is ORBX_E_INVALID -- plus the staging of
 * one edit upload (512 KiB + max_features, and a pinned host buffer of that size).  The host keeps a mirror of the same size, on which
 * every refusal is decided: every refusal comes before any device work and leaves the graph unchanged.  The queries run on the
 * device's copy alone.
 * Each edit is one packed upload -- 8 bytes for every word of the graph that the edit changes, whatever the capacities -- and one
 * scatter launch on the calling thread's own stream; the call does not wait for them, later calls on the graph are ordered behind
 * them.  Calls on one handle serialise inside it (the reference holds mMutexFeatures). */
typedef struct orbx_mapgraph orbx_mapgraph;
/* ORBX_E_INVALID: out == NULL, max_keyframes or max_features outside [1, 65535], max_points outside [1, 2^24], max_obs outside [4, 256] */
int orbx_mapgraph_create(int device, int max_keyframes, int max_features, int max_points, int max_obs, orbx_mapgraph **out);
void orbx_mapgraph_destroy(orbx_mapgraph *g);
int orbx_mapgraph_clear(orbx_mapgraph *g);   /* Map::clear: every keyframe slot and point slot free */
/* A new keyframe of n features in the free slot kf, all matches -1.  octave[i] <= 31; stereo[i] / close[i]: any non-zero byte sets the bit.
 * ORBX_E_INVALID: a negative slot, a slot in use, a free slot that observations still name, an octave above 31; ORBX_E_CAPACITY:
 * kf >= max_keyframes, n > max_features. */
int orbx_mapgraph_set_keyframe(orbx_mapgraph *g, int kf, int n, const uint8_t *octave, const uint8_t *stereo, const uint8_t *close);
/* KeyFrame::AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch: match[kf][idx[j]] = point[j] (-1 erases); touches the keyframe view
 * only.  ORBX_E_INVALID: kf not in use, a feature outside the keyframe or named twice, a point slot < -1; ORBX_E_CAPACITY: a point
 * slot >= max_points. */
int orbx_mapgraph_set_matches(orbx_mapgraph *g, int kf, const int32_t *idx, const int32_t *point, int n);
/* MapPoint::AddObservation (src/MapPoint.cc:106-117), entry by entry in the given order: a keyframe already in the row is a no-op; a
 * point's first observation makes it live.  ORBX_E_INVALID: a negative point slot, a keyframe slot not in use, a feature outside the
 * keyframe, a (point, keyframe) pair named twice; ORBX_E_CAPACITY: a point slot >= max_points, a row beyond max_obs. */
int orbx_mapgraph_add_observations(orbx_mapgraph *g, const int32_t *point, const int32_t *kf, const int32_t *idx, int n);
/* MapPoint::EraseObservation (src/MapPoint.cc:119-145): nObs drops by the weight of the stored entry; a point that ends at nObs <= 2
 * after losing an entry goes bad: its row is cleared and the match at every former observer's index is set to -1 (whatever it was:
 * KeyFrame::EraseMapPointMatch does not look).  A keyframe that is not in the row is a no-op.  Several erasures of one point in a batch
 * are order-free.  ORBX_E_INVALID: a negative slot, a pair named twice; ORBX_E_CAPACITY: a slot beyond its capacity. */
int orbx_mapgraph_erase_observations(orbx_mapgraph *g, const int32_t *point, const int32_t *kf, int n);
/* MapPoint::SetBadFlag (src/MapPoint.cc:159-176): bad, the row cleared, the observers' matches -1.  ORBX_E_INVALID: a negative slot, a
 * slot named twice; ORBX_E_CAPACITY: a slot >= max_points. */
int orbx_mapgraph_erase_points(orbx_mapgraph *g, const int32_t *point, int n);
/* The map-point part of KeyFrame::SetBadFlag (src/KeyFrame.cc:505-507): EraseObservation(kf) on the point of every match, then the slot
 * is free.  ORBX_E_INVALID: kf not in use. */
int orbx_mapgraph_erase_keyframe(orbx_mapgraph *g, int kf);
/* The row entries that name keyframe slot kf, in use or free (a negative code on error).  An observation without a match survives
 * erase_keyframe, so a free slot may still be named; orbx_mapgraph_set_keyframe refuses such a slot, and a caller that hands out slots
 * asks here first (or erases those observations). */
int orbx_mapgraph_keyframe_observations(orbx_mapgraph *g, int kf);
/* tests and debugging, read from the device's copy.  *n = the feature count, -1 for a free slot; point / octave / stereo / close[max_features]
 * (NULL arguments are skipped). */
int orbx_mapgraph_read_keyframe(orbx_mapgraph *g, int kf, int *n, int32_t *point, uint8_t *octave, uint8_t *stereo, uint8_t *close);
/* point slots first .. first + n - 1: n_obs[n] = nObs, flags[n] bit 0 = live, bit 1 = bad, n_entries[n], and kf / idx[n][max_obs] = the rows,
 * n_entries[p] words of each (NULL arrays are skipped) */
int orbx_mapgraph_read_points(orbx_mapgraph *g, int first, int n, int32_t *n_obs, uint8_t *flags, int32_t *n_entries, int32_t *kf, int32_t *idx);
/* keyframeCounter of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1519-1538): for every listed point that is live and not bad,
 * counts[observer]++ for each entry of its row.  counts[max_keyframes] comes back dense, by keyframe slot; nz_slots[max_keyframes] / *n_nz
 * (either may be NULL) receive the slots with a non-zero count, ascending.  Integer sums only: exact in any order.  One upload, one
 * launch (a workgroup histogram in LDS up to 8192 keyframe slots, global integer atomics beyond), one download.  The threshold, the
 * maximum and the sort stay with the caller: they depend on the reference's pointer order.  ORBX_E_INVALID: n outside [0, 2^20], a
 * point slot outside [0, max_points). */
int orbx_mapgraph_vote(orbx_mapgraph *g, const int32_t *points, int n, int32_t *counts, int32_t *nz_slots, int *n_nz);
/* KFcounter of KeyFrame::UpdateConnections (src/KeyFrame.cc:305-338): the same kernel over kf's own matches, kf itself left out.  No
 * upload.  ORBX_E_INVALID: kf not in use. */
int orbx_mapgraph_covisibility(orbx_mapgraph *g, int kf, int32_t *counts, int32_t *nz_slots, int *n_nz);
/* The loop of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:713-774) over local[0 .. n_local) in the given order; the caller
 * leaves out mnId == 0.  Per keyframe k: over its matches i with a live, not-bad point p, skipped unless `monocular` or close: nMPs++;
 * if nObs(p) > 3, the row entries (k', i') with k' != k and octave(k', i') <= octave(k, i) + 1 are counted, and 3 or more make the
 * feature redundant.  k is culled when (double)nRedundant > 0.9 * (double)nMPs, one fp64 product as the reference writes it.  A culled
 * keyframe with not_erase[j] set gets culled[j] = 2 and the graph stays as it is (mbToBeErased); otherwise culled[j] = 1 and
 * orbx_mapgraph_erase_keyframe, with its cascade of bad points, happens BEFORE the next keyframe is judged.  n_mps[j] / n_redundant[j]
 * (may be NULL) are the values seen at that keyframe's turn; bad_points[cap] / *n_bad the point slots that went bad, ascending;
 * ORBX_E_CAPACITY with *n_bad = the true count when there are more than cap (the call has run like any other, the graph has changed).
 * One upload, two launches -- every (keyframe, feature) judged on the graph as it stands, then one workgroup that takes the keyframes in
 * order and, behind a real cull, judges every later keyframe again -- one download.  n_local == 0: ORBX_OK, no launch.
 * ORBX_E_INVALID: a keyframe slot not in use or named twice, n_local > 65535. */
int orbx_mapgraph_cull_keyframes(orbx_mapgraph *g, const int32_t *local, const uint8_t *not_erase, int n_local, int monocular,
                                 uint8_t *culled, int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points, int cap, int *n_bad);

/* ---- map points refreshed on the device: MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors -----------
 * The loops over map points behind SearchInNeighbors, CreateNewMapPoints, the bundle adjustments and the essential-graph correction
 * (src/LocalMapping.cc:187-188, :505-507, :595-596, src/Optimizer.cc:860, :1151, src/LoopClosing.cc) call src/MapPoint.cc:371-420 and
 * :266-340 point by point.  Their inputs are resident: the rows, live and bad bits and octaves in the graph, the keyframes' descriptors
 * in their orbx_frame, the positions in the orbx_mappoints table (or handed over by a bundle adjustment); their outputs are exactly the
 * 64 bytes per slot of that table.  One call reads the graph and the frames and writes the table in place; the same values come back
 * for the MapPoint members.
 * Per listed point i:
 *   status[i]   bit 0: the geometry was updated, bit 1: the descriptor was updated.  A point that is not live, is bad or has an empty row
 *               gets 0 and nothing of it is written anywhere (the reference's early return).
 *   GEOM        every row entry counts, bad keyframes and entries that outlived their keyframe included (the reference does not ask
 *               isBad() here).  The reference feature is the row entry of ref_kf[i]; a row without one takes feature 0 of that
 *               keyframe (observations[pRefKF] on the reference's local copy default-inserts 0).  geom[i][8] = X Y Z mfMinDistance nx
 *               ny nz mfMaxDistance, the table's record: X Y Z are pos[i], or what the table held.
 *   DESC        only entries whose keyframe has kf_bad == 0 take part; if none does, bit 1 stays clear and the descriptor is left alone.
 *               best_kf[i] / best_idx[i] name the winning (keyframe slot, feature), desc[i][32] is its descriptor.
 *   ORDER       entries are taken in ascending keyframe slot (a keyframe is in a row at most once).  The stored order of a row is
 *               unobservable, so the result does not depend on it.  A STATED DEVIATION: the reference iterates in KeyFrame* address
 *               order, whatever its allocator produced.  The order decides the rounding of the float sum, and the winner among equal
 *               medians: the first in order, as `median < BestMedian` has it.
 * All five output arrays may be NULL; rows whose status bit is clear are not written.  With m != NULL the updated halves go into the
 * table's slots (table_slot[i], or point[i] when table_slot is NULL) on the device, with no host round trip between the compute and the
 * write, and the table's "given" bitmap follows; a half whose status bit is clear stays byte for byte as it was.
 * The arithmetic is fixed, float unless a step says double, every operation rounded on its own (no fused multiply-add), division and
 * square root correctly rounded:
 *   1. per entry k in order: d = P - Ow_k per component; nrm = sqrt(((double)dx*dx + (double)dy*dy) + (double)dz*dz); inv = 1.0 / nrm in
 *      double; normal_c = normal_c + (float)((double)d_c * inv), from normal = 0
 *   2. mNormalVector_c = (float)((double)normal_c * (1.0 / (double)N)), N = the entries of the row
 *   3. dist = (float)sqrt(...) of P - Ow_ref as in step 1; mfMaxDistance = dist * scale_factors[octave(ref_kf, ref feature)];
 *      mfMinDistance = mfMaxDistance / scale_factors[nlevels - 1]
 *   4. the descriptor as orbx_distinctive_descriptors: the Hamming matrix of the entries that take part, per row the median
 *      sorted[(int)(0.5 * (N - 1))], the first row with the smallest
 * A zero distance gives the IEEE result (NaN or infinity), as in the reference.  Against OpenCV's own cv::Mat expression arithmetic this
 * restatement is unpinned.
 * Every refusal is decided on the graph's host mirror and the table's host state before any device work and leaves the graph, the table
 * and the outputs unchanged.  ORBX_E_INVALID: `what` outside {1, 2, 3}; a negative slot or a slot listed twice (point, table_slot,
 * kf_slot); a live, not-bad listed point whose row names a keyframe that is not in kf_slot; with GEOM, for such a point with a row, a
 * ref_kf that is not listed or not in use, a reference feature outside the keyframe or of an octave >= nlevels, nlevels outside [1, 32],
 * and pos == NULL while the table never got that slot's geometry (or without a table); with DESC, a keyframe with kf_bad == 0 in such a
 * row whose kf_frame is NULL or has no feature of the entry's index; the graph, the table and the frames on different devices.  (GEOM
 * alone into a table slot that never had a descriptor is fine, as is the converse.)  ORBX_E_CAPACITY: a slot beyond its capacity.
 * n == 0: ORBX_OK, no launch.  "Unchanged" covers these refusals (ORBX_E_INVALID, ORBX_E_CAPACITY) only: ORBX_E_HIP -- a failing HIP
 * call behind the launch, or a device status that differs from the one the mirror predicted -- is returned with the table possibly
 * written and its "given" bits set, as a failing orbx_mappoints_set leaves it.
 * One packed upload (the points, pos, ref_kf, scale_factors and a keyframe table indexed by slot: centre, bad, descriptor base, n), one
 * launch of k_mp_refresh (a wave per point), one group of downloads -- only the arrays asked for -- behind one synchronisation, on
 * `stream` (NULL: the calling thread's own).  The graph serialises as for every call; the table is held as orbx_mappoints_set holds it
 * and its event is recorded; frames still pending are waited for through their events. */
#define ORBX_REFRESH_GEOM 1   /* UpdateNormalAndDepth */
#define ORBX_REFRESH_DESC 2   /* ComputeDistinctiveDescriptors */
typedef struct {
    int what;                          /* a non-empty OR of the two */
    /* the points */
    int n; const int32_t *point;       /* graph point slots, each at most once */
    const int32_t *table_slot;         /* [n] slots of `m`; NULL: the same numbers as point[] */
    const float *pos;                  /* [n][3] mWorldPos; NULL: X Y Z as the table holds them */
    const int32_t *ref_kf;             /* [n] keyframe slot of mpRefKF (GEOM only) */
    /* every keyframe that a row of a listed point may name, and every ref_kf */
    int nk; const int32_t *kf_slot;    /* each at most once */
    const float *kf_centre;            /* [nk][3] GetCameraCenter() */
    const uint8_t *kf_bad;             /* [nk] KeyFrame::isBad() */
    const orbx_frame *const *kf_frame; /* [nk] resident descriptors; needed for DESC on a keyframe that is not bad, else may be NULL */
    const float *scale_factors; int nlevels;   /* mvScaleFactors, mnScaleLevels (GEOM) */
} orbx_refresh_job;
int orbx_mapgraph_refresh_points(orbx_mapgraph *g, orbx_mappoints *m /* may be NULL */, const orbx_refresh_job *job,
                                 uint8_t *status, float *geom, int32_t *best_kf, int32_t *best_idx, uint8_t *desc, void *stream);

/* ---- Optimizer::PoseOptimization: motion-only pose optimisation (src/Optimizer.cc:286-513) ---------------------------
 * The one per-frame step of Tracking that g2o solved on a host core (TrackWithMotionModel, TrackReferenceKeyFrame, TrackLocalMap;
 * Relocalization up to three times per candidate, src/Tracking.cc:1730-1800): one 6-DoF vertex, one unary edge per feature that
 * holds a map point.  The whole function -- four rounds of at most ten Levenberg iterations with at most ten damping trials each,
 * and the inlier / outlier classification between the rounds -- is ONE kernel launch, one workgroup per job.  Only this function:
 * the other functions of src/Optimizer.cc have calls of their own below (orbx_local_bundle_adjustment, orbx_bundle_adjustment,
 * orbx_sim3_optimize, orbx_optimize_essential_graph).
 * The arithmetic, in double unless a step says float, every operation rounded on its own (no fused multiply-add):
 *   edges    feature i with has_point[i] is a monocular edge (src/Optimizer.cc:335-377) if u_right[i] < 0, else a stereo edge
 *            (:378-416).  Measurement, Xw, cam and inv_sigma2 are floats widened to double; information = inv_sigma2[i] * I.
 *   start    Converter::toSE3Quat(mTcw): the float rotation block goes to a quaternion (Eigen's Quaternion(Matrix3)), w >= 0,
 *            normalised -- it is never used as a matrix.  EVERY round restarts from this pose (:437).
 *   error    measurement - projection of Pc = q * Xw + t.  Monocular: (Pc.x / Pc.z) * fx + cx, likewise y.  Stereo: invz =
 *            (double)(float)(1.0 / Pc.z) (types_six_dof_expmap.cpp:300 keeps it in a float), u = (Pc.x * invz) * fx + cx, v
 *            likewise, third row u - mbf * invz.  chi2 = sum_r e_r * (inv_sigma2 * e_r).
 *   Jacobian types_six_dof_expmap.cpp:266-288 / :335-364, with the double 1.0 / Pc.z also for the stereo edge.
 *   Huber    delta = (float)sqrt(5.991) / (float)sqrt(7.815), robust_kernel_impl.cpp:78-91; b -= rho1 * A^T (w e),
 *            H += A^T (rho1 w) A (base_unary_edge.hpp:56-66).  The active robust chi2 sums rho0, or chi2 in the fourth round.
 *   system   21 + 6 + 1 sums over the active edges.  The summation order is a fixed function of (n, thread index): results are
 *            bit-reproducible from run to run and do not depend on the other jobs of a launch.  No atomics.
 *   solve    (H + lambda I) x = b by LDL^T without pivoting; a pivot <= 0 makes the trial's chi2 DBL_MAX (linear_solver_dense.h).
 *   update   pose = SE3Quat::exp(x) * pose, x[0..2] rotation, x[3..5] translation, with the theta < 1e-5 branch of se3quat.h:237
 *            and the quaternion re-normalised after the product.
 *   Levenberg optimization_algorithm_levenberg.cpp:61-189: lambda = 1e-5 * max |H_jj| at iteration 0 of every round; rho = (cur -
 *            temp) / (sum_j x_j (lambda x_j + b_j) + 1e-3); accept on rho > 0 && isfinite(temp) with lambda *= clamp(1 - (2 rho -
 *            1)^3, 1/3, 2/3), else lambda *= ni, ni *= 2; at most 10 trials; the iteration loop ends on 10 trials, on rho == 0 or
 *            when (iniChi - currentChi) * 1e3 < iniChi held three times in a row.
 *   rounds   after a round (:441-502) an edge flagged outlier gets a fresh error at the round's final pose, an active edge keeps
 *            the error of the LAST EVALUATED TRIAL -- after a rejected last trial that is the rejected pose (g2o's pop() restores
 *            the vertex, not the edge errors).  outlier = (float)chi2 > 5.991f (monocular) / 7.815f (stereo); outliers leave the next
 *            round's system; after the third round the Huber kernels go; with fewer than 10 edges (all, not only active ones)
 *            there is one round only.
 *   result   Converter::toCvMat(SE3Quat): the quaternion to a rotation matrix, [R | t] cast to float, last row 0 0 0 1.
 * Fewer than 3 correspondences (:423-424): the return value is 0, Tcw_out is Tcw bit for bit, the flags are 0.
 * Outside the contract: a correspondence whose projection is not finite at a pose the solver visits (Pc.z == 0, NaN inputs).  A
 * finite point behind the camera is inside it (it projects mirrored, as in the reference, and normally ends as an outlier).
 * Against g2o's own arithmetic (Eigen's LDLT pivots, its product evaluation order) this restatement is unpinned: DESIGN.md. */
typedef struct {
    int n;                     /* Frame::N, 0 .. 65535 */
    const float *x, *y;        /* mvKeysUn[i].pt */
    const float *u_right;      /* mvuRight[i] */
    const float *inv_sigma2;   /* mvInvLevelSigma2[mvKeysUn[i].octave] */
    const float *Xw;           /* [n][3] pMP->GetWorldPos(); read only where has_point[i] */
    const uint8_t *has_point;  /* mvpMapPoints[i] != NULL */
} orbx_pose_obs;
typedef struct {
    int n_corr;                /* nInitialCorrespondences */
    int rounds;                /* rounds run: 0 (fewer than 3 correspondences), 1 (fewer than 10) or 4 */
    int n_bad[4];              /* nBad after each round */
    int iterations[4];         /* Levenberg iterations of each round */
    double chi2[4];            /* the active robust chi2 each round ended with */
    double pose[12];           /* the final [R | t], row major, in double: Tcw_out is exactly its float cast */
} orbx_pose_report;
/* cam = fx fy cx cy mbf; Tcw / Tcw_out = 16 floats, row major (may alias).  outlier[n] = mvbOutlier, written only where
 * has_point[i]; *n_inliers = the reference's return value, nInitialCorrespondences - nBad; report may be NULL.  One upload, one
 * launch, one download.  ORBX_E_INVALID before any device work: NULL obs / cam / Tcw / Tcw_out / n_inliers, n outside [0, 65535],
 * with n > 0 a NULL array of obs or NULL outlier. */
int orbx_pose_optimize(int device, const orbx_pose_obs *obs, const float *cam, const float *Tcw, float *Tcw_out, uint8_t *outlier,
                       int *n_inliers, orbx_pose_report *report);
/* one job of a batch: the arguments of orbx_pose_optimize */
typedef struct {
    const orbx_pose_obs *obs; const float *cam, *Tcw;
    float *Tcw_out; uint8_t *outlier;
    int n_inliers;                               /* out */
    orbx_pose_report *report;                    /* out, may be NULL */
} orbx_pose_job;
/* njobs optimisations (Relocalization's candidates; a server tracking many streams) as ONE upload, ONE launch of njobs
 * workgroups, ONE download; every job's results are byte-equal to its single call.  ORBX_E_INVALID: njobs outside [1, 1024], any
 * refusal of the single call in any job; ORBX_E_CAPACITY: more than 2^22 features in all. */
int orbx_pose_optimize_batch(int device, orbx_pose_job *jobs, int njobs);
/* On a resident frame and a resident map-point table: slot_of_feature[cur n] names each feature's point (-1: none); positions,
 * octaves and u_right are read from the frame, Xw from the table (geom[0..2]), inv_sigma2 = inv_level_sigma2[octave].  Up go n
 * int32 slots and the pose, back come n flag bytes and the pose; results are byte-equal to orbx_pose_optimize on the same
 * values.  The call is ordered behind a pending orbx_mappoints_set or frame creation through the events the handles keep; both
 * handles are only read (several threads may optimise on one frame and one table).  ORBX_E_INVALID before any device work: the
 * refusals of orbx_pose_optimize; a slot >= capacity or < -1, or not set; a frame and a table on different devices; nlevels
 * outside [1, 16]; a feature with a point whose octave is outside [0, nlevels).  (The octaves of a frame made by
 * orbx_frame_create_from_extraction exist on the device only: for such a frame the kernel makes that last check before it
 * optimises, writes nothing, and the call returns ORBX_E_INVALID after its one launch.) */
int orbx_frame_pose_optimize(const orbx_frame *cur, const orbx_mappoints *m, const int32_t *slot_of_feature,
                             const float *inv_level_sigma2, int nlevels, const float *cam, const float *Tcw, float *Tcw_out,
                             uint8_t *outlier, int *n_inliers, orbx_pose_report *report);

/* ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:528-862; LocalMapping::Run) ---------
 * The optimisation of the local window behind SearchInNeighbors, which g2o solved on one host core per inserted keyframe: 6-DoF
 * vertices for the local and the fixed keyframes, marginalised 3-D vertices for the local points, one binary edge per observation.
 * Everything between :584 (the optimizer's set-up) and :825 (vToErase) is this call; the three lists before it and the map update
 * behind it stay with the adaptor (adapter/lba/LocalBundleAdjustment.cc).  The host drives the Levenberg loop and polls the stop flag;
 * a linearisation and a damping trial are short chains of launches (orbx_lba.hip), with one small status record read back after each.
 * The arithmetic, in double unless a step says float, every operation rounded on its own (no fused multiply-add):
 *   start    Converter::toSE3Quat(GetPose()) per keyframe as in orbx_pose_optimize: the float rotation block to a quaternion, w >= 0,
 *            normalised.  Tcw_out of a FIXED keyframe is that quaternion turned back into a matrix and cast to float (:847-850 calls
 *            SetPose with exactly that for the keyframe with mnId == 0); its bits can differ from the input.  Points: Xw widened.
 *   edges    edge e joins point edge_point[e] (vertex 0) and keyframe edge_kf[e] (vertex 1); monocular (EdgeSE3ProjectXYZ, :675-701)
 *            if u_right[e] < 0, else stereo (EdgeStereoSE3ProjectXYZ, :702-731).  Information = inv_sigma2[e] * I.  Error =
 *            measurement - projection of Pc = q * X + t: monocular (Pc.x / Pc.z) * fx + cx, likewise y; stereo invz =
 *            (double)(float)(1.0 / Pc.z) (types_six_dof_expmap.cpp:151), u = (Pc.x * invz) * fx + cx, v likewise, third row
 *            u - mbf * invz.  chi2 = sum_r e_r * (inv_sigma2 * e_r).
 *   Jacobians linearizeOplus (types_six_dof_expmap.cpp:103-139, :188-234), as written there (x*y/z_2 *fx, -1./z *fx, ...), with
 *            R = the quaternion's rotation matrix.  _jacobianOplusXj is the 2/3 x 6 pose block Jp.  _jacobianOplusXi is the 2/3 x 3 point
 *            block Jl: stereo entry by entry as :202-212; monocular (-1./z * tmp) * R with every sum ((t_i0 R_0c + t_i1 R_1c) + t_i2 R_2c),
 *            the zero entries of tmp included.
 *   Huber    delta = (float)sqrt(5.991) / (float)sqrt(7.815) (:650-651), robust_kernel_impl.cpp:78-91, in round 1 only.
 *   quadratic form  base_binary_edge.hpp constructQuadraticForm: omega_r = -(inv_sigma2 e) * rho1; rw = rho1 * inv_sigma2 (rho2 is
 *            ignored); per edge  Hll += Jl^T rw Jl, bl += Jl^T omega_r, and for a free keyframe  Hpp += Jp^T rw Jp, bp += Jp^T omega_r,
 *            W = Jp^T rw Jl (6 x 3).  An entry of such a product is ((a_0 rw) b_0 + (a_1 rw) b_1) + (a_2 rw) b_2 over the edge's rows (two
 *            for a monocular edge's non-zero rows; the third adds an exact zero).  No pose block and no b for a fixed keyframe.
 *   system   per point, Hll and bl are summed over the point's active edges one after the other in edge order: that fixes them bit for
 *            bit.  Per free keyframe, Hpp and bp are summed over its active edges, taken in point order, in a fixed order that is a function
 *            of their count only.  setLambda adds lambda to the diagonals of every Hpp and every Hll block.  Dinv = (Hll + lambda I)^-1 is
 *            the closed 3 x 3 cofactor inverse (Eigen's fixed-size inverse(): determinant along the first column), no singularity test.
 *            S = Hpp + lambda I - sum_points sum_{i<=j} (W_i Dinv) W_j^T, b_S = bp - sum W_i (Dinv bl) (block_solver.hpp:372-439), the sums
 *            in a fixed order; rows and columns of S are the active free keyframes in keyframe order.
 *   solve    S x_p = b_S by a dense LDL^T without pivoting on the lower triangle (the mirror image of what the sums give for the upper one),
 *            column by column: l_ij = s_ij / d_j, then s_ik -= (l_ij l_kj) d_j for i >= k > j; forward substitution y_i -= l_ij y_j in
 *            ascending j, y_i / d_i, backward substitution x_i -= l_ji x_j in descending j.  A pivot <= 0 makes the trial's chi2 DBL_MAX
 *            and leaves x as the previous trial left it (0 at the start).  THIS DENSE SOLVE IS THE STATED DEVIATION: g2o factors the same
 *            matrix with Eigen's sparse SimplicialLDLT under an AMD ordering -- the same solution, with different rounding.
 *            x_l = Dinv (bl - sum_edges W^T x_p), the edges of the point in order.
 *   update   pose = SE3Quat::exp(x) * pose as in orbx_pose_optimize; point += x_l.
 *   Levenberg optimization_algorithm_levenberg.cpp:61-189 as restated for orbx_pose_optimize.  computeLambdaInit takes the maximum over
 *            the diagonals of ALL active vertices, poses and points; computeScale runs over the whole x and b (bp and bl, not b_S), poses
 *            first, in a fixed order; ni and lambda are set anew at iteration 0 of each round; at most 10 trials per iteration; the
 *            _nBad >= 3 stop and the rho == 0 stop are kept.  The active robust chi2 sums, in a fixed order over the points, each point's
 *            sum of rho0 (chi2 in round 2) over its active edges in edge order.
 *   rounds   (:740-825) round 1 = optimize(5) on all edges with Huber.  The classification sets level 1 where chi2 > 5.991 (7.815
 *            stereo) or isDepthPositive fails, and removes every kernel.  initializeOptimization(0): a point with no level-0 edge, or a
 *            free keyframe with no level-0 edge, leaves the active set and keeps its estimate; it has no row in the system and no share
 *            in lambdaInit.  Round 2 = optimize(10) without a kernel; a round with no active edge does nothing (optimize returns -1).
 *            The final check marks vToErase by the same test.  An active edge's chi2() is that of the LAST EVALUATED TRIAL -- after a
 *            rejected last trial that is the rejected state (the pose-optimisation rule).  A level-1 edge is never re-evaluated in round 2:
 *            in the final check it still carries its round-1 error.  isDepthPositive() (Pc.z > 0) is always evaluated at the current,
 *            restored estimates.  The thresholds compare as the reference's doubles do, chi2 > 5.991: no float cast here, unlike
 *            PoseOptimization.
 *   stop     *stop (mbAbortBA) is read on entry (:736), before every iteration and between trials (terminate()), and after round 1
 *            (:745).  debug_stop_at_trial = t behaves as if the flag rose when the running count of trials (both rounds) reaches t; it
 *            exists so that the bDoMore = false path is testable, an adaptor never sets it.  stopped = 2: round 2 is skipped; bit 0 of
 *            the flags then holds the test the skipped classification would have made (the reference sets no level there), and bit 1
 *            equals it.  Stated deviation: if the stop comes before any evaluation, the errors are those at the start estimates (the
 *            reference would read uninitialised memory there).
 *   result   pose_out = [R | t] of the final quaternion, point_out the final points, in double; Tcw_out and Xw_out are their
 *            Converter::toCvMat float casts (last row 0 0 0 1).  A point without edges returns Xw bit for bit.
 * A call is byte-reproducible: no atomics, every reduction in a fixed order.  iterations / trials near convergence hang on the sign of
 * rounding noise and are reported, not promised.  Outside the contract: a projection that is not finite at a state the solver visits.
 * Against g2o's own arithmetic (SimplicialLDLT, Eigen's product evaluation order) this restatement is unpinned: DESIGN.md. */
typedef struct {
    int n_kf;                       /* local + fixed keyframes, 1 .. 1024; at most 256 with fixed[k] == 0 */
    const float *Tcw;               /* [n_kf][16] GetPose(), row major */
    const float *cam;               /* [n_kf][5] fx fy cx cy mbf */
    const uint8_t *fixed;           /* [n_kf]: lFixedCameras, and the keyframe with mnId == 0 */
    int n_points;                   /* 0 .. 2^20 */
    const float *Xw;                /* [n_points][3] GetWorldPos() */
    int n_edges;                    /* 0 .. 2^22; edges of one point are contiguous, points ascending */
    const int32_t *edge_kf, *edge_point;
    const float *x, *y, *u_right, *inv_sigma2;   /* mvKeysUn[idx].pt, mvuRight[idx] (< 0: monocular edge), mvInvLevelSigma2[octave] */
} orbx_lba_problem;
typedef struct { const volatile unsigned char *stop; int debug_stop_at_trial; } orbx_lba_options;   /* NULL / -1: never */
typedef struct {
    int stopped;                    /* 0 no, 1 on entry (nothing written), 2 in round 1 (round 2 skipped), 3 in round 2 */
    int iterations[2], trials[2];   /* Levenberg iterations / damping trials of optimize(5) and optimize(10) */
    int n_level1, n_erase;          /* edges set to level 1 after round 1; edges in vToErase */
    int n_active_kf[2], n_active_points[2];
    double chi2[2], lambda[2];      /* active robust chi2 and lambda each round ended with */
} orbx_lba_report;
/* One upload in front, one download behind; the device buffers are the calling thread's (orbx_thread_release).  Refusals before any
 * device work.  ORBX_E_INVALID: a NULL argument or array that the sizes need (opt, pose_out, point_out, report may be NULL; Xw_out with
 * n_points == 0 and edge_flags with n_edges == 0 too), n_kf < 1 or a negative size, an index out of range, edges of a point not
 * contiguous or points not ascending, more than one edge between a point and a keyframe.  ORBX_E_CAPACITY: n_kf > 1024, n_points >
 * 2^20, n_edges > 2^22, more than 256 keyframes with fixed[k] == 0.  stopped == 1: nothing but the report is written.
 * The limits say what the buffers hold, not what runs well: the reduced system (6 x the free keyframes) is factored by one workgroup,
 * which suits the tens of free keyframes of a covisibility window; at 256 a trial costs on the order of 0.1 s. */
int orbx_local_bundle_adjustment(int device, const orbx_lba_problem *p, const orbx_lba_options *opt /* may be NULL */,
                                 float *Tcw_out /* [n_kf][16] */, float *Xw_out /* [n_points][3] */,
                                 uint8_t *edge_flags /* [n_edges]: bit 0 level 1 after round 1, bit 1 in vToErase */,
                                 double *pose_out /* [n_kf][12], may be NULL */, double *point_out /* [n_points][3], may be NULL */,
                                 orbx_lba_report *report /* may be NULL */);

/* ---- Optimizer::BundleAdjustment (src/Optimizer.cc:48-281; Tracking::CreateInitialMapMonocular, LoopClosing::RunGlobalBundleAdjustment) ----
 * The global bundle adjustment over a whole map: everything between :67 (the optimiser's set-up) and :232 (the recovery loops) is this
 * call; the two lists in front and the recovery behind stay with the adaptor (adapter/ba/BundleAdjustment.cc).  It takes the problem of
 * orbx_local_bundle_adjustment, and its start, edges, Jacobians, quadratic form, system, solve, update, Levenberg rules and result are that
 * contract's, operation for operation (the block above; not repeated here).  What differs:
 *   rounds   ONE round, optimize(iterations), on every edge.  robust != 0: Huber on every edge throughout, with thHuber2D =
 *            (float)sqrt(5.99) for a monocular edge (:101 -- not LocalBundleAdjustment's 5.991) and thHuber3D = (float)sqrt(7.815) for a
 *            stereo one; robust == 0: no kernel.  No classification, no levels: every edge is active for the whole call, and there are
 *            no edge flags.
 *   vertices a point without an edge is not a vertex (:215-219, vbNotIncludedMP): point_included = 0 and Xw_out = Xw bit for bit.  A free
 *            keyframe without an edge has no row in the system and keeps its estimate (through the quaternion round trip, like a fixed one).
 *   solve    the same dense LDL^T with the same per-entry operation order, computed in panels over many workgroups (orbx_ldlt.hip), so the
 *            bytes of x are those the one-workgroup kernel of orbx_local_bundle_adjustment would give.
 *   stop     there is no return on entry: the reference only hands the flag to setForceStopFlag (:64-65).  With *stop up on entry no
 *            iteration runs and the outputs are the start estimates through the quaternion round trip, stopped = 1.  After that the flag is
 *            polled before every iteration and between trials as in orbx_local_bundle_adjustment; stopped = 2 if it is up when the round
 *            ends.  debug_stop_at_trial as there.
 *   sizes    n_kf <= 4096, at most 2048 keyframes with fixed == 0, n_points <= 2^20, n_edges <= 2^22.  The reduced system is dense:
 *            8 (6 F)^2 bytes for F free keyframes with an edge, 1.2 GB at 2048 (the thread's work area grows to twice its largest request).
 * opt == NULL: no flag, 10 iterations, robust.  Refusals before any device work: ORBX_E_INVALID as for orbx_local_bundle_adjustment
 * (point_included is needed when n_points > 0), and for iterations < 0; ORBX_E_CAPACITY beyond a size above. */
typedef struct { const volatile unsigned char *stop; int debug_stop_at_trial; int iterations; int robust; } orbx_ba_options;
typedef struct {
    int stopped;                    /* 0 no, 1 the flag was up on entry (no iteration), 2 it rose during the round */
    int iterations, trials;
    int n_active_kf, n_active_points;   /* rows of the reduced system / 6; points with an edge */
    double chi2, lambda, lambda_init;   /* active (robust) chi2 and lambda at the end, computeLambdaInit's value; 0 if no iteration ran */
} orbx_ba_report;
int orbx_bundle_adjustment(int device, const orbx_lba_problem *p, const orbx_ba_options *opt /* may be NULL */,
                           float *Tcw_out /* [n_kf][16] */, float *Xw_out /* [n_points][3] */,
                           uint8_t *point_included /* [n_points]: 0 = no edge, vbNotIncludedMP */,
                           double *pose_out /* [n_kf][12], may be NULL */, double *point_out /* [n_points][3], may be NULL */,
                           orbx_ba_report *report /* may be NULL */);

/* ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:885-1153; LoopClosing::CorrectLoop) ----------------------------------
 * The pose graph over the essential graph behind a loop closure, between ComputeSim3 and the global bundle adjustment: one 7-DoF
 * VertexSim3Expmap per good keyframe (pLoopKF fixed), binary EdgeSim3 edges, no points; then the correction of every map point by its
 * reference keyframe.  Graph selection stays with the adaptor (adapter/essential/OptimizeEssentialGraph.cc): GetWeight < minFeat, parents,
 * GetLoopEdges, GetCovisiblesByWeight, sInsertedEdges walk KeyFrame pointers.  Everything arithmetic is this call, in double, every
 * operation rounded on its own (no fused multiply-add), a Sim3 as qx qy qz qw tx ty tz s with the quaternion NEVER normalised:
 *   vScw     vScw[k] = S_corrected[corrected[k]] where corrected[k] >= 0 (:923-929), else Sim3(Matrix3d(Rcw), tcw, 1.0) of the float pose
 *            (:933-937): Eigen's Quaternion(Matrix3) on the doubles of the floats, not normalised (sim3.h:64-67).  It is the start estimate.
 *   edges    edge e joins vertex 0 = edge_i[e] and vertex 1 = edge_j[e] with the measurement Sji = Sjw * Swi, Swi = Siw.inverse()
 *            (sim3.h:233-236, :266-272).  edge_kind 0 (:958-989): Siw = vScw[i], Sjw = vScw[j].  edge_kind 1 (:992-1092): each end's
 *            S_noncorrected[noncorrected[.]] where it has one, else its vScw.  information = I, no robust kernel.
 *   error    log(C * Si * Sj^-1) = ((C * Si) * Sj.inverse()).log() (types_seven_dof_expmap.h:106-114).  Sim3::log (sim3.h:148-230): sigma =
 *            log(s); R = r.toRotationMatrix() of the quaternion as it stands; d = 0.5 * (((R00 + R11) + R22) - 1); eps = 1e-5; the four
 *            branches on fabs(sigma) < eps and d > 1 - eps, omega = 0.5 deltaR(R) or acos(d) / (2 sqrt(1 - d d)) deltaR(R), A B C as the
 *            text has them; W = (A Omega + (B Omega) Omega) + C I with B Omega rounded first and each product entry summed (p0 + p1) + p2;
 *            upsilon = W.lu().solve(t): Eigen's 3 x 3 PartialPivLU -- in column k the FIRST row >= k of the largest magnitude is the pivot,
 *            rows exchanged, the entries below divided by the pivot (a division, not a product with its reciprocal), the trailing block
 *            updated entry by entry; forward y1 = t1 - l10 y0, y2 = t2 - (l20 y0 + l21 y1); backward x2 = y2 / u22, x1 = (y1 - u12 x2) /
 *            u11, x0 = (y0 - (u01 x1 + u02 x2)) / u00.  chi2 of an edge = ((((((e0 e0 + e1 e1) + e2 e2) + e3 e3) + e4 e4) + e5 e5) + e6 e6.
 *   jacobian base_binary_edge.hpp:131-205 for each end that is not fixed: column d = (1 / (2 delta)) * (e(+delta) - e(-delta)), delta = 1e-9,
 *            the end's estimate replaced by Sim3(+-delta e_d) * estimate (VertexSim3Expmap::oplusImpl); with fix_scale oplusImpl zeroes
 *            update[6], both sides of column 6 are the same evaluation and the column is an exact zero.  The 14 transforms Sim3(+-delta
 *            e_d) do not depend on the vertex and are computed once per call.
 *   system   constructQuadraticForm (:55-120) without a kernel: for a free vertex 0, b_i += A^T (-e), H_ii += A^T A; for a free vertex 1
 *            likewise with B; both free: the pair's off-diagonal block += A^T B, read transposed where the row order asks for it.  A
 *            product entry is the sum over the 7 error rows in ascending order.  FIXED ORDERS: a vertex's H_ii and b are summed over its
 *            incident edges in edge order; a pair's block over that pair's edges in edge order (several edges may join one pair; g2o maps
 *            them to one block); chi2 = the edges strided over 256 partial sums (edge e to partial e % 256, ascending), the partials summed
 *            by a butterfly over 64 and ((w0 + w1) + (w2 + w3)) -- a function of n_edges alone.  Rows: the free keyframes in keyframe order.
 *   damping  optimization_algorithm_levenberg.cpp:61-189 as in orbx_local_bundle_adjustment, with setUserLambdaInit(1e-16) (:899):
 *            computeLambdaInit returns 1e-16, not 1e-5 * the largest diagonal entry.  setLambda adds lambda to every diagonal entry;
 *            computeScale = sum of x_j (lambda x_j + b_j) over the whole x, per vertex in ascending j, the vertices' sums in the chi2 order,
 *            after oplus has zeroed x[6] of every vertex under fix_scale; rho = (chi2 - trial chi2) / (scale + 1e-3); the qmax == 10,
 *            rho == 0 and _nBad >= 3 stops.  The function has no stop flag, and neither has this call.
 *   solve    the dense 7F x 7F matrix zeroed, its lower triangle filled, factored by the panel LDL^T of orbx_bundle_adjustment
 *            (orbx_ldlt.hip).  A pivot that is not > 0: the trial's chi2 is DBL_MAX and x is what the previous trial left (0 at the start).
 *            THIS DENSE SOLVE IS THE STATED DEVIATION, the bundle adjustments' own: g2o solves the same matrix with Eigen's sparse Cholesky;
 *            the same solution, other rounding.  A vertex without an edge has the block lambda I and b = 0, hence x = 0 and exp(0) * S = S
 *            bit for bit; under fix_scale every scale row has the pivot lambda and x = 0.
 *   update   trial estimate = Sim3(x_k) * S_k (sim3.h:70-142).
 *   result   (:1101-1152) S_out[k] = the final estimate; Tcw_out[k] = [R | t * (1. / s)], R = rotation().toRotationMatrix(), cast to float
 *            as Converter::toCvSE3 does, last row 0 0 0 1; the fixed keyframe goes through the same recovery.  point_out[p] =
 *            S_out[ref].inverse().map(vScw[ref].map(Xw[p])), ref = point_ref[p]; Xw_out = its float cast.
 * sizes: n_kf 1 .. 4096 with EXACTLY ONE fixed[k] != 0 and at most 1536 free; n_edges 0 .. 2^18; n_points 0 .. 2^20; n_corrected and
 * n_noncorrected 0 .. 4096.  1536 is the round
 * number below the 1755 that the panel solver's n <= 12288 allows; the dense matrix is 0.92 GB there (the thread's work area grows to
 * twice its largest request).  The limits say what the buffers hold, not what runs well: the factorisation is dense and dominates above
 * a few hundred keyframes.  A call is byte-reproducible: no atomics, no cooperative launch.
 * opt == NULL: 20 iterations (:1096).  One upload in front, one download behind; the device buffers are the calling thread's.  Refusals
 * before any device work.  ORBX_E_INVALID: a NULL argument or array that the sizes need (opt, S_out, point_out, report may be NULL; Xw_out
 * with n_points == 0 too; S_corrected / S_noncorrected where no index names them), n_kf < 1 or a negative size, an index out of range
 * (edge_i, edge_j, point_ref; corrected / noncorrected below -1), edge_i == edge_j, edge_kind above 1, not exactly one fixed keyframe,
 * iterations < 0.  ORBX_E_CAPACITY: a size beyond those above.
 * Against g2o's own arithmetic (Eigen's sparse Cholesky, its product evaluation order, the PartialPivLU of the Eigen version at hand)
 * this restatement is unpinned: DESIGN.md. */
typedef struct {
    int n_kf;                       /* good keyframes of the map, 1 .. 4096; exactly one with fixed[k] != 0 (pLoopKF); at most 1536 free */
    const float *Tcw;               /* [n_kf][16] GetPose(), row major */
    const uint8_t *fixed;           /* [n_kf] */
    const int32_t *corrected;       /* [n_kf] index into S_corrected or -1 (CorrectedSim3.find) */
    const int32_t *noncorrected;    /* [n_kf] index into S_noncorrected or -1 (NonCorrectedSim3.find) */
    int n_corrected, n_noncorrected;   /* entries of the two arrays below */
    const double *S_corrected, *S_noncorrected;   /* [.][8] qx qy qz qw tx ty tz s */
    int n_edges;                    /* 0 .. 2^18 */
    const int32_t *edge_i, *edge_j; /* vertex 0 and vertex 1 of the EdgeSim3, i != j */
    const uint8_t *edge_kind;       /* 0: loop-connection edge (:958-989), 1: normal edge (:992-1092) */
    int n_points;                   /* 0 .. 2^20 */
    const float *Xw;                /* [n_points][3] GetWorldPos() */
    const int32_t *point_ref;       /* [n_points] nIDr's keyframe index (:1129-1138) */
    int fix_scale;
} orbx_eg_problem;
typedef struct { int iterations; } orbx_eg_options;
typedef struct {
    int iterations, trials, n_free, n_solve_failed;
    double chi2_start, chi2, lambda;   /* chi2 at the start estimates and at the end, lambda at the end; 0 if no iteration ran */
} orbx_eg_report;
int orbx_optimize_essential_graph(int device, const orbx_eg_problem *p, const orbx_eg_options *opt /* may be NULL */,
                                  float *Tcw_out /* [n_kf][16] */, float *Xw_out /* [n_points][3] */,
                                  double *S_out /* [n_kf][8], may be NULL */, double *point_out /* [n_points][3], may be NULL */,
                                  orbx_eg_report *report /* may be NULL */);

/* ---- the same call for large maps: the system as an ENVELOPE, 4095 free keyframes ---------------------------------------
 * orbx_optimize_essential_graph2 is orbx_optimize_essential_graph with a choice of the solve.  Everything above holds but "solve" and the
 * sizes.  opt->solver:
 *   ORBX_EG_SOLVER_DENSE     the call above: the same launches, the same bytes, the same sizes and refusals.
 *   ORBX_EG_SOLVER_ENVELOPE  the lower triangle is stored and factored as an envelope (skyline), rows in keyframe order as before.  The
 *            envelope rule: the 7 rows of free keyframe r start at column 7 x (the smallest row r shares an edge with; r itself where
 *            there is none), rounded down to a multiple of 32, the solver's panel width; row i holds its columns from there to i, the
 *            rows one behind the other.  Only the envelope is zeroed and filled; every block of the system lies inside it.  The
 *            factorisation (orbx_ldlt_env.hip) is the panel LDL^T on those entries: THE SAME OPERATIONS IN THE SAME ORDER AS THE DENSE
 *            SOLVE, MINUS TERMS THAT ARE AN EXACT ZERO -- a factorisation in this row order fills nothing to the left of a row's first
 *            entry, so what is left out are x - (l * 0) * d with l an entry the dense solve holds as 0.  The values are the dense
 *            solve's; a -0 that the dense solve's x - (+-0) turns into +0 can stay a -0, which no later operation tells apart unless
 *            it is divided by.  No reordering: the stated deviation from g2o does not grow, and the call stays byte-reproducible.
 *            The cost follows the keyframe order: narrow where a keyframe's edges go to recent neighbours (creation order; the loop's
 *            few long edges cost their rows only), the whole triangle for a shuffled list.  orbx_eg_envelope tells in advance.
 *   ORBX_EG_SOLVER_AUTO      ENVELOPE where more than 1536 keyframes are free or the envelope holds at most half of the triangle's
 *            entries, else DENSE.  opt == NULL: 20 iterations, AUTO.
 * sizes: DENSE as above.  ENVELOPE and AUTO: n_kf 1 .. 4096, so up to 4095 free; the envelope at most ORBX_EG_MAX_ENVELOPE = 2^27 doubles
 * (1 GiB, about the dense matrix at its limit); the other sizes as above.  Refusals before any device work, as above, and: ORBX_E_INVALID
 * for a solver that is none of the three; ORBX_E_CAPACITY for an envelope beyond the limit, the message naming its size and the limit. */
#define ORBX_EG_SOLVER_DENSE 0
#define ORBX_EG_SOLVER_ENVELOPE 1
#define ORBX_EG_SOLVER_AUTO 2
#define ORBX_EG_MAX_ENVELOPE ((int64_t)1 << 27)
typedef struct { int iterations; int solver; } orbx_eg_options2;
int orbx_optimize_essential_graph2(int device, const orbx_eg_problem *p, const orbx_eg_options2 *opt /* may be NULL */,
                                   float *Tcw_out /* [n_kf][16] */, float *Xw_out /* [n_points][3] */,
                                   double *S_out /* [n_kf][8], may be NULL */, double *point_out /* [n_points][3], may be NULL */,
                                   orbx_eg_report *report /* may be NULL */);
/* what a keyframe order costs: *entries = the doubles of the envelope of p's system by the rule above, *triangle = those of its whole
 * lower triangle, n (n + 1) / 2 with n = 7 x the free keyframes.  Host only, no device is opened.  The problem is checked as
 * orbx_optimize_essential_graph2 checks it for ENVELOPE (Tcw_out and Xw_out apart); an envelope beyond ORBX_EG_MAX_ENVELOPE is reported,
 * not refused.  ORBX_E_INVALID for a NULL entries or triangle. */
int orbx_eg_envelope(const orbx_eg_problem *p, int64_t *entries, int64_t *triangle);

/* ---- Optimizer::OptimizeSim3: the Sim3 between two keyframes (src/Optimizer.cc:1164-1365) ------------------------------
 * Step 4 of LoopClosing::ComputeSim3 (src/LoopClosing.cc:282-460), between SearchBySim3 and the Sim3 SearchByProjection.  Every
 * VertexSBAPointXYZ of the function is fixed: the one free vertex is a 7-DoF VertexSim3Expmap, and the whole function -- two rounds
 * of Levenberg iterations and the classification after each -- is ONE kernel launch, one workgroup per job (k_sim3_opt).
 * The arithmetic, in double unless a step says float, every operation rounded on its own (no fused multiply-add):
 *   pairs    feature i of KF1 with has_pair[i] carries two edges.  Edge 12 (EdgeSim3ProjectXYZ): obs (x1, y1) - cam_map1(project(
 *            S12.map(P2c))).  Edge 21 (EdgeInverseSim3ProjectXYZ): obs (x2, y2) - cam_map2(project(S12.inverse().map(P1c))).
 *            project = (x / z, y / z); cam_map = v * f + c; information = inv_sigma2 * I; chi2 = sum_r e_r * (inv_sigma2 * e_r).
 *            Points, observations, cameras and inv_sigma2 are floats widened to double.
 *   Sim3     sim3.h, literally: the estimate is (r, t, s) with r a quaternion that is NEVER normalised -- the start is S12 exactly as
 *            handed in; map(p) = s * (r * p) + t with Eigen's r * p (uv = 2 r.vec x p; p + r.w uv + r.vec x uv); inverse() =
 *            (conj r, conj r * ((-1 / s) * t), 1 / s); a * b = (a.r * b.r, a.s * (a.r * b.t) + a.t, a.s * b.s), no normalisation.
 *   exp      Sim3(Vector7d), update = (omega, upsilon, sigma): s = exp(sigma), theta = |omega|, R = I + Omega + Omega^2 where theta
 *            < 1e-5, else I + sin(theta) / theta Omega + (1 - cos(theta)) / theta^2 Omega^2; r = Quaterniond(R), not normalised; t =
 *            (A Omega + B Omega^2 + C I) upsilon with A, B, C from the four branches on |sigma| < 1e-5 and theta < 1e-5 (sim3.h:92-135).
 *   update   estimate = exp(x) * estimate.  fix_scale: x[6] = 0 first, written into the solver's x (VertexSim3Expmap::oplusImpl).
 *   Jacobian the reference's central difference (both edges leave linearizeOplus commented out; base_binary_edge.hpp:131-205): column
 *            d = (e(exp(+1e-9 e_d) * S) - e(exp(-1e-9 e_d) * S)) * (1 / 2e-9).  With fix_scale column 6 is exactly 0.
 *   Huber    delta = (float)sqrt(th2) in both rounds; b -= rho1 * A^T (w e), H += A^T (rho1 w) A, the active robust chi2 sums rho0
 *            (base_binary_edge.hpp:55-120), edge 12 then edge 21 of a pair.
 *   system   28 + 7 + 1 sums over the edges of the pairs still in the graph, in an order that is a fixed function of (n, thread
 *            index): results are bit-reproducible from run to run and do not depend on the other jobs of a launch.  No atomics.
 *   solve    (H + lambda I) x = b by LDL^T without pivoting; a pivot <= 0 makes the trial's chi2 DBL_MAX and leaves x as it was --
 *            x survives from the first round into the second (Solver::resizeVector does not reallocate), and starts as zeros.
 *   Levenberg as orbx_pose_optimize; lambda and ni are set anew at iteration 0 of each round.
 *   rounds   optimize(5); a pair with chi2_12 > th2 || chi2_21 > th2 (double against the float th2), at the errors of the LAST
 *            EVALUATED TRIAL, leaves the graph for good and its match is cleared; n_bad of them.  n_corr - n_bad < 10: the return
 *            value is 0 and S12_out is S12 bit for bit (the matches round 1 threw out stay cleared).  Else optimize(n_bad > 0 ? 10
 *            : 5) CONTINUING from the first round's estimate, the same test once more, and the return value counts what is left.
 * Outside the contract: a pair whose projection is not finite at an estimate the solver visits.  Against g2o's own arithmetic (Eigen's
 * LDLT, its product evaluation order) and the C library's sin / cos / exp this restatement is unpinned: DESIGN.md. */
typedef struct {
    int n;                     /* vpMatches1.size(), 0 .. 65535 */
    const uint8_t *has_pair;   /* the test of :1223-1260 passed: both points, neither bad, i2 >= 0 */
    const float *P1c, *P2c;    /* [n][3] R1w * P3D1w + t1w and R2w * P3D2w + t2w (:1241-1251); read only where has_pair[i] */
    const float *x1, *y1;      /* pKF1->mvKeysUn[i].pt */
    const float *inv_sigma2_1; /* pKF1->mvInvLevelSigma2[octave of that keypoint] */
    const float *x2, *y2;      /* pKF2->mvKeysUn[i2].pt */
    const float *inv_sigma2_2;
} orbx_sim3opt_obs;
typedef struct {
    int n_corr;                /* nCorrespondences */
    int rounds;                /* 0 (no correspondence), 1 (fewer than 10 left after the first) or 2 */
    int n_bad;                 /* nBad after round 1 */
    int more_iterations;       /* nMoreIterations: 5 or 10 */
    int iterations[2];         /* Levenberg iterations of each round */
    double chi2[2];            /* the active robust chi2 each round ended with */
    double S12[8];             /* S12_out */
} orbx_sim3opt_report;
/* cam1 / cam2 = fx fy cx cy of pKF1->mK / pKF2->mK; S12 / S12_out = qx qy qz qw tx ty tz s in double (may alias).  inlier[i] = 1
 * where vpMatches1[i] is still non-NULL on return, written only where has_pair[i]; *n_inliers = the reference's return value;
 * report may be NULL.  One upload, one launch, one download; no correspondence at all: ORBX_OK without a launch.  ORBX_E_INVALID
 * before any device work: NULL obs / cam1 / cam2 / S12 / S12_out / n_inliers, n outside [0, 65535], th2 not positive and finite,
 * with n > 0 a NULL array of obs or NULL inlier. */
int orbx_sim3_optimize(int device, const orbx_sim3opt_obs *obs, const float *cam1, const float *cam2, const double *S12, float th2,
                       int fix_scale, double *S12_out, uint8_t *inlier, int *n_inliers, orbx_sim3opt_report *report);
/* one job of a batch: the arguments of orbx_sim3_optimize */
typedef struct {
    const orbx_sim3opt_obs *obs; const float *cam1, *cam2; const double *S12;
    float th2; int fix_scale;
    double *S12_out; uint8_t *inlier;
    int n_inliers;                               /* out */
    orbx_sim3opt_report *report;                 /* out, may be NULL */
} orbx_sim3opt_job;
/* njobs optimisations (the loop candidates of one ComputeSim3) as ONE upload, ONE launch of njobs workgroups, ONE download; every
 * job's results are byte-equal to its single call.  ORBX_E_INVALID: njobs outside [1, 64], any refusal of the single call. */
int orbx_sim3_optimize_batch(int device, orbx_sim3opt_job *jobs, int njobs);

/* ---- LocalMapping::CreateNewMapPoints: the triangulation half (src/LocalMapping.cc:327-511) ---------------------------
 * The search half of the function is orbx_kf_search_for_triangulation.  This is the body of its match loop: per pair (idx1 of
 * the current keyframe, idx2 of neighbour i) the parallax test, the 4x4 SVD triangulation or KeyFrame::UnprojectStereo, two depth
 * tests, two reprojection gates and the scale-consistency gate -- one thread per pair, all neighbours in one launch (k_triangulate),
 * followed by two short launches that apply the loop's order rule (k_tri_resolve).
 * THE ORDER RULE.  The reference's loop is sequential over the neighbours: a point created for feature idx1 at neighbour i makes
 * SearchForTriangulation skip idx1 at every later neighbour (src/ORBmatcher.cc:750-751).  vbMatched2 is never written there (:725,
 * :773), so the rows of a search are independent, and with checkOri == false -- what CreateNewMapPoints passes -- dropping a row
 * changes nothing else.  The loop therefore equals: search every neighbour with the flags as they are at entry, test every pair on
 * its own, and per idx1 keep the pair of the FIRST neighbour whose tests pass.  A pair that passes at a later neighbour gets status
 * 32 + its creating status.  An earlier pair that FAILS blocks nothing.  With checkOri == true the equality does not hold.
 * The arithmetic follows the C++ types of the reference text; every operation is rounded on its own (no fused multiply-add).
 * "dotd(a, b)" is ((double)a0*b0 + (double)a1*b1) + (double)a2*b2.  Rwc is the exact transpose of the rotation block of Tcw.
 *   rays     xn = ((x - cx) * invfx, (y - cy) * invfy, 1) in float (:350-351); ray[r] = (float)dotd(Rwc.row(r), xn) (:353-355);
 *            cosParallaxRays = (float)(dotd(ray1, ray2) / (sqrt(dotd(ray1, ray1)) * sqrt(dotd(ray2, ray2)))) (:358).
 *   stereo   a feature is stereo where u_right >= 0.  cosParallaxStereo1 = cosParallaxStereo2 = cosParallaxRays + 1 in float;
 *            `if (bStereo1) 1 = S(mb1, depth1[idx1]); else if (bStereo2) 2 = S(mb2, depth2[idx2])` as written at :364-367;
 *            cosParallaxStereo = the smaller (:369).  S(mb, depth) stands for cos(2 atan2(mb / 2, depth)) and is evaluated as
 *            (float)((d*d - h*h) / (d*d + h*h)) in double with h = (double)(mb / 2) (the division in float), d = (double)depth:
 *            a STATED DEVIATION at rounding level (no device matches the C library's cos and atan2 bit for bit).
 *   branch   :372-402 literally: triangulate if cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 ||
 *            bStereo2 || (double)cosParallaxRays < 0.9998); else UnprojectStereo of keyframe 1 if bStereo1 && 1 < 2; else of
 *            keyframe 2 if bStereo2 && 2 < 1; else status 16.
 *   A        rows (xn1.x * T1.row(2)) - T1.row(0), (xn1.y * T1.row(2)) - T1.row(1), and the same two of view 2, in float (:376-379).
 *   SVD      one-sided Jacobi on the four columns of A in float, the shape of OpenCV's JacobiSVDImpl_: V = I; W[i] = the squared
 *            norm of column i, summed in double; sweeps over the column pairs (i, j), i < j, in lexicographic order.  Per pair
 *            p = sum_k (double)A[k][i] * A[k][j]; the pair is skipped when |p| <= (double)(2 * FLT_EPSILON) * sqrt(W[i] * W[j]) --
 *            this is the stopping test: a sweep that skipped all six pairs ends the iteration, which runs 30 sweeps at most.
 *            Otherwise p *= 2, beta = W[i] - W[j], gamma = sqrt(p*p + beta*beta) (OpenCV calls hypot), and in double, cast to float:
 *            beta < 0: s = sqrt(((gamma - beta) * 0.5) / gamma), c = p / ((gamma * s) * 2); else c = sqrt((gamma + beta) / (gamma *
 *            2)), s = p / ((gamma * c) * 2).  Columns i, j of A and rows i, j of V become t0 = c*a + s*b, t1 = (-s)*a + c*b in
 *            float; W[i], W[j] = the new columns' squared norms in double.  At the end the squared norms of all four columns are
 *            summed again in double; the row of V of the SMALLEST one is the solution v, and of equal ones the LATER column.
 *   point    v[3] == 0: status 17.  x3D = v[0..2] / v[3] in float (:390); the sign of v cancels.
 *   Unproject (src/KeyFrame.cc:654-670) depth[i] <= 0 (or NaN): status 24 (the reference dereferences an empty Mat).  x = (raw_x[i] -
 *            cx) * z * invfx, y likewise, left to right in float, from the RAW keypoint mvKeys[i]; x3D[r] = (float)(dotd(Rwc.row(r),
 *            (x, y, z)) + (double)Ow[r]) (cv::gemm adds in double and casts once).
 *   depth    z1 = (float)(dotd(R1.row(2), x3D) + (double)t1[2]); z1 <= 0: status 18; z2 likewise: 19 (:408-414).
 *   gates    x, y as z; invz = (float)(1.0 / (double)z); u = fx * x * invz + cx, v = fy * y * invz + cy, left to right in float;
 *            errors u - kp.x, v - kp.y and, for a stereo feature, (u - mbf * invz) - u_right, where mbf is the CURRENT keyframe's
 *            for BOTH keyframes (the reference's :465).  Rejected (status 20 / 21) when (double)(float sum of the squares, left to
 *            right) > 5.991 * (double)sigma2 (monocular) or 7.8 * (double)sigma2 (stereo), sigma2 = level_sigma2[octave].
 *   scale    dist = (float)sqrt(squared norm of (x3D - Ow) summed in double), the difference in float; a zero distance: status 22;
 *            ratioDist = dist2 / dist1, ratioOctave = scale_factors[octave1] / scale_factors[octave2]; status 23 when ratioDist *
 *            ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor (:490), in float.
 * status: 0 created by triangulation, 1 / 2 created from keyframe 1's / 2's stereo depth, 16 no stereo and low parallax, 17 w ==
 * 0, 18 z1 <= 0, 19 z2 <= 0, 20 / 21 reprojection gate of keyframe 1 / 2, 22 zero distance, 23 scale ratio, 24 stereo feature
 * without positive depth, 32 + (0, 1, 2) superseded by an earlier neighbour.  x3d holds the position of every pair that reached
 * one (status 0-2, 18-23, 32-34) and zeros otherwise.  Against OpenCV's own arithmetic (its gemm, dot and SVD kernels differ by
 * build) this restatement is unpinned: DESIGN.md. */
typedef struct { float Tcw[12]; float Ow[3]; float fx, fy, cx, cy, invfx, invfy, mb, mbf; } orbx_tri_view; /* Tcw: 3 x 4 row major */
typedef struct {
    int n;
    const float *x, *y;        /* mvKeysUn[i].pt */
    const int32_t *octave;     /* mvKeysUn[i].octave */
    const float *u_right;      /* mvuRight */
    const float *depth;        /* mvDepth; may be NULL when no feature named by a pair is stereo */
    const float *raw_x, *raw_y;/* mvKeys[i].pt; both NULL = x and y (rectified stereo: mvKeys == mvKeysUn) */
} orbx_tri_feats;
/* pairs[n2][2*cap] and npairs[n2] as orbx_kf_search_for_triangulation returns them; one table of level factors for all keyframes.
 * status[n2][cap] and x3d[n2][cap][3] are written for the first npairs[i] entries of each row only; *n_new = pairs with status 0-2.
 * One upload, three launches on one stream, one download.  ORBX_E_INVALID before any device work: a NULL argument or keyframe
 * array (depth: see above), n2 outside [1, 64], cap < 1, npairs[i] outside [0, cap], a pair index outside its keyframe, nlevels
 * outside [1, 16], an octave of a paired feature outside [0, nlevels).  ORBX_E_CAPACITY: more than 2^22 pairs in all. */
int orbx_triangulate_pairs(int device, const orbx_tri_feats *k1, const orbx_tri_view *v1, const orbx_tri_feats *const *k2s,
                           const orbx_tri_view *v2s, int n2, const int32_t *pairs, int cap, const int *npairs,
                           const float *scale_factors, const float *level_sigma2, int nlevels, float ratio_factor,
                           uint8_t *status, float *x3d, int *n_new);
/* mvDepth and the raw positions mvKeys[i].pt ([n] each; raw_x = raw_y = NULL: the frame's own x / y) for a resident keyframe: one
 * upload, once per frame -- a second call is ORBX_E_INVALID; they are immutable like the rest of the frame.  Only
 * orbx_frame_triangulate reads them: the call may run beside other threads' searches on the frame, but not beside another
 * orbx_frame_set_depth or an orbx_frame_triangulate on it. */
int orbx_frame_set_depth(orbx_frame *f, const float *depth, const float *raw_x, const float *raw_y);
/* orbx_triangulate_pairs on resident keyframes: up go the views and the pair lists, back come status and x3d, byte-equal to the
 * host-pointer call on the same values.  The frames are only read (several threads may share them); a frame whose creation is
 * pending is waited for through its event.  ORBX_E_INVALID also for frames on different devices and for a frame that has stereo
 * features, or was made by orbx_frame_create_from_extraction, and has no depth attached.  (The octaves of a frame made from an
 * extraction exist on the device only: the kernel checks them, and the call returns ORBX_E_INVALID after its launches.) */
int orbx_frame_triangulate(const orbx_frame *k1, const orbx_tri_view *v1, const orbx_frame *const *k2s, const orbx_tri_view *v2s,
                           int n2, const int32_t *pairs, int cap, const int *npairs, const float *scale_factors,
                           const float *level_sigma2, int nlevels, float ratio_factor, uint8_t *status, float *x3d, int *n_new);

/* ---- Sim3Solver: the hypotheses of LoopClosing::ComputeSim3's RANSAC (src/Sim3Solver.cc:233-433) ----------------------
 * Sim3Solver::iterate draws three correspondences, solves Horn's closed form on them (ComputeSim3), reprojects EVERY
 * correspondence both ways (CheckInliers) and counts.  The early return and the best-so-far bookkeeping of iterate depend on the
 * order of the hypotheses and cost nothing; they stay on the host.  The device evaluates the WHOLE TABLE of hypotheses of a
 * solver -- of every solver of a ComputeSim3 call -- in one launch (k_sim3: one wave per hypothesis, one lane per point, the
 * ballot of the inlier test is the mask word), and the host replays iterate over the table (adapter/sim3, Sim3Ransac in orbx.py).
 * The arithmetic follows the C++ types of the reference text; every operation is rounded on its own (no fused multiply-add).
 * "dotd(a, b)" is ((double)a0*b0 + (double)a1*b1) + (double)a2*b2, cast to float ONCE where a cv::Mat product stores it.
 *   points   P1 / P2 = the three sampled columns of X1 / X2 (:176-177), in the order of the sample row.
 *   centroid O[r] = (float)((double)((P[r][0] + P[r][1]) + P[r][2]) * (1.0 / 3.0)), the sum in float (cv::reduce, then C / P.cols);
 *            Pr[r][i] = P[r][i] - O[r] in float (:219-228).
 *   M        M[r][c] = (float)dotd(Pr2.row(r), Pr1.row(c)) (:250).
 *   N        the ten entries of :258-267 as sums and differences of FLOATS, left to right, the leading minus first ((-M00) + M11) -
 *            M22; the double variables of the text hold float values, N stores them as float.
 *   eigen    cv::eigen(N) is restated as a cyclic Jacobi in float on the upper triangle A = N, diagonal W[i] = A[i][i], V = I
 *            (eigenvectors are V's rows).  Sweeps over the pivots (k, l), k < l, in lexicographic order.  With p = A[k][l] the
 *            pivot is skipped when (double)p * p <= 2^-46 * |(double)W[k] * W[l]| (|p| <= FLT_EPSILON * sqrt|W[k] W[l]|, evaluated
 *            exactly) -- this is the stopping test: a sweep that skipped all six pivots ends the iteration, which runs 30 sweeps
 *            at most.  Otherwise, in float, hyp(a, b) = (float)sqrt((double)a*a + (double)b*b) where OpenCV calls hypot:
 *            y = (W[l] - W[k]) * 0.5; t = |y| + hyp(p, y); s = hyp(p, t); c = t / s; s = p / s; t = (p / t) * p; y < 0 negates s
 *            and t; A[k][l] = 0; W[k] -= t; W[l] += t; then rot(a, b) = (a*c - b*s, a*s + b*c) on (A[i][k], A[i][l]) for i < k,
 *            (A[k][i], A[i][l]) for k < i < l, (A[k][i], A[l][i]) for i > l and (V[k][i], V[l][i]) for every i (the shape of
 *            OpenCV's JacobiImpl_, which picks the largest pivot instead of sweeping).  q = the row of V of the LARGEST W, and of
 *            equal ones the EARLIER (cv::eigen sorts descending; the reference reads evec.row(0)).  The sign of q cancels below.
 *   rotation a STATED DEVIATION at rounding level: the reference goes q -> atan2 -> angle-axis -> cv::Rodrigues (:281-291), and no
 *            device matches the C library's atan2, sin and cos bit for bit.  The same rotation is evaluated algebraically: with
 *            (w, x, y, z) = q widened to double, every product formed once in double and n2 = ((ww + xx) + yy) + zz,
 *              R00 = (((ww + xx) - yy) - zz) / n2   R01 = (2 (xy - wz)) / n2             R02 = (2 (xz + wy)) / n2
 *              R10 = (2 (xy + wz)) / n2             R11 = (((ww - xx) + yy) - zz) / n2   R12 = (2 (yz - wx)) / n2
 *              R20 = (2 (xz - wy)) / n2             R21 = (2 (yz + wx)) / n2             R22 = (((ww - xx) - yy) + zz) / n2
 *            each cast to float.  It depends on q's direction only, as the reference's does.
 *   degenerate  x == y == z == 0 exactly (norm(vec) == 0: the reference divides by it and every entry becomes NaN): n_inliers =
 *            0, the mask is 0 and all 13 floats of srt are the quiet NaN 0x7fc00000, with fix_scale too.  Nothing else is special-
 *            cased: a NaN or infinite s, R or t makes every comparison below false, which is the reference's outcome.
 *   scale    P3[r][i] = (float)dotd(R.row(r), Pr2.col(i)) (:295).  nom = sum of (double)Pr1[r][i] * (double)P3[r][i], den = sum of
 *            (double)(P3[r][i] * P3[r][i]) -- the square in FLOAT (cv::pow) -- both from 0.0 in row-major order; ms12i =
 *            (float)(nom / den), or 1.0f with fix_scale (:299-318).
 *   t12      mt12i[r] = (float)((double)O1[r] - (double)ms12i * dotd(R.row(r), O2)) (:323: one gemm, one cast).
 *   T12, T21 sR[r][c] = (float)((double)ms12i * (double)R[r][c]); sRinv[r][c] = (float)((1.0 / (double)ms12i) * (double)R[c][r]);
 *            tinv[r] = (float)(-dotd(sRinv.row(r), mt12i)) (:330-343).
 *   Project  (:389-410) Pc[r] = (float)(dotd(sR.row(r), X) + (double)t[r]); invz = 1 / Pc[2], a FLOAT division; x = Pc[0] * invz,
 *            y = Pc[1] * invz; u = fx * x + cx, v = fy * y + cy, left to right in float.  FromCameraToImage (:414-433) is the same
 *            from X itself.  A point behind the camera projects mirrored, as in the reference; z == 0 gives a non-finite error.
 *   inliers  err1 = |P1im1 - Project(X2, T12, K1)|^2, err2 = |Project(X1, T21, K2) - P2im2|^2, each difference in float and the two
 *            squares summed as (float)((double)d0*d0 + (double)d1*d1); inlier = err1 < max_err1[i] && err2 < max_err2[i], strict
 *            and false for NaN (:355-370).
 *   size_t   include/Sim3Solver.h:78-79 declares mvnMaxError1/2 as vector<size_t>, so push_back(9.210 * sigmaSquare) (:87-88)
 *            TRUNCATES: the threshold the comparison sees is (float)(size_t)(9.210 * (double)sigma2) -- 9 at level 0, not 9.21.
 *            The caller computes it so; max_err1 / max_err2 take the resulting float.
 * Against OpenCV's own arithmetic (its reduce, gemm and dot kernels differ by build, and JacobiImpl_ pivots differently) this
 * restatement is unpinned: DESIGN.md. */
typedef struct {
    int n;                          /* correspondences, Sim3Solver's N: 3 .. 65535 */
    const float *X1, *X2;           /* [n][3] mvX3Dc1 / mvX3Dc2: the points in camera 1 / camera 2 coordinates */
    const float *max_err1, *max_err2; /* [n] mvnMaxError1/2 as the float the comparison sees ("size_t" above) */
    float K1[4], K2[4];             /* fx fy cx cy */
    int fix_scale;                  /* mbFixScale */
    int n_hyp;                      /* hypotheses to evaluate: 1 .. 1024 */
    const int32_t *samples;         /* [n_hyp][3] indices into 0 .. n-1, the three of a row distinct */
    /* out */
    int32_t *n_inliers;             /* [n_hyp] mnInliersi */
    float *srt;                     /* [n_hyp][13] ms12i, mR12i row major, mt12i */
    uint64_t *inlier_bits;          /* [n_hyp][(n+63)/64] bit i%64 of word i/64 = mvbInliersi[i]; bits >= n are 0 */
} orbx_sim3_job;
/* One upload, one launch, one download.  ORBX_E_INVALID before any device work: a NULL job or array, n outside [3, 65535], n_hyp
 * outside [1, 1024], a sample index outside [0, n), a row of samples with two equal indices. */
int orbx_sim3_hypotheses(int device, orbx_sim3_job *job);
/* The solvers of one ComputeSim3 call as ONE upload, ONE launch, ONE download; every job's results are byte-equal to its single
 * call.  ORBX_E_INVALID: njobs outside [1, 64], any refusal of the single call in any job; ORBX_E_CAPACITY: more than 2^22 mask
 * words in all. */
int orbx_sim3_hypotheses_batch(int device, orbx_sim3_job *jobs, int njobs);

/* ---- PnPsolver: the hypotheses of Tracking::Relocalization's EPnP RANSAC (src/PnPsolver.cc:176-350, 386-961) --------------
 * PnPsolver::iterate draws four correspondences, runs EPnP on them (compute_pose), reprojects EVERY correspondence (CheckInliers)
 * and, when the count reaches mRansacMinInliers, runs EPnP again on the inliers and reprojects again (Refine).  As for Sim3Solver
 * the bookkeeping of iterate stays on the host and the device evaluates the WHOLE TABLE of hypotheses of a solver -- of every
 * candidate's solver of one Relocalization -- in one launch (k_pnp: one wave per hypothesis), and the host replays iterate over
 * the table (PnPRansac in orbx.py).  Refine in the reference reads mvbBestInliers, the best set so far, so it depends on the
 * replay's state; but the best set changes only at a row that beats it, and refining an UNCHANGED set repeats a refinement that
 * has already failed (had it succeeded, iterate would have returned).  So a refinement of every qualifying row from its OWN
 * mask is all a replay can ever ask for: a row that qualifies without beating the best set re-fails, which the replay knows
 * without looking.  The table therefore holds two results per row.
 * All of compute_pose is fp64 as in the reference text; every operation is rounded on its own (no fused multiply-add); sums and
 * products associate left to right unless brackets say otherwise.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2.
 *   members  compute_pose runs on a list of correspondences: the four of a sample row in the row's order, or (Refine) the set bits
 *            of the row's mask in rising index.  pw = (double)P3Dw[i], (u, v) = (double)P2D[i], nc = (double)(their number).
 *   sums     "SUM x" over the members: for the four of a sample row, serially in the row's order from 0.0.  For a mask: lane l of
 *            64 adds the members i = l (mod 64) in rising i from 0.0 (non-members add nothing), then a xor butterfly over the
 *            strides 32, 16, 8, 4, 2, 1 (v[l] = v[l] + v[l ^ stride]); every lane ends with the same bits because a + b == b + a.
 *   SVD      every OpenCV call of the text (cvMulTransposed is the SUM of products itself; cvSVD of PW0tPW0, MtM and ABt;
 *            cvInvert(CV_SVD); cvSolve(CV_SVD)) is restated through ONE routine, a one-sided cyclic Jacobi on an m x n matrix A,
 *            m >= n, V = I (n x n): with N = n rounded up to even, a sweep is the N - 1 rounds r = 0 .. N-2 of the round-robin
 *            schedule, round r holding the pivots {N-1, r} and {(r + k) mod (N-1), (r - k) mod (N-1)} for k = 1 .. N/2 - 1, each
 *            taken as (p, q) with p < q and left out when q >= n; the pivots of a round touch disjoint columns, so their order
 *            is immaterial.  For a pivot: a = SUM_i A[i][p]^2, b = SUM_i A[i][q]^2, g = SUM_i A[i][p] A[i][q], i rising from 0.0.
 *            The pivot is skipped when |g| <= 2^-49 * sqrt(a * b) (false for NaN) -- this is the stopping test: a sweep that
 *            skipped every pivot ends the iteration, which runs 30 sweeps at most.  Otherwise g2 = g * 2, beta = a - b, gamma =
 *            sqrt(g2 * g2 + beta * beta); beta < 0: delta = (gamma - beta) * 0.5, s = sqrt(delta / gamma), c = g2 / ((gamma * s)
 *            * 2); else c = sqrt((gamma + beta) / (gamma * 2)), s = g2 / ((gamma * c) * 2); then every row (x, y) = (.[p], .[q])
 *            of A and of V becomes (c*x + s*y, c*y - s*x) (the shape of OpenCV's JacobiSVDImpl_, which sweeps lexicographically
 *            and rotates with its own hypot).  Afterwards w[j] = sqrt(SUM_i A[i][j]^2).
 *   sort     where an order is needed: descending w, of equal values the earlier index first (selection: the r-th is the first
 *            unused j whose w no later unused one exceeds).
 *   eigen    cvSVD(.., CV_SVD_U_T) of the symmetric PW0tPW0 and MtM: dc / d = the sorted w, row k of uct / ut = COLUMN order[k]
 *            of V (U = V where w > 0 for such a matrix, and V is defined where w = 0).  With four points MtM has rank <= 8; the
 *            four vectors compute_L_6x10 reads span a null space and their order among near-zero values is what the sort gives.
 *   solve    cvSolve(A, b, x, CV_SVD): thr = (SUM_k w[k], k rising from 0.0) * 2^-51; x = 0.0; for k rising with w[k] > thr:
 *            t = ((SUM_i A[i][k] b[i]) / w[k]) / w[k] on the rotated A, x[j] = x[j] + V[j][k] * t.  cvInvert(CC, CV_SVD): column j
 *            of CC_inv is the solve with b = the j-th unit vector.
 *   control  cws[0] = (SUM pw) / nc.  PW0tPW0[j][k] (j <= k, mirrored) = SUM (pw[j] - cws[0][j]) * (pw[k] - cws[0][k]).
 *            cws[i][j] = cws[0][j] + sqrt(dc[i-1] / nc) * uct[i-1][j] (:386-420).
 *   alphas   (:422-445) with d = pw - cws[0]: a[1+j] = (ci[3j] d0 + ci[3j+1] d1) + ci[3j+2] d2, a[0] = ((1.0 - a[1]) - a[2]) - a[3]
 *            (the text's 1.0f widens exactly); they are recomputed from the same values wherever they are read.
 *   MtM      rows M1, M2 of fill_M (:447-462) literally, zeros included; MtM[j][k] (j <= k, mirrored) = SUM of the two products
 *            M1[j] M1[k] then M2[j] M2[k], added in turn to the running value.
 *   betas    compute_L_6x10 (2.0f widens exactly), compute_rho, find_betas_approx_1/2/3, compute_A_and_b_gauss_newton and
 *            qr_solve are the text's own scalar code (:678-961), left to right.  qr_solve's pivot scan (:891-896) never looks at
 *            the last row; on a zero pivot it returns and leaves x as it was, and x is DEFINED as zero at the start of each
 *            gauss_newton (the reference reads it uninitialised: a stated deviation).
 *   R, t     compute_ccs (from 0.0, i rising); solve_for_sign looks at the first member only: its pc[2] < 0 negates ccs (and with
 *            them every pc).  pc0 = (SUM pc) / nc; pw0 IS cws[0] (the same sum, the same division).  ABt[j][c] = SUM (pc[j] -
 *            pc0[j]) * (pw[c] - pw0[c]).  cvSVD(ABt): U[i][k] = A[i][k] / w[k] on the rotated A, columns in place (no sort, no
 *            completion of a zero singular value: the pose is then not finite); R[i][j] = dot(U row i, V row j); det as the text
 *            writes it, each triple product (x*y)*z; det < 0 negates row 2; t[i] = pc0[i] - dot(R row i, pw0).
 *            reprojection_error: SUM sqrt(eu*eu + ev*ev) / nc with ue = uc + (fu * Xc) * inv_Zc.  The second and third solution
 *            replace the kept one when their error is strictly smaller (:529-531).
 *   inliers  CheckInliers (:319-350) with the text's mix: Xc, Yc = (float)(dot(R row, P) + t) with P widened; invZc = (float)(1.0 /
 *            (dot(R row 2, P) + t[2])); ue = uc + (fu * (double)Xc) * (double)invZc in double; distX = (float)((double)P2D.x - ue);
 *            error2 = distX * distX + distY * distY in float; inlier = error2 < max_err[i], strict and false for NaN.  A point
 *            behind the camera projects mirrored, as in the reference.
 *   special  a pose with a NaN or an infinity among its twelve numbers: n_inliers = 0, the mask is 0 and all twelve doubles are
 *            the quiet NaN 0x7ff8000000000000 (stated, by analogy with srt: an infinite t[2] alone would otherwise pass points).
 *            A row whose n_inliers is below min_inliers is not refined: n_refined = -1, a zero mask, twelve quiet NaNs.
 * Against OpenCV's own arithmetic (its SVD sweeps and rotates differently, completes zero singular values and cuts by its own
 * threshold) this restatement is unpinned: DESIGN.md. */
typedef struct {
    int n;                          /* correspondences, PnPsolver's N: 4 .. 65535 */
    const float *P3Dw;              /* [n][3] mvP3Dw */
    const float *P2D;               /* [n][2] mvP2D */
    const float *max_err;           /* [n] mvMaxError = mvSigma2[i] * th2, the float product */
    double K[4];                    /* fu fv uc vc: the reference widens F.fx .. to double members */
    int min_inliers;                /* mRansacMinInliers after SetRansacParameters' adjustment: >= 4 */
    int n_hyp;                      /* hypotheses to evaluate: 1 .. 1024 */
    const int32_t *samples;         /* [n_hyp][4] indices into 0 .. n-1, the four of a row distinct */
    /* out */
    int32_t *n_inliers;             /* [n_hyp] mnInliersi */
    double *Rt;                     /* [n_hyp][12] mRi row major, then mti */
    uint64_t *inlier_bits;          /* [n_hyp][(n+63)/64] bit i%64 of word i/64 = mvbInliersi[i]; bits >= n are 0 */
    int32_t *n_refined;             /* [n_hyp] mnRefinedInliers of Refine from this row's mask; -1: the row did not qualify */
    double *Rt_refined;             /* [n_hyp][12] */
    uint64_t *refined_bits;         /* [n_hyp][(n+63)/64] mvbRefinedInliers */
} orbx_pnp_job;
/* One upload, one launch, one download.  ORBX_E_INVALID before any device work: a NULL job or array, n outside [4, 65535], n_hyp
 * outside [1, 1024], min_inliers < 4, a sample index outside [0, n), a row of samples with two equal indices. */
int orbx_pnp_hypotheses(int device, orbx_pnp_job *job);
/* The solvers of one Relocalization as ONE upload, ONE launch, ONE download; every job's results are byte-equal to its single
 * call.  ORBX_E_INVALID: njobs outside [1, 64], any refusal of the single call in any job; ORBX_E_CAPACITY: more than 2^22 mask
 * words in all (both masks counted). */
int orbx_pnp_hypotheses_batch(int device, orbx_pnp_job *jobs, int njobs);

/* ---- Initializer: Tracking::MonocularInitialization's H / F RANSAC and reconstruction (src/Initializer.cc:37-1026) --------
 * Initializer::Initialize runs FindHomography and FindFundamental over the same 200 sample rows (mvSets), picks a model by the
 * ratio of the two best scores and reconstructs the motion from it (ReconstructH / ReconstructF over CheckRT).  The device
 * evaluates the WHOLE TABLE of both models in one launch (k_mono_hyp: one wave per (model, hypothesis), the ballot of the inlier
 * test is the mask word), every motion hypothesis in a second (k_mono_reconstruct: one workgroup each, the arg-max of the table
 * and the decomposition repeated in every wave) and the final choice in a third (k_mono_decide: one workgroup).  "mono_init":
 * "init" alone names SearchForInitialization and the library's set-up.
 * The arithmetic follows the C++ types of the reference text; every operation is rounded on its own (no fused multiply-add); float
 * sums and products associate left to right as C parses them.  "dotd(a, b)" is ((double)a0*b0 + (double)a1*b1) + (double)a2*b2, and
 * every cv::Mat product X*Y is mm(X, Y)[r][c] = (float)dotd(X.row(r), Y.col(c)), one cast from a double accumulation; a product of
 * three is (X*Y)*Z with the middle result stored as float.  "1.0 / x" with a float x is (float)(1.0 / (double)x) wherever the text
 * writes it: w2in1inv, w1in2inv, invSigmaSquare, invZ1, invZ2, sX, sY.
 *   Normalize (:831-883) on the HOST half of the call, over ALL keypoints of a frame in index order: meanX, meanY = the serial
 *            float sums from 0.0f divided by (float)N; meanDevX, meanDevY = the serial float sums of |x - meanX|, |y - meanY|
 *            divided by (float)N; sX = 1.0 / meanDevX, sY likewise; T = (sX 0 (-meanX)*sX; 0 sY (-meanY)*sY; 0 0 1).  A normalised
 *            point is ((x - meanX) * sX, (y - meanY) * sY), which the device evaluates for the eight matches of a sample row.
 *   det, inv det(M) = (m00*(m11*m22 - m12*m21) - m01*(m10*m22 - m12*m20)) + m02*(m10*m21 - m11*m20) with every factor widened to
 *            double (cv::determinant).  inv(M): d = det(M); d == 0: NINE ZEROS (cv::Mat::inv of a singular matrix); else d = 1.0 / d
 *            and inv[r][c] = (float)(cof * d), cof = the difference of two double products of the adjugate, in the order
 *            m11*m22 - m12*m21, m02*m21 - m01*m22, m01*m12 - m02*m11 / m12*m20 - m10*m22, m00*m22 - m02*m20, m02*m10 - m00*m12 /
 *            m10*m21 - m11*m20, m01*m20 - m00*m21, m00*m11 - m01*m10.  T2inv = inv(T2) (:164), H12i = inv(H21i) (:194), invK (:654).
 *   SVD      every cv::SVDecomp / cv::SVD::compute of the file (:305, :349, :353, :667, :1009) is ONE routine, a one-sided (Hestenes)
 *            Jacobi on the n columns of an m x n FLOAT matrix A, n odd (9 or 3), V = I (n x n, float).  A sweep is the n rounds r =
 *            0 .. n-1 of the round-robin schedule of the PnP block for N = n + 1: round r holds the pivots {(r + k) mod n, (r - k)
 *            mod n}, k = 1 .. (n-1)/2, each taken as (p, q) with p < q (the pair of the schedule that holds the padding column N-1
 *            does not exist); the pivots of a round touch disjoint columns, so their order is immaterial.  For a pivot, in DOUBLE:
 *            a = SUM (double)A[i][p]*A[i][p], b = SUM (double)A[i][q]*A[i][q], g = SUM (double)A[i][p]*A[i][q], where SUM is a
 *            STATED BUTTERFLY over 16 slots (m <= 16): slot i holds 0.0 + the product of row i (0.0 for i >= m), then v[i] = v[i] +
 *            v[i ^ stride] for the strides 8, 4, 2, 1; every slot ends with the same bits.  (Measured against the serial sum in
 *            rising i: profiles/r19_init.txt.)  The pivot is skipped when |g| <= (double)(2 * FLT_EPSILON) * sqrt(a * b) (false for NaN) --
 *            the stopping test: a sweep that skipped every pivot ends the iteration, which runs 30 sweeps at most.  Otherwise g2 =
 *            g * 2, beta = a - b, gamma = sqrt(g2*g2 + beta*beta), and in double, cast to float: beta < 0: s = sqrt(((gamma - beta) *
 *            0.5) / gamma), c = g2 / ((gamma * s) * 2); else c = sqrt((gamma + beta) / (gamma * 2)), s = g2 / ((gamma * c) * 2) (s
 *            resp. c re-widened from its float).  Every row (x, y) = (.[p], .[q]) of A and of V becomes (c*x + s*y, (-s)*x + c*y) in
 *            float.  Afterwards W2[j] = the SERIAL sum over rising i, from 0.0, of (double)A[i][j]^2.  (The shape of OpenCV's float JacobiSVDImpl_, which
 *            sweeps lexicographically, carries the norms along and calls hypot.)
 *   null     vt.row(8) (:307, :351): column j of V for the SMALLEST W2[j], of equal ones the LATER (j = 0, then every j whose W2[j]
 *            <= the kept one).  The sign cancels in everything that follows.
 *   U w Vt   of a 3 x 3 matrix: order = descending W2, of equal values the earlier index first (selection: the r-th is the first
 *            unused j whose W2 no later unused one exceeds); wd = sqrt(W2[j]) in double, w[r] = (float)wd, column r of U = the
 *            rotated column j of A times (float)(1.0 / wd) -- times 0.0f when wd <= FLT_MIN: no completion of a zero singular
 *            value -- and row r of Vt = column j of V.
 *   H        A of ComputeH21 (:274-301) literally, in float ((-u2)*u1 for -u2*u1), m = 16; Hn = null reshaped 3 x 3; H21i =
 *            mm(mm(T2inv, Hn), T1) (:193); H12i = inv(H21i).
 *   F        A of ComputeF21 (:329-345), m = 8; Fpre = null reshaped; U w Vt of Fpre; Fn = mm(mm(U, diag(w0, w1, 0)), Vt) (:355-
 *            357); F21i = mm(mm(T2^T, Fn), T1) (:253).
 *   check    CheckHomography (:360-448) / CheckFundamental (:450-528) literally in float, th = 5.991f resp. th = 3.841f with thScore
 *            = 5.991f, invSigmaSquare = 1.0 / (sigma*sigma).  The gate is `if (chi > th) bIn = false; else score += th - chi`: a
 *            NaN chi takes the else -- the score becomes NaN and the match STAYS an inlier.  A singular H21i gives H12i = 0, hence
 *            w2in1inv = inf, u2in1 = NaN, chiSquare1 = NaN and a NaN score with every first gate open.
 *   score    a STATED DEVIATION from the reference's single serial float sum: lane l of 64 adds, from 0.0f and in rising i, the
 *            two terms of every match i = l (mod 64) in the text's order, then a xor butterfly over the strides 32, 16, 8, 4, 2, 1
 *            (v[l] = v[l] + v[l ^ stride]); every lane ends with the same bits.
 *   choice   (:203, :257) best_h = the EARLIEST hypothesis whose score_h is strictly the greatest and > 0.0f (currentScore > score
 *            from 0.0f: a NaN never wins), -1 if none, SH its score or 0.0f; best_f, SF likewise.  RH = SH / (SH + SF) in float;
 *            (double)RH > 0.40 takes H, else F (:133-142).  A STATED DEVIATION: when the model taken has no winner -- SH == SF ==
 *            0, RH is NaN -- the reference's F21 is an empty matrix and its mask has no element (FindFundamental sizes them from
 *            the empty argument, :219) and ReconstructF reads out of range; here model = 0, ok = 0, nothing is reconstructed.
 *   ReconstructH (:642-812) A = mm(mm(invK, H21), K); U w Vt of A; s = (float)(det(U) * det(Vt)); (d1, d2, d3) = w; `(double)(d1 /
 *            d2) < 1.00001 || (double)(d2 / d3) < 1.00001` (float quotients): ok = 0 with every row zero.  aux1, aux3, aux_stheta,
 *            ctheta, aux_sphi, cphi (:688-733) in float, sqrt correctly rounded; x1, x3, stheta, sphi by the four sign rows of the
 *            text.  Hypothesis i < 4: Rp = (ctheta 0 -stheta[i]; 0 1 0; stheta[i] 0 ctheta), tp = (x1[i], 0, -x3[i]) each times (d1 -
 *            d3) in float; 4 + i: Rp = (cphi 0 sphi[i]; 0 -1 0; sphi[i] 0 -cphi), tp = (x1[i], 0, x3[i]) each times (d1 + d3).  R =
 *            mm(mm(sU, Rp), Vt) with sU = s * U in float; t = U*tp as a Mat product, then t[k] = (float)((double)t[k] * (1.0 /
 *            sqrt(dotd(t, t)))) (t / cv::norm(t)).  The normals vn are never read.
 *   ReconstructF (:533-640) E21 = mm(mm(K^T, F21), K); DecomposeE (:1006-1026): U w Vt of E21; t = U.col(2) normalised as above;
 *            R1 = mm(mm(U, W), Vt), W = (0 -1 0; 1 0 0; 0 0 1), negated when det(R1) < 0; R2 likewise with W^T.  Rows: (R1, t),
 *            (R2, t), (R1, -t), (R2, -t).  Which of R1 / R2 is which and the sign of t follow from the restated SVD; the SET of
 *            four is the same.
 *   CheckRT  (:886-1004) th2 = (float)(4.0 * (double)(sigma*sigma)).  P1 = K[I|0], P2 = mm(K, [R|t]) (3 x 4), O2[r] =
 *            (float)(-dotd(R.col(r), t)).  Per match of the mask: A (:818-821) rows u1*P1.row(2) - P1.row(0), v1*P1.row(2) -
 *            P1.row(1), u2*P2.row(2) - P2.row(0), v2*P2.row(2) - P2.row(1) in float; v = the 4x4 routine of the triangulation
 *            block ("SVD" there, unchanged); p = v[0..2] / v[3], float divisions as there.  A non-finite p is skipped.  dist1 =
 *            (float)sqrt(dotd(p, p)); n2 = p - O2 in float, dist2 likewise; cosParallax = (float)(dotd(p, n2) / (double)(dist1 *
 *            dist2)).  `p.z <= 0 && (double)cosParallax < 0.99998` skips; p2[r] = (float)(dotd(R.row(r), p) + (double)t[r]); p2.z
 *            likewise.  invZ1 = 1.0 / p.z; im1x = fx*p.x*invZ1 + cx, left to right; squareError1 > th2 skips (a NaN error does NOT
 *            skip); view 2 likewise.  Every match that arrives here is ACCEPTED: it counts in n_good and its point is kept;
 *            triangulated is true only where (double)cosParallax < 0.99998.
 *   rank     cos_parallax of a row = the accepted cosine of rank min(50, n_good - 1) in ascending order, a NaN above every number
 *            and returned as 0x7fc00000; 1.0f when n_good == 0 (the text's parallax = 0).
 *   acos     parallax = acos(c)*180/CV_PI goes through the C library, which no device matches bit for bit.  The host bisects once
 *            per call the float thresholds c_gt and c_ge with (float)(acos((double)c) * 180 / CV_PI) > min_parallax exactly when c
 *            < c_gt, and >= min_parallax exactly when c < c_ge, over the floats of [-1, 1] (the float above 1 when every one
 *            passes).  The device tests `c >= -1.0f && c < c_gt` (ReconstructF's `>`, :595) resp. c_ge (ReconstructH's `>=`,
 *            :801); a NaN fails as in the text.  Degrees are formed from the returned cosine by the host's acos.
 *   decide H (:769-811) literally over the eight rows in order: nGood > bestGood moves bestGood to secondBestGood and takes the
 *            row; else nGood > secondBestGood takes its place.  ok = (double)secondBestGood < 0.75 * bestGood && parallax(best) >=
 *            min_parallax && bestGood > min_triangulated && (double)bestGood > 0.9 * N, N = the bits of the mask.  winner =
 *            bestSolutionIdx (-1 when no row has a point).
 *   decide F (:569-639) maxGood = the largest of the four; nMinGood = max((int)(0.9 * N), min_triangulated); nsimilar = rows with
 *            (double)nGood > 0.7 * maxGood; maxGood < nMinGood || nsimilar > 1: ok = 0, winner = -1.  Else winner = the FIRST row
 *            whose nGood == maxGood (the else-if chain tries no other) and ok = parallax(winner) > min_parallax.
 *   points   P3D[first] / triangulated[first] of the winner's accepted matches when ok; zero / false everywhere else.
 *   NaN      every NaN among the returned floats (scores, H21, F21, R, t, cos_parallax, parallax) is the quiet NaN 0x7fc00000: the
 *            sign and payload of an invalid operation's result differ between processors.
 * Against OpenCV's own arithmetic (SVDecomp sweeps, rotates and sorts differently and completes zero singular values; its gemm,
 * inv and determinant kernels differ by build) this restatement is unpinned: DESIGN.md. */
typedef struct {
    int n1, n2;                     /* keypoints of the reference / current frame: n .. 65535 each */
    const float *xy1, *xy2;         /* [n1][2], [n2][2] mvKeys1 / mvKeys2 (undistorted): pt.x, pt.y */
    int n;                          /* matches, mvMatches12.size(): 8 .. 8192 */
    const int32_t *matches;         /* [n][2] mvMatches12: (first, second), first STRICTLY rising */
    float sigma;                    /* mSigma */
    float K[4];                     /* fx fy cx cy of mK; read by orbx_mono_init_reconstruct / _initialize */
    float min_parallax;             /* minParallax (Initialize passes 1.0); read as K is */
    int min_triangulated;           /* minTriangulated (Initialize passes 50); read as K is */
    int n_hyp;                      /* mMaxIterations: 1 .. 1024; not read by orbx_mono_init_reconstruct */
    const int32_t *samples;         /* [n_hyp][8] mvSets: indices into 0 .. n-1, the eight of a row distinct; as n_hyp */
    /* out of orbx_mono_init_hypotheses alone */
    float *score_h, *score_f;       /* [n_hyp] currentScore of CheckHomography / CheckFundamental */
    float *H21, *F21;               /* [n_hyp][9] H21i / F21i row major */
    uint64_t *bits_h, *bits_f;      /* [n_hyp][(n+63)/64] bit i%64 of word i/64 = vbCurrentInliers[i]; bits >= n are 0 */
} orbx_mono_init_job;
/* The whole table of FindHomography and FindFundamental.  One upload, one launch, one download.  ORBX_E_INVALID before any device
 * work: a NULL job or array, n outside [8, 8192], n1 or n2 outside [n, 65535], n_hyp outside [1, 1024], a match index outside its
 * frame, firsts not strictly rising, a sample index outside [0, n), a row of samples with two equal indices. */
int orbx_mono_init_hypotheses(int device, orbx_mono_init_job *job);
typedef struct {
    int ok;                         /* the return value of ReconstructH / ReconstructF */
    int winner;                     /* the row the decision settled on ("decide"), -1 none */
    int32_t n_good[8];              /* nGood of CheckRT per motion hypothesis: 8 rows for H, 4 for F (the others 0) */
    float cos_parallax[8];          /* "rank" above */
    float R[8][9], t[8][3];         /* the motion hypotheses, R row major; zero for rows that do not exist */
    float *P3D;                     /* [n1][3] vP3D */
    uint8_t *triangulated;          /* [n1] vbTriangulated */
} orbx_mono_init_recon;
/* ReconstructH (model = 1, M = H21) or ReconstructF (model = 2, M = F21) on a model and an inlier mask[(n+63)/64] of the caller's
 * choosing; job gives the keypoints, the matches, sigma, K, min_parallax and min_triangulated.  One upload, two launches on one
 * stream, one download.  ORBX_E_INVALID before any device work: a NULL argument or array, model outside {1, 2}, a mask bit >= n, the
 * refusals of orbx_mono_init_hypotheses that do not concern samples. */
int orbx_mono_init_reconstruct(int device, const orbx_mono_init_job *job, int model, const float *M, const uint64_t *mask,
                               orbx_mono_init_recon *out);
typedef struct {
    int ok;                         /* Initialize's return value */
    int model;                      /* 0 none ("choice"), 1 H, 2 F */
    int best_h, best_f;             /* -1: no hypothesis scored above 0 */
    float SH, SF;
    float M[9];                     /* H21 of best_h or F21 of best_f by model; zero for model 0 */
    float R21[9], t21[3];           /* the winner's motion when ok, else zero */
    float parallax;                 /* degrees, (float)(acos((double)cos_parallax[winner]) * 180 / CV_PI) on the host; 0 without a winner */
    int winner;
    int32_t n_good[8];
    float cos_parallax[8];
    float *P3D;                     /* [n1][3] */
    uint8_t *triangulated;          /* [n1] */
} orbx_mono_init_result;
/* Initialize (:52-145) behind the drawing of mvSets: the table, the choice, the decomposition, CheckRT of every motion hypothesis
 * and the decision as three launches chained on one stream with no host step between them; one upload, and only the result comes
 * down.  Everything it returns is byte-equal to orbx_mono_init_reconstruct on the winner of orbx_mono_init_hypotheses.  The table
 * outputs of job are not written.  ORBX_E_INVALID as orbx_mono_init_hypotheses, and for a NULL res or array of it. */
int orbx_mono_init_initialize(int device, orbx_mono_init_job *job, orbx_mono_init_result *res);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (src/ORBmatcher.cc:1396-1553;
 * Tracking::TrackWithMotionModel).  direction: 0 none, 1 bForward, 2 bBackward (:1412-1413).  match_cur[cur->n] =
 * index of the point each current feature finally holds (-1 none); *nmatches = the reference's return value
 * (it counts every accepted point, also one whose feature a later point overwrote).
 * check_orientation: 0 off, 1 on, 3 on + a feature whose match the rotation filter cleared reads -2 instead of -1: the
 * reference sets CurrentFrame.mvpMapPoints[...] = NULL there (:1526-1545), which differs from "never matched" when the
 * feature held a point before the call; the same two bits in orbx_search_by_projection_keyframe (:1660-1680). */
int orbx_search_by_projection_last_frame(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts,
                                         const float *scale_factors, int nlevels, float th, int direction, float mbf,
                                         int check_orientation, int32_t *match_cur, int *nmatches);
/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:48-129; Tracking::SearchLocalPoints) */
int orbx_search_by_projection_map_points(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts,
                                         const float *scale_factors, int nlevels, float th, float nnratio,
                                         int32_t *match_cur, int *nmatches);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:1555-1685; Tracking::Relocalization).  pts = pKF->GetMapPointMatches() in keypoint order, projected
 * by the adaptor with CurrentFrame.mTcw: u, v (:1588-1589), level = PredictScale (:1607), angle = pKF->mvKeysUn[i].angle,
 * valid = pMP && !isBad() && !sAlreadyFound.count(pMP) && distance range (:1577-1605); aux / view_cos / has_obs unused.
 * cur->occupied = CurrentFrame.mvpMapPoints[i] != NULL; every accepted match blocks its feature (:1624-1625). */
int orbx_search_by_projection_keyframe(int device, const orbx_frame_feats *cur, const orbx_proj_points *pts,
                                       const float *scale_factors, int nlevels, float th, int orb_dist,
                                       int check_orientation, int32_t *match_cur, int *nmatches);
/* ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, th)
 * (src/ORBmatcher.cc:305-415; LoopClosing::ComputeSim3).  pts = vpPoints projected with Scw (:336-352), level = PredictScale
 * (:374), valid = !isBad() && !spAlreadyFound.count(pMP) && depth > 0 && distance range && viewing angle (:331-372); the
 * IsInImage test (:355) is done here from kf's bounds.  kf->occupied = vpMatched[idx] != NULL.  match_kf[kf->n] = the
 * point this call writes to vpMatched[idx], or -1. */
int orbx_search_by_projection_sim3(int device, const orbx_frame_feats *kf, const orbx_proj_points *pts,
                                   const float *scale_factors, int nlevels, float th, int32_t *match_kf, int *nmatches);
/* The search half of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:873-1038; chi2 = 1,
 * max_dist = TH_LOW 50, aux = ur = u - bf*invz, inv_sigma2 = pKF->mvInvLevelSigma2), of Fuse(KeyFrame*, Scw, vpPoints, th,
 * vpReplacePoint) (:1040-1164; chi2 = 0, max_dist = 50) and of each direction of SearchBySim3 (max_dist = TH_HIGH 100):
 * best_idx[pts->n] = most similar keypoint of kf inside the window with octave in [level-1, level] whose distance is
 * <= max_dist, else -1; best_dist (may be NULL) its distance; *nfound = points with a result.  Points do not interact;
 * Replace / AddObservation / vpReplacePoint stay with the adaptor, which also re-checks isBad()/IsInKeyFrame() as
 * it walks the results in order (those flags can change through its own Replace calls). */
int orbx_window_best(int device, const orbx_frame_feats *kf, const orbx_proj_points *pts, const float *scale_factors,
                     const float *inv_sigma2, int nlevels, float th, int chi2, int max_dist, int32_t *best_idx,
                     int32_t *best_dist, int *nfound);
/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1166-1394; LoopClosing::ComputeSim3).
 * pts12 = KF1's map points (one entry per KF1 keypoint; valid = has a point, !vbAlreadyMatched1, !isBad(), depth and range
 * tests :1221-1259) projected into KF2 with level = PredictScale(dist3D, pKF2); pts21 the reverse direction.
 * match12[kf1->n] = idx2 where the two directions agree (:1375-1391), else -1; *nfound = the return value. */
int orbx_search_by_sim3(int device, const orbx_frame_feats *kf1, const orbx_frame_feats *kf2, const orbx_proj_points *pts12,
                        const orbx_proj_points *pts21, const float *scale_factors1, const float *scale_factors2, int nlevels,
                        float th, int32_t *match12, int *nfound);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:430-556;
 * Tracking::MonocularInitialization).  prev_matched_xy[f1->n][2] = vbPrevMatched; matches12[f1->n] = vnMatches12;
 * *nmatches = the return value.  The update of vbPrevMatched (:544-546: the matched F2 keypoint's position) is a
 * copy the adaptor does from matches12.  Only level-0 keypoints of either frame take part (:451-455). */
int orbx_search_for_initialization(int device, const orbx_frame_feats *f1, const orbx_frame_feats *f2,
                                   const float *prev_matched_xy, int window_size, float nnratio, int check_orientation,
                                   int32_t *matches12, int *nmatches);

/* ---- Frame::UndistortKeyPoints (src/Frame.cc:470-515) -------------------
 * cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) on n keypoint positions xy[n][2] -> xy_out[n][2] (may alias).
 * fx, fy, cx, cy = mK's float entries; dist_coef = mDistCoef (k1 k2 p1 p2 [k3]).  dist_coef[0] == 0 copies (:472-476).
 * Frame::ComputeImageBounds (:517-552) is the same call on the four image corners followed by min/max on the host. */
int orbx_undistort_keypoints(int device, const float *xy, int n, float fx, float fy, float cx, float cy,
                             const float *dist_coef, int ndist, float *xy_out);

/* ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:266-340) -- */

/* Batched over map points: point p owns descriptors desc[off[p] .. off[p+1]) (its non-bad observations in the
 * reference's std::map iteration order, at most 256 each).  best_idx[p] = index (relative to off[p]) of the
 * descriptor with the smallest median Hamming distance to the others (first wins ties), or -1 for an empty
 * point.  Host pointers. */
int orbx_distinctive_descriptors(int device, const uint8_t *desc, const int32_t *off, int npoints, int32_t *best_idx);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------- */

enum { ORBX_STAGE_RESIZE = 0, ORBX_STAGE_FAST = 1, ORBX_STAGE_TREE = 2, ORBX_STAGE_DESC = 3,
       ORBX_STAGE_STEREO = 4, ORBX_STAGE_STEREO_CUT = 5, ORBX_STAGE_COUNT = 6 };
/* (ORBX_STAGE_STEREO_CUT is kept for the numbering only: the median cut of src/Frame.cc:737-750 now runs inside the stereo launch,
 * in the last workgroup of each pair, and the row table of :584-604 inside the descriptor launch -- their times are part of
 * ORBX_STAGE_STEREO / ORBX_STAGE_DESC and this stage reads 0.) */
/* enable: record HIP events around every kernel launch of this handle (on the launch stream) */
int orbx_profile_enable(orbx_extractor *e, int enable);
/* Which stages record events while profiling is enabled: bit ORBX_STAGE_* (default: all).  An event between two kernels costs a
 * few microseconds of idle GPU (barrier packet), so a throughput measurement selects only the kernel it needs the duration of. */
int orbx_profile_stages(orbx_extractor *e, unsigned stage_mask);
/* synchronises, then returns accumulated kernel time (ms) and launch count per stage since the
 * last reset; arrays of ORBX_STAGE_COUNT entries */
int orbx_profile_read(orbx_extractor *e, float *ms, int *launches, int reset);

/* debug/inspection (used by the parity tests to localise a mismatch): FAST candidates and
 * per-level keypoint counts of image `image_index` of the most recent extract call.
 * x,y are relative to (16,16) like the reference's vToDistributeKeys. */
int orbx_debug_candidates(orbx_extractor *e, int image_index, int level, int32_t *x, int32_t *y, int32_t *resp, int cap, int *n);
int orbx_debug_level_counts(orbx_extractor *e, int image_index, int32_t *counts /*[nlevels]*/);
/* which FAST kernel the most recent extraction launched: 1 = a cell per wave (or several waves per cell), 2 = a pair of cells per wave */
int orbx_debug_fast_form(const orbx_extractor *e);
/* which form each size- and geometry-dependent launch of the handle took: the most recent extraction, and the most recent
 * stereo launch with `e` as the left handle (launches of `e` itself: the pipelined forms run on internal lanes).  Writes the
 * first min(n, 10) fields and returns 10 (the field count):
 *   [0] pyramid regime: 2 = grouped launches, 1 = per level for the big levels + grouped small ones, 0 = one launch per level
 *   [1] FAST waves per cell (1 .. 4; 0 = k_fast2)     [2] FAST grid order: 1 = image-major, 0 = cell-major
 *   [3] quadtree threads (1024, 256)   [4] node tables in LDS (1) or HBM (0)   [5] register point form (1 / 0)
 *   [6] k_desc level template (8, 16)
 *   [7] stereo keypoints per wave (1, 4; 0 = no stereo launch yet)   [8] stereo XCD-owned pair grid (1 / 0)
 *   [9] k_desc row pass: 2 = matrix cores, 1 = vector ALUs (ORBX_DESC_VALU_ROWPASS=1 when the handle was created)
 * All 0 before the first launch. */
int orbx_debug_launch_forms(const orbx_extractor *e, int32_t *out, int n);
/* The per-lane geometry of the FAST kernel's pretest and list phases as the host tabulates it for one detect shape (dw x dh pixels of a cell,
 * tile pitch 48 or 80): out[64][4] = the 64 lanes' 16-byte entries, uni[0] = detect rows per pretest iteration, uni[1] = 1 for half-row list
 * segments.  Entry: [0] pixel mask of the lane's pretest group (0: idle lane); [1] bits 0-15 tile byte offset of the group's centre dword,
 * bits 16-31 byte offset of its bitmap word; [2] bits 0-15 list segment (row << 6 | first bit), bit 16 row exists, bits 24-28 nibble shift;
 * [3] 0.  A pure host function: needs no device. */
int orbx_debug_fast_lane_table(int tile_pitch, int dw, int dh, uint32_t *out, int32_t *uni);
/* The FAST cell records of the handle's current geometry, eight ints per cell: level, skip, ini_x, ini_y, tw, th (rectangle incl. the 3-px
 * halo), level pitch, shape class (the cell's block of the lane table).  Writes them if cap >= the number of cells; returns that number
 * (0 before the first extraction). */
int orbx_debug_fast_cells(const orbx_extractor *e, int32_t *out, int cap);
/* test hook: the SearchByBoW kernels exist in a latency form (one 16-wave workgroup per pair) and a throughput form
 * (LDS distance table + row fixpoint); a call picks by problem size.  form = 1 / 2 forces the wave / table form for
 * every later call of the process, 0 restores the automatic choice.  Both forms return identical matches. */
int orbx_debug_set_bow_form(int form);
/* process-wide, like orbx_debug_set_bow_form: the form the most recent SearchByBoW launch took.  out[0] = 1 wave / 2 table form
 * (0 = none yet), out[1] = 1 if keyframes were placed on XCDs in whole groups, out[2] = 1 for compact (slot, value) lists */
int orbx_debug_bow_last_form(int32_t out[3]);
/* test hook: a per-call matcher search of ONE pair with at most 144 work items hands them to its kernel by value, in the kernel-argument
 * segment (one dependent PCIe read less per call); in_memory = 1 makes such calls read their items from mapped host memory as calls with
 * several pairs do, 0 restores the default.  Both forms return identical matches. */
int orbx_debug_set_match_items(int in_memory);
/* host phases of the calling thread's most recent per-call matcher search (orbx_match.hip), microseconds:
 * [0] prepare (node intersection, participation bytes, packing), [1] launch, [2] wait for the kernel's ticket, [3] copy-out */
int orbx_debug_match_timing(double *out4);
/* measurement hook (tools/bench_lba.py): enable = 1 makes every launch of the calling thread's later orbx_local_bundle_adjustment calls sit
 * between two events and be waited for, its device time going to its kernel's slot; enable = 0 ends that, writes the milliseconds and
 * launch counts gathered since (ms[12], launches[12], either may be NULL) and returns 12, the slot count.  Slots: 0 k_lba_init, 1 k_lba_active,
 * 2 k_lba_points<true>, 3 k_lba_kf, 4 k_lba_reduce, 5 k_lba_prep, 6 k_lba_schur, 7 k_lba_solve, 8 k_lba_update, 9 k_lba_points<false>,
 * 10 k_lba_classify, 11 k_lba_finish.  Results are the same bytes with and without it.  The events belong to the thread's context and go
 * with it (orbx_thread_release, or the thread's end). */
int orbx_debug_lba_profile(int enable, double *ms, int32_t *launches);
/* the same hook for the calling thread's orbx_optimize_essential_graph and orbx_optimize_essential_graph2 calls (tools/bench_eg.py): ms[10],
 * launches[10], returns 10.  Slots: 0 k_eg_setup, 1 k_eg_edges<true>, 2 k_eg_rows, 3 k_eg_reduce, 4 the fill (both phases, in either form),
 * 5 the solve (the panels or the envelope), 6 k_eg_update, 7 k_eg_edges<false>, 8 k_eg_finish, 9 k_eg_points. */
int orbx_debug_eg_profile(int enable, double *ms, int32_t *launches);
/* test hook (tests/test_eg_stages.py): what every kernel of orbx_optimize_essential_graph leaves in device memory.  The problem is checked,
 * staged and set up as in that call and taken through ONE linearisation at the start estimates and, with trial != 0, ONE Levenberg trial
 * from them with the given lambda, by the same launch sequences.  With x_in ([7 F], F = n_kf - 1 free keyframes in keyframe order = the
 * rows) the solve is skipped and x_in is what the update reads.  n = 7 F, E = n_edges, K = n_kf.  Every array may be NULL (not wanted):
 *   behind the setup          vS [K][8] the start estimates; meas [E][8] Sjw * Swi; xf [14][8], xf[2 d] = Sim3(+delta e_d), xf[2 d + 1] =
 *                             Sim3(-delta e_d) (e_6 zeroed under fix_scale).  Every Sim3 is qx qy qz qw tx ty tz s.
 *   behind the linearisation  rec [E][120]: with J = [A | B] (7 x 14, columns 0 .. 6 vertex 0 = edge_i, 7 .. 13 vertex 1 = edge_j; the
 *                             columns of a fixed end are zeros), rec[0 .. 104] = the upper triangle of J^T J in row order (entry (r, c),
 *                             r <= c, at 14 r - r (r - 1) / 2 + (c - r)), rec[105 .. 118] = -J^T e, rec[119] = chi2;  echi [E] = chi2;
 *                             Hd [F][28] the upper triangle of a row's diagonal block in row order (entry (r, c) at 7 r - r (r - 1) / 2 +
 *                             (c - r)); bv [F][7]; *n_pairs = NP, pair [NP][2] = (higher row, lower row) of every pair of free vertices
 *                             an edge joins, sorted by (higher, lower), each once; Off [NP][49], entry [a][c] for dof a of the higher row
 *                             and dof c of the lower one (pair and Off need room for E pairs); status_lin [4] = chi2, 0, the largest
 *                             |diagonal entry|, 0.
 *   err [E][29][7]            from a kernel of this call alone (k_eg_probe), a thread per evaluation, on the same stored estimates,
 *                             measurements and xf: evaluation 0 is the error, 1 + 2 c and 2 + 2 c the plus and the minus side of column c
 *                             of J.  The evaluations of a fixed end, which the linearisation does not make, are zeros.
 *   behind the trial          S [n][n] row major as the fill left it, in front of the solve that factors it in place (lower triangle
 *                             and diagonal; above the diagonal the memory is not written); y [n]; *solve_ok = 1 / 0, or -1 with x_in;
 *                             x [n] behind the update (which zeroes x[7 r + 6] under fix_scale); trial [K][8] the trial estimates;
 *                             sc [F] the rows' x (lambda x + b); echi_trial [E]; status_trial [4] = trial chi2, the sum of sc, the
 *                             largest diagonal entry, solve ok.
 * A graph without an edge or without a free keyframe gets vS, meas, xf and *n_pairs only: the full call runs no iteration on it.
 * Refusals before any device work: those of orbx_optimize_essential_graph for the problem; ORBX_E_INVALID for a NULL dump or a lambda
 * that is negative or not finite; ORBX_E_CAPACITY for S with n > ORBX_EG_STAGES_MAX_N or err with E > ORBX_EG_STAGES_MAX_PROBED. */
#define ORBX_EG_STAGES_MAX_N 1024
#define ORBX_EG_STAGES_MAX_PROBED 4096
typedef struct {
    double *vS, *meas, *xf;
    double *rec, *echi, *Hd, *bv;
    int32_t *n_pairs, *pair;
    double *Off, *status_lin, *err;
    double *S, *y;
    int32_t *solve_ok;
    double *x, *trial, *sc, *echi_trial, *status_trial;
} orbx_eg_stages;
int orbx_debug_eg_stages(int device, const orbx_eg_problem *p, double lambda, const double *x_in /* [7 F], may be NULL */, int trial,
                         orbx_eg_stages *dump);
/* test hooks for the dense LDL^T of the two bundle adjustments.  It exists in two forms that give the same bytes: 0, one workgroup
 * (k_lba_solve, n <= 1536), and 1, panels of orbx_debug_ldlt_panel_width() columns over many workgroups (orbx_ldlt.hip, n <= 12288).
 * orbx_debug_ldlt_solve uploads a dense system (S [n][n] row major, only its lower triangle is read; b [n]) and solves it with the named
 * form: *ok = 1 and x = the solution, or *ok = 0 at a pivot that is not > 0, x as the caller left it.  orbx_debug_set_lba_solver makes the
 * calling thread's later orbx_local_bundle_adjustment calls use the named form (default 0); orbx_bundle_adjustment always uses form 1.
 * With orbx_debug_lba_profile on, slot 7 holds the whole solve in either form, and orbx_bundle_adjustment's two active-set kernels share slot 1. */
int orbx_debug_ldlt_solve(int device, int n, const double *S, const double *b, double *x, int form, int *ok);
int orbx_debug_set_lba_solver(int form);
int orbx_debug_ldlt_panel_width(void);
/* test hook for the envelope form of the panel LDL^T (orbx_ldlt_env.hip, tests/test_ldlt_envelope.py).  S is dense [n][n] row major and
 * first [n] gives every row's first column, 0 <= first[i] <= i, rounded down here to the panel width.  Only the entries first[i] <= j <= i
 * are read: they are packed on the host, uploaded and solved by the envelope solver.  x and *ok as orbx_debug_ldlt_solve; n <= 12288, so
 * that form 1 can be run beside it.  ORBX_E_INVALID for a NULL argument, n < 1 or a first[i] outside 0 .. i. */
int orbx_debug_ldlt_solve_envelope(int device, int n, const int32_t *first, const double *S, const double *b, double *x, int *ok);
/* process-wide: the per-thread search contexts (see orbx_thread_release) that are set up right now, over all threads, families and
 * devices.  A thread's share leaves the count when it calls orbx_thread_release or ends. */
int orbx_debug_thread_contexts(void);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */

/*
 * dvo_amd.h -- C ABI of the MI355X-native dense RGB-D tracking core.
 *
 * Drop-in boundary for ONE path of jesusbriales/dvo_slam: dvo::DenseTracker::match() over
 * dvo::core::RgbdImagePyramid (dvo_core/include/dvo/dense_tracking.h:39-213,
 * dvo_core/include/dvo/core/rgbd_image.h:127-262).  The reference has no FFI layer (its seam is a
 * C++ class using Eigen / cv::Mat / boost::shared_ptr types), so this header declares the POD
 * interface a binding would use; include/dvo_amd/dense_tracking.hpp re-declares the reference's
 * class / field names on top of it.  Plain pointers and sizes only; no exceptions cross the ABI;
 * every entry point returns a dvo_amd_status.
 *
 * Conventions (same as the reference):
 *  - intensity: float32, 0..255 (benchmark_slam.cpp:60-68); depth: float32 metres, NaN = invalid
 *    (surface_pyramid.cpp:65-105); both row-major, same size; width of every used pyramid level must
 *    be a multiple of 4 (the reference's SSE derivative needs this too: rgbd_image_sse.cpp:258).
 *  - 4x4 transforms are column-major double[16] (Eigen::Affine3d::matrix().data()).
 *  - 6x6 matrices are column-major double[36] (symmetric anyway).
 *  - Result transformation maps current-frame points into the reference frame
 *    (dense_tracking.cpp:371: estimate^-1).
 */
#ifndef DVO_AMD_H_
#define DVO_AMD_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVO_AMD_MAX_LEVELS 8
#define DVO_AMD_ABI_VERSION 3

typedef enum {
  DVO_AMD_OK = 0,
  DVO_AMD_ERR_INVALID_ARGUMENT = 1,
  DVO_AMD_ERR_NO_DEVICE = 2,        /* HIP runtime / GPU not usable: the library never falls back to a CPU path */
  DVO_AMD_ERR_HIP = 3,              /* a HIP call failed; see dvo_amd_last_error() */
  DVO_AMD_ERR_OUT_OF_MEMORY = 4,
  DVO_AMD_ERR_INSANE_CONFIG = 5,    /* Config::IsSane() false (dense_tracking_config.cpp:55-58) */
  DVO_AMD_ERR_TOO_FEW_LEVELS = 6,   /* pyramid holds fewer levels than FirstLevel + 1 */
  DVO_AMD_ERR_CAPACITY = 7,         /* caller-provided iteration array too small */
  DVO_AMD_ERR_DEVICE_MISMATCH = 8,
  DVO_AMD_ERR_NAN_INIT = 9,         /* UseInitialEstimate with a NaN transform (dense_tracking.cpp:139 assert) */
  DVO_AMD_ERR_COMM = 10,
  DVO_AMD_ERR_IO = 11,              /* file cannot be opened / read */
  DVO_AMD_ERR_FORMAT = 12           /* file is not what the reader supports (see the reader's comment) */
} dvo_amd_status;

/* DenseTracker::TerminationCriteria::Enum, dense_tracking.h:71-81 */
typedef enum {
  DVO_AMD_TERM_ITERATIONS_EXCEEDED = 0,
  DVO_AMD_TERM_INCREMENT_TOO_SMALL = 1,
  DVO_AMD_TERM_LOGLIKELIHOOD_DECREASED = 2,
  DVO_AMD_TERM_TOO_FEW_CONSTRAINTS = 3,
  DVO_AMD_TERM_UNSET = -1
} dvo_amd_termination;

/* The live fields of DenseTracker::Config (dense_tracking.h:42-69); defaults dense_tracking_config.cpp:27-41.
 * UseWeighting / UseParallel / InfluenceFunction* / ScaleEstimator* are never read by match() and are not mirrored. */
typedef struct {
  int first_level;                /* FirstLevel, default 3 */
  int last_level;                 /* LastLevel, default 1 */
  int max_iterations_per_level;   /* MaxIterationsPerLevel, default 100 */
  double precision;               /* Precision, default 5e-7 */
  double mu;                      /* Mu, default 0 */
  int use_initial_estimate;       /* UseInitialEstimate, default 0 */
  float intensity_derivative_threshold; /* IntensityDerivativeThreshold, default 0 */
  float depth_derivative_threshold;     /* DepthDerivativeThreshold, default 0 */
  /* NOT a field of the reference (ABI version 3): how a pyramid level is cut into wave segments -- where the fp32 sums of a
   * residual pass are cut.  The pass walks the level's SELECTED pixels in scan order (the points PointSelection keeps, compacted
   * like the reference's own array), a wave takes a run of consecutive points in steps of 64.  Like every other field of this
   * struct it is part of what a result is a function of: two trackers with different values agree to summation noise, not bit for
   * bit; under ONE value match(), the batched forms, the queue, the validator's workers and every band count agree bit for bit
   * (tests/test_determinism.py runs under both).
   *   DVO_AMD_GEOMETRY_THROUGHPUT (default): 640x480 levels 3..0 run 4 / 4 / 10 / 10 steps per wave -- on a level of 64 000
   *     pixels or more a wave segment holds as many points as an image row has pixels (ten steps for a 640-pixel row, twenty for
   *     1280; 16 steps where a row is no whole number of steps): long segments amortise a block's prologue and epilogue, and the
   *     four waves of a block, about a row apart, share the lines they gather -- the most pairs per second;
   *   DVO_AMD_GEOMETRY_LATENCY: 1 / 2 / 2 / 4 -- short segments spread a coarse level over more waves: the shortest single
   *     match() (the reference's default deployment is one match() per frame, dvo_ros/src/camera_dense_tracking.cpp:269), a few
   *     per cent fewer pairs per second in large batches. */
  int segment_geometry;
  int reserved;
} dvo_amd_config;
#define DVO_AMD_GEOMETRY_THROUGHPUT 0
#define DVO_AMD_GEOMETRY_LATENCY 1

/* DenseTracker::IterationStats, dense_tracking.h:83-100 */
typedef struct {
  int id;
  int valid_constraints;
  double tdist_loglik;
  double tdist_mean[2];
  double tdist_precision[4];  /* column-major 2x2 */
  double prior_loglik;
  double increment[6];        /* EstimateIncrement (upsilon, omega); valid if has_increment */
  double information[36];     /* EstimateInformation; valid if has_increment */
  int has_increment;          /* 0 for the iteration a level broke out of (TooFewConstraints / LogLikelihoodDecreased) */
  int reserved;
  /* instrumentation (not in the reference): estimate().matrix() of this iteration, column-major 4x4 -- the transform whose
   * float cast the residual stage used (dense_tracking.cpp:263).  The parity tests replay single iterations from it. */
  double estimate[16];
  double initial[16];         /* likewise initial() of this iteration (dense_tracking.cpp:260,302,346: the prior term) */
} dvo_amd_iteration_stats;

/* DenseTracker::LevelStats, dense_tracking.h:103-116 */
typedef struct {
  int id;
  int max_valid_pixels;
  int valid_pixels;
  int termination;      /* dvo_amd_termination */
  int n_iterations;
  int first_iteration;  /* index of the level's first entry in dvo_amd_result.iterations */
} dvo_amd_level_stats;

/* DenseTracker::Result, dense_tracking.h:125-140 */
typedef struct {
  double transformation[16];
  double information[36];
  double loglik;
  int is_nan;                               /* Result::isNaN(), dense_tracking_config.cpp:96 */
  int n_levels;
  dvo_amd_level_stats levels[DVO_AMD_MAX_LEVELS];
  int n_iterations;                         /* entries written */
  int iterations_capacity;                  /* in: size of iterations[] (0 / NULL: per-iteration stats are dropped) */
  dvo_amd_iteration_stats *iterations;      /* caller-provided */
  /* instrumentation (not in the reference) */
  int n_ticks;                              /* host<->device round trips spent */
  int n_residual_passes;                    /* fused warp+residual+normal-equation launches (incl. discarded speculative ones) */
  double alg_bytes;                         /* 56 B x selected points x residual passes */
  double alg_bytes_discarded;               /* the part of alg_bytes spent on speculative passes whose iteration was rolled back */
} dvo_amd_result;

typedef struct dvo_amd_context dvo_amd_context; /* one DenseTracker instance: one HIP stream + scratch; NOT thread-safe */
typedef struct dvo_amd_pyramid dvo_amd_pyramid; /* one RgbdImagePyramid: refcounted, immutable after create, shareable */

int dvo_amd_abi_version(void);
/* The build this binary is: the first 16 hex digits of the sha256 over the compiler flags and every source file and header of
 * the library (dvo_slam_amd/_build.py: source_id; the Makefile passes the same string).  The Python binding refuses a library
 * whose id is not the hash of the sources next to it, and rebuilds it where hipcc exists.  "unknown" for a hand-made build. */
const char *dvo_amd_build_id(void);
const char *dvo_amd_status_string(int status);
/* text of the most recent HIP failure on the calling thread ("" if none) */
const char *dvo_amd_last_error(void);
int dvo_amd_device_count(void);

/* DenseTracker::Config::Config(), dense_tracking_config.cpp:27-41 */
void dvo_amd_default_config(dvo_amd_config *cfg);

/* DenseTracker::DenseTracker(cfg) / configure(), dense_tracking.cpp:54-97 */
int dvo_amd_context_create(int device, const dvo_amd_config *cfg, dvo_amd_context **out);
void dvo_amd_context_destroy(dvo_amd_context *ctx);
/* the HIP device the context was created on */
int dvo_amd_context_device(const dvo_amd_context *ctx, int *device);

/* The reciprocal the warp stage and the t-distribution weights use (dense_tracking_impl.cpp:192,700: _mm_rcp_ps, a ~12-bit
 * approximation whose bits differ between CPU vendors).
 *   DVO_AMD_RCP_EXACT (default): 1 / z of the projection is the exactly truncated quotient, the weight's reciprocal is within
 *     1 ulp: the same on every machine.
 *   DVO_AMD_RCP_HOST_SSE: both are THIS HOST's _mm_rcp_ps, bit for bit, from a table probed on the host when the mode is
 *     switched on (2^11 or 2^12 entries on the Xeons / EPYCs seen so far): residuals and validity decisions are then
 *     bit-identical to the reference's SSE path as this host runs it, and so is every t-distribution weight: the body of a
 *     pass as 7 rcpps(5 + d) with d formed product by product (:669-700), the last V mod 4 by computeWeight's exact division
 *     (:702-706, Q7 -- a small kernel between the two kernels of a tick finds those pixels once the pass has counted V and
 *     leaves what their exact weights add to the pair sums and the moments).  The one exception: a pair tile-sharded over
 *     SEVERAL GPUs keeps the table's weight for those <= 3 pixels (no rank sees the whole level's counts before the
 *     exchange).  Sums are still taken in this library's order, so whole-match parity stays at tolerance level.  Returns
 *     DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error() if the host's instruction does not have the
 *     structure the table assumes, or under DVO_AMD_ACCUM=valu (the mode is built for the default accumulator only); refused
 *     while pairs are queued.
 * DVO_AMD_RCP=host in the environment makes it the default of every new context. */
#define DVO_AMD_RCP_EXACT 0
#define DVO_AMD_RCP_HOST_SSE 1
int dvo_amd_set_reciprocal_mode(dvo_amd_context *ctx, int mode);
int dvo_amd_get_reciprocal_mode(const dvo_amd_context *ctx, int *mode, int *table_mantissa_bits);
int dvo_amd_configure(dvo_amd_context *ctx, const dvo_amd_config *cfg);
int dvo_amd_get_config(const dvo_amd_context *ctx, dvo_amd_config *cfg);

/*
 * RgbdCameraPyramid(w,h,K).create(intensity, depth) + RgbdImagePyramid::build(levels) + everything match() would build
 * lazily (derivatives, point-cloud rays, gather layout): rgbd_image.cpp:141-172,245-296,419-489,534-543.
 * stride is in floats (>= width).  The host overload copies the two base planes H2D; the device overload reads planes that
 * are already resident in HBM on `device` (no PCIe traffic).  All work is enqueued on an internal stream and complete on return.
 */
int dvo_amd_pyramid_create(int device, const float *intensity, const float *depth, int width, int height, int stride,
                           float fx, float fy, float ox, float oy, int levels, double timestamp, dvo_amd_pyramid **out);
int dvo_amd_pyramid_create_from_device(int device, const float *d_intensity, const float *d_depth, int width, int height,
                                       int stride, float fx, float fy, float ox, float oy, int levels, double timestamp,
                                       dvo_amd_pyramid **out);
/*
 * Frame ingest on the device: the pyramid straight from a raw sensor frame, replacing the host-side
 * cv::cvtColor(CV_BGR2GRAY) + convertTo(CV_32F) (benchmark_slam.cpp:60-68, camera_dense_tracking.cpp:219-229) and
 * SurfacePyramid::convertRawDepthImageSse (surface_pyramid.cpp:65-105) in front of RgbdCameraPyramid::create.
 *   image : uint8, `channels` = 1 (gray) or 3 (B,G,R interleaved); image_stride_bytes >= width * channels
 *   depth : uint16, 0 = no measurement -> NaN, else (float)raw * depth_scale (1/5000 for TUM PNGs, 0.001 for OpenNI)
 *   on_device != 0: both pointers are device memory on `device` (no PCIe traffic); else host memory (5 B/px cross PCIe
 *   instead of the 8 B/px of two float planes).
 * Gray conversion is OpenCV's 8-bit rule Y = (1868 B + 9617 G + 4899 R + 8192) >> 14.
 */
int dvo_amd_pyramid_create_raw(int device, const unsigned char *image, int channels, int image_stride_bytes,
                               const unsigned short *depth, int depth_stride, float depth_scale, int on_device, int width,
                               int height, float fx, float fy, float ox, float oy, int levels, double timestamp,
                               dvo_amd_pyramid **out);

/*
 * Many pyramids in one call: dvo_amd_pyramid_create_raw for `count` raw frames that share one geometry, one set of intrinsics
 * and one level count (a caller with several cameras makes one call per camera), optionally with each pyramid's first point
 * selection.  One frame at a time costs about two dozen dependent kernel launches, three small copies and two host
 * synchronisations, and the launch chain, not the pixel work, sets the rate; here the frames share every launch -- the number of
 * launches of a call depends on `levels` alone -- and the call synchronises once, at its end.
 *   images, depths : `count` pointers each, to frames laid out as dvo_amd_pyramid_create_raw's; all in host memory
 *                    (on_device == 0) or all in device memory on `device`
 *   timestamps     : `count` values, or NULL for 0.0
 *   build_selection: 1 = every pyramid leaves the call with the selection for (intensity_threshold, depth_threshold) in its
 *                    cache, exactly as the first dvo_amd_pyramid_select / match with those thresholds would have built it
 *                    (a later match with them builds nothing); 0 = selections are built on first use, as ever
 * The results are `count` ordinary pyramids -- refcounted, immutable, released one by one, accepted by every entry -- and
 * bit-identical, selection included, to the ones dvo_amd_pyramid_create_raw makes from the same frames.
 * DVO_AMD_ERR_INVALID_ARGUMENT (all before DVO_AMD_ERR_NO_DEVICE, with a sentence in dvo_amd_last_error()): count < 1; a NULL
 * pointer, in either array too; everything dvo_amd_pyramid_create_raw rejects; build_selection outside {0, 1}; with
 * build_selection, a non-finite threshold.  After any failure every one of the `count` entries of `out` is NULL and nothing of
 * the call is left on the device's pools' books.
 */
typedef struct dvo_amd_raw_batch {
  int count;                               /* frames, >= 1 */
  const unsigned char *const *images;      /* count pointers, uint8 grey or BGR */
  const unsigned short *const *depths;     /* count pointers, uint16 */
  const double *timestamps;                /* count values, or NULL for 0.0 */
  int channels, image_stride_bytes, depth_stride;
  float depth_scale;
  int on_device;                           /* all frames in host, or all in device memory */
  int width, height;
  float fx, fy, ox, oy;
  int levels;
  int build_selection;                     /* 0 or 1 */
  float intensity_threshold, depth_threshold;   /* used when build_selection != 0 */
} dvo_amd_raw_batch;
int dvo_amd_pyramid_create_raw_batch(int device, const dvo_amd_raw_batch *batch, dvo_amd_pyramid **out /* count entries */);

/*
 * Rectification at ingest: remap tables on the device and a frame ingest that resamples through one.
 *
 * The reference assumes a rectified image: camera_keyframe_tracking.cpp:89 builds its intrinsics from CameraInfo::P, the
 * projection matrix of the rectified camera, and relies on image_proc having run cv::initUndistortRectifyMap + cv::remap on the
 * CPU upstream.  These entries are that step for a caller that holds the sensor's own frame: a dvo_amd_remap is made once per
 * camera, and dvo_amd_pyramid_create_raw_remapped takes every raw frame through it on the way into level 0 -- a frame that is
 * already in HBM never comes back to the host to be rectified.
 *
 * A dvo_amd_remap is an immutable, refcounted, device-resident pair of float planes map_x[n], map_y[n] (n = width * height of
 * the OUTPUT image, row-major, one plane after the other): output pixel i takes its value from position (map_x[i], map_y[i]) of
 * the source image, in pixels, the convention of cv::remap with a CV_32FC1 pair.  It also stores the size of the source it
 * refers to.  Like a pyramid it may be shared between contexts and threads; a pyramid built through it does not retain it (the
 * pyramid holds planes, not positions), so the two may be released in either order.
 *   dvo_amd_remap_create            the two planes from the host (stride in floats, >= width): any map -- a stereo
 *                                   rectification, a fisheye model, a crop or a resize
 *   dvo_amd_remap_create_undistort  the planes computed on the device from the five-coefficient lens model, by the rule below
 *   dvo_amd_remap_info              sizes and n_inside (any output may be NULL)
 *   dvo_amd_remap_download          the two planes back to the host (width * height floats each)
 * k_out, k_src = {fx, fy, ox, oy} of the rectified (output) and the real (source) camera; dist = {k1, k2, p1, p2, k3} in OpenCV's
 * order.  The output obeys dvo_amd_pyramid_create_raw's size rules (width >= 4 and a multiple of 4, height >= 2; for the pyramid
 * entry on every level asked for) and holds at most 2^30 pixels; the source is at least 2x2 and at most 2^20 pixels a side.
 *
 * The undistortion rule.  cv::initUndistortRectifyMap with R = I and newCameraMatrix = k_out, in fp32 throughout and in this
 * order.  (The reference's tree holds no OpenCV, and OpenCV itself works in double and rounds at the end: the order below is this
 * library's rule, as with FLANN above.)  Every operation is fp32 and rounds once -- the library is built with -ffp-contract=off
 * -- and the two divisions are correctly rounded, as in the ray tables of a pyramid level.  For output pixel (u, v):
 *     x  = ((float)u - ox) / fx            y  = ((float)v - oy) / fy                         (k_out)
 *     xx = x*x    yy = y*y    r2 = xx + yy    xy = x*y
 *     rad = ((k3*r2 + k2)*r2 + k1)*r2 + 1
 *     xd = x*rad + ((2p1*xy) + p2*(r2 + (xx + xx)))
 *     yd = y*rad + (p1*(r2 + (yy + yy)) + (2p2*xy))            with 2p1 = 2.0f*p1, 2p2 = 2.0f*p2
 *     map_x = xd*fx_src + ox_src           map_y = yd*fy_src + oy_src                        (k_src)
 *
 * The sampling rule.  For output pixel i with (sx, sy) = (map_x[i], map_y[i]) and a source of sw x sh pixels:
 *  1. inside = sx >= 0 && sx < (float)(sw - 1) && sy >= 0 && sy < (float)(sh - 1).  The test is made in float before any
 *     conversion to int: NaN, +-inf and 1e30 are outside, never an overflow; -0.0 is inside and is position 0.  n_inside counts
 *     these pixels.
 *  2. Outside: intensity 0.0f (cv::remap's BORDER_CONSTANT with a zero border value), depth NaN.
 *  3. Intensity, bilinear on the grey values of the four taps:
 *       x0 = floorf(sx), ax = sx - x0; y0 = floorf(sy), ay = sy - y0;
 *       g00, g01, g10, g11 = the grey values at (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) as floats: the byte itself, or for
 *         a BGR source dvo_amd_pyramid_create_raw's integer rule (1868 B + 9617 G + 4899 R + 8192) >> 14 applied PER TAP (the
 *         library converts the frame to a 1 B/px grey plane once and gathers from that: the same integers);
 *       top = g00 + ax*(g01 - g00), bot = g10 + ax*(g11 - g10), I = top + ay*(bot - top).
 *     The result stays float.  Stated deviation: cv::remap on 8-bit data quantises the weights to 5 bits and rounds the result
 *     to a byte; this rule keeps the fp32 weights and the fp32 value.
 *  4. Depth, nearest and never blended, so that no depth is invented across a discontinuity:
 *       px = floorf(sx + 0.5f), py = floorf(sy + 0.5f), the fp32 sums as written, including where they round up
 *       (0.49999997f + 0.5f is 1.0f); raw 0 -> NaN, else (float)raw * depth_scale.
 * Consequences.  An identity map (sx = u, sy = v, source and output of one size) reproduces dvo_amd_pyramid_create_raw's level-0
 * planes bit for bit except in the last row and the last column, which are outside (0 / NaN).  A valid pixel next to an outside
 * one gets NaN depth derivatives, so the point selection and the gather skip it exactly as they skip the rim of a sensor hole.
 * Every output pixel has one writer and there is no floating-point sum across pixels: the planes do not depend on the launch
 * geometry, and the levels above level 0 are built from them as for any other pyramid.
 *
 * dvo_amd_pyramid_create_raw_remapped is dvo_amd_pyramid_create_raw with the resampling in front: the raw frame has the remap's
 * SOURCE size (image_stride_bytes >= src_width * channels, depth_stride >= src_width), the pyramid has the remap's OUTPUT size,
 * and fx..oy are the intrinsics of the rectified camera, which the pyramid carries (k_out for an undistortion map).  A raw frame
 * from the host is uploaded into a per-device staging area that grows to the largest source seen and is kept.
 *
 * Errors.  DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error(), before a device is looked for: a NULL pointer; a
 * size that breaks the rules above; stride < width; src_width or src_height < 2; a non-finite entry of k_out, k_src or dist, or
 * fx or fy of either camera <= 0; a stride of the raw frame smaller than the remap's source row; depth_scale not > 0; channels
 * other than 1 or 3; levels outside 1..DVO_AMD_MAX_LEVELS.  Then DVO_AMD_ERR_NO_DEVICE without a GPU, and
 * DVO_AMD_ERR_DEVICE_MISMATCH for a remap that lives on another device than `device`.
 *
 * Not covered: lens models other than the five-coefficient one (they come in as tables through dvo_amd_remap_create);
 * remapping float planes.  Depth-to-colour registration is dvo_amd_pyramid_create_raw_registered below.
 */
typedef struct dvo_amd_remap dvo_amd_remap;
int dvo_amd_remap_create(int device, int width, int height, const float *map_x, const float *map_y, int stride, int src_width,
                         int src_height, dvo_amd_remap **out);
int dvo_amd_remap_create_undistort(int device, int width, int height, const float k_out[4], int src_width, int src_height,
                                   const float k_src[4], const float dist[5], dvo_amd_remap **out);
void dvo_amd_remap_retain(dvo_amd_remap *r);
void dvo_amd_remap_release(dvo_amd_remap *r);
int dvo_amd_remap_info(const dvo_amd_remap *r, int *width, int *height, int *src_width, int *src_height, int *n_inside);
int dvo_amd_remap_download(const dvo_amd_remap *r, float *map_x, float *map_y);
int dvo_amd_pyramid_create_raw_remapped(int device, const unsigned char *image, int channels, int image_stride_bytes,
                                        const unsigned short *depth, int depth_stride, float depth_scale, int on_device,
                                        const dvo_amd_remap *remap, float fx, float fy, float ox, float oy, int levels,
                                        double timestamp, dvo_amd_pyramid **out);

/*
 * Depth-to-colour registration at ingest: raw depth in the DEPTH camera's frame and a raw colour image, straight into a pyramid.
 *
 * The reference never sees an unregistered frame: dvo_ros/src/camera_base.cpp:31-33 subscribes to
 * camera/depth_registered/image_rect_raw, the output of depth_image_proc/register on the CPU upstream, and TUM's PNGs were
 * registered by the driver.  A caller that holds the sensor's own two streams has depth in the IR camera's frame: a few
 * centimetres beside the colour camera, with other intrinsics and often another resolution.  This entry is that step on the
 * device: every depth measurement is back-projected, moved into the colour camera and splatted into level 0's depth plane with a
 * nearest-depth test.
 *
 * width, height and fx..oy describe the pyramid's level 0, the colour camera the tracker sees; the size rules are
 * dvo_amd_pyramid_create_raw's.  With remap == NULL the image is width x height and the intensity plane is exactly what
 * dvo_amd_pyramid_create_raw writes.  With a remap the image has the remap's source size, width x height must equal the remap's
 * output size, and the intensity plane is exactly what dvo_amd_pyramid_create_raw_remapped writes.  In both cases the raw depth
 * has reg->depth_width x reg->depth_height elements with depth_stride >= depth_width; it does NOT go through the remap (k_depth
 * is a rectified pinhole camera) but through the rule below.  A raw frame from the host is uploaded into the per-device staging
 * area of the remapped ingest; the depth frame takes its own size there.
 *
 * The registration rule.  Every operation is fp32 and rounds once (-ffp-contract=off); the divisions are correctly rounded.  The
 * host casts rows 0..2 of T to float -- it takes the transform as rigid and checks only that the entries are finite -- and
 * computes mx = fx / fx_d, my = fy / fy_d in float.  For depth pixel (u, v) with raw value d:
 *  1. d == 0: no measurement.  Else z = (float)d * depth_scale, counted in `measurements`.
 *  2. Back-project: rx = ((float)u - ox_d) / fx_d, ry = ((float)v - oy_d) / fy_d, X = rx*z, Y = ry*z.
 *  3. Transform: c = ((T0*X + T1*Y) + T2*z) + T3 per row (cx, cy, cz), the order of the point cloud and of the render.
 *  4. Cull: the measurement is dropped and counted in `behind` unless cz > min_z (false for NaN).  min_z >= 0, so every kept
 *     cz is > 0 and its bit pattern, read as an unsigned word, orders like its value.
 *  5. Project and footprint: uc = (cx*fx)/cz + ox, vc = (cy*fy)/cz + oy.
 *       fill == 0: the footprint is the single pixel floorf(uc + 0.5f), floorf(vc + 0.5f).
 *       fill == 1: hx = fminf(0.5f*(mx*(z/cz)), 4.0f), hy = fminf(0.5f*(my*(z/cz)), 4.0f) (fminf returns the other operand for a
 *         NaN: 4.0f); columns and rows then follow rule 5 of dvo_amd_map_render word for word: ceilf(uc - hx) .. floorf(uc + hx),
 *         and floorf(uc + 0.5f) alone when that range is empty (a footprint narrower than a pixel that holds no centre).
 *     The visibility test is made in float before any conversion to int -- the footprint is visible on an axis iff
 *     last >= 0 && first <= (float)(size - 1); NaN and +-inf are outside -- and the footprint is then clamped to the image.  The
 *     4.0 cap bounds a side at 9 pixel centres.  A measurement is counted in `outside` or in `drawn`.
 *  6. Depth test: every covered pixel of level 0's depth plane keeps the minimum of bits(cz) as an unsigned 32-bit word.  The
 *     plane is first cleared to NaN 0x7FC00000, which lies above every finite pattern: a pixel nothing covers stays NaN and no
 *     resolve pass is needed.  The written depth is cz, metres in the colour camera's frame.  `covered_pixels` counts the non-NaN
 *     pixels afterwards.
 * No value depends on the launch geometry or on the order the atomics land in.  measurements == behind + outside + drawn.
 * Consequence: with T = I, equal sizes and equal intrinsics a measurement lands on its own pixel with cz = z, and the plane is
 * dvo_amd_pyramid_create_raw's (tested for power-of-two and for the synthetic camera's intrinsics; not a theorem for every K).
 * Stated deviations from depth_image_proc/register: it works in double and re-quantises to uint16, and in fill mode it averages
 * the two corner depths and projects the two corners; this rule keeps fp32, the centre's cz and a centred footprint.
 *
 * Errors.  DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error(), before a device is looked for: a NULL reg, image,
 * depth or out; a depth side outside 1..2^20; depth_stride < depth_width; a non-finite entry of k_depth, of the first three rows
 * of T or of fx..oy; fx_d, fy_d, fx or fy <= 0; min_z negative or not finite; fill other than 0 or 1; a remap whose output size
 * differs from width x height; an image stride smaller than the row it must hold; everything dvo_amd_pyramid_create_raw rejects.
 * Then DVO_AMD_ERR_NO_DEVICE without a GPU, and DVO_AMD_ERR_DEVICE_MISMATCH for a remap on another device.
 *
 * Not covered: a distortion model for the depth camera; hole filling beyond the footprint; smoothing (both are what
 * dvo_amd_pyramid_filter_depth does to the pyramid this entry returns: "Depth filtering"); float depth planes.
 */
typedef struct {
  int   depth_width, depth_height;  /* size of the raw depth frame: 1..2^20 a side */
  float k_depth[4];                 /* fx, fy, ox, oy of the depth camera */
  double T[16];                     /* depth camera -> colour camera, column-major 4x4 like every pose here */
  float min_z;                      /* >= 0; a measurement is kept only if its colour-frame z > min_z */
  int   fill;                       /* 0: one pixel per measurement; 1: the measurement's footprint (rule 5) */
} dvo_amd_registration;
typedef struct { long long measurements, behind, outside, drawn, covered_pixels; } dvo_amd_registration_stats;

void dvo_amd_default_registration(dvo_amd_registration *reg);   /* identity T, min_z 0, fill 0, sizes and k_depth zero */
int dvo_amd_pyramid_create_raw_registered(int device, const unsigned char *image, int channels, int image_stride_bytes,
        const unsigned short *depth, int depth_stride, float depth_scale, int on_device,
        const dvo_amd_registration *reg, const dvo_amd_remap *remap /* may be NULL */,
        int width, int height, float fx, float fy, float ox, float oy, int levels, double timestamp,
        dvo_amd_pyramid **out, dvo_amd_registration_stats *stats /* may be NULL */);

void dvo_amd_pyramid_retain(dvo_amd_pyramid *p);
void dvo_amd_pyramid_release(dvo_amd_pyramid *p);
int dvo_amd_pyramid_levels(const dvo_amd_pyramid *p);
double dvo_amd_pyramid_timestamp(const dvo_amd_pyramid *p);
/* RgbdImagePyramid::level(l): size and intrinsics {fx,fy,ox,oy} of a level */
int dvo_amd_pyramid_level_info(const dvo_amd_pyramid *p, int level, int *width, int *height, float k[4]);
/* download one plane of a level: 0 I, 1 Z, 2 Ix, 3 Iy, 4 Zx, 5 Zy (RgbdImage::intensity, depth, *_dx, *_dy) */
int dvo_amd_pyramid_download_plane(const dvo_amd_pyramid *p, int level, int plane, float *dst);
/* PointSelection::select(level) (point_selection.cpp:89-117): number of selected pixels for the thresholds, and optionally
 * the per-pixel mask (1 = selected, row-major) */
int dvo_amd_pyramid_select(dvo_amd_pyramid *p, int level, float intensity_threshold, float depth_threshold, int *count,
                           unsigned char *mask);

/* DenseTracker::match(RgbdImagePyramid& reference, RgbdImagePyramid& current, Result&), dense_tracking.cpp:123-376.
 * T_init (may be NULL) is read only if use_initial_estimate (dense_tracking.cpp:137-144). */
int dvo_amd_match(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, const double *T_init,
                  dvo_amd_result *result);

/* DenseTracker::match(PointSelection& reference, RgbdImagePyramid& current, Result&), dense_tracking.cpp:131-376: the
 * reference pixels are the ones the PointSelection's own predicate keeps (point_selection.h:49-67: z, zdx, zdy valid and a
 * gradient above the thresholds; thresholds of -1 reproduce ValidPointPredicate), whatever thresholds the tracker's
 * configuration holds.  Selections are cached per (pyramid, threshold pair), like a PointSelection caches per level. */
int dvo_amd_match_selection(dvo_amd_context *ctx, dvo_amd_pyramid *reference, float intensity_threshold, float depth_threshold,
                            dvo_amd_pyramid *current, const double *T_init, dvo_amd_result *result);

/*
 * Selection masks: any predicate over the reference pixels.
 *
 * The reference's PointSelection takes any PointSelectionPredicate, and isPointOk sees the pixel's position
 * (point_selection.h:32-37, point_selection.cpp:128-147): a caller may cut out a region, follow a segmentation, keep a region of
 * interest.  Here that decision arrives as a dvo_amd_mask: an immutable, refcounted, device-resident pyramid of byte planes, one
 * per level, row-major, level l of size (width >> l) x (height >> l) under the size rules of dvo_amd_pyramid_create_raw.  Planes
 * are stored normalised: any non-zero input byte is 1 (keep), 0 is drop, and a download returns 0 or 1.  A mask is shareable
 * between contexts and threads and is retained and released independently of any pyramid.  It carries a process-wide 64-bit
 * serial number, never 0 and never reused, which is its identity in a pyramid's selection cache (a released mask's address may
 * come back; its serial does not).
 *
 *   dvo_amd_mask_create          level 0 is given (stride in bytes, >= width), in host memory or -- on_device != 0 -- in device
 *                                memory on `device` (a segmentation network's output tensor); levels 1..levels-1 are derived on
 *                                the device: with DVO_AMD_MASK_ALL pixel (x, y) of level l+1 is kept iff all of (2x, 2y),
 *                                (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1) of level l are kept (the conservative rule for excluding
 *                                things), with DVO_AMD_MASK_ANY iff any of them is.  An odd trailing row of a level has no
 *                                parent, as in the pyramid itself.  The number of kernel launches depends on `levels` alone.
 *   dvo_amd_mask_create_levels   every level is given (planes[l], strides[l] >= width >> l): what a per-level predicate needs
 *   dvo_amd_mask_info            sizes, and kept[l] = the kept pixels of level l for l < levels (any output may be NULL)
 *   dvo_amd_mask_download        one level back to the host, (width >> level) * (height >> level) bytes of 0 / 1
 *
 * Errors of the two create entries.  DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error(), before a device is
 * looked for: a NULL pointer (inside planes / strides too); a size that breaks the pyramid size rules on any level asked for;
 * a stride smaller than the width of its level; levels outside 1..DVO_AMD_MAX_LEVELS; an unknown rule.  Then
 * DVO_AMD_ERR_NO_DEVICE.
 *
 * The predicate of a masked selection is
 *     keep(l, i) = mask[l][i] != 0  &&  ValidPointAndGradientThresholdPredicate(ti, td)(pixel i of level l)
 * with thresholds of -1 leaving validity only, as for dvo_amd_match_selection.  Stated deviation: a pixel with NaN z, zdx or zdy
 * is never selected, whatever the mask says (a reference predicate that admitted such a point would put it into the point list).
 * The mask enters in the select kernel and nowhere else: the compaction, the residual passes and the reducers walk the selected
 * pixels in scan order as they always did, so a masked alignment whose mask keeps what a threshold pair keeps IS the alignment
 * of dvo_amd_match_selection with that pair, bit for bit (tests/test_selection_mask.py).
 *
 * Cache.  A pyramid's selections are keyed by (intensity_threshold, depth_threshold, mask serial), serial 0 meaning no mask.  A
 * masked selection holds planes of its own, not the mask: once built, the mask may be released and the selection stays valid
 * for the life of the pyramid.  A pyramid caches at most DVO_AMD_MAX_MASKED_SELECTIONS masked selections: one more distinct mask
 * returns DVO_AMD_ERR_CAPACITY and leaves the pyramid as it was (unmasked selections are not counted and not limited).  Checked
 * before any device work, in this order: DVO_AMD_ERR_INVALID_ARGUMENT for a mask whose level-0 size differs from the pyramid's
 * or that has fewer levels than the pyramid; DVO_AMD_ERR_DEVICE_MISMATCH for a mask on another device.
 *
 *   dvo_amd_pyramid_select_masked  dvo_amd_pyramid_select behind `mask` (NULL: exactly dvo_amd_pyramid_select); count includes
 *                                  an odd trailing point and out_mask marks it, as there
 *   dvo_amd_match_masked           dvo_amd_match_selection behind `mask`: the queue must be idle, the thresholds given override
 *                                  the configuration's for this call; mask == NULL is exactly dvo_amd_match_selection
 *   dvo_amd_match_many_masked      dvo_amd_match_many with one mask per pair and the configuration's thresholds; masks == NULL
 *                                  or masks[i] == NULL: that pair is unmasked.  The queue retains a mask from submission until
 *                                  that pair's selection has been resolved.  (There is no submit / wait / poll form.)
 * Guarantees, all bit for bit: a pair with a NULL mask gives dvo_amd_match's result; a pair with an all-ones mask gives the
 * unmasked result; any pair's result is a function of its inputs, its mask and the configuration alone, at any max_in_flight
 * and whatever shares the batch (the determinism contract of dvo_amd_match_batch, extended).
 *
 * Not covered: dvo_amd_track_frame, dvo_amd_validate_proposals, dvo_amd_match_banded / _sharded, dvo_amd_residuals,
 * dvo_amd_error_image, the debug and bench entries and the build_selection of dvo_amd_pyramid_create_raw_batch keep their
 * thresholds-only selection and take no mask.  There are no masks on the current side: the current image is gathered wherever
 * the warp lands, which is the reference's behaviour.  (A mask made FROM an alignment's residuals: "Residual masks" below; that
 * entry reads the pyramids' planes and needs neither dvo_amd_residuals nor a selection.)
 */
#define DVO_AMD_MASK_ALL 0
#define DVO_AMD_MASK_ANY 1
#define DVO_AMD_MAX_MASKED_SELECTIONS 8
typedef struct dvo_amd_mask dvo_amd_mask;
int dvo_amd_mask_create(int device, int width, int height, int levels, const unsigned char *mask0, int stride, int on_device, int rule,
                        dvo_amd_mask **out);
int dvo_amd_mask_create_levels(int device, int width, int height, int levels, const unsigned char *const *planes, const int *strides,
                               int on_device, dvo_amd_mask **out);
void dvo_amd_mask_retain(dvo_amd_mask *mask);
void dvo_amd_mask_release(dvo_amd_mask *mask);
int dvo_amd_mask_info(const dvo_amd_mask *mask, int *width, int *height, int *levels, long long *kept /* [levels] */);
int dvo_amd_mask_download(const dvo_amd_mask *mask, int level, unsigned char *dst);
int dvo_amd_pyramid_select_masked(dvo_amd_pyramid *p, int level, float intensity_threshold, float depth_threshold,
                                  const dvo_amd_mask *mask, int *count, unsigned char *out_mask);
int dvo_amd_match_masked(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_mask *mask, float intensity_threshold,
                         float depth_threshold, dvo_amd_pyramid *current, const double *T_init, dvo_amd_result *result);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Point-budget masks: a selection mask built on the device from a resident pyramid.
 *
 * The residual pass walks the compacted selection, so a thinner selection is a cheaper alignment.  The two gradient thresholds
 * thin it only by trial; a budget says how many points to keep, or how to spread them.  dvo_amd_mask_create_budget ranks the
 * pixels of every level of `pyramid` on the device and returns an ordinary dvo_amd_mask (level-0 size, level count and device of
 * the pyramid) that enters wherever a mask enters: dvo_amd_pyramid_select_masked, dvo_amd_match_masked,
 * dvo_amd_match_many_masked.  The pyramid is only read.
 *
 * Saliency.  For pixel i of level l, in fp32, round to nearest, every product and sum rounded by itself (no contraction):
 *     a = Ix*Ix + Iy*Iy
 *     s = a                                   if depth_weight == 0 (the depth term is not formed)
 *     s = a + depth_weight * (Zx*Zx + Zy*Zy)  otherwise
 * The sort key of the pixel is the bit pattern of s as an unsigned 32-bit integer: s >= 0, so integer order is value order,
 * and +inf sorts highest.
 *
 * Candidates.  Pixel i of level l is a candidate iff ValidPointAndGradientThresholdPredicate(intensity_threshold,
 * depth_threshold) keeps it (the predicate of the selection; thresholds of -1 leave validity only), and `within` is NULL or
 * within[l][i] != 0, and s == s.  C_l, the candidates of level l, are ordered by (key descending, pixel index ascending): a
 * total order.
 *
 *   DVO_AMD_BUDGET_TOPK  level l keeps the first min(budget[l], |C_l|) candidates in that order -- exactly that many, whatever
 *                        ties exist: among equal keys the lowest pixel indices.  budget[l] == 0 keeps none, budget[l] < 0 keeps
 *                        every candidate.
 *   DVO_AMD_BUDGET_GRID  level l is cut into cells of cell[l] x cell[l] pixels anchored at (0, 0) (the cells of the last column
 *                        and row may be partial); each cell keeps its first candidate in that order, a cell without a candidate
 *                        keeps nothing.  cell[l] == 1 keeps every candidate.
 * Entries of budget / cell beyond the pyramid's levels are not looked at, and neither is the array of the other rule.
 *
 * Result.  kept[l] (dvo_amd_mask_info) is the number of pixels kept on level l.  Every kept pixel passes the predicate the mask
 * was built with, so tracking behind the mask with those thresholds or with (-1, -1) selects exactly the kept pixels (an odd
 * trailing point stays the selection's business, Q3, as for every mask).  The planes are a function of the pyramid and the
 * options alone.
 *
 * Errors, before any device work, *out NULL on every failure: DVO_AMD_ERR_INVALID_ARGUMENT (reason in dvo_amd_last_error()) for a
 * NULL pointer, an unknown rule, GRID with cell[l] < 1 on a level the pyramid has, a non-finite threshold, a depth_weight that
 * is negative or not finite; then `within` as dvo_amd_pyramid_select_masked checks a mask: DVO_AMD_ERR_INVALID_ARGUMENT for
 * another level-0 size or fewer levels than the pyramid, DVO_AMD_ERR_DEVICE_MISMATCH for another device.
 *
 * Cost.  The number of kernel launches depends on the pyramid's level count and the rule alone (12 per level for TOPK, 2 for
 * GRID); nothing comes back to the host between them -- the digits of the exact radix select over the keys and the tie count
 * are chosen by a device kernel -- and the call synchronises once, at its end.
 *
 * Not covered: whatever takes no mask takes no budget (the list under "Selection masks").
 */
#define DVO_AMD_BUDGET_TOPK 0
#define DVO_AMD_BUDGET_GRID 1
typedef struct dvo_amd_budget_options {
  int rule;                                   /* DVO_AMD_BUDGET_TOPK | DVO_AMD_BUDGET_GRID */
  long long budget[DVO_AMD_MAX_LEVELS];       /* TOPK: points kept on level l; < 0 = every candidate of that level */
  int cell[DVO_AMD_MAX_LEVELS];               /* GRID: cell edge in pixels of level l, >= 1 (1 = every candidate) */
  float intensity_threshold, depth_threshold; /* the predicate that makes a pixel a candidate */
  float depth_weight;                         /* >= 0, finite */
  const dvo_amd_mask *within;                 /* optional: candidates only where this mask keeps */
} dvo_amd_budget_options;
/* TOPK, every budget -1, every cell 1, thresholds 0, depth_weight 0, within NULL */
void dvo_amd_default_budget_options(dvo_amd_budget_options *opt);
int dvo_amd_mask_create_budget(dvo_amd_pyramid *pyramid, const dvo_amd_budget_options *opt, dvo_amd_mask **out);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Mask operations: combine two masks, grow or shrink one, carry one onto another frame -- on the device.
 *
 * What a user of a segmentation mask does next: "not a person" AND "a GRID budget"; dilate a border that is never pixel-exact;
 * take the mask of the keyframe the network saw to the frame it did not see.  Every entry below reads its inputs only and
 * returns a new dvo_amd_mask -- immutable, refcounted, with a serial of its own -- that enters wherever a mask enters.  *out is
 * NULL on every failure.  Argument errors (DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error(), then
 * DVO_AMD_ERR_DEVICE_MISMATCH) are reported before any device work and before DVO_AMD_ERR_NO_DEVICE.  The number of kernel
 * launches does not depend on the content, only on the level count at most: each call is ONE launch (combine and morph over all
 * levels, warp over all pairs and levels of the call), and it synchronises once, at its end.
 *
 * dvo_amd_mask_combine(a, b, op, out).  Level by level, out[l][i] = op(a[l][i] != 0, b[l][i] != 0) with op one of
 *     DVO_AMD_MASK_AND      a && b
 *     DVO_AMD_MASK_OR       a || b
 *     DVO_AMD_MASK_ANDNOT   a && !b
 *     DVO_AMD_MASK_NOT      !a         (b must be NULL; for every other op b must not be)
 * a and b must have the same level-0 size and the same level count (else INVALID_ARGUMENT) and live on one device (else
 * DEVICE_MISMATCH).
 *
 * dvo_amd_mask_morph(mask, op, radius, out).  op is DVO_AMD_MASK_DILATE or DVO_AMD_MASK_ERODE, the structuring element of level l
 * the square of edge 2 * radius[l] + 1.  With W(x, y) the window around (x, y) CLIPPED TO THE PLANE:
 *     dilate   out[l](x, y) = 1  iff  any pixel of W(x, y) is kept in mask[l]
 *     erode    out[l](x, y) = 1  iff  every pixel of W(x, y) is kept in mask[l]
 * Pixels outside the plane have no vote (OpenCV's default border for both operations), so erode(m) == NOT dilate(NOT m).
 * radius[l] == 0 copies the level; a radius at least as large as the plane saturates it and is no error.
 * 0 <= radius[l] <= DVO_AMD_MASK_MAX_RADIUS on every level the mask has, else INVALID_ARGUMENT; entries beyond the mask's levels
 * are not read.  Every level is processed on its own from the same level of the input: that is NOT morphing level 0 and deriving
 * the coarser levels again (a caller who wants that downloads level 0 of the result and calls dvo_amd_mask_create).  A radius of
 * r0 pixels of level 0 is (r0 + (1 << l) - 1) >> l pixels of level l, rounded up.
 *
 * dvo_amd_mask_warp_many(n, masks, sources, targets, T, opt, out, counts); dvo_amd_mask_warp is the case n = 1.  masks[k], a mask
 * on the pixels of the pyramid sources[k], is carried onto the pixels of the pyramid targets[k].  T: n x 16 doubles, column-major
 * like every transformation of this interface; T[k] maps points of the TARGET camera frame into the SOURCE camera frame.  For
 * dvo_amd_match(reference = source, current = target) that is result.transformation as returned (dense_tracking.cpp:371 returns
 * the inverse of the estimate).  The output has the target's level-0 size and level count; level l comes from level l of the
 * mask and of both pyramids.  The sizes and intrinsics of source and target may differ.
 * The rule is a gather over the target's pixels -- no scatter, no holes -- and is dvo_amd_covisibility's rule with a = target and
 * b = source.  The host casts rows 0..2 of T to float.  A target pixel (u, v) of level l whose depth z is not finite has the
 * outcome no_target_depth.  Otherwise, in fp32, every operation rounded on its own:
 *     (x, y, z) = (tx[u] z, ty[v] z, z)                          the target level's rays
 *     q         = ((T0 x + T1 y) + T2 z) + T3                    per row of T
 *     !(qz >= near_z)                                            -> behind
 *     pu = floorf(((qx fx) / qz + ox) + 0.5f), pv likewise       the source level's intrinsics
 *     !(0 <= pu <= ws - 1 && 0 <= pv <= hs - 1), tested in float -> outside
 *     Zs = source depth at (pu, pv) is NaN                       -> no_depth
 *     d = Zs - qz, tol = depth_sigmas * (0.0012f + 0.0019f * (qz - 0.4f)^2)
 *     d < -tol -> occluded,  d > tol -> seen_through,  else consistent
 *     out[l](u, v) = masks[k][l][pv * ws + pu] != 0      if consistent
 *                  = opt->inconsistent_keep != 0         if occluded or seen_through
 *                  = opt->unseen_keep != 0               for every other outcome
 * The defaults (near_z 0.1, depth_sigmas 20, unseen_keep 1, inconsistent_keep 1) transport the source's verdicts and add none of
 * their own; inconsistent_keep = 0 drops what moved or was disoccluded between the two frames.
 * counts (may be NULL): for pair k, in pair order, one record of eight long long per level of targets[k]:
 *     valid, behind, outside, no_depth, consistent, occluded, seen_through, dropped_by_source
 * valid = target pixels with a finite depth = the sum of the next six; dropped_by_source = consistent pixels whose source mask
 * byte is 0.  The first seven are dvo_amd_covisibility's of the ordered pair (target, source) at that level.
 * Errors: INVALID_ARGUMENT for a NULL pointer (inside the arrays too), n < 0, a non-finite entry of T, near_z not finite or
 * <= 0, depth_sigmas not finite or < 0, a source with fewer levels than its target, a mask that does not fit its source as
 * dvo_amd_pyramid_select_masked checks it; then DEVICE_MISMATCH unless all objects of the call live on one device.
 *
 * Not covered: there are still no masks on the current side (see "Selection masks").
 */
#define DVO_AMD_MASK_AND 0
#define DVO_AMD_MASK_OR 1
#define DVO_AMD_MASK_ANDNOT 2
#define DVO_AMD_MASK_NOT 3
#define DVO_AMD_MASK_DILATE 0
#define DVO_AMD_MASK_ERODE 1
#define DVO_AMD_MASK_MAX_RADIUS 64
typedef struct dvo_amd_mask_warp_options {
  float near_z;          /* > 0, finite */
  float depth_sigmas;    /* >= 0, finite */
  int unseen_keep;       /* the output where the target pixel has no depth or lands behind, outside or on no depth */
  int inconsistent_keep; /* the output where the two depths disagree (occluded, seen_through) */
} dvo_amd_mask_warp_options;
/* near_z 0.1, depth_sigmas 20, unseen_keep 1, inconsistent_keep 1 */
void dvo_amd_default_mask_warp_options(dvo_amd_mask_warp_options *opt);
int dvo_amd_mask_combine(const dvo_amd_mask *a, const dvo_amd_mask *b, int op, dvo_amd_mask **out);
int dvo_amd_mask_morph(const dvo_amd_mask *mask, int op, const int *radius /* [levels] */, dvo_amd_mask **out);
int dvo_amd_mask_warp(const dvo_amd_mask *mask, const dvo_amd_pyramid *source, const dvo_amd_pyramid *target, const double *T,
                      const dvo_amd_mask_warp_options *opt, dvo_amd_mask **out, long long *counts /* [levels][8] or NULL */);
int dvo_amd_mask_warp_many(int n, const dvo_amd_mask *const *masks, const dvo_amd_pyramid *const *sources,
                           const dvo_amd_pyramid *const *targets, const double *T, const dvo_amd_mask_warp_options *opt,
                           dvo_amd_mask **out, long long *counts /* packed in pair order, or NULL */);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Residual masks: a mask from what the tracker itself knows -- the inliers of an alignment's residuals, on the device.
 *
 * After an alignment the pixels whose residuals the t-distribution down-weights are the moving objects, the specular surfaces and
 * the depth ghosts.  dvo_amd_mask_from_residuals keeps the others, so that
 *     match -> inlier mask -> dvo_amd_mask_morph (erode) -> dvo_amd_mask_warp to the next keyframe -> dvo_amd_match_masked
 * needs no segmentation network and nothing leaves the device between the steps.  The result is an ordinary dvo_amd_mask --
 * immutable, refcounted, with a serial of its own -- of the REFERENCE's level-0 size and level count; *out (every out[k]) is NULL
 * on every failure.  A call is ONE kernel launch for all its pairs and levels and synchronises once, at its end.  The context
 * gives its device and its reciprocal mode, nothing else: no tracker slot is used, no selection is built, looked up or cached, and
 * the context's queue need not be idle.
 *
 * dvo_amd_mask_from_residuals_many(ctx, n, references, currents, T, opts, out, counts); dvo_amd_mask_from_residuals is the case
 * n = 1 with the per-pixel distances on request.  T: n x 16 doubles, column-major, reference -> current: the ESTIMATE, exactly
 * what dvo_amd_error_image takes, and the host casts it to float as that entry does.  For dvo_amd_match(reference, current) that
 * is the INVERSE of result.transformation as returned (dense_tracking.cpp:371 returns the inverse of the estimate; see the mask
 * warp above, which takes it as returned).  opts: one dvo_amd_residual_mask_options per pair.  The rule, for pair k, every level l
 * of the reference and every pixel i of that level, with P = opts[k].precision[l] a column-major 2 x 2:
 *     unevaluated   unless z, zdx and zdy of pixel i are all no NaN: ValidPointAndGradientThresholdPredicate(-1, -1) as the select
 *                   kernels test it, the set of pixels a selection can ever keep (the stated deviation of "Selection masks")
 *                       out[l][i] = opts[k].unevaluated_keep != 0
 *     (r0, r1, valid) otherwise: the residual stage of the tracker for that pixel, in round-toward-zero, with the level's K T, wcur,
 *                   wref and bounds as dvo_amd_residuals builds them -- the pair of floats dvo_amd_residuals returns for the
 *                   pixel under thresholds (-1, -1), bit for bit, and valid false exactly where it returns NaN:
 *     invalid       !valid: out of bounds, a NaN among the blended channels, the occlusion test -- and Q3: where the number of
 *                   evaluated pixels of the level is odd, the last of them in scan order, which the tracker's point list never
 *                   reaches (dense_tracking_impl.cpp:169-171)
 *                       out[l][i] = opts[k].invalid_keep != 0
 *     distance      otherwise, in round-to-nearest fp32, every operation rounded on its own, mahalanobis()'s order:
 *                       t0 = r0 P[0] + r1 P[1],  t1 = r0 P[2] + r1 P[3],  d = t0 r0 + t1 r1
 *                   the d whose weight 7 / (5 + d) computeWeightsSse forms; the mean is zero (quirk Q4)
 *     verdict       d <= opts[k].max_distance[l] -> inlier, out = 1; otherwise, a NaN d included -> outlier, out = 0
 * Defaults: precision all 0, which means "not set" and is refused (the caller copies tdist_precision of the last iteration of each
 * level from a dvo_amd_result's statistics); max_distance 9.2103f on every level, -2 ln 0.01, the 99 % point of chi-square with
 * two degrees of freedom; both keeps 0.
 * distance (may be NULL, and so may any distance[l]): distance[l] receives d per pixel of level l, NaN where the pixel is
 * unevaluated or invalid -- the soft form of the mask.
 * counts (may be NULL): for pair k, in pair order, one record of DVO_AMD_RESIDUAL_MASK_COUNTS long long per level of references[k]:
 *     evaluated, invalid, inlier, outlier, kept
 * evaluated = invalid + inlier + outlier; kept = the ones of the output = dvo_amd_mask_info's kept[l].  All counts are integers
 * and no value depends on the launch geometry or on the order atomics land in.
 * Errors, before any device work: DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error() that starts with the entry's
 * name, for a NULL pointer (inside the arrays too); n < 0; a non-finite entry of T; a non-finite entry of a used precision[l] or
 * one that is all zero; a max_distance[l] that is NaN or negative (+inf is allowed); a level of the reference that the current
 * lacks or has in another size (dvo_amd_residuals' check); a context in the host-rcpps reciprocal mode
 * (dvo_amd_set_reciprocal_mode), whose residual stage this entry does not cover.  Then DVO_AMD_ERR_DEVICE_MISMATCH unless both
 * pyramids live on the context's device, then DVO_AMD_ERR_NO_DEVICE.  n == 0 is OK and does nothing.
 *
 * Not covered: the host-rcpps reciprocal mode; a mean other than zero; a distance under another selection than validity (the
 * residual of a pixel does not depend on which other pixels are selected, but Q3's pixel does: it is the validity selection's).
 */
#define DVO_AMD_RESIDUAL_MASK_COUNTS 5 /* evaluated, invalid, inlier, outlier, kept */
typedef struct dvo_amd_residual_mask_options {
  float precision[DVO_AMD_MAX_LEVELS][4]; /* per level: column-major 2 x 2, finite, not all zero on the reference's levels */
  float max_distance[DVO_AMD_MAX_LEVELS]; /* per level: >= 0, +inf allowed */
  int invalid_keep, unevaluated_keep;
} dvo_amd_residual_mask_options;
/* precision all 0 (not set), max_distance 9.2103f on every level, both keeps 0; a NULL opt is a no-op */
void dvo_amd_default_residual_mask_options(dvo_amd_residual_mask_options *opt);
int dvo_amd_mask_from_residuals(dvo_amd_context *ctx, const dvo_amd_pyramid *reference, const dvo_amd_pyramid *current, const double *T,
                                const dvo_amd_residual_mask_options *opt, dvo_amd_mask **out,
                                long long *counts /* [levels][5] or NULL */, float *const *distance /* [levels] host planes or NULL */);
int dvo_amd_mask_from_residuals_many(dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                                     const dvo_amd_pyramid *const *currents, const double *T /* n x 16 */,
                                     const dvo_amd_residual_mask_options *opts /* n */, dvo_amd_mask **out /* n */,
                                     long long *counts /* packed in pair order, or NULL */);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Pose scoring: many candidate transformations of a pair scored at one coarse level, on the device -- seeds for loop closures.
 *
 * The place index answers "which keyframes look like this frame" without a pose; dvo_amd_match is a local method with a basin of
 * a few degrees and centimetres.  After drift, or for a tracker that is lost, neither start dvo_amd_proposals_for_candidates
 * offers lies inside that basin.  dvo_amd_score_poses evaluates a set of hypotheses -- dvo_amd_pose_grid builds the usual one --
 * and dvo_amd_rank_poses hands the best few to dvo_amd_match or dvo_amd_validate_proposals as initial transformations.  It refines
 * no pose, estimates no precision and decides no closure.
 *
 * dvo_amd_score_poses_many(ctx, n, references, currents, m, T, opts, scores) scores pair k = (references[k], currents[k]) under
 * m[k] transformations; dvo_amd_score_poses is the case n = 1.  T: 16 doubles per transformation, column-major, reference ->
 * current (the ESTIMATE, as dvo_amd_mask_from_residuals takes it), packed in pair order: pair 0's m[0], then pair 1's m[1], ...
 * scores receives one dvo_amd_pose_score per transformation in the same order.  Every transformation is cast to float and turned
 * into K T exactly as dvo_amd_mask_from_residuals does.  opts[k] gives ONE level (scoring two levels is two calls), the column-
 * major 2 x 2 precision P of that level, max_distance and invalid_distance.
 *
 * The rule, for pair k, hypothesis j and every pixel i of the reference's level, with (class, d) exactly what "Residual masks"
 * above defines at that T, P and max_distance -- unevaluated / invalid / inlier / outlier, Q3 included: where the number of
 * evaluated pixels of the level is odd, the last of them in scan order is invalid:
 *     unevaluated, invalid   cost nothing by themselves
 *     inlier                 costs q(d)
 *     outlier                (a NaN d included) costs q(max_distance)
 *     q(x) = (uint32) floor(x * 1024.0f) in fp32, and 0 for x < 0 (a precision that is not positive semidefinite).  The product is
 *            exact, so q is a pure function of the bits of d; x <= max_distance <= 1024 gives q <= 2^20.
 * The record of (k, j):
 *     evaluated, invalid, inlier, outlier    pixel counts, evaluated = invalid + inlier + outlier
 *     cost                                   the sum of the pixel costs
 *     total = cost + invalid * q(invalid_distance)      (a negative invalid_distance: q(max_distance))
 * Everything is an integer sum: the result does not depend on the order of summation, on the launch geometry or on atomics, and
 * two runs are bit-identical.  evaluated and the Q3 pixel are properties of the reference level alone, the same for all
 * hypotheses of a pair: ranking by total is ranking by the mean cost with out-of-view pixels charged invalid_distance, and no
 * division appears anywhere.
 *
 * A call makes two kernel launches (the Q3 pixel of each (reference, level), then all pairs and hypotheses) and synchronises once,
 * whatever n and m are.  The context gives its device and its reciprocal mode, nothing else: no tracker slot is used, no selection
 * is built, and the context's queue need not be idle.  The pyramids are only read.
 *
 * Errors, before any device is looked for: DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error() that starts with
 * the entry's name, for a NULL pointer (inside the arrays too); n < 0; m[k] < 1; more than 2^22 hypotheses in a call; a level that
 * is negative or that either pyramid lacks; a level of another size in the current (dvo_amd_residuals' check); a precision with a
 * non-finite entry or all zero (there is no default); max_distance not finite, not > 0 or > 1024; invalid_distance not finite or
 * > max_distance; a non-finite entry of any T; a context in the host-rcpps reciprocal mode (dvo_amd_set_reciprocal_mode), whose
 * residual stage this entry does not cover.  Then DVO_AMD_ERR_DEVICE_MISMATCH, then DVO_AMD_ERR_NO_DEVICE.  n == 0 is OK and does
 * nothing.  On every failure scores is left untouched.
 *
 * dvo_amd_rank_poses(scores, m, k, order, n_out): host-only, needs no device.  order receives the min(k, m) indices of smallest
 * total, smallest first, ties going to the lower index; *n_out their number.
 *
 * dvo_amd_pose_grid(opt, T_centre, T_out, capacity, n_out): host-only, needs no device.  opt holds six (count, step) pairs for
 * xi = (vx, vy, vz, wx, wy, wz), the tangent order of Sophus::SE3d (translation first); every count is odd and >= 1, and axis a
 * takes the values (-(count[a] - 1) / 2 ... (count[a] - 1) / 2) * step[a].  Hypothesis j is Exp(xi_j) * T_centre in double, 16
 * doubles column-major; j runs with wz FASTEST and vx SLOWEST:
 *     j = ((((i_vx * count[1] + i_vy) * count[2] + i_vz) * count[3] + i_wx) * count[4] + i_wy) * count[5] + i_wz
 * The middle index, (count[0] * ... * count[5] - 1) / 2, is T_centre itself, bit for bit: it does not go through Exp.  *n_out is
 * the number of hypotheses; with T_out NULL nothing else is done; otherwise capacity (in transformations) must hold them all.
 * DVO_AMD_ERR_INVALID_ARGUMENT for a NULL opt, T_centre or n_out, an even or non-positive count, a non-finite step or centre, more
 * than 2^22 hypotheses, a capacity that is too small.
 *
 * Not covered: refinement of a pose; tracker state of any kind; the host-rcpps reciprocal mode; more than one level per call; an
 * estimate of the precision (the caller brings one, e.g. tdist_precision of an earlier alignment at that level); the decision
 * whether a candidate is a closure, which stays with dvo_amd_validate_proposals.
 */
typedef struct dvo_amd_pose_score_options {
  int level;              /* the level scored: it must exist in both pyramids */
  float precision[4];     /* column-major 2 x 2, finite, not all zero; no default */
  float max_distance;     /* finite, > 0, <= 1024 */
  float invalid_distance; /* finite, <= max_distance; negative: = max_distance */
} dvo_amd_pose_score_options;
typedef struct dvo_amd_pose_score {
  long long evaluated, invalid, inlier, outlier;
  unsigned long long cost, total;
} dvo_amd_pose_score;
typedef struct dvo_amd_pose_grid_options {
  int count[6];   /* (vx, vy, vz, wx, wy, wz): odd, >= 1 */
  double step[6]; /* metres, radians */
} dvo_amd_pose_grid_options;
/* level 0, precision all 0 (not set), max_distance 9.2103f, invalid_distance -1.0f (= max_distance); a NULL opt is a no-op */
void dvo_amd_default_pose_score_options(dvo_amd_pose_score_options *opt);
int dvo_amd_score_poses(dvo_amd_context *ctx, const dvo_amd_pyramid *reference, const dvo_amd_pyramid *current, int m,
                        const double *T /* m x 16 */, const dvo_amd_pose_score_options *opt, dvo_amd_pose_score *scores /* m */);
int dvo_amd_score_poses_many(dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                             const dvo_amd_pyramid *const *currents, const int *m /* n */, const double *T /* sum(m) x 16 */,
                             const dvo_amd_pose_score_options *opts /* n */, dvo_amd_pose_score *scores /* sum(m) */);
int dvo_amd_rank_poses(const dvo_amd_pose_score *scores, int m, int k, int *order /* min(k, m) */, int *n_out);
int dvo_amd_pose_grid(const dvo_amd_pose_grid_options *opt, const double *T_centre, double *T_out /* capacity x 16, or NULL */,
                      int capacity, int *n_out);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Exposure compensation: the gain and bias between two frames fitted on the device, and a frame's intensity adjusted by them.
 *
 * The tracker assumes that a surface keeps its grey value from one frame to the next; a camera with auto-exposure breaks that, and
 * a loop closure pairs keyframes taken minutes apart.  The t-distribution weights absorb moving objects, not a global gain or bias,
 * which shifts every intensity residual at once.  dvo_amd_estimate_exposure fits  I_ref ~ gain * I_cur + bias  over the pixels both
 * frames see; dvo_amd_pyramid_adjust_intensity returns the current frame with that model applied, an ordinary pyramid that enters
 * wherever a pyramid enters.  Nothing leaves the device but the sums of the fit.
 *
 * dvo_amd_estimate_exposure_many(ctx, n, references, currents, T, masks, opts, out); dvo_amd_estimate_exposure is the case n = 1.
 * Pair k is (references[k], currents[k]) at ONE level L = opts[k].level of both pyramids, whose sizes and intrinsics may differ.
 * T: n x 16 doubles, column-major, reference -> current: the ESTIMATE, exactly as dvo_amd_mask_from_residuals takes it (for
 * dvo_amd_match(reference, current) the INVERSE of result.transformation as returned).  T == NULL is the identity for every pair:
 * what a tracker has before its first match, and enough for the motion between neighbouring frames.  masks may be NULL and so may
 * any masks[k]; a mask lies on the REFERENCE's pixels and must fit the reference as dvo_amd_pyramid_select_masked checks it.
 *
 * The rule for one pair.  Reference pixel i = (u, v) of level L gets an outcome and a landing pixel (pu, pv) in the current's level L
 * exactly as dvo_amd_mask_warp's rule ("Mask operations") gives them with target = reference and source = current, near_z and
 * depth_sigmas from the options: rows 0..2 of T cast to float, every fp32 operation rounded on its own.
 *   1. An outcome other than consistent counts under that outcome (behind, outside, no_depth, occluded, seen_through), and the pixel
 *      is done; a pixel without a finite depth counts nowhere.  valid = the sum of the six outcomes, as in dvo_amd_covisibility.
 *   2. With a mask whose byte at i on level L is 0 the pixel counts as masked.
 *   3. y = I_ref[i], x = I_cur[pv * ws + pu]: the nearest sample, never blended.  Unless min_intensity <= x <= max_intensity and
 *      min_intensity <= y <= max_intensity the pixel counts as saturated (a NaN compares false and lands here).
 *   4. Every other pixel is a candidate, quantised as X = (long long) rintf(x * scale), Y = (long long) rintf(y * scale): the
 *      product rounded in fp32, round to nearest, then to the nearest integer, ties to even.
 *   5. Pass 0 uses every candidate.  Pass p >= 1 uses the candidates with
 *          fabsf(((float) gain * x + (float) bias) - y) <= trim
 *      for the gain and bias of pass p - 1, every operation rounded on its own (no FMA); the others count as trimmed in that pass.
 *   6. A pass forms n = the pairs used and sx = sum X, sy = sum Y, sxx = sum X X, sxy = sum X Y, syy = sum Y Y as exact 64-bit
 *      integers (a level of more than 2^22 pixels is refused and |bound| * scale <= 2^20, so sxx <= 2^62).
 *   7. The host forms three exact integers in 128 bits,
 *          det = n sxx - sx sx,   ng = n sxy - sx sy,   nb = sy sxx - sx sxy,
 *      and from them, every conversion of a 128-bit integer to double correctly rounded,
 *          gain = (double) ng / (double) det
 *          bias = ((double) nb / (double) det) / (double) scale
 *          r2   = ((double) ng / (double) det) * ((double) ng / (double) dety),  dety = n syy - sy sy;  0 if dety <= 0
 *   8. A pass is degenerate with code 1 if n < min_pairs, else 2 if det <= 0, else 3 if the gain is not finite or outside
 *      [min_gain, max_gain].  The estimate ends there with gain 1, bias 0, r2 0 and the code.
 * There are refits + 1 passes unless one is degenerate.  The record:
 *     gain, bias, r2, passes, degenerate     the last pass's fit; passes = the passes that formed sums, the degenerate one included
 *     valid ... seen_through                 dvo_amd_covisibility's seven counts of the ordered pair (reference, current) at level L
 *     masked, saturated, candidates          consistent = masked + saturated + candidates
 *     used, trimmed                          of the last pass: candidates = used + trimmed
 *     n, sx, sy, sxx, sxy, syy               the last pass's sums; n == used
 *     gain_pass[p], bias_pass[p], used_pass[p]   per pass p < passes (1 and 0 for a degenerate pass); 0 beyond
 * Every sum is an integer: no value depends on the launch geometry or on the order atomics land in, and two runs are bit-identical.
 *
 * What the fit is and is not.  It is ordinary least squares of y on x, and x carries the sensor's noise: the gain comes out low by
 * about var(noise) / var(texture), half a percent for 1.5 grey levels of noise on the synthetic sensor frames (regression dilution,
 * a property of least squares that the refits do not remove).  Pixels the exposure clipped are kept out by the intensity bounds on
 * both sides; what moved between the frames, and what the estimate T misplaces on strong texture, is kept out by the trim.
 *
 * One kernel launch per pass serves all pairs of a call: refits_max + 1 launches and as many synchronisations, whatever n is.  The
 * context gives its device and nothing else: no tracker slot is used, no selection is built, and the context's queue need not be
 * idle.  The pyramids and masks are only read.
 *
 * Errors, before any device is looked for: DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error() that starts with the
 * entry's name, for a NULL pointer (inside the arrays too; T, masks and masks[k] may be NULL); n < 0; a level that is negative or
 * that either pyramid lacks; a reference level of more than 2^22 pixels; an option outside the range its field states below; a
 * non-finite entry of T; a mask that does not fit its reference.  Then DVO_AMD_ERR_DEVICE_MISMATCH unless pyramids and masks live on
 * the context's device, then DVO_AMD_ERR_NO_DEVICE.  n == 0 is OK and does nothing.  On every failure out is left untouched.
 *
 * dvo_amd_pyramid_adjust_intensity_many(n, p, gain, bias, out); dvo_amd_pyramid_adjust_intensity is the case n = 1.  Level 0's
 * intensity becomes ((float) gain[k] * I) + (float) bias[k], product and sum rounded separately, and is NOT clamped.  out[k] is a new
 * ordinary pyramid with the input's depth bit for bit, its timestamp, intrinsics and level count, and every other plane what the
 * builder derives: plane for plane the pyramid dvo_amd_pyramid_create makes of those two level-0 planes.  All items of a call, of
 * any sizes, share ONE launch; the entries take no context and run on the device's internal stream, like the depth filter.  The
 * inputs are only read.  Errors: INVALID_ARGUMENT for a NULL pointer (inside the array too), n < 0, a gain or bias that is not
 * finite; then DEVICE_MISMATCH unless all pyramids live on one device; then NO_DEVICE.  Every out[k] is NULL on failure.
 *
 * Not covered: affine parameters inside the Gauss-Newton step (the fit runs before the alignment, at an estimate); a per-pixel or
 * vignetting model; an estimate without depth on both sides; a clamp of the adjusted values; dvo_amd_track_frame and the validator
 * do not compensate by themselves -- the caller adjusts the pyramid first.
 */
#define DVO_AMD_EXPOSURE_MAX_REFITS 8
typedef struct dvo_amd_exposure_options {
  int level;                          /* the level fitted: it must exist in both pyramids */
  float near_z, depth_sigmas;         /* the covisibility rule's: near_z finite, > 0; depth_sigmas finite, >= 0 */
  float min_intensity, max_intensity; /* both sides; finite, min <= max, |.| * scale <= 2^20 */
  float scale;                        /* quantisation: finite, > 0 */
  float trim;                         /* grey levels; > 0, +inf allowed (no trimming) */
  int refits;                         /* 0..DVO_AMD_EXPOSURE_MAX_REFITS */
  long long min_pairs;                /* >= 2 */
  double min_gain, max_gain;          /* finite, 0 < min <= max */
} dvo_amd_exposure_options;
typedef struct dvo_amd_exposure_estimate {
  double gain, bias, r2;
  int passes, degenerate;
  long long valid, behind, outside, no_depth, consistent, occluded, seen_through, masked, saturated, candidates;
  long long used, trimmed;
  long long n, sx, sy, sxx, sxy, syy;
  double gain_pass[DVO_AMD_EXPOSURE_MAX_REFITS + 1], bias_pass[DVO_AMD_EXPOSURE_MAX_REFITS + 1];
  long long used_pass[DVO_AMD_EXPOSURE_MAX_REFITS + 1];
} dvo_amd_exposure_estimate;
/* level 0, near_z 0.1, depth_sigmas 20, intensities 4..251, scale 16, trim 12, refits 4, min_pairs 64, gains 0.25..4; a NULL opt is
 * a no-op */
void dvo_amd_default_exposure_options(dvo_amd_exposure_options *opt);
int dvo_amd_estimate_exposure(dvo_amd_context *ctx, const dvo_amd_pyramid *reference, const dvo_amd_pyramid *current,
                              const double *T /* 16, or NULL */, const dvo_amd_mask *mask /* or NULL */,
                              const dvo_amd_exposure_options *opt, dvo_amd_exposure_estimate *out);
int dvo_amd_estimate_exposure_many(dvo_amd_context *ctx, int n, const dvo_amd_pyramid *const *references,
                                   const dvo_amd_pyramid *const *currents, const double *T /* n x 16, or NULL */,
                                   const dvo_amd_mask *const *masks /* n, or NULL */, const dvo_amd_exposure_options *opts /* n */,
                                   dvo_amd_exposure_estimate *out /* n */);
int dvo_amd_pyramid_adjust_intensity(const dvo_amd_pyramid *p, double gain, double bias, dvo_amd_pyramid **out);
int dvo_amd_pyramid_adjust_intensity_many(int n, const dvo_amd_pyramid *const *p, const double *gain /* n */,
                                          const double *bias /* n */, dvo_amd_pyramid **out /* n */);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Depth fusion: the depth of the frames tracked against a keyframe averaged into the keyframe, on the device.
 *
 * A keyframe's depth plane is one raw sensor frame with that frame's noise, and everything that follows is tracked against it.
 * The frames tracked against it measured the same surfaces again, and their poses relative to it are what dvo_amd_match returned.
 * dvo_amd_pyramid_fuse_depth_many(n_keyframes, keyframes, frame_offsets, frames, T, opt, out, ...) carries each frame's depth onto
 * its keyframe's pixels by dvo_amd_covisibility's rule and averages what agrees, weighted by the inverse variance of the sensor
 * model; dvo_amd_pyramid_fuse_depth is the case n_keyframes = 1.  Keyframe j owns frames[frame_offsets[j] .. frame_offsets[j+1])
 * and the transformations at the same positions of T (16 doubles each, column-major).  The entries take no context: like the mask
 * operations they run on the device's internal stream, use no tracker slot, and may be called while pairs are queued elsewhere.
 * (The reference has no counterpart: it tracks against the raw keyframe.)
 *
 * The result out[j] is a new ordinary pyramid -- immutable, refcounted, accepted by every entry that accepts a pyramid -- with the
 * keyframe's size, intrinsics, level count and timestamp.  Its level-0 intensity is the keyframe's, bit for bit; its level-0 depth
 * is the fused plane; every other level and plane is what the builder derives from those two: it equals, plane for plane,
 * dvo_amd_pyramid_create called with the same two float planes.  It has no selection yet (the keyframe's cached selections do not
 * carry over).  The inputs are only read.  *out, and in the many form every out[j], is NULL on every failure.  All keyframes of a
 * call are fused in ONE kernel launch and the call synchronises once for it, then as the builder does per keyframe.
 *
 * The rule, operation by operation; the library is built without contraction, so every product, sum and quotient rounds on its
 * own, and divisions are correctly rounded.  T[k] is result.transformation of dvo_amd_match(reference = keyframe, current =
 * frames[k]) AS RETURNED: it maps points of frame k's camera into the keyframe's camera.  The host inverts it as a rigid
 * transformation in double with the summation order of dvo_amd_covisibility's step 1 (Ri = R^T, ti[r] = -((R[0][r] t0 + R[1][r] t1)
 * + R[2][r] t2)) and casts rows 0..2 to float: M, with rows M0..M2 and columns 0..3.  Only level 0 of every pyramid is read; a
 * frame may differ from its keyframe in size, intrinsics and level count.  sigma(z) = 0.0012f + 0.0019f * ((z - 0.4f) * (z - 0.4f))
 * (depthStdDevZ, dense_tracking_impl.cpp:122-128).  For the keyframe pixel (u, v) with depth z0, in fp32:
 *  1. no depth: if z0 is not finite the output depth is NaN and observations = 0; the pixel is not counted in with_depth and no
 *     frame count moves;
 *  2. the keyframe's own observation: w = 1 / (sigma(z0) * sigma(z0)); sw = w; swz = w * z0; n_obs = 0; the pixel counts as
 *     with_depth;
 *  3. for k = 0 .. n - 1, in this order:
 *       (x, y) = (tx[u] * z0, ty[v] * z0)                          the keyframe's level-0 rays
 *       q_r = ((M_r0 * x + M_r1 * y) + M_r2 * z0) + M_r3           per row r; frame k counts `valid`
 *       !(qz >= near_z)                                            -> behind
 *       px = (qx * fx) / qz + ox, py = (qy * fy) / qz + oy         frame k's intrinsics
 *     DVO_AMD_FUSE_NEAREST:
 *       pu = floorf(px + 0.5f), pv = floorf(py + 0.5f)
 *       !(0 <= pu <= w_k - 1 && 0 <= pv <= h_k - 1), in float      -> outside
 *       Zs = Z_k[pv, pu] is NaN                                    -> no_depth
 *     DVO_AMD_FUSE_BILINEAR:
 *       x0 = floorf(px), y0 = floorf(py)
 *       !(0 <= x0 <= w_k - 2 && 0 <= y0 <= h_k - 2), in float      -> outside
 *       a = px - x0, b = py - y0
 *       any of z00, z10, z01, z11 is NaN                           -> no_depth     (column x0 / x0 + 1, row y0 / y0 + 1)
 *       top = z00 + a * (z10 - z00); bot = z01 + a * (z11 - z01); Zs = top + b * (bot - top)
 *     then
 *       d = Zs - qz, tol = depth_sigmas * sigma(qz)
 *       d < -tol -> occluded,  d > tol -> seen_through,  else consistent
 *       where consistent: c = (M_20 * tx[u] + M_21 * ty[v]) + M_22   the change of qz per unit of z0
 *       !(c >= min_cos)                                            -> grazing: the pixel contributes nothing
 *       otherwise fused: z_obs = z0 + d / c; w = 1 / (sigma(Zs) * sigma(Zs)); sw = sw + w; swz = swz + w * z_obs; n_obs += 1
 *  4. output: fusedz = swz / sw.  If n_obs >= min_observations the depth is fusedz and the pixel counts as confirmed; otherwise
 *     the depth is NaN when drop_unconfirmed != 0 (unconfirmed_dropped) and fusedz when it is 0 (unconfirmed_kept).
 *     observations[v * w + u] = n_obs (n <= DVO_AMD_FUSE_MAX_FRAMES: it fits a byte).
 * frame_counts (may be NULL): DVO_AMD_FUSE_FRAME_COUNTS long long per (keyframe, frame), in frame order over the packed list:
 *     valid, behind, outside, no_depth, consistent, occluded, seen_through, fused
 * valid = keyframe pixels with a finite depth = the sum of the next six; grazing = consistent - fused.  With DVO_AMD_FUSE_NEAREST
 * the first seven are dvo_amd_covisibility's counts at level 0 for the ordered pair (keyframe, frame) at those poses, near_z and
 * depth_sigmas.
 * keyframe_counts (may be NULL): DVO_AMD_FUSE_KEYFRAME_COUNTS long long per keyframe:
 *     with_depth, confirmed, unconfirmed_kept, unconfirmed_dropped
 * with_depth is the sum of the other three.  observations (may be NULL; in the many form any entry may be NULL): host memory, w * h
 * bytes per keyframe.  All counts are integers and every pixel's sums are taken in frame order: no value depends on the launch
 * geometry, on the order atomics land in or on what else is in the call.
 * n = 0 is legal (frames and T may then be NULL): the result is (w * z0) / w wherever z0 is finite.  A keyframe among its own
 * frames and a frame repeated are legal.  n_keyframes == 0 is DVO_AMD_OK and does nothing.
 * Errors, in this order and before any device work.  DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error() that starts
 * with the entry's name: a NULL pointer (inside the arrays too; frames and T only where the call has frames); n < 0 or
 * n > DVO_AMD_FUSE_MAX_FRAMES for a keyframe; n_keyframes < 0; offsets that do not start at 0 or that decrease; a non-finite entry of
 * T; near_z or min_cos not finite or <= 0; depth_sigmas not finite or < 0; an unknown sample; min_observations outside
 * 0 .. DVO_AMD_FUSE_MAX_FRAMES.  Then DVO_AMD_ERR_DEVICE_MISMATCH unless every object of the call lives on one device, then
 * DVO_AMD_ERR_NO_DEVICE.
 *
 * Not covered: holes are not filled (a keyframe pixel without depth stays without); no per-pixel variance is kept in the pyramid
 * (sw is dropped after the division); the intensity is not fused; the frames' levels above 0 are not read.
 */
#define DVO_AMD_FUSE_BILINEAR 0
#define DVO_AMD_FUSE_NEAREST 1
#define DVO_AMD_FUSE_MAX_FRAMES 255
#define DVO_AMD_FUSE_FRAME_COUNTS 8    /* valid, behind, outside, no_depth, consistent, occluded, seen_through, fused */
#define DVO_AMD_FUSE_KEYFRAME_COUNTS 4 /* with_depth, confirmed, unconfirmed_kept, unconfirmed_dropped */
typedef struct dvo_amd_fuse_options {
  float near_z;           /* > 0, finite; default 0.1 */
  float depth_sigmas;     /* >= 0, finite; default 5 */
  float min_cos;          /* finite, > 0; default 0.5: see `grazing` */
  int sample;             /* DVO_AMD_FUSE_BILINEAR (default) | DVO_AMD_FUSE_NEAREST */
  int min_observations;   /* 0 .. DVO_AMD_FUSE_MAX_FRAMES; default 0 */
  int drop_unconfirmed;   /* default 0 */
} dvo_amd_fuse_options;
/* near_z 0.1, depth_sigmas 5, min_cos 0.5, BILINEAR, min_observations 0, drop_unconfirmed 0; a NULL opt is a no-op */
void dvo_amd_default_fuse_options(dvo_amd_fuse_options *opt);
int dvo_amd_pyramid_fuse_depth(const dvo_amd_pyramid *keyframe, int n, const dvo_amd_pyramid *const *frames, const double *T,
                               const dvo_amd_fuse_options *opt, dvo_amd_pyramid **out, long long *frame_counts /* [n][8] or NULL */,
                               long long *keyframe_counts /* [4] or NULL */, unsigned char *observations /* host, w*h, or NULL */);
int dvo_amd_pyramid_fuse_depth_many(int n_keyframes, const dvo_amd_pyramid *const *keyframes, const int *frame_offsets /* [n_keyframes+1] */,
                                    const dvo_amd_pyramid *const *frames, const double *T, const dvo_amd_fuse_options *opt,
                                    dvo_amd_pyramid **out, long long *frame_counts, long long *keyframe_counts,
                                    unsigned char *const *observations /* NULL, or n_keyframes pointers each NULL or w*h */);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Depth filtering: one frame's level-0 depth denoised, its unsupported pixels dropped and its small holes filled, on the device.
 *
 * Depth fusion above cures the noise of a keyframe that has had frames tracked against it.  The first keyframe, every current frame
 * and every frame handed to the place index or the map have none: their depth is one raw sensor frame.  The single-frame
 * counterpart is an edge-preserving filter over a (2 radius + 1)^2 window whose range scale is the sensor's own noise model, so that
 * a depth step larger than the noise is never smoothed across; a pixel too few of whose neighbours agree with it (a flying pixel
 * at a depth discontinuity) can be dropped, and a hole can be filled from the farthest surface around it.
 * dvo_amd_pyramid_filter_depth_many(n, p, opt, out, ...) filters n pyramids, which may differ in size, intrinsics and level count;
 * dvo_amd_pyramid_filter_depth is the case n = 1.  The entries take no context: like depth fusion they run on the device's internal
 * stream, use no tracker slot, and may be called while pairs are queued elsewhere.  (The reference has no counterpart.)
 *
 * The result out[j] is a new ordinary pyramid -- immutable, refcounted, accepted by every entry that accepts a pyramid -- with the
 * input's size, intrinsics, level count and timestamp.  Its level-0 intensity is the input's, bit for bit; its level-0 depth is the
 * filtered plane; every other level and plane is what the builder derives from those two: it equals, plane for plane,
 * dvo_amd_pyramid_create called with the same two float planes.  It has no selection yet.  The input is only read.  *out, and in the
 * many form every out[j], is NULL on every failure.  All pyramids of a call are filtered in ONE kernel launch and the call
 * synchronises once for it, then as the builder does per pyramid.
 *
 * The rule, operation by operation; the library is built without contraction, so every product, sum and quotient rounds on its
 * own, and divisions are correctly rounded.  All arithmetic is fp32.
 *   sigma(z) = 0.0012f + 0.0019f * ((z - 0.4f) * (z - 0.4f))      depthStdDevZ, dense_tracking_impl.cpp:122-128
 *   B_r[d] = (float) C(2r, r + d), d = -r .. r                     binomial weights: exact integers (at most 12870), no
 *                                                                  transcendental; their standard deviation is sqrt(r / 2) pixels
 *   ws(dy, dx) = B_r[dy] * B_r[dx]                                 one rounded product
 * Only the input plane Z is read: nothing cascades from pixel to pixel.  For the pixel (u, v) with zc = Z[v, u]:
 *  1. a pixel with depth: zc is finite; the pixel counts in with_depth.  s = range_sigmas * sigma(zc); sw = 0, swd = 0, n = 0.
 *     For dy = -radius .. radius (outer), dx = -radius .. radius (inner), skipping a position outside the plane:
 *       zm = Z[v + dy, u + dx]; d = zm - zc
 *       member iff fabsf(d) <= s                                   (a NaN zm is never a member)
 *       for a member, in this order:
 *         wr = 1.0f - (d * d) / (s * s)
 *         w  = ws(dy, dx) * wr
 *         sw = sw + w; swd = swd + w * d; n = n + 1
 *     The centre is always a member, with wr = 1.
 *  2. keep or drop: if n >= min_support the output is zc + swd / sw and the pixel counts as kept; otherwise the output is NaN and
 *     the pixel counts as dropped.  support[v * w + u] = n (at most 289).
 *  3. a hole: zc is not finite (NaN or an infinity); the pixel counts in holes and support is 0.  With fill_radius == 0 the output
 *     is NaN.  Otherwise, over the (2 fill_radius + 1)^2 window in the same order: zfar is the largest finite zm; if there is none
 *     the output is NaN.  s = range_sigmas * sigma(zfar); sw = 0, swd = 0, n = 0.
 *       member iff zm is finite and zfar - zm <= s
 *       for a member, with ws from B_fill_radius:
 *         sw = sw + ws; swd = swd + ws * (zm - zfar); n = n + 1
 *     If n >= min_fill_support the output is zfar + swd / sw and the pixel counts as filled; otherwise the output is NaN.
 *     (Why the farthest surface: holes in structured-light depth are occlusion shadows, and they lie on the background.)
 *  4. counts (may be NULL): DVO_AMD_DEPTH_FILTER_COUNTS long long per pyramid: with_depth, kept, dropped, holes, filled.
 *     with_depth = kept + dropped; with_depth + holes = w * h; filled <= holes.  All counts are integers and every pixel's sums are
 *     taken in window order: no value depends on the launch geometry, on the order atomics land in or on what else is in the call.
 * Every NaN of the output is the one quiet NaN 0x7FC00000.
 * Consequences.  With radius 0 and fill_radius 0 the output plane is the input plane bit for bit (d = 0, so swd = 0 and
 * zc + 0 / sw = zc), a NaN's payload and the sign of a zero depth apart.  A window whose members all have the same depth leaves
 * that depth bit for bit.  A range_sigmas so small that s * s underflows to 0 makes the centre's quotient 0 / 0: keep it above 1e-15.
 * support (may be NULL; in the many form any entry may be NULL): host memory, w * h unsigned shorts per pyramid.
 * n == 0 is DVO_AMD_OK and does nothing.
 * Errors, in this order and before any device work.  DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error() that starts
 * with the entry's name: a NULL pointer (inside the array too); n < 0; radius or fill_radius outside
 * 0 .. DVO_AMD_DEPTH_FILTER_MAX_RADIUS; range_sigmas not finite or <= 0; min_support outside 1 .. (2 radius + 1)^2; with
 * fill_radius > 0, min_fill_support outside 1 .. (2 fill_radius + 1)^2.  Then DVO_AMD_ERR_DEVICE_MISMATCH unless every pyramid of
 * the call lives on one device, then DVO_AMD_ERR_NO_DEVICE.
 *
 * Not covered: the intensity is not filtered; no per-pixel variance is kept in the pyramid (sw is dropped after the division); the
 * filter is not folded into the ingest kernels (the raw entries are untouched: filter what they return); there is no sensor model
 * other than depthStdDevZ scaled by range_sigmas; a hole wider than the fill window keeps its centre.
 */
#define DVO_AMD_DEPTH_FILTER_MAX_RADIUS 8
#define DVO_AMD_DEPTH_FILTER_COUNTS 5   /* with_depth, kept, dropped, holes, filled */
typedef struct dvo_amd_depth_filter_options {
  int   radius;            /* 0 .. 8; default 2: the window is (2 radius + 1)^2, clipped to the plane */
  float range_sigmas;      /* finite, > 0; default 3 */
  int   min_support;       /* 1 .. (2 radius + 1)^2; default 1 = nothing is ever dropped */
  int   fill_radius;       /* 0 .. 8; default 0 = holes stay holes */
  int   min_fill_support;  /* 1 .. (2 fill_radius + 1)^2 when fill_radius > 0; default 3 */
} dvo_amd_depth_filter_options;
/* radius 2, range_sigmas 3, min_support 1, fill_radius 0, min_fill_support 3; a NULL opt is a no-op */
void dvo_amd_default_depth_filter_options(dvo_amd_depth_filter_options *opt);
int dvo_amd_pyramid_filter_depth(const dvo_amd_pyramid *p, const dvo_amd_depth_filter_options *opt, dvo_amd_pyramid **out,
                                 long long *counts /* [5] or NULL */, unsigned short *support /* host, w*h, or NULL */);
int dvo_amd_pyramid_filter_depth_many(int n, const dvo_amd_pyramid *const *p, const dvo_amd_depth_filter_options *opt,
                                      dvo_amd_pyramid **out, long long *counts /* [n][5] or NULL */,
                                      unsigned short *const *support /* NULL, or n pointers each NULL or w*h */);

/* n independent match() calls advanced in lock step on one GPU (the shape of LocalTracker::update's tbb::parallel_invoke,
 * local_tracker.cpp:184, and of the loop-closure validator's parallel_reduce, keyframe_graph.cpp:576-593).
 * T_inits: n x 16 doubles or NULL.  Results are identical to n dvo_amd_match() calls BIT FOR BIT: a pair's result is a function
 * of its inputs and the configuration alone -- the reference's guarantee for match() calls that run side by side under TBB
 * (keyframe_graph.cpp:587-590, local_tracker.cpp:184).  The same holds for dvo_amd_match_many at any max_in_flight, for the
 * submit / wait / poll queue whatever else is queued, for dvo_amd_validate_proposals at any number of workers, and for
 * dvo_amd_match_banded / dvo_amd_match_sharded at 1, 2, 4, 8 and 16 bands (tests/test_determinism.py): the geometry of a residual
 * pass is the pyramid level's own and every sum across blocks follows one tree per level (csrc/dvo_types.h). */
int dvo_amd_match_batch(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *references, dvo_amd_pyramid *const *currents,
                        const double *T_inits, dvo_amd_result *results);

/* The same n alignments with at most max_in_flight of them resident at a time: a pair that finishes hands its slot to the
 * next pending pair, so every launch stays full although pairs need different numbers of iterations (the shape of the
 * loop-closure validator working through a proposal list, keyframe_graph.cpp:576-593).  max_in_flight <= 0: all n at once. */
int dvo_amd_match_many(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *references, dvo_amd_pyramid *const *currents,
                       const double *T_inits, dvo_amd_result *results, int max_in_flight);
/* ... with one selection mask per pair (see "Selection masks" above) */
int dvo_amd_match_many_masked(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *references, dvo_amd_mask *const *masks,
                              dvo_amd_pyramid *const *currents, const double *T_inits, dvo_amd_result *results, int max_in_flight);

/*
 * The same queue without draining between calls.  A tracker that works through proposals as they come (the loop-closure
 * validator's tbb::parallel_reduce with grain 1 over a proposal list, keyframe_graph.cpp:587-590, called again for every new
 * keyframe, :434-498) keeps `max_in_flight` pairs resident ACROSS calls: dvo_amd_match_submit appends n pairs to the
 * context's queue and returns at once (pairs start as soon as a slot is free), dvo_amd_match_wait drives the queue until every
 * pair of that submission is finished (ticket 0: everything submitted so far), dvo_amd_match_poll advances whatever has
 * landed without waiting for the GPU and reports whether the submission is complete.  dvo_amd_match_many(...) is
 * submit + wait.  Contract: one host thread per context, as for every entry point; `results` (and their iteration arrays)
 * stay valid and untouched until the submission is complete; the queue retains the pyramids itself; the tracker's
 * configuration must not change while pairs are queued (dvo_amd_configure refuses); a different max_in_flight or larger
 * frames than the queue was laid out for let the queued pairs run to completion first.  Results are those of n dvo_amd_match()
 * calls, bit for bit.  While pairs are queued every entry point that works outside the queue in the context's scratch
 * (dvo_amd_match_banded / _sharded, dvo_amd_match_selection, dvo_amd_residuals, dvo_amd_error_image, the debug and bench
 * entries) returns DVO_AMD_ERR_INVALID_ARGUMENT, like dvo_amd_configure.  If a tick fails, every queued pair is dropped,
 * nothing of the context is running any more when the error is returned, and the wait / poll of each submission that was still
 * open then returns that status (a submission that had completed before keeps its OK; ticket 0 returns a failure that no
 * wait / poll has reported yet, once).
 */
int dvo_amd_match_submit(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *references, dvo_amd_pyramid *const *currents,
                         const double *T_inits, dvo_amd_result *results, int max_in_flight, unsigned long long *ticket);
int dvo_amd_match_wait(dvo_amd_context *ctx, unsigned long long ticket);
int dvo_amd_match_poll(dvo_amd_context *ctx, unsigned long long ticket, int *done);

/*
 * One pair tile-sharded over several GPUs (BASELINE config 4).  Every rank holds both pyramids and processes one band of
 * scan-order blocks of every level (whole chunks of the level's summation tree); per Gauss-Newton tick the ranks all-gather
 * one 784-byte record per band over RCCL and fold them along that tree, so every rank runs the identical state machine and
 * returns the identical result -- for 1, 2, 4, 8 and 16 ranks the result of dvo_amd_match() on one GPU, bit for bit (other
 * rank counts: to the rounding of the fp64 sums).
 *   id = dvo_amd_comm_unique_id() on rank 0, broadcast by the caller (torch.distributed, MPI, a file ...);
 *   dvo_amd_comm_create(ctx, id, nranks, rank) on every rank;  dvo_amd_match_sharded(...) on every rank, same arguments.
 * dvo_amd_match_banded runs the same band pipeline with all n_bands bands on ONE GPU (no communicator): it is how the band
 * logic is verified against the unsharded path on a single-GPU box.
 */
int dvo_amd_comm_unique_id(unsigned char *id128);
int dvo_amd_comm_create(dvo_amd_context *ctx, const unsigned char *id128, int nranks, int rank);
void dvo_amd_comm_destroy(dvo_amd_context *ctx);
/* The same exchange without a collective (SURVEY.md 8e "implementation note"): every rank maps every peer's exchange buffer
 * (hipIpc, fine-grained device memory) and its finalize record of a tick is written straight into all of them over xGMI,
 * payload first, a sequence word last; one small kernel per tick pushes, waits (bounded) for the peers' records and forwards
 * them to pinned host memory the host polls: one hop, no D2H copy, no stream synchronisation, deterministic fold in rank
 * order.  dvo_amd_exchange_create on every rank returns the 64-byte handle of its buffer; the caller all-gathers the handles
 * (torch.distributed, MPI, a file ...) and passes all nranks x 64 bytes, in rank order, to dvo_amd_exchange_attach.  Once
 * attached, dvo_amd_match_sharded uses this path; the RCCL communicator above stays available as the fallback. */
int dvo_amd_exchange_create(dvo_amd_context *ctx, int nranks, int rank, unsigned char *handle64);
int dvo_amd_exchange_attach(dvo_amd_context *ctx, const unsigned char *handles);
void dvo_amd_exchange_destroy(dvo_amd_context *ctx);
int dvo_amd_match_sharded(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, const double *T_init,
                          dvo_amd_result *result);
int dvo_amd_match_banded(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, const double *T_init,
                         dvo_amd_result *result, int n_bands);

/*
 * Batched 2-stage loop-closure validation: dvo_slam::constraints::ConstraintProposalValidator::validate
 * (constraint_proposal_validator.cpp:69-166) with the voters of constraint_proposal_voter.cpp:34-186, fed by ONE call: every
 * stage aligns all of its proposals (and the cross-validation inverses) as one batch on the GPU (dvo_amd_match_many), in
 * place of the tbb::parallel_reduce over single proposals in keyframe_graph.cpp:525-593.
 */
/* dvo_slam::TrackingResultEvaluation subclasses (tracking_result_evaluation.cpp:54-67): value(r) */
typedef enum {
  DVO_AMD_EVAL_LOGLIKELIHOOD = 0,            /* -r.LogLikelihood (the one KeyframeTracker creates, keyframe_tracker.cpp:95) */
  DVO_AMD_EVAL_NORMALIZED_LOGLIKELIHOOD = 1, /* -r.LogLikelihood / Levels.back().Iterations.back().ValidConstraints */
  DVO_AMD_EVAL_ENTROPY = 2                   /* log(det(r.Information)) */
} dvo_amd_evaluation_kind;

/* dvo_slam::Keyframe as the validator reads it (id(), image(), pose(), evaluation()) */
typedef struct {
  int id;
  dvo_amd_pyramid *image;
  double pose[16];               /* column-major 4x4 */
  int evaluation_kind;           /* dvo_amd_evaluation_kind */
  double evaluation_average;     /* TrackingResultEvaluation::average_ (sum of the values added so far) */
  double evaluation_n;           /* TrackingResultEvaluation::n_ */
} dvo_amd_keyframe;

typedef enum {
  DVO_AMD_VOTER_ODOMETRY_CONSTRAINT = 0,        /* reject |ref.id - cur.id| <= 1                    (voter.cpp:167-184) */
  DVO_AMD_VOTER_NAN_RESULT = 1,                 /* reject TrackingResult.isNaN()                     (voter.cpp:147-162) */
  DVO_AMD_VOTER_CONSTRAINT_RATIO = 2,           /* ValidConstraints / ValidPixels >= threshold       (voter.cpp:124-142) */
  DVO_AMD_VOTER_TRACKING_RESULT_EVALUATION = 3, /* ratioWithAverage >= threshold, Score = ratio      (voter.cpp:103-119) */
  DVO_AMD_VOTER_CROSS_VALIDATION = 4            /* |t(T_inverse * T)| <= threshold; adds the inverse proposals (voter.cpp:34-97) */
} dvo_amd_voter_kind;

#define DVO_AMD_MAX_VOTERS 8
typedef struct {
  int kind;          /* dvo_amd_voter_kind */
  double threshold;
} dvo_amd_voter;

/* ConstraintProposalValidator::Stage (constraint_proposal_validator.h) */
typedef struct {
  int id;
  int only_keep_best;               /* keepBest() / keepAll() */
  dvo_amd_config tracking_config;
  int n_voters;
  dvo_amd_voter voters[DVO_AMD_MAX_VOTERS];
} dvo_amd_validator_stage;

/* ConstraintProposal::Vote; `value` is the quantity the voter tested (what the reference prints into Vote::Reason) */
typedef struct {
  int voter_kind;
  int reject;       /* Vote::Decision: 0 Accept, 1 Reject */
  double score;
  double value;
} dvo_amd_vote;

/* dvo_slam::constraints::ConstraintProposal: reference / current are indices into the keyframe array */
typedef struct {
  int reference, current;
  double initial_transformation[16];
  dvo_amd_result tracking_result;  /* of the last stage the proposal went through; iterations is ignored (set to NULL) */
  int n_votes;
  dvo_amd_vote votes[DVO_AMD_MAX_VOTERS];
  /* instrumentation (not in the reference), out only: which input proposal a survivor descends from -- its index i in the
   * array passed to dvo_amd_validate_proposals, or -(i + 1) if it is that proposal's cross-validation inverse.  Lets a checker
   * compare a survivor with the alignment of the SAME (reference, current, initial transformation) on its own side. */
  int origin;
  int reserved;
  /* instrumentation, out only: the initial transformation the LAST stage aligned this proposal from (initial_transformation
   * above is updated behind every stage to the inverse of the stage's estimate, validator.cpp:95-100, and the inverse proposals
   * of the cross-validation are formed inside the call): what a checker needs to repeat exactly this alignment */
  double stage_initial_transformation[16];
} dvo_amd_constraint_proposal;

/* the two stages KeyframeGraph builds (keyframe_graph.cpp:500-523) with the tracker configs of configureValidationTracking
 * (:819-838): stage 1 = level 3 only, keepAll, {Odometry, NaN, ConstraintRatio(min_constraint_ratio), Evaluation(ratio_coarse),
 * CrossValidation(1.0)}; stage 2 = levels 3..1, keepBest, {NaN, ConstraintRatio, Evaluation(ratio_fine)} */
void dvo_amd_default_validator_stages(const dvo_amd_config *frontend_cfg, double min_constraint_ratio, double ratio_coarse,
                                      double ratio_fine, dvo_amd_validator_stage stages[2]);
/* the initial proposal list of validateKeyframeConstraintsParallel (keyframe_graph.cpp:577-585): for every candidate one
 * proposal with identity and one with the relative pose current.pose^-1 * reference.pose.  proposals: 2 * n_candidates */
int dvo_amd_proposals_for_candidates(const dvo_amd_keyframe *keyframes, int keyframe, int n_candidates, const int *candidates,
                                     dvo_amd_constraint_proposal *proposals);
/* validate(): proposals[0..n_proposals) in, survivors compacted to the front in the reference's order, *n_out of them.
 * The context's tracker configuration is restored before returning.  max_in_flight as in dvo_amd_match_many.  A stage of many
 * alignments is dealt over a few worker contexts of the library's own (same device, created on first use, own host threads for
 * the duration of the call: keyframe_graph.cpp:576-593 deals the proposals over TBB workers the same way). */
int dvo_amd_validate_proposals(dvo_amd_context *ctx, int n_keyframes, const dvo_amd_keyframe *keyframes, int n_stages,
                               const dvo_amd_validator_stage *stages, int n_proposals,
                               dvo_amd_constraint_proposal *proposals, int *n_out, int max_in_flight);

/*
 * Loop-closure candidates: what feeds dvo_amd_proposals_for_candidates.  dvo_amd_find_constraint_candidates is
 * dvo_slam::NearestNeighborConstraintSearch::findPossibleConstraints (keyframe_constraint_search.cpp:41-72: a radius search on
 * the keyframes' translations, called for a new keyframe at keyframe_graph.cpp:456 and for every keyframe at :233) and, with
 * min_overlap > 0, THIS LIBRARY'S EXTENSION of it: the radius candidates are pruned by how much of one keyframe the other
 * actually sees, counted on the device by dvo_amd_covisibility before any alignment runs.  (A keyframe half a metre away that
 * looks the other way is a radius candidate; the validator spends four level-3 alignments on it before its voters reject it.)
 *
 * dvo_amd_covisibility: the seven counts of n_pairs ordered keyframe pairs (a, b) in one call.  The rule, operation by
 * operation; the library is built without contraction, so every product and sum rounds on its own.  `level` is clamped to the
 * coarsest level both pyramids of the pair have; where the two levels differ in size, the rays are a's own and the projection
 * uses b's width, height and intrinsics.  For the ordered pair (a, b):
 *  1. transform: the host forms T = pose_b^-1 * pose_a in double, the inverse taken as that of a rigid transform (R^T, -R^T t)
 *     as dvo_amd_map_render does (only finiteness is checked): Ri = Rb^T, ti[r] = -((Rb[0][r]*tb0 + Rb[1][r]*tb1) + Rb[2][r]*tb2);
 *     T[r][c] = (Ri[r][0]*Ra[0][c] + Ri[r][1]*Ra[1][c]) + Ri[r][2]*Ra[2][c] and
 *     T[r][3] = ((Ri[r][0]*ta0 + Ri[r][1]*ta1) + Ri[r][2]*ta2) + ti[r]: products summed in index order; rows 0..2 are cast to
 *     float;
 *  2. point: for every pixel (u, v) of a with a finite depth z the camera point is (tx[u]*z, ty[v]*z, z) with the level's rays
 *     tx[u] = (u - ox) / fx, ty[v] = (v - oy) / fy, moved into b's frame by q = ((T0*x + T1*y) + T2*z) + T3 per row in fp32 (the
 *     arithmetic of the point cloud above); the pixel counts as `valid`;
 *  3. near plane: if !(qz >= near_z) the pixel counts as `behind` (NaN included);
 *  4. projection: pu = floorf(((qx*fx) / qz + ox) + 0.5f), pv = floorf(((qy*fy) / qz + oy) + 0.5f) with b's fx, fy, ox, oy, the
 *     division correctly rounded; if !(pu >= 0 && pu <= (float)(w-1) && pv >= 0 && pv <= (float)(h-1)) the pixel counts as
 *     `outside`: the test is made in float before any conversion to int, so NaN and 1e30 are outside, never an overflow;
 *  5. depth lookup: Zb = depth_b[pv, pu]; if it is NaN the pixel counts as `no_depth`;
 *  6. tolerance: s = qz - 0.4f, tol = depth_sigmas * (0.0012f + 0.0019f * (s*s)): the reference's own depth noise model and
 *     factor of its occlusion test (dense_tracking_impl.cpp:122-128,275; default depth_sigmas 20);
 *  7. classification: d = Zb - qz; d < -tol counts as `occluded` (b sees a nearer surface), d > tol as `seen_through` (b sees
 *     past the point), anything else as `consistent`.
 * By construction valid = behind + outside + no_depth + consistent + occluded + seen_through.  The overlap of (a, b) is
 * (double)consistent / (double)valid, and 0 when valid == 0.  Pair (a, a) and repeated pairs are legal.  All counts are
 * integers: the result does not depend on the launch geometry, on the order of the pairs or on what else is in the call.
 * One launch, one copy back and one synchronisation per call whatever n_pairs is; buffers are the context's, grown to the
 * largest call and kept.
 *
 * Errors of dvo_amd_covisibility.  DVO_AMD_ERR_INVALID_ARGUMENT (reason in dvo_amd_last_error()), before a device is looked
 * for: a NULL array with n_pairs > 0, an index outside [0, n_keyframes), a keyframe of a pair without an image or with a
 * non-finite pose entry, level < 0, depth_sigmas non-finite or negative, near_z non-finite or <= 0.  Then DVO_AMD_ERR_NO_DEVICE
 * without a GPU, DVO_AMD_ERR_INVALID_ARGUMENT for a NULL context, DVO_AMD_ERR_DEVICE_MISMATCH for a pyramid of another device,
 * DVO_AMD_ERR_INVALID_ARGUMENT while pairs are queued on the context.  n_pairs == 0 is DVO_AMD_OK.
 *
 * dvo_amd_find_constraint_candidates.  Radius stage (host code): translations are cast to float (pcl::PointXYZ stores them so),
 * d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, and keyframe k is a candidate iff d2 <= max_distance * max_distance (fp32).  The query
 * keyframe itself is included, as in the reference (the odometry voter rejects it later).  Candidates come out in ascending
 * keyframe index.  The reference delegates the boundary and the order to FLANN (pcl::KdTreeFLANN::radiusSearch), whose source
 * is not in its tree: `<=` and ascending index are this library's rule.
 * Overlap stage, when min_overlap > 0 (opt is then required, and every keyframe within the radius needs an image): one
 * dvo_amd_covisibility call over both directions of every radius candidate; a candidate c is kept iff
 * max(overlap(q -> c), overlap(c -> q)) >= min_overlap -- the maximum, so that a close-up of part of a wider view still counts --
 * and overlap[] (may be NULL) receives that maximum for every kept candidate.  When min_overlap <= 0 the entry is exactly the
 * reference's search: no device is needed and none is looked for, ctx may be NULL, and overlap[] is filled with NaN.
 * DVO_AMD_ERR_INVALID_ARGUMENT for: NULL keyframes or n_out, n_keyframes < 1, `keyframe` out of range, capacity < 0 or a NULL
 * candidate array with capacity > 0, max_distance non-finite or negative, a NaN min_overlap, a non-finite pose entry of any
 * keyframe; with min_overlap > 0 the errors of dvo_amd_covisibility as well.  If capacity is too small: DVO_AMD_ERR_CAPACITY
 * with *n_out set to the size needed (candidates untouched).
 */
typedef struct {
  unsigned valid;        /* pixels of a with finite depth at the level */
  unsigned behind;       /* ... whose point has !(qz >= near_z) in b */
  unsigned outside;      /* ... that project outside b's image */
  unsigned no_depth;     /* ... that land on a NaN depth of b */
  unsigned consistent;   /* |Zb - qz| <= tol */
  unsigned occluded;     /* Zb - qz < -tol : b sees a nearer surface */
  unsigned seen_through; /* Zb - qz >  tol : b sees past the point */
  unsigned reserved;
} dvo_amd_covisibility_counts;

typedef struct {
  int level;           /* default 3 */
  float near_z;        /* default 0.1 */
  float depth_sigmas;  /* default 20 */
} dvo_amd_covisibility_options;

void dvo_amd_default_covisibility_options(dvo_amd_covisibility_options *opt);

int dvo_amd_covisibility(dvo_amd_context *ctx, int n_keyframes, const dvo_amd_keyframe *keyframes,
                         const dvo_amd_covisibility_options *opt, int n_pairs, const int *pair_a, const int *pair_b,
                         dvo_amd_covisibility_counts *out);

int dvo_amd_find_constraint_candidates(dvo_amd_context *ctx, int n_keyframes, const dvo_amd_keyframe *keyframes, int keyframe,
                                       float max_distance, double min_overlap, const dvo_amd_covisibility_options *opt,
                                       int *candidates, double *overlap, int capacity, int *n_out);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Place index: loop-closure candidates by appearance, on the device.
 *
 * dvo_amd_find_constraint_candidates trusts the estimated poses in both of its stages.  After a long loop the true revisit lies
 * outside max_distance and is never proposed; when tracking is lost there is no pose to search around.  A dvo_amd_place_index
 * answers "which keyframes look like this one / like this frame" without any pose: it keeps one int8 descriptor per keyframe on the
 * device and returns, per query, the k keys of highest cosine.  Its output is a candidate list like the radius search's: it feeds
 * dvo_amd_proposals_for_candidates and the validator unchanged.  (The reference has no counterpart: keyframe_constraint_search.cpp is
 * all it has.)  The entries take no context: like the mask operations and the depth fusion they run on the device's internal
 * stream, use no tracker slot and may be called while pairs are queued.  Pyramids are only read.  Calls on one index are serialised
 * by the index; different indices are independent.
 *
 * The descriptor of a pyramid is its intensity plane I at level `level` (width w, height h), high-passed and quantised.  Per
 * pixel p = (u, v), in fp32, operation by operation (the library is built without contraction; the division is correctly rounded):
 *  1. s = the sum of I over the 3x3 neighbourhood of p clipped to the plane, rows ascending, columns ascending within a row, added
 *     one after the other starting from 0.0f; c = the number of pixels summed (4, 6 or 9) as a float;
 *  2. m = s / c; d = (I[p] - m) * gain;
 *  3. q[p] = 0 if d is not finite, otherwise (int8) min(127, max(-127, rintf(d))), ties to even.  -128 never occurs.
 * A descriptor is the w * h values in row-major order, zero-padded to dim = 64 * ceil(w * h / 64) bytes; its norm is nn = sum q * q,
 * an int32 (dim <= DVO_AMD_PLACE_MAX_DIM, so the sum cannot overflow: a larger level is refused).  Removing the local mean makes the
 * descriptor invariant to a brightness offset, the cosine below makes the score invariant to a gain.
 *
 * The index is a growable row-major N x dim int8 matrix on the device with nn and r per row.  r = 1.0 / sqrt((double)nn), formed in
 * double ON THE HOST when the row is added (correctly rounded square root and quotient), and 0 when nn == 0.  Ids are the rows'
 * positions: consecutive from 0 in insertion order.  The first add fixes (w, h).  The capacity starts at
 * DVO_AMD_PLACE_INITIAL_CAPACITY rows and doubles: growth allocates anew and copies on the device.
 *
 * dvo_amd_place_index_add describes all n pyramids in ONE kernel launch and synchronises once; *first_id (may be NULL) receives
 * the id of pyramids[0].  dvo_amd_place_index_info: any of the four outputs may be NULL; width, height and dim are 0 before the
 * first add.  dvo_amd_place_index_download: rows [first, first + n) as n * dim bytes and n norms (either may be NULL).
 * dvo_amd_place_scores: dots[i * n + j] = sum_k q_{query_ids[i]}[k] * q_{first + j}[k], an exact int32, computed on the int8 matrix
 * instruction.
 * dvo_amd_place_query: key j is eligible for query i iff |j - query_ids[i]| > exclude_recent (so never the query's own row) and
 * score >= min_score, where score = ((double)dot * r_query) * r_j: two double products, each rounded on its own.  The result of a
 * query is the k eligible keys of highest score, ties going to the lower id, ordered by descending score, then ascending id:
 * candidates[i * k + t] and scores[i * k + t] for t < counts[i], -1 and NaN behind.  dvo_amd_place_query_frames does the same for
 * pyramids that are not in the index: their descriptors are built into scratch with the index's options, their norms come back to
 * the host for r_query (one more synchronisation), and no key is excluded, a frame having no id.  Against an empty index every
 * count is 0.  The dots of a query call live in device scratch; above DVO_AMD_PLACE_DOTS_CAP_MB they are processed in panels of query
 * rows.  Every value is an integer or a double formed from integers in a fixed order: no result depends on the launch geometry, on
 * the panels or on what else is in the call.
 *
 * Errors, before any device work.  DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error() that starts with the entry's
 * name: a NULL pointer (inside the arrays too; an array only where its count is positive); a negative count; an id or a range
 * outside the index; level outside 0 .. DVO_AMD_MAX_LEVELS - 1; gain not finite or <= 0; k outside 1 .. DVO_AMD_PLACE_MAX_K; a NaN
 * min_score; a negative exclude_recent; a pyramid with fewer than level + 1 levels; a pyramid whose level has another size than the
 * index's (in the first add: than the call's first pyramid's); w * h > DVO_AMD_PLACE_MAX_DIM.  Then DVO_AMD_ERR_DEVICE_MISMATCH for
 * a pyramid of another device than the index's, then DVO_AMD_ERR_NO_DEVICE.  n == 0 / n_queries == 0 is DVO_AMD_OK and does nothing.
 * dvo_amd_place_index_create needs a device: DVO_AMD_ERR_NO_DEVICE without one, then DVO_AMD_ERR_INVALID_ARGUMENT for a device that
 * does not exist; *out is NULL on every failure.
 *
 * Not covered: rows are never removed or re-ordered; one image size per index; no viewpoint invariance beyond what a coarse level
 * gives; no depth in the descriptor.  The entry only proposes: the validator still decides.
 */
#define DVO_AMD_PLACE_MAX_K 64
#define DVO_AMD_PLACE_MAX_DIM 65536
#define DVO_AMD_PLACE_INITIAL_CAPACITY 64
#define DVO_AMD_PLACE_DOTS_CAP_MB 256
typedef struct dvo_amd_place_index dvo_amd_place_index;
typedef struct dvo_amd_place_options {
  int level;   /* default 3 */
  float gain;  /* default 1; finite, > 0 */
} dvo_amd_place_options;
typedef struct dvo_amd_place_query_options {
  int k;               /* 1 .. DVO_AMD_PLACE_MAX_K; default 5 */
  double min_score;    /* default 0; NaN refused */
  int exclude_recent;  /* default 0; >= 0 */
} dvo_amd_place_query_options;
/* level 3, gain 1 / k 5, min_score 0, exclude_recent 0; a NULL opt is a no-op */
void dvo_amd_default_place_options(dvo_amd_place_options *opt);
void dvo_amd_default_place_query_options(dvo_amd_place_query_options *opt);
int dvo_amd_place_index_create(int device, const dvo_amd_place_options *opt, dvo_amd_place_index **out);
void dvo_amd_place_index_destroy(dvo_amd_place_index *index);
int dvo_amd_place_index_add(dvo_amd_place_index *index, int n, const dvo_amd_pyramid *const *pyramids, int *first_id);
int dvo_amd_place_index_info(const dvo_amd_place_index *index, int *size, int *width, int *height, int *dim);
int dvo_amd_place_index_download(const dvo_amd_place_index *index, int first, int n, signed char *descriptors /* n * dim, or NULL */,
                                 int *norms /* n, or NULL */);
int dvo_amd_place_scores(const dvo_amd_place_index *index, int n_queries, const int *query_ids, int first, int n,
                         int *dots /* n_queries * n */);
int dvo_amd_place_query(const dvo_amd_place_index *index, int n_queries, const int *query_ids,
                        const dvo_amd_place_query_options *opt, int *candidates /* n_queries * k */, double *scores /* n_queries * k */,
                        int *counts /* n_queries */);
int dvo_amd_place_query_frames(const dvo_amd_place_index *index, int n_queries, const dvo_amd_pyramid *const *frames,
                               const dvo_amd_place_query_options *opt, int *candidates, double *scores, int *counts);

/*
 * Dual-match front-end step: the two alignments LocalTracker::update runs per frame with
 * tbb::parallel_invoke (local_tracker.cpp:170-186) -- keyframe -> frame starting from last_keyframe_pose^-1 and
 * last frame -> frame starting from identity -- as ONE two-pair batch sharing the frame's pyramid, plus the quantities the
 * accept callbacks of KeyframeTracker test on the two results (keyframe_tracker.cpp:105-190).
 */
typedef struct {
  int odometry_is_nan, keyframe_is_nan;   /* force a new keyframe (local_tracker.cpp:191) */
  double odometry_translation_norm;       /* onAcceptCriterionEstimateDivergence: rejects > 0.1 */
  double keyframe_translation_norm;       /* ... and > 1.5 MaxTranslationalDistance; onAcceptCriterionDistance */
  double keyframe_constraint_ratio;       /* onAcceptCriterionConstraintRatio: Levels.back().Iterations.back().ValidConstraints / ValidPixels */
  double odometry_neg_loglik;             /* onAcceptCriterionTrackingResultEvaluation: -LogLikelihood (value() of the evaluation) */
  double keyframe_neg_loglik;
  double odometry_condition_number;       /* onAcceptCriterionConditionNumber: |lambda_max / lambda_min| of Information */
  double keyframe_condition_number;
} dvo_amd_frame_criteria;
/* last_keyframe_pose: column-major 4x4 (LocalTrackerImpl::last_keyframe_pose_), NULL = identity.  r_keyframe / r_odometry
 * follow dvo_amd_match's conventions; criteria may be NULL. */
int dvo_amd_track_frame(dvo_amd_context *ctx, dvo_amd_pyramid *keyframe, dvo_amd_pyramid *last_frame, dvo_amd_pyramid *frame,
                        const double *last_keyframe_pose, dvo_amd_result *r_keyframe, dvo_amd_result *r_odometry,
                        dvo_amd_frame_criteria *criteria);

/*
 * TUM RGB-D benchmark on-disk formats, host code only.
 * The reference reads frames with cv::imread (benchmark_slam.cpp:50-51): the colour image as 3-channel 8-bit BGR
 * (flag 1), the depth image unchanged (flag -1, 16-bit gray in TUM sequences).  OpenCV is not available here, so a PNG
 * decoder (zlib inflate + the five PNG filters; 8/16-bit gray, gray+alpha, RGB, RGBA, and 1/2/4/8-bit palette or gray;
 * non-interlaced only) stands in for those two calls.  16-bit colour samples keep their high byte, alpha is dropped,
 * gray is replicated to B=G=R: what imread(.., 1) returns.
 */
int dvo_amd_png_info(const char *path, int *width, int *height, int *channels, int *bit_depth);
int dvo_amd_png_read_bgr8(const char *path, unsigned char *dst, int width, int height);      /* width*height*3 bytes */
int dvo_amd_png_read_gray16(const char *path, unsigned short *dst, int width, int height);   /* gray PNGs only; 8-bit values are widened */
/* One line of the estimated trajectory exactly as benchmark_slam.cpp:490-504 / map_serializer.cpp:61-66 print it:
 * "<sec>.<nsec, 9 digits> tx ty tz qx qy qz qw \n" with the default ostream formatting of doubles (%g, 6 significant
 * digits), the stamp split like ros::Time::fromSec, the quaternion as Eigen::Quaterniond(rotation) builds it.
 * T: column-major 4x4.  Returns the number of characters written (excluding the terminator), or -1 if capacity is too small. */
int dvo_amd_format_trajectory_line(double timestamp, const double *T, char *buf, int capacity);

/*
 * The keyframe map's point cloud (AsyncPointCloudBuilder::BuildJob::build, async_point_cloud_builder.cpp:61-110, over
 * RgbdCamera::buildPointCloud, rgbd_image.cpp:245-262; PointCloudAggregator::build, point_cloud_aggregator.cpp:74-109).
 *
 * Point record: 16 bytes, rgb packed 0x00RRGGBB the way PCL packs PointXYZRGB.
 *
 * Organized cloud of one image (dvo_amd_point_cloud): w*h points of the requested level in scan order, NaN points included
 * (the reference pushes them).  Camera point (tx[u]*z, ty[v]*z, z) in fp32, z the level's depth plane (NaN where invalid),
 * tx[u] = (u - ox) / fx and ty[v] = (v - oy) / fy the level's rays.  World point: T = (float)pose element by element, then
 * x' = ((T00*x + T01*y) + T02*z) + T03 and the same order for y' and z', every product and sum rounded on its own (no
 * contraction).  The reference computes the transform with Eigen's 4x4 product, whose summation order is Eigen's and is not
 * pinned here (like Q7 / Q8): the two agree to fp32 rounding, not bit for bit.  Colour: from the caller's 8-bit BGR image of
 * the level (w*h*3, stride in bytes) when one is given; otherwise grey from the intensity plane, r = g = b = the value clamped
 * to [0, 255] and truncated, NaN -> 0 (the reference's implicit float -> uint8 conversion is undefined out of range).
 *
 * Voxel aggregate (dvo_amd_map_cloud over level 0 of every image, dvo_amd_voxel_downsample over given points):
 *  - non-finite points are dropped;
 *  - voxel index i = (int)floorf(x * inv) with inv = 1.0f / leaf_size in fp32, the same for j and k (pcl::VoxelGrid's rule);
 *    a point with an index outside [-2^20, 2^20) is dropped and counted in out_of_range;
 *  - one point per occupied voxel, in ascending order of the 63-bit key ((i+2^20)<<42) | ((j+2^20)<<21) | (k+2^20);
 *  - centroid in fixed point: every coordinate becomes q = llrint((double)x * 2^24), summed in int64 per voxel; the output is
 *    (float)((double)sum / ((double)count * 2^24)).  The sums are exact while the |q| of a voxel add up to less than 2^63
 *    (2^31 points within 256 m of the origin); beyond that they wrap modulo 2^64 -- still the same bits in every run;
 *  - colour: every channel is (sum + count/2) / count in integers.
 * Integer sums make the result independent of the order the points arrive in: bit-identical from run to run, for any keyframe
 * order and any launch geometry (as for match(), tests/test_determinism.py).
 * Departure from the reference: PCL's ApproximateVoxelGrid (setDownsampleAllData(true), leaf 1 cm) keeps a 512-entry hash and
 * flushes a voxel whenever another voxel lands on its slot, so it may emit one voxel several times and its output depends on
 * the point order -- a sequential artefact.  This follows pcl::VoxelGrid's one point per voxel instead.
 * leaf_size must be finite and in (0, 65536] m (DVO_AMD_ERR_INVALID_ARGUMENT otherwise: a larger leaf would let llrint leave
 * the int64 range); at most 2^31 points per call (DVO_AMD_ERR_INVALID_ARGUMENT beyond).  When `capacity` is smaller than the number of voxels the call returns
 * DVO_AMD_ERR_CAPACITY with stats->voxels set to the size needed (out untouched).  stats may be NULL.
 * Like every compute entry: DVO_AMD_ERR_NO_DEVICE without a GPU, DVO_AMD_ERR_DEVICE_MISMATCH for a pyramid of another device,
 * DVO_AMD_ERR_INVALID_ARGUMENT while pairs are queued on the context (dvo_amd_match_submit).  Buffers are the context's, grown to
 * the largest call and kept: nothing is allocated per call once warm.
 */
typedef struct {
  float x, y, z;
  unsigned int rgb;
} dvo_amd_point;

typedef struct {
  long long points_in;     /* points handed to the call (NaN ones included) */
  long long finite;        /* ... of them with three finite coordinates */
  long long out_of_range;  /* finite points dropped for a voxel index outside [-2^20, 2^20) */
  long long voxels;        /* occupied voxels: points written, or the capacity needed */
} dvo_amd_cloud_stats;

/* pose: column-major 4x4, NULL = identity; bgr: NULL = grey from the intensity plane; out: w*h points of the level */
int dvo_amd_point_cloud(dvo_amd_context *ctx, dvo_amd_pyramid *image, int level, const double *pose,
                        const unsigned char *bgr, int bgr_stride_bytes, dvo_amd_point *out);
/* the organized clouds of level 0 of n images at their poses (n x 16 doubles, column-major each), aggregated in one call.
 * bgrs: NULL or n entries, each NULL (grey) or the image's level-0 BGR (w*h*3, bgr_strides[k] bytes per row; bgr_strides NULL:
 * tight rows) */
int dvo_amd_map_cloud(dvo_amd_context *ctx, int n, dvo_amd_pyramid *const *images, const double *poses,
                      const unsigned char *const *bgrs, const int *bgr_strides, float leaf_size, dvo_amd_point *out,
                      long long capacity, dvo_amd_cloud_stats *stats);
int dvo_amd_voxel_downsample(dvo_amd_context *ctx, long long n, const dvo_amd_point *in, float leaf_size,
                             dvo_amd_point *out, long long capacity, dvo_amd_cloud_stats *stats);

/*
 * The keyframe map kept on the device: keyframes are inserted, moved and removed one event at a time, and the voxel aggregate
 * is updated by the difference instead of being rebuilt.  A voxel is a set of integer sums (above) and the world point of a
 * pixel at a pose is a pinned sequence of fp32 operations, so a keyframe's contribution at its old pose is recomputed and
 * subtracted exactly.
 *
 * The contract: after any sequence of successful calls, dvo_amd_map_extract(map, NULL, ...) returns exactly what
 * dvo_amd_map_cloud returns for the keyframes now in the map -- their current poses and BGR images, the map's leaf_size: the
 * same voxels in the same ascending key order with the same coordinate and colour bits -- and dvo_amd_map_stats returns that
 * call's points_in, finite, out_of_range and voxels.  The history does not show in the result: not the order of the
 * operations, not how they were batched, not the launch geometry.  Every rule of the voxel aggregate carries over unchanged:
 * the index rule and the 2^20 range with its out_of_range count, NaN points dropped, sums wrapping modulo 2^64 (for which
 * subtraction is still exact), the leaf bounds.  At most 2^31 points per update.
 *
 * Box extraction: with a box {xmin,ymin,zmin,xmax,ymax,zmax} a voxel is returned when its output centroid c satisfies
 * min <= c < max on all three axes, compared in fp32; the voxels keep their order: the result is the full extract filtered, bit
 * for bit.  A box with a NaN or with min >= max on any axis: DVO_AMD_ERR_INVALID_ARGUMENT.
 *
 * Ownership: insert retains the pyramid (dvo_amd_pyramid_retain) and copies the BGR image to the device, packed to w*3 bytes
 * per row; the map holds both until remove or destroy.  The caller may release its handle and free its image as soon as
 * insert returns.
 *
 * Errors: a failed call leaves the map exactly as it was.  DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error()
 * for: insert of an id already present; an unknown id in set_poses or remove; the same id twice in one call; a non-finite pose
 * entry.  set_poses with a pose whose 16 doubles round to the same floats as the stored one does nothing for that keyframe.
 * extract with too small a capacity returns DVO_AMD_ERR_CAPACITY with *n_out set to the size needed (out untouched).  Like
 * every compute entry: DVO_AMD_ERR_NO_DEVICE without a GPU, DVO_AMD_ERR_DEVICE_MISMATCH for a pyramid of another device,
 * DVO_AMD_ERR_INVALID_ARGUMENT while pairs are queued on the context.
 *
 * The map is bound to its context: it shares the context's stream and buffers and is no more thread-safe than the context.
 * The context must outlive its maps; destroying a context with live maps is the caller's error (destroy the maps first).
 */
typedef struct dvo_amd_map dvo_amd_map;
int dvo_amd_map_create(dvo_amd_context *ctx, float leaf_size, dvo_amd_map **out);
void dvo_amd_map_destroy(dvo_amd_map *map);
/* level 0 of the pyramid; pose: column-major 4x4, NULL = identity; bgr: NULL = grey, else w*h*3 with bgr_stride_bytes per row
 * (0: tight rows) */
int dvo_amd_map_insert(dvo_amd_map *map, int id, dvo_amd_pyramid *image, const double *pose, const unsigned char *bgr,
                       int bgr_stride_bytes);
/* poses: n x 16 doubles, column-major each */
int dvo_amd_map_set_poses(dvo_amd_map *map, int n, const int *ids, const double *poses);
int dvo_amd_map_remove(dvo_amd_map *map, int n, const int *ids);
/* stats and n_keyframes may be NULL */
int dvo_amd_map_stats(const dvo_amd_map *map, dvo_amd_cloud_stats *stats, int *n_keyframes);
/* box: NULL, or {xmin,ymin,zmin,xmax,ymax,zmax} */
int dvo_amd_map_extract(dvo_amd_map *map, const float *box, dvo_amd_point *out, long long capacity, long long *n_out);

/*
 * The keyframe map rendered into a camera view on the device: every voxel is forward-projected into the image with a
 * nearest-depth test, the way RgbdImage::warpDepthForward / warpIntensityForward / warpDepthForwardAdvanced
 * (rgbd_image.cpp:604-781) splat points.  The view's depth and intensity planes are an RgbdImagePyramid's level 0
 * (dvo_amd_map_render_pyramid), so every tracker entry can align a live frame to the fused model.
 *
 * The rule, operation by operation; the result is a function of the map and the view alone -- not of the launch geometry, not
 * of the order the atomics land in.  pose: camera -> world, column-major 4x4 doubles, NULL = identity (as dvo_amd_map_insert).
 * Pixel centres sit at integer coordinates: the ray of column u is (u - ox) / fx.  For the voxel of rank r (its position in the
 * store's ascending key order = its index in dvo_amd_map_extract(map, NULL, ...)):
 *  1. centroid (x, y, z) and packed colour: the bits dvo_amd_map_extract returns;
 *  2. world -> camera: the host forms the inverse of the pose in double, taking it as rigid (only finiteness is checked):
 *     Ri = R^T, ti[r] = -((R[0][r]*t0 + R[1][r]*t1) + R[2][r]*t2), every product and sum rounded on its own; each entry is cast to
 *     float; the device computes c = ((T0*x + T1*y) + T2*z) + T3 per row in fp32, uncontracted (the order of the point cloud);
 *  3. cull: the voxel is dropped unless cz >= near_z (false for NaN) and counted in behind_near;
 *  4. project, in fp32, every operation rounded: u = (cx*fx)/cz + ox, v = (cy*fy)/cz + oy, the division correctly rounded;
 *  5. footprint: the voxel covers a square of its own size: hx = 0.5f*((leaf*fx)/cz); columns u0 = ceilf(u - hx) to
 *     u1 = floorf(u + hx); if u1 < u0 the footprint holds no pixel centre and u0 = u1 = floorf(u + 0.5f); rows the same way with
 *     fy.  The voxel is drawn only if u1 >= 0 && u0 <= (float)(width-1) && v1 >= 0 && v0 <= (float)(height-1), compared in float
 *     before any conversion to int (false for NaN); otherwise it is counted in outside.  The footprint is then clamped to the
 *     image: columns from (u0 > 0 ? (int)u0 : 0) to (u1 < (float)(width-1) ? (int)u1 : width-1), rows alike ((float)(width-1)
 *     is exact up to 2^24; beyond, a range left empty by its rounding draws no pixel);
 *  6. depth test: every covered pixel keeps the minimum of the 64-bit word (bits(cz) << 32) | r.  cz > 0, so its bit pattern
 *     orders like its value; ties in depth go to the lower rank;
 *  7. resolve, per pixel: covered: depth = cz, rgb = the voxel's packed colour, intensity = (float)((1868 B + 9617 G + 4899 R
 *     + 8192) >> 14) (the ingest's grey rule: a grey keyframe's value comes back unchanged), index = r; empty: depth = NaN
 *     (0x7FC00000), rgb = 0, intensity = 0, index = -1.
 * There is no hole filling and no smoothing: a pixel no footprint covers stays empty (dvo_amd_pyramid_filter_depth on the rendered
 * pyramid does both).
 *
 * A footprint side is bounded by the view, not by clipping: near_z < (leaf * max(fx, fy)) / 32 (in fp32) is rejected, so no
 * voxel spans more than 32 pixels (33 pixel centres).  DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error() for
 * that and for: width or height < 1 or width*height > 2^26; fx or fy not finite and positive; ox, oy or near_z not finite;
 * near_z <= 0; a non-finite pose entry; pairs queued on the context.  DVO_AMD_ERR_NO_DEVICE as for every compute entry.  An
 * empty map renders an all-empty view and returns DVO_AMD_OK.  A render never changes the map.  stats (may be NULL):
 * voxels = behind_near + outside + drawn; covered_pixels = the pixels that are not empty.
 */
typedef struct {
  int width, height;
  float fx, fy, ox, oy;
  float near_z;
} dvo_amd_view;

typedef struct {
  long long voxels, behind_near, outside, drawn, covered_pixels;
} dvo_amd_render_stats;

/* any of depth / rgb / intensity / index may be NULL; each is width*height, row-major, host memory */
int dvo_amd_map_render(dvo_amd_map *map, const double *pose, const dvo_amd_view *view, float *depth, unsigned int *rgb,
                       float *intensity, int *index, dvo_amd_render_stats *stats);
/* the same view as a pyramid (dvo_amd_pyramid_create_from_device's rules for width, height and levels), built from the device
 * planes without a host round trip: level 0's intensity and depth planes are exactly dvo_amd_map_render's */
int dvo_amd_map_render_pyramid(dvo_amd_map *map, const double *pose, const dvo_amd_view *view, int levels, double timestamp,
                               dvo_amd_pyramid **out, dvo_amd_render_stats *stats);

/*
 * Frame warps: a frame's grey values and depth resampled into another camera's pixels, on the device.
 *
 * RgbdImage::warpIntensity / warpIntensitySse (the inverse warp: a gather over the target's pixels) and warpIntensityForward /
 * warpDepthForward / warpDepthForwardAdvanced (the forward warp: a scatter of the source's pixels), rgbd_image.cpp:545-781.  The
 * operation underneath dvo_amd_mask_warp (masks), dvo_amd_pyramid_fuse_depth (depth) and dvo_amd_map_render (the map): to look at
 * an alignment, to difference two frames in one pixel grid, to feed a view-normalised frame to the place index or to
 * dvo_amd_estimate_exposure, to predict the next frame from the last one -- without downloading planes and uploading a result.
 *
 * Both directions.  T: 16 doubles, column-major, maps points of the MOVING frame's camera into the FIXED camera: for
 * dvo_amd_match(reference = fixed, current = moving) the result's transformation as returned (the convention of
 * dvo_amd_mask_warp and dvo_amd_pyramid_fuse_depth).  The moving frame is the one whose grey values travel; the result lies on
 * the fixed camera's pixels.  All fp32 arithmetic is uncontracted, every operation rounded on its own, divisions correctly
 * rounded.  Every count is an integer sum and every collision a 64-bit minimum: no value depends on the launch geometry, on the
 * order atomics land in or on what else is in the call, and two runs are bit-identical.  The entries take no context, use no
 * tracker slot and run on the device's internal stream.
 *
 * 1. The inverse warp (dvo_amd_warp_inverse / _many): for every pixel of level `level` of fixed[k], the grey value of level
 *    `level` of moving[k] where that pixel's point lands -- moving.warpIntensity(T^-1, fixed.pointcloud, ...).  The two frames
 *    may differ in size and intrinsics.  The host forms rows 0..2 of the rigid inverse M of T as depth fusion does: Ri = R^T,
 *    ti[r] = -((R[0][r]*t0 + R[1][r]*t1) + R[2][r]*t2) in double, each entry cast to float.  Per fixed pixel (u, v), depth z:
 *     a. z not finite: `no_depth`; both outputs empty;
 *     b. (x, y, z) = (tx[u]*z, ty[v]*z, z) with the fixed level's rays; q = ((M0*x + M1*y) + M2*z) + M3 per row;
 *     c. !(qz >= near_z): `behind`; both outputs empty;
 *     d. px = (qx*fx)/qz + ox, py = (qy*fy)/qz + oy with the moving level's intrinsics;
 *     e. !(px >= 0 && px < wm && py >= 0 && py < hm), compared in float before any conversion: `outside` (the reference's
 *        inImage); both outputs empty;
 *     f. x0 = floorf(px), y0 = floorf(py); x0 + 1 >= wm || y0 + 1 >= hm: `border` (bilinearWithDepthBuffer's first return);
 *     g. a = px - x0, b = py - y0, wa = 1 - a, wb = 1 - b; the taps (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) in this order
 *        with the weights wa*wb, a*wb, wa*b, a*b.  A tap takes part iff its moving depth is finite and > qz - occlusion_margin;
 *        then val = val + w*I and sum = sum + w (each product and sum rounded, from val = sum = 0).  sum > 0: `warped`, the
 *        intensity is val / sum; otherwise `hidden`.  `partial` counts the warped pixels of which fewer than four taps took part;
 *     h. the depth plane holds, for every pixel that passed e (border, hidden and warped pixels alike, as in the reference), qz
 *        (depth == DVO_AMD_WARP_DEPTH_TRANSFORMED, the reference's rule) or z (DVO_AMD_WARP_DEPTH_FIXED: the geometry of the
 *        camera the image is now in); the intensity of a border or hidden pixel is empty.
 *    An empty intensity or depth is NaN (0x7FC00000).  intensity_out / depth_out: host planes of the fixed level's size, either
 *    may be NULL (in the many form: arrays of n pointers, the array or any entry may be NULL).  counts (may be NULL): per pair
 *    DVO_AMD_WARP_INVERSE_COUNTS values valid, behind, outside, border, hidden, warped, partial, no_depth; valid = behind + outside
 *    + border + hidden + warped.
 *    dvo_amd_pyramid_warp_inverse / _many do the same at level 0 and return an ordinary pyramid with the fixed pyramid's size,
 *    intrinsics, level count and timestamp.  There every pixel that is not warped is empty in BOTH planes -- intensity
 *    fill_intensity, depth NaN, dvo_amd_map_render_pyramid's empty pixel -- so that no pixel with a depth but no grey value is
 *    ever tracked.
 *    A call is ONE kernel launch for all its pairs and synchronises once; a pyramid form then builds each pyramid as every
 *    builder does.
 *
 * 2. The forward warp (dvo_amd_warp_forward / _many): every pixel of level `level` of moving[k] with a finite depth is
 *    projected into a view and drawn with a nearest-depth test.  views: n views, or NULL: the fixed camera is the moving
 *    level's own (its size and intrinsics, near_z = opt->near_z); with a view, the view's near_z applies.  The rule is
 *    dvo_amd_map_render's steps 2 to 7 with "voxel of rank r" read as "moving pixel of index r = v*w + u": rows 0..2 of T cast
 *    to float (no inverse); (x, y, z) = (tx[u]*z, ty[v]*z, z); c = ((T0*x + T1*y) + T2*z) + T3; !(cz >= near_z): `behind`;
 *    pu = (cx*fx)/cz + ox, pv = (cy*fy)/cz + oy with the view's intrinsics.  The pixels covered (opt->splat), columns a0..a1:
 *     DVO_AMD_WARP_SPLAT_NEAREST    a0 = a1 = floorf(pu + 0.5f);
 *     DVO_AMD_WARP_SPLAT_FLOOR      a0 = a1 = floorf(pu), the reference's pixel;
 *     DVO_AMD_WARP_SPLAT_FOOTPRINT  the square the moving pixel spans at its new depth: hx = 0.5f*(((z/fx_m)*fx)/cz) (fx_m: the
 *                                   moving level's), a0 = ceilf(pu - hx), a1 = floorf(pu + hx), and a0 = a1 = floorf(pu + 0.5f)
 *                                   where a1 < a0;
 *    rows b0..b1 the same way with pv, fy and fy_m.  a1 - a0 > 15 || b1 - b0 > 15 (more than DVO_AMD_WARP_MAX_FOOTPRINT columns
 *    or rows before clamping): not drawn, `too_large`.  Otherwise drawn only if a1 >= 0 && a0 <= (float)(width-1) && b1 >= 0 &&
 *    b0 <= (float)(height-1), compared in float before any conversion to int (false for NaN), else `outside`; the footprint is
 *    clamped to the view as in dvo_amd_map_render's step 5.  Every covered pixel keeps the minimum of (bits(cz) << 32) | r: the
 *    nearest depth wins, ties go to the lower index.  Per pixel of the view: depth = cz, intensity = the moving pixel's grey
 *    value bit for bit, index = r; empty: depth NaN, intensity NaN, index -1.
 *    (The reference's 5 cm hysteresis and "the last writer in scan order wins" depend on the order of the scan; the
 *    nearest-depth rule of the map render and of the depth registration replaces them.)
 *    depth_out / intensity_out / index_out: host planes of the view's size, any may be NULL (many form: arrays of n pointers).
 *    counts (may be NULL): per item DVO_AMD_WARP_FORWARD_COUNTS values valid, behind, outside, too_large, drawn, covered_pixels,
 *    no_depth; valid = behind + outside + too_large + drawn; covered_pixels = the pixels of the view that are not empty.
 *    dvo_amd_pyramid_warp_forward / _many work at level 0 and return a pyramid of the view with the moving pyramid's level count
 *    and timestamp (dvo_amd_pyramid_create_from_device's rules for width, height and levels); an empty pixel's intensity is
 *    fill_intensity there.
 *    A call is THREE kernel launches for all its items (clear, splat, resolve) and synchronises once.
 *
 * Errors, in this order: DVO_AMD_ERR_INVALID_ARGUMENT with a reason that starts with the entry's name, before a device is looked
 * for (a NULL pointer, also inside an array; n < 0; a level beyond either pyramid; a non-finite entry of T; near_z not finite and
 * positive; occlusion_margin not >= 0 (+inf switches the depth-buffer test off); an unknown depth or splat; a non-finite
 * fill_intensity; a view dvo_amd_map_render would refuse); DVO_AMD_ERR_DEVICE_MISMATCH; DVO_AMD_ERR_NO_DEVICE.  n == 0 is OK and
 * does nothing.  On failure the outputs are untouched and every out[k] is NULL.
 */
#define DVO_AMD_WARP_DEPTH_TRANSFORMED 0
#define DVO_AMD_WARP_DEPTH_FIXED 1
#define DVO_AMD_WARP_SPLAT_NEAREST 0
#define DVO_AMD_WARP_SPLAT_FLOOR 1
#define DVO_AMD_WARP_SPLAT_FOOTPRINT 2
#define DVO_AMD_WARP_MAX_FOOTPRINT 16
#define DVO_AMD_WARP_INVERSE_COUNTS 8
#define DVO_AMD_WARP_FORWARD_COUNTS 7

typedef struct {
  float near_z;            /* 0.1; > 0 */
  float occlusion_margin;  /* 0.05, the reference's constant; >= 0, +inf: no depth-buffer test (inverse) */
  int depth;               /* DVO_AMD_WARP_DEPTH_TRANSFORMED (inverse) */
  int splat;               /* DVO_AMD_WARP_SPLAT_NEAREST (forward) */
  float fill_intensity;    /* 0: an empty pixel's intensity in the pyramid forms */
} dvo_amd_warp_options;

void dvo_amd_default_warp_options(dvo_amd_warp_options *opt);
int dvo_amd_warp_inverse(const dvo_amd_pyramid *fixed, const dvo_amd_pyramid *moving, const double *T, int level,
                         const dvo_amd_warp_options *opt, float *intensity_out, float *depth_out, long long *counts);
int dvo_amd_warp_inverse_many(int n, const dvo_amd_pyramid *const *fixed, const dvo_amd_pyramid *const *moving, const double *T, int level,
                              const dvo_amd_warp_options *opt, float *const *intensity_out, float *const *depth_out, long long *counts);
int dvo_amd_pyramid_warp_inverse(const dvo_amd_pyramid *fixed, const dvo_amd_pyramid *moving, const double *T,
                                 const dvo_amd_warp_options *opt, dvo_amd_pyramid **out, long long *counts);
int dvo_amd_pyramid_warp_inverse_many(int n, const dvo_amd_pyramid *const *fixed, const dvo_amd_pyramid *const *moving, const double *T,
                                      const dvo_amd_warp_options *opt, dvo_amd_pyramid **out, long long *counts);
int dvo_amd_warp_forward(const dvo_amd_pyramid *moving, const double *T, const dvo_amd_view *view, int level, const dvo_amd_warp_options *opt,
                         float *depth_out, float *intensity_out, int *index_out, long long *counts);
int dvo_amd_warp_forward_many(int n, const dvo_amd_pyramid *const *moving, const double *T, const dvo_amd_view *views, int level,
                              const dvo_amd_warp_options *opt, float *const *depth_out, float *const *intensity_out, int *const *index_out,
                              long long *counts);
int dvo_amd_pyramid_warp_forward(const dvo_amd_pyramid *moving, const double *T, const dvo_amd_view *view, const dvo_amd_warp_options *opt,
                                 dvo_amd_pyramid **out, long long *counts);
int dvo_amd_pyramid_warp_forward_many(int n, const dvo_amd_pyramid *const *moving, const double *T, const dvo_amd_view *views,
                                      const dvo_amd_warp_options *opt, dvo_amd_pyramid **out, long long *counts);

/*
 * A truncated signed-distance volume on the device (dvo_amd_volume): keyframes fused into a dense voxel grid that is raycast
 * into a hole-free, denoised model view and from which surface points are pulled.  Context-free like the place index and the
 * warps: the device's prep stream, scratch from the slab pool, no tracker slot; calls on one volume are serialised by the caller.
 *
 * The store.  nx*ny*nz voxels, index L = (iz*ny + iy)*nx + ix (x fastest); origin is the world position of voxel (0,0,0)'s centre.
 * Per voxel four int32 sums {w_sum, sd_sum, iw_sum, i_sum} (dvo_amd_volume_voxel), all taken modulo 2^32, so subtracting what was
 * added is exact even after a wrap.  With |q| <= 2047 and a weight <= 256 per observation no sum has wrapped while a voxel holds
 * at most 4096 full-weight observations (4096 * 256 * 2047 < 2^31; i_sum: at most 2056 of them at the brightest grey value 4080).
 *
 * The integration rule, per voxel (ix,iy,iz) and frame (level `level` of a pyramid: intrinsics fx,fy,ox,oy, size w x h, planes Z
 * and I); all arithmetic fp32, every operation rounded on its own (no contraction), divisions correctly rounded.  pose: camera ->
 * world, column-major 4x4 doubles, NULL = identity; the host forms the rigid inverse M in double exactly as dvo_amd_map_render's
 * step 2 does and casts every entry to float.
 *  1. x = origin[0] + (float)ix*voxel, y and z alike; c_r = ((M_r0*x + M_r1*y) + M_r2*z) + M_r3 for r = x, y, z.  Position and
 *     transformation are formed from the indices for every voxel (a running sum along an axis would round differently);
 *  2. !(cz >= near_z): skip;
 *  3. px = (cx*fx)/cz + ox, py = (cy*fy)/cz + oy; pu = floorf(px + 0.5f), pv = floorf(py + 0.5f);
 *  4. !(0 <= pu && pu <= (float)(w-1) && 0 <= pv && pv <= (float)(h-1)), compared in float before any conversion: skip;
 *  5. Zs = Z[pv,pu], Is = I[pv,pu]; !(isfinite(Zs) && isfinite(Is) && Zs <= far_z): skip;
 *  6. d = Zs - cz; d < -trunc: skip (hidden);
 *  7. near = d <= trunc; dc = fminf(d, trunc); q = (int)rintf((dc/trunc)*2047.0f);
 *  8. weight: DVO_AMD_VOLUME_WEIGHT_CONSTANT: wgt = 1.  DVO_AMD_VOLUME_WEIGHT_SENSOR: s = 0.0012f + 0.0019f*((Zs-0.4f)*(Zs-0.4f))
 *     (depthStdDevZ), wgt = (int)fminf(fmaxf(rintf(256.0f*((0.0012f*0.0012f)/(s*s))), 1.0f), 256.0f);
 *  9. g = (int)fminf(fmaxf(rintf(Is*16.0f), 0.0f), 4080.0f);
 * 10. with sign = +1 or -1: w_sum += sign*wgt, sd_sum += sign*wgt*q; where near: iw_sum += sign*wgt, i_sum += sign*wgt*g.
 * Per frame three integer counts come back (dvo_amd_volume_counts): updated = near + free, the voxels that reached step 10.
 * A voxel with cz > far_z + trunc can never be updated, so the host bounds every frame by a conservative index box of (its
 * frustum between near_z and far_z + trunc) intersected with the volume, computed in double with a margin of a voxel; the launch
 * covers the union of the call's boxes and a voxel outside a frame's box skips that frame.  Culling drops only what the rule
 * skips: records and counts do not depend on it.
 *
 * Entries.  dvo_amd_volume_integrate is the anonymous form (no bookkeeping; sign -1 undoes sign +1 exactly).  The tracked form
 * mirrors the map: insert retains the pyramids until remove or destroy, set_poses subtracts a keyframe at its stored float inverse
 * pose and adds it at the new one in the same launch (a new pose whose inverse casts to the same floats does nothing), remove
 * subtracts.  One call is one kernel launch and one synchronisation whatever n is: a lane accumulates all frames of the call for
 * its voxel in registers and reads and writes each plane once.
 * The contract: after any sequence of successful calls the records equal those of a fresh volume into which the keyframes now
 * present were integrated at their current poses in one call -- bit for bit, independent of order, batching and launch geometry.
 * Errors: a failed call leaves the volume as it was.  DVO_AMD_ERR_INVALID_ARGUMENT with a reason in dvo_amd_last_error() that starts
 * with the entry's name: a NULL pointer (also inside an array); n < 0; a level beyond a pyramid (or negative); a non-finite pose
 * entry; sign other than +1 / -1; insert of an id already present, an unknown id in set_poses or remove, the same id twice in one
 * call; in create: a dimension outside 2..2048, nx*ny*nz > 2^30, voxel, trunc, near_z or far_z not finite and positive,
 * trunc < voxel, far_z <= near_z, a non-finite origin, an unknown weight.  Then DVO_AMD_ERR_DEVICE_MISMATCH, then
 * DVO_AMD_ERR_NO_DEVICE.  n == 0 is OK and does nothing.
 * dvo_amd_volume_download returns the records of an index box {x0,y0,z0,x1,y1,z1} (inclusive, NULL: the whole volume) in the
 * order of L; a capacity too small: DVO_AMD_ERR_CAPACITY with *n_out the size needed and records untouched.
 *
 * The raycast.  view: a dvo_amd_view, its near_z is where the march starts; step = step_fraction*trunc (fp32);
 * step_fraction in (0, 1], min_weight >= 1, fill_intensity finite and (far_z - near_z)/step <= 8192 or
 * DVO_AMD_ERR_INVALID_ARGUMENT; the view is checked as dvo_amd_warp_forward checks one.  Per pixel (u,v), with rows P of `pose`
 * cast to float:
 *  1. rx = ((float)u - ox)/fx, ry = ((float)v - oy)/fy;
 *  2. sample k is at t_k = near_z + (float)k*step (this product, never an accumulation); the march goes on while t_k <= far_z;
 *  3. x = rx*t, y = ry*t; p_r = ((P_r0*x + P_r1*y) + P_r2*t) + P_r3; g_a = (p_a - origin[a])/voxel;
 *  4. the sample is known iff 0 <= g_a && g_a < (float)(n_a - 1) on all axes (false for NaN) and all eight corners have
 *     w_sum >= min_weight;
 *  5. a corner's value is Fv = (float)sd_sum/(float)w_sum; trilinear blend with i0 = floorf(g), fr = g - i0: along x first,
 *     c00 = F000 + fr_x*(F100 - F000) and likewise c10 (y+1), c01 (z+1), c11 (y+1, z+1); then y, c0 = c00 + fr_y*(c10 - c00)
 *     and c1 = c01 + fr_y*(c11 - c01); then z, f = c0 + fr_z*(c1 - c0);
 *  6. with the previous sample known: f_prev > 0 && f <= 0 is a hit at t* = t_prev + step*(f_prev/(f_prev - f));
 *     f_prev < 0 && f > 0 ends the ray empty (backface); an unknown sample forgets f_prev; a ray that ends otherwise is missed;
 *  7. depth = t* (the ray's z component is 1: the camera's z depth);
 *  8. intensity: steps 3 to 5 at t = t* with Gv = (float)i_sum/(float)iw_sum in Fv's place, times 0.0625f; valid iff that sample
 *     satisfies step 4's inequalities and all eight corners have iw_sum > 0, otherwise the pixel counts as uncoloured and its
 *     intensity is empty;
 *  9. weight (may be NULL): w_sum of the corner nearest to the sample at t*, i0 + (fr >= 0.5f ? 1 : 0) per axis; 0 where the pixel
 *     is not hit or that sample fails step 4's inequalities;
 * 10. empty values are NaN (0x7FC00000) in the plane form; in the pyramid form every pixel that is not hit and coloured is empty
 *     in both planes (depth NaN, intensity fill_intensity), as dvo_amd_pyramid_warp_inverse does;
 * 11. stats: pixels = hit + backface + missed; uncoloured counts hit pixels.
 * One launch and one synchronisation per call; the pyramid form hands the device planes to the ordinary builder
 * (dvo_amd_pyramid_create_from_device's rules for width, height and levels).  There is no empty-space skipping.
 *
 * The surface.  dvo_amd_volume_extract writes one dvo_amd_point per crossing: candidates are voxel L and axis a in {x,y,z} where
 * the neighbour at +1 along a exists and both voxels have w_sum >= min_weight (>= 1); with Fa, Fb the two values (step 5's Fv)
 * there is a crossing iff (Fa > 0 && Fb <= 0) || (Fa <= 0 && Fb > 0); s = Fa/(Fa - Fb); the coordinate along a is
 * origin[a] + ((float)i_a + s)*voxel, the other two are the voxel centre's (step 1 of the integration rule).  Colour: with
 * iw_sum > 0 on both voxels grey = (int)fminf(fmaxf(rintf((Ga + s*(Gb - Ga))*0.0625f), 0.0f), 255.0f), packed B = G = R; otherwise
 * rgb = 0 and the point counts as uncoloured.  Points come in ascending 3*L + a.  Capacity as in dvo_amd_map_extract:
 * DVO_AMD_ERR_CAPACITY with *n_out the size needed and out untouched.  The result goes straight into dvo_amd_write_pcd.
 *
 * The mesh.  dvo_amd_volume_mesh writes the same surface as an indexed triangle mesh by naive surface nets: one vertex per cell
 * the surface runs through, one quad (two triangles) per crossing edge, i.e. per point of dvo_amd_volume_extract.  All arithmetic
 * fp32, every operation rounded on its own (no contraction), divisions and the square root correctly rounded.
 *  Cells.  Cell C = (cx,cy,cz), 0 <= c_a <= n_a - 2, index Lc = (cz*(ny-1) + cy)*(nx-1) + cx; its corner k = dx + 2*dy + 4*dz is
 *   voxel (cx+dx, cy+dy, cz+dz).  A cell is KNOWN iff all eight corners have w_sum >= min_weight (>= 1).  F_k = (float)sd_sum /
 *   (float)w_sum (the raycast's step 5); corner k is INSIDE iff F_k <= 0, so the two corners of an edge differ in this exactly
 *   when dvo_amd_volume_extract sees a crossing there.  A cell is ACTIVE iff it is known and its corners are neither all inside
 *   nor all outside.  Vertices: one per active cell in ascending Lc; a vertex's index is its rank in that order.
 *  Edges.  The twelve edges of a cell are walked in the order e = 4*a + j: axis a = 0,1,2, the other two axes (b,c) = (1,2), (2,0),
 *   (0,1) (cyclic), j = db + 2*dc; the edge runs from corner lo (offset 0 along a, db along b, dc along c) to corner hi (offset 1
 *   along a, the same along b and c); Fa = F_lo, Fb = F_hi; it crosses iff (Fa > 0 && Fb <= 0) || (Fa <= 0 && Fb > 0).
 *  Position.  Over the crossing edges in order e: s = Fa/(Fa - Fb); the crossing's local point is s along a, (float)db along b,
 *   (float)dc along c; three sums S_x, S_y, S_z start at 0 and add the local points one after the other; m = the number of
 *   crossings (>= 3 in an active cell); p_a = S_a/(float)m; the coordinate is origin[a] + ((float)c_a + p_a)*voxel.
 *  Colour.  Over the crossing edges whose two voxels both have iw_sum > 0, in order e: g = Ga + s*(Gb - Ga) with
 *   Gv = (float)i_sum/(float)iw_sum, added one after the other to a sum that starts at 0; mc of them.  mc > 0:
 *   grey = (int)fminf(fmaxf(rintf((sum/(float)mc)*0.0625f), 0.0f), 255.0f), packed B = G = R; otherwise rgb = 0 and the vertex
 *   counts as uncoloured.
 *  Normal (normals may be NULL; 3 floats per vertex): the gradient of F over the cell.  G_a starts at 0 and adds (Fb - Fa) of the
 *   axis's four edges in order j, crossing or not; len = sqrtf((G_x*G_x + G_y*G_y) + G_z*G_z); n = (G_x/len, G_y/len, G_z/len);
 *   len == 0 (a 3-D checkerboard of signs): n = (0,0,0) and the vertex counts as flat.  F is positive in front of the surface,
 *   so the normal points out of the solid, towards where the cameras were.
 *  Faces.  Over dvo_amd_volume_extract's candidates (L, a) that cross, in ascending 3*L + a, voxel (ix,iy,iz), (b,c) as above: the
 *   four cells around the edge have i_a along a and (i_b-1, i_c-1), (i_b, i_c-1), (i_b, i_c), (i_b-1, i_c) along (b,c): q0..q3,
 *   counter-clockwise seen from +a.  If one of them does not exist or is not known the edge yields no face and counts as open;
 *   otherwise two triangles on the diagonal q0-q2: (q0,q1,q2), (q0,q2,q3) when Fb > 0 (the surface faces +a), else (q0,q2,q1),
 *   (q0,q3,q2).  Triangles are int vertex indices, three each, in that order.  (A known cell around a crossing edge is active.)
 *  So triangles/2 + open_edges == the points of dvo_amd_volume_extract for the same min_weight, and a closed surface inside the
 *  known region comes out closed, consistently oriented (counter-clockwise seen from outside) with normals on the faces' side.
 *  What the rule does not promise: where two solids touch along an edge or at a corner the mesh is not manifold there (surface
 *  nets' known ambiguity: one vertex serves both sheets); an active cell at the rim of the known region has a vertex that no face
 *  may use; a quad is split on a fixed diagonal, whatever its shape.
 * counts (never NULL) receives {vertices, triangles, open_edges, uncoloured, flat}.  Capacities are in vertices and in triangles:
 * if either is too small the call returns DVO_AMD_ERR_CAPACITY with counts->vertices, ->triangles and ->open_edges set (the other
 * two 0) and no array touched.  Three launches and one synchronisation find the sizes, two launches and a second synchronisation
 * write (one launch when there is no face, none when there is no vertex), whatever the volume holds.  Nothing is kept per cell but
 * one bit; there is no floating-point atomic.  Argument errors as above: a NULL volume or counts, min_weight < 1, a negative
 * capacity, a capacity without its array.
 *
 * dvo_amd_volume_upload is the inverse of dvo_amd_volume_download: it overwrites the records of the box (NULL: the whole volume)
 * with n records in the order of L; n must be the number of voxels of the box.  It saves and restores a volume, and places crafted
 * records.  While the tracked form holds keyframes it returns DVO_AMD_ERR_INVALID_ARGUMENT, because their contract (above)
 * would no longer hold: remove them or clear first.
 */
#define DVO_AMD_VOLUME_WEIGHT_CONSTANT 0
#define DVO_AMD_VOLUME_WEIGHT_SENSOR 1
#define DVO_AMD_VOLUME_MAX_STEPS 8192

typedef struct {
  int nx, ny, nz;      /* 2..2048 each, nx*ny*nz <= 2^30 */
  float voxel;         /* edge of a voxel in metres */
  float origin[3];     /* world position of the centre of voxel (0,0,0) */
  float trunc;         /* truncation distance, >= voxel */
  float near_z, far_z; /* sensor depths used: cz >= near_z, Zs <= far_z */
  int weight;          /* DVO_AMD_VOLUME_WEIGHT_CONSTANT or _SENSOR */
} dvo_amd_volume_options;

typedef struct {
  int w_sum, sd_sum, iw_sum, i_sum;
} dvo_amd_volume_voxel;

typedef struct {
  long long updated, near, free;
} dvo_amd_volume_counts;

typedef struct {
  float step_fraction;  /* 0.5; in (0, 1] */
  int min_weight;       /* 1; >= 1 */
  float fill_intensity; /* 0: an empty pixel's intensity in the pyramid form */
} dvo_amd_volume_raycast_options;

typedef struct {
  long long pixels, hit, backface, missed, uncoloured;
} dvo_amd_volume_raycast_stats;

typedef struct {
  long long points, uncoloured;
} dvo_amd_volume_extract_counts;

typedef struct {
  long long vertices, triangles, open_edges, uncoloured, flat;
} dvo_amd_volume_mesh_counts;

typedef struct dvo_amd_volume dvo_amd_volume;
/* 64 x 64 x 64 voxels of 0.05 m, origin (-1.6, -1.6, 0.4), trunc 0.15, near_z 0.4, far_z 5, sensor weights */
void dvo_amd_default_volume_options(dvo_amd_volume_options *opt);
/* step_fraction 0.5, min_weight 1, fill_intensity 0 */
void dvo_amd_default_volume_raycast_options(dvo_amd_volume_raycast_options *opt);
int dvo_amd_volume_create(int device, const dvo_amd_volume_options *opt, dvo_amd_volume **out);
void dvo_amd_volume_destroy(dvo_amd_volume *vol);
/* all records to zero; the keyframes of the tracked form are released */
int dvo_amd_volume_clear(dvo_amd_volume *vol);
int dvo_amd_volume_options_get(const dvo_amd_volume *vol, dvo_amd_volume_options *opt);
/* poses: NULL (all identity) or n x 16 doubles, column-major each; counts: NULL or n records */
int dvo_amd_volume_integrate(dvo_amd_volume *vol, int n, const dvo_amd_pyramid *const *pyramids, int level, const double *poses, int sign,
                             dvo_amd_volume_counts *counts);
int dvo_amd_volume_insert(dvo_amd_volume *vol, int n, const int *ids, dvo_amd_pyramid *const *pyramids, int level, const double *poses,
                          dvo_amd_volume_counts *counts);
int dvo_amd_volume_set_poses(dvo_amd_volume *vol, int n, const int *ids, const double *poses);
int dvo_amd_volume_remove(dvo_amd_volume *vol, int n, const int *ids);
/* n_keyframes: the keyframes of the tracked form; updated_total: the sum of their `updated` counts at their current poses */
int dvo_amd_volume_stats(const dvo_amd_volume *vol, int *n_keyframes, long long *updated_total);
/* box: NULL or {x0,y0,z0,x1,y1,z1}, inclusive voxel indices with 0 <= x0 <= x1 < nx and alike */
int dvo_amd_volume_download(dvo_amd_volume *vol, const int *box, dvo_amd_volume_voxel *records, long long capacity, long long *n_out);
/* any of depth / intensity / weight / stats may be NULL; each plane is width*height, row-major, host memory */
int dvo_amd_volume_raycast(dvo_amd_volume *vol, const double *pose, const dvo_amd_view *view, const dvo_amd_volume_raycast_options *opt,
                           float *depth, float *intensity, int *weight, dvo_amd_volume_raycast_stats *stats);
int dvo_amd_volume_raycast_pyramid(dvo_amd_volume *vol, const double *pose, const dvo_amd_view *view,
                                   const dvo_amd_volume_raycast_options *opt, int levels, double timestamp, dvo_amd_pyramid **out,
                                   dvo_amd_volume_raycast_stats *stats);
int dvo_amd_volume_extract(dvo_amd_volume *vol, int min_weight, dvo_amd_point *out, long long capacity, long long *n_out,
                           dvo_amd_volume_extract_counts *counts);
/* vertices: vertex_capacity records; normals: NULL or 3 floats per vertex; triangles: 3 ints per triangle; host memory */
int dvo_amd_volume_mesh(dvo_amd_volume *vol, int min_weight, dvo_amd_point *vertices, float *normals, long long vertex_capacity, int *triangles,
                        long long triangle_capacity, dvo_amd_volume_mesh_counts *counts);
/* box: as in dvo_amd_volume_download; n: the number of voxels of the box */
int dvo_amd_volume_upload(dvo_amd_volume *vol, const int *box, const dvo_amd_volume_voxel *records, long long n);

/* PLY, format binary_little_endian 1.0: element vertex with float x y z, with normals float nx ny nz (3 floats per vertex, as
 * dvo_amd_volume_mesh writes them), uchar red green blue (from the packed rgb); element face with `list uchar int vertex_indices`,
 * three indices each.  DVO_AMD_ERR_INVALID_ARGUMENT: a NULL path or array, a negative count, an index outside 0..n_vertices-1.
 * Host code only. */
int dvo_amd_write_ply(const char *path, const dvo_amd_point *vertices, const float *normals, long long n_vertices, const int *triangles,
                      long long n_triangles);

/* Binary PCD v0.7 as pcl::io::savePCDFileBinary writes a PointXYZRGB cloud: FIELDS x y z rgb, SIZE 4 4 4 4, TYPE F F F F
 * (rgb holds the packed bits), COUNT 1 1 1 1, WIDTH / HEIGHT as given (organized, or n x 1), VIEWPOINT 0 0 0 1 0 0 0,
 * POINTS width*height (= n), then the records.  Host code only. */
int dvo_amd_write_pcd(const char *path, const dvo_amd_point *points, long long n, int width, int height);

/*
 * Surface normals (RgbdImage::calculateNormals, rgbd_image.cpp:502-532; its members `normals`, CV_32FC4, and `angles`, CV_32FC1).
 *
 * Which way the surface under a pixel faces, from a pyramid level's depth plane and rays.  The reference takes the cross
 * product of the one-pixel central differences of the back-projected points; on sensor depth (noise of depthStdDevZ, 1/5000 m
 * steps) that alone is off by tens of degrees, so the rule here is the reference's plus a windowed, depth-aware sum of the
 * un-normalised cross products (DESIGN.md 4.18 has the measured errors).  With every option 0 it IS the reference's rule.
 *
 * The rule for level l of a pyramid, size w x h, pixel (u, v).  All arithmetic is fp32, round to nearest; every product, sum,
 * quotient and square root is rounded on its own (no contraction), sqrtf and / are the correctly rounded ones, denormals are kept.
 *  1. point: P(u,v) = (tx[u]*z, ty[v]*z, z), z the level's depth plane, tx / ty the level's rays: the bits dvo_amd_point_cloud
 *     produces at the identity pose;
 *  2. raw cross product c(u,v), with the reference's clamped indices:
 *       a = P(min(u+1,w-1), v) - P(max(u-1,0), v),   b = P(u, min(v+1,h-1)) - P(u, max(v-1,0)),
 *       c = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x);  c is USABLE iff its three components are finite;
 *  3. window sum, r = opt.radius[l] (0 <= r <= DVO_AMD_NORMAL_MAX_RADIUS): the pixel is UNDEFINED if its own z is not finite.
 *     Otherwise the members (u+du, v+dv) are visited with dv = -r..r outer and du = -r..r inner; a member is added iff it lies
 *     inside the plane, its c is usable and, when opt.depth_step_ratio > 0, fabsf(z_member - z) <= opt.depth_step_ratio * z.
 *     m is the first added member's c as it is; every later member is added to it component by component, in that order.  No
 *     member added: the pixel is undefined.  (r = 0 with ratio 0 is exactly the reference's per-pixel rule.)
 *  4. normalise: s = (m.x*m.x + m.y*m.y) + m.z*m.z; if !(s >= 1e-30f) the pixel is undefined; len = sqrtf(s);
 *     n = (m.x/len, m.y/len, m.z/len, 0);
 *  5. orientation: d = (n.x*P.x + n.y*P.y) + n.z*P.z with the centre's P; with opt.toward_camera != 0 and d > 0 the three
 *     components are negated (the default 0 keeps the reference's sign);
 *  6. facing value: DVO_AMD_NORMAL_FACING_AXIS (the reference's `angles`): fabsf(n.z); DVO_AMD_NORMAL_FACING_RAY:
 *     fabsf(d) / sqrtf((P.x*P.x + P.y*P.y) + P.z*P.z), the cosine between the normal and the viewing ray, NaN when that
 *     square is not > 0;
 *  7. undefined pixels: all four normal components are NaN (what normalize() of a NaN vector leaves in the reference), and so
 *     is the facing value.
 * The result is a function of the pyramid and the options alone: not of the launch geometry, not of the tiles a level is cut
 * into.  There is no floating-point atomic; the counts are integers.
 *
 * Departures from the reference: Eigen's cross3 / normalize take their sums in Eigen's order, which is not pinned here (like
 * the point cloud's transform): the two agree to fp32 rounding, not bit for bit.  A zero-length cross product (s < 1e-30) is
 * undefined here; the reference divides by its length.
 *
 * dvo_amd_pyramid_normals: one level into host memory, one kernel launch and one synchronisation.
 * dvo_amd_mask_from_normals: an ordinary mask (dvo_amd_mask_create's kind: erode it, warp it, match behind it) of the
 * pyramid's size and level count: 1 iff the pixel is defined and its facing value >= min_facing[l] (a NaN facing value: 0);
 * an undefined pixel: undefined_keep != 0.  One kernel launch for all levels and one synchronisation.
 * dvo_amd_point_cloud_normals: dvo_amd_point_cloud (the same arguments, the same bits in `out`) plus every point's normal in
 * the pose's frame: R = (float)pose's rotation element by element, n' = ((R_r0*n.x + R_r1*n.y) + R_r2*n.z) per row r, the
 * fourth component carried over; an undefined pixel stays four NaNs.  pose NULL: the identity, applied the same way.
 * dvo_amd_write_pcd_normals: binary PCD v0.7 as pcl::io::savePCDFileBinary writes a PointXYZRGBNormal cloud: FIELDS x y z rgb
 * normal_x normal_y normal_z curvature, SIZE 4 x 8, TYPE F x 8, COUNT 1 x 8, 32-byte records (curvature 0); `normals` holds
 * four floats per point, of which the first three are written.  Host code only.
 *
 * No context is needed except by the cloud; the entries run on the device's internal stream with storage of the call's own and
 * keep nothing: the pyramid is only read.  DVO_AMD_ERR_INVALID_ARGUMENT comes first and needs no device, with a reason in
 * dvo_amd_last_error() that starts with the entry's name: a NULL pyramid, options, min_facing or output; a level the pyramid
 * does not have; a radius outside 0..DVO_AMD_NORMAL_MAX_RADIUS on a level the pyramid has; a depth_step_ratio that is negative
 * or not finite; an unknown `facing`; a NaN min_facing[l]; a non-finite pose entry.  Then DVO_AMD_ERR_DEVICE_MISMATCH, then
 * DVO_AMD_ERR_NO_DEVICE.  *out is NULL after every failure.
 */
#define DVO_AMD_NORMAL_MAX_RADIUS 8
#define DVO_AMD_NORMAL_FACING_AXIS 0
#define DVO_AMD_NORMAL_FACING_RAY 1
typedef struct dvo_amd_normal_options {
  int radius[DVO_AMD_MAX_LEVELS];   /* 0..DVO_AMD_NORMAL_MAX_RADIUS per level */
  float depth_step_ratio;           /* >= 0, finite; 0: no test */
  int facing;                       /* DVO_AMD_NORMAL_FACING_AXIS | DVO_AMD_NORMAL_FACING_RAY */
  int toward_camera;
} dvo_amd_normal_options;
/* all 0: RgbdImage::calculateNormals; a NULL opt is a no-op */
void dvo_amd_default_normal_options(dvo_amd_normal_options *opt);
/* normals: w*h*4 floats, facing: w*h floats, host memory, either may be NULL; counts: {defined, undefined} or NULL */
int dvo_amd_pyramid_normals(const dvo_amd_pyramid *p, int level, const dvo_amd_normal_options *opt, float *normals, float *facing,
                            long long *counts);
/* min_facing: one value per level of p; counts: per level {defined, undefined, kept}, or NULL */
int dvo_amd_mask_from_normals(const dvo_amd_pyramid *p, const dvo_amd_normal_options *opt, const float *min_facing,
                              int undefined_keep, dvo_amd_mask **out, long long *counts);
/* out: w*h points of the level; normals: w*h*4 floats */
int dvo_amd_point_cloud_normals(dvo_amd_context *ctx, dvo_amd_pyramid *image, int level, const double *pose, const unsigned char *bgr,
                                int bgr_stride_bytes, const dvo_amd_normal_options *opt, dvo_amd_point *out, float *normals);
int dvo_amd_write_pcd_normals(const char *path, const dvo_amd_point *points, const float *normals, long long n, int width, int height);

/*
 * Mask components: connected-component labelling of a mask, of a depth plane or of both, with per-component statistics -- on the
 * device.
 *
 * Every producer of masks makes speckle (isolated residual outliers, normals that flicker at grazing angles, single-pixel
 * disagreements of a warp along depth edges), and dvo_amd_mask_morph's erode removes thin true structure with it.  The entries
 * below tell a 3-pixel speckle from a 3000-pixel object: they drop components by area, keep the k largest, or keep the
 * components a trusted (eroded) mask still touches -- an erosion's speckle removal without its loss of shape.  With a pyramid's
 * depth the same kernels segment a frame into depth-connected surfaces (cv::filterSpeckles' case: a floating blob larger than
 * dvo_amd_pyramid_filter_depth's window).  Inputs are only read; the result is an ordinary dvo_amd_mask -- immutable,
 * refcounted, with a serial of its own -- that enters wherever a mask enters.
 *
 * Processing.  Each level is processed on its own, from the same level of its inputs, as dvo_amd_mask_morph does.
 * Foreground.  Pixel i of level l is foreground iff (mask is NULL or mask[l][i] != 0) and (depth is NULL or the depth plane of
 * level l of the pyramid `depth` is finite at i).  At least one of mask and depth must be given.
 * Edges.  Two foreground pixels are adjacent under connectivity 4 (left/right, up/down) or 8 (plus the diagonals); nothing wraps
 * at the plane's border.  Without depth every adjacent foreground pair is an edge.  With depth an adjacent pair (a, b) is an
 * edge iff, in fp32, every operation rounded on its own, no contraction,
 *     zn  = fminf(za, zb)
 *     t   = zn - 0.4f
 *     tol = max_step + depth_sigmas * (0.0012f + 0.0019f * (t * t))
 *     fabsf(za - zb) <= tol
 * which is the project's depthStdDevZ (the mask warp's and the depth fusion's) evaluated at the nearer depth, so that the rule
 * is symmetric.  Components are the connected components of that undirected graph.  The relation is NOT transitive pixel to
 * pixel: a ramp whose every step passes is one component, however far apart its ends are.  That is intended -- a floor seen at
 * a grazing angle is one surface.
 * Canonical names.  The root of a component is its smallest linear pixel index y * w + x; its label is root + 1; background is
 * 0.  Every output below is therefore a function of the inputs alone, whatever order the device worked in.
 * Per-component record.  dvo_amd_component {root, area, x0, y0, x1, y1, seeded}: the inclusive bounding box, and seeded = 1 iff
 * `seeds` is given and keeps at least one pixel of the component on that level.
 * Filter.  A component is kept iff all three hold:
 *     min_area[l] <= area, and max_area[l] < 0 or area <= max_area[l];
 *     seeds is NULL or the component is seeded;
 *     keep_largest == 0, or the component is among the first keep_largest of those that passed the two tests before, ordered by
 *     (area descending, root ascending).
 * keep_largest ranges over 0 .. DVO_AMD_COMPONENTS_MAX_LARGEST.  The output mask keeps exactly the pixels of kept components; it
 * has the input's level-0 size and level count (with mask NULL: the pyramid's).
 * Counts (may be NULL).  One record of DVO_AMD_COMPONENTS_COUNTS long long per level, in item order:
 *     foreground, components, kept_components, kept_pixels, largest_area, edges_cut
 * largest_area is the area of the level's largest component, kept or not (0 without any).  edges_cut is the number of adjacent
 * foreground pairs under the chosen connectivity that the depth rule refused, each pair counted once; 0 without depth.
 *
 * Defaults (dvo_amd_default_component_options): connectivity 8, max_step 0, depth_sigmas 10, every min_area 0, every max_area
 * -1, keep_largest 0 -- with these the call returns the foreground unchanged.  depth_sigmas 10 is a default, not a bar: on the
 * project's synthetic 160x120 and 80x60 sensor frames 6 was the smallest of {3, 6, 10, 20} at which the smooth room stays one
 * component (at 3 it shatters into 7 to 28), and 10 leaves a margin over that.
 *
 *   dvo_amd_mask_filter_components        one item
 *   dvo_amd_mask_filter_components_many   n items that may differ in size and level count, as dvo_amd_pyramid_filter_depth_many's;
 *                                         depths and seeds may be NULL or hold NULL entries, masks may too where the item has a
 *                                         depth.  All items and levels share every kernel launch: a call is FIVE launches (tile
 *                                         labelling, seams, flatten + records, selection, write) whatever the content, n or the
 *                                         level count; nothing comes back to the host between them and the call synchronises
 *                                         once, at its end.  An item's outputs equal its single call's, bit for bit.
 *   dvo_amd_mask_components               the inspection entry for one level: the label plane (w * h ints of that level, may be
 *                                         NULL) and the records in ascending root order.  *n_components is always the true
 *                                         total; at most `capacity` records are written.  It reads opt only for the edge rule
 *                                         (connectivity, max_step, depth_sigmas); the other fields are still validated (keep_largest, and
 *                                         min_area on the levels the item has).
 * All atomics are integer and the canonical root makes every output order-independent: two runs are bit-identical.
 * Working memory.  A call labels in 41 bytes per pixel of all its items and levels together (an int32 parent, a 32-byte record,
 * a work-list entry and an edge byte; each plane rounded up to 256 pixels): 16.7 MB for one 640x480 item of four levels, 1.07 GB
 * for 64 of them in one call.  It is one area per device, grown to the largest call so far and kept for the life of the process,
 * as the mask warp's table is -- a caller to whom a gigabyte matters splits a large _many call into smaller ones.
 *
 * Errors, all reported before any device work, with *out NULL (every out[k] NULL) on every failure:
 * DVO_AMD_ERR_INVALID_ARGUMENT, with a reason in dvo_amd_last_error(), for NULL where not allowed (including inside the
 * arrays), mask and depth both NULL, a connectivity other than 4 or 8, a max_step or depth_sigmas that is not finite or is
 * negative, min_area[l] < 0 on a level the item has, keep_largest outside its range, a depth or seeds that does not fit the mask
 * as dvo_amd_pyramid_select_masked checks a mask (another level-0 size, or fewer levels), a level outside the item's levels, a
 * negative capacity; then DVO_AMD_ERR_DEVICE_MISMATCH; then DVO_AMD_ERR_NO_DEVICE.
 *
 * Not covered: no hole-filling of components, no labels cached in a mask, no removal of depth from a pyramid (one tracks behind
 * the mask), no 3-D connectivity over the map's voxels.
 */
#define DVO_AMD_COMPONENTS_MAX_LARGEST 8
#define DVO_AMD_COMPONENTS_COUNTS 6 /* foreground, components, kept_components, kept_pixels, largest_area, edges_cut */
typedef struct dvo_amd_component_options {
  int connectivity;                     /* 4 or 8 */
  float max_step;                       /* metres added to the depth tolerance; >= 0 */
  float depth_sigmas;                   /* multiples of depthStdDevZ at the nearer depth; >= 0 */
  int min_area[DVO_AMD_MAX_LEVELS];     /* per level; >= 0 */
  int max_area[DVO_AMD_MAX_LEVELS];     /* per level; < 0: no upper bound */
  int keep_largest;                     /* 0: all that pass; else 1 .. DVO_AMD_COMPONENTS_MAX_LARGEST */
} dvo_amd_component_options;
typedef struct dvo_amd_component {
  int root, area, x0, y0, x1, y1, seeded;
} dvo_amd_component;

void dvo_amd_default_component_options(dvo_amd_component_options *opt);
int dvo_amd_mask_filter_components(const dvo_amd_mask *mask, const dvo_amd_pyramid *depth, const dvo_amd_mask *seeds,
                                   const dvo_amd_component_options *opt, dvo_amd_mask **out,
                                   long long *counts /* [levels][6] or NULL */);
int dvo_amd_mask_filter_components_many(int n, const dvo_amd_mask *const *masks, const dvo_amd_pyramid *const *depths,
                                        const dvo_amd_mask *const *seeds, const dvo_amd_component_options *opt,
                                        dvo_amd_mask **out /* n */, long long *counts /* packed in item order, or NULL */);
int dvo_amd_mask_components(const dvo_amd_mask *mask, const dvo_amd_pyramid *depth, const dvo_amd_mask *seeds,
                            const dvo_amd_component_options *opt, int level, int *labels /* w*h of that level, may be NULL */,
                            dvo_amd_component *components, int capacity, int *n_components);

/* dvo::core::computeResidualsAndValidFlagsSse (dense_tracking_impl.cpp:400-403) for one level and one float transform
 * (column-major 4x4, reference -> current).  residuals: width*height x 2 floats in pixel order, NaN where the pixel is not
 * selected or its warp is invalid.  Used by the parity tests and by dvo_amd_error_image. */
int dvo_amd_residuals(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, int level,
                      const float *T, float *residuals, int *n_valid);
/* DenseTracker::computeIntensityErrorImage, dense_tracking.cpp:378-444: |intensity residual| per reference pixel, 0 elsewhere */
int dvo_amd_error_image(dvo_amd_context *ctx, dvo_amd_pyramid *reference, dvo_amd_pyramid *current, const double *T,
                        int level, float *image);


/*
 * Pose-graph optimization (KeyframeGraph's g2o::SparseOptimizer with OptimizationAlgorithmDogleg, keyframe_graph.cpp:137-144,
 * and LocalMap::optimize's OptimizationAlgorithmLevenberg, local_map.cpp:205-210; both over VertexSE3 / EdgeSE3 with an
 * optional RobustKernelCauchy).  The semantics are pinned here, not by g2o's source; tests/pose_graph_restatement.py restates
 * them in float64 numpy.
 *
 * Vertices: SE3 poses, column-major double[16].  A vertex is free unless fixed[i] != 0 (fixed may be NULL: all free).  A vertex
 * touched by no edge is inactive and returned unchanged (g2o's initializeOptimization leaves it out).  The unknowns are the free
 * active vertices in increasing vertex index, m of them, n = 6m unknowns.
 * Increment (VertexSE3::oplusImpl, fromVectorMQT): X <- X * inc(d), d = (tx, ty, tz, qx, qy, qz); inc(d) has translation t and
 * the rotation of the quaternion (w, qx, qy, qz), w = sqrt(1 - |q|^2); when 1 - |q|^2 < 0 the rotation is the identity.  g2o
 * re-normalises a vertex's rotation every 1000 updates; this entry does not.
 * Edge error (EdgeSE3::computeError, toVectorMQT): edge (from, to, Z, Omega), Delta = Z^-1 * (X_from^-1 * X_to) (inverses of
 * isometries: (R^T, -R^T t)), e = (t(Delta), q_xyz(Delta)) with q the unit quaternion of R(Delta) (Eigen's Quaternion(R),
 * normalised) with its sign chosen so that w >= 0; chi2 = e^T Omega e.
 * Jacobians: analytic, of e with respect to d_from and d_to at d = 0, in fp64.  With R, t the rotation and translation of Delta,
 * (w, v) its quaternion, Rz, tz those of Z and [a]x the cross-product matrix:
 *   J_to   = [ R      0                         ]      J_from = [ -Rz^T   2 ([t]x Rz^T + Rz^T [tz]x) ]
 *            [ 0      w I + [v]x                ]               [ 0       -(w I - [v]x) Rz^T          ]
 * (rows: t, q_xyz; columns: translation, quaternion part of d).  inc(d) rotates by I + 2[dq]x to first order; J_to is
 * Delta*inc(d), J_from is Z^-1 inc(d)^-1 Z Delta.
 * Robust kernel (RobustKernelCauchy): delta > 0 and a = chi2 / delta^2 + 1 (computed as (1/delta^2) * chi2 + 1):
 * rho0 = delta^2 log a, rho1 = 1 / a; delta <= 0: rho0 = chi2, rho1 = 1.  The objective is F = sum over edges of rho0.
 * Normal equations (BaseBinaryEdge::constructQuadraticForm with robustInformation = rho1 Omega, no second-order term):
 * H += J_i^T (rho1 Omega) J_j and b -= J_i^T (rho1 Omega) e over the edge's free blocks; H x = b; x is applied vertex by vertex
 * with inc.  A Cholesky pivot <= 0 (or NaN) is a failed solve.
 * Levenberg-Marquardt (OptimizationAlgorithmLevenberg::solve): at the first iteration of a call lambda = 1e-5 * max diag(H), or
 * initial_lambda when > 0, and nu = 2.  Every iteration linearises once and makes up to max_trials attempts: solve
 * (H + lambda I) x = b, apply x, evaluate F' (+inf for a failed solve, whose x is not applied), rho = (F - F') /
 * (1e-3 + sum x_i (lambda x_i + b_i)) (rho = -inf for a failed solve).  rho > 0 and F' finite: lambda *= max(1/3, min(2/3,
 * 1 - (2 rho - 1)^3)), nu = 2, the step is kept and the iteration ends.  Otherwise lambda *= nu, nu *= 2, the estimate is
 * restored, and the attempts go on while rho < 0.  The call terminates (DVO_AMD_GRAPH_TERMINATE) when an iteration used all
 * max_trials attempts, ended with rho == 0, or left lambda non-finite.
 * Dogleg (OptimizationAlgorithmDogleg::solve): per call Delta = initial_delta (1e4), lambda = initial_lambda (1e-7), and
 * "positive definite so far".  Per iteration: h_sd = alpha b with alpha = |b|^2 / (b^T H b); h_gn solves H x = b undamped while
 * every solve so far succeeded; from the first failed Cholesky on it solves (H + lambda I) x = b, a failure multiplies lambda
 * by 10 (the call fails, DVO_AMD_GRAPH_FAIL, when lambda would exceed 1e3), a success sets lambda = max(1e-12, lambda / 5).
 * h_gn is solved once per iteration.  The step h: h_gn if |h_gn| < Delta; else (Delta / |h_sd|) h_sd if |h_sd| > Delta; else
 * h_sd + beta (h_gn - h_sd) with c = h_sd . (h_gn - h_sd), s = |h_gn - h_sd|^2 and beta = (-c + sqrt(c^2 + s (Delta^2 -
 * |h_sd|^2))) / s when c <= 0, (Delta^2 - |h_sd|^2) / (c + sqrt(c^2 + s (Delta^2 - |h_sd|^2))) otherwise.  Linear gain
 * g = 2 b^T h - h^T H h, replaced by 1e-12 when |g| < 1e-12; rho = (F - F') / g; the step is kept if rho > 0; then Delta =
 * max(Delta, 3 |h|) if rho > 0.75, Delta /= 2 if rho < 0.25.  Up to max_trials (100) attempts per iteration without
 * re-linearising; the call terminates when an iteration used all max_trials attempts or kept no step.
 * Outputs: the optimized poses of all vertices (fixed and inactive ones bit for bit as given); per edge chi2 and rho1 at the
 * final estimate (what removeOutlierConstraints, keyframe_graph.cpp:643-675, thresholds); per iteration F after it, the norm of
 * the kept step (0 when none), lambda and Delta after it, the attempts made and whether a step was kept.  An iteration that
 * ends the call, a failing dogleg one included, is counted and recorded.
 * Determinism: every sum has a fixed order (by edge index within a block, a fixed tile order in the factorization, fixed-shape
 * reductions); no floating-point atomics: the result is a function of the inputs in their order and of the options alone,
 * bit-identical between runs and contexts on one device.
 * Limits and solvers (options.solver):
 * DVO_AMD_GRAPH_SOLVER_DENSE (0, the default): H is solved densely (O(n^3) per factorization, fp64; H is n x n on the
 * device).  That fits a keyframe-only graph and the dense final graph of a sequence of some hundred frames (fr1/desk: 573
 * frames, n = 3438); more than DVO_AMD_GRAPH_MAX_FREE_VERTICES (1024) free active vertices return DVO_AMD_ERR_CAPACITY with
 * poses untouched.
 * DVO_AMD_GRAPH_SOLVER_SPARSE (1): a multifrontal sparse Cholesky on the 6 x 6 block pattern of H (g2o's LinearSolverCSparse
 * role), for the one-vertex-per-frame final graph of sequences of thousands of frames.  Once per call the host orders the free
 * active vertices by nested dissection (recursive bisection with BFS level-structure vertex separators, down to parts of at
 * most 16 vertices or parts no BFS level separates; components as a forest).  The order and the assembly tree are a function
 * of the graph's structure alone (the free active vertices, the edges and their order; ties go by vertex slot).  H is stored
 * as its nonzero 6 x 6 blocks, each bit-identical to the same block of the dense path's H; the factorization runs level by
 * level up the assembly tree, and a call with no free active vertex returns DVO_AMD_OK with poses untouched, as the dense
 * path does.
 *   - Same iteration semantics: every rule above (increment, error, Jacobians, Cauchy kernel, Levenberg and dogleg drivers,
 *     failure rules) applies unchanged.
 *   - A different elimination order and summation order: solves, b^T H b and h^T H h agree with the dense path to rounding,
 *     not bit for bit, and so may the iterations built on them.
 *   - Deterministic: no floating-point atomics; results are bit-identical between runs and contexts on one device.
 *   - A pivot <= 0 or NaN in any front is a failed solve, counted in cholesky_failures, and the step is not applied.
 *   - A zero row or column of H fails on both paths.  A numerically singular system (a component with no fixed vertex) or a
 *     near-singular one may fail on one path and not on the other: the two orders round differently.
 *   - More than DVO_AMD_GRAPH_MAX_FREE_VERTICES_SPARSE (65536) free active vertices return DVO_AMD_ERR_CAPACITY with poses
 *     untouched (slots and block indices are 32-bit; 6 x 65536 unknowns index every front and vector in int).  When the
 *     storage the symbolic phase predicts for the sparse solver (front matrices and vectors, H blocks, index maps) exceeds
 *     90 % of the device's free memory plus what the context already holds of it, the call returns
 *     DVO_AMD_ERR_OUT_OF_MEMORY with poses untouched, as does a device allocation that fails later; there is no fall-back to
 *     another path.
 * Argument checks come first and need no device: DVO_AMD_ERR_INVALID_ARGUMENT for an out-of-range vertex index, from == to, a
 * non-finite measurement, information or pose, an information matrix not symmetric to 1e-9 relative (|O_ij - O_ji| >
 * 1e-9 max(|O_ij|, |O_ji|, 1e-300)), bad options (algorithm, solver, max_iterations < 0, max_trials < 1, non-finite values).
 * Then DVO_AMD_ERR_NO_DEVICE without a GPU and DVO_AMD_ERR_INVALID_ARGUMENT for a NULL ctx or a context with queued pairs.
 */
#define DVO_AMD_GRAPH_LEVENBERG 0
#define DVO_AMD_GRAPH_DOGLEG 1
#define DVO_AMD_GRAPH_MAX_FREE_VERTICES 1024
#define DVO_AMD_GRAPH_MAX_FREE_VERTICES_SPARSE 65536
/* options.solver */
#define DVO_AMD_GRAPH_SOLVER_DENSE 0
#define DVO_AMD_GRAPH_SOLVER_SPARSE 1
/* termination */
#define DVO_AMD_GRAPH_ITERATIONS_EXHAUSTED 0
#define DVO_AMD_GRAPH_TERMINATE 1
#define DVO_AMD_GRAPH_FAIL 2

typedef struct {
  int from, to;              /* vertex indices: edge vertex 0 and vertex 1 */
  double measurement[16];    /* Z, column-major */
  double information[36];    /* Omega, column-major, symmetric */
} dvo_amd_graph_edge;

typedef struct {
  int algorithm;             /* DVO_AMD_GRAPH_LEVENBERG / _DOGLEG */
  int max_iterations;
  int max_trials;            /* attempts per iteration: 10 (Levenberg), 100 (dogleg) */
  int solver;                /* DVO_AMD_GRAPH_SOLVER_DENSE (0, default) / _SPARSE */
  double robust_delta;       /* Cauchy kernel delta on every edge; <= 0: no kernel */
  double initial_lambda;     /* Levenberg: <= 0 = 1e-5 max diag(H); dogleg: 1e-7 */
  double initial_delta;      /* dogleg trust region: 1e4 (unused by Levenberg) */
} dvo_amd_graph_options;

typedef struct {
  double objective;          /* F after the iteration */
  double step_norm;          /* |x| of the kept step, 0 if none */
  double lambda, delta;      /* after the iteration (delta: 0 for Levenberg) */
  int trials;
  int accepted;
} dvo_amd_graph_iteration;

typedef struct {
  int iterations;            /* iterations done */
  int termination;           /* DVO_AMD_GRAPH_ITERATIONS_EXHAUSTED / _TERMINATE / _FAIL */
  int n_free;                /* m: free active vertices */
  int cholesky_failures;     /* factorizations that met a pivot <= 0 */
  double initial_objective, final_objective, lambda, delta;
} dvo_amd_graph_stats;

/* the reference's values above for the algorithm: Levenberg max_iterations 50, max_trials 10, initial_lambda 0 (= tau max
 * diag); dogleg max_iterations 100, max_trials 100, initial_lambda 1e-7, initial_delta 1e4; robust_delta 5 for both */
void dvo_amd_default_graph_options(int algorithm, dvo_amd_graph_options *opt);
/* poses: n_vertices x 16 doubles, optimized in place.  edge_chi2 / edge_weight (n_edges each), iterations (iteration_capacity
 * records; later iterations are counted in stats but not recorded) and stats may be NULL. */
int dvo_amd_optimize_graph(dvo_amd_context *ctx, int n_vertices, double *poses, const int *fixed, int n_edges,
                           const dvo_amd_graph_edge *edges, const dvo_amd_graph_options *opt, double *edge_chi2,
                           double *edge_weight, int iteration_capacity, dvo_amd_graph_iteration *iterations,
                           dvo_amd_graph_stats *stats);

/*
 * Many small, independent pose graphs in one call: the local maps of a sequence (LocalMap::optimize, local_map.cpp:197-213: a
 * fixed keyframe, one vertex per frame, an odometry and a keyframe edge per frame, Levenberg) or the frames between two fixed
 * keyframes (KeyframeGraph::optimizeInterKeyframePoses, keyframe_graph.cpp:294-332).  One workgroup optimizes one graph and the
 * whole optimization of every graph runs in one kernel launch.
 * Per graph the semantics are those pinned above for dvo_amd_optimize_graph -- increment, edge error, Jacobians, Cauchy kernel,
 * normal equations, the Levenberg and the dogleg driver with their failure rules, fixed and inactive vertices returned bit for
 * bit, termination codes, cholesky_failures -- with one set of options for the whole batch.  What differs:
 *  - opt->solver must be DVO_AMD_GRAPH_SOLVER_DENSE (DVO_AMD_ERR_INVALID_ARGUMENT otherwise).
 *  - The order of the floating-point sums inside a graph is this entry's own, and fixed.  H and b: contributors in edge order
 *    (the same bits as the dense path's).  Cholesky: right-looking over the packed lower triangle, one vertex (6 columns) at a
 *    time -- the 6 x 6 diagonal block column by column, then every row below against it (columns 0 to 5), then every trailing
 *    entry minus its 6 products in column order.  Substitution: forward by vertex (the block's 6 unknowns in order, then every
 *    later row minus its 6 products in order), backward its mirror image.  F and the dot products: 256 strided partial sums,
 *    an xor butterfly (32, 16, 8, 4, 2, 1) over each group of 64 and ((s0 + s1) + s2) + s3 over the four groups.  H v: per
 *    row 64 strided partial sums and the same butterfly.  Levenberg's (2 rho - 1)^3 is t * t * t.  Results agree with
 *    dvo_amd_optimize_graph(DVO_AMD_GRAPH_SOLVER_DENSE) on the same graph to rounding, not bit for bit -- the relationship the
 *    sparse solver has to the dense one.
 *  - A graph's result (poses, edge_chi2, edge_weight, stats) is a function of that graph and the options alone: bit-identical
 *    whatever else is in the batch, at whatever index it stands, for any n_graphs, between runs and between contexts on one
 *    device.  No floating-point atomics; workgroups do not communicate.
 *  - Per-iteration records are not returned, only stats.
 *  - Capacity: a graph with more than DVO_AMD_GRAPH_BATCH_MAX_FREE_VERTICES free active vertices makes the whole call return
 *    DVO_AMD_ERR_CAPACITY with every pose of every item untouched; this is checked on the host, after the argument checks and
 *    before the device is looked for.  Vertices (fixed ones) and edges per graph are not limited.
 *  - Argument checks are those of dvo_amd_optimize_graph, in its order: the options first, then item by item in index order.
 *    A bad item makes the whole call return DVO_AMD_ERR_INVALID_ARGUMENT, dvo_amd_last_error() names the item ("item 3: ..."),
 *    and nothing is touched.  Then the capacity check, DVO_AMD_ERR_NO_DEVICE without a GPU, DVO_AMD_ERR_INVALID_ARGUMENT for a
 *    NULL ctx or a context with queued pairs.  n_graphs == 0 is DVO_AMD_OK.  A graph with no free active vertex or no edge
 *    keeps its poses and reports zero iterations (its objective and edge outputs are still evaluated), as on the single path.
 *  - What happens inside a graph (a failing dogleg: DVO_AMD_GRAPH_FAIL; Levenberg's terminate) is reported in that item's
 *    stats and does not touch the other graphs: the call returns DVO_AMD_OK.
 * Buffers are the context's, grown to the largest call and kept.
 */
#define DVO_AMD_GRAPH_BATCH_MAX_FREE_VERTICES 32   /* per graph: 192 unknowns, the packed factor (145 KB) fits one workgroup's LDS */

typedef struct {
  int n_vertices;
  double *poses;                     /* n_vertices x 16, column-major, optimized in place */
  const int *fixed;                  /* may be NULL: all free */
  int n_edges;
  const dvo_amd_graph_edge *edges;
  double *edge_chi2, *edge_weight;   /* n_edges each, may be NULL */
  dvo_amd_graph_stats stats;         /* out */
} dvo_amd_graph_batch_item;

int dvo_amd_optimize_graphs_batch(dvo_amd_context *ctx, int n_graphs, dvo_amd_graph_batch_item *items,
                                  const dvo_amd_graph_options *opt);

/*
 * Marginal covariances of pose-graph vertices: blocks of Sigma = H^-1 (g2o::SparseOptimizer::computeMarginals' role).
 *  - The matrix.  H is exactly the first system dvo_amd_optimize_graph builds at the given poses: the linearisation, the
 *    Cauchy weights (opt->robust_delta), rho1 Omega, no second-order term, the free active vertices in increasing index, and no
 *    damping (lambda = 0).  Of opt only solver and robust_delta are read; the other fields are still validated as
 *    dvo_amd_optimize_graph validates them.
 *  - Coordinates.  Sigma is the covariance of the increment d = (tx, ty, tz, qx, qy, qz) of X <- X * inc(d): a perturbation on
 *    the right, in the vertex's own frame, the rotation in quaternion-vector units (half a rotation vector to first order;
 *    S Sigma S with S = diag(1, 1, 1, 2, 2, 2) is in rotation-vector units, radians).
 *  - Requests.  Block k holds the rows of vertex block_a[k] and the columns of vertex block_b[k], column-major at
 *    blocks + 36 k; a == b is a vertex's marginal covariance.  Any pair of vertices may be asked for, in any order, repeated
 *    or not.  n_blocks == 0 is valid (stats only; block_a, block_b and blocks may then be NULL).
 *  - Fixed and inactive vertices.  A block that touches a fixed vertex is all zeros (known exactly); otherwise a block that
 *    touches an inactive vertex (no edge: unconstrained) is all NaN.  Both are counted in stats.
 *  - Failure.  A pivot <= 0 or NaN (for instance a component with no fixed vertex) is not an error of the call: it returns
 *    DVO_AMD_OK with factorized = 0, and every block that would have held numbers is NaN (the zeros of fixed vertices stay).
 *    No free active vertex: DVO_AMD_OK, factorized = 1, n_free = 0.
 *  - Symmetry.  A diagonal block is exactly symmetric and block (b, a) is the transpose of block (a, b) bit for bit: one
 *    triangle of Sigma is computed and every reader takes entry (max, min).
 *  - Determinism.  Fixed summation orders, no floating-point atomics: bit-identical between runs and between contexts on one
 *    device, and a block's bits do not depend on which other blocks were requested with it.
 *  - Solvers.  DVO_AMD_GRAPH_SOLVER_DENSE forms the whole lower triangle of Sigma on the device from the tiled Cholesky
 *    factor (a blocked selected inversion over 64 x 64 tiles, which for a full matrix is the full inverse) and reads the
 *    requested blocks from it.  DVO_AMD_GRAPH_SOLVER_SPARSE runs the selected inversion over the assembly tree of the
 *    multifrontal factor, root to leaves (per front Y = L21 L11^-1, Z21 = -Z22 Y, Z11 = L11^-T L11^-1 - Y^T Z21, Z22 gathered
 *    from the parent), at the cost of a small multiple of one factorization, and serves from it every pair whose two vertices
 *    meet in one front: every diagonal block and every pair joined by an edge.  Any other pair takes the slow path: the block
 *    column of the pair's lower free slot by 6 unit right-hand sides through the forward / backward substitution, once per
 *    distinct such vertex (stats->solved_columns), each solve as serial as any solve of the sparse path.  The two solvers
 *    agree to rounding, not bit for bit.
 *  - Limits and errors.  The argument checks of dvo_amd_optimize_graph in its order, then DVO_AMD_ERR_INVALID_ARGUMENT for
 *    n_blocks < 0, NULL block_a / block_b / blocks with n_blocks > 0 or a vertex index out of range; then the capacity rule of
 *    the chosen solver (1024 / 65536 free active vertices: DVO_AMD_ERR_CAPACITY); all of these before any device is looked
 *    for.  Then DVO_AMD_ERR_NO_DEVICE, DVO_AMD_ERR_INVALID_ARGUMENT for a NULL ctx or a context with queued pairs, and the
 *    sparse solver's DVO_AMD_ERR_OUT_OF_MEMORY prediction, which here counts the storage of the inverse (a second set of front
 *    matrices) as well.  poses is const; on any error nothing of the caller's is written except *stats (zeroed).
 */
typedef struct {
  int n_free;            /* m: free active vertices */
  int factorized;        /* 1: H was positive definite; 0: a pivot <= 0 or NaN was met, every block is NaN */
  int fixed_blocks;      /* requested blocks that touch a fixed vertex (returned as zeros) */
  int inactive_blocks;   /* requested blocks that touch an inactive vertex (returned as NaN) */
  int solved_columns;    /* sparse solver: distinct vertices whose block column had to be obtained by 6 solves */
  int reserved;
} dvo_amd_graph_marginal_stats;

int dvo_amd_graph_marginals(dvo_amd_context *ctx, int n_vertices, const double *poses, const int *fixed, int n_edges,
                            const dvo_amd_graph_edge *edges, const dvo_amd_graph_options *opt, int n_blocks, const int *block_a,
                            const int *block_b, double *blocks, dvo_amd_graph_marginal_stats *stats);

/* Host-side helpers (no GPU needed): the SE(3) exponential / logarithm with Sophus' tangent order (upsilon, omega) and the
 * pivoted LDL^T 6x6 solve the driver uses in place of Sophus::SE3d::exp/log and Eigen::LDLT (dense_tracking.cpp:238,259,347).
 * Exported so that bindings do not need Sophus to build a T_init or to compare poses. */
void dvo_amd_se3_exp(const double *xi, double *T);
void dvo_amd_se3_log(const double *T, double *xi);
void dvo_amd_solve6(const double *A, const double *b, double *x);


/* Test probes, diagnostics and micro-benchmarks (dvo_amd_debug_*, dvo_amd_bench_*, dvo_amd_kernel_timing) are exported by the
 * same library but declared in dvo_amd_debug.h: they are scaffolding of this repository's tests and bench, not part of the
 * boundary a caller of the reference would bind. */

#ifdef __cplusplus
}
#endif
#endif

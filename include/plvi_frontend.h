/* plvi_frontend.h — C-ABI of the MI355X-native PL-VI-ORBSLAM3 feature front end.
 *
 * Plain pointers and sizes only.  Each entry point replaces one reference
 * interface (cited per function); INTEGRATION.md gives the C++ shim bodies
 * a maintainer drops into the reference classes (ORBextractor,
 * Lineextractor, ORBmatcher, LineMatcher, ORBVocabulary), and
 * pl-vi-orbslam3_amd/plvi/ is the Python (ctypes) mirror.
 *
 * Status codes: 0 = ok, negative = error (PLVI_E_*).  ORBextractor's
 * "empty image -> -1" convention (src/ORBextractor.cc:1072-1073) is kept by
 * plvi_orb_extract returning PLVI_E_EMPTY (-1).
 *
 * Threading: handles are independent and may be used from
 * different host threads concurrently (each owns its device scratch and HIP
 * stream); one handle is not re-entrant, exactly like the reference
 * extractor whose operator() mutates mvImagePyramid.
 */
#ifndef PLVI_FRONTEND_H
#define PLVI_FRONTEND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  PLVI_OK = 0,
  PLVI_E_EMPTY = -1,    /* empty image (ORBextractor.cc:1072) */
  PLVI_E_BADARG = -2,   /* bad size / parameter / type */
  PLVI_E_CAPACITY = -3, /* caller's output capacity too small (count still written) */
  PLVI_E_HIP = -4,      /* HIP runtime failure */
  PLVI_E_OVERFLOW = -5, /* internal fixed-capacity table overflowed on device */
  PLVI_E_SIZE = -6,     /* descriptor row counts differ (LineMatcher.cpp:50-51) */
  PLVI_E_CAPTURE = -7,  /* stream capture of the multi-stream frame schedule on a HIP runtime < 7.2 */
};

/* OpenCV-semantics switches for the items no reference test can pin
 * (confidence "M"); 0 = the default guesses.  Set in
 * plvi_orb_params.compat / plvi_line_params.compat at create time; the CPU
 * oracle takes the same flags.
 *  GAUSS_ROUNDED   A.4: GaussianBlur CV_8U taps by plain rounding
 *                  ([18,34,49,55,49,34,18] for 7x7 sigma 2, ORBextractor.cc:1115;
 *                  [14,63,103,63,14] for 5x5 sigma 1, binary_descriptor_custom.cpp:359)
 *                  instead of the error-diffused [18,34,48,56,..] / [14,62,104,..]
 *  RESIZE_V_GENERIC A.1: cv::resize INTER_LINEAR 8U vertical pass by the generic
 *                  (b0*H0 + b1*H1 + (1<<21)) >> 22 instead of the 8U
 *                  specialisation ((b0*(H0>>4))>>16 + (b1*(H1>>4))>>16 + 2) >> 2
 *                  (ORBextractor.cc:1165)
 *  EXP_CV_TABLE    A.6: the f64 7-tap LSD Gaussian (lsd.cpp:455) built with
 *                  OpenCV's table + polynomial exp (EXPTAB_SCALE 6) instead of
 *                  glibc exp (which equals the correctly rounded exp there)
 *  GEMM_FMA        the pose product Rcw*P + tcw of the frustum tests (cv::gemm,
 *                  3x3 * 3x1 + 3x1 float) as OpenCV's AVX2-dispatched build
 *                  contracts it, fma(a2,b2, fma(a0,b0, a1*b1)), instead of the
 *                  baseline (a0*b0 + a1*b1) + a2*b2 (plvi_frustum_params.compat)
 *  SCALEADD_FMA    the accumulation normal + normali / cv::norm(normali) of
 *                  UpdateNormalAndDepth (cv::scaleAdd of a 3x1 float row, its
 *                  scalar tail) as OpenCV's AVX2-dispatched build contracts it,
 *                  fma(normali, alpha, normal), instead of the baseline
 *                  normali*alpha + normal (plvi_refresh_params.compat) */
enum {
  PLVI_COMPAT_GAUSS_ROUNDED = 1,
  PLVI_COMPAT_RESIZE_V_GENERIC = 2,
  PLVI_COMPAT_EXP_CV_TABLE = 4,
  PLVI_COMPAT_GEMM_FMA = 8,
  PLVI_COMPAT_SCALEADD_FMA = 16,
};

/* Per-frame device error flags of a batch (plvi_orb_errors / plvi_lines_errors). */
enum {
  PLVI_FERR_OCTREE = 1,   /* ORB: an octree level exceeded its node table (level dropped) */
  PLVI_FERR_LSD_TILE = 2, /* lines: reserved (the streaming LSD prep has no tile to overflow) */
  PLVI_FERR_LSD_RAW = 4,  /* lines: more LSD regions than the raw line table holds */
  PLVI_FERR_KEYLINES = 8, /* lines: keyline table overflow (frame emitted with 0 lines) */
};

/* cv::KeyPoint layout (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct plvi_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} plvi_keypoint;

/* cv::line_descriptor::KeyLine layout (descriptor_custom.hpp:107-146). */
typedef struct plvi_keyline {
  float angle;
  int32_t class_id;
  int32_t octave;
  float pt_x, pt_y;
  float response;
  float size;
  float startPointX, startPointY, endPointX, endPointY;
  float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
  float lineLength;
  int32_t numOfPixels;
} plvi_keyline;

/* ------------------------------------------------------------------ ORB
 * Replaces ORB_SLAM3::ORBextractor (include/ORBextractor.h:44-110,
 * src/ORBextractor.cc:408-1177). */
typedef struct plvi_orb_extractor plvi_orb_extractor;

typedef struct plvi_orb_params {
  int nfeatures;      /* ORBextractor(int nfeatures, ...) */
  float scale_factor; /* float scaleFactor (stored as double, .h:97) */
  int nlevels;
  int ini_th_fast;
  int min_th_fast;
  unsigned compat;    /* PLVI_COMPAT_* (0 = defaults) */
} plvi_orb_params;

/* Create an extractor for frames of width x height, batches of up to
 * max_batch frames, on HIP device `device`.  Replaces the constructor
 * (ORBextractor.cc:408-468).  Any size, up to 16 levels, any scale factor
 * > 1 (2.0 on even sizes takes cv::resize's INTER_AREA path, like the
 * reference), any thresholds, nfeatures >= 0.  PLVI_E_BADARG where the
 * reference itself cannot run -- a level without a 30-px cell (below 62 x 62)
 * or with 0 octree roots (more than twice as tall as wide between the
 * borders) -- and above 8 octree roots (a limit of this implementation). */
int plvi_orb_create(const plvi_orb_params* p, int width, int height, int max_batch, int device,
                    plvi_orb_extractor** out);
int plvi_orb_destroy(plvi_orb_extractor* h);

/* One frame from host memory, synchronous: ORBextractor::operator()
 * (ORBextractor.cc:1068-1150).  Keypoints are written in the reference's
 * slot order (mono slots ascending from 0, vLappingArea slots from the back);
 * descriptors are n x 32 bytes in the same row order.  *n = number of
 * keypoints, *mono_index = return value of operator() (monoIndex).
 * Returns PLVI_E_EMPTY for an empty image.  Like operator() it accepts any
 * frame size: a size other than the handle's re-plans the handle (pyramid,
 * cells, buffers) for the new size, which the batch entry points then use. */
int plvi_orb_extract(plvi_orb_extractor* h, const uint8_t* img, int width, int height, size_t stride,
                     int lap0, int lap1, plvi_keypoint* kps, uint8_t* desc, int cap, int* n, int* mono_index);

/* Batched, device-resident variant: n_frames frames at d_frames (device
 * pointer, frame f row r at d_frames + f*frame_stride + r*row_stride), all
 * of the handle's width x height.  Asynchronous on `stream` (hipStream_t,
 * NULL = the handle's own stream).  Results stay on the device: see
 * plvi_orb_outputs. */
int plvi_orb_extract_batch(plvi_orb_extractor* h, const uint8_t* d_frames, int n_frames, size_t frame_stride,
                           size_t row_stride, int lap0, int lap1, void* stream);

/* Device error flags of the batches run since the last call (PLVI_FERR_*),
 * read and cleared: frame_flags[f] for frame slot f (max_batch ints, may be
 * NULL), *any = OR over all slots (may be NULL).  Synchronises `stream`
 * (NULL = the handle's stream), on which the flags are read and reset.  A
 * frame with a flag set has truncated tables; the single-frame entry
 * points report the same condition as PLVI_E_OVERFLOW. */
int plvi_orb_errors(plvi_orb_extractor* h, int* frame_flags, int* any, void* stream);

/* Device pointers to the last batch's outputs: keypoints [max_batch][cap],
 * descriptors [max_batch][cap][32], counts [max_batch], mono [max_batch].
 * *cap = per-frame keypoint capacity (sum of per-level octree capacities). */
int plvi_orb_outputs(plvi_orb_extractor* h, plvi_keypoint** d_kps, uint8_t** d_desc, int** d_count, int** d_mono,
                     int* cap);

/* mvImagePyramid[level] of frame `frame` of the last call (lazy D2H copy).
 * dst must hold w*h bytes; pass dst=NULL to query the size.  Level 0 is read
 * from the last call's input frames when they were packed (see
 * plvi_orb_pyramid_device), so call this before they are overwritten. */
int plvi_orb_pyramid_level(plvi_orb_extractor* h, int frame, int level, uint8_t* dst, int* w, int* hgt);

/* Device view of mvImagePyramid (include/ORBextractor.h:84, read by
 * Frame::ComputeStereoMatches, src/Frame.cc:1235,1325,1344): level `level`
 * of frame f is the w x hgt u8 image (row stride w) at
 * *d_frame0 + f * *frame_stride, valid after the last extraction on the
 * handle's stream.  Level 0 is the input image itself (ORBextractor.cc:1165
 * copies it unchanged): when the last batch's rows were packed (row_stride ==
 * width) it is returned as a view of the caller's frames (the batch pointer and
 * its frame_stride; plvi_orb_extract's own staging copy for single frames),
 * valid while that buffer is unchanged; otherwise the handle holds a copy.
 * level = -1 only reports *nlevels.  Any out pointer may be NULL. */
int plvi_orb_pyramid_device(plvi_orb_extractor* h, int level, const uint8_t** d_frame0, size_t* frame_stride, int* w,
                            int* hgt, int* nlevels);

/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:62-82): nlevels floats each. */
int plvi_orb_scale_tables(plvi_orb_extractor* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);

/* Per-level feature quota (mnFeaturesPerLevel, ORBextractor.cc:433-444). */
int plvi_orb_level_quota(plvi_orb_extractor* h, int* quota);

/* Stage timing (HIP events on the launch stream) for bench.py's roofline:
 * enable=1 resets and starts recording, 0 stops.  profile_read synchronises
 * and returns per-stage milliseconds summed over the recorded runs (up to
 * 512): [0] level build (resize+blur+FAST score), [1] cell NMS, [2] SAT,
 * [3] octree, [4] node best, [5] orientation+rBRIEF, [6] output assembly. */
int plvi_orb_profile(plvi_orb_extractor* h, int enable);
int plvi_orb_profile_read(plvi_orb_extractor* h, float* stage_ms, int* runs);

/* Per-launch timing of the pyramid blur + FAST kernel (bench.py's roofline
 * kernel) and of the pyramid kernel: enable=1 resets and records an event pair around every launch on
 * its launch stream (up to 4096 launches); read synchronises and returns the
 * summed milliseconds and the launch count. */
int plvi_orb_kernel_timing(plvi_orb_extractor* h, int enable);
int plvi_orb_kernel_timing_read(plvi_orb_extractor* h, float* total_ms, int* launches);
/* The same for kind 0 = blur + FAST, 1 = orb_pyramid_kernel (roofline_pyramid). */
int plvi_orb_kernel_timing_read_kind(plvi_orb_extractor* h, int kind, float* total_ms, int* launches);
/* Diagnostic: cap every level's octree node capacity at `cap` (<= 0 restores
 * the planned capacities).  A level whose DistributeOctTree needs more nodes
 * flags its frame (plvi_orb_errors bit 1) and yields no keypoints; the test
 * hook for that path. */
int plvi_orb_debug_node_cap(plvi_orb_extractor* h, int cap);

/* ------------------------------------------------------------------ Lines
 * Replaces ORB_SLAM3::Lineextractor (include/LineExtractor.h:49-93,
 * src/LineExtractor.cc:39-117): LSDDetectorC pyramid + LSD
 * (src/LSD/lsd.cpp) + KeyLine assembly + top-k + LBD
 * (Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp). */
typedef struct plvi_line_extractor plvi_line_extractor;

typedef struct plvi_line_params {
  int nfeatures;   /* lsd_nfeatures (0 = keep all) */
  int refine;      /* lsd_refine: only 0 (LSD_REFINE_NONE, the config) is supported */
  float lsd_scale; /* lsd_scale (LSDOptions::scale, float) */
  int nlevels;     /* pyramid octaves (<= 2) */
  float scale;     /* pyramid scale factor (2.0) */
  int extractor;   /* 0 = LSD (EDLines, extractor==1, is out of scope) */
  unsigned compat; /* PLVI_COMPAT_* (0 = defaults) */
} plvi_line_params;

int plvi_lines_create(const plvi_line_params* p, int width, int height, int max_batch, int device,
                      plvi_line_extractor** out);
int plvi_lines_destroy(plvi_line_extractor* h);

/* One frame from host memory, synchronous: Lineextractor::operator()
 * (LineExtractor.cc:45-117).  keylines (KeyLine layout) in the reference's
 * order (post top-k sort when truncated), LBD descriptors n x 32, and the
 * normalised line equations n x 3 doubles (keylineFunction).  The reference
 * APPENDS to keylineFunction; callers append line_fns themselves. Any frame
 * size is accepted (re-plans the handle, as for plvi_orb_extract). */
int plvi_lines_extract(plvi_line_extractor* h, const uint8_t* img, int width, int height, size_t stride,
                       plvi_keyline* keylines, uint8_t* desc, double* line_fns, int cap, int* n);

/* Batched device-resident variant (same frame addressing as ORB). */
int plvi_lines_extract_batch(plvi_line_extractor* h, const uint8_t* d_frames, int n_frames, size_t frame_stride,
                             size_t row_stride, void* stream);
int plvi_lines_outputs(plvi_line_extractor* h, plvi_keyline** d_kl, uint8_t** d_desc, double** d_fn, int** d_count,
                       int* cap);
/* Per-frame device error flags (PLVI_FERR_*), read and cleared; as plvi_orb_errors. */
int plvi_lines_errors(plvi_line_extractor* h, int* frame_flags, int* any, void* stream);

/* mvImagePyramid_l[level] (gaussianPyrs, level >= 1; level 0 is the input). */
int plvi_lines_pyramid_level(plvi_line_extractor* h, int frame, int level, uint8_t* dst, int* w, int* hgt);

/* mvScaleFactor_l / mvInvScaleFactor_l / mvLevelSigma2_l / mvInvLevelSigma2_l (LineExtractor.cc:86-100). */
int plvi_lines_scale_tables(plvi_line_extractor* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);

/* Stage timing: [0] octave pyramid, [1] LSD prep (blur f64, resize, gradient),
 * [2] region growing + rect, [3] keyline assembly + top-k, [4] LBD. */
int plvi_lines_profile(plvi_line_extractor* h, int enable);
/* Diagnostic cycle accounting inside the region-growing kernel (s_memtime):
 * per (frame, octave) 24 uint64 = [total, block setup, rounds, rect, seeds,
 * blocks, rounds, rect points, commits, 4 round phases, seed scan, seed
 * starts, init, HW_ID, XCC_ID, start time, -]; NULL disables. */
int plvi_lines_debug_stats(plvi_line_extractor* h, unsigned long long* d_stats);
/* Diagnostic counters of the multi-wave (small-batch) region-growing kernel:
 * per (frame, octave) 16 int32 = [regions dispatched speculatively, dropped,
 * regrown after a failed validation, grown exactly by the walk (never
 * dispatched), trivial seeds, speculative regions committed, walk cycles,
 * walker growth cycles, walk entries, walks blocked on a growing head seed,
 * kernel cycles, speculative growth cycles, idle polls, 0, 0, 0]; NULL
 * disables.  Batches up to PLVI_GROW_MW frames (default 256) take that kernel. */
int plvi_lines_debug_mw_stats(plvi_line_extractor* h, int* d_stats);
/* Diagnostic: LSD planes of the last batch for one (frame, octave), copied to
 * host: angle in degrees (float, NOTDEF = -1024), modgrad (f64), cos/sin
 * pairs (float2, defined pixels only); any pointer may be NULL. */
int plvi_lines_debug_planes(plvi_line_extractor* h, int frame, int octave, float* deg, double* modgrad, float* cs,
                            int* sw, int* sh);
/* Diagnostic: LBD Sobel plane of the last batch for one (frame, octave),
 * interleaved int16 (dx, dy) per pixel, copied to host; dxdy may be NULL. */
int plvi_lines_debug_sobel(plvi_line_extractor* h, int frame, int octave, short* dxdy, int* w, int* hgt);
/* Diagnostic: region2rect's segments of the last batch for one (frame,
 * octave): one (x1, y1, x2, y2) float quadruple per region kept by region
 * growing, in region order, before any length filter (what
 * LineSegmentDetectorImpl::detect returns), copied to host.  *n = the count;
 * PLVI_E_CAPACITY when it exceeds cap (nothing copied); out may be NULL. */
int plvi_lines_debug_raw_lines(plvi_line_extractor* h, int frame, int octave, float* out, int cap, int* n);
int plvi_lines_profile_read(plvi_line_extractor* h, float* stage_ms, int* runs);
/* Per-launch timing of lsd_prep_kernel (bench.py's LSD-pass roofline), one
 * launch per octave: as plvi_orb_kernel_timing / _read. */
int plvi_lines_kernel_timing(plvi_line_extractor* h, int enable);
int plvi_lines_kernel_timing_read(plvi_line_extractor* h, float* total_ms, int* launches);
/* The same timing per kernel kind: 0 = lsd_prep_kernel, 1 = lbd_sobel0_kernel
 * (octave-0 5x5 blur + Sobel), 2 = lbd_sobel1_kernel (pyrDown + Sobel),
 * 3 = lsd_rect_lanes_kernel (region2rect; one launch for all octaves, or one
 * per stream where octave 0 grows beside the others), 4 = lbd_describe_kernel
 * (one launch per batch). */
int plvi_lines_kernel_timing_read_kind(plvi_line_extractor* h, int kind, float* total_ms, int* launches);

/* ------------------------------------------------------------------ Hamming
 * ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2350-2366) over a batch. */

/* cv::BFMatcher(NORM_HAMMING).knnMatch(q, t, k=2) semantics (scan train rows
 * ascending, strict-< insertion): for each query i, idx0/d0 = best train row
 * and distance, idx1/d1 = second.  Missing entries are -1 / INT32_MAX.
 * Batched over n_pairs independent (query,train) pairs; all pointers device.
 * q: [n_pairs][nq_cap][32], t: [n_pairs][nt_cap][32]; nq/nt: per-pair counts
 * (device int arrays).  Outputs [n_pairs][nq_cap].
 *
 * The count contract, common to every batched entry point of this header
 * that takes a device count array next to a table capacity (per pair or
 * per frame; keypoint, line, MapPoint and FeatureVector node counts alike):
 *   1. a count outside [0, cap] is read as clamped to that range;
 *   2. input rows at or past the clamped count are never read;
 *   3. output rows at or past it are never written (the per-pair result
 *      counts are always written).
 * Tables may therefore carry anything in their padding rows, and outputs may
 * be packed with stride cap without clearing them first. */
int plvi_hamming_knn2_batch(const uint8_t* d_q, const int* d_nq, int nq_cap, const uint8_t* d_t, const int* d_nt,
                            int nt_cap, int n_pairs, int* d_idx0, int* d_d0, int* d_idx1, int* d_d1, void* stream);

/* Host convenience wrapper (one pair, synchronous). */
int plvi_hamming_knn2(const uint8_t* q, int nq, const uint8_t* t, int nt, int* idx0, int* d0, int* idx1, int* d1);

/* LineMatcher::matchNNR (src/LineMatcher.cpp:41-61): matches_12[i] = train
 * index or -1; returns the number of matches (>=0) or an error code.
 * Requires nt >= 2 (the reference indexes matches_[idx][1]). */
int plvi_line_match_nnr(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr, int* matches_12);

/* LineMatcher::match(desc1, desc2, nnr, matches_12) (LineMatcher.cpp:92-111):
 * matchNNR both ways + mutual check. */
int plvi_line_match(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr, int* matches_12);

/* In/out variants with the reference's std::vector semantics: matches_12
 * holds the caller's n_prev existing entries on entry, and
 * matches_12.resize(n1, -1) (LineMatcher.cpp:44) keeps the first
 * min(n_prev, n1) of them (only accepted matches overwrite an entry) and
 * sets the rest to -1.  In plvi_line_match_inout a kept entry i2 >= 0 then
 * goes through the mutual check like a fresh one (LineMatcher.cpp:101-106);
 * a kept i2 >= n2 is out of range there (undefined in the reference) and
 * returns PLVI_E_BADARG. */
int plvi_line_match_nnr_inout(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr, int* matches_12,
                              int n_prev);
int plvi_line_match_inout(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr, int* matches_12,
                          int n_prev);

/* Batched LineMatcher::match on device descriptor tables: pair p matches
 * desc1[p] (n1[p] rows, stride cap1) against desc2[p] (n2[p] rows, stride
 * cap2).  d_scratch must hold 4*n_pairs*(cap1+cap2) ints.  Outputs
 * matches_12 [n_pairs][cap1] and per-pair match counts.  Pairs with fewer
 * than 2 rows on the train side produce no matches.  n1 / n2 follow the
 * count contract (plvi_hamming_knn2_batch). */
int plvi_line_match_batch(const uint8_t* d_desc1, const int* d_n1, int cap1, const uint8_t* d_desc2, const int* d_n2,
                          int cap2, int n_pairs, float nnr, int* d_scratch, int* d_matches_12, int* d_nmatch,
                          void* stream);

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2350-2366) or, with
 * line_matcher_quirk != 0, LineMatcher::DescriptorDistance
 * (src/LineMatcher.cpp:487-499: per-word count >> 25) of n row pairs
 * (d_a[i], d_b[i]), 32 bytes each; device pointers, asynchronous. */
int plvi_descriptor_distance_batch(const uint8_t* d_a, const uint8_t* d_b, int n, int line_matcher_quirk, int* d_out,
                                   void* stream);

/* ------------------------------------------------------------- SearchByBoW
 * ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>&)
 * (src/ORBmatcher.cc:269-471) with ComputeThreeMaxima (:2304-2345),
 * monocular branch (F.Nleft == -1, no second camera).  FeatureVectors are
 * CSR arrays sorted by node id: node[i], off[i]..off[i+1] into idx[] (the
 * keypoint indices of node i in FeatureVector order).  kf_live[k] = the KF
 * keypoint has a MapPoint that is not bad (evaluated by the caller).
 * Angles: pKF->mvKeysUn[k].angle and F.mvKeys[i].angle.  Output
 * match_kf[i] = KF keypoint index whose MapPoint goes to
 * vpMapPointMatches[i], or -1.  Returns nmatches (>= 0) or an error. */
int plvi_search_by_bow(float nnratio, int check_orientation, const uint8_t* kf_desc, const float* kf_angle,
                       const uint8_t* kf_live, int kf_n, const int* kf_node, const int* kf_off, int kf_nnodes,
                       const int* kf_idx, const uint8_t* f_desc, const float* f_angle, int f_n, const int* f_node,
                       const int* f_off, int f_nnodes, const int* f_idx, int* match_kf);

/* Batched device variant: pair p uses rows p*kf_cap / p*f_cap of the
 * keypoint arrays, p*node_cap (node ids) and p*(node_cap+1) (offsets) of
 * the CSR arrays, counts kf_nnodes[p], f_nnodes[p], f_n[p].  Outputs
 * match_kf [n_pairs][f_cap], nmatches [n_pairs].  f_n follows the count
 * contract (plvi_hamming_knn2_batch) against f_cap, both node counts against
 * node_cap.  Needs 4*f_cap + 8*node_cap <= 65536 bytes of LDS (an odd f_cap
 * is rounded up to even inside, which this bound already covers). */
int plvi_search_by_bow_batch(int n_pairs, float nnratio, int check_orientation, int kf_cap, int f_cap, int node_cap,
                             const uint8_t* d_kf_desc, const float* d_kf_angle, const uint8_t* d_kf_live,
                             const int* d_kf_node, const int* d_kf_off, const int* d_kf_nnodes, const int* d_kf_idx,
                             const uint8_t* d_f_desc, const float* d_f_angle, const int* d_f_n, const int* d_f_node,
                             const int* d_f_off, const int* d_f_nnodes, const int* d_f_idx, int* d_match_kf,
                             int* d_nmatches, void* stream);

/* The same with the two-camera branch of the reference (ORBmatcher.cc:321-420,
 * F.Nleft != -1: KannalaBrandt8 stereo rigs): keypoints [0, Nleft) are the
 * left camera's, [Nleft, N) the right one's (mvKeysRight); every KF keypoint
 * keeps a best / second pair per camera, and when the left best passes
 * TH_LOW the right best is also taken if it passes TH_LOW (its ratio test is
 * `|| true` in the reference).  Angles are per keypoint index as the
 * reference reads them (F: mvKeys for left indices, mvKeysRight[i - Nleft]
 * for right ones; KF: mvKeysUn without a second camera, else mvKeys /
 * mvKeysRight).  f_nleft = F.Nleft (-1 = one camera: plvi_search_by_bow);
 * d_f_nleft [n_pairs] (NULL = all -1). */
int plvi_search_by_bow_stereo(float nnratio, int check_orientation, const uint8_t* kf_desc, const float* kf_angle,
                              const uint8_t* kf_live, int kf_n, const int* kf_node, const int* kf_off, int kf_nnodes,
                              const int* kf_idx, const uint8_t* f_desc, const float* f_angle, int f_n,
                              const int* f_node, const int* f_off, int f_nnodes, const int* f_idx, int f_nleft,
                              int* match_kf);
int plvi_search_by_bow_stereo_batch(int n_pairs, float nnratio, int check_orientation, int kf_cap, int f_cap,
                                    int node_cap, const uint8_t* d_kf_desc, const float* d_kf_angle,
                                    const uint8_t* d_kf_live, const int* d_kf_node, const int* d_kf_off,
                                    const int* d_kf_nnodes, const int* d_kf_idx, const uint8_t* d_f_desc,
                                    const float* d_f_angle, const int* d_f_n, const int* d_f_node, const int* d_f_off,
                                    const int* d_f_nnodes, const int* d_f_idx, const int* d_f_nleft, int* d_match_kf,
                                    int* d_nmatches, void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>&
 * vpMatches12) (src/ORBmatcher.cc:823-963), the candidate search of
 * LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:823, once per
 * candidate and covisible: a batch of (current KF, KF_j) pairs), single-camera
 * branch (NLeft == -1 on both sides).  Per side s = 1, 2:
 *   desc   = pKFs->mDescriptors rows;  angle = pKFs->mvKeysUn[i].angle;
 *   live[i] = GetMapPointMatches()[i] != NULL && !isBad(), evaluated by the
 *             caller (replaces :862-866 and :882-888);
 *   node / off / idx = pKFs->mFeatVec as CSR arrays sorted by node id, as in
 *             plvi_search_by_bow.  A keypoint is in at most one node.
 * The device does the rest: the lower_bound merge walk; per shared node the
 * KF1 entries in list order, each against the node's KF2 entries that are
 * live and not yet in vbMatched2 (which this function, unlike
 * SearchForTriangulation, writes: :911); best / second with strict `<`
 * (first wins); bestDist1 < TH_LOW = 50, strict here (the KF-Frame function
 * has <=); (float)bestDist1 < nnratio * (float)bestDist2 (256 with a single
 * candidate); the 30-bin rotation histogram of angle1[idx1] - angle2[idx2]
 * and ComputeThreeMaxima.  Output matches12[idx1] = the KF2 keypoint index
 * whose MapPoint the reference stores in vpMatches12[idx1]
 * (vpMapPoints2[idx2] on the caller's side), or -1; nmatches is counted
 * after the rotation filter.
 *
 * Batched device variant, layout as plvi_search_by_bow_batch: pair p uses
 * rows p*cap1 / p*cap2 of the keypoint tables and of idx, p*node_cap (node
 * ids, ascending) and p*(node_cap+1) (offsets) of the CSR arrays.  Outputs
 * matches12 [n_pairs][cap1], nmatches [n_pairs]; rows [0, n1) of matches12
 * are fully written.  d_n1 / d_n2 follow the count contract
 * (plvi_hamming_knn2_batch) against cap1 / cap2 and the node counts against
 * node_cap; an offset outside [0, list length] is read as clamped and a list
 * entry outside [0, n) is ignored.
 * LDS: 4*cap1 (cap1 rounded up to even) + 8*node_cap + cap2 bytes, which with
 * the kernel's static data must fit the 160 KB of a CU; a larger table
 * returns PLVI_E_CAPACITY and nothing is launched.  Asynchronous on `stream`.
 * Replaces ORBmatcher.h:68 (SearchByBoW(KeyFrame*, KeyFrame*, ...)). */
int plvi_search_by_bow_kf_batch(int n_pairs, float nnratio, int check_orientation, int cap1, int cap2, int node_cap,
                                const uint8_t* d_desc1, const float* d_angle1, const uint8_t* d_live1,
                                const int* d_n1, const int* d_node1, const int* d_off1, const int* d_nnodes1,
                                const int* d_idx1, const uint8_t* d_desc2, const float* d_angle2,
                                const uint8_t* d_live2, const int* d_n2, const int* d_node2, const int* d_off2,
                                const int* d_nnodes2, const int* d_idx2, int* d_matches12, int* d_nmatches,
                                void* stream);

/* Single pair from host memory, synchronous: matches12 [n1]; returns
 * nmatches (>= 0) or an error.  n1 == 0 or n2 == 0: matches12 all -1,
 * returns 0, nothing is launched. */
int plvi_search_by_bow_kf(float nnratio, int check_orientation, const uint8_t* desc1, const float* angle1,
                          const uint8_t* live1, int n1, const int* node1, const int* off1, int nnodes1,
                          const int* idx1, const uint8_t* desc2, const float* angle2, const uint8_t* live2, int n2,
                          const int* node2, const int* off2, int nnodes2, const int* idx2, int* matches12);

/* ------------------------------------------------------------- matchGrid
 * LineMatcher::matchGrid(lines1, desc1, grid, desc2, directions2, w,
 * matches_12) (src/LineMatcher.cpp:191-272) with GridStructure::get
 * (src/gridStructure.cpp:64-75).  lines1: n1 x 4 ints (sp.x, sp.y, ep.x,
 * ep.y) = the line_2d grid coordinates (pair<int,int>, Frame.cc:1424-1427);
 * grid: CSR over grid_cols x grid_rows cells, cell (x, y) = x*grid_rows + y,
 * cell_off[ncell+1], cell_idx[] in std::list order; directions2: n2 x 2
 * doubles; window = GridWindow{width(w0, w1), height(h0, h1)}.
 * libstdcxx_range_hint selects the std::unordered_set range-insert rehash
 * rule that orders the candidates (1: GCC <= 10, the reference's Ubuntu
 * 20.04 toolchain; 0: GCC >= 11).  matches_12 is fully written (-1 = no
 * match).  Returns the match count or an error (n1, n2 <= 2048). */
int plvi_line_match_grid(const int* lines1, const uint8_t* desc1, int n1, int grid_cols, int grid_rows,
                         const int* cell_off, const int* cell_idx, const uint8_t* desc2, const double* directions2,
                         int n2, int win_w0, int win_w1, int win_h0, int win_h1, int libstdcxx_range_hint,
                         int* matches_12);

/* Batched device variant: pair p uses lines1 + p*cap1*4, desc1 + p*cap1*32,
 * cell_off + p*(ncell+1), cell_idx + p*idx_cap, desc2 + p*cap2*32,
 * directions2 + p*cap2*2, counts n1[p], n2[p] (count contract of
 * plvi_hamming_knn2_batch; cap1, cap2 <= 2048).  Outputs matches_12
 * [n_pairs][cap1], nmatches [n_pairs]; *d_err |= 1 when a candidate set
 * exceeds 1024 lines (d_err may be NULL: no report). */
int plvi_line_match_grid_batch(int n_pairs, const int* d_lines1, const uint8_t* d_desc1, const int* d_n1, int cap1,
                               int grid_cols, int grid_rows, const int* d_cell_off, const int* d_cell_idx,
                               int idx_cap, const uint8_t* d_desc2, const double* d_directions2, const int* d_n2,
                               int cap2, int win_w0, int win_w1, int win_h0, int win_h1, int libstdcxx_range_hint,
                               int* d_matches_12, int* d_nmatches, int* d_err, void* stream);

/* LineMatcher::SearchByProjection(Frame& CurrentFrame, Frame& LastFrame,
 * const GridStructure& grid, th, angth) (src/LineMatcher.cpp:274-372; its
 * Tracking.cc:3976/3984 call sites are commented out in the reference, kept
 * for drop-in completeness).  Per last-frame line (in order): flags bit0 =
 * mvpMapLines[i] && !mvbOutlier_Line[i], bit1 = that MapLine's
 * Observations() > 0; x3dc[6] = Rcw*x3Dw+tcw of its start and end point
 * (cv::Mat float, the caller's); octave = mvKeys_Line[i].octave; the
 * MapLine descriptor.  Current frame: mvKeysUn_Line angles, descriptors,
 * blocked = mvpMapLines[i2] && Observations() > 0 on entry (NULL = none),
 * grid_Line as in plvi_line_match_grid (cell (x, y) = x * rows + y, list
 * order).  Output match [cur] = last-frame line whose MapLine the call
 * stores in mvpMapLines[i2], -1 untouched; the count of assignments. */
typedef struct plvi_line_proj_params {
  float fx, fy, cx, cy;             /* Pinhole mvParameters */
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  double inv_w, inv_h;              /* Frame::inv_width / inv_height (grid cells per pixel) */
  float th, angth;
  int grid_cols, grid_rows;
  int range_hint;                   /* unordered_set range-insert rule: 1 = GCC <= 10, 0 = GCC >= 11 */
  int nlevels;                      /* <= 8 */
  float scale_l[8];                 /* CurrentFrame.mvScaleFactors_l */
} plvi_line_proj_params;

int plvi_line_search_projection_batch(int n_pairs, const plvi_line_proj_params* p, const float* d_cur_angle,
                                      const uint8_t* d_cur_desc, const uint8_t* d_cur_blocked, const int* d_cur_n,
                                      int cur_cap, const int* d_cell_off, const int* d_cell_idx, int idx_cap,
                                      const uint8_t* d_last_flags, const float* d_x3dc, const int* d_last_octave,
                                      const uint8_t* d_ml_desc, const int* d_last_n, int last_cap, int* d_match,
                                      int* d_nmatches, int* d_err, void* stream);
/* d_err (may be NULL): |= 1 when a candidate set overflows, |= 2 when a last-frame
 * octave is outside [0, nlevels) (that line is skipped).  Pair p uses rows
 * p*cur_cap / p*last_cap (x3dc: p*last_cap*6), cell_off + p*(ncell+1) and
 * cell_idx + p*idx_cap; cur_n / last_n follow the count contract
 * (plvi_hamming_knn2_batch), match rows [0, cur_n) are fully written. */
/* One pair from host memory, synchronous (n_cur <= 2048).  Returns the
 * count or an error (PLVI_E_CAPACITY when a candidate set exceeds 1024). */
int plvi_line_search_projection(const plvi_line_proj_params* p, const float* cur_angle, const uint8_t* cur_desc,
                                const uint8_t* cur_blocked, int n_cur, const int* cell_off, const int* cell_idx,
                                const uint8_t* last_flags, const float* x3dc, const int* last_octave,
                                const uint8_t* ml_desc, int n_last, int* match);

/* ------------------------------------------------------------- Vocabulary
 * DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h), the ORB vocabulary of
 * Frame::ComputeBoW (src/Frame.cc:1115-1122) and KeyFrame::ComputeBoW
 * (src/KeyFrame.cc:111).  Node ids and word ids follow the reference's
 * loader (node i = i-th line after the header, word ids in leaf order). */
typedef struct plvi_vocabulary plvi_vocabulary;

/* loadFromTextFile (TemplatedVocabulary.h:1338-1424; System.cc:84).
 * The reference's loop also builds a node from the empty line after the
 * file's final newline; its parent, leaf flag and descriptor are never
 * assigned (the istream sentry fails), i.e. undefined behaviour.
 * emulate_tail = 0 (recommended) skips it; != 0 models one outcome: a
 * weight-0, zero-descriptor, non-word child of the root. */
int plvi_vocab_load_text(const char* path, int emulate_tail, int device, plvi_vocabulary** out);

/* Build from a node table (row i = node i+1 in file order; parent[i] < i+1):
 * the structure loadFromTextFile would produce from the same lines. */
int plvi_vocab_create(int k, int L, int scoring, int weighting, int n_nodes, const int* parent,
                      const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device,
                      plvi_vocabulary** out);
int plvi_vocab_destroy(plvi_vocabulary* h);

/* info[6] = k, L, scoring, weighting, node count (incl. root), word count. */
int plvi_vocab_info(plvi_vocabulary* h, int* info);

/* transform(features, BowVector&, FeatureVector&, levelsup)
 * (TemplatedVocabulary.h:1126-1194) for one frame from host memory:
 * BowVector (std::map<WordId, WordValue>) as bow_word/bow_value in map order,
 * FeatureVector (std::map<NodeId, vector<unsigned>>) as CSR fv_node[i],
 * fv_idx[fv_off[i] .. fv_off[i+1]) in map order.  Arrays hold n entries
 * (fv_off n + 1). */
int plvi_vocab_transform(plvi_vocabulary* h, const uint8_t* desc, int n, int levelsup, unsigned* bow_word,
                         double* bow_value, int* bow_n, unsigned* fv_node, int* fv_off, unsigned* fv_idx,
                         int* fv_n);

/* Per-descriptor descent (transform(feature, word_id, weight, &nid, levelsup),
 * :1217-1259): word id and the node at level L - levelsup. */
int plvi_vocab_transform_features(plvi_vocabulary* h, const uint8_t* desc, int n, int levelsup, unsigned* word,
                                  unsigned* nid);

/* Batched device variant over n_frames descriptor tables [n_frames][cap][32]
 * with counts d_count (e.g. plvi_orb_outputs): outputs [n_frames][cap]
 * (fv_off [n_frames][cap+1]) and per-frame counts.  d_feat_word/d_feat_nid
 * (nullable) receive the per-descriptor descent.  d_count follows the count
 * contract (plvi_hamming_knn2_batch) with one addition: a count above cap is
 * not clamped silently, it also sets bit 0 of the handle's internal error
 * word (the synchronous wrappers then return PLVI_E_OVERFLOW).  Asynchronous. */
int plvi_vocab_transform_batch(plvi_vocabulary* h, const uint8_t* d_desc, const int* d_count, int cap, int n_frames,
                               int levelsup, unsigned* d_bow_word, double* d_bow_value, int* d_bow_n,
                               unsigned* d_fv_node, int* d_fv_off, unsigned* d_fv_idx, int* d_fv_n,
                               unsigned* d_feat_word, unsigned* d_feat_nid, void* stream);

/* ----------------------------------------------------------- Undistortion
 * Frame::UndistortKeyPoints (src/Frame.cc:1124-1157), UndistortKeyLines
 * (:1159-1197) and ComputeImageBounds (:1199-1226) = cv::undistortPoints
 * (OpenCV 4.2, 5 iterations, R = I, P = K).  mDistCoef[0] == 0 copies the
 * points unchanged, as the reference does. */
typedef struct plvi_camera {
  float fx, fy, cx, cy; /* mK */
  float dist[5];        /* mDistCoef: k1, k2, p1, p2[, k3] */
  int ndist;            /* 4 or 5 */
} plvi_camera;

/* n points (x, y float pairs, device), asynchronous. */
int plvi_undistort_points(const plvi_camera* cam, const float* d_xy, int n, float* d_out, void* stream);
/* mvKeysUn of keypoint tables [n_frames][cap] (counts d_count): each
 * keypoint copied with its pt undistorted. */
int plvi_undistort_keypoints_batch(const plvi_camera* cam, const plvi_keypoint* d_kps, const int* d_count, int cap,
                                   int n_frames, plvi_keypoint* d_out, void* stream);
/* Undistorted keyline endpoints [n_frames][cap][4] = startX, startY, endX, endY. */
int plvi_undistort_keylines_batch(const plvi_camera* cam, const plvi_keyline* d_kl, const int* d_count, int cap,
                                  int n_frames, float* d_endpoints, void* stream);
/* mnMinX, mnMaxX, mnMinY, mnMaxY (synchronous). */
int plvi_image_bounds(const plvi_camera* cam, int cols, int rows, float* bounds);

/* ------------------------------------------------------ SearchByProjection
 * The steady-state frame-to-frame ORB matcher of Tracking::TrackWithMotionModel
 * (src/Tracking.cc:3957): Frame::AssignFeaturesToGrid (src/Frame.cc:644-675),
 * Frame::GetFeaturesInArea (:1006-1075) and
 * ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)
 * (src/ORBmatcher.cc:1962-2178, single camera: Nleft == -1). */

/* Frame grid geometry: mnMinX, mnMinY, mfGridElementWidthInv/HeightInv
 * (Frame.cc:156-157); the grid is FRAME_GRID_COLS x ROWS = 64 x 48. */
typedef struct plvi_grid_params {
  float min_x, min_y, inv_w, inv_h;
} plvi_grid_params;

/* AssignFeaturesToGrid of n_frames keypoint tables [n_frames][cap]
 * (mvKeysUn; counts d_count) as CSR: cell (ix, iy) = ix*48 + iy lists its
 * keypoints at d_cell_idx[f*cap + d_cell_off[f*3073 + cell] ...] in index
 * order (= mGrid[ix][iy]).  cap <= 8192.  d_count follows the count contract
 * (plvi_hamming_knn2_batch); d_cell_off is written whole for every frame,
 * d_cell_idx up to the frame's in-grid count.  Asynchronous. */
int plvi_assign_grid_batch(const plvi_keypoint* d_kps, const int* d_count, int cap, int n_frames,
                           const plvi_grid_params* gp, int* d_cell_off, int* d_cell_idx, void* stream);

typedef struct plvi_proj_params {
  float fx, fy, cx, cy;            /* Pinhole mvParameters (CameraModels/Pinhole.cpp:30-33) */
  float mbf;                       /* CurrentFrame.mbf (mvuRight check, :2041-2047) */
  float th;                        /* window radius at octave 0 (radius = th * mvScaleFactors[octave]) */
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  float inv_w, inv_h;              /* mfGridElementWidthInv / HeightInv */
  int forward, backward;           /* bForward / bBackward (:1982-1983; both 0 for bMono) */
  int check_orientation;           /* mbCheckOrientation */
  int nlevels;
  float scale_factors[16];         /* CurrentFrame.mvScaleFactors */
} plvi_proj_params;

/* Batched SearchByProjection over n_pairs (CurrentFrame, LastFrame) pairs.
 * Current frame p: keypoints/descriptors [p][cur_cap] (mvKeysUn, counts
 * d_cur_n), grid CSR from plvi_assign_grid_batch, blocked[i2] =
 * mvpMapPoints[i2] && Observations() > 0 on entry (NULL = none), mvuRight
 * (NULL = none).  Last frame p: [p][last_cap] x3Dc = Rcw*x3Dw + tcw of the
 * point's MapPoint (3 floats), octave (mvKeys[i].octave), angle
 * (mvKeysUn[i].angle), MapPoint descriptor (32 B), flags bit0 = has a
 * MapPoint and is not an outlier, bit1 = that MapPoint's Observations() > 0.
 * Output match [p][cur_cap]: LastFrame index whose MapPoint
 * mvpMapPoints[i2] holds on return, -2 = set to NULL by the rotation filter,
 * -1 = untouched; nmatches [p] = the return value.  cur_cap, last_cap <= 65535
 * and the LDS footprint (~19 B per current + 8 B per last keypoint + 12 KB)
 * <= 160 KB.  d_cur_n / d_last_n follow the count contract
 * (plvi_hamming_knn2_batch). */
int plvi_search_by_projection_batch(int n_pairs, const plvi_proj_params* p, const plvi_keypoint* d_cur_kps,
                                    const uint8_t* d_cur_desc, const int* d_cur_n, int cur_cap,
                                    const uint8_t* d_cur_blocked, const float* d_cur_uright, const int* d_cell_off,
                                    const int* d_cell_idx, const float* d_x3dc, const int* d_last_octave,
                                    const float* d_last_angle, const uint8_t* d_mp_desc, const uint8_t* d_last_flags,
                                    const int* d_last_n, int last_cap, int* d_match, int* d_nmatches, void* stream);

/* One pair from host memory, synchronous (grid built on the device).
 * Returns nmatches (>= 0) or an error. */
int plvi_search_by_projection(const plvi_proj_params* p, const plvi_keypoint* cur_kps, const uint8_t* cur_desc,
                              int n_cur, const uint8_t* cur_blocked, const float* cur_uright, const float* x3dc,
                              const int* last_octave, const float* last_angle, const uint8_t* mp_desc,
                              const uint8_t* last_flags, int n_last, int* match);

/* The same search with a two-camera CurrentFrame (CurrentFrame.Nleft != -1,
 * src/ORBmatcher.cc:1985-2153).  kb8 = KannalaBrandt8 k1..k4 of
 * CurrentFrame.mpCamera (fx, fy, cx, cy from p; NULL = Pinhole).  Left:
 * mvKeys [p][cap] (counts d_n), descriptor rows 0..Nleft-1, blocked, mGrid
 * (plvi_assign_grid_batch over the left keypoints); right: mvKeysRight
 * [p][cap_r], rows Nleft.., blocked of mvpMapPoints[Nleft + idx], mGridRight
 * (the grid kernel over the right keypoints).  LastFrame point i: x3Dc, x3Dr
 * = mTrl * x3Dc (the caller's cv::Mat products), octave (mvKeys[i] or
 * mvKeysRight[i - Nleft] of LastFrame), angle (mvKeysUn / mvKeys /
 * mvKeysRight as :2067-2069), descriptor, flags as above.  A point is
 * searched in the right image only when its left pass did not end early
 * (behind the camera, outside mnMin/MaxX/Y, empty window: :2000-2026).
 * Outputs match [p][cap] / match_r [p][cap_r] (-2 = NULL by the rotation
 * filter, which sees both images' matches in one histogram), nmatches [p].
 * A searched point whose octave is outside [0, nlevels) gets no candidate in
 * either image (the reference would index mvScaleFactors out of range).
 * p->mbf is unused.  d_n / d_n_r / d_last_n follow the count contract
 * (plvi_hamming_knn2_batch).  Asynchronous on `stream`. */
int plvi_search_by_projection_stereo_batch(int n_pairs, const plvi_proj_params* p, const float* kb8,
                                           const plvi_keypoint* d_kps, const uint8_t* d_desc, const int* d_n, int cap,
                                           const uint8_t* d_blocked, const int* d_cell_off, const int* d_cell_idx,
                                           const plvi_keypoint* d_kps_r, const uint8_t* d_desc_r, const int* d_n_r,
                                           int cap_r, const uint8_t* d_blocked_r, const int* d_cell_off_r,
                                           const int* d_cell_idx_r, const float* d_x3dc, const float* d_x3dr,
                                           const int* d_last_octave, const float* d_last_angle,
                                           const uint8_t* d_mp_desc, const uint8_t* d_last_flags, const int* d_last_n,
                                           int last_cap, int* d_match, int* d_match_r, int* d_nmatches, void* stream);

/* One pair from host memory, synchronous; the same contract as the batch
 * (an octave outside [0, nlevels): no candidate).  Returns nmatches or an
 * error. */
int plvi_search_by_projection_stereo(const plvi_proj_params* p, const float* kb8, const plvi_keypoint* kps,
                                     const uint8_t* desc, int n, const uint8_t* blocked, const plvi_keypoint* kps_r,
                                     const uint8_t* desc_r, int n_r, const uint8_t* blocked_r, const float* x3dc,
                                     const float* x3dr, const int* last_octave, const float* last_angle,
                                     const uint8_t* mp_desc, const uint8_t* last_flags, int n_last, int* match,
                                     int* match_r);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
 * const set<MapPoint*>& sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2180-2300):
 * the relocalization guided search of Tracking::Relocalization
 * (src/Tracking.cc:5857 th 10 / ORBdist 100, :5871 th 3 / ORBdist 64, with
 * ORBmatcher(0.9, true)), single camera.  The MapPoint reads stay with the
 * caller (they take the MapPoint mutexes): per KF MapPoint i, in
 * pKF->GetMapPointMatches() order,
 *   flags bit0 = pMP && !pMP->isBad() && !sAlreadyFound.count(pMP);
 *   x3dc [3]   = Rcw*x3Dw + tcw (cv::Mat float gemm);
 *   dist [3]   = { dist3D = cv::norm(x3Dw - Ow), GetMinDistanceInvariance(),
 *                  GetMaxDistanceInvariance() };
 *   level      = pMP->PredictScale(dist3D, &CurrentFrame);
 *   angle      = pKF->mvKeysUn[i].angle;  desc = pMP->GetDescriptor().
 * The device does the rest: Pinhole::project, the bounds and distance tests,
 * GetFeaturesInArea(u, v, th*mvScaleFactors[level], level-1, level+1), the
 * best candidate among keypoints whose mvpMapPoints[i2] is NULL (those
 * assigned earlier in the same call included), bestDist <= ORBdist, and the
 * rotation-histogram filter. */
typedef struct plvi_reloc_params {
  float fx, fy, cx, cy;             /* Pinhole mvParameters */
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  float inv_w, inv_h;               /* mfGridElementWidthInv / HeightInv */
  float th;                         /* window radius at level 0 */
  int orb_dist;                     /* ORBdist (< 256: at 256 an empty search would index mvpMapPoints[-1]) */
  int check_orientation;            /* mbCheckOrientation */
  int nlevels;                      /* CurrentFrame.mnScaleLevels (levels outside [0, nlevels) get no candidate) */
  float scale_factors[16];          /* CurrentFrame.mvScaleFactors */
} plvi_reloc_params;

/* Batched over n_pairs (CurrentFrame, KeyFrame) pairs.  Current frame p:
 * keypoints/descriptors [p][cur_cap] (mvKeysUn, counts d_cur_n), grid CSR from
 * plvi_assign_grid_batch, blocked[i2] = mvpMapPoints[i2] != NULL on entry
 * (NULL = none).  KeyFrame p: [p][kf_cap] flags, x3dc [3], dist [3], level,
 * angle, desc [32] as above (counts d_kf_n).  Output match [p][cur_cap]: KF
 * MapPoint index stored in mvpMapPoints[i2] by the call, -2 = set to NULL by
 * the rotation filter, -1 = untouched; nmatches [p] = the return value.
 * cur_cap, kf_cap <= 65535 and ~19 B per current + 8 B per KF point + 12 KB of
 * LDS <= 160 KB.  d_cur_n / d_kf_n follow the count contract
 * (plvi_hamming_knn2_batch).  Asynchronous on `stream`. */
int plvi_search_reloc_batch(int n_pairs, const plvi_reloc_params* p, const plvi_keypoint* d_cur_kps,
                            const uint8_t* d_cur_desc, const int* d_cur_n, int cur_cap, const uint8_t* d_cur_blocked,
                            const int* d_cell_off, const int* d_cell_idx, const uint8_t* d_kf_flags,
                            const float* d_x3dc, const float* d_dist, const int* d_level, const float* d_kf_angle,
                            const uint8_t* d_mp_desc, const int* d_kf_n, int kf_cap, int* d_match, int* d_nmatches,
                            void* stream);

/* One pair from host memory, synchronous (grid built on the device).
 * Returns nmatches (>= 0) or an error. */
int plvi_search_reloc(const plvi_reloc_params* p, const plvi_keypoint* cur_kps, const uint8_t* cur_desc, int n_cur,
                      const uint8_t* cur_blocked, const uint8_t* kf_flags, const float* x3dc, const float* dist,
                      const int* level, const float* kf_angle, const uint8_t* mp_desc, int n_kf, int* match);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints,
 * vpMatched, th, ratioHamming) (src/ORBmatcher.cc:473-586; LoopClosing.cc:954
 * th 5 / ratio 1.0, :1207 th 3 / ratio 1.5) and the overload with
 * vpPointsKFs / vpMatchedKF (:588-704; LoopClosing.cc:929 th 8 / ratio 1.5):
 * the Sim3-guided searches of loop closing and map merging.  The MapPoint
 * reads (they take the MapPoint mutexes) and every cv::Mat product stay with
 * the caller: with sRcw = Scw(0:3, 0:3), scw = sqrt(sRcw.row(0).dot(sRcw.row(0))),
 * Rcw = sRcw/scw, tcw = Scw(0:3, 3)/scw, Ow = -Rcw.t()*tcw (:483-487), per
 * candidate MapPoint i, in vpPoints order,
 *   flags bit0 = !pMP->isBad() && !spAlreadyFound.count(pMP) (:501; the set
 *                is built from vpMatched on entry);
 *   x3dc [3]   = Rcw*p3Dw + tcw (:508);
 *   dist [3]   = { cv::norm(p3Dw - Ow) as float (:529), GetMinDistanceInvariance(),
 *                  GetMaxDistanceInvariance() };
 *   dot        = PO.dot(Pn) with PO = p3Dw - Ow, Pn = pMP->GetNormal() (:537;
 *                cv::Mat::dot returns double, and the compare is in double);
 *   level      = pMP->PredictScale(dist, pKF);  desc = pMP->GetDescriptor().
 * The device does the rest, bit-exact with the reference build: z < 0.0
 * skips; the projection -- 0: pKF->mpCamera->project, Pinhole,
 * (fx*x)/z + cx (the :473 overload, no fused operation); 1: invz = 1/z,
 * u = fma(x*invz, fx, cx) (the :588 overload; the reference object fuses
 * both sums) --; KeyFrame::IsInImage (u >= min_x && u < max_x, likewise v);
 * dist < min || dist > max skips; dot < 0.5 * (double)dist skips; a level
 * outside [0, nlevels) gets no candidate; KeyFrame::GetFeaturesInArea(u, v,
 * th * mvScaleFactors[level]) (KeyFrame.cc:1200-1244, the Frame's cell
 * arithmetic without a level filter); candidates whose vpMatched[idx] is
 * non-NULL -- on entry or assigned earlier in this call -- or whose octave is
 * outside [level-1, level] are skipped; the first keypoint with the smallest
 * distance wins; accepted when (float)bestDist <= 50.0f * ratio_hamming.
 * The two overloads are not aliases: where x*invz*fx + cx rounds differently
 * from (fx*x)/z + cx the window, and with it the result, can differ. */
typedef struct plvi_sim3_proj_params {
  float fx, fy, cx, cy;             /* pKF->fx, fy, cx, cy (Pinhole mvParameters) */
  float min_x, max_x, min_y, max_y; /* pKF->mnMinX, mnMaxX, mnMinY, mnMaxY (ints in KeyFrame, compared as float) */
  float inv_w, inv_h;               /* pKF->mfGridElementWidthInv / HeightInv */
  int th;                           /* th (an int in the reference: radius = (float)th * mvScaleFactors[level]) */
  float ratio_hamming;              /* ratioHamming; 50 * ratio_hamming < 256 is required (PLVI_E_BADARG):
                                       beyond it a search without a candidate would index vpMatched[-1] */
  int projection;                   /* 0: the :473 overload, 1: the :588 overload */
  int nlevels;                      /* pKF->mnScaleLevels, in [1, 16] */
  float scale_factors[16];          /* pKF->mvScaleFactors */
} plvi_sim3_proj_params;

/* Batched over n_pairs (KeyFrame, point list) pairs.  KeyFrame p:
 * keypoints / descriptors [p][kp_cap] (mvKeysUn, mDescriptors, counts d_kp_n),
 * the grid CSR from plvi_assign_grid_batch (the KeyFrame copies the Frame's
 * 64 x 48 grid), matched[idx] = vpMatched[idx] != NULL on entry (d_matched
 * NULL = none).  Points p: [p][pt_cap] flags, x3dc [3], dist [3], dot
 * (double), level, desc [32] as above (counts d_pt_n).  Output match
 * [p][kp_cap]: the point index i this call stored in vpMatched[idx], or -1
 * (entry-matched rows stay -1); nmatches [p] = the return value.  The
 * vpMatchedKF of the second overload is vpPointsKFs[match[idx]], a lookup on
 * the caller's side.
 * kp_cap <= 65535; pt_cap is bounded by LDS only: 17*kp_cap + 4*pt_cap +
 * 12292 + 64 bytes, which with the kernel's static data must fit the 160 KB
 * of a CU (8000 points against 2000 keypoints take 77 KB); a larger table
 * returns PLVI_E_CAPACITY and nothing is launched -- no list is truncated.
 * d_kp_n / d_pt_n follow the count contract (plvi_hamming_knn2_batch).
 * Asynchronous on `stream`.  Replaces ORBmatcher.h:58 and :62. */
int plvi_search_sim3_projection_batch(int n_pairs, const plvi_sim3_proj_params* p, const plvi_keypoint* d_kps,
                                      const uint8_t* d_desc, const int* d_kp_n, int kp_cap, const uint8_t* d_matched,
                                      const int* d_cell_off, const int* d_cell_idx, const uint8_t* d_flags,
                                      const float* d_x3dc, const float* d_dist, const double* d_dot,
                                      const int* d_level, const uint8_t* d_mp_desc, const int* d_pt_n, int pt_cap,
                                      int* d_match, int* d_nmatches, void* stream);

/* One pair from host memory, synchronous (grid built on the device, so
 * n_kp <= 8192 as in plvi_assign_grid_batch).  match [n_kp]; returns
 * nmatches (>= 0) or an error. */
int plvi_search_sim3_projection(const plvi_sim3_proj_params* p, const plvi_keypoint* kps, const uint8_t* desc,
                                int n_kp, const uint8_t* matched, const uint8_t* flags, const float* x3dc,
                                const float* dist, const double* dot, const int* level, const uint8_t* mp_desc,
                                int n_pt, int* match);

/* ------------------------------------------------------------------ Fuse
 * ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th,
 * bRight = false) (src/ORBmatcher.cc:1399-1610; LocalMapping.cc:1383 / :1434
 * per neighbour and back, LoopClosing.cc:3515 / :3573) -- mode 0 -- and
 * ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint)
 * (:1612-1734; LoopClosing::SearchAndFuse) -- mode 1 --, as a pure search:
 * inside one call bestIdx / bestDist of a point depend only on the pose
 * product, the keyframe's immutable tables (mvKeysUn, mvuRight, mDescriptors,
 * the grid) and the point's own data; the map mutation (GetMapPoint, Replace,
 * AddObservation, AddMapPoint, vpReplacePoint) starts after the search and
 * stays with the caller, which replays it in list order.
 * Single-camera keyframe only: NLeft == -1, bRight == false, mvKeysUn.
 * The caller provides, per candidate MapPoint i in list order,
 *   flags bit0 = mode 0: pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF) on
 *                entry (:1435-1452); mode 1: !pMP->isBad() &&
 *                !spAlreadyFound.count(pMP) (:1640);
 *   x3dc [3]   = Rcw*p3Dw + tcw (:1456 / :1647; mode 1 with the Rcw, tcw of
 *                the decomposed Scw, :1621-1625);
 *   dist [3]   = { cv::norm(p3Dw - Ow) as float, GetMinDistanceInvariance(),
 *                  GetMaxDistanceInvariance() };
 *   dot        = PO.dot(Pn) (cv::Mat::dot returns double; compared in double);
 *   level      = pMP->PredictScale(dist3D, pKF);  desc = pMP->GetDescriptor().
 * The device does the rest, bit-exact with the reference build: z < 0.0f
 * skips; Pinhole::project, (fx*x)/z + cx, no fused operation; KeyFrame::
 * IsInImage (strict upper bounds); dist < min || dist > max skips; dot <
 * 0.5 * (double)dist skips; a level outside [0, nlevels) gets no candidate;
 * radius = th * mvScaleFactors[level] with th a float; KeyFrame::
 * GetFeaturesInArea(u, v, radius) (no level filter inside); the octave must
 * lie in [level-1, level]; mode 0 only, the reprojection gate (:1533-1557)
 * with ur = fma(-bf, invz, u): where mvuRight[idx] >= 0, e2 = fma(er, er,
 * fma(ex, ex, ey*ey)) and (double)(e2 * mvInvLevelSigma2[octave]) > 7.8
 * skips, otherwise e2 = fma(ex, ex, ey*ey) against 5.99 (the fused sites are
 * the reference object's, tests/test_ref_objects_fuse.py; a keypoint with a
 * negative octave, for which the reference would read mvInvLevelSigma2[-1],
 * is no candidate in mode 0); the first keypoint with the smallest distance
 * wins; accepted when bestDist <= TH_LOW = 50.  bestDist starts at 256 in
 * mode 0 and INT_MAX in mode 1, which differs only for a lone candidate at
 * distance 256 -- rejected either way, hence one output convention:
 *   fuse_idx[i]  = the accepted keypoint index (bestIdx), else -1;
 *   fuse_dist[i] = its distance, else -1;
 *   nfused       = the number of accepted rows = the return value when no
 *                  flag changes during the call. */
#define PLVI_FUSE_CHUNK 64 /* candidates per workgroup of the two Fuse kernels */

typedef struct plvi_fuse_params {
  float fx, fy, cx, cy;             /* pKF->fx, fy, cx, cy (Pinhole mvParameters) */
  float min_x, max_x, min_y, max_y; /* pKF->mnMinX, mnMaxX, mnMinY, mnMaxY (ints in KeyFrame, compared as float) */
  float inv_w, inv_h;               /* pKF->mfGridElementWidthInv / HeightInv */
  float th;                         /* th, a float here (SearchByProjection(pKF, Scw, ...) has an int) */
  float bf;                         /* pKF->mbf (mode 0) */
  int mode;                         /* 0: Fuse(pKF, vpMapPoints, th), 1: Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) */
  int nlevels;                      /* pKF->mnScaleLevels, in [1, 16] */
  float scale_factors[16];          /* pKF->mvScaleFactors */
  float inv_level_sigma2[16];       /* pKF->mvInvLevelSigma2 (mode 0) */
} plvi_fuse_params;

/* Batched over n_pairs (KeyFrame, point list) pairs, tables laid out as in
 * plvi_search_sim3_projection_batch.  KeyFrame p: keypoints / descriptors
 * [p][kp_cap] (counts d_kp_n), the grid CSR from plvi_assign_grid_batch,
 * d_uright [p][kp_cap] = pKF->mvuRight (NULL = monocular: every entry
 * negative; not read in mode 1).  Points p: [p][pt_cap] flags, x3dc [3],
 * dist [3], dot (double), level, desc [32] (counts d_pt_n).  Outputs
 * fuse_idx / fuse_dist [p][pt_cap], rows [0, pt_n) fully written; nfused [p]
 * is written by the call (the caller does not zero it).
 * The kernel runs one workgroup per PLVI_FUSE_CHUNK points of a pair (grid =
 * point chunks x pairs) and reads the keyframe side through L2, so neither
 * capacity is bounded by LDS: kp_cap <= 65535 (PLVI_E_BADARG beyond, as
 * elsewhere); a launch of more than 2^31 - 1 workgroups (chunks of pt_cap
 * times n_pairs) returns PLVI_E_CAPACITY and nothing is launched.  d_kp_n /
 * d_pt_n follow the count contract (plvi_hamming_knn2_batch), clamped to
 * [0, cap]; a grid entry outside [0, kp_n) is ignored.  Asynchronous on
 * `stream`.  Replaces ORBmatcher.h:85 and :88 (the two Fuse overloads). */
int plvi_fuse_points_batch(int n_pairs, const plvi_fuse_params* p, const plvi_keypoint* d_kps, const uint8_t* d_desc,
                           const int* d_kp_n, int kp_cap, const float* d_uright, const int* d_cell_off,
                           const int* d_cell_idx, const uint8_t* d_flags, const float* d_x3dc, const float* d_dist,
                           const double* d_dot, const int* d_level, const uint8_t* d_mp_desc, const int* d_pt_n,
                           int pt_cap, int* d_fuse_idx, int* d_fuse_dist, int* d_nfused, void* stream);

/* One pair from host memory, synchronous (grid built on the device, so
 * n_kp <= 8192 as in plvi_assign_grid_batch; PLVI_E_BADARG beyond).
 * fuse_idx / fuse_dist [n_pt]; returns nfused (>= 0) or an error.  n_pt == 0
 * returns 0; n_kp == 0 writes -1 everywhere and returns 0; neither launches. */
int plvi_fuse_points(const plvi_fuse_params* p, const plvi_keypoint* kps, const uint8_t* desc, int n_kp,
                     const float* uright, const uint8_t* flags, const float* x3dc, const float* dist,
                     const double* dot, const int* level, const uint8_t* mp_desc, int n_pt, int* fuse_idx,
                     int* fuse_dist);

/* LineMatcher::Fuse(KeyFrame* pKF, const vector<MapLine*>& vpMapLines, th)
 * (src/LineMatcher.cpp:373-485; LocalMapping.cc:1412 / :1452, LoopClosing.cc
 * :3555 / :3595), the same split.  The caller provides, per MapLine i,
 *   flags bit0 = pML && !pML->isBad() (:390);
 *   spc [3], epc [3] = Rcw*SP + tcw, Rcw*EP + tcw (:398, :403);
 *   dist [3]   = { cv::norm(0.5*(SP+EP) - Ow) as float, min, max invariance };
 *   dot        = OM.dot(pn) (double);  level = pML->PredictScale(dist,
 *                pKF->mfLogScaleFactor);  desc = pML->GetDescriptor().
 * The device: either z < 0.0f skips; invz = 1.0f/z, u = fma(fx*X, invz, cx)
 * (the reference object fuses the second product of each of the four sums);
 * u < mnMinX || u > mnMaxX skips, likewise v -- both ends inclusive, not
 * IsInImage --, endpoint 1 before endpoint 2; the distance and viewing-angle
 * tests as for points; a level outside [0, nlevels) gets no candidate;
 * r = th * pKF->mvScaleFactors[level] (the ORB scale factors, as the
 * reference indexes); KeyFrame::GetLinesInArea(u1, v1, u2, v2, r)
 * (KeyFrame.cc:1170-1198) with the header's default levels -1 / -1, i.e. no
 * level filter: a scan of every keyline in index order with, as
 * KeyFrame.cc.o computes them, dx = fma(0.5, (double)(u1 + u2), -pt.x), dy
 * likewise, (float)fma(dx, dx, dy*dy) > r*r (float) skips, and
 * (double)((v1 - v2)/(u1 - u2) - angle) > (double)r * 0.01 skips -- no
 * absolute value, and u1 == u2 gives +-inf or NaN (NaN passes): both are the
 * reference's behaviour and stay; the octave must lie in [level-1, level];
 * LineMatcher::DescriptorDistance with its >> 25 quirk; the first minimum
 * wins (bestDist starts at INT_MAX); accepted when bestDist <= 50.  Outputs
 * as for points, fuse_idx = the keyline index. */
typedef struct plvi_fuse_line_params {
  float fx, fy, cx, cy;             /* pKF->fx, fy, cx, cy */
  float min_x, max_x, min_y, max_y; /* pKF->mnMinX, mnMaxX, mnMinY, mnMaxY */
  float th;
  int nlevels;                      /* pKF->mnScaleLevels, in [1, 16] */
  float scale_factors[16];          /* pKF->mvScaleFactors */
} plvi_fuse_line_params;

/* Batched: KeyFrame p = the 68-byte KeyLine rows and LBD descriptors
 * [p][kl_cap] (pKF->mvKeys_Line, mDescriptors_l; counts d_kl_n); MapLines p =
 * [p][ml_cap] tables as above (counts d_ml_n).  One workgroup per
 * PLVI_FUSE_CHUNK MapLines of a pair stages the keyframe's pt, angle, octave
 * and descriptors in LDS: 48 * kl_cap bytes, which with the kernel's static
 * data must fit the 160 KB of a CU (kl_cap <= 3413); a larger table, or a
 * launch of more than 2^31 - 1 workgroups, returns PLVI_E_CAPACITY and
 * nothing is launched.  Counts are clamped to [0, cap]; nfused [p] is written
 * by the call.  Asynchronous on `stream`.  Replaces LineMatcher.h:105. */
int plvi_fuse_lines_batch(int n_pairs, const plvi_fuse_line_params* p, const plvi_keyline* d_kl,
                          const uint8_t* d_kl_desc, const int* d_kl_n, int kl_cap, const uint8_t* d_flags,
                          const float* d_spc, const float* d_epc, const float* d_dist, const double* d_dot,
                          const int* d_level, const uint8_t* d_ml_desc, const int* d_ml_n, int ml_cap,
                          int* d_fuse_idx, int* d_fuse_dist, int* d_nfused, void* stream);

/* One pair from host memory, synchronous.  fuse_idx / fuse_dist [n_ml];
 * returns nfused (>= 0) or an error; n_ml == 0 or n_kl == 0 as above. */
int plvi_fuse_lines(const plvi_fuse_line_params* p, const plvi_keyline* kl, const uint8_t* kl_desc, int n_kl,
                    const uint8_t* flags, const float* spc, const float* epc, const float* dist, const double* dot,
                    const int* level, const uint8_t* ml_desc, int n_ml, int* fuse_idx, int* fuse_dist);

/* ------------------------------------------ ComputeDistinctiveDescriptors
 * MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:330-404) and
 * MapLine::ComputeDistinctiveDescriptors() (src/MapLine.cc:264-331, identical
 * from the point where vDescriptors is filled): the refresh of a map
 * feature's descriptor that follows every matcher call site (LocalMapping.cc
 * :553 / :600 / :621 / :1059 / :1312 / :1416-1429 / :1454-1463, LoopClosing.cc
 * :1389 / :1630, Tracking.cc, MapPoint::Replace / MapLine::Replace), as a
 * pure function of the feature's observed 32-byte rows in list order:
 *   Distances[i][j] = ORBmatcher::DescriptorDistance(row i, row j), the plain
 *     256-bit popcount, for points AND lines: MapLine.cc:305 calls ORBmatcher's
 *     function, not LineMatcher::DescriptorDistance with its >> 25 quirk (both
 *     MapPoint.cc.o and MapLine.cc.o carry a relocation to ORBmatcher::
 *     DescriptorDistance(cv::Mat const&, cv::Mat const&) inside the function
 *     and none to LineMatcher's; tests/test_ref_objects_distinctive.py).  The
 *     reference's float storage is exact (every value <= 256);
 *   median(i) = element floor((N-1)/2) of row i's N distances sorted
 *     ascending, the self-distance 0 included (`vDists[0.5*(N-1)]`);
 *   BestIdx = the first i with the smallest median (`median < BestMedian`,
 *     strict, from INT_MAX): the lexicographic minimum of (median, position).
 * N = 1 and N = 2 give row 0.  The result depends on the list order only
 * through that first-wins tie; the reference's order is the iteration order of
 * std::map<KeyFrame*, ...>, i.e. heap-address order, so the library takes the
 * order the caller gives.  Integers only: there is no float
 * on this path.
 *
 * One implementation serves points and lines: a pool of descriptor rows plus
 * a CSR observation list.
 *   d_pool [pool_rows][32]: descriptor rows (e.g. K keyframe tables
 *     [K][cap][32]: row = kf*cap + idx); byte offsets are computed in size_t.
 *   d_obs_off [n_feat+1], d_obs_row [d_obs_off[n_feat]]: feature i lists pool
 *     rows d_obs_row[off[i] .. off[i+1]).
 * List length: off[i+1] - off[i], read as clamped to [0, max_obs] (the count
 * contract of plvi_hamming_knn2_batch: entries past the clamp are never read,
 * a decreasing offset reads as an empty list).  An entry whose row is outside
 * [0, pool_rows) is ignored, as a grid entry outside [0, kp_n) is elsewhere --
 * which doubles as the way to pass leftIndex / rightIndex pairs with -1 for
 * the absent one; N is the number of entries that remain.
 * Outputs [n_feat], always written for every feature:
 *   best_pos    = the position of BestIdx inside the feature's list, ignored
 *                 entries counted (the pool row is obs_row[off[i] + best_pos]);
 *                 -1 when N == 0;
 *   best_median = BestMedian, -1 when N == 0;
 *   d_out_desc [n_feat][32] (may be NULL): row i = the chosen descriptor,
 *                 written only when N > 0 (the reference leaves mDescriptor
 *                 alone otherwise).
 * max_obs above PLVI_DISTINCTIVE_MAX_OBS returns PLVI_E_CAPACITY and nothing
 * is launched; no list is ever truncated below the max_obs the caller passed.
 * (The reference's `float Distances[N][N]` on a default 8 MiB thread stack
 * cannot exceed N ~ 1448, so no reference run has produced a longer list.)
 * Lists of up to 64 entries share waves (one lane per entry, several features
 * per wave when max_obs <= 32); a longer list has its rows staged in LDS once
 * per workgroup -- 36 * max_obs (rounded up to a multiple of 4) + 16656
 * bytes, 90 KB at the limit -- and its
 * N*N distances spread over several workgroups, so that it does not hold up
 * the short ones.
 * n_feat == 0 returns 0 without a launch; negative n_feat, pool_rows or
 * max_obs returns PLVI_E_BADARG; n_feat times the workgroups of a long list
 * beyond 2^31 - 1 returns PLVI_E_CAPACITY.  Asynchronous on `stream`, no host
 * read of device data, capturable in a graph like the other batch calls. */
#define PLVI_DISTINCTIVE_MAX_OBS 2048 /* longest observation list of plvi_distinctive_descriptors[_batch] */

int plvi_distinctive_descriptors_batch(int n_feat, const uint8_t* d_pool, int pool_rows, const int* d_obs_off,
                                       const int* d_obs_row, int max_obs, int* d_best_pos, int* d_best_median,
                                       uint8_t* d_out_desc, void* stream);

/* From host memory, synchronous.  obs_off must start at >= 0 and be
 * non-decreasing (PLVI_E_BADARG otherwise); max_obs is the longest list
 * (PLVI_E_CAPACITY above the limit).  best_pos / best_median [n_feat];
 * out_desc [n_feat][32] may be NULL, rows with best_pos = -1 are not written.
 * Returns the number of features with best_pos >= 0, or an error. */
int plvi_distinctive_descriptors(const uint8_t* pool, int pool_rows, const int* obs_off, const int* obs_row,
                                 int n_feat, int* best_pos, int* best_median, uint8_t* out_desc);

/* -------------------------------------------------------- KeyFrameDatabase
 * ORB_SLAM3::KeyFrameDatabase (src/KeyFrameDatabase.cc): add (:46-52), erase
 * (:54-73), clear (:75-79), clearMap (:81-105) and the two detectors the
 * reference calls, DetectRelocalizationCandidates (:790-902; Tracking.cc:5752)
 * and DetectNBestCandidates (:619-787; LoopClosing.cc:660 with 3 candidates).
 * DetectLoopCandidates, DetectCandidates and DetectBestCandidates have no
 * caller in the reference and are not provided.
 *
 * A keyframe lives in a caller-chosen slot in [0, slot_cap); slot numbers are
 * what every table and output below speaks (INTEGRATION.md maps them to
 * KeyFrame*).  Per slot the handle keeps, on the device: the BowVector
 * forward (words ascending as unsigned, values as double, word_cap entries),
 * a map id, a monotone add-sequence number, and two floats that stand for the
 * members KeyFrame::mPlaceRecognitionScore and KeyFrame::mRelocScore, which
 * persist from one query to the next.  There is no inverted file: the order
 * of the reference's lKFsSharingWords (semantics 3) follows from the forward
 * tables.
 *
 * Limits.  word_cap and q_cap <= PLVI_KFDB_MAX_WORDS: a query's words and
 * values are staged in LDS, 12 bytes a word (96 KB of a CU's 160 KB at the
 * limit); the reference's largest BowVector has 5 * nFeatures entries (the
 * initial keyframes' extractor, Tracking.cc:921).  slot_cap <= 2^24.  Both
 * return PLVI_E_CAPACITY beyond.  The handle's device memory is 12 * slot_cap
 * * word_cap bytes plus 28 * slot_cap per query of the largest batch seen.
 *
 * scoring is the vocabulary's DBoW2::ScoringType (info[2] of plvi_vocab_info):
 * only L1_NORM = 0 is supported, any other value returns PLVI_E_BADARG.
 * n_words is the vocabulary's word count; a word id at or above it sets bit 1
 * of the handle's error word (the reference would index mvInvertedFile out of
 * range).
 *
 * Calls on one handle must be ordered by the caller: issue them on one stream,
 * or order the streams with events.  The occupancy test of add is made on the
 * host at call time, in call order. */
#define PLVI_KFDB_MAX_WORDS 8192 /* longest BowVector of a slot or a query: 12 bytes of LDS per query word */
#define PLVI_KFDB_NEIGHBOURS 10  /* row length of d_covis: GetBestCovisibilityKeyFrames(10) */
typedef struct plvi_kf_database plvi_kf_database;

int plvi_kfdb_create(int n_words, int slot_cap, int word_cap, int scoring, int device, plvi_kf_database** out);
int plvi_kfdb_destroy(plvi_kf_database* h);

/* add (:46-52) of n keyframes straight from the [frame][cap] tables that
 * plvi_vocab_transform_batch writes.  entries (host) [n][3] = frame row,
 * slot, map id.  d_bow_n follows the count contract (plvi_hamming_knn2_batch)
 * with the addition of plvi_vocab_transform_batch: a count above word_cap is
 * clamped to it and sets bit 0 of the handle's error word (plvi_kfdb_errors).
 * A slot outside [0, slot_cap), a negative row, a slot that is occupied or
 * named twice returns PLVI_E_BADARG and nothing is added.  add zeroes both
 * score members of the slot.  For mPlaceRecognitionScore that is the
 * reference's own value (the KeyFrame constructors, KeyFrame.cc:37 / :55); it
 * never initialises mRelocScore, so a read before the first score (semantics
 * 4) is undefined there, and the handle models one outcome, 0, as emulate_tail
 * does for the vocabulary loader.  A keyframe with an empty BowVector occupies its slot
 * and shares a word with nothing.  After 2^32 - 1 adds since create or the last
 * clear the call returns PLVI_E_OVERFLOW.  Asynchronous on `stream`; the
 * entries are read before the call returns. */
int plvi_kfdb_add_batch(plvi_kf_database* h, int n, const int* entries, const unsigned* d_bow_word,
                        const double* d_bow_value, const int* d_bow_n, int cap, void* stream);

/* One keyframe from host memory, synchronous.  n above word_cap adds the first
 * word_cap words and returns PLVI_E_OVERFLOW. */
int plvi_kfdb_add(plvi_kf_database* h, int slot, int map_id, const unsigned* word, const double* value, int n);

/* erase (:54-73) of n slots (host array); an empty slot is left alone, as the
 * reference's erase of a keyframe that is in no list; a slot outside
 * [0, slot_cap) returns PLVI_E_BADARG.  A later add to the slot gets a later
 * sequence number.  clear_map (:81-105) erases every slot of one map id, clear
 * (:75-79) all of them.  Asynchronous on `stream`. */
int plvi_kfdb_erase(plvi_kf_database* h, int n, const int* slots, void* stream);
int plvi_kfdb_clear_map(plvi_kf_database* h, int map_id, void* stream);
int plvi_kfdb_clear(plvi_kf_database* h, void* stream);

/* Waits for `stream`, reads and clears the handle's error word into *flags
 * (may be NULL; bit 0 = a count above word_cap, bit 1 = a word id >= n_words)
 * and returns PLVI_E_OVERFLOW if it was not zero. */
int plvi_kfdb_errors(plvi_kf_database* h, int* flags, void* stream);

/* n_queries queries against the handle.  mode 0 =
 * DetectRelocalizationCandidates(F, pMap), mode 1 = DetectNBestCandidates(pKF,
 * vpLoopCand, vpMergeCand, n_best).
 * Inputs (device):
 *   d_q_word / d_q_value [q][q_cap], d_q_n [q]: the queries' BowVectors in the
 *     layout of plvi_vocab_transform_batch, counts under the count contract;
 *     words strictly ascending (a std::map's order);
 *   d_q_map [q]: F's / pKF's map id;
 *   d_conn_off [q+1], d_conn_slot (mode 1; both NULL = none): per query the
 *     slots of pKF->GetConnectedKeyFrames(); slots outside [0, slot_cap) are
 *     ignored.  Unused in mode 0;
 *   d_covis [slot_cap][PLVI_KFDB_NEIGHBOURS] (NULL = no keyframe has
 *     neighbours): row s = the slots of GetBestCovisibilityKeyFrames(10) of
 *     the keyframe in slot s, in that order; a negative entry ends the row;
 *     an entry naming an empty slot, or one outside [0, slot_cap), is skipped;
 *   d_map_bad [n_maps] (NULL = none): Map::IsBad() by map id; an id outside
 *     [0, n_maps) is not bad.
 * Stage outputs (device, each may be NULL):
 *   d_words [q][slot_cap]: the final mnRelocWords / mnPlaceRecognitionWords of
 *     the keyframes in lKFsSharingWords, -1 for every other slot;
 *   d_score [q][slot_cap] double: what mpVoc->score returned, before the float
 *     store, for the scored keyframes; other cells are not written;
 *   d_order [q][slot_cap], d_norder [q]: the slots in lKFsSharingWords order
 *     and their number; cells past the number are not written.
 * Final outputs (device):
 *   mode 0: d_cand [q][cand_cap], d_ncand [q]: vpRelocCandidates.  The full
 *     count is always written; rows at or past cand_cap are not;
 *   mode 1: d_loop / d_merge [q][n_best], d_nloop / d_nmerge [q].
 * Semantics:
 *   1. Sharing list (:631-660 / :798-813).  A keyframe sharing at least one
 *      word with the query enters lKFsSharingWords; in mode 1 the connected
 *      keyframes never enter it and never receive the query's stamp (:645).
 *      words = |common words|; minCommonWords = (int)(maxCommonWords * 0.8f)
 *      (:673 / :826), and only words > minCommonWords is scored (:684 / :837).
 *   2. Score (ScoringObject.cpp:23-68).  score += (fabs(vi - wi) - fabs(vi)) -
 *      fabs(wi) over the common words in ascending word id, in double, vi the
 *      query's value; then -score * 0.5 (the object negates and multiplies:
 *      tests/test_ref_objects_kfdb.py); then the float store into the score
 *      member (:688 / :841).  The sum is taken strictly in that order.
 *   3. Encounter order.  The reference walks the query's words ascending and
 *      each word's std::list in insertion order, and a keyframe enters the list
 *      at its first hit: lKFsSharingWords is ordered by (smallest word id shared
 *      with the query, add sequence).  Mode 0's output order and every tie
 *      below depend on it.
 *   4. Accumulation (:700-725 / :853-878).  Per scored keyframe in list order:
 *      accScore starts as its own float score; its neighbours are walked in
 *      table order, those without this query's stamp (sharing no word,
 *      connected in mode 1, or an empty slot) are skipped; accScore += the
 *      neighbour's score MEMBER, and pBestKF moves on a strict >.  A neighbour
 *      that shares a word but failed the threshold contributes its stale
 *      member: the value of the latest earlier query of the same mode that
 *      scored it, or 0 after add.
 *   5. Mode 0 selection (:880-899).  bestAccScore starts at 0 and moves on >;
 *      entries with accScore > 0.75f * bestAccScore are kept, those whose
 *      pBestKF is of another map than the query's dropped, then de-duplicated
 *      by pBestKF; output in list order, unsorted.
 *   6. Mode 1 selection (:729-759).  std::list::sort(compFirst) is a stable
 *      descending sort by accScore (ties keep list order); the sorted list is
 *      walked while either output has room: same map and room in loop -> loop;
 *      else another map, room in merge and a map that is not bad -> merge;
 *      every visited pBestKF is marked as added.  The caller must erase a
 *      keyframe before it goes bad, as KeyFrame::SetBadFlag does: the
 *      reference's `continue` without an increment (:742-743) would spin on
 *      a bad one, and the handle has no such flag.
 *   7. Batch = sequential.  The queries of one call behave as n_queries single
 *      calls in index order, the stale members of 4 included; after the call
 *      the members hold the last write.  Each query is a fresh stamp: the
 *      reference's stamp 0 (a frame or keyframe id 0 equals the initial
 *      mnRelocQuery / mnPlaceRecognitionQuery) and a repeated query id are
 *      outside the model.
 * q_cap above PLVI_KFDB_MAX_WORDS, n_queries above 65535 or n_queries *
 * slot_cap above 2^31 - 1 returns PLVI_E_CAPACITY; n_best <= 65535.
 * n_queries == 0 returns 0 without a launch.  A batch larger than any before
 * grows the handle's scratch (an allocation); otherwise the call is
 * asynchronous on `stream` with no host read of device data. */
int plvi_kfdb_query_batch(plvi_kf_database* h, int n_queries, const unsigned* d_q_word, const double* d_q_value,
                          const int* d_q_n, int q_cap, const int* d_q_map, int mode, int n_best,
                          const int* d_conn_off, const int* d_conn_slot, const int* d_covis, const uint8_t* d_map_bad,
                          int n_maps, int* d_words, double* d_score, int* d_order, int* d_norder, int* d_cand,
                          int cand_cap, int* d_ncand, int* d_loop, int* d_nloop, int* d_merge, int* d_nmerge,
                          void* stream);

/* One query from host memory, synchronous.  conn [n_conn], covis
 * [slot_cap][PLVI_KFDB_NEIGHBOURS] (may be NULL), map_bad [n_maps] (may be
 * NULL).  Mode 0: cand [cand_cap] receives at most cand_cap candidates and the
 * full count is returned.  Mode 1: loop / merge [n_best] and *n_loop /
 * *n_merge; returns their sum.  Negative = error. */
int plvi_kfdb_query(plvi_kf_database* h, const unsigned* q_word, const double* q_value, int q_n, int q_map, int mode,
                    int n_best, const int* conn, int n_conn, const int* covis, const uint8_t* map_bad, int n_maps,
                    int* cand, int cand_cap, int* loop, int* n_loop, int* merge, int* n_merge);

/* ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&
 * vpMapPoints, th, bFarPoints, thFarPoints) (src/ORBmatcher.cc:44-145,
 * F.Nleft == -1, RadiusByViewingCos :216-222): the local-map search of
 * Tracking::SearchLocalPoints (src/Tracking.cc:5119/5211). */
typedef struct plvi_local_params {
  float min_x, min_y, inv_w, inv_h; /* F.mnMinX, mnMinY, mfGridElementWidthInv / HeightInv */
  float th;                         /* th (the radius is scaled by th when th != 1) */
  float nnratio;                    /* ORBmatcher(nnratio): 0.8 in SearchLocalPoints */
  int nlevels;
  float scale_factors[16];          /* F.mvScaleFactors */
} plvi_local_params;

/* Batched over n_frames frames: frame f's keypoints (mvKeysUn) /
 * descriptors [f][cap] (counts d_n), grid CSR from plvi_assign_grid_batch,
 * blocked[idx] = mvpMapPoints[idx] && Observations() > 0 on entry (NULL =
 * none), mvuRight (NULL = none); its MapPoints [f][mp_cap] (counts d_mp_n,
 * vector order): flags bit0 = searched (mbTrackInView && not far &&
 * !isBad()), bit1 = Observations() > 0; proj [4] = mTrackProjX,
 * mTrackProjY, mTrackProjXR, mTrackViewCos; level = mnTrackScaleLevel;
 * GetDescriptor() (32 B).  Output match [f][cap] = the MapPoint index
 * stored in F.mvpMapPoints[idx] by the call, or -1; nmatches [f] = the
 * return value.  A MapPoint whose level is outside [0, nlevels) gets no
 * candidate.  cap <= 65535 and ~17 B per keypoint + 8 B per MapPoint +
 * 12 KB of LDS <= 160 KB.  d_n / d_mp_n follow the count contract
 * (plvi_hamming_knn2_batch). */
int plvi_search_local_batch(int n_frames, const plvi_local_params* p, const plvi_keypoint* d_kps, const uint8_t* d_desc,
                            const int* d_n, int cap, const uint8_t* d_blocked, const float* d_uright,
                            const int* d_cell_off, const int* d_cell_idx, const uint8_t* d_mp_flags,
                            const float* d_mp_proj, const int* d_mp_level, const uint8_t* d_mp_desc, const int* d_mp_n,
                            int mp_cap, int* d_match, int* d_nmatches, void* stream);

/* One frame from host memory, synchronous.  Returns nmatches or an error. */
int plvi_search_local(const plvi_local_params* p, const plvi_keypoint* kps, const uint8_t* desc, int n,
                      const uint8_t* blocked, const float* uright, const uint8_t* mp_flags, const float* mp_proj,
                      const int* mp_level, const uint8_t* mp_desc, int n_mp, int* match);

/* The same search on a two-camera Frame (F.Nleft != -1, src/ORBmatcher.cc:
 * 44-214; replaces the reference's loop for KannalaBrandt8 stereo rigs).
 * Left side: mvKeys [f][cap] (counts d_n) with their descriptors (rows
 * 0..Nleft-1 of mDescriptors), blocked (mvpMapPoints[idx] && Observations()
 * > 0), mvLeftToRightMatch (NULL = all -1) and the left grid (mGrid,
 * plvi_assign_grid_batch over the left keypoints); right side: mvKeysRight
 * [f][cap_r] (counts d_n_r), descriptors rows Nleft.., blocked of
 * mvpMapPoints[Nleft + idx], mvRightToLeftMatch and mGridRight (the grid
 * kernel over the right keypoints: right-relative indices).  MapPoints:
 * flags bit0 = searched left (mbTrackInView && not far && !isBad()), bit1 =
 * Observations() > 0, bit2 = searched right (mbTrackInViewR && not far &&
 * !isBad()); proj [4] = mTrackProjX, mTrackProjY, (unused), mTrackViewCos;
 * level = mnTrackScaleLevel; proj_r [4] = mTrackProjXR, mTrackProjYR,
 * (unused), mTrackViewCosR; level_r = mnTrackScaleLevelR (-1: no right
 * search).  Outputs match [f][cap] / match_r [f][cap_r] = the MapPoint
 * index stored in mvpMapPoints[idx] / mvpMapPoints[Nleft + idx] by the
 * call, or -1; nmatches [f] = the return value.  d_n / d_n_r / d_mp_n follow
 * the count contract (plvi_hamming_knn2_batch).  Asynchronous on `stream`. */
int plvi_search_local_stereo_batch(int n_frames, const plvi_local_params* p, const plvi_keypoint* d_kps,
                                   const uint8_t* d_desc, const int* d_n, int cap, const uint8_t* d_blocked,
                                   const int* d_l2r, const int* d_cell_off, const int* d_cell_idx,
                                   const plvi_keypoint* d_kps_r, const uint8_t* d_desc_r, const int* d_n_r, int cap_r,
                                   const uint8_t* d_blocked_r, const int* d_r2l, const int* d_cell_off_r,
                                   const int* d_cell_idx_r, const uint8_t* d_mp_flags, const float* d_mp_proj,
                                   const int* d_mp_level, const float* d_mp_proj_r, const int* d_mp_level_r,
                                   const uint8_t* d_mp_desc, const int* d_mp_n, int mp_cap, int* d_match,
                                   int* d_match_r, int* d_nmatches, void* stream);

/* One two-camera frame from host memory, synchronous.  Returns nmatches or
 * an error. */
int plvi_search_local_stereo(const plvi_local_params* p, const plvi_keypoint* kps, const uint8_t* desc, int n,
                             const uint8_t* blocked, const int* l2r, const plvi_keypoint* kps_r, const uint8_t* desc_r,
                             int n_r, const uint8_t* blocked_r, const int* r2l, const uint8_t* mp_flags,
                             const float* mp_proj, const int* mp_level, const float* mp_proj_r, const int* mp_level_r,
                             const uint8_t* mp_desc, int n_mp, int* match, int* match_r);

/* --------------------------------------------------------------- Frustum
 * The local-map visibility test of Tracking::SearchLocalPoints /
 * SearchLocalPointsAndLines (src/Tracking.cc:5074-5092, :5166-5184,
 * :5219-5234): Frame::isInFrustum (src/Frame.cc:758-835, Nleft == -1;
 * :836-846 + isInFrustumChecks :1751-1824, Nleft != -1), Frame::isInFrustum_l
 * (:849-933), MapPoint::PredictScale(dist, Frame*) (src/MapPoint.cc:531-546),
 * Get{Min,Max}DistanceInvariance (MapPoint.cc:502-512, MapLine.cc:384-394).
 * The outputs are the MapPoint fields the local search reads, in the layout
 * of plvi_search_local_batch / plvi_search_local_stereo_batch, so the two run
 * back to back on the device.
 *
 * One camera of a frame: the world->camera pose of the product Pc = R*P + t
 * and the centre O of the distance test.  Left / one-camera frames: R = mRcw,
 * t = mtcw, O = mOw, the camera mpCamera.  Right camera of a two-camera frame:
 * R = Rrl*mRcw, t = Rrl*mtcw + trl, O = mRwc*tlr + mOw (Frame.cc:1757-1761,
 * per frame, the caller's cv::Mat products), the camera mpCamera2. */
typedef struct plvi_frustum_camera {
  float R[9]; /* row-major */
  float t[3];
  float O[3];
  float fx, fy, cx, cy; /* Pinhole / KannalaBrandt8 mvParameters[0..3]; lines: Frame::fx, fy, cx, cy */
  float kb[4];          /* KannalaBrandt8 k1..k4 (mvParameters[4..7]) */
  int model;            /* 0 = Pinhole, 1 = KannalaBrandt8 */
} plvi_frustum_camera;

typedef struct plvi_frustum_params {
  plvi_frustum_camera cam[2];       /* cam[1] only with two_camera */
  int two_camera;                   /* F.Nleft != -1 */
  float mbf;                        /* Frame::mbf (mTrackProjXR of a one-camera frame) */
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  float view_cos_limit;             /* 0.5 in SearchLocalPoints */
  int far_points;                   /* mpLocalMapper->mbFarPoints */
  float far_th;                     /* mpLocalMapper->mThFarPoints */
  int nlevels;                      /* mnScaleLevels (1..16) */
  float log_scale_factor;           /* mfLogScaleFactor */
  float level_ratio[16];            /* filled by plvi_frustum_params_init */
  unsigned compat;                  /* PLVI_COMPAT_GEMM_FMA */
} plvi_frustum_params;

/* PredictScale as a table: level_ratio[n] = the least float ratio =
 * mfMaxDistance/dist with ceil(logf(ratio)/mfLogScaleFactor) >= n (host glibc
 * logf, as MapPoint.cc.o calls it); +inf when none.  Call once per
 * (nlevels, log_scale_factor) before uploading the params.  PLVI_E_BADARG for
 * nlevels outside 1..16 or a negative / NaN log_scale_factor. */
int plvi_frustum_params_init(plvi_frustum_params* p);

/* Output flags of plvi_frustum_points_batch. */
enum {
  PLVI_FRUSTUM_SEARCH = 1,    /* searched by SearchByProjection (left): in view, not far (== local bit0) */
  PLVI_FRUSTUM_OBS = 2,       /* Observations() > 0, copied from the input (== local bit1) */
  PLVI_FRUSTUM_SEARCH_R = 4,  /* two-camera: searched right (== local-stereo bit2) */
  PLVI_FRUSTUM_VISIBLE = 8,   /* isInFrustum returned true: IncreaseVisible, nToMatch */
  PLVI_FRUSTUM_TRACK = 16,    /* mbTrackInView after the call: mmProjectPoints[mnId] = (ProjX, ProjY) */
};

/* Per frame f (d_params[f] on the device), its local MapPoints [f][cap] in
 * mvpLocalMapPoints order (counts d_n): pos [3] = GetWorldPos(), normal [3] =
 * GetNormal(), dist [2] = {mfMinDistance, mfMaxDistance}, in_flags bit0 =
 * the loop reaches isInFrustum (mnLastFrameSeen != mnId && !isBad()), bit1 =
 * Observations() > 0.  Outputs, for evaluated MapPoints only (others keep the
 * buffers' contents, flags 0 apart from OBS): proj [4] = {mTrackProjX,
 * mTrackProjY, mTrackProjXR, mTrackViewCos}, level = mnTrackScaleLevel, depth
 * = mTrackDepth (in/out: a two-camera far test reads the entry value when the
 * left test fails); two-camera frames: proj[2] untouched, proj_r [4] =
 * {mTrackProjXR, mTrackProjYR, -, mTrackViewCosR}, level_r =
 * mnTrackScaleLevelR (-1 = not in view).  Fields the reference leaves stale
 * are left as they were.  nvisible [f] = nToMatch.  proj_r / level_r may be
 * NULL for one-camera batches, nvisible may be NULL.  Asynchronous. */
int plvi_frustum_points_batch(int n_frames, const plvi_frustum_params* d_params, const float* d_pos,
                              const float* d_normal, const float* d_dist, const uint8_t* d_in_flags, const int* d_n,
                              int cap, uint8_t* d_flags, float* d_proj, int* d_level, float* d_proj_r, int* d_level_r,
                              float* d_depth, int* d_nvisible, void* stream);

/* One frame from host memory, synchronous.  Returns nToMatch or an error. */
int plvi_frustum_points(const plvi_frustum_params* p, const float* pos, const float* normal, const float* dist,
                        const uint8_t* in_flags, int n, uint8_t* flags, float* proj, int* level, float* proj_r,
                        int* level_r, float* depth);

/* isInFrustum_l over frame f's local MapLines [f][cap] (mvpLocalMapLines
 * order, counts d_n): sep [6] = GetWorldPos() (double), normal [3] =
 * GetNormal(), dist [2] = {mfMinDistance, mfMaxDistance}, in_flags bit0 =
 * evaluated (mnLastFrameSeen != mnId && !isBad()), desc [32] =
 * GetDescriptor() (NULL: no gather).  Outputs: inview = mbTrackInView (0 for
 * lines not evaluated), proj [4] = {mTrackProjsX, mTrackProjsY, mTrackProjeX,
 * mTrackProjeY} (each pair written once its endpoint passes, as the
 * reference does), angle = mnTrackangle (in view only); the order-preserving
 * list mvpLocalMapLines_InFrustum as local indices compact [f][cap] (count
 * ncompact [f] = nToMatch) and their descriptors compact_desc [f][cap][32],
 * the desc1 of LineMatcher::match (plvi_line_match_batch).  Asynchronous. */
int plvi_frustum_lines_batch(int n_frames, const plvi_frustum_params* d_params, const double* d_sep,
                             const float* d_normal, const float* d_dist, const uint8_t* d_in_flags,
                             const uint8_t* d_desc, const int* d_n, int cap, uint8_t* d_inview, float* d_proj,
                             double* d_angle, int* d_compact, uint8_t* d_compact_desc, int* d_ncompact, void* stream);

/* One frame from host memory, synchronous.  Returns nToMatch or an error. */
int plvi_frustum_lines(const plvi_frustum_params* p, const double* sep, const float* normal, const float* dist,
                       const uint8_t* in_flags, const uint8_t* desc, int n, uint8_t* inview, float* proj,
                       double* angle, int* compact, uint8_t* compact_desc);

/* The orientation / position filter after LineMatcher::match in
 * SearchLocalPointsAndLines (src/Tracking.cc:5244-5292).  Frame f: matches_12
 * [f][cap] over its ncompact [f] in-frustum lines (in/out: rejected entries
 * set to -1, as the reference does), compact / proj / angle from
 * plvi_frustum_lines_batch, the frame's mvKeysUn_Line [f][kl_cap] (counts
 * d_nkl), blocked [f][kl_cap] = mvpMapLines[i2] && Observations() > 0 on
 * entry (NULL = none).  Output assign [f][kl_cap] = the local MapLine index
 * stored in mvpMapLines[i2] by the loop, or -1; nassigned [f] = their count.
 * The bounds for deltaWidth / deltaHeight come from d_params[f]. */
int plvi_local_lines_filter_batch(int n_frames, const plvi_frustum_params* d_params, int* d_matches_12,
                                  const int* d_ncompact, const int* d_compact, int cap, const float* d_proj,
                                  const double* d_angle, const plvi_keyline* d_kl, const int* d_nkl, int kl_cap,
                                  const uint8_t* d_blocked, int* d_assign, int* d_nassigned, void* stream);

/* -------------------------------------------------------------- Local map
 * Tracking::UpdateLocalMap() / UpdateLocalMapWithLines() (src/Tracking.cc:
 * 5304-5323; called once per tracked frame from TrackLocalMap :4153 /
 * TrackLocalMapWithLines :4268): UpdateLocalKeyFrames[WithLines] (:5399-5551
 * / :5553-5745) and UpdateLocalPoints[AndLines] (:5325-5352 / :5354-5397) for
 * every frame of a batch.  The local lists come out as keyframe slots and
 * pool ids, in the reference's order, together with the input tables of
 * plvi_frustum_points_batch / plvi_frustum_lines_batch (and the desc table of
 * plvi_search_local_batch), so the per-frame chain local map -> frustum ->
 * grid -> search stays on the device.  Integers only: every output equals the
 * reference's entry for entry.
 *
 * Keyframes live in the caller-chosen slots of the keyframe database
 * ([0, kf_cap)); MapPoints and MapLines live in two pools indexed by id.
 * All pointers of the four structs are device pointers for
 * plvi_local_map_batch and host pointers for plvi_local_map.
 *
 * Semantics:
 *   1. Vote (:5405-5421, :5559-5592).  Each voting feature that is not bad
 *      adds 1 to every keyframe of its observation list; with lines, points
 *      and lines vote into one counter.  A bad voting entry is written back
 *      as -1 (:5418 / :5442, :5589 / :5632) and casts no vote.  An id outside
 *      [0, n) is read as NULL.
 *   2. K1 (:5456-5471).  `order` is walked; a keyframe with a count that is
 *      not bad is listed (a bad one is skipped even with votes, :5460).
 *      ref_kf = pKFmax = the first keyframe in that order whose count is
 *      strictly above every earlier one (max starts at 0), -1 when nothing
 *      was counted (mpReferenceKF is then left alone, :5546).  K1 is not
 *      bounded; the 80 of :5477 limits the expansion only.
 *   3. Expansion (:5474-5524).  itEndKF is taken before the loop and the
 *      reserve(3 * size) of :5453 keeps it valid, so the loop visits the K1
 *      members only, in order, and stops once the list holds more than 80
 *      (size() > 80, tested before each visit).  Per visited keyframe: the
 *      first covisible that is not bad and not listed; then the first child
 *      in set order that is not bad and not listed; then the parent if it is
 *      not listed -- no isBad() test -- and adding a parent leaves the OUTER
 *      loop (:5521 / :5712): no later K1 member is expanded.
 *   4. Temporal walk (:5527-5544).  Only with last_kf[f] >= 0 (and prev_kf
 *      given) and fewer than 80 listed; at most 20 rounds; the walk moves to
 *      mPrevKF only after an insertion, so it ends at the first listed
 *      keyframe.
 *   5. Points (:5331-5351).  The local keyframes in REVERSE list order, each
 *      keyframe's table in index order, the first occurrence of every id that
 *      is not NULL and not bad.  Lines likewise; the reference interleaves
 *      them per keyframe (:5382-5395) into a list and a stamp of their own,
 *      which the two outputs cannot show.
 *   6. Not modelled.  mnTrackReferenceForFrame is written by these functions
 *      only and they run once per frame id, so "already listed" is state of
 *      one call: each frame of a batch is a fresh stamp.  A frame with mnId
 *      == 0 equals the constructors' stamp 0 and would list nothing in the
 *      reference; that is outside the model.
 *
 * Limits.  The vote histogram and the listed-set of a frame are kept in LDS
 * up to PLVI_LOCAL_MAP_LDS_KF slots (33 KB) and in the scratch block above.
 * The list passes run ceil(kf_cap * max(kp_cap, kl_cap) /
 * PLVI_LOCAL_MAP_GROUP_ENTRIES) workgroups per frame and kind, at least 1 and
 * at most PLVI_LOCAL_MAP_MAX_GROUPS, each over a contiguous
 * ceil(n_local_kf * cap / workgroups) entries of the walk.  An entry's
 * position in the walk is an int kept in a table whose "none" value is the
 * byte fill 0x7f7f7f7f, so kf_cap * max(kp_cap, kl_cap) is at most
 * PLVI_LOCAL_MAP_MAX_ENTRIES; more, or n_frames above 65535, returns
 * PLVI_E_CAPACITY and nothing is launched. */
#define PLVI_LOCAL_MAP_MAX_ENTRIES 0x7f7f7f7f /* largest kf_cap * max(kp_cap, kl_cap) */
#define PLVI_LOCAL_MAP_LDS_KF 8192        /* largest kf_cap whose vote histogram is kept in LDS */
#define PLVI_LOCAL_MAP_GROUP_ENTRIES 2048 /* keyframe-table entries per workgroup of the list passes */
#define PLVI_LOCAL_MAP_MAX_GROUPS 64
enum {
  PLVI_LOCAL_MAP_ERR_KF = 1, /* mvpLocalKeyFrames is longer than lkf_cap */
  PLVI_LOCAL_MAP_ERR_MP = 2, /* mvpLocalMapPoints is longer than lmp_cap */
  PLVI_LOCAL_MAP_ERR_ML = 4, /* mvpLocalMapLines is longer than lml_cap */
};

/* The keyframe side, by slot. */
typedef struct plvi_local_map_keyframes {
  int kf_cap;           /* slots */
  int n_order;          /* entries of order */
  int kp_cap, kl_cap;   /* row lengths of mp / ml */
  const uint8_t* bad;   /* [kf_cap] isBad(); 1 for an empty slot */
  const int* order;     /* [n_order] the occupied slots as a std::map<KeyFrame*, int> iterates them
                           (ascending address: INTEGRATION.md "Order"); a slot outside [0, kf_cap)
                           is ignored; a slot named twice is listed once, at either of its two positions (which one is
                           not specified: a std::map has no second key) */
  const int* covis;     /* [kf_cap][PLVI_KFDB_NEIGHBOURS] GetBestCovisibilityKeyFrames(10), ended by -1
                           (the table of plvi_kfdb_query_batch); NULL = none */
  const int* child_off; /* [kf_cap + 1] CSR of GetChilds() in std::set<KeyFrame*> order; NULL (both) = none */
  const int* child;
  const int* parent;    /* [kf_cap] GetParent() or -1; NULL = none */
  const int* prev_kf;   /* [kf_cap] mPrevKF or -1; NULL = no IMU sensor: the temporal walk never runs */
  const int* mp;        /* [kf_cap][kp_cap] GetMapPointMatches() as pool ids, -1 = NULL */
  const int* nmp;       /* [kf_cap] counts (count contract against kp_cap) */
  const int* ml;        /* [kf_cap][kl_cap] GetMapLineMatches(); NULL selects the point-only functions */
  const int* nml;
} plvi_local_map_keyframes;

/* One feature pool (MapPoints or MapLines), by id.  The attribute rows are
 * optional: a NULL row cannot be gathered.  desc rows are moved as dwords and
 * must be 4-byte aligned. */
typedef struct plvi_local_map_pool {
  int n;
  const uint8_t* bad;  /* [n] isBad() */
  const int* obs_off;  /* [n + 1] CSR of GetObservations() as keyframe slots; a keyframe appears once per */
  const int* obs_kf;   /*         feature (observations are map keys); a slot outside [0, kf_cap) is ignored */
  const float* pos;    /* MapPoints: [n][3] GetWorldPos() */
  const double* sep;   /* MapLines:  [n][6] GetWorldPos() */
  const float* normal; /* [n][3] GetNormal() */
  const float* dist;   /* [n][2] mfMinDistance, mfMaxDistance */
  const uint8_t* desc; /* [n][32] GetDescriptor() */
} plvi_local_map_pool;

/* Per frame f.  vote_*: the features that vote -- mCurrentFrame.mvpMapPoints,
 * or mLastFrame.mvpMapPoints in the IMU branch (:5403 against :5423), the
 * caller chooses -- as pool ids, -1 = NULL; in/out (semantics 1).  seen_*:
 * the CURRENT frame's own tables, which decide in_flags bit0; NULL = the vote
 * tables.  Every count follows the count contract (plvi_hamming_knn2_batch)
 * against its capacity.  vote_ml / seen_ml are read only with keyframes->ml. */
typedef struct plvi_local_map_frames {
  int* vote_mp;         /* [f][vote_mp_cap]; NULL = no point votes */
  const int* n_vote_mp; /* [f] */
  int vote_mp_cap;
  int* vote_ml;
  const int* n_vote_ml;
  int vote_ml_cap;
  const int* seen_mp;   /* [f][seen_mp_cap] */
  const int* n_seen_mp;
  int seen_mp_cap;
  const int* seen_ml;
  const int* n_seen_ml;
  int seen_ml_cap;
  const int* last_kf;   /* [f] mCurrentFrame.mpLastKeyFrame for IMU sensors, -1 otherwise; NULL = all -1 */
} plvi_local_map_frames;

/* Per frame f.  The n_* counts are always written and are the FULL list
 * lengths; list cells and gathered rows at or past min(count, capacity) are
 * never written, and a list longer than its capacity sets its bit of err[f]
 * (err[f] is written by every call, 0 when all three fit).  As counts they can
 * be handed to the frustum calls as they are (the count contract clamps
 * them).  The gathered tables have the layouts of plvi_frustum_points_batch
 * (pos, normal, dist, in_flags; desc is the d_mp_desc of
 * plvi_search_local_batch) and plvi_frustum_lines_batch (sep, normal, dist,
 * in_flags, desc), row stride lmp_cap / lml_cap; each may be NULL (no
 * gather).  in_flags bit0 = the id does not occur in the frame's seen table,
 * bad entries not counted (mnLastFrameSeen != mnId after the first loop of
 * SearchLocalPoints[AndLines], :5052-5069 / :5126-5161; a listed feature is
 * never bad); bit1 = its observation list is not empty (Observations() > 0). */
typedef struct plvi_local_map_outputs {
  int lkf_cap, lmp_cap, lml_cap;
  int* local_kf;   /* [f][lkf_cap] mvpLocalKeyFrames as slots */
  int* n_local_kf; /* [f] */
  int* ref_kf;     /* [f] pKFmax, -1 = leave mpReferenceKF alone */
  int* local_mp;   /* [f][lmp_cap] mvpLocalMapPoints as pool ids */
  int* n_local_mp;
  int* local_ml;   /* [f][lml_cap] mvpLocalMapLines; written with keyframes->ml only */
  int* n_local_ml;
  float* mp_pos;
  float* mp_normal;
  float* mp_dist;
  uint8_t* mp_in_flags;
  uint8_t* mp_desc;
  double* ml_sep;
  float* ml_normal;
  float* ml_dist;
  uint8_t* ml_in_flags;
  uint8_t* ml_desc;
  int* err;        /* [f] PLVI_LOCAL_MAP_ERR_* */
} plvi_local_map_outputs;

/* Bytes of the scratch block of plvi_local_map_batch: per frame 4 * (mp_n +
 * ml_n) for the first-occurrence tables, (mp_n + ml_n) / 8 for the seen-sets,
 * 4 * kf_cap for the full keyframe list (+ 4.125 * kf_cap above
 * PLVI_LOCAL_MAP_LDS_KF).  0 for a negative argument. */
size_t plvi_local_map_scratch_bytes(int n_frames, int kf_cap, int mp_n, int ml_n);

/* The batch call.  The structs themselves are host memory, read before the
 * call returns; ml may be NULL without keyframes->ml.  d_scratch holds at
 * least plvi_local_map_scratch_bytes(n_frames, kf_cap, mp->n, ml ? ml->n : 0)
 * bytes (PLVI_E_BADARG below) and needs no initialisation; calls that share a
 * scratch block must be ordered.  PLVI_E_BADARG for a negative size or a
 * missing required pointer, PLVI_E_CAPACITY as stated under Limits, 0 without
 * a launch for n_frames == 0.  Asynchronous on `stream`, no host read of
 * device data, no allocation: capturable like the other batch calls. */
int plvi_local_map_batch(int n_frames, const plvi_local_map_keyframes* kf, const plvi_local_map_pool* mp,
                         const plvi_local_map_pool* ml, const plvi_local_map_frames* frames,
                         const plvi_local_map_outputs* out, void* d_scratch, size_t scratch_bytes, void* stream);

/* One frame from host memory, synchronous: the same structs with host
 * pointers (per-frame arrays of one frame).  Lists and gathered rows are
 * copied back up to min(count, capacity); the vote tables are updated in
 * place.  Returns 0, PLVI_E_CAPACITY when err[0] != 0 (counts and err are
 * still written), or another error. */
int plvi_local_map(const plvi_local_map_keyframes* kf, const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                   const plvi_local_map_frames* frames, const plvi_local_map_outputs* out);

/* ------------------------------------------------------ Covisibility graph
 * KeyFrame::UpdateConnections / UpdateConnectionsWithLines
 * (src/KeyFrame.cc:499-622 / :624-769) for a batch of keyframes, with
 * AddConnection (:201-214), UpdateBestCovisibles (:216-238), EraseConnection
 * (:1154-1168), GetCovisiblesByWeight (:265-286) and GetWeight (:288-295), over
 * a device-resident graph.  It writes the covis table that plvi_kfdb_query_batch
 * and plvi_local_map_batch read, and the parent table of the latter.  Integers
 * only: every list equals the reference's entry for entry.
 *
 * The graph (plvi_covis_graph) holds, per keyframe slot of [0, kf_cap):
 *   the weight map   mConnectedKeyFrameWeights as unsorted (slot, weight)
 *                    pairs, at most conn_cap;
 *   the ordered list mvpOrderedConnectedKeyFrames / mvOrderedWeights, at most
 *                    conn_cap, descending by (weight, address);
 *   an error bit     set when either would exceed conn_cap: the excess is
 *                    dropped, the slot's state is then unspecified (memory
 *                    safety is not) until the slot is erased or updated again.
 *
 * Semantics of one query keyframe q (plvi_covis_update_batch):
 *   1. Count (:512-531).  Every entry of mp[q] (and of ml[q] with lines) that
 *      is not NULL, in range and not bad adds 1 to every keyframe of its
 *      observation list; one id twice counts twice.  A keyframe is left out if
 *      it is q itself, is bad, has another map_id, lies outside [0, kf_cap) or
 *      is not named in `order`.  An empty counter changes nothing (:534):
 *      n_counted = n_conn = 0, kf_max = -1, new_parent = -1.
 *   2. Walk (:547-567) in `order`.  kf_max / w_max = the first keyframe whose
 *      count is strictly above every earlier one.  Every keyframe with a count
 *      >= PLVI_COVIS_TH is listed and receives AddConnection(q, count); if
 *      there is none, kf_max alone.
 *   3. q's ordered list = the listed pairs, descending by (weight, address)
 *      -- sort() on pair<int, KeyFrame*> and push_front, :569-576; the address
 *      is the position in `order`, so of two equal weights the LATER keyframe
 *      of `order` comes first; NOT filtered for bad.  q's weight map = the whole counter,
 *      entries below the threshold included (:582).
 *   4. AddConnection on a neighbour: insert or overwrite q's entry; an entry
 *      that already held the weight leaves the neighbour alone; otherwise its
 *      ordered list becomes its WHOLE weight map minus the bad keyframes,
 *      sorted as in 3.  A list built by 3 and one built by 4 differ.
 *   5. Parent (:593-619).  With first_conn[q] set and init_kf[q] clear:
 *      parent[q] = the front of the new list, first_conn[q] = 0, new_parent =
 *      that slot (the caller does AddChild); -1 otherwise.
 * A batch equals the reference applied to the queries one after another in
 * index order: a keyframe that is itself query j (with a counter) loses the
 * connections added by the queries before j, whose own update overwrites them.
 * A slot of a map entry that `order` no longer names has an address above
 * the named ones, by slot.
 *
 * covis rows.  Every slot whose ordered list is rewritten gets its row of the
 * caller's covis [kf_cap][PLVI_KFDB_NEIGHBOURS] rewritten whole: the first
 * min(n, 10) entries, -1 in the cells after them.
 *
 * Limits.  conn_cap <= PLVI_COVIS_MAX_CONN (a list is sorted in LDS), kf_cap
 * <= 2^24, n_queries <= 65535: PLVI_E_CAPACITY beyond.  The vote histogram is
 * in LDS up to PLVI_COVIS_LDS_KF slots and in the scratch block above.  The
 * calls on one graph must be ordered (one stream, or events): they share its
 * work tables. */
#define PLVI_COVIS_LDS_KF 8192   /* largest kf_cap whose vote histogram is kept in LDS */
#define PLVI_COVIS_MAX_CONN 2048 /* largest conn_cap */
#define PLVI_COVIS_TH 15         /* th of KeyFrame.cc:541 */
#define PLVI_COVIS_MAX_QUERIES 65535

typedef struct plvi_covis_graph plvi_covis_graph;

/* The keyframe side, by slot; the layouts of plvi_local_map_keyframes.  Device
 * pointers for the batch call, host pointers for plvi_covis_update. */
typedef struct plvi_covis_keyframes {
  int kf_cap;             /* slots; equals the graph's */
  int n_order;            /* entries of order */
  int kp_cap, kl_cap;     /* row lengths of mp / ml */
  const uint8_t* bad;     /* [kf_cap] isBad(); 1 for an empty slot */
  const int* order;       /* [n_order] the occupied slots in ascending address; a slot named twice counts at its
                             first position */
  const int* mp;          /* [kf_cap][kp_cap] mvpMapPoints as pool ids, -1 = NULL */
  const int* nmp;         /* [kf_cap] counts (count contract against kp_cap) */
  const int* ml;          /* [kf_cap][kl_cap] mvpMapLines; NULL selects UpdateConnections */
  const int* nml;
  const int* map_id;      /* [kf_cap] GetMap() as an id; NULL = one map */
  const uint8_t* init_kf; /* [kf_cap] mnId == mpMap->GetInitKFid(); NULL = none */
  uint8_t* first_conn;    /* [kf_cap] mbFirstConnection, in/out; NULL (with parent) = semantics 5 is skipped */
  int* parent;            /* [kf_cap] mpParent as a slot, in/out */
  int* covis;             /* [kf_cap][PLVI_KFDB_NEIGHBOURS] out; may be NULL */
} plvi_covis_keyframes;

/* Per query, all required. */
typedef struct plvi_covis_outputs {
  int* n_counted;  /* KFcounter.size() */
  int* n_conn;     /* length of the ordered list built (before the cut at conn_cap) */
  int* kf_max;     /* pKFmax, -1 for an empty counter */
  int* w_max;      /* nmax */
  int* new_parent; /* the parent set by semantics 5, -1 = unchanged */
  int* err;        /* 1 = the query's map or list exceeded conn_cap */
} plvi_covis_outputs;

/* PLVI_E_BADARG for kf_cap < 1 or conn_cap < 1, PLVI_E_CAPACITY above the
 * limits.  Device memory: 16 * kf_cap * conn_cap + 32 * kf_cap bytes. */
int plvi_covis_create(int kf_cap, int conn_cap, int device, plvi_covis_graph** out);
int plvi_covis_destroy(plvi_covis_graph* h);

/* Bytes of the scratch block of plvi_covis_update_batch: 4 * n_queries *
 * kf_cap above PLVI_COVIS_LDS_KF, a few bytes below.  0 for a negative
 * argument. */
size_t plvi_covis_scratch_bytes(int n_queries, int kf_cap);

/* The batch call.  q_slot [n_queries] is host memory, read before the call
 * returns; a slot outside [0, kf_cap) or named twice returns PLVI_E_BADARG and
 * nothing is launched.  mp / ml: only n, bad, obs_off, obs_kf are read; ml ==
 * NULL or kf->ml == NULL selects the point-only function.  n_queries == 0
 * returns 0 without a launch.  Asynchronous on `stream`, no host read of
 * device data, no allocation: capturable like the other batch calls. */
int plvi_covis_update_batch(plvi_covis_graph* h, int n_queries, const int* q_slot, const plvi_covis_keyframes* kf,
                            const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                            const plvi_covis_outputs* out, void* d_scratch, size_t scratch_bytes, void* stream);

/* The connection part of SetBadFlag (:894-897, :915-916) for n slots (host
 * array, distinct, in range: PLVI_E_BADARG otherwise): EraseConnection(slot) on
 * every key of the slot's weight map -- the entry removed if present and only
 * then the neighbour re-sorted as in semantics 4 -- then the slot's own map,
 * list and error bit cleared.  Order-free.  d_bad / d_order as in
 * plvi_covis_keyframes; d_covis may be NULL.  The spanning tree stays with
 * the caller. */
int plvi_covis_erase_batch(plvi_covis_graph* h, int n, const int* slots, const uint8_t* d_bad, const int* d_order,
                           int n_order, int* d_covis, void* stream);

/* A bare UpdateBestCovisibles (LocalMapping.cc:1573, :1727) of n slots. */
int plvi_covis_resort_batch(plvi_covis_graph* h, int n, const int* slots, const uint8_t* d_bad, const int* d_order,
                            int n_order, int* d_covis, void* stream);

/* GetCovisiblesByWeight(d_w[i]) of slot d_slot[i]: d_count[i] = the length of
 * the prefix of the ordered list with weight >= w (0 for a slot out of
 * range). */
int plvi_covis_by_weight_batch(plvi_covis_graph* h, int n, const int* d_slot, const int* d_w, int* d_count,
                               void* stream);

/* d_weight[i] = d_a[i]->GetWeight(d_b[i]): the map entry or 0. */
int plvi_covis_weight_batch(plvi_covis_graph* h, int n, const int* d_a, const int* d_b, int* d_weight, void* stream);

/* Device pointers to the ordered tables [kf_cap][conn_cap] and their counts
 * [kf_cap] (GetVectorCovisibleKeyFrames without a copy); each may be NULL. */
int plvi_covis_rows(plvi_covis_graph* h, const int** d_ord_kf, const int** d_ord_w, const int** d_ord_n, int* conn_cap);

/* The twin for the weight maps: device pointers to the key and weight tables
 * [kf_cap][conn_cap], rows unsorted, and their counts [kf_cap]
 * (mConnectedKeyFrameWeights without a copy); each may be NULL. */
int plvi_covis_map_rows(plvi_covis_graph* h, const int** d_map_kf, const int** d_map_w, const int** d_map_n,
                        int* conn_cap);

/* Host copies of one slot, synchronous: the map in ascending slot order, the
 * ordered list as stored; tables of conn_cap entries, each may be NULL. */
int plvi_covis_download(plvi_covis_graph* h, int slot, int* map_kf, int* map_w, int* n_map, int* ord_kf, int* ord_w,
                        int* n_ord, int* err);

/* One keyframe from host tables, synchronous: first_conn, parent and covis
 * are updated in place (whole tables), out holds one entry each.  Returns 0,
 * PLVI_E_CAPACITY when err[0] != 0, or another error. */
int plvi_covis_update(plvi_covis_graph* h, int slot, const plvi_covis_keyframes* kf, const plvi_local_map_pool* mp,
                      const plvi_local_map_pool* ml, const plvi_covis_outputs* out);

/* -------------------------------------------------------- Keyframe culling
 * LocalMapping::KeyFrameCulling() / KeyFrameCullingWithLines()
 * (src/LocalMapping.cc:1566-1718 / :1720-1964) after their first two lines,
 * which are plvi_covis_resort_batch and plvi_covis_rows: the walk over the
 * current keyframe's covisibles that decides which of them are redundant.  The
 * walk is sequential -- a culled keyframe's SetBadFlag erases its
 * observations, which changes Observations() and the observer counts of every
 * later candidate and can kill features -- and is reproduced as such: every
 * output equals the reference's, candidate for candidate.  Nothing is applied
 * to the caller's tables: the call keeps the effects of its own culls in an
 * overlay and returns them as the changed list, which the caller replays.
 *
 * Tables.  Keyframes by slot and the two pools by id, in the layouts of
 * plvi_local_map_keyframes / plvi_local_map_pool -- of a pool only n, bad,
 * obs_off and obs_kf are read -- with two additions: one info byte per keyframe-table
 * entry and, per pool, a plvi_cull_features.  Device pointers for the batch
 * call, host pointers for plvi_keyframe_culling.
 *
 * Precondition (the map's own invariant): every observation (id, K, idx) of a
 * pool's CSR has mp[K][idx] == id (ml for lines) with idx < nmp[K].  A table
 * entry without an observation is allowed: EraseObservation then does nothing.
 * An observation whose slot lies outside [0, kf_cap) or whose idx lies outside
 * [0, kp_cap) is ignored.  The two-camera branches (NLeft != -1) are not
 * modelled.
 *
 * Semantics of one query (current keyframe q_slot, candidates cand[q_slot]):
 *   1. Candidates and the break (:1603-1609, :1713).  Candidates are visited
 *      in list order and `count` is incremented first.  The initial keyframe
 *      (SKIP_INIT) and a bad one (SKIP_BAD; also a slot outside [0, kf_cap) and
 *      a keyframe this walk has already erased) are skipped by `continue`.  The
 *      break test (count > 20 && abort_ba) || count > 100 stands at the bottom
 *      of the body and every `continue` skips it, the two inertial ones of 6
 *      included, so the walk can pass 101.
 *   2. Points (:1616-1672).  Every entry of mp[K] that is not NULL, not bad,
 *      not dead (5) and, with monocular == 0, not left out by depth (info bit
 *      6) counts into nMPs; one id twice counts twice.  It is redundant iff its
 *      live Observations() > 3 (:1630) and at least 4 OTHER observers (slot !=
 *      K) have an octave <= its own octave + 1 (nObs > thObs, :1661).  In the
 *      lines function it is counted into nRedundant only with slam_mode == 0
 *      (:1819); the points function does not read slam_mode.
 *   3. Lines (:1831-1873).  The same on ml[K] / kl_info, except that 3 other
 *      observers are enough (nObs >= thObs, :1862); always counted.
 *   4. The test (:1674, :1877, :1919) is (float)nRedundant > redundant_th *
 *      (float)n with the product rounded to float, n = nMPs (points function),
 *      nMPs + nMLs (lines, slam_mode == 0) or nMLs (lines, slam_mode != 0).
 *      0.9f * 10 rounds up to 9.0f: 9 of 10 is kept.  A candidate that fails
 *      the test is KEEP.
 *   5. Non-inertial cull (:1710, :1913): SetBadFlag (points function) or
 *      SetBadFlagWithLines.  With not_erase set nothing changes (CULLED |
 *      DEFERRED).  Otherwise every observation by the culled keyframe is
 *      erased: the feature's live nObs drops by 2 when bit 7 of the erased
 *      entry's info byte is set and by 1 otherwise, and a feature that had at
 *      least one erase and ends at nObs <= 2 is dead from then on -- bad, and
 *      gone from every later candidate's table.  nObs only decreases, so the
 *      dead set is a function of the set of culled keyframes.
 *   6. Inertial mode (:1676-1707), in the reference's order: n_kf_in_map <= 21
 *      -> KEEP_FEW_KF, continue (n_kf_in_map drops by one per keyframe really
 *      erased); kf_id > kf_id[q_slot] - 2 in unsigned 64-bit -> KEEP_RECENT,
 *      continue (never for kf_id[q_slot] < 2); prev or next missing ->
 *      KEEP_NO_CHAIN; t = (float)(timestamp[next] - timestamp[prev]), a double
 *      subtraction; (imu_init && kf_id < last_ID && t < 3) || t < 0.5 ->
 *      CULLED_TIME, where last_ID is the id reached by at most 21 prev steps
 *      from q_slot on the call's own prev_kf table; otherwise inertial_ba2 or
 *      !(t < 3) -> KEEP_TIME; otherwise the norm decides (7).  A cull relinks
 *      the chain (next->prev = prev, prev->next = next, own links cleared)
 *      BEFORE SetBadFlag, so a not_erase keyframe is relinked without being
 *      erased, and it calls SetBadFlag(), not SetBadFlagWithLines(), from the
 *      lines function too: the line observations of an inertially culled
 *      keyframe are NOT erased.
 *   7. cv::norm stays with the caller.  Where the decision hinges on the norm
 *      the walk STOPS: the candidate's outcome is NEEDS_NORM, stop is
 *      PLVI_CULL_STOP_NEEDS_NORM and the candidate stands at position
 *      n_visited - 1.  The caller evaluates norm < 0.02 and calls again with
 *      the SAME tables, start = that position, verdict = 0 or 1 and pre_* =
 *      the changed list of the earlier call as written.  The device rebuilds
 *      its overlay from that list with the code that applies a cull inside the
 *      loop; count continues from start; the verdict gives KEEP_NORM or
 *      CULLED_NORM.  The changed list of a resumed call begins with the pre
 *      list, so it is fed back whole to the next resume.
 * The queries of one call are independent: each starts from the call's tables
 * with its own overlay, and two queries on one map do not see each other's
 * culls.
 *
 * Limits.  The overlay is a list of at most PLVI_CULL_MAX_CHANGED keyframes
 * in LDS (a walk changes at most 101: a cull does not `continue`), whatever
 * kf_cap is.  n_queries <= 65535 (PLVI_E_CAPACITY beyond). */
#define PLVI_CULL_MAX_CHANGED 128
#define PLVI_CULL_SPEC 101 /* candidates from start whose counts are taken ahead of the walk */
enum { /* stop[q] */
  PLVI_CULL_STOP_END = 0,         /* the list ended */
  PLVI_CULL_STOP_BREAK_ABORT = 1, /* count > 20 && abort_ba */
  PLVI_CULL_STOP_BREAK_100 = 2,   /* count > 100 */
  PLVI_CULL_STOP_NEEDS_NORM = 3,
};
enum { /* outcome[q][p]: one code per exit of the loop body, | PLVI_CULL_DEFERRED */
  PLVI_CULL_NOT_VISITED = 0, /* never written; for the caller's fill */
  PLVI_CULL_SKIP_INIT = 1,
  PLVI_CULL_SKIP_BAD = 2,
  PLVI_CULL_KEEP = 3,          /* the test of semantics 4 failed */
  PLVI_CULL_KEEP_FEW_KF = 4,   /* redundant; KeyFramesInMap() <= 21 */
  PLVI_CULL_KEEP_RECENT = 5,   /* redundant; mnId > current mnId - 2 */
  PLVI_CULL_KEEP_NO_CHAIN = 6, /* redundant; mPrevKF or mNextKF missing */
  PLVI_CULL_KEEP_TIME = 7,     /* redundant; neither time rule culls and the norm cannot */
  PLVI_CULL_KEEP_NORM = 8,     /* redundant; verdict 0 */
  PLVI_CULL_CULLED = 9,        /* non-inertial */
  PLVI_CULL_CULLED_TIME = 10,
  PLVI_CULL_CULLED_NORM = 11,  /* verdict 1 */
  PLVI_CULL_NEEDS_NORM = 12,
  PLVI_CULL_DEFERRED = 0x80,   /* with a CULLED code: mbNotErase, SetBadFlag only set mbToBeErased */
};
enum { /* changed_kind, bits */
  PLVI_CULL_KIND_POINTS = 1,   /* erased: its MapPoint observations are gone, KeyFramesInMap() dropped */
  PLVI_CULL_KIND_LINES = 2,    /* its MapLine observations are gone too (SetBadFlagWithLines) */
  PLVI_CULL_KIND_RELINKED = 4, /* taken out of the mPrevKF / mNextKF chain (MergePrevious is due) */
  PLVI_CULL_KIND_DEFERRED = 8, /* mbToBeErased */
};
enum { /* err[q], bits */
  PLVI_CULL_ERR_OUT = 1,     /* candidates were visited at positions >= out_cap */
  PLVI_CULL_ERR_CHANGED = 2, /* the changed list is longer than changed_cap (or PLVI_CULL_MAX_CHANGED) */
  PLVI_CULL_ERR_PRE = 4,     /* pre_n above min(pre_cap, PLVI_CULL_MAX_CHANGED), or an entry with a slot out of
                                range or unknown kind bits (such an entry is left out) */
  PLVI_CULL_ERR_QUERY = 8,   /* q_slot outside [0, kf_cap) or start < 0: nothing visited */
};

/* The keyframe side, by slot. */
typedef struct plvi_cull_keyframes {
  int kf_cap;               /* slots */
  int kp_cap, kl_cap;       /* row lengths of mp / kp_info and ml / kl_info */
  int cand_stride;          /* row length of cand */
  const uint8_t* bad;       /* [kf_cap] isBad(); 1 for an empty slot */
  const uint8_t* init_kf;   /* [kf_cap] mnId == GetMap()->GetInitKFid(); NULL = none */
  const uint8_t* not_erase; /* [kf_cap] mbNotErase; NULL = none */
  const int* mp;            /* [kf_cap][kp_cap] GetMapPointMatches() as pool ids, -1 = NULL */
  const int* nmp;           /* [kf_cap] counts (count contract against kp_cap) */
  const int* ml;            /* [kf_cap][kl_cap] GetMapLineMatches(); NULL selects KeyFrameCulling() */
  const int* nml;
  const uint8_t* kp_info;   /* [kf_cap][kp_cap] bits 0-5 mvKeysUn[i].octave; bit 6 left out by depth: mvDepth[i] >
                               mThDepth || mvDepth[i] < 0 (read only with monocular == 0); bit 7 erasing this
                               observation takes 2 off nObs: !mpCamera2 && mvuRight[i] >= 0 (MapPoint.cc:180) */
  const uint8_t* kl_info;   /* [kf_cap][kl_cap] bits 0-5 mvKeysUn_Line[i].octave; bit 6 the four-way test of :1842;
                               bit 7 both mvDepth_l[i] >= 0 (MapLine.cc:139) */
  const int* cand;          /* [kf_cap][cand_stride] GetVectorCovisibleKeyFrames() per slot: the d_ord_kf of */
  const int* n_cand;        /* [kf_cap]              plvi_covis_rows, read in place (stride conn_cap), and d_ord_n */
  const unsigned* kf_id;    /* [kf_cap] mnId.  These four are read, and required, with inertial != 0 only */
  const double* timestamp;  /* [kf_cap] mTimeStamp */
  const int* prev_kf;       /* [kf_cap] mPrevKF or -1 */
  const int* next_kf;       /* [kf_cap] mNextKF or -1 */
} plvi_cull_keyframes;

/* What the walk reads of a pool besides plvi_local_map_pool. */
typedef struct plvi_cull_features {
  const int* obs_idx; /* parallel to obs_kf: the feature's index in that keyframe (get<0> of the tuple) */
  const int* nobs;    /* [n] Observations(): the reference keeps nObs apart from the map (a stereo point counts 2,
                         MapLine::AddObservation adds 1 where EraseObservation may take 2); NULL = the list length */
} plvi_cull_features;

/* Host struct, read before the call returns. */
typedef struct plvi_cull_params {
  float redundant_th; /* 0.9f or 0.5f as :1576-1582 chooses */
  int monocular;      /* mbMonocular */
  int inertial;       /* mbInertial */
  int slam_mode;      /* mpTracker->SLAM; read by the lines function only */
} plvi_cull_params;

/* Per query q; arrays of n_queries entries.  start / verdict / pre_* may be
 * NULL together = every query is fresh. */
typedef struct plvi_cull_queries {
  const int* q_slot;       /* mpCurrentKeyFrame: its row of cand is walked */
  const int* abort_ba;     /* mbAbortBA */
  const int* n_kf_in_map;  /* mpAtlas->KeyFramesInMap() BEFORE the walk (a resumed call gives it again) */
  const int* imu_init;     /* mpAtlas->isImuInitialized() */
  const int* inertial_ba2; /* GetIniertialBA2() */
  const int* start;        /* first position to visit; 0 for a fresh query */
  const int* verdict;      /* norm < 0.02 for the candidate at start: 0 or 1; -1 = none */
  int pre_cap;             /* row length of pre_slot / pre_kind */
  const int* pre_n;        /* the changed list of the call that stopped at start; 0 for a fresh query */
  const int* pre_slot;     /* [q][pre_cap] */
  const int* pre_kind;
} plvi_cull_queries;

/* Per query q.  Cells at positions < start, >= n_visited or >= out_cap are
 * never written, nor are changed cells at or past min(n_changed, changed_cap);
 * n_visited, stop, n_kf_in_map, err and n_changed are always written. */
typedef struct plvi_cull_outputs {
  int out_cap, changed_cap;
  int* n_visited;     /* count: one past the position of the last candidate visited */
  int* stop;          /* PLVI_CULL_STOP_* */
  int* n_kf_in_map;   /* KeyFramesInMap() after the walk */
  int* err;           /* PLVI_CULL_ERR_* */
  uint8_t* outcome;   /* [q][out_cap] by position in the candidate list */
  int* n_mps;         /* [q][out_cap] nMPs (0 for a skipped candidate, as the other two) */
  int* n_mls;         /* [q][out_cap] nMLs; 0 in the points function */
  int* n_redundant;   /* [q][out_cap] nRedundantObservations */
  int* n_changed;     /* full length of the changed list */
  int* changed_slot;  /* [q][changed_cap] every candidate culled, deferred or relinked, in order */
  int* changed_kind;  /* [q][changed_cap] PLVI_CULL_KIND_* */
} plvi_cull_outputs;

/* The batch call.  The structs themselves are host memory, read before the
 * call returns.  ml / fml may be NULL without kf->ml; kf->ml == NULL or ml ==
 * NULL selects KeyFrameCulling().  PLVI_E_BADARG for a negative size, a
 * missing required pointer (every pointer not marked optional; fmp->obs_idx
 * with mp->n > 0) or start / verdict / pre_* given in part; n_queries == 0
 * returns 0 without a launch.  d_scratch holds at least
 * plvi_keyframe_culling_scratch_bytes(n_queries) bytes (PLVI_E_BADARG below)
 * and needs no initialisation; calls that share a scratch block must be
 * ordered.  Two launches: the counts of the first PLVI_CULL_SPEC candidates of
 * every query are taken ahead, one workgroup each, against the overlay known
 * at launch; the walk, one workgroup per query, uses them until it erases a
 * keyframe and from then on counts each candidate itself under its overlay,
 * thread 0 doing the gates.  Asynchronous on `stream`, no host read of device
 * data, no allocation: capturable like the other batch calls. */
size_t plvi_keyframe_culling_scratch_bytes(int n_queries); /* 256 + 16 * PLVI_CULL_SPEC * n_queries; 0 if negative */
int plvi_keyframe_culling_batch(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                                const plvi_cull_features* fmp, const plvi_local_map_pool* ml,
                                const plvi_cull_features* fml, const plvi_cull_params* params,
                                const plvi_cull_queries* queries, const plvi_cull_outputs* out, void* d_scratch,
                                size_t scratch_bytes, void* stream);

/* One query from host tables, synchronous: the same structs with host
 * pointers, per-query arrays of one entry.  Returns 0, PLVI_E_CAPACITY when
 * err[0] != 0 (everything is still written), or another error. */
int plvi_keyframe_culling(const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp, const plvi_cull_features* fmp,
                          const plvi_local_map_pool* ml, const plvi_cull_features* fml, const plvi_cull_params* params,
                          const plvi_cull_queries* queries, const plvi_cull_outputs* out);

/* ------------------------------------------------------- Local BA window
 * The set-up of Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap,
 * num_fixedKF) (src/Optimizer.cc:4851-4960, edge loop :5048-5168),
 * LocalBundleAdjustmentOnlyLines / ...OnlyLinesAngle / ...OnlyLinesWithAngle
 * (:6181-6233, :6433-6485, :6689-6741, one text three times; edge loop
 * :6291-6337, whose condition the two Angle variants share) and
 * LocalInertialBA (:9185-9307, :9521-9640) for a batch of current keyframes:
 * the local keyframes, the local features, the fixed cameras and the
 * (feature, keyframe, index) edge list.  Integers only; every output equals
 * the reference's.  g2o, the vertex estimates, invSigma2, the inertial edges
 * and the outlier pass stay with the caller.
 *
 * Tables.  The keyframe side is plvi_cull_keyframes, of which mp / nmp / ml /
 * nml, bad, init_kf, cand / n_cand, kf_id (POINTS), prev_kf (INERTIAL) and bit
 * 7 of kp_info are read; the pools are plvi_local_map_pool, read for n, bad,
 * obs_off and obs_kf, with a plvi_ba_features each.  kf_map_id [kf_cap] and
 * plvi_ba_features.map_id are GetMap() as an integer, NULL = one map:
 * `GetMap() == pCurrentMap` is map_id == kf_map_id[q_slot].  POINTS and
 * INERTIAL read mp / fmp, LINES reads kf->ml / ml / fml.  A NULL kp_info
 * makes every point edge a mono edge.
 *
 * The mnBALocalForKF / mnBAFixedForKF stamps are state of one query (each
 * query is a fresh mnId; mnId == 0 equals the constructors' stamp and is
 * outside the model), kept as per-slot tables and resolved as "the smallest
 * traversal position wins".
 *
 * Semantics of one query (keyframe q = q_slot, map M = kf_map_id[q]):
 *   1. Local keyframes, visual modes (:4857-4868): q, then q's cand row in
 *      order.  Every row entry in [0, kf_cap) is stamped local; it is listed
 *      iff it is not bad and (POINTS) in map M -- the lines functions have no
 *      map test (:6195).  q in its own row is listed twice.
 *   2. Local features (:4874-4896, :6201-6215): the listed keyframes in list
 *      order, each table in index order; the first occurrence of every id
 *      that is in range, not bad and (visual modes) in map M.  init_in_local
 *      = some listed keyframe has init_kf set.
 *   3. Fixed cameras (:4899-4914): the local features in list order, each
 *      observation list in CSR order; a keyframe in [0, kf_cap) stamped
 *      neither local nor fixed is stamped fixed, and listed iff it is not bad
 *      and in map M.
 *   4. POINTS only (:4915-4954): num_fixed = n_fixed + init_in_local; below 2
 *      the selection loop runs over the local list as written -- q and the
 *      initial keyframe are skipped; mnId < lowerId compares the 64-bit mnId
 *      with the SIGN-EXTENDED int, unsigned (movslq / cmp / jb in the
 *      reference's object); the `else if` gives the second candidate only to a
 *      keyframe that did not take "lowest" -- and pLowerKf, then (still below
 *      2) pSecondLowerKF, move from the local list (every equal element) to
 *      the end of the fixed list.  A pointer never assigned moves nothing and
 *      sets PLVI_BA_ERR_UNDEFINED; num_fixed is incremented all the same.
 *      The features of 2 are not recomputed.
 *   5. INERTIAL (:9197-9307): Nd = min(n_kf_in_map - 2, max_opt); the
 *      optimizable list is q and prev_kf steps while it is shorter than Nd (no
 *      bad test, no map test), local features from those keyframes as in 2
 *      WITHOUT the map test (:9229).  If the back's prev_kf exists it is the
 *      first fixed keyframe; otherwise the back itself is, and is popped from
 *      the optimizable list (its features stay).  The covisible loop of :9255
 *      never runs (maxCovKF is 0).  Then, per local feature in order, the
 *      first observer in CSR order that is in range, unstamped and not bad is
 *      stamped fixed and listed and the feature's loop breaks (bad unstamped
 *      observers are stamped and passed); after each feature the walk ends
 *      once the fixed list holds PLVI_BA_MAX_FIXED_INERTIAL keyframes.
 *      non_fixed = the fixed list is empty.
 *   6. Edges: the local features in list order, each observation list in CSR
 *      order; an observation is an edge iff its keyframe is in range, not bad
 *      and in map M, (INERTIAL) stamped local or fixed (:9538), and obs_idx is
 *      inside the keyframe table's row.  Kind: PLVI_BA_EDGE_STEREO where bit 7
 *      of kp_info[kf][idx] is set, else MONO; LINE in LINES.  vpEdgesMono... are
 *      the kind-0 subsequence of the merged list, vpEdgesStereo... the kind-1
 *      one.  edge_feat is the feature's position in local_feat, edge_cam the
 *      keyframe's first position in local_kf || fixed_kf after the moves of 4
 *      and the pop of 5; it would be -1 for a keyframe in neither list, which
 *      no input produces (the argument per mode is in DESIGN.md).  The
 *      two-camera branches are not modelled.
 *
 * Outputs follow the count contract: counts are full lengths, nothing is
 * written at or past min(count, cap), err[q] has a bit per overflowed list.
 *
 * Limits.  n_queries <= 65535 and kf_cap * max(kp_cap, kl_cap) <=
 * PLVI_LOCAL_MAP_MAX_ENTRIES (PLVI_E_CAPACITY beyond); max_opt <=
 * PLVI_BA_MAX_OPT (PLVI_E_BADARG beyond).  The per-slot stamp / position
 * tables are in LDS up to kf_cap = PLVI_BA_LDS_KF and in the scratch block
 * above.  No other bound on kf_cap, n, cand_stride or the list lengths. */
#define PLVI_BA_LDS_KF 2048           /* largest kf_cap whose per-slot tables are kept in LDS (24 KB) */
#define PLVI_BA_MAX_OPT 64            /* largest max_opt */
#define PLVI_BA_MAX_FIXED_INERTIAL 200 /* maxFixKF of :9284 */
enum { /* plvi_ba_params.mode */
  PLVI_BA_POINTS = 0,
  PLVI_BA_LINES = 1,
  PLVI_BA_INERTIAL = 2,
};
enum { /* edge_kind */
  PLVI_BA_EDGE_MONO = 0,
  PLVI_BA_EDGE_STEREO = 1,
  PLVI_BA_EDGE_LINE = 2,
};
enum { /* err[q] */
  PLVI_BA_ERR_LOCAL_KF = 1,   /* local_kf is longer than lkf_cap */
  PLVI_BA_ERR_FIXED_KF = 2,   /* fixed_kf is longer than fkf_cap */
  PLVI_BA_ERR_FEAT = 4,       /* local_feat is longer than feat_cap */
  PLVI_BA_ERR_EDGE = 8,       /* the edge list is longer than edge_cap */
  PLVI_BA_ERR_UNDEFINED = 16, /* the reference would push an uninitialised pLowerKf / pSecondLowerKF */
  PLVI_BA_ERR_QUERY = 32,     /* q_slot outside [0, kf_cap): every count is 0 */
};

typedef struct plvi_ba_features {
  const int* obs_idx; /* parallel to obs_kf: get<0> of the tuple for points, the size_t for lines */
  const int* map_id;  /* [n] GetMap(); NULL = one map */
} plvi_ba_features;

/* Host struct, read before the call returns. */
typedef struct plvi_ba_params {
  int mode;    /* PLVI_BA_* */
  int max_opt; /* INERTIAL: 10 or 25 as bLarge chooses (:9190-9196) */
} plvi_ba_params;

typedef struct plvi_ba_queries {
  const int* q_slot;      /* [q] pKF */
  const int* n_kf_in_map; /* [q] pCurrentMap->KeyFramesInMap(); INERTIAL only, NULL otherwise */
} plvi_ba_queries;

typedef struct plvi_ba_outputs {
  int lkf_cap, fkf_cap, feat_cap, edge_cap;
  int* local_kf;      /* [q][lkf_cap] lLocalKeyFrames / vpOptimizableKFs as slots */
  int* n_local_kf;
  int* fixed_kf;      /* [q][fkf_cap] lFixedCameras / lFixedKeyFrames */
  int* n_fixed_kf;
  int* num_fixed;     /* POINTS: num_fixedKF as the reference leaves it; otherwise n_fixed_kf */
  int* init_in_local;
  int* non_fixed;     /* n_fixed_kf == 0 (bNonFixed) */
  int* local_feat;    /* [q][feat_cap] lLocalMapPoints / lLocalMapLines as pool ids */
  int* n_local_feat;
  int* edge_feat;     /* [q][edge_cap] position in local_feat */
  int* edge_kf;       /* [q][edge_cap] slot */
  int* edge_idx;      /* [q][edge_cap] */
  int* edge_cam;      /* [q][edge_cap] position in local_kf || fixed_kf, or -1 */
  uint8_t* edge_kind; /* [q][edge_cap] PLVI_BA_EDGE_* */
  int* n_mono;        /* the edge list is n_mono + n_stereo + n_line long */
  int* n_stereo;
  int* n_line;
  int* err;           /* PLVI_BA_ERR_* */
} plvi_ba_outputs;

/* The batch call: one workgroup per query, one launch.  The structs are host
 * memory, read before the call returns; their pointers are device pointers.
 * The pool of the mode (mp / fmp, or ml / fml for LINES) is required, the other
 * may be NULL.  PLVI_E_BADARG for a negative size, an unknown mode or a
 * missing required pointer; n_queries == 0 returns 0 without a launch.
 * d_scratch holds at least plvi_ba_window_scratch_bytes(...) bytes, needs no
 * initialisation, and calls that share it must be ordered.  Asynchronous on
 * `stream`, no host read of device data, no allocation: capturable. */
size_t plvi_ba_window_scratch_bytes(int n_queries, int kf_cap, int mp_n, int ml_n);
int plvi_ba_window_batch(int n_queries, const plvi_cull_keyframes* kf, const int* kf_map_id,
                         const plvi_local_map_pool* mp, const plvi_ba_features* fmp, const plvi_local_map_pool* ml,
                         const plvi_ba_features* fml, const plvi_ba_params* params, const plvi_ba_queries* queries,
                         const plvi_ba_outputs* out, void* d_scratch, size_t scratch_bytes, void* stream);

/* One query from host tables, synchronous: the same structs with host
 * pointers, per-query arrays of one entry.  Returns 0, PLVI_E_CAPACITY when
 * err[0] has an overflow bit or PLVI_BA_ERR_QUERY (everything is still
 * written), or another error. */
int plvi_ba_window(const plvi_cull_keyframes* kf, const int* kf_map_id, const plvi_local_map_pool* mp,
                   const plvi_ba_features* fmp, const plvi_local_map_pool* ml, const plvi_ba_features* fml,
                   const plvi_ba_params* params, const plvi_ba_queries* queries, const plvi_ba_outputs* out);

/* ------------------------------------------------- Loop-detection windows
 * The integer work of LoopClosing::NewDetectCommonRegions between its device
 * calls (src/LoopClosing.cc): the six-keyframe window around a BoW candidate
 * and its abort by proximity (DetectCommonRegionsFromBoW, :797-804 and
 * :833-840), the first-come merge of the six SearchByBoW results into one
 * match table (:818-858), the covisible window of :893-915 with its point
 * cloud and owners (vpPoints / vpPointsKFs of
 * plvi_search_sim3_projection_batch) and the window and point cloud of
 * FindMatchesByProjection (:1162-1199).  Integers only; every output equals
 * the reference's.  Sim3Solver, OptimizeSim3, every g2o::Sim3 / cv::Mat
 * product, the per-point inputs of the projection search, the thresholds and
 * SetNotErase / SetErase stay with the caller.
 *
 * Tables.  The keyframe side is plvi_cull_keyframes, of which kf_cap, kp_cap,
 * bad, mp / nmp (nmp under the count contract against kp_cap) and cand /
 * n_cand / cand_stride are read: the rows of plvi_covis_rows in place.  The
 * pool is plvi_local_map_pool, read for n and bad, and for pos / normal / dist
 * / desc where a gather is asked for.  cov5(s) below is
 * GetBestCovisibilityKeyFrames(5) (KeyFrame.cc:255-263): the first
 * min(PLVI_LOOP_COVISIBLES, n_cand[s]) entries of row s as stored, with no
 * isBad() test.  An entry outside [0, kf_cap) is listed in the window as
 * stored and contributes neither a table nor (LAST) a row of its own.
 *
 * Semantics of one query, by kind:
 *   BOW (candidate i = kf_slot, current keyframe cur_slot).  A bad candidate
 *      is skipped (:797): n_win = 0, abort_at = -1.  Otherwise the window is
 *      cov5(i), push_back(front), [0] = i (:802-804): i, c1, c2, c3, c4, c0 --
 *      i, c0 with one covisible.  With none the reference indexes an empty
 *      vector; the window is i alone and PLVI_LOOP_ERR_UNDEFINED is set.
 *      abort_at = the first window position whose keyframe is in the connected
 *      set of the query (:833-840; a bad member is tested like any other), -1
 *      without one.  It depends on nothing SearchByBoW produces, so it is
 *      known before the six searches.  n_pts = 0.
 *   PROJ (around m = kf_slot; pMostBoWMatchesKF is never reassigned after
 *      :811, so m is always the candidate).  The window is cov5(m) followed by
 *      m (:893-895).  The tables of the window are walked in that order, each
 *      in index order; the first occurrence of every id that is in range and
 *      not bad is listed in pts, with the keyframe where it occurred in pts_kf
 *      (:901-915).  No isBad() test on the window's members.
 *   LAST (around m).  cov5(m), m, then for each of the first |cov5(m)| members
 *      in order ALL of its cov5 (:1167-1182; the nInserted loop writes a set
 *      that nothing reads): at most 5 + 1 + 25 entries, repeats and m itself
 *      included.  A repeated keyframe contributes nothing the second time.
 *      pts as for PROJ; pts_kf is not written.  The window depends on m
 *      alone: one query serves every call of FindMatchesByProjection against
 *      the same pMatchedKFw.
 *
 * Merge (:842-857), one per BOW query.  Members j < min(n_win, abort_at if >=
 * 0) that are in range and not bad (a bad member was not searched, :820) are
 * read in order, each for k ascending over [0, n1): p = mp[win[j]][m] with m =
 * matches12[q][j][k], skipped when m is outside the member's table or p is
 * NULL, out of range or bad.  A p not seen before is inserted: num is
 * incremented, matched_mp[k] = p, matched_kf[k] = win[j].  A later member can
 * overwrite cell k with another new point, so num counts distinct points and
 * can exceed the number of cells that are not -1.  nIndexMostBoWMatchesKF is
 * computed by the reference and never read; it has no counterpart here.
 *
 * Outputs follow the count contract: n_win and n_pts are full lengths,
 * nothing is written at or past a capacity, err[q] is written by every call.
 *
 * Limits.  n_queries <= 65535, max(kf_cap, PLVI_LOOP_WIN_MAX) * kp_cap and
 * PLVI_LOOP_BOW_WIN * cap1 <= PLVI_LOCAL_MAP_MAX_ENTRIES (a walk position is
 * an unsigned int; PLVI_E_CAPACITY beyond).  No bound on the pool. */
#define PLVI_LOOP_COVISIBLES 5 /* nNumCovisibles */
#define PLVI_LOOP_BOW_WIN 6    /* longest BOW window */
#define PLVI_LOOP_WIN_MAX 31   /* longest LAST window; row length of win */
enum { /* plvi_loop_queries.kind */
  PLVI_LOOP_WIN_BOW = 0,
  PLVI_LOOP_WIN_PROJ = 1,
  PLVI_LOOP_WIN_LAST = 2,
};
enum { /* err[q], bits */
  PLVI_LOOP_ERR_PTS = 1,       /* the point list is longer than pt_cap */
  PLVI_LOOP_ERR_UNDEFINED = 2, /* a BOW candidate has no covisible: the reference reads vpCovKFi[0] of an empty vector */
  PLVI_LOOP_ERR_QUERY = 4,     /* kf_slot (or a given cur_slot, BOW) outside [0, kf_cap), or an unknown kind:
                                  n_win = n_pts = 0, abort_at = -1 */
};

/* Per query q; arrays of n_queries entries. */
typedef struct plvi_loop_queries {
  const int* kind;      /* PLVI_LOOP_WIN_* */
  const int* kf_slot;   /* i for BOW, m for PROJ and LAST */
  const int* cur_slot;  /* BOW: mpCurrentKF, the keyframe whose connected set row q of the CSR below holds.  It is
                           checked against [0, kf_cap) and not otherwise read (the set never holds the keyframe
                           itself); NULL = not checked */
  const int* conn_off;  /* [q + 1] CSR of GetConnectedKeyFrames() per query, the layout of plvi_kfdb_query_batch; */
  const int* conn_slot; /*         both NULL = no keyframe is connected; a slot outside [0, kf_cap) is ignored */
} plvi_loop_queries;

/* Per query q.  The gathered rows have the layouts of plvi_local_map_outputs
 * (pos [q][pt_cap][3], normal [q][pt_cap][3], dist [q][pt_cap][2], desc
 * [q][pt_cap][32], moved as dwords: 4-byte aligned), row stride pt_cap; each
 * may be NULL (no gather) and needs its row of the pool. */
typedef struct plvi_loop_outputs {
  int pt_cap;
  int* win;      /* [q][PLVI_LOOP_WIN_MAX] the window as slots */
  int* n_win;    /* [q] */
  int* abort_at; /* [q] BOW: the window position that aborts by proximity or -1; -1 for the other kinds */
  int* pts;      /* [q][pt_cap] vpMapPoints as pool ids (PROJ, LAST) */
  int* pts_kf;   /* [q][pt_cap] vpKeyFrames: the slot where the point occurred first; written by PROJ; may be NULL */
  int* n_pts;    /* [q] full length; 0 for BOW */
  float* pos;
  float* normal;
  float* dist;
  uint8_t* desc;
  int* err;      /* [q] PLVI_LOOP_ERR_* */
} plvi_loop_outputs;

/* Bytes of the scratch block of both batch calls: 256 + 4 * mp_n per query (a
 * first-occurrence table by pool id).  0 for a negative argument. */
size_t plvi_loop_window_scratch_bytes(int n_queries, int mp_n);

/* The window call: one workgroup per query, plus one launch of (pt_cap / 256
 * chunks, queries) when a gather is asked for.  The structs are host memory,
 * read before the call returns; their pointers are device pointers.
 * PLVI_E_BADARG for a negative size, a missing required pointer (everything
 * not marked optional; pts with pt_cap > 0), conn_off / conn_slot given in
 * part, or a gather without its pool row; n_queries == 0 returns 0 without a
 * launch.  d_scratch holds at least plvi_loop_window_scratch_bytes(n_queries,
 * mp->n) bytes (PLVI_E_BADARG below), needs no initialisation, and calls that
 * share it must be ordered.  Asynchronous on `stream`, no host read of device
 * data, no allocation: capturable. */
int plvi_loop_window_batch(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                           const plvi_loop_queries* queries, const plvi_loop_outputs* out, void* d_scratch,
                           size_t scratch_bytes, void* stream);

/* The merge call, one workgroup per query.  d_win [q][PLVI_LOOP_WIN_MAX],
 * d_n_win [q] and d_abort_at [q] as plvi_loop_window_batch wrote them for BOW
 * queries; d_matches12 [q][PLVI_LOOP_BOW_WIN][cap1] is the output of
 * plvi_search_by_bow_kf_batch with n_pairs = 6 * n_queries and pair p = 6 * q
 * + j; d_n1 [q] follows the count contract against cap1.  Rows of bad members
 * and of members at or past abort_at or n_win are not read.  Outputs
 * d_matched_mp / d_matched_kf [q][cap1] (pool id / slot, or -1; rows [0, n1)
 * are fully written, nothing past them) and d_num [q].  kf is read for kf_cap,
 * kp_cap, bad, mp and nmp, mp for n and bad.  Scratch, errors and
 * capturability as above. */
int plvi_loop_bow_merge_batch(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                              const int* d_win, const int* d_n_win, const int* d_abort_at, const int* d_matches12,
                              const int* d_n1, int cap1, int* d_matched_mp, int* d_matched_kf, int* d_num,
                              void* d_scratch, size_t scratch_bytes, void* stream);

/* One query from host tables, synchronous: the same structs with host
 * pointers, per-query arrays of one entry (conn_off of two).  Returns 0,
 * PLVI_E_CAPACITY when err[0] has PLVI_LOOP_ERR_PTS or PLVI_LOOP_ERR_QUERY
 * (everything is still written), or another error. */
int plvi_loop_window(const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp, const plvi_loop_queries* queries,
                     const plvi_loop_outputs* out);

/* One merge from host memory, synchronous: win [PLVI_LOOP_WIN_MAX], matches12
 * [PLVI_LOOP_BOW_WIN][cap1], matched_mp / matched_kf [cap1], the rest one int
 * each. */
int plvi_loop_bow_merge(const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp, const int* win,
                        const int* n_win, const int* abort_at, const int* matches12, const int* n1, int cap1,
                        int* matched_mp, int* matched_kf, int* num);

/* -------------------------------------------------------- Essential graph
 * The integer work of LoopClosing::CorrectLoop[WithLines]
 * (src/LoopClosing.cc:1212-1473, :1475-1712) and of
 * Optimizer::OptimizeEssentialGraph / OptimizeEssentialGraph4DoF
 * (src/Optimizer.cc:6952-7305, :14411-) around the Sim3 arithmetic and the
 * solver: the corrected window with the keyframe that corrects each MapPoint
 * / MapLine first (plvi_loop_correct), and the vertex list, the ordered edge
 * list and the reference keyframe of every feature (plvi_essential_graph).
 * Integers only; every output equals the reference's.  One loop closure per
 * call.  Every Sim3 / cv::Mat product, the measurements and information
 * matrices, the solver, SetPose and UpdateNormalAndDepth stay with the caller.
 *
 * Tables.  plvi_cull_keyframes is read for kf_cap, kp_cap / kl_cap, bad,
 * init_kf, mp / nmp, ml / nml, cand / n_cand / cand_stride (the ordered rows
 * of plvi_covis_rows in place), kf_id, prev_kf and next_kf; the last three are
 * required here.  The pools are read for n and bad.  plvi_eg_keyframes adds
 * what the two functions read besides; plvi_eg_features is one per pool.
 * Distinct slots have distinct kf_id (the reference keys sInsertedEdges and
 * the cur / loop exemption by mnId; here both go by slot).
 *
 * Address order.  `order` models every std::set<KeyFrame*> and std::map<
 * KeyFrame*, ...> iteration: a slot named twice counts at its first position,
 * a slot in [0, kf_cap) that `order` does not name sorts above the named ones,
 * by slot.
 *
 * plvi_loop_correct (:1252-1253, :1294-1345; the points-only twin :1557-1586:
 * ml == NULL or kf->ml == NULL selects CorrectLoop).
 *   1. win = the cand row of cur_slot as stored, then cur_slot
 *      (mvpCurrentConnectedKFs).  An entry outside [0, kf_cap) is listed as
 *      stored and contributes nothing.  No isBad() and no map test (:1294).
 *   2. win_sorted = the distinct members in range, in address order (the
 *      iteration of CorrectedSim3).
 *   3. The members of win_sorted are walked in order, each one's mp row in
 *      index order.  An entry is listed in pts, with the member in pts_kf, iff
 *      it is not NULL, in range, not bad, corr_by[id] != kf_id[cur_slot] on
 *      entry, and was not met earlier in the walk.  Lines likewise over ml.
 *   4. Every listed feature is stamped: corr_by[id] = kf_id[cur_slot],
 *      corr_ref[id] = the member -- past pt_cap / ln_cap too: the stamp is
 *      state, not a list.  A NULL features struct, or a NULL corr_by in it,
 *      means nothing is stamped on entry and nothing is written.
 *
 * plvi_essential_graph.  M = map_id[cur_slot]; vpKFs = the entries of `order`
 * (first positions, in range) whose map is M, in order.  win / n_win [1] are
 * those of plvi_loop_correct (n_win under the count contract against
 * win_cap); lc_kf [win_cap][lc_cap] / n_lc [win_cap] hold LoopConnections by
 * window position, each row in address order.  A slot at two positions is
 * read at its last one (LoopConnections[pKFi] = overwrites).
 *   1. Vertices (:6985-7021, :14442-14479): the members of vpKFs that are not
 *      bad, in order.  vert_flags bit 0 = fixed (init_kf in 7DOF, slot ==
 *      loop_slot in 4DOF), bit 1 = the slot is a window member (its estimate
 *      comes from CorrectedSim3).
 *   2. Loop-connection edges (:7030-7058): keys = the distinct window slots in
 *      range, in address order; each key's row in its order.  The pair (i, j)
 *      is skipped iff !(i == cur_slot && j == loop_slot) and GetWeight(i, j) <
 *      PLVI_EG_MIN_FEAT (the map rows, 0 if absent); an entry outside [0,
 *      kf_cap) is skipped.  Otherwise edge LOOPCONN (i, j), and the unordered
 *      pair counts as inserted.
 *   3. Normal edges, for every member i of vpKFs in order -- a bad one too
 *      (:7068 has no isBad()).  parent, loop and prev_kf entries outside [0,
 *      kf_cap) are read as NULL.
 *      7DOF: TREE (i, parent); LOOP (i, l) for l in i's loop row in order with
 *        kf_id[l] < kf_id[i]; COVIS (i, n) for n in the prefix of i's ordered
 *        row with weight >= PLVI_EG_MIN_FEAT (the rule of
 *        plvi_covis_by_weight_batch) in order, with n in range, n != parent,
 *        not a child of i, not in i's loop row, not bad, kf_id[n] < kf_id[i]
 *        and the pair not inserted; INERTIAL (i, prev_kf) if imu[i].
 *      4DOF: no TREE edge and no parent test (pParentKF is a literal NULL,
 *        :14545); INERTIAL (i, prev_kf) first, without the imu test; then
 *        LOOP; then COVIS with the extra tests n != prev_kf[i] and n !=
 *        next_kf[i].
 *   4. edge_a is vertex 0 (i), edge_b vertex 1.  n_edges [5] counts by kind;
 *      the edge list is their sum long.  PLVI_EG_ERR_NO_VERTEX is set when an
 *      emitted edge names a slot that is not a vertex (bad, or outside vpKFs:
 *      the reference hands g2o a null vertex); the edge is emitted all the
 *      same.
 *   5. pt_ref [mp->n] / ln_ref [ml->n] (optional; :7235-7301): -1 for a bad
 *      feature or one outside map M; else, in 7DOF, corr_by[id] ==
 *      kf_id[cur_slot] ? corr_ref[id] : ref_kf[id]; in 4DOF ref_kf[id].
 *
 * Outputs follow the count contract: every count is a full length, nothing is
 * written at or past a capacity, err is written by every call.
 *
 * Limits.  cand_stride and win_cap <= PLVI_EG_MAX_WIN - 1 resp.
 * PLVI_EG_MAX_WIN (the window is sorted in LDS), PLVI_EG_MAX_WIN * max(kp_cap,
 * kl_cap) <= PLVI_LOCAL_MAP_MAX_ENTRIES, kf_cap <= 2^24, n_order <= 2^30;
 * PLVI_E_CAPACITY beyond.  No bound on kf_cap from LDS, none on the pools. */
#define PLVI_EG_MAX_WIN (PLVI_COVIS_MAX_CONN + 1) /* longest window */
#define PLVI_EG_MIN_FEAT 100                      /* minFeat of Optimizer.cc:6982 / :14440 */
enum { /* mode */
  PLVI_EG_7DOF = 0, /* OptimizeEssentialGraph */
  PLVI_EG_4DOF = 1, /* OptimizeEssentialGraph4DoF */
};
enum { /* edge_kind, and the index into n_edges */
  PLVI_EG_EDGE_LOOPCONN = 0,
  PLVI_EG_EDGE_TREE = 1,
  PLVI_EG_EDGE_LOOP = 2,
  PLVI_EG_EDGE_COVIS = 3,
  PLVI_EG_EDGE_INERTIAL = 4,
};
enum { /* err, bits */
  PLVI_EG_ERR_WIN = 1,        /* the window is longer than win_cap */
  PLVI_EG_ERR_PTS = 2,        /* the point list is longer than pt_cap */
  PLVI_EG_ERR_LNS = 4,        /* the line list is longer than ln_cap */
  PLVI_EG_ERR_QUERY = 8,      /* cur_slot (or loop_slot) outside [0, kf_cap): every count is 0, nothing else written */
  PLVI_EG_ERR_VERT = 16,      /* more vertices than vert_cap */
  PLVI_EG_ERR_EDGE = 32,      /* more edges than edge_cap */
  PLVI_EG_ERR_NO_VERTEX = 64, /* an emitted edge names a slot that is not a vertex */
  PLVI_EG_ERR_LC = 128,       /* a row of LoopConnections is longer than lc_cap */
};

/* The keyframe side besides plvi_cull_keyframes, by slot. */
typedef struct plvi_eg_keyframes {
  int n_order;          /* entries of order */
  int map_stride;       /* row length of map_kf / map_w */
  const int* order;     /* [n_order] the occupied slots in ascending address, as in plvi_covis_keyframes */
  const int* map_id;    /* [kf_cap] GetMap() as an id; NULL = one map */
  const int* parent;    /* [kf_cap] GetParent() or -1; NULL = none */
  const int* child_off; /* [kf_cap + 1] CSR of GetChilds(), membership only; NULL (both) = none */
  const int* child;
  const int* loop_off;  /* [kf_cap + 1] CSR of GetLoopEdges() in std::set<KeyFrame*> order; NULL (both) = none */
  const int* loop;
  const uint8_t* imu;   /* [kf_cap] bImu; NULL = 0 */
  const int* cand_w;    /* [kf_cap][cand_stride] mvOrderedWeights: d_ord_w of plvi_covis_rows in place */
  const int* map_kf;    /* [kf_cap][map_stride] the keys of mConnectedKeyFrameWeights, unsorted: */
  const int* map_w;     /* [kf_cap][map_stride] plvi_covis_map_rows in place */
  const int* map_n;     /* [kf_cap] */
} plvi_eg_keyframes;

/* One per pool, by id. */
typedef struct plvi_eg_features {
  const int* ref_kf;  /* [n] GetReferenceKeyFrame() as a slot */
  unsigned* corr_by;  /* [n] mnCorrectedByKF, in/out */
  int* corr_ref;      /* [n] mnCorrectedReference as a slot, in/out; required with corr_by */
  const int* map_id;  /* [n] GetMap() as an id; NULL = one map */
} plvi_eg_features;

typedef struct plvi_loop_correct_outputs {
  int win_cap, pt_cap, ln_cap;
  int* win;        /* [win_cap] mvpCurrentConnectedKFs as slots */
  int* n_win;      /* [1] */
  int* win_sorted; /* [win_cap] the distinct members in range, in address order */
  int* n_sorted;   /* [1] */
  int* pts;        /* [pt_cap] the MapPoints corrected, in traversal order */
  int* pts_kf;     /* [pt_cap] the member that corrects each */
  int* n_pts;      /* [1] */
  int* lns;        /* [ln_cap] */
  int* lns_kf;     /* [ln_cap] */
  int* n_lns;      /* [1]; 0 without lines */
  int* err;        /* [1] PLVI_EG_ERR_* */
} plvi_loop_correct_outputs;

typedef struct plvi_eg_outputs {
  int vert_cap, edge_cap;
  int* vert;       /* [vert_cap] slots */
  int* vert_flags; /* [vert_cap] bit 0 fixed, bit 1 window member */
  int* n_vert;     /* [1] */
  int* edge_a;     /* [edge_cap] vertex 0 */
  int* edge_b;     /* [edge_cap] vertex 1 */
  int* edge_kind;  /* [edge_cap] PLVI_EG_EDGE_* */
  int* n_edges;    /* [5] by kind */
  int* pt_ref;     /* [mp->n]; may be NULL; needs fmp */
  int* ln_ref;     /* [ml->n]; may be NULL; needs ml and fml */
  int* err;        /* [1] PLVI_EG_ERR_* */
} plvi_eg_outputs;

/* Bytes of the scratch blocks: a rank table by slot plus, for the correction,
 * a first-occurrence table by pool id; for the graph, the last window
 * position by slot, two counts per entry of order and a flag per cell of
 * lc_kf.  0 for a negative argument. */
size_t plvi_loop_correct_scratch_bytes(int kf_cap, int mp_n, int ml_n);
size_t plvi_essential_graph_scratch_bytes(int kf_cap, int n_order, int win_cap, int lc_cap);

/* The device forms.  The structs are host memory, read before the call
 * returns; their pointers are device pointers.  PLVI_E_BADARG for a negative
 * size, a missing required pointer (everything not marked optional; a list
 * with capacity 0 may be NULL), a CSR given in part, corr_by without corr_ref,
 * an unknown mode or a scratch block below its size.  d_scratch needs no
 * initialisation; calls that share it must be ordered.  Asynchronous on
 * `stream`, no host read of device data, no allocation: capturable.
 * plvi_loop_correct_device reads of eg only order / n_order.  One 1024-thread
 * workgroup walks the window; the normal edges run a wave per entry of
 * order. */
int plvi_loop_correct_device(int cur_slot, const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                             const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                             const plvi_eg_features* fmp, const plvi_eg_features* fml,
                             const plvi_loop_correct_outputs* out, void* d_scratch, size_t scratch_bytes,
                             void* stream);
int plvi_essential_graph_device(int cur_slot, int loop_slot, int mode, const int* d_win, const int* d_n_win,
                                int win_cap, const int* d_lc_kf, const int* d_n_lc, int lc_cap,
                                const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                                const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                const plvi_eg_features* fmp, const plvi_eg_features* fml, const plvi_eg_outputs* out,
                                void* d_scratch, size_t scratch_bytes, void* stream);

/* LoopConnections (:1406-1424) on a covisibility graph, between the two calls
 * above.  win [n_win] is host memory in both forms (the caller has it: it
 * computes a pose per member).  For each window position p in order whose
 * slot is in range: the slot's ordered row is copied to scratch row p
 * (vpPreviousNeighbors: it sees the updates of the positions before p), then
 * plvi_covis_update_batch runs for that one query with its outputs at index p
 * of `out` (arrays of n_win entries; the cells of a position that names no
 * slot are not written).  After the last position, per position:
 *   lc_kf[p] = the keys of the slot's weight map minus scratch row p minus
 *   every window member, in address order (kf->order); n_lc[p] its full
 *   length, 0 for a position that names no slot.
 * Taking the keys after the last update is exact: an update rewrites the map
 * of its own keyframe only, from a counter that does not depend on connection
 * state, and otherwise adds the updated keyframe -- a window member, erased
 * anyway -- to other maps.  d_err [1] has PLVI_EG_ERR_LC when a row is longer
 * than lc_cap; the graph's own overflow is out->err[p].  A slot at two
 * positions gets two rows.  kf / mp / ml / out as for
 * plvi_covis_update_batch; n_win <= PLVI_EG_MAX_WIN.  The scratch block is
 * plvi_covis_scratch_bytes(1, kf_cap) plus a rank table, the window and the
 * snapshot rows.  The device form is capturable like the batch call. */
size_t plvi_loop_connections_scratch_bytes(int n_win, int kf_cap, int conn_cap);
int plvi_loop_connections_device(plvi_covis_graph* h, int n_win, const int* win, const plvi_covis_keyframes* kf,
                                 const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                 const plvi_covis_outputs* out, int lc_cap, int* d_lc_kf, int* d_n_lc, int* d_err,
                                 void* d_scratch, size_t scratch_bytes, void* stream);
/* ... from host tables, synchronous: first_conn, parent and covis are updated
 * in place.  Returns 0, PLVI_E_CAPACITY when err[0] != 0, or another error. */
int plvi_loop_connections(plvi_covis_graph* h, int n_win, const int* win, const plvi_covis_keyframes* kf,
                          const plvi_local_map_pool* mp, const plvi_local_map_pool* ml, const plvi_covis_outputs* out,
                          int lc_cap, int* lc_kf, int* n_lc, int* err);

/* The host forms, synchronous: the same structs and arrays with host pointers
 * (corr_by / corr_ref are updated in place).  Return 0, PLVI_E_CAPACITY when
 * err has a bit other than PLVI_EG_ERR_NO_VERTEX (everything is still
 * written), or another error. */
int plvi_loop_correct(int cur_slot, const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                      const plvi_local_map_pool* mp, const plvi_local_map_pool* ml, const plvi_eg_features* fmp,
                      const plvi_eg_features* fml, const plvi_loop_correct_outputs* out);
int plvi_essential_graph(int cur_slot, int loop_slot, int mode, const int* win, const int* n_win, int win_cap,
                         const int* lc_kf, const int* n_lc, int lc_cap, const plvi_cull_keyframes* kf,
                         const plvi_eg_keyframes* eg, const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                         const plvi_eg_features* fmp, const plvi_eg_features* fml, const plvi_eg_outputs* out);

/* --------------------------------------------------------- Feature refresh
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:427-494) and
 * MapLine::UpdateNormalAndDepth (src/MapLine.cc:339-382) for NLeft == -1
 * (leftIndex always valid, rightIndex always -1), and
 * ComputeDistinctiveDescriptors (plvi_distinctive_descriptors_batch above)
 * fed from resident tables: the pair the reference calls back to back after
 * local BA, SearchInNeighbors, CreateNewMapPoints, Replace, CorrectLoop and
 * global BA.  The columns normal / dist / desc of plvi_local_map_pool are
 * updated in place at the rows a list of pool ids names, so a resident map
 * needs no host walk between a traversal (local_feat of plvi_ba_window, pts /
 * lns of plvi_loop_correct, the targets of Fuse) and the next frustum test.
 *
 * One implementation serves both kinds (params->kind).  what is a mask of
 * PLVI_REFRESH_NORMAL and PLVI_REFRESH_DESC.
 *
 * NORMAL, per id (state bit 0):
 *  1. a bad feature returns.  The list is obs_off[id+1] - obs_off[id] clamped
 *     to [0, max_obs]; entries whose obs_kf is outside [0, kf_cap) are ignored;
 *     a list with no entry left returns (observations.empty()).  The row is
 *     left alone.
 *  2. Pos: pos[id] for points; for lines the midpoint of sep[id] in double,
 *     an add then a multiply by 0.5, then (float) (Converter::toCvMat).
 *  3. for each observer in list order -- bad keyframes are NOT skipped, the
 *     reference's loop has no isBad():
 *       normali = Pos - ow[kf]            one float subtract per component
 *       s       = cv::norm(normali)       exact float squares summed in double, sqrt
 *       alpha   = (float)(1.0 / s)
 *       normal  = normali * alpha + normal   per component (see below)
 *  4. n = the observers counted; normal * (float)(1.0 / (double)n).
 *  5. dist = (float)cv::norm(Pos - ow[ref_kf]).
 *  6. level: points, the octave info[ref_kf][idx], idx the obs_idx of ref_kf's
 *     entry in the list -- or 0 when ref_kf is not in the list
 *     (observations[pRefKF] default-constructs the tuple: the octave of
 *     keypoint 0); lines, 0 (MapLine.cc:373).
 *  7. mfMaxDistance = dist * scale[level]; mfMinDistance = mfMaxDistance /
 *     scale[n_levels - 1]; dist[id] = {min, max}.
 * Precondition failures: the row is left alone, the state is 0 and one err bit
 * is raised: ref_kf outside [0, kf_cap) (ERR_REF), level >= n_levels
 * (ERR_LEVEL), idx outside [0, min(cnt[ref_kf], cap)) -- which includes
 * cnt[ref_kf] == 0 when ref_kf is not in the list (ERR_KEYPOINT; points only).
 * A keyframe must appear once per list (observations are map keys); of two
 * entries for ref_kf the first is taken.  The float sum of step 3 depends on
 * the list order in its last bits: the library takes the caller's order
 * (INTEGRATION.md).
 *
 * What the reference objects pin (tests/test_ref_objects_feature_refresh.py):
 * the calls operator-(Mat, Mat), cv::norm, operator/(Mat, double),
 * operator+(Mat const&, MatExpr const&); the double add and multiply of the
 * midpoint; cvtsi2sd of n ahead of operator/; cvtsd2ss behind cv::norm; the
 * mulss and divss of step 7; no fused instruction in either function.
 * Parity unpinned: OpenCV's own arithmetic inside those calls.  cv::norm and
 * the elementwise subtract are taken as the frustum tests take them.
 * normal + normali / s is taken as MatOp_AddEx resolving to
 * scaleAdd(normali, 1/s, normal): alpha narrowed to float, then
 * src * alpha + acc per element in the scalar tail of a 3-element row.  An
 * AVX2-dispatched OpenCV contracts that tail to a fused multiply-add, the
 * baseline does not: PLVI_COMPAT_SCALEADD_FMA (params->compat) selects
 * fma(normali, alpha, normal); 0 is the unfused form.  normal / n goes through
 * convertTo with a zero offset, which contraction cannot change.
 *
 * DESC, per id (state bit 1): the function of
 * plvi_distinctive_descriptors_batch on the list of step 1 (a bad feature has
 * an empty list), where an entry is ignored when its keyframe is out of
 * range or bad (MapPoint.cc:349) or its obs_idx is outside
 * [0, min(cnt[kf], cap)); the pool row is kf * cap + obs_idx of kf->desc.  A
 * CSR over the ids (every list at its clamped length, ignored entries as row
 * -1, so best_pos counts them as f19 does) is built in scratch, the public
 * batch call runs on it, and row id of desc is written where best_pos >= 0.
 * n_rows is the full length of that CSR; when it exceeds row_cap,
 * PLVI_REFRESH_ERR_ROWS is raised, no descriptor is written and best_pos is
 * -1 for every id.  NORMAL is unaffected.
 *
 * Outputs by id position i: state[i] is always written (0 for an id outside
 * [0, n)); best_pos / best_median are written when DESC is in what.
 * Duplicate ids are allowed: both writers store the same values.  n_rows and
 * err are written by every call (n_rows = 0 without DESC).
 *
 * Lists of up to 8 / 16 / 32 entries (by max_obs) share a wave in groups of
 * that many lanes: a lane per observer for the gather, the reciprocal norm and
 * the product, then the group adds in list order.  A longer list is walked by
 * its group 32 entries at a time.  kf_cap * cap and n_ids * max_obs must fit
 * an int (PLVI_E_CAPACITY). */
enum { /* plvi_refresh_params.kind */
  PLVI_REFRESH_POINTS = 0,
  PLVI_REFRESH_LINES = 1,
};
enum { /* plvi_refresh_params.what, and the bits of state */
  PLVI_REFRESH_NORMAL = 1,
  PLVI_REFRESH_DESC = 2,
};
enum { /* err, bits */
  PLVI_REFRESH_ERR_ROWS = 1,     /* n_rows > row_cap: no descriptor written */
  PLVI_REFRESH_ERR_REF = 2,      /* a ref_kf outside [0, kf_cap) */
  PLVI_REFRESH_ERR_LEVEL = 4,    /* an octave >= n_levels */
  PLVI_REFRESH_ERR_KEYPOINT = 8, /* ref_kf's keypoint index outside its table (cnt 0 in the absent case) */
};
#define PLVI_REFRESH_MAX_LEVELS 64

/* The keyframe side of one kind, by slot. */
typedef struct plvi_refresh_keyframes {
  int kf_cap;
  int cap;             /* row length of info / desc: kp_cap or kl_cap */
  const uint8_t* bad;  /* [kf_cap] isBad() */
  const float* ow;     /* [kf_cap][3] GetCameraCenter() */
  const int* cnt;      /* [kf_cap] N or N_l, read as clamped to [0, cap] */
  const uint8_t* info; /* [kf_cap][cap] bits 0-5 the octave: kp_info / kl_info in place; points only */
  const uint8_t* desc; /* [kf_cap][cap][32] mDescriptors / mDescriptors_Line; DESC only */
} plvi_refresh_keyframes;

/* Host struct, read before the call returns. */
typedef struct plvi_refresh_params {
  int kind;     /* PLVI_REFRESH_POINTS / LINES */
  int what;     /* PLVI_REFRESH_NORMAL | PLVI_REFRESH_DESC */
  int n_levels; /* mnScaleLevels / mnScaleLevels_l, 1 .. PLVI_REFRESH_MAX_LEVELS */
  int max_obs;  /* <= PLVI_DISTINCTIVE_MAX_OBS */
  int row_cap;  /* rows of the scratch CSR; DESC only */
  int compat;   /* PLVI_COMPAT_SCALEADD_FMA */
  float scale[PLVI_REFRESH_MAX_LEVELS]; /* mvScaleFactors / mvScaleFactors_l */
} plvi_refresh_params;

typedef struct plvi_refresh_outputs {
  float* normal;    /* [n][3] in place; may be the pool's own column; NULL without NORMAL */
  float* dist;      /* [n][2] likewise */
  uint8_t* desc;    /* [n][32] likewise; NULL without DESC; 4-byte aligned */
  uint8_t* state;   /* [n_ids] */
  int* best_pos;    /* [n_ids] optional */
  int* best_median; /* [n_ids] optional */
  int* n_rows;      /* [1] */
  int* err;         /* [1] PLVI_REFRESH_ERR_* */
} plvi_refresh_outputs;

/* Bytes of the scratch block: the CSR, best_pos / best_median and the chosen
 * rows.  0 for a negative argument. */
size_t plvi_feature_refresh_scratch_bytes(int n_ids, int row_cap);

/* The device form: the structs are host memory read before the call returns,
 * their pointers device pointers.  pool is read for n, bad, obs_off, obs_kf
 * and pos (points) or sep (lines); feat for obs_idx; ref for ref_kf.
 * PLVI_E_BADARG for a negative size, a missing pointer its kind and what
 * need, an unknown kind, a what of 0 or with other bits, n_levels outside
 * its range or a scratch block below its size; PLVI_E_CAPACITY for max_obs
 * above PLVI_DISTINCTIVE_MAX_OBS.  n_ids == 0 writes n_rows and err only.
 * d_scratch needs no initialisation; calls that share it must be ordered.
 * Asynchronous on `stream`, no host read of device data, no allocation:
 * capturable. */
int plvi_feature_refresh_batch(const plvi_refresh_keyframes* kf, const plvi_local_map_pool* pool,
                               const plvi_ba_features* feat, const plvi_eg_features* ref,
                               const plvi_refresh_params* params, const int* d_ids, int n_ids,
                               const plvi_refresh_outputs* out, void* d_scratch, size_t scratch_bytes, void* stream);

/* The host form, synchronous: the same structs and arrays with host pointers;
 * normal / dist / desc are updated in place.  Returns the number of ids with
 * the NORMAL bit set, PLVI_E_CAPACITY when err != 0 (everything is still
 * written), or another error. */
int plvi_feature_refresh(const plvi_refresh_keyframes* kf, const plvi_local_map_pool* pool,
                         const plvi_ba_features* feat, const plvi_eg_features* ref,
                         const plvi_refresh_params* params, const int* ids, int n_ids,
                         const plvi_refresh_outputs* out);

/* --------------------------------------------------------- GBA propagation
 * The second half of LoopClosing::RunGlobalBundleAdjustment[WithLines]
 * (src/LoopClosing.cc:3727-3930 and the line twin from :3996), once the
 * solver has returned: the breadth-first walk of the spanning tree from the
 * map's origin keyframes (plvi_gba_walk) and the pass over every MapPoint and
 * MapLine of the map (plvi_gba_correct).  The walk is integers only.  Every
 * 4x4 pose product, the velocity and the bias, SetPose, the solver and
 * InformNewBigChange stay with the caller (INTEGRATION.md has the sequence).
 * One-camera keyframes.
 *
 * plvi_gba_walk (:3727-3843).  plvi_cull_keyframes is read for kf_cap and
 * bad; plvi_eg_keyframes for order / n_order and child_off / child (NULL,
 * both = no children).  The child rows carry membership only; the call sorts
 * them.  origins [n_origins] are slots (mvpKeyFrameOrigins in vector order),
 * loop_kf is nLoopKF, kf_ba_for [kf_cap] is mnBAGlobalForKF, in/out.
 *   1. The queue starts as origins in the order given.  An origin outside
 *      [0, kf_cap) is left out and raises PLVI_GBA_ERR_ORIGIN.  An origin is
 *      not tested for bad or for its stamp, and is not stamped (:3731).
 *   2. The front entry's child row is taken in address order: ascending rank,
 *      the rank of a slot being its first position in `order`, n_order + slot
 *      for a slot that order does not name.  A child outside [0, kf_cap) or
 *      bad is skipped with everything below it (:3741).  A child whose stamp
 *      is not loop_kf is stamped and flagged new (:3744-3768): the caller owes
 *      it Tchildc * parent.mTcwGBA, the velocity and the bias.  Every child
 *      not skipped is appended, new or not (:3769).
 *   3. Every queue entry is a keyframe whose mTcwBefGBA / SetPose the caller
 *      replays (:3773-3775).
 * walk [walk_cap] is the queue in order, walk_parent the slot whose row
 * queued each entry (-1 for an origin), walk_new 0 / 1.  A parent stands
 * before its children, so one pass over the list computes the new poses.
 * n_walk, n_new and err are written by every call; n_walk is a full length
 * under the count contract: nothing is written at or past walk_cap, and
 * n_walk > walk_cap raises PLVI_GBA_ERR_WALK.  The stamps are state, as in
 * plvi_loop_correct: every visited child is stamped whatever walk_cap is.
 * visited [kf_cap] (optional) gets a 1 for every queue entry and is not
 * cleared: the !mTcwBefGBA.empty() the correction needs after a first GBA.
 *
 * Precondition: the child CSR is a forest -- no slot in two rows, no origin
 * in a row, no origin twice.  The queue is kf_cap entries of scratch.  Tables
 * that are no forest are still walked as the reference's loop walks them (a
 * child met twice is new at its first queue position only) for as long as
 * the queue holds; when the tail would pass kf_cap the walk stops and
 * PLVI_GBA_ERR_CYCLE is raised -- the reference would not terminate or would
 * visit more than kf_cap entries -- and the outputs are unspecified but
 * inside their arrays.  A child row that does not lie inside the first kf_cap
 * entries of child (a forest has fewer) is read as empty and raises the same
 * bit.  Limits as for the essential graph: kf_cap <= 2^24, n_order <= 2^30,
 * PLVI_E_CAPACITY beyond.
 *
 * plvi_gba_correct (:3847-3884 points, :3887-3930 lines; params->kind).  The
 * pool is read for n, bad and pos (points) or sep (lines); feat for ref_kf
 * and map_id; feat_ba_for [n] is the feature's mnBAGlobalForKF; pos_gba is
 * mPosGBA, [n][3] float for points, [n][6] double for lines.  Per pool id:
 *   state 0  a bad feature, or one whose map_id is not params->map
 *            (GetAllMapPoints of the active map): the row is left alone.
 *   state 1  feat_ba_for[id] == loop_kf: the row becomes pos_gba[id], a bit
 *            copy (:3856-3860).
 *   else r = ref_kf[id].  r outside [0, kf_cap): state 0 and
 *            PLVI_GBA_ERR_REF (the reference would dereference NULL).
 *            kf_ba_for[r] != loop_kf or !has_bef[r]: state 0 (:3866-3870).
 *            bad[r] is not tested: the reference has no isBad() there.
 *   state 2  Xc = Rcw_bef * X + tcw_bef, X' = Rwc * Xc + twc (:3873-3882).
 *            Lines: each endpoint narrowed to float (Converter::toCvMat),
 *            the same two products, the result widened to double
 *            (Converter::toVector3d).
 * Each of the six rows is cv::Mat R * X + t in the form the frustum tests
 * take for Rcw * P + tcw: float products and sums in cv::gemm's small-matrix
 * order, contracted with PLVI_COMPAT_GEMM_FMA (params->compat), then
 * (float)((double)s + (double)t).  What pins it:
 * tests/test_ref_objects_gba_propagate.py.  The output column may be the
 * array the pool names as const.  state [n] is written for every id, counts
 * [3] by state and err by every call. */
enum { /* plvi_gba_params.kind */
  PLVI_GBA_POINTS = 0,
  PLVI_GBA_LINES = 1,
};
enum { /* err, bits */
  PLVI_GBA_ERR_ORIGIN = 1, /* an origin outside [0, kf_cap): left out */
  PLVI_GBA_ERR_CYCLE = 2,  /* the child CSR is not a forest: the walk stopped at kf_cap queue entries */
  PLVI_GBA_ERR_WALK = 4,   /* n_walk > walk_cap */
  PLVI_GBA_ERR_REF = 8,    /* a ref_kf outside [0, kf_cap) */
};

typedef struct plvi_gba_walk_outputs {
  int walk_cap;
  int* walk;         /* [walk_cap] slots in queue order */
  int* walk_parent;  /* [walk_cap] the slot whose row queued the entry; -1 for an origin */
  uint8_t* walk_new; /* [walk_cap] 1 = stamped by this call */
  int* n_walk;       /* [1] */
  int* n_new;        /* [1] */
  int* err;          /* [1] PLVI_GBA_ERR_* */
  uint8_t* visited;  /* [kf_cap] optional; 1 for every queue entry, otherwise untouched */
} plvi_gba_walk_outputs;

/* The keyframe side of the correction, by slot.  A pose is 12 floats: the
 * nine entries of R row-major, then t. */
typedef struct plvi_gba_poses {
  int kf_cap;
  const unsigned* kf_ba_for; /* [kf_cap] mnBAGlobalForKF after the walk */
  const uint8_t* has_bef;    /* [kf_cap] !mTcwBefGBA.empty() */
  const float* tcw_bef;      /* [kf_cap][12] mTcwBefGBA */
  const float* twc;          /* [kf_cap][12] GetPoseInverse() after SetPose */
} plvi_gba_poses;

/* Host struct, read before the call returns. */
typedef struct plvi_gba_params {
  int kind;         /* PLVI_GBA_POINTS / LINES */
  unsigned loop_kf; /* nLoopKF */
  int map;          /* the active map's id, compared with feat->map_id (NULL = one map) */
  int compat;       /* PLVI_COMPAT_GEMM_FMA */
} plvi_gba_params;

typedef struct plvi_gba_correct_outputs {
  float* pos;     /* [n][3] points: may be the pool's own column */
  double* sep;    /* [n][6] lines: likewise */
  uint8_t* state; /* [n] 0 left alone, 1 the solver's position, 2 carried by the reference keyframe */
  int* counts;    /* [3] by state */
  int* err;       /* [1] PLVI_GBA_ERR_REF */
} plvi_gba_correct_outputs;

/* Bytes of the walk's scratch block: the rank table, the first queue
 * position, the usable count and the sorted rows by slot, and the queue.  0
 * for a negative argument. */
size_t plvi_gba_walk_scratch_bytes(int kf_cap);

/* The device forms.  The structs are host memory, read before the call
 * returns; their pointers are device pointers.  PLVI_E_BADARG for a negative
 * size, kf_cap < 1, a missing required pointer (a list with capacity 0 may be
 * NULL), a CSR given in part, an unknown kind or a scratch block below its
 * size.  d_scratch needs no initialisation; calls that share it must be
 * ordered.  Asynchronous on `stream`, no host read of device data, no
 * allocation, the counters reset by memset nodes: capturable.  A wave per
 * slot sorts the rows, then one 1024-thread workgroup walks the queue up to
 * 1024 entries a step (one wave alone while the frontier fits it); the
 * correction runs a thread per pool id. */
int plvi_gba_walk_device(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg, const int* d_origins,
                         int n_origins, unsigned loop_kf, unsigned* d_kf_ba_for, const plvi_gba_walk_outputs* out,
                         void* d_scratch, size_t scratch_bytes, void* stream);
int plvi_gba_correct_device(const plvi_local_map_pool* pool, const plvi_eg_features* feat,
                            const unsigned* d_feat_ba_for, const void* d_pos_gba, const plvi_gba_poses* poses,
                            const plvi_gba_params* params, const plvi_gba_correct_outputs* out, void* stream);

/* The host forms, synchronous: the same structs and arrays with host
 * pointers; kf_ba_for, visited and the output column are updated in place.
 * plvi_gba_walk returns n_walk, plvi_gba_correct the number of rows written
 * (states 1 and 2); PLVI_E_CAPACITY when err != 0 (everything is still
 * written), or another error. */
int plvi_gba_walk(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg, const int* origins, int n_origins,
                  unsigned loop_kf, unsigned* kf_ba_for, const plvi_gba_walk_outputs* out);
int plvi_gba_correct(const plvi_local_map_pool* pool, const plvi_eg_features* feat, const unsigned* feat_ba_for,
                     const void* pos_gba, const plvi_gba_poses* poses, const plvi_gba_params* params,
                     const plvi_gba_correct_outputs* out);

/* ---------------------------------------------------------------- Stereo
 * Rectified stereo of the stereo Frame constructors (src/Frame.cc:95-140,
 * :225-300). */

/* Frame::ComputeStereoMatches (src/Frame.cc:1228-1406) for n_frames pairs
 * extracted by two ORB handles of the same geometry (mpORBextractorLeft /
 * Right, vLappingArea {0,0}): keypoints, descriptors and mvImagePyramid are
 * read on the device.  mb / mbf: Frame::mb, mbf.  Outputs mvuRight /
 * mvDepth [n_frames][cap] (cap of plvi_orb_outputs, -1 = no depth),
 * d_nstereo [n_frames] = left keypoints with a depth; *d_err |= 1 when a
 * right keypoint's row band leaves the image (the reference indexes
 * vRowIndices out of range), |= 2 when an SAD window leaves its level (the
 * reference's rowRange/colRange assert).  The counts are the handles' own
 * (at most cap); the kernel clamps them to cap like every count of the count
 * contract (plvi_hamming_knn2_batch).  Asynchronous on `stream`. */
int plvi_stereo_match_batch(plvi_orb_extractor* left, plvi_orb_extractor* right, int n_frames, float mb, float mbf,
                            float* d_uright, float* d_depth, int* d_nstereo, int* d_err, void* stream);

/* One pair from host memory, synchronous.  Pyramids: level l of each side
 * at pyr + lvl_off[l], lvl_w[l] x lvl_h[l] (row stride lvl_w[l]); scale /
 * inv_scale = mvScaleFactors / mvInvScaleFactors.  Returns the number of
 * left keypoints with a depth, or an error (PLVI_E_OVERFLOW for the
 * reference's out-of-range cases above). */
int plvi_stereo_match(const plvi_keypoint* kpsL, const uint8_t* descL, int nL, const plvi_keypoint* kpsR,
                      const uint8_t* descR, int nR, int nlevels, const float* scale, const float* inv_scale,
                      const uint8_t* pyrL, const uint8_t* pyrR, const long long* lvl_off, const int* lvl_w,
                      const int* lvl_h, float mb, float mbf, float* uright, float* depth);

/* Frame::ComputeStereoMatches_Lines (src/Frame.cc:1408-1492): GridStructure
 * of the right lines (getLineCoords, src/gridStructure.cpp:32-40), the
 * line_2d coordinates and directions, LineMatcher::matchGrid with the
 * stereo window {width (7,0), height (2,2)}, then the endpoint disparities
 * (lineSegmentOverlapStereo :1494-1529, filterLineSegmentDisparity
 * :1531-1542) and mvle_l from mvKeysUn_Line (d_klUn; NULL = the left
 * keylines).  Per pair p: keylines/descriptors at p*cap, counts n[p].
 * Outputs matches_12 [n][capL], mvDisparity_l / mvDepth_l [n][capL][2]
 * floats (-1 = none), mvle_l [n][capL][3] doubles (0 when either side has
 * no lines, as the reference returns before computing it), d_nstereo [n].
 * d_scratch: plvi_stereo_lines_scratch_bytes(n, capL, capR, idx_cap) bytes;
 * idx_cap bounds the grid entries of one frame (*d_err |= 4 if exceeded).
 * d_nL / d_nR follow the count contract (plvi_hamming_knn2_batch).
 * Asynchronous on `stream`. */
size_t plvi_stereo_lines_scratch_bytes(int n_frames, int capL, int capR, int idx_cap);
int plvi_stereo_lines_batch(int n_frames, const plvi_keyline* d_klL, const uint8_t* d_descL, const int* d_nL, int capL,
                            const plvi_keyline* d_klR, const uint8_t* d_descR, const int* d_nR, int capR,
                            const plvi_keyline* d_klUn, int width, int height, float mbf, int libstdcxx_range_hint,
                            int idx_cap, void* d_scratch, size_t scratch_bytes, int* d_matches_12, float* d_disparity,
                            float* d_depth, double* d_le, int* d_nstereo, int* d_err, void* stream);

/* One pair from host memory, synchronous (n <= 2048 lines per side).
 * Returns the number of lines with a depth, or an error. */
int plvi_stereo_lines(const plvi_keyline* klL, const uint8_t* descL, int nL, const plvi_keyline* klR,
                      const uint8_t* descR, int nR, const plvi_keyline* klUn, int width, int height, float mbf,
                      int libstdcxx_range_hint, int* matches_12, float* disparity, float* depth, double* le);

/* ------------------------------------------------------------ Frame level
 * Frame::Frame's extraction (src/Frame.cc:537-641, ExtractORB/ExtractLine
 * :677-692): the ORB and line extractors on the same batch of frames, run
 * as one schedule (LSD prep, then region growing concurrent with the ORB
 * pipeline and the LBD Sobel pyramid on the handles' own streams).
 * Asynchronous with respect to `stream`, which it joins at the end; the
 * results are read with plvi_orb_outputs / plvi_lines_outputs. */
int plvi_frame_extract_batch(plvi_orb_extractor* orb, plvi_line_extractor* lines, const uint8_t* d_frames,
                             int n_frames, size_t frame_stride, size_t row_stride, int lap0, int lap1, void* stream);

/* plvi_frame_extract_batch followed by the step's matching of every frame t
 * in the batch against frame t-1: the ORB kNN-2 (plvi_hamming_knn2_batch of
 * descriptor rows t vs t-1: outputs [n_frames-1][orb cap]) issued on the
 * schedule's ORB stream as soon as the ORB extraction is done, and
 * LineMatcher::match (plvi_line_match_batch, nnr, scratch as there: outputs
 * [n_frames-1][line cap]) on the line path's stream right after the LBD
 * descriptors -- no join of the schedule's streams in between.  Joins
 * `stream` at the end.  n_frames >= 2. */
int plvi_frame_extract_match_batch(plvi_orb_extractor* orb, plvi_line_extractor* lines, const uint8_t* d_frames,
                                   int n_frames, size_t frame_stride, size_t row_stride, int lap0, int lap1,
                                   int* d_idx0, int* d_d0, int* d_idx1, int* d_d1, float nnr, int* d_line_scratch,
                                   int* d_line_matches, int* d_line_nmatch, void* stream);

/* The event the last plvi_frame_extract_batch on `lines` recorded once its
 * ORB extraction was complete (a hipEvent_t owned by the handle): work on the
 * ORB tables -- kNN-2 against the previous frame -- can wait on it
 * (plvi_stream_wait_event) and overlap the rest of the line path instead of
 * waiting for the whole frame.  After plvi_frame_extract_match_batch the same
 * event is recorded after the ORB kNN-2 as well (it then covers extraction
 * AND d_idx0/d_d0/d_idx1/d_d1).  The handle re-records it on its next
 * extract call: issue every wait on it before the next extract call on the
 * same handle, or the wait refers to the newer batch. */
int plvi_frame_orb_event(plvi_line_extractor* lines, void** event);

/* ------------------------------------------------------------ initialization
 * The monocular initializer's matchers, called on every frame until
 * Tracking::MonocularInitialization succeeds (src/Tracking.cc:3111-3113). */

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12,
 * windowSize) (src/ORBmatcher.cc:705-814). */
typedef struct plvi_init_params {
  float min_x, min_y, inv_w, inv_h; /* F2.mnMinX, mnMinY, mfGridElementWidthInv / HeightInv */
  int window;                       /* windowSize (100 in MonocularInitialization) */
  float nnratio;                    /* ORBmatcher(0.9, true): mfNNratio */
  int check_orientation;            /* mbCheckOrientation */
} plvi_init_params;

/* Batched over n_pairs (F1 = mInitialFrame, F2 = mCurrentFrame) pairs.
 * F1 p: keypoints (mvKeysUn) / descriptors [p][cap1] (counts d_n1) and
 * vbPrevMatched as float2 [p][cap1] (in/out: matched entries become
 * F2.mvKeysUn[vnMatches12[i1]].pt, as the reference updates them); F2 p:
 * keypoints / descriptors [p][cap2] (counts d_n2) and the grid CSR from
 * plvi_assign_grid_batch over the same keypoints.  Output vnMatches12
 * [p][cap1] (first n1 entries) and nmatches [p].  cap1, cap2 <= 65535 and
 * ~24 B per F1 + ~19 B per F2 keypoint + 12 KB of LDS <= 160 KB.
 * d_n1 / d_n2 follow the count contract (plvi_hamming_knn2_batch); rows of
 * vbPrevMatched at or past n1 keep their values.
 * Replaces ORBmatcher.h:71 (SearchForInitialization). */
int plvi_search_for_initialization_batch(int n_pairs, const plvi_init_params* p, const plvi_keypoint* d_kps1,
                                         const uint8_t* d_desc1, const int* d_n1, int cap1, float* d_prev_matched,
                                         const plvi_keypoint* d_kps2, const uint8_t* d_desc2, const int* d_n2,
                                         int cap2, const int* d_cell_off, const int* d_cell_idx, int* d_matches12,
                                         int* d_nmatches, void* stream);

/* LineMatcher::SerachForInitialize(InitialFrame, CurrentFrame, LineMatches)
 * (src/LineMatcher.cpp:113-139) with Frame::lineDescriptorMAD
 * (src/Frame.cc:1089-1112): knnMatch(k=2) of the initial frame's LBD
 * descriptors [p][cap1] (counts d_n1) against the current frame's [p][cap2],
 * then the pairs whose d1 - d0 exceeds 0.5 * nn12_mad.  Output LineMatches
 * as int2 (query, train) [p][cap1] in query order, their count [p], and
 * (nullable) {nn_mad, nn12_mad} as double [p][2].  d_scratch holds
 * 4 * n_pairs * cap1 ints.  The reference reads lmatches[0] and [i][1]:
 * with no query lines or fewer than 2 train lines it is undefined; here the
 * pair gets 0 matches.  d_n1 / d_n2 follow the count contract
 * (plvi_hamming_knn2_batch); pair rows at or past the pair count are not
 * written.  Replaces LineMatcher.h:95 (SerachForInitialize). */
int plvi_line_search_init_batch(const uint8_t* d_desc1, const int* d_n1, int cap1, const uint8_t* d_desc2,
                                const int* d_n2, int cap2, int n_pairs, int* d_scratch, int* d_pairs, int* d_npairs,
                                double* d_mad, void* stream);

/* The stereo-line Frame ctor (src/Frame.cc:200-249: ExtractORB left || right,
 * ExtractLine left || right): both sides' ORB + line extraction of a batch of
 * rectified pairs as two concurrent frame schedules (the right one forked
 * from `stream` onto lines_right's own stream and joined back).  Asynchronous
 * on `stream`; each handle keeps its side's results (plvi_orb_outputs /
 * plvi_lines_outputs), which plvi_stereo_match_batch and
 * plvi_stereo_lines_batch then read on the same stream.  Left and right
 * handles must be distinct. */
int plvi_stereo_frame_extract_batch(plvi_orb_extractor* orb_left, plvi_orb_extractor* orb_right,
                                    plvi_line_extractor* lines_left, plvi_line_extractor* lines_right,
                                    const uint8_t* d_left, const uint8_t* d_right, int n_frames, size_t frame_stride,
                                    size_t row_stride, int lap0, int lap1, void* stream);

/* ----------------------------------------------------------- triangulation
 * The candidate searches of LocalMapping::CreateNewMapPoints /
 * CreateNewMapLines, called once per covisible neighbour of every new
 * keyframe (src/LocalMapping.cc:804, :1135). */

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs,
 * bOnlyStereo, bCoarse) (src/ORBmatcher.cc:965-1206), the single-camera
 * branch: !pKF1->mpCamera2 && !pKF2->mpCamera2, NLeft == -1, Pinhole;
 * keypoints are mvKeysUn.  The constants of one (KF1, KF2) pair:
 *   F12   row-major 3x3.  Replaces the matrix Pinhole::epipolarConstrain
 *         (src/CameraModels/Pinhole.cpp:137-140) rebuilds for every
 *         candidate, K1.t().inv() * SkewSymmetricMatrix(t12) * R12 * K2.inv()
 *         with R12 = R1w*R2w.t() and t12 = -R1w*R2w.t()*t2w + t1w
 *         (ORBmatcher.cc:991-992): in this branch it is the same for every
 *         candidate, and it is built with cv::Mat::inv and cv::gemm, whose
 *         arithmetic is outside the reference tree.  (The F12 argument of
 *         the reference function itself is never read.)
 *   ep    the epipole in KF2, replaces pKF2->mpCamera->project(R2w*Cw + t2w)
 *         with Cw = pKF1->GetCameraCenter() (ORBmatcher.cc:972-977).
 *   sigma2 / scale_factors   pKF2->mvLevelSigma2 and pKF2->mvScaleFactors,
 *         indexed by kp2.octave (an octave outside [0, n) reads the nearest
 *         entry; n_* outside [1, 16] is clamped).
 * Everything downstream of these inputs is bit-exact with the reference
 * build: the epipolar line, num, den and dsqr in float with the reference
 * object's fused multiply-adds, the double compare dsqr < 3.84*unc, den == 0
 * rejecting, `|| bCoarse`, the epipole rejection (only when neither keypoint
 * is stereo) in float, TH_LOW = 50, last-wins among equal distances, the
 * rotation histogram and ComputeThreeMaxima; nmatches counts after the
 * histogram filter.
 * Out of scope: the KannalaBrandt8 / two-camera branch (:994-1003,
 * :1099-1129; its epipolarConstrain is TriangulateMatches with an OpenCV SVD,
 * VERDICT.md), the overload with vMatchedPoints (:1208) and SearchBySim3.
 * (Fuse is plvi_fuse_points / plvi_fuse_lines above.) */
typedef struct plvi_triangulation_pair {
  float F12[9];
  float ep[2];
  int n_sigma2;
  float sigma2[16];
  int n_scale_factors;
  float scale_factors[16];
  int only_stereo;       /* bOnlyStereo */
  int coarse;            /* bCoarse */
  int check_orientation; /* mbCheckOrientation */
} plvi_triangulation_pair;

/* Batched device variant, layout as plvi_search_by_bow_batch: pair p uses
 * rows p*cap1 / p*cap2 of the keypoint tables (kps, desc, has_point, uright
 * and the FeatureVector index list idx), p*node_cap (node ids, ascending)
 * and p*(node_cap+1) (offsets) of the CSR arrays, and d_pairs[p].
 * has_point[i] = GetMapPoint(i) != NULL (skipped on either side), uright =
 * mvuRight (>= 0: stereo).  A keypoint is in at most one node.  Outputs
 * matches12 [n_pairs][cap1] (vMatches12: KF2 index or -1) and nmatches
 * [n_pairs]; vMatchedPairs is the in-order compaction of matches12.
 * d_n1 / d_n2 follow the count contract (plvi_hamming_knn2_batch) against
 * cap1 / cap2 and the node counts against node_cap; an offset outside
 * [0, list length] is read as clamped and a list entry outside [0, n) is
 * ignored.  rows [0, n1) of matches12 are fully written.
 * The KF2 list is staged whole in LDS: 52*cap2 + 16*node_cap + 8 bytes, which
 * with the kernel's static data must fit the 160 KB of a CU (cap2 up to
 * ~3000); a larger table returns PLVI_E_CAPACITY and nothing is launched --
 * no pair is truncated.  Asynchronous on `stream`.
 * Replaces ORBmatcher.h:74 (SearchForTriangulation). */
int plvi_search_for_triangulation_batch(int n_pairs, const plvi_triangulation_pair* d_pairs, int cap1, int cap2,
                                        int node_cap, const plvi_keypoint* d_kps1, const uint8_t* d_desc1,
                                        const int* d_n1, const int* d_node1, const int* d_off1, const int* d_nnodes1,
                                        const int* d_idx1, const uint8_t* d_has_point1, const float* d_uright1,
                                        const plvi_keypoint* d_kps2, const uint8_t* d_desc2, const int* d_n2,
                                        const int* d_node2, const int* d_off2, const int* d_nnodes2,
                                        const int* d_idx2, const uint8_t* d_has_point2, const float* d_uright2,
                                        int* d_matches12, int* d_nmatches, void* stream);

/* Single pair from host memory, synchronous (like plvi_search_by_bow):
 * matches12 [n1]; returns nmatches (>= 0) or an error. */
int plvi_search_for_triangulation(const plvi_triangulation_pair* pair, const plvi_keypoint* kps1,
                                  const uint8_t* desc1, int n1, const int* node1, const int* off1, int nnodes1,
                                  const int* idx1, const uint8_t* has_point1, const float* uright1,
                                  const plvi_keypoint* kps2, const uint8_t* desc2, int n2, const int* node2,
                                  const int* off2, int nnodes2, const int* idx2, const uint8_t* has_point2,
                                  const float* uright2, int* matches12);

/* LineMatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs)
 * (src/LineMatcher.cpp:142-171): plvi_line_search_init_batch with the
 * threshold 0.1 * nn12_mad (pKF1->lineDescriptorMAD) and without the pairs
 * whose query line (d_has_line1 [p][cap1], pKF1->GetMapLine(qdx)) or train
 * line (d_has_line2 [p][cap2], pKF2->GetMapLine(tdx)) already has a MapLine.
 * The masks act after the MAD: a masked line still counts in nn12_mad.
 * Same tables, scratch (4 * n_pairs * cap1 ints), outputs, count contract
 * and 0 matches for n1 = 0 or n2 < 2 as plvi_line_search_init_batch.
 * Replaces LineMatcher.h:97 (SearchForTriangulation). */
int plvi_line_search_triangulation_batch(const uint8_t* d_desc1, const int* d_n1, int cap1, const uint8_t* d_desc2,
                                         const int* d_n2, int cap2, int n_pairs, const uint8_t* d_has_line1,
                                         const uint8_t* d_has_line2, int* d_scratch, int* d_pairs, int* d_npairs,
                                         double* d_mad, void* stream);

/* Device memory helpers for bindings that have no HIP runtime of their own
 * (ctypes, JNI): thin wrappers over hipMalloc/hipFree/hipMemcpy on the
 * current device.  kind: 1 = host->device, 2 = device->host, 3 = d->d. */
int plvi_device_malloc(void** ptr, size_t bytes);
int plvi_device_free(void* ptr);
int plvi_memcpy(void* dst, const void* src, size_t bytes, int kind);
/* Same, asynchronous on `stream` (hipStream_t). */
int plvi_memcpy_async(void* dst, const void* src, size_t bytes, int kind, void* stream);
int plvi_device_synchronize(void);
/* A non-blocking HIP stream (hipStreamCreateWithFlags(hipStreamNonBlocking))
 * for bindings without a HIP runtime of their own; destroy / synchronize. */
int plvi_stream_create(void** stream);
int plvi_stream_destroy(void* stream);
int plvi_stream_synchronize(void* stream);
/* Events for the same bindings (hipEventCreateWithFlags(hipEventDisableTiming),
 * hipEventRecord, hipStreamWaitEvent, hipEventDestroy). */
int plvi_event_create(void** event);
int plvi_event_record(void* event, void* stream);
int plvi_stream_wait_event(void* stream, void* event);
int plvi_event_destroy(void* event);

/* HIP graphs (no reference counterpart: a runtime facility of this
 * library).  plvi_graph_capture_begin starts capturing `stream` (a created
 * stream, not the null stream); every plvi_* call issued on it until
 * plvi_graph_capture_end is recorded, not run, including the work the
 * extractors fork to their own streams.  The captured step is instantiated
 * into *graph_exec and replayed by plvi_graph_launch with the same device
 * pointers and parameters; plvi_graph_destroy frees it.  The multi-stream
 * frame schedule (plvi_frame_extract_batch) needs HIP runtime >= 7.2 to be
 * captured (the 7.0 runtime crashes in hipStreamEndCapture on its
 * fork/join): on an older runtime it returns PLVI_E_CAPTURE while capturing. */
int plvi_graph_capture_begin(void* stream);
int plvi_graph_capture_end(void* stream, void** graph_exec);
int plvi_graph_launch(void* graph_exec, void* stream);
int plvi_graph_destroy(void* graph_exec);

/* Device/library information for diagnostics. */
const char* plvi_version(void);
int plvi_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* PLVI_FRONTEND_H */

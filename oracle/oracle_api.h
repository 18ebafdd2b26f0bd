// oracle/oracle_api.h — TEST INFRASTRUCTURE ONLY: C entry points of the CPU
// restatement (loaded by tests/ via ctypes).  Layouts mirror cv::KeyPoint
// (28 B) and line_descriptor::KeyLine; they are declared here independently
// of the product headers so the checker shares no code with the product.
#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } plvi_keypoint;
// One record per seed flsd visits (every region_grow call), in visiting order.
typedef struct { int32_t seed_x, seed_y, size, depth /* largest point row - seed row */, min_reg_size; } oracle_lsd_region;
// Region census of one image at the given LSD scale (lines_oracle.cpp): *n =
// records, written to recs[0 .. *n) when they fit cap (else -3 is returned).
int oracle_lsd_regions(const uint8_t* img, int w, int h, float lsd_scale, int32_t* recs /* cap x 5 */, int cap, int* n);
#ifdef __cplusplus
}
#endif

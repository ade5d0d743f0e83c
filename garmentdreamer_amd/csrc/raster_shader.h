// raster_shader.h -- what raster_shader.hip and raster_shader_mfma.hip share: the argument checks and the split of the
// caller's scratch (include/gd_shader.h, "scratch").
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gd {

constexpr size_t kShaderSlabFloats = 256 * 256 + 256;   // Op_l Kp_l + Op_l of the largest layer

int shader_capacity_ok(const char* what, int64_t capacity); // -1 with a message unless 1 <= capacity <= 2^24
int shader_null(const char* what);                          // -1, "null pointer"
size_t shader_align256(size_t x);

// the L1's partials come first in the scratch, the weight gradient's slabs behind them
inline size_t shader_l1_scratch_bytes(int64_t rows) { return (((size_t)rows + 255) / 256 * sizeof(float) + 255) & ~(size_t)255; }

}  // namespace gd

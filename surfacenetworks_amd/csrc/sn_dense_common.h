// sn_dense_common.h — what sn_dense.hip and sn_pair.hip share (internal: not part of the C interface).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f16v mfma_f16(const u4 &a, const u4 &b, const f16v &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8v, a), __builtin_bit_cast(h8v, b), c, 0, 0, 0);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

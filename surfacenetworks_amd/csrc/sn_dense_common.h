// sn_dense_common.h — what sn_dense.hip, sn_gemm.hip and sn_pair.hip share (internal: not part of the C interface).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;
#define kCUs sn_internal_cu_count()      // compute units of the current device (256 on an MI355X in SPX mode)

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef unsigned int u2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f16v mfma_f16(const u4 &a, const u4 &b, const f16v &c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8v, a), __builtin_bit_cast(h8v, b), c, 0, 0, 0);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// compile-time loop: f(IC<I>{}) for I in [I, N) — the index is a constant expression inside f
template <int I>
struct IC {
  static constexpr int value = I;
};
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(IC<I>{});
    static_for<I + 1, N>(f);
  }
}

// LDS writes of this wave done, then the workgroup barrier — without the vmcnt(0) a __syncthreads() fence would add
// (it would drain the global prefetch and wait for earlier stores to be acknowledged).
#define SN_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Exact power-of-two scales that bring a bound m = f·2^E, f in [0.5, 1), to [2^(T-1), 2^T): pow2_up<T> = 2^(T - E), pow2_down<T>
// its inverse from the same exponent, pow2_inv the inverse of any 2^k, k in [-115, 115].  (T = 14: rows and weight columns of
// the Linear kernels; T = 15: the operands of the two-piece weight gradient.)
__device__ __forceinline__ int pow2_exponent(float m) {
  const int e = (int)((__float_as_uint(m) >> 23) & 0xffu) - 126;
  return e < -100 ? -100 : (e > 100 ? 100 : e);           // zero / denormal / non-finite bounds: any finite scale will do
}
template <int T>
__device__ __forceinline__ float pow2_up(float m) { return __uint_as_float((unsigned)(127 + T - pow2_exponent(m)) << 23); }
template <int T>
__device__ __forceinline__ float pow2_down(float m) { return __uint_as_float((unsigned)(127 - T + pow2_exponent(m)) << 23); }
__device__ __forceinline__ float pow2_inv(float p) { return __uint_as_float((254u << 23) - __float_as_uint(p)); }

// SN_GEMM_VARIANT: default (unset / anything but 0) the 16-bit matrix-pipe kernels; 0 = the fp32-MFMA kernels, the ONE A/B
// baseline of the Linear kernels (exact fp32 products; no fused epilogues).  Read once per process, in sn_gemm_variant().
inline int gemm_variant() { return sn_gemm_variant(); }

// One kernel launch; with the timing facility on (both events set: sn_internal_timing_slot) the kernel's own start and stop
// are stamped into them.
template <class... P, class... A>
inline void launch_timed(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, hipEvent_t t_start, hipEvent_t t_stop,
                         A... args) {
  if (t_start) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, t_start, t_stop, 0, static_cast<P>(args)...);
  else hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<P>(args)...);
}

}  // namespace

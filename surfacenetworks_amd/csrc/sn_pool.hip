// sn_pool.hip — the two parameter-free pooling operations of the cascade model over sibling pairs of rows (gfx950).
// The definition is the section "Sibling-pair pooling" of sn_spmm.h.  Pure streaming passes: every operand is read or written once,
// one 16-byte item per thread where the rows allow it, non-temporal loads and stores, launches only (no memset, nothing that
// synchronises), so a step that holds them still captures into a hipGraph.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 ldv(const f4 *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ float ldv(const float *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void stv(f4 *p, f4 v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void stv(float *p, float v) { __builtin_nontemporal_store(v, p); }

// torch's MaxPool1d(2) choice: the second element iff it is larger or a NaN (a tie and (NaN, x) keep the first)
__device__ __forceinline__ bool second(float a, float b) { return b > a || b != b; }
__device__ __forceinline__ float pick(float a, float b) { return second(a, b) ? b : a; }
__device__ __forceinline__ f4 pick(f4 a, f4 b) { return f4{pick(a.x, b.x), pick(a.y, b.y), pick(a.z, b.z), pick(a.w, b.w)}; }
// (to the first, to the second) of a gradient g under that choice
__device__ __forceinline__ void route(float a, float b, float g, float &ga, float &gb) {
  const bool s = second(a, b);
  ga = s ? 0.f : g;
  gb = s ? g : 0.f;
}
__device__ __forceinline__ void route(f4 a, f4 b, f4 g, f4 &ga, f4 &gb) {
  float a0, b0, a1, b1, a2, b2, a3, b3;
  route(a.x, b.x, g.x, a0, b0);
  route(a.y, b.y, g.y, a1, b1);
  route(a.z, b.z, g.z, a2, b2);
  route(a.w, b.w, g.w, a3, b3);
  ga = f4{a0, a1, a2, a3};
  gb = f4{b0, b1, b2, b3};
}

// One item = W floats of one PAIR of fine rows (2 j, 2 j + 1) and of coarse row j; T is float (W = 1) or f4 (W = 4).  The leading
// dimensions are in floats.  pairs * (C / W) items, grid-stride.
template <class T>
struct Item {
  static constexpr int W = sizeof(T) / sizeof(float);
  int64_t j;
  int c;
  __device__ Item(int64_t t, int cw) {
    if (t <= (int64_t)UINT32_MAX) {      // (the 64-bit division is a long instruction sequence: only items past 2^32 pay for it)
      const uint32_t q = (uint32_t)t / (uint32_t)cw;
      j = q;
      c = (int)((uint32_t)t - q * (uint32_t)cw) * W;
    } else {
      j = t / cw;
      c = (int)(t - j * cw) * W;
    }
  }
  __device__ const T *fine(const float *p, int64_t ld, int s) const { return reinterpret_cast<const T *>(p + (2 * j + s) * ld + c); }
  __device__ T *fine(float *p, int64_t ld, int s) const { return reinterpret_cast<T *>(p + (2 * j + s) * ld + c); }
  __device__ const T *coarse(const float *p, int64_t ld) const { return reinterpret_cast<const T *>(p + j * ld + c); }
  __device__ T *coarse(float *p, int64_t ld) const { return reinterpret_cast<T *>(p + j * ld + c); }
};

template <class T>
__global__ __launch_bounds__(kWG) void pool_max2_fwd_k(const float *__restrict__ x, int64_t ldx, float *__restrict__ y, int64_t ldy,
                                                       int64_t pairs, int C) {
  const int cw = C / Item<T>::W;
  const int64_t total = pairs * cw;
  for (int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x; t < total; t += (int64_t)gridDim.x * kWG) {
    const Item<T> it(t, cw);
    const T a = ldv(it.fine(x, ldx, 0)), b = ldv(it.fine(x, ldx, 1));
    stv(it.coarse(y, ldy), pick(a, b));
  }
}

template <class T>
__global__ __launch_bounds__(kWG) void pool_max2_bwd_k(const float *__restrict__ x, int64_t ldx, const float *__restrict__ g,
                                                       int64_t ldg, float *__restrict__ gx, int64_t ldgx, int64_t pairs, int C) {
  const int cw = C / Item<T>::W;
  const int64_t total = pairs * cw;
  for (int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x; t < total; t += (int64_t)gridDim.x * kWG) {
    const Item<T> it(t, cw);
    const T a = ldv(it.fine(x, ldx, 0)), b = ldv(it.fine(x, ldx, 1)), gv = ldv(it.coarse(g, ldg));
    T ga, gb;
    route(a, b, gv, ga, gb);
    stv(it.fine(gx, ldgx, 0), ga);
    stv(it.fine(gx, ldgx, 1), gb);
  }
}

template <class T>
__global__ __launch_bounds__(kWG) void unpool2_add_fwd_k(const float *__restrict__ x, int64_t ldx, const float *__restrict__ skip,
                                                         int64_t lds, float *__restrict__ y, int64_t ldy, int64_t pairs, int C) {
  const int cw = C / Item<T>::W;
  const int64_t total = pairs * cw;
  for (int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x; t < total; t += (int64_t)gridDim.x * kWG) {
    const Item<T> it(t, cw);
    const T v = ldv(it.coarse(x, ldx)), s0 = ldv(it.fine(skip, lds, 0)), s1 = ldv(it.fine(skip, lds, 1));
    stv(it.fine(y, ldy, 0), v + s0);
    stv(it.fine(y, ldy, 1), v + s1);
  }
}

template <class T>
__global__ __launch_bounds__(kWG) void unpool2_bwd_k(const float *__restrict__ g, int64_t ldg, float *__restrict__ gx, int64_t ldgx,
                                                     int64_t pairs, int C) {
  const int cw = C / Item<T>::W;
  const int64_t total = pairs * cw;
  for (int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x; t < total; t += (int64_t)gridDim.x * kWG) {
    const Item<T> it(t, cw);
    const T g0 = ldv(it.fine(g, ldg, 0)), g1 = ldv(it.fine(g, ldg, 1));
    stv(it.coarse(gx, ldgx), g0 + g1);
  }
}

inline bool vec_ok(const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && ld % 4 == 0; }

// argument checks every entry shares: the pair count, the width, the leading dimensions (each >= C) and the item count
inline int check(int64_t pairs, int32_t C, const int64_t *ld, int n) {
  if (pairs < 0 || C < 1) return SN_E_SHAPE;
  for (int i = 0; i < n; ++i)
    if (ld[i] < C) return SN_E_SHAPE;
  if (pairs > INT64_MAX / 4 / (int64_t)C) return SN_E_RANGE;
  return SN_OK;
}

}  // namespace

#define SN_POOL_LAUNCH(kernel, vec, ...)                                                                                      \
  do {                                                                                                                        \
    if (vec)                                                                                                                  \
      hipLaunchKernelGGL((kernel<f4>), dim3(grid_for(pairs * (C / 4), kWG, INT_MAX)), dim3(kWG), 0, s, __VA_ARGS__);          \
    else                                                                                                                      \
      hipLaunchKernelGGL((kernel<float>), dim3(grid_for(pairs * (int64_t)C, kWG, INT_MAX)), dim3(kWG), 0, s, __VA_ARGS__);    \
  } while (0)

extern "C" {

int sn_pool_max2_fwd_f32(const float *x, int64_t ldx, int64_t pairs, int32_t C, float *y, int64_t ldy, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  const int64_t ld[] = {ldx, ldy};
  if (const int e = check(pairs, C, ld, 2)) return e;
  if (pairs == 0) return SN_OK;
  if (!x || !y) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = C % 4 == 0 && vec_ok(x, ldx) && vec_ok(y, ldy);
  SN_POOL_LAUNCH(pool_max2_fwd_k, vec, x, ldx, y, ldy, pairs, (int)C);
  return launch_status();
}

int sn_pool_max2_bwd_f32(const float *x, int64_t ldx, const float *g, int64_t ldg, int64_t pairs, int32_t C, float *gx,
                         int64_t ldgx, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  const int64_t ld[] = {ldx, ldg, ldgx};
  if (const int e = check(pairs, C, ld, 3)) return e;
  if (pairs == 0) return SN_OK;
  if (!x || !g || !gx) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = C % 4 == 0 && vec_ok(x, ldx) && vec_ok(g, ldg) && vec_ok(gx, ldgx);
  SN_POOL_LAUNCH(pool_max2_bwd_k, vec, x, ldx, g, ldg, gx, ldgx, pairs, (int)C);
  return launch_status();
}

int sn_unpool2_add_fwd_f32(const float *x, int64_t ldx, const float *skip, int64_t lds, int64_t pairs, int32_t C, float *y,
                           int64_t ldy, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  const int64_t ld[] = {ldx, lds, ldy};
  if (const int e = check(pairs, C, ld, 3)) return e;
  if (pairs == 0) return SN_OK;
  if (!x || !skip || !y) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = C % 4 == 0 && vec_ok(x, ldx) && vec_ok(skip, lds) && vec_ok(y, ldy);
  SN_POOL_LAUNCH(unpool2_add_fwd_k, vec, x, ldx, skip, lds, y, ldy, pairs, (int)C);
  return launch_status();
}

int sn_unpool2_bwd_f32(const float *g, int64_t ldg, int64_t pairs, int32_t C, float *gx, int64_t ldgx, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  const int64_t ld[] = {ldg, ldgx};
  if (const int e = check(pairs, C, ld, 2)) return e;
  if (pairs == 0) return SN_OK;
  if (!g || !gx) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = C % 4 == 0 && vec_ok(g, ldg) && vec_ok(gx, ldgx);
  SN_POOL_LAUNCH(unpool2_bwd_k, vec, g, ldg, gx, ldgx, pairs, (int)C);
  return launch_status();
}

}  // extern "C"

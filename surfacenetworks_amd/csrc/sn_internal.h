// sn_internal.h — what the translation units of the library share with each other (internal: not part of the C interface).
// The functions are defined in sn_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_spmm.h"

// compute units of the current device (256 when there is no device to ask)
int sn_internal_cu_count();

// fills and device-to-device copies as kernels of this library (sn_kernels.hip says why not hipMemsetAsync / hipMemcpy2DAsync)
hipError_t sn_internal_fill(void *dst, int value, size_t bytes, hipStream_t s);
hipError_t sn_internal_fill2d(void *dst, int64_t pitch, int value, int64_t width, int64_t rows, hipStream_t s);
hipError_t sn_internal_copy2d(void *dst, int64_t dpitch, const void *src, int64_t spitch, int64_t width, int64_t rows, hipStream_t s);

// per-launch timing (the facility behind sn_timing_*)
bool sn_internal_timing_on();
bool sn_internal_timing_slot(int kind, int64_t rows, int64_t width, int64_t bytes, int outw, hipEvent_t *s, hipEvent_t *e);

// Exclusive scan of in[0..n) into out[0..n) on stream s, three launches; out may be in.  sums: sn_scan_workspace_bytes(n) bytes
// of device scratch.  The block sums are added up in int64.  With a status word: too_large is OR-ed into it when the total
// exceeds INT_MAX, and out is left untouched once *status holds a bit of skip_mask.  Launches only: the caller asks for the
// launch status.
void sn_internal_scan_i32(const int *in, int64_t n, int *out, int *sums, int *status, int too_large, int skip_mask, hipStream_t s);

// Workspace layouts are written once, over a Carver: without a base it only measures, with one it hands out the slices, each
// padded to 16 bytes.  The *_workspace_bytes query and the entry point run the same description.
struct SnCarver {
  char *base;
  size_t bytes = 0;
  explicit SnCarver(void *workspace) : base(static_cast<char *>(workspace)) {}
  template <class T>
  T *take(size_t count) {
    T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
    bytes += (count * sizeof(T) + 15) & ~(size_t)15;
    return p;
  }
  int *take_scan(int64_t n) { return take<int>(sn_scan_workspace_bytes(n) / sizeof(int)); }      // scratch of a scan over n items
};

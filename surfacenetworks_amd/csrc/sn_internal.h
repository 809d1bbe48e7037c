// sn_internal.h — what the translation units of the library share with each other (internal: not part of the C interface).
// The functions are defined in sn_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_spmm.h"

// what an entry point returns after its launches: SN_OK, or the runtime's error
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SN_OK : (int)e;
}
// workgroups for n items at per_block items each: at least one, at most cap (grid-stride loops take the rest)
inline unsigned grid_for(int64_t n, int per_block, int64_t cap = 65535 * 16) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

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

// By-vertex incidence of the good faces of F (sn_meshops.hip: bucket_count_k, bucket_offsets, bucket_fill_k, vertex_sort_k):
// ptr[nV + 1] and inc[ptr[v] .. ptr[v + 1]) = the codes 3 f + c of the corners at vertex v, ascending.  A face with an index outside
// 0..nV-1 or a repeated index is left out and raises bad_face_bit in *status: the caller's own bit in its own status word
// (SN_ARAP_BAD_FACE for sn_arap_weights_f64, SN_DESC_BAD_FACE for sn_mesh_principal_curvature_f32).  The arrays live in the
// workspace (sn_internal_incidence_bytes); sums is scan scratch for nV + 1 items that the caller may use afterwards.
size_t sn_internal_incidence_bytes(int64_t nV, int64_t nF);
int sn_internal_incidence(const int *F, int64_t nV, int64_t nF, void *workspace, int *status, int bad_face_bit, const int **ptr,
                          const int **inc, int **sums, hipStream_t s);

// stable insertion sort of key[b..e), ascending, that carries up to two payload arrays along
template <class A = char, class B = char>
__device__ __forceinline__ void sort_run(int *key, int b, int e, A *pa = nullptr, B *pb = nullptr) {
  for (int i = b + 1; i < e; ++i) {
    const int k = key[i];
    const A va = pa ? pa[i] : A();
    const B vb = pb ? pb[i] : B();
    int j = i - 1;
    while (j >= b && key[j] > k) {
      key[j + 1] = key[j];
      if (pa) pa[j + 1] = pa[j];
      if (pb) pb[j + 1] = pb[j];
      --j;
    }
    key[j + 1] = k;
    if (pa) pa[j + 1] = va;
    if (pb) pb[j + 1] = vb;
  }
}

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

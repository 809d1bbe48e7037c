// sn_hierarchy.hip — one coarsening step of a mesh hierarchy: edge scores, handshake matching, restriction weights (gfx950).
// The definition is the section "Mesh hierarchy" of sn_spmm.h; mesh_ops.hierarchy_scores / handshake_matching / coarsen_operator
// are its numpy statement and this file is its other transcription: fp32, no contraction, correctly rounded divisions, ties to
// the smallest column, so the two agree bit for bit.  One workgroup walks the whole operator: the rounds of the matching run
// inside the kernel, propose and accept separated by barriers, the state in global memory, no host read-back between rounds.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kThreads = SN_HIER_THREADS;

struct MatchWs {
  SnCarver c;
  float *diag;       // [n]   |L_ii|, 0 where the row stores no diagonal entry
  float *score;      // [nnz] s_ij per stored entry, 0 on the diagonal and where a diagonal is 0
  int *prop;         // [n]   the proposal of the current round, -1 for none
  MatchWs(void *w, int64_t n, int64_t nnz) : c(w), diag(c.take<float>(n)), score(c.take<float>(nnz)), prop(c.take<int>(n)) {}
};

// |L_ji| of the stored entry (j, i), 0 if row j stores none: binary search over the ascending columns of row j
__device__ __forceinline__ float stored_abs(const int *rowptr, const int *colind, const float *vals, int j, int i) {
  int lo = rowptr[j], hi = rowptr[j + 1];
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (colind[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return (lo < rowptr[j + 1] && colind[lo] == i) ? fabsf(vals[lo]) : 0.f;
}

__global__ __launch_bounds__(kThreads) void mesh_match_k(const int *__restrict__ rowptr, const int *__restrict__ colind,
                                                         const float *__restrict__ vals, const float *__restrict__ mass, int n,
                                                         int max_rounds, int *mate, float *r, float *msum, int *out, float *diag,
                                                         float *score, int *prop) {
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  int status = 0;
  // a column outside the operator: nothing below may index with it
  if (tid == 0) s_flag = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kThreads)
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p)
      if (colind[p] < 0 || colind[p] >= n) s_flag = 1;
  __syncthreads();
  if (s_flag) {
    for (int i = tid; i < n; i += kThreads) {
      mate[i] = -1;
      r[i] = 1.f;
      msum[i] = mass ? mass[i] : 1.f;
    }
    if (tid == 0) {
      out[0] = 0;
      out[1] = SN_HIER_BAD_COLUMN;
    }
    return;
  }
  for (int i = tid; i < n; i += kThreads) {
    float d = 0.f;
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p)
      if (colind[p] == i) d = fabsf(vals[p]);
    diag[i] = d;
    mate[i] = -1;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    const float di = diag[i];
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) {
      const int j = colind[p];
      float s = 0.f;
      if (j != i && di > 0.f && diag[j] > 0.f) s = fabsf(vals[p]) / di + stored_abs(rowptr, colind, vals, j, i) / diag[j];
      score[p] = s;
    }
  }
  __syncthreads();
  int rounds = 0;
  for (;;) {
    if (tid == 0) s_flag = 0;
    // propose: the unmatched neighbour with the largest positive score, ties to the smallest column (columns ascend)
    for (int i = tid; i < n; i += kThreads) {
      int best = -1;
      if (mate[i] < 0) {
        float bs = 0.f;
        for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) {
          const float s = score[p];
          if (s > bs && mate[colind[p]] < 0) {
            bs = s;
            best = colind[p];
          }
        }
      }
      prop[i] = best;
    }
    __syncthreads();
    // is any proposal mutual?
    for (int i = tid; i < n; i += kThreads) {
      const int j = prop[i];
      if (j >= 0 && prop[j] == i) s_flag = 1;
    }
    __syncthreads();
    const int made = s_flag;
    if (!made) break;
    if (rounds >= max_rounds) {
      status = SN_HIER_NOT_FINISHED;
      break;
    }
    for (int i = tid; i < n; i += kThreads) {
      const int j = prop[i];
      if (j >= 0 && prop[j] == i) mate[i] = j;
    }
    ++rounds;
    __syncthreads();      // the mates of this round are written, and every thread has read s_flag, before the next round begins
  }
  __syncthreads();
  // restriction weights: r_i = m_i / (m_i + m_mate), r = 1 for a singleton; msum_i = m_i + m_mate (m_i for a singleton)
  for (int i = tid; i < n; i += kThreads) {
    const float mi = mass ? mass[i] : 1.f;
    const int j = mate[i];
    float sum = mi, ri = 1.f;
    if (j >= 0) {
      sum = mi + (mass ? mass[j] : 1.f);
      ri = mi / sum;
    }
    msum[i] = sum;
    r[i] = ri;
  }
  if (tid == 0) {
    out[0] = rounds;
    out[1] = status;
  }
}

}  // namespace

size_t sn_mesh_match_workspace_bytes(int64_t n, int64_t nnz) {
  if (n < 0 || nnz < 0) return 0;
  return MatchWs(nullptr, n, nnz).c.bytes;
}

int sn_mesh_match_f32(const int32_t *rowptr, const int32_t *colind, const float *vals, const float *mass, int64_t n, int64_t nnz,
                      int32_t max_rounds, int32_t *mate, float *r, float *msum, int32_t *out, void *workspace,
                      size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (n < 0 || nnz < 0 || max_rounds < 0) return SN_E_SHAPE;
  if (n + 1 > (int64_t)INT_MAX || nnz > (int64_t)INT_MAX) return SN_E_RANGE;
  if (!out || !rowptr || (n > 0 && (!mate || !r || !msum)) || (nnz > 0 && (!colind || !vals))) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_match_workspace_bytes(n, nnz) || (n > 0 && !workspace)) return SN_E_WORKSPACE;
  MatchWs ws(workspace, n, nnz);
  hipLaunchKernelGGL(mesh_match_k, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), rowptr, colind, vals, mass, (int)n,
                     (int)max_rounds, mate, r, msum, out, ws.diag, ws.score, ws.prop);
  return launch_status();
}

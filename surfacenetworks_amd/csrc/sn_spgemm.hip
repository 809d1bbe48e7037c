// sn_spgemm.hip — sparse x sparse CSR products and the symmetric diagonal scaling of the 'amp' tower's operators  (gfx950).
// Every product and every sum rounds on its own: FMA contraction is switched off for this file and the arithmetic is written
// out here, so the results are the ones the written definition (include/sn_spmm.h) gives on any host.  (Not __fmul_rn /
// __fadd_rn: the runtime header that defines them as x * y and x + y is parsed BEFORE the pragma below, both carry the
// `contract` flag, and once inlined the compiler fuses them — measured: v_fmac_f32 in the fill kernel, other bits than scipy's.)
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;
constexpr int kWaves = kWG / 64;
constexpr int kMaxWindow = SN_SPGEMM_MAX_WINDOW;      // columns one result row may span: one bit each in LDS
constexpr int kMaxWords = kMaxWindow / 32;            // 4096 words = 16 KiB per workgroup, 8 workgroups per CU fit 160 KiB
constexpr int kRefusal = SN_SPGEMM_TOO_WIDE | SN_SPGEMM_TOO_LARGE;

// exclusive scan of one value per thread across the workgroup (numbers a row's candidate columns); *total: the workgroup's sum
__device__ __forceinline__ int block_excl_scan(int v, int *total) {
  __shared__ int wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    if (i < wave) off += wsum[i];
    tot += wsum[i];
  }
  *total = tot;
  return off + incl - v;
}

// counts[0..M] (a zero at M) and the scratch of their scan: sn_csr_spgemm_workspace_bytes and both entry points
struct CountsWs {
  int *counts, *sums;
  size_t bytes;
  CountsWs(void *workspace, int64_t M) {
    SnCarver c(workspace);
    counts = c.take<int>(M + 1);
    sums = c.take_scan(M + 1);
    bytes = c.bytes;
  }
};
// counts[0..n1) -> out[0..n1), the scan of sn_kernels.hip.  With a status word a total that does not fit the int32 row pointers
// is refused, and out is left as it is once the call is refused (a count is at most kMaxWindow: a tile's sum stays below 2^28)
int scan_counts(const CountsWs &w, int64_t n1, int *out, int *status, hipStream_t s) {
  sn_internal_scan_i32(w.counts, n1, out, w.sums, status, SN_SPGEMM_TOO_LARGE, kRefusal, s);
  return launch_status();
}

// ---- one result row per workgroup ---------------------------------------------------------------------------------------------
// The row's candidate columns are the union of the rows j of B over the entries (i, j) of A.  They are marked as bits of an LDS
// bitmap over the row's column window [lo, hi] (atomicOr on bits: the outcome does not depend on the order), a popcount prefix
// over the words numbers them in ascending column order, and — FILL — every thread then owns result entries: it walks A's row in
// storage (= ascending column) order and looks k up in B's row j by binary search, so each sum is sequential in j.
// FILL = false: counts[row] = structural entries.  FILL = true: columns and values at s_rowptr[row], nzcount[row] = values != 0.
template <bool FILL>
__global__ __launch_bounds__(kWG) void spgemm_row_k(const int *__restrict__ a_rp, const int *__restrict__ a_ci,
                                                    const float *__restrict__ a_v, const int *__restrict__ b_rp,
                                                    const int *__restrict__ b_ci, const float *__restrict__ b_v, int M, int K, int N,
                                                    int *__restrict__ counts, const int *__restrict__ s_rowptr,
                                                    int *__restrict__ s_colind, float *__restrict__ s_vals, int *__restrict__ nzcount,
                                                    int *__restrict__ status) {
  __shared__ unsigned bits[kMaxWords];
  __shared__ int sh_lo, sh_hi, sh_nz;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (FILL && (*status & kRefusal)) return;               // (uniform: written by an earlier launch)
  int flags = 0;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const int a0 = a_rp[row], a1 = a_rp[row + 1];
    if (tid == 0) {
      sh_lo = INT_MAX;
      sh_hi = -1;
      sh_nz = 0;
    }
    __syncthreads();
    int lo = INT_MAX, hi = -1;
    for (int p = a0 + tid; p < a1; p += kWG) {
      const int j = a_ci[p];
      if (j < 0 || j >= K) {
        flags |= SN_SPGEMM_BAD_COLUMN;
        continue;
      }
      const int b0 = b_rp[j], b1 = b_rp[j + 1];
      if (b1 > b0) {
        const int first = b_ci[b0], last = b_ci[b1 - 1];
        if (first < 0 || last >= N) flags |= SN_SPGEMM_BAD_COLUMN;      // (reported even when the clamped window is refused)
        lo = min(lo, first);
        hi = max(hi, last);
      }
    }
    if (hi >= lo) {
      atomicMin(&sh_lo, lo);
      atomicMax(&sh_hi, hi);
    }
    __syncthreads();
    lo = max(sh_lo, 0);
    hi = min(sh_hi, N - 1);
    int total = 0;
    const bool empty = hi < lo;                            // (uniform) no candidate inside 0..N-1
    const bool wide = !empty && hi - lo >= kMaxWindow;     // (uniform) the bitmap cannot hold this row: the call is refused
    if (wide) flags |= SN_SPGEMM_TOO_WIDE;
    if (!empty && !wide) {
      const int nwords = ((hi - lo) >> 5) + 1;
      for (int w = tid; w < nwords; w += kWG) bits[w] = 0u;
      __syncthreads();
      // mark: one wave per entry of A's row, its lanes along the row of B
      for (int p = a0 + wave; p < a1; p += kWaves) {
        const int j = a_ci[p];
        if (j < 0 || j >= K) continue;
        const int b1 = b_rp[j + 1];
        for (int q = b_rp[j] + lane; q < b1; q += 64) {
          const int k = b_ci[q];
          if (k < 0 || k >= N) flags |= SN_SPGEMM_BAD_COLUMN;
          else if (k >= lo && k <= hi) atomicOr(&bits[(k - lo) >> 5], 1u << ((k - lo) & 31));
        }
      }
      __syncthreads();
      // number the set bits: each thread owns a run of consecutive words
      const int wpt = (nwords + kWG - 1) / kWG;
      const int w0 = min(tid * wpt, nwords), w1 = min(w0 + wpt, nwords);
      int mine = 0;
      for (int w = w0; w < w1; ++w) mine += __popc(bits[w]);
      int off = block_excl_scan(mine, &total);
      if (FILL) {
        const int base = s_rowptr[row], end = s_colind && s_vals ? s_rowptr[row + 1] : base;      // (no arrays: nothing to fill)
        for (int w = w0; w < w1; ++w) {
          unsigned m = bits[w];
          while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            if (base + off < end) s_colind[base + off] = lo + (w << 5) + b;
            ++off;
          }
        }
        __syncthreads();                                   // (the columns written above are read by other threads below)
        const int cnt = min(total, end - base);
        int nz = 0;
        for (int e = tid; e < cnt; e += kWG) {
          const int k = s_colind[base + e];
          float acc = 0.0f;
          for (int p = a0; p < a1; ++p) {
            const int j = a_ci[p];
            if (j < 0 || j >= K) continue;
            int l = b_rp[j], r = b_rp[j + 1];
            while (l < r) {                                // first position with column >= k
              const int mid = l + ((r - l) >> 1);
              if (b_ci[mid] < k) l = mid + 1;
              else r = mid;
            }
            if (l < b_rp[j + 1] && b_ci[l] == k) {
              const float prod = a_v[p] * b_v[l];          // (contraction is off for this file: a product, then a sum)
              acc = acc + prod;
            }
          }
          s_vals[base + e] = acc;
          nz += (acc != 0.0f) ? 1 : 0;
        }
        if (nz) atomicAdd(&sh_nz, nz);
      }
    }
    __syncthreads();
    if (tid == 0) {
      if (FILL) nzcount[row] = sh_nz;
      else counts[row] = total;
    }
    __syncthreads();                                       // (sh_* and bits are reused by the next row)
  }
  if (!FILL && flags) atomicOr(status, flags);
}

// ---- D^-1/2 from the row lengths, the scaling on the pattern, and the compaction both builders end with -------------------------
__global__ __launch_bounds__(kWG) void inv_sqrt_degree_k(const int *__restrict__ rowptr, int64_t M, float *__restrict__ d,
                                                         int *__restrict__ status) {
  int flags = 0;
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < M; i += (int64_t)gridDim.x * kWG) {
    const int deg = rowptr[i + 1] - rowptr[i] - 1;
    if (deg < 1) flags = SN_CSR_NO_OFFDIAGONAL;
    d[i] = (float)(1.0 / sqrt((double)deg));
  }
  if (flags) atomicOr(status, flags);
}

// one wave per row: s_vals on A's pattern, nzcount[row] = results != 0
__global__ __launch_bounds__(kWG) void scale_sym_k(const int *__restrict__ rowptr, const int *__restrict__ colind,
                                                   const float *__restrict__ vals, const float *__restrict__ d, int64_t M,
                                                   float *__restrict__ s_vals, int *__restrict__ nzcount, int *__restrict__ status) {
  const int lane = threadIdx.x & 63;
  int flags = 0;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * kWaves) {
    const int p0 = rowptr[row], p1 = rowptr[row + 1];
    const float di = d[row];
    int nz = 0;
    for (int p = p0 + lane; p < p1; p += 64) {
      const int j = colind[p];
      float v = 0.0f;
      if (j < 0 || j >= M) flags = SN_SPGEMM_BAD_COLUMN;
      else v = (di * vals[p]) * d[j];
      if (s_vals) s_vals[p] = v;
      nz += (v != 0.0f) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
    if (lane == 0) nzcount[row] = nz;
  }
  if (flags) atomicOr(status, flags);
}

// one wave per row: the entries with a value != 0, in order, from (s_rowptr, s_colind, s_vals) to (rowptr, colind, vals)
__global__ __launch_bounds__(kWG) void compact_nonzero_k(const int *__restrict__ s_rowptr, const int *__restrict__ s_colind,
                                                         const float *__restrict__ s_vals, int64_t M, const int *__restrict__ rowptr,
                                                         int *__restrict__ colind, float *__restrict__ vals) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * kWaves) {
    const int p0 = s_rowptr[row], p1 = s_rowptr[row + 1];
    const int end = rowptr[row + 1];
    int out = rowptr[row];
    for (int c0 = p0; c0 < p1; c0 += 64) {                 // (uniform per wave)
      const int p = c0 + lane;
      const float v = p < p1 ? s_vals[p] : 0.0f;
      const bool keep = p < p1 && v != 0.0f;
      const unsigned long long m = __ballot(keep);
      const int pos = out + __popcll(m & ((1ull << lane) - 1ull));
      if (keep && pos < end) {
        colind[pos] = s_colind[p];
        vals[pos] = v;
      }
      out += __popcll(m);
    }
  }
}

int compact(const int32_t *s_rowptr, const int32_t *s_colind, const float *s_vals, int64_t M, const int32_t *rowptr,
            int32_t *colind, float *vals, hipStream_t s) {
  if (M == 0 || !colind) return SN_OK;                     // (no row, or a result without entries)
  if (!s_colind || !s_vals || !vals) return SN_E_NULL;
  hipLaunchKernelGGL(compact_nonzero_k, dim3(grid_for(M, kWaves)), dim3(kWG), 0, s, s_rowptr, s_colind, s_vals, M, rowptr, colind,
                     vals);
  return launch_status();
}

}  // namespace

extern "C" {

int64_t sn_csr_spgemm_max_window(void) { return kMaxWindow; }

size_t sn_csr_spgemm_workspace_bytes(int64_t M) {
  return CountsWs(nullptr, M < 0 ? 0 : M).bytes;
}

int sn_csr_spgemm_f32(const int32_t *a_rowptr, const int32_t *a_colind, const float *a_vals, const int32_t *b_rowptr,
                      const int32_t *b_colind, const float *b_vals, int64_t M, int64_t K, int64_t N, int32_t phase,
                      int32_t *s_rowptr, int32_t *s_colind, float *s_vals, int32_t *rowptr, int32_t *colind, float *vals,
                      int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (M < 0 || K < 0 || N < 0 || phase < 0 || phase > 2) return SN_E_SHAPE;
  if (M + 1 > INT_MAX || K + 1 > INT_MAX || N > INT_MAX) return SN_E_RANGE;
  if (!a_rowptr || !b_rowptr || !s_rowptr || !status) return SN_E_NULL;
  if (phase >= 1 && !rowptr) return SN_E_NULL;
  if (workspace_bytes < sn_csr_spgemm_workspace_bytes(M) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CountsWs ws(workspace, M);
  int *counts = ws.counts;
  const unsigned grid = (unsigned)(M < 1 ? 1 : (M > 65535 * 16 ? 65535 * 16 : M));
  if (phase == 0) {
    hipError_t e = sn_internal_fill(status, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    e = sn_internal_fill(counts + M, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (M > 0)
      hipLaunchKernelGGL((spgemm_row_k<false>), dim3(grid), dim3(kWG), 0, s, a_rowptr, a_colind, a_vals, b_rowptr, b_colind, b_vals,
                         (int)M, (int)K, (int)N, counts, (const int *)nullptr, (int *)nullptr, (float *)nullptr, (int *)nullptr,
                         status);
    return scan_counts(ws, M + 1, s_rowptr, status, s);
  }
  if (phase == 1) {
    // a product without structural entries has nothing to fill: s_colind / s_vals may then be NULL, the kernel writes neither
    hipError_t e = sn_internal_fill(counts + M, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (M > 0)
      hipLaunchKernelGGL((spgemm_row_k<true>), dim3(grid), dim3(kWG), 0, s, a_rowptr, a_colind, a_vals, b_rowptr, b_colind, b_vals,
                         (int)M, (int)K, (int)N, (int *)nullptr, (const int *)s_rowptr, s_colind, s_vals, counts, status);
    return scan_counts(ws, M + 1, rowptr, status, s);
  }
  return compact(s_rowptr, s_colind, s_vals, M, rowptr, colind, vals, s);
}

int sn_csr_inv_sqrt_degree_f32(const int32_t *rowptr, int64_t M, float *d, int32_t *status, void *stream) {
  (void)hipGetLastError();
  if (M < 0) return SN_E_SHAPE;
  if (M + 1 > INT_MAX) return SN_E_RANGE;
  if (!status) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (M == 0) return SN_OK;
  if (!rowptr || !d) return SN_E_NULL;
  hipLaunchKernelGGL(inv_sqrt_degree_k, dim3(grid_for(M, kWG)), dim3(kWG), 0, s, rowptr, M, d, status);
  return launch_status();
}

int sn_csr_scale_sym_f32(const int32_t *a_rowptr, const int32_t *a_colind, const float *a_vals, const float *d, int64_t M,
                         int32_t phase, float *s_vals, int32_t *rowptr, int32_t *colind, float *vals, int32_t *status,
                         void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (M < 0 || (phase != 0 && phase != 1)) return SN_E_SHAPE;
  if (M + 1 > INT_MAX) return SN_E_RANGE;
  if (!a_rowptr || !rowptr || !status) return SN_E_NULL;
  if (workspace_bytes < sn_csr_spgemm_workspace_bytes(M) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CountsWs ws(workspace, M);
  int *counts = ws.counts;
  if (phase == 0) {
    hipError_t e = sn_internal_fill(status, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    e = sn_internal_fill(counts + M, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (M > 0) {
      if (!d) return SN_E_NULL;
      hipLaunchKernelGGL(scale_sym_k, dim3(grid_for(M, kWaves)), dim3(kWG), 0, s, a_rowptr, a_colind, a_vals, d, M, s_vals, counts,
                         status);
    }
    return scan_counts(ws, M + 1, rowptr, (int *)nullptr, s);
  }
  return compact(a_rowptr, a_colind, s_vals, M, rowptr, colind, vals, s);
}

}  // extern "C"

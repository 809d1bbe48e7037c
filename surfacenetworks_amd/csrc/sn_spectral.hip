// sn_spectral.hip — the device side of the eigen-solver for the cotangent pencil and of the wave kernel signature (gfx950):
// the start block, the Chebyshev filter step and the WKS contraction (definition: include/sn_spmm.h, "Spectral"; host statement:
// mesh_ops.spectral_start, cheb_filter_step, wks_contract).  Everything is fp64 in the header's operation order; FMA contraction
// is switched off for this file so that every rounding is the one numpy makes.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;
constexpr int kMaxT = 4;      // columns a lane of the filter step keeps at once


// the mesh of row i: the last b with voff[b] <= i (meshes without rows are passed over)
__device__ __forceinline__ int mesh_of(const int *__restrict__ voff, int B, int i) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (voff[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kWG) void spectral_start_k(uint64_t seed, const int *__restrict__ voff, int B, int64_t n, int64_t m,
                                                        double *__restrict__ X) {
  const uint64_t golden = 0x9E3779B97F4A7C15ull;
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < n * m; e += (int64_t)gridDim.x * kWG) {
    const int i = (int)(e / m);
    const int64_t c = e - (int64_t)i * m;
    const int row = i - voff[mesh_of(voff, B, i)];
    const uint64_t h = mix64(mix64(seed + golden + (uint64_t)row) + golden + (uint64_t)c);
    X[e] = (double)(h >> 11) * 0x1p-53 - 0.5;
  }
}

// One group of W lanes takes T * W columns of one row: lane l the columns c0 + l, c0 + l + W, ...  W = 64 is the form for wide
// blocks (m >= 64): the row, its mesh and its stored entries are then the same for the whole wave, the row number is made
// scalar, and every gather of Y[j, :] reads 512 contiguous bytes per wave and kept column set; T independent loads per stored
// entry are in flight per lane.  W < 64 (m < 64) puts 64 / W rows into a wave.  The sum of a row is serial over its entries.
template <int W, int T>
__global__ __launch_bounds__(kWG) void cheb_step_k(const int *__restrict__ rowptr, const int *__restrict__ colind,
                                                   const double *__restrict__ vals, const int *__restrict__ voff, int B, int64_t n,
                                                   int64_t m, int64_t chunks, const double *__restrict__ alpha,
                                                   const double *__restrict__ beta, const double *__restrict__ shift,
                                                   const double *X, const double *__restrict__ Y, double *Z) {
  const int lane = threadIdx.x % W;
  const int64_t groups = n * chunks;
  for (int64_t g = ((int64_t)blockIdx.x * kWG + threadIdx.x) / W; g < groups; g += (int64_t)gridDim.x * (kWG / W)) {
    int i = (int)(g / chunks);
    int chunk = (int)(g - (int64_t)i * chunks);
    if constexpr (W == 64) {      // a wave is one group
      i = __builtin_amdgcn_readfirstlane(i);
      chunk = __builtin_amdgcn_readfirstlane(chunk);
    }
    const int64_t c0 = (int64_t)chunk * (W * T) + lane;
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    const int pe = rowptr[i + 1];
    for (int p = rowptr[i]; p < pe; ++p) {
      const int j = colind[p];
      if ((uint32_t)j >= (uint32_t)n) continue;      // a column outside the matrix is not read (n fits int32)
      const double a = vals[p];
      const double *__restrict__ y = Y + (int64_t)j * m;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int64_t c = c0 + (int64_t)t * W;
        if (c < m) acc[t] = acc[t] + a * y[c];
      }
    }
    const int b = mesh_of(voff, B, i);
    const double al = alpha[b], be = beta[b], sh = shift[b];
    const int64_t base = (int64_t)i * m;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int64_t c = c0 + (int64_t)t * W;
      if (c < m) Z[base + c] = (al * (acc[t] - sh * Y[base + c])) - be * X[base + c];
    }
  }
}

template <int W, int T>
void cheb_launch(const int *rowptr, const int *colind, const double *vals, const int *voff, int B, int64_t n, int64_t m, int64_t chunks,
                 const double *alpha, const double *beta, const double *shift, const double *X, const double *Y, double *Z,
                 hipStream_t s) {
  hipLaunchKernelGGL((cheb_step_k<W, T>), dim3(grid_for(n * chunks * W, kWG)), dim3(kWG), 0, s, rowptr, colind, vals, voff, B, n, m, chunks,
                     alpha, beta, shift, X, Y, Z);
}

// one thread per output element: the squares of a vertex's row of phi against column i of its mesh's W, serial over k
template <class O>
__global__ __launch_bounds__(kWG) void wks_k(const double *__restrict__ phi, const int *__restrict__ voff, int B, int64_t nV, int64_t k,
                                             int64_t N, const double *__restrict__ Wt, const double *__restrict__ Cn,
                                             O *__restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < nV * N; e += (int64_t)gridDim.x * kWG) {
    const int v = (int)(e / N);
    const int64_t i = e - (int64_t)v * N;
    const int b = mesh_of(voff, B, v);
    const double *__restrict__ p = phi + (int64_t)v * k;
    const double *__restrict__ w = Wt + (int64_t)b * k * N + i;
    double acc = 0.0;
    for (int64_t j = 0; j < k; ++j) acc = acc + (p[j] * p[j]) * w[j * N];
    out[e] = (O)(acc / Cn[(int64_t)b * N + i]);
  }
}

inline bool overlap(const double *a, const double *b, int64_t count) { return a < b + count && b < a + count; }

}  // namespace

extern "C" {

int sn_spectral_start_f64(uint64_t seed, const int32_t *voff, int64_t B, int64_t n, int64_t m, double *X, void *stream) {
  (void)hipGetLastError();
  if (B < 1 || n < 0 || m < 1) return SN_E_SHAPE;
  if (n > INT_MAX - 1 || B > INT_MAX - 1) return SN_E_RANGE;
  if (!voff || (n > 0 && !X)) return SN_E_NULL;
  if (n > 0)
    hipLaunchKernelGGL(spectral_start_k, dim3(grid_for(n * m, kWG)), dim3(kWG), 0, static_cast<hipStream_t>(stream), seed, voff, (int)B, n, m,
                       X);
  return launch_status();
}

int sn_cheb_filter_step_f64(const int32_t *rowptr, const int32_t *colind, const double *vals, const int32_t *voff, int64_t B, int64_t n,
                            int64_t m, const double *alpha, const double *beta, const double *shift, const double *X, const double *Y,
                            double *Z, void *stream) {
  (void)hipGetLastError();
  if (B < 1 || n < 0 || m < 1) return SN_E_SHAPE;
  if (n > INT_MAX - 1 || B > INT_MAX - 1 || m > INT_MAX) return SN_E_RANGE;
  if (!rowptr || !voff || !alpha || !beta || !shift) return SN_E_NULL;
  if (n == 0) return SN_OK;
  if (!X || !Y || !Z || !colind || !vals) return SN_E_NULL;
  if (overlap(Z, Y, n * m) || (Z != X && overlap(Z, X, n * m))) return SN_E_SHAPE;      // Z may BE X; it must not touch Y
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int iB = (int)B;
#define SN_CHEB(W, T) cheb_launch<W, T>(rowptr, colind, vals, voff, iB, n, m, chunks, alpha, beta, shift, X, Y, Z, s)
  if (m >= 64) {
    const int64_t per = (m + 63) / 64;                        // wave-wide column sets of a row
    const int64_t chunks = (per + kMaxT - 1) / kMaxT;         // groups per row, each with the same number of sets
    switch ((per + chunks - 1) / chunks) {
      case 1: SN_CHEB(64, 1); break;
      case 2: SN_CHEB(64, 2); break;
      case 3: SN_CHEB(64, 3); break;
      default: SN_CHEB(64, 4); break;
    }
  } else {
    const int64_t chunks = 1;
    if (m > 32) SN_CHEB(64, 1);
    else if (m > 16) SN_CHEB(32, 1);
    else if (m > 8) SN_CHEB(16, 1);
    else if (m > 4) SN_CHEB(8, 1);
    else SN_CHEB(4, 1);
  }
#undef SN_CHEB
  return launch_status();
}

int sn_wks_f64(const double *phi, const int32_t *voff, int64_t B, int64_t nV, int64_t k, int64_t N, const double *W, const double *Cn,
               int32_t out_f32, void *out, void *stream) {
  (void)hipGetLastError();
  if (B < 1 || nV < 0 || k < 1 || N < 1) return SN_E_SHAPE;
  if (nV > INT_MAX - 1 || B > INT_MAX - 1) return SN_E_RANGE;
  if (!voff) return SN_E_NULL;
  if (nV == 0) return SN_OK;
  if (!phi || !W || !Cn || !out) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (out_f32)
    hipLaunchKernelGGL((wks_k<float>), dim3(grid_for(nV * N, kWG)), dim3(kWG), 0, s, phi, voff, (int)B, nV, k, N, W, Cn, (float *)out);
  else
    hipLaunchKernelGGL((wks_k<double>), dim3(grid_for(nV * N, kWG)), dim3(kWG), 0, s, phi, voff, (int)B, nV, k, N, W, Cn, (double *)out);
  return launch_status();
}

}  // extern "C"

// sn_arap.hip — as-rigid-as-possible deformation sequences on the device (gfx950): the weight builder and the frame kernel
// (definition: include/sn_spmm.h, "ARAP deformation"; host statement: mesh_ops.arap_*).  Everything is fp64 in the header's
// operation order; FMA contraction is switched off for this file so that every rounding is the one numpy makes.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;
constexpr int kNT = SN_ARAP_THREADS;          // threads of a frame workgroup = the width of the reduction
constexpr int kWaves = kNT / 64;
constexpr int kRedMax = 9;                    // values reduced at once
constexpr int kRedDoubles = 2 * kWaves * kRedMax;      // two alternating buffers of wave sums
constexpr int kLdsBytes = 160 * 1024 - 1024;      // dynamic LDS of a frame workgroup: the CU's, less room for what the compiler adds
constexpr int kMaxN = (kLdsBytes - kRedDoubles * 8) / 24;
constexpr int kMaxDeg = SN_LAP_MAX_DEGREE;


__device__ __forceinline__ double edge_len(const float *__restrict__ V, int a, int b) {
  const double dx = (double)V[3 * a] - (double)V[3 * b];
  const double dy = (double)V[3 * a + 1] - (double)V[3 * b + 1];
  const double dz = (double)V[3 * a + 2] - (double)V[3 * b + 2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// ---- weights: thread i walks its incident good faces (ascending face id), the frame of laplacian_rows_k -------------------------
template <bool FILL>
__global__ __launch_bounds__(kWG) void arap_weight_rows_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                          const int *__restrict__ vptr, const int *__restrict__ inc,
                                                          int *__restrict__ rowptr, int *__restrict__ colind, double *__restrict__ w,
                                                          double *__restrict__ d, int *__restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < nV; i += (int64_t)gridDim.x * kWG) {
    const int b = vptr[i], e = vptr[i + 1];
    if (e - b > kMaxDeg) {
      if constexpr (FILL) d[i] = 0.0; else { rowptr[i] = 0; atomicOr(status, SN_ARAP_DEGREE); }
      continue;
    }
    int nb[2 * kMaxDeg];
    double wij[2 * kMaxDeg];
    int n = 0;
    for (int o = b; o < e; ++o) {
      const int64_t f = inc[o] / 3;
      const int c = inc[o] % 3;
      const int v[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
      const double l[3] = {edge_len(V, v[0], v[1]), edge_len(V, v[1], v[2]), edge_len(V, v[2], v[0])};
      const double h = ((l[0] + l[1]) + l[2]) / 2;
      const double q = ((h * (h - l[0])) * (h - l[1])) * (h - l[2]);
      const double den = 8 * (q > 0 ? sqrt(q) : 1e-6) + 1e-6;
      const double a2 = l[c] * l[c], b2 = l[(c + 1) % 3] * l[(c + 1) % 3], c2 = l[(c + 2) % 3] * l[(c + 2) % 3];
      nb[n] = v[(c + 1) % 3]; wij[n] = ((-a2 + b2) + c2) / den; ++n;      // permutation (i, j, k)
      nb[n] = v[(c + 2) % 3]; wij[n] = ((-c2 + b2) + a2) / den; ++n;      // permutation (i, k, j)
    }
    sort_run(nb, 0, n, wij);      // by neighbour id; stable: the contributions of one entry stay in face order
    int out = FILL ? rowptr[i] : 0;
    double dsum = 0.0;
    for (int x = 0; x < n;) {
      const int kn = nb[x];
      double s = wij[x++];
      while (x < n && nb[x] == kn) s = s + wij[x++];
      if constexpr (FILL) {
        colind[out] = kn;
        w[out] = s;
        dsum = dsum + s;
      }
      ++out;
    }
    if constexpr (FILL) d[i] = dsum; else rowptr[i] = out;
  }
}

// ---- the frame kernel ---------------------------------------------------------------------------------------------------------
struct ArapArgs {
  const float *V0;
  const int *rowptr, *colind;
  const double *w, *d;
  const int *voff, *hoff, *handles;
  const float *H;
  int64_t nV, nH, T;
  int max_n, frame_begin, frame_count, iters, max_cg;
  double tol;
  float *frames;
  int *cg_iters;
  double *energy;
  int *status;
  double *R_first, *rhs_first;
  double *x, *xs, *r, *Ap, *R;      // workspace: 3, 3, 3, 3, 9 doubles per vertex
  int *fixed;                        // workspace: one flag per vertex
};

// The header's <u v>: every thread brings its serial partial sums; all threads return with the same K totals.
template <int K>
__device__ __forceinline__ void reduce(double (&v)[K], double *red, int &parity) {
  static_assert(K <= kRedMax, "reduction width");
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = v[k] + __shfl_down(v[k], s, 64);
  double *buf = red + parity * (kWaves * kRedMax);
  parity ^= 1;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) buf[(threadIdx.x >> 6) * kRedMax + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double g[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) g[i] = buf[i * kRedMax + k];
#pragma unroll
    for (int s = kWaves / 2; s >= 1; s >>= 1)
#pragma unroll
      for (int i = 0; i < s; ++i) g[i] = g[i] + g[i + s];
    v[k] = g[0];
  }
}

__device__ __forceinline__ double dot3(const double *u, const double *v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ __forceinline__ void cross3(const double *u, const double *v, double *o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ __forceinline__ void matvec3(const double *M, const double *v, double *o) {
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = (M[3 * a] * v[0] + M[3 * a + 1] * v[1]) + M[3 * a + 2] * v[2];
}

// one Jacobi rotation of the pair (P, Q); arp, arq: the entries that couple the third index to p and q
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double (&V)[3][3]) {
  if (apq != 0) {
    const double theta = (aqq - app) / (2 * apq);
    double t = 1 / (fabs(theta) + sqrt(theta * theta + 1));
    if (theta < 0) t = -t;
    const double c = 1 / sqrt(t * t + 1), s = t * c;
    const double napp = app - t * apq, naqq = aqq + t * apq;
    const double narp = c * arp - s * arq, narq = s * arp + c * arq;
    app = napp; aqq = naqq; arp = narp; arq = narq; apq = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double vp = V[k][P], vq = V[k][Q];
      V[k][P] = c * vp - s * vq;
      V[k][Q] = s * vp + c * vq;
    }
  }
}

template <int A, int B>
__device__ __forceinline__ void sort_exchange(double (&lam)[3], double (&V)[3][3]) {
  if (lam[A] < lam[B]) {
    double t = lam[A]; lam[A] = lam[B]; lam[B] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) { t = V[k][A]; V[k][A] = V[k][B]; V[k][B] = t; }
  }
}

// R (row-major 3x3) from S; false: rank below 2, R = I
__device__ bool rotation_from_covariance(const double *S, double *R) {
  double a00 = (S[0] * S[0] + S[3] * S[3]) + S[6] * S[6], a01 = (S[0] * S[1] + S[3] * S[4]) + S[6] * S[7];
  double a02 = (S[0] * S[2] + S[3] * S[5]) + S[6] * S[8], a11 = (S[1] * S[1] + S[4] * S[4]) + S[7] * S[7];
  double a12 = (S[1] * S[2] + S[4] * S[5]) + S[7] * S[8], a22 = (S[2] * S[2] + S[5] * S[5]) + S[8] * S[8];
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < SN_ARAP_JACOBI_SWEEPS; ++sweep) {
    jacobi_rot<0, 1>(a00, a11, a01, a02, a12, V);      // r = 2: (a_20, a_21)
    jacobi_rot<0, 2>(a00, a22, a02, a01, a12, V);      // r = 1: (a_10, a_12)
    jacobi_rot<1, 2>(a11, a22, a12, a01, a02, V);      // r = 0: (a_01, a_02)
  }
  double lam[3] = {a00, a11, a22};
  sort_exchange<0, 1>(lam, V);
  sort_exchange<1, 2>(lam, V);
  sort_exchange<0, 1>(lam, V);
  const double v1[3] = {V[0][0], V[1][0], V[2][0]}, v2[3] = {V[0][1], V[1][1], V[2][1]};
  double v3[3], a1[3], a2[3], u1[3], u2[3], u3[3], a2p[3];
  cross3(v1, v2, v3);
  matvec3(S, v1, a1);
  matvec3(S, v2, a2);
  const double n1 = dot3(a1, a1), l1 = sqrt(n1);
#pragma unroll
  for (int k = 0; k < 3; ++k) u1[k] = a1[k] / l1;
  const double dp = dot3(u1, a2);
#pragma unroll
  for (int k = 0; k < 3; ++k) a2p[k] = a2[k] - dp * u1[k];
  const double n2 = dot3(a2p, a2p), l2 = sqrt(n2);
#pragma unroll
  for (int k = 0; k < 3; ++k) u2[k] = a2p[k] / l2;
  cross3(u1, u2, u3);
  const bool ok = n1 > 0 && n2 > SN_ARAP_RANK_EPS * n1;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[3 * a + b] = ok ? (v1[a] * u1[b] + v2[a] * u2[b]) + v3[a] * u3[b] : (a == b ? 1.0 : 0.0);
  return ok;
}

__global__ __launch_bounds__(kNT) void arap_frames_k(const ArapArgs A) {
  extern __shared__ __align__(16) double arap_lds[];
  double *red = arap_lds;
  double *p = arap_lds + kRedDoubles;      // p[3 i + c], i local
  const int tid = threadIdx.x, m = blockIdx.x;
  const int v0 = A.voff[m], n = A.voff[m + 1] - v0;
  const int h0 = A.hoff[m], h1 = A.hoff[m + 1];
  const int T = (int)A.T, iters = A.iters;
  const int t_end = A.frame_begin + A.frame_count;
  if (v0 < 0 || n <= 0 || (int64_t)v0 + n > A.nV || h0 < 0 || h1 < h0 || h1 > A.nH || n > A.max_n) {
    // nothing to deform, or a mesh this launch has no room for: the frames are the rest pose
    const bool rows = v0 >= 0 && n > 0 && (int64_t)v0 + n <= A.nV;
    for (int t = A.frame_begin; t < t_end; ++t) {
      if (rows)
        for (int i = tid; i < 3 * n; i += kNT) A.frames[((int64_t)t * A.nV + v0) * 3 + i] = A.V0[(int64_t)3 * v0 + i];
      for (int i = tid; i < iters; i += kNT) A.cg_iters[((int64_t)m * T + t) * iters + i] = 0;
      if (tid == 0) A.energy[(int64_t)m * T + t] = 0.0;
    }
    if (tid == 0) A.status[m] = (A.frame_begin == 0 ? 0 : A.status[m]) | (rows ? SN_ARAP_TOO_LARGE : 0);
    return;
  }
  const float *V0 = A.V0 + (int64_t)3 * v0;
  double *x = A.x + (int64_t)3 * v0, *xs = A.xs + (int64_t)3 * v0, *r = A.r + (int64_t)3 * v0, *Ap = A.Ap + (int64_t)3 * v0;
  double *R = A.R + (int64_t)9 * v0;
  int *fixed = A.fixed + v0;
  const int *rowptr = A.rowptr + v0;
  const double *d = A.d + v0;
  int parity = 0, st = 0;

  for (int i = tid; i < n; i += kNT) fixed[i] = 0;
  __syncthreads();
  for (int k = h0 + tid; k < h1; k += kNT) {
    const int h = A.handles[k] - v0;
    if ((unsigned)h < (unsigned)n) fixed[h] = 1;
  }
  if (A.frame_begin == 0)
    for (int i = tid; i < 3 * n; i += kNT) x[i] = (double)V0[i];
  __syncthreads();
  int bad = 0;
  for (int i = tid; i < n; i += kNT) bad |= (!fixed[i] && !(d[i] > 0));
  const bool dbad = __syncthreads_or(bad) != 0;
  if (dbad) {
    st |= SN_ARAP_BREAKDOWN;
    for (int i = tid; i < 9 * n; i += kNT) R[i] = (i % 9) % 4 == 0 ? 1.0 : 0.0;
  }

  for (int t = A.frame_begin; t < t_end; ++t) {
    for (int k = h0 + tid; k < h1; k += kNT) {
      const int h = A.handles[k] - v0;
      if ((unsigned)h < (unsigned)n)
#pragma unroll
        for (int c = 0; c < 3; ++c) x[3 * h + c] = (double)A.H[((int64_t)t * A.nH + k) * 3 + c];
    }
    __syncthreads();
    for (int i = tid; i < n; i += kNT)
#pragma unroll
      for (int c = 0; c < 3; ++c) xs[3 * i + c] = x[3 * i + c];
    bool broken = dbad;
    for (int it = 0; it < iters; ++it) {
      int count = 0;
      if (!broken) {
        // ---- local step: R_i of every row
        for (int i = tid; i < n; i += kNT) {
          double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          const double pi[3] = {(double)V0[3 * i], (double)V0[3 * i + 1], (double)V0[3 * i + 2]};
          const double xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
          for (int o = rowptr[i]; o < rowptr[i + 1]; ++o) {
            const int j = A.colind[o] - v0;
            if ((unsigned)j >= (unsigned)n) continue;
            const double wo = A.w[o];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const double we = wo * (pi[a] - (double)V0[3 * j + a]);
#pragma unroll
              for (int b = 0; b < 3; ++b) S[3 * a + b] = S[3 * a + b] + we * (xi[b] - x[3 * j + b]);
            }
          }
          double Ri[9];
          if (!rotation_from_covariance(S, Ri)) st |= SN_ARAP_DEGENERATE;
#pragma unroll
          for (int k = 0; k < 9; ++k) R[9 * i + k] = Ri[k];
        }
        __syncthreads();
        // ---- right-hand side, start residual and start direction
        double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // rz[3], rr[3], bb[3]
        const bool first = A.R_first != nullptr && t == 0 && it == 0;
        for (int i = tid; i < n; i += kNT) {
          double b[3] = {0.0, 0.0, 0.0}, hs[3] = {0.0, 0.0, 0.0}, off[3] = {0.0, 0.0, 0.0};
          const double pi[3] = {(double)V0[3 * i], (double)V0[3 * i + 1], (double)V0[3 * i + 2]};
          for (int o = rowptr[i]; o < rowptr[i + 1]; ++o) {
            const int j = A.colind[o] - v0;
            if ((unsigned)j >= (unsigned)n) continue;
            const double half = A.w[o] * 0.5;
            double M[9], e[3], v[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = R[9 * i + k] + R[9 * j + k];
#pragma unroll
            for (int a = 0; a < 3; ++a) e[a] = pi[a] - (double)V0[3 * j + a];
            matvec3(M, e, v);
#pragma unroll
            for (int a = 0; a < 3; ++a) b[a] = b[a] + half * v[a];
          }
          if (first) {
#pragma unroll
            for (int k = 0; k < 9; ++k) A.R_first[9 * ((int64_t)v0 + i) + k] = R[9 * i + k];
#pragma unroll
            for (int a = 0; a < 3; ++a) A.rhs_first[3 * ((int64_t)v0 + i) + a] = b[a];
          }
          if (fixed[i]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[3 * i + c] = 0.0;
            continue;
          }
          // handle columns go to the right-hand side (hs continues b), free columns into the product
#pragma unroll
          for (int c = 0; c < 3; ++c) hs[c] = b[c];
          for (int o = rowptr[i]; o < rowptr[i + 1]; ++o) {
            const int j = A.colind[o] - v0;
            if ((unsigned)j >= (unsigned)n) continue;
            const double wo = A.w[o];
            if (fixed[j]) {
#pragma unroll
              for (int c = 0; c < 3; ++c) hs[c] = hs[c] + wo * x[3 * j + c];
            } else {
#pragma unroll
              for (int c = 0; c < 3; ++c) off[c] = off[c] + wo * x[3 * j + c];
            }
          }
          const double di = d[i];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double ri = hs[c] - (di * x[3 * i + c] - off[c]);
            const double zi = ri / di;
            r[3 * i + c] = ri;
            p[3 * i + c] = zi;
            acc[c] = acc[c] + ri * zi;
            acc[3 + c] = acc[3 + c] + ri * ri;
            acc[6 + c] = acc[6 + c] + hs[c] * hs[c];
          }
        }
        reduce<9>(acc, red, parity);
        double rz[3] = {acc[0], acc[1], acc[2]}, thr[3];
        bool conv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          thr[c] = A.tol * sqrt(acc[6 + c]);
          conv[c] = sqrt(acc[3 + c]) <= thr[c];
        }
        // ---- CG: every branch below is taken by all threads alike (its operands come out of reduce)
        bool brk = false;
        for (int cg = 0; cg < A.max_cg; ++cg) {
          if (conv[0] && conv[1] && conv[2]) break;
          double pAp[3] = {0.0, 0.0, 0.0};
          for (int i = tid; i < n; i += kNT) {
            if (fixed[i]) continue;
            double off[3] = {0.0, 0.0, 0.0};
            for (int o = rowptr[i]; o < rowptr[i + 1]; ++o) {
              const int j = A.colind[o] - v0;
              if ((unsigned)j >= (unsigned)n || fixed[j]) continue;
              const double wo = A.w[o];
#pragma unroll
              for (int c = 0; c < 3; ++c) off[c] = off[c] + wo * p[3 * j + c];
            }
            const double di = d[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double pc = p[3 * i + c], ap = di * pc - off[c];
              Ap[3 * i + c] = ap;
              pAp[c] = pAp[c] + pc * ap;
            }
          }
          reduce<3>(pAp, red, parity);
          if ((!conv[0] && !(pAp[0] > 0)) || (!conv[1] && !(pAp[1] > 0)) || (!conv[2] && !(pAp[2] > 0))) {
            brk = true;
            break;
          }
          double alpha[3], acc2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int c = 0; c < 3; ++c) alpha[c] = rz[c] / pAp[c];
          for (int i = tid; i < n; i += kNT) {
            if (fixed[i]) continue;
            const double di = d[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              double ri = r[3 * i + c];
              if (!conv[c]) {
                x[3 * i + c] = x[3 * i + c] + alpha[c] * p[3 * i + c];
                ri = ri - alpha[c] * Ap[3 * i + c];
                r[3 * i + c] = ri;
              }
              const double zi = ri / di;
              acc2[c] = acc2[c] + ri * zi;
              acc2[3 + c] = acc2[3 + c] + ri * ri;
            }
          }
          reduce<6>(acc2, red, parity);
          ++count;
          double beta[3];
          bool run[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            conv[c] = conv[c] || sqrt(acc2[3 + c]) <= thr[c];
            run[c] = !conv[c];
            beta[c] = acc2[c] / rz[c];
            if (run[c]) rz[c] = acc2[c];
          }
          for (int i = tid; i < n; i += kNT) {
            if (fixed[i]) continue;
            const double di = d[i];
#pragma unroll
            for (int c = 0; c < 3; ++c)
              if (run[c]) p[3 * i + c] = r[3 * i + c] / di + beta[c] * p[3 * i + c];
          }
          __syncthreads();
        }
        if (brk) {
          st |= SN_ARAP_BREAKDOWN;
          broken = true;
          for (int i = tid; i < n; i += kNT)
#pragma unroll
            for (int c = 0; c < 3; ++c) x[3 * i + c] = xs[3 * i + c];
        } else if (!(conv[0] && conv[1] && conv[2])) {
          st |= SN_ARAP_NOT_CONVERGED;
        }
        __syncthreads();
      }
      if (tid == 0) A.cg_iters[((int64_t)m * T + t) * iters + it] = count;
    }
    // ---- energy with the rotations of the last local step, and the frame
    double en[1] = {0.0};
    for (int i = tid; i < n; i += kNT) {
      double ei = 0.0;
      const double pi[3] = {(double)V0[3 * i], (double)V0[3 * i + 1], (double)V0[3 * i + 2]};
      for (int o = rowptr[i]; o < rowptr[i + 1]; ++o) {
        const int j = A.colind[o] - v0;
        if ((unsigned)j >= (unsigned)n) continue;
        double e[3], re[3], df[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) e[a] = pi[a] - (double)V0[3 * j + a];
        matvec3(R + 9 * i, e, re);
#pragma unroll
        for (int a = 0; a < 3; ++a) df[a] = (x[3 * i + a] - x[3 * j + a]) - re[a];
        ei = ei + A.w[o] * dot3(df, df);
      }
      en[0] = en[0] + ei;
#pragma unroll
      for (int c = 0; c < 3; ++c) A.frames[((int64_t)t * A.nV + v0 + i) * 3 + c] = (float)x[3 * i + c];
    }
    reduce<1>(en, red, parity);
    if (tid == 0) A.energy[(int64_t)m * T + t] = en[0];
  }
  if (A.frame_begin == 0 && tid == 0) A.status[m] = 0;
  __syncthreads();
  if (st) atomicOr(&A.status[m], st);
}

struct WeightsWs {      // the shared incidence, then nothing of its own
  size_t bytes;
  explicit WeightsWs(int64_t nV, int64_t nF) : bytes(sn_internal_incidence_bytes(nV, nF)) {}
};
struct FramesWs {
  SnCarver c;
  double *x, *xs, *r, *Ap, *R;
  int *fixed;
  FramesWs(void *w, int64_t nV)
      : c(w), x(c.take<double>(3 * nV)), xs(c.take<double>(3 * nV)), r(c.take<double>(3 * nV)), Ap(c.take<double>(3 * nV)),
        R(c.take<double>(9 * nV)), fixed(c.take<int>(nV)) {}
};

}  // namespace

extern "C" {

int64_t sn_arap_max_vertices(void) { return kMaxN; }

size_t sn_arap_weights_workspace_bytes(int64_t nV, int64_t nF) { return WeightsWs(nV < 0 ? 0 : nV, nF < 0 ? 0 : nF).bytes; }

int sn_arap_weights_f64(const float *V0, const int32_t *F, int64_t nV, int64_t nF, int32_t *rowptr, int32_t *colind, double *w,
                        double *d, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 6 * nF > INT_MAX) return SN_E_RANGE;
  if (!rowptr || !status) return SN_E_NULL;
  if (nV > 0 && (!V0 || !d)) return SN_E_NULL;
  if (nF > 0 && (!F || !colind || !w)) return SN_E_NULL;
  if (workspace_bytes < sn_arap_weights_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const int *vptr, *inc;
  int *sums;
  const int st = sn_internal_incidence(F, nV, nF, workspace, status, SN_ARAP_BAD_FACE, &vptr, &inc, &sums, s);
  if (st != SN_OK) return st;
  e = sn_internal_fill(rowptr + nV, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nV > 0) {
    hipLaunchKernelGGL((arap_weight_rows_k<false>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V0, F, nV, vptr, inc, rowptr, (int *)nullptr,
                       (double *)nullptr, (double *)nullptr, status);
  }
  sn_internal_scan_i32(rowptr, nV + 1, rowptr, sums, nullptr, 0, 0, s);
  if (nV > 0)
    hipLaunchKernelGGL((arap_weight_rows_k<true>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V0, F, nV, vptr, inc, rowptr, colind, w, d,
                       status);
  return launch_status();
}

size_t sn_arap_frames_workspace_bytes(int64_t nV) { return FramesWs(nullptr, nV < 0 ? 0 : nV).c.bytes; }

int sn_arap_frames_f64(const float *V0, const int32_t *rowptr, const int32_t *colind, const double *w, const double *d,
                       const int32_t *voff, const int32_t *hoff, const int32_t *handles, const float *H, int64_t B, int64_t nV,
                       int64_t nH, int64_t T, int64_t max_mesh_vertices, int32_t frame_begin, int32_t frame_count, int32_t iters,
                       double tol, int32_t max_cg, float *frames, int32_t *cg_iters, double *energy, int32_t *status,
                       double *R_first, double *rhs_first, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (B < 0 || nV < 0 || nH < 0 || T < 0 || max_mesh_vertices < 0 || frame_begin < 0 || frame_count < 0 || iters < 1 || max_cg < 0)
    return SN_E_SHAPE;
  if ((int64_t)frame_begin + frame_count > T) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || nH > INT_MAX || T > INT_MAX || B > 65535 * 16 || max_cg > SN_ARAP_MAX_CG) return SN_E_RANGE;
  if (max_mesh_vertices > kMaxN) return SN_E_UNSUPPORTED;
  if (!(tol >= 0)) return SN_E_SHAPE;
  if (!R_first != !rhs_first) return SN_E_NULL;
  if (B == 0 || frame_count == 0) return SN_OK;
  if (!voff || !hoff || !rowptr || !frames || !cg_iters || !energy || !status) return SN_E_NULL;
  if (nV > 0 && (!V0 || !d)) return SN_E_NULL;
  if (nH > 0 && (!handles || !H)) return SN_E_NULL;
  if (workspace_bytes < sn_arap_frames_workspace_bytes(nV) || !workspace) return SN_E_WORKSPACE;
  const FramesWs ws(workspace, nV);
  ArapArgs a;
  a.V0 = V0; a.rowptr = rowptr; a.colind = colind; a.w = w; a.d = d;
  a.voff = voff; a.hoff = hoff; a.handles = handles; a.H = H;
  a.nV = nV; a.nH = nH; a.T = T;
  a.max_n = (int)max_mesh_vertices; a.frame_begin = frame_begin; a.frame_count = frame_count; a.iters = iters; a.max_cg = max_cg;
  a.tol = tol;
  a.frames = frames; a.cg_iters = cg_iters; a.energy = energy; a.status = status;
  a.R_first = R_first; a.rhs_first = rhs_first;
  a.x = ws.x; a.xs = ws.xs; a.r = ws.r; a.Ap = ws.Ap; a.R = ws.R; a.fixed = ws.fixed;
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void *>(arap_frames_k), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (attr != hipSuccess) return (int)attr;
  const size_t lds = (size_t)kRedDoubles * 8 + (size_t)24 * (max_mesh_vertices > 0 ? max_mesh_vertices : 1);
  hipLaunchKernelGGL(arap_frames_k, dim3((unsigned)B), dim3(kNT), lds, static_cast<hipStream_t>(stream), a);
  return launch_status();
}

}  // extern "C"

// sn_curvature.hip — principal curvatures and directions from a quadric fitted over the k-ring patch of every vertex (gfx950).
// The definition is the section "Principal curvatures" of sn_spmm.h; mesh_ops.principal_curvatures is its numpy statement and
// this file is its other transcription: fp64 on the widened fp32 coordinates, no contraction, every patch sum serial over
// ascending vertex id, so the two agree bit for bit.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;
constexpr int kWave = 64;                       // one wavefront, one workgroup, one vertex at a time
constexpr int kMaxRing = SN_CURV_MAX_RING;
constexpr int kTable = 2 * kMaxRing;            // open-addressing slots beside the list: never more than kMaxRing + 1 + kWave keys
constexpr int kTableBits = 11;
static_assert(kTable == 1 << kTableBits, "the hash keeps kTableBits bits");
static_assert((kMaxRing & (kMaxRing - 1)) == 0, "the sort pads the list to a power of two inside the list");

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}

struct CurvWs {      // the shared incidence first (it takes the front of the workspace), then what this file adds
  size_t inc_bytes;
  SnCarver c;
  double *normal;    // [nV][3] the unit area-weighted normals in fp64, zero where a vertex has none
  CurvWs(void *w, int64_t nV, int64_t nF)
      : inc_bytes((sn_internal_incidence_bytes(nV, nF) + 15) & ~(size_t)15), c(w ? static_cast<char *>(w) + inc_bytes : nullptr),
        normal(c.take<double>(3 * nV)) {}
  size_t bytes() const { return inc_bytes + c.bytes; }
};

// n_x of the definition: one thread per vertex streams over its sorted incidence list, as desc_vertex_k does for N_area
__global__ __launch_bounds__(kWG) void curv_normals_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                      const int *__restrict__ vptr, const int *__restrict__ inc,
                                                      double *__restrict__ normal) {
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v < nV; v += (int64_t)gridDim.x * kWG) {
    double sx = 0, sy = 0, sz = 0;
    for (int o = vptr[v]; o < vptr[v + 1]; ++o) {
      const int64_t f = inc[o] / 3;
      const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
      const double ix = V[3 * i], iy = V[3 * i + 1], iz = V[3 * i + 2];
      const double ax = (double)V[3 * j] - ix, ay = (double)V[3 * j + 1] - iy, az = (double)V[3 * j + 2] - iz;
      const double bx = (double)V[3 * k] - ix, by = (double)V[3 * k + 1] - iy, bz = (double)V[3 * k + 2] - iz;
      const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
      if (!(sqrt(dot3(nx, ny, nz, nx, ny, nz)) > 0)) continue;      // FLAT
      sx += nx; sy += ny; sz += nz;
    }
    const double len = sqrt(dot3(sx, sy, sz, sx, sy, sz));
    const bool ok = len > 0;
    normal[3 * v] = ok ? sx / len : 0.0;
    normal[3 * v + 1] = ok ? sy / len : 0.0;
    normal[3 * v + 2] = ok ? sz / len : 0.0;
  }
}

struct CurvOut {
  float *k1, *k2, *d1, *d2;
  int *ring_size, *status;
};

// the value of lane j (wave-uniform j) in every lane
__device__ __forceinline__ double lane_value(double x, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), j), hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
  return __hiloint2double(hi, lo);
}

// a vertex that failed: NaN in what was asked for, the patch size, its bit (lane 0)
__device__ __forceinline__ void curv_fail(const CurvOut &o, int64_t v, int size, int bit) {
  const float nan = __int_as_float(0x7FC00000);
  if (o.k1) o.k1[v] = nan;
  if (o.k2) o.k2[v] = nan;
  for (int c = 0; c < 3; ++c) {
    if (o.d1) o.d1[3 * v + c] = nan;
    if (o.d2) o.d2[3 * v + c] = nan;
  }
  if (o.ring_size) o.ring_size[v] = size;
  atomicOr(o.status, bit);
}

// One wavefront per vertex.  The patch is a list of vertex ids in LDS with an open-addressing table beside it: the lanes split a
// level's members, walk their incidence lists and claim new ids with a compare-and-swap; the list is then filtered and sorted,
// and only then does any floating-point sum run — serially over the sorted list, the same value in every lane, so no sum
// depends on how the search found its members.  The workgroup is the wave: its barriers order the LDS accesses and cost nothing.
__global__ __launch_bounds__(kWave) void curv_fit_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                    const int *__restrict__ vptr, const int *__restrict__ inc,
                                                    const double *__restrict__ normal, int radius, CurvOut out) {
  __shared__ int list[kMaxRing];
  __shared__ int table[kTable];
  __shared__ int count;
  const int lane = threadIdx.x;
  volatile int *live_count = &count;

  for (int64_t v64 = blockIdx.x; v64 < nV; v64 += gridDim.x) {
    const int v = (int)v64;
    __syncthreads();
    for (int i = lane; i < kTable; i += kWave) table[i] = -1;
    __syncthreads();
    if (lane == 0) {
      list[0] = v;
      count = 1;
      table[((unsigned)v * 2654435761u) >> (32 - kTableBits)] = v;
    }
    __syncthreads();

    // ---- ring: level by level, the frontier is what the level before appended
    int begin = 0, end = 1;
    bool overflow = false;
    for (int level = 0; level < radius && begin < end && !overflow; ++level) {
      for (int base = begin; base < end && !overflow; base += kWave) {
        const int i = base + lane;
        if (i < end) {
          const int x = list[i];
          for (int o = vptr[x]; o < vptr[x + 1]; ++o) {
            const int code = inc[o], c = code % 3;
            const int64_t f = code / 3;
            const int two[2] = {F[3 * f + (c + 1) % 3], F[3 * f + (c + 2) % 3]};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              if (*live_count > kMaxRing) break;      // overflowed already: the table takes no more keys
              const int key = two[t];
              unsigned slot = ((unsigned)key * 2654435761u) >> (32 - kTableBits);
              for (;;) {
                const int seen = atomicCAS(&table[slot], -1, key);
                if (seen == -1) {
                  const int pos = atomicAdd(&count, 1);
                  if (pos < kMaxRing) list[pos] = key;
                  break;
                }
                if (seen == key) break;
                slot = (slot + 1) & (kTable - 1);
              }
            }
          }
        }
        __syncthreads();
        overflow = count > kMaxRing;
      }
      begin = end;
      end = overflow ? end : count;
    }
    if (overflow) {
      if (lane == 0) curv_fail(out, v, kMaxRing + 1, SN_CURV_OVERFLOW);
      continue;
    }
    int n = count;

    // ---- projection-plane check
    const double nvx = normal[3 * v64], nvy = normal[3 * v64 + 1], nvz = normal[3 * v64 + 2];
    if (!(nvx != 0 || nvy != 0 || nvz != 0)) {
      if (lane == 0) curv_fail(out, v, n, SN_CURV_NO_NORMAL);
      continue;
    }
    int kept = 0;
    unsigned keep_bits = 0;      // bit r: this lane's member of round r stays
    for (int base = 0, r = 0; base < n; base += kWave, ++r) {
      const int i = base + lane;
      bool p = false;
      if (i < n) {
        const int64_t x = list[i];
        p = dot3(normal[3 * x], normal[3 * x + 1], normal[3 * x + 2], nvx, nvy, nvz) > 0;
      }
      keep_bits |= (unsigned)p << r;
      kept += __popcll(__ballot(p));
    }
    if (kept >= SN_CURV_MIN_POINTS && kept < n) {
      int w = 0;
      for (int base = 0, r = 0; base < n; base += kWave, ++r) {
        const int i = base + lane;
        const int x = i < n ? list[i] : 0;
        const bool p = (keep_bits >> r) & 1u;
        const unsigned long long m = __ballot(p);
        __syncthreads();
        if (p) list[w + __popcll(m & ((1ull << lane) - 1))] = x;
        w += __popcll(m);
        __syncthreads();
      }
      n = kept;
    }
    if (n < SN_CURV_MIN_POINTS) {
      if (lane == 0) curv_fail(out, v, n, SN_CURV_FEW_POINTS);
      continue;
    }

    // ---- order: bitonic sort of the list, padded to a power of two with INT_MAX
    int padded = 1;
    while (padded < n) padded <<= 1;
    __syncthreads();
    for (int i = n + lane; i < padded; i += kWave) list[i] = INT_MAX;
    __syncthreads();
    for (int k = 2; k <= padded; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; t < padded / 2; t += kWave) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int a = list[i], b = list[i + j];
          if ((a > b) == ((i & k) == 0)) {
            list[i] = b;
            list[i + j] = a;
          }
        }
        __syncthreads();
      }
    }

    // ---- from here on every lane holds the same values
    const double pvx = V[3 * v64], pvy = V[3 * v64 + 1], pvz = V[3 * v64 + 2];
    double mx = 0, my = 0, mz = 0, h2 = 0;
    for (int j = 0; j < n; ++j) {
      const int64_t x = __builtin_amdgcn_readfirstlane(list[j]);
      mx += normal[3 * x]; my += normal[3 * x + 1]; mz += normal[3 * x + 2];
      const double cx = (double)V[3 * x] - pvx, cy = (double)V[3 * x + 1] - pvy, cz = (double)V[3 * x + 2] - pvz;
      const double cc = dot3(cx, cy, cz, cx, cy, cz);
      if (cc > h2) h2 = cc;
    }
    const double lm = sqrt(dot3(mx, my, mz, mx, my, mz));
    bool degenerate = !(lm > 0);
    mx = mx / lm; my = my / lm; mz = mz / lm;

    // frame: the neighbour of smallest id whose projection has a length
    int best = INT_MAX;
    double tx = 0, ty = 0, tz = 0, lt = 0;
    for (int o = vptr[v]; o < vptr[v + 1]; ++o) {
      const int code = inc[o], c = code % 3;
      const int64_t f = code / 3;
      const int two[2] = {F[3 * f + (c + 1) % 3], F[3 * f + (c + 2) % 3]};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int64_t a = two[t];
        if (a >= best) continue;
        const double cx = (double)V[3 * a] - pvx, cy = (double)V[3 * a + 1] - pvy, cz = (double)V[3 * a + 2] - pvz;
        const double cm = dot3(cx, cy, cz, mx, my, mz);
        const double ux = cx - cm * mx, uy = cy - cm * my, uz = cz - cm * mz;
        const double lu = sqrt(dot3(ux, uy, uz, ux, uy, uz));
        if (lu > 0) {
          best = (int)a;
          tx = ux; ty = uy; tz = uz; lt = lu;
        }
      }
    }
    degenerate = degenerate || !(lt > 0);
    const double e1x = tx / lt, e1y = ty / lt, e1z = tz / lt;
    const double e2x = my * e1z - mz * e1y, e2y = mz * e1x - mx * e1z, e2z = mx * e1y - my * e1x;
    const double h = sqrt(h2);
    degenerate = degenerate || !(h > 0);
    if (degenerate) {
      if (lane == 0) curv_fail(out, v, n, SN_CURV_DEGENERATE);
      continue;
    }

    // ---- normal equations: the lanes compute the local coordinates of 64 members at a time, the sums run over them in order
    double G[5][5], g[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      g[a] = 0;
#pragma unroll
      for (int b = 0; b < 5; ++b) G[a][b] = 0;
    }
    for (int base = 0; base < n; base += kWave) {
      const int i = base + lane;
      double xi = 0, eta = 0, zeta = 0;
      if (i < n) {
        const int64_t x = list[i];
        const double cx = (double)V[3 * x] - pvx, cy = (double)V[3 * x + 1] - pvy, cz = (double)V[3 * x + 2] - pvz;
        xi = dot3(cx, cy, cz, e1x, e1y, e1z) / h;
        eta = dot3(cx, cy, cz, e2x, e2y, e2z) / h;
        zeta = dot3(cx, cy, cz, mx, my, mz) / h;
      }
      const int members = n - base < kWave ? n - base : kWave;
      for (int j = 0; j < members; ++j) {
        const double xj = lane_value(xi, j), ej = lane_value(eta, j), zj = lane_value(zeta, j);
        const double row[5] = {xj * xj, xj * ej, ej * ej, xj, ej};
#pragma unroll
        for (int a = 0; a < 5; ++a) {
#pragma unroll
          for (int b = a; b < 5; ++b) G[a][b] += row[a] * row[b];
          g[a] += zj * row[a];
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 5; ++a) {
#pragma unroll
      for (int b = a + 1; b < 5; ++b) G[b][a] = G[a][b];
    }

    // Cholesky G = L L^T without pivoting, column by column, and the two triangular solves
    double L[5][5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      double d = G[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
      degenerate = degenerate || !(d > SN_CURV_PIVOT_FLOOR * G[j][j]);
      L[j][j] = sqrt(d);
#pragma unroll
      for (int i = j + 1; i < 5; ++i) {
        double x = G[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) x = x - L[i][k] * L[j][k];
        L[i][j] = x / L[j][j];
      }
    }
    if (degenerate) {
      if (lane == 0) curv_fail(out, v, n, SN_CURV_DEGENERATE);
      continue;
    }
    double y[5], q[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      double x = g[i];
#pragma unroll
      for (int k = 0; k < i; ++k) x = x - L[i][k] * y[k];
      y[i] = x / L[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {
      double x = y[i];
#pragma unroll
      for (int k = i + 1; k < 5; ++k) x = x - L[k][i] * q[k];
      q[i] = x / L[i][i];
    }
    const double qa = q[0] / h, qb = q[1] / h, qc = q[2] / h, qd = q[3], qe = q[4];

    // fundamental forms, the symmetric 2 x 2 matrix, its eigenvalues (negated) and eigenvectors
    const double E = 1 + qd * qd, Ff = qd * qe, Gg = 1 + qe * qe;
    const double w = sqrt((1 + qd * qd) + qe * qe);
    const double Lf = (2 * qa) / w, Mf = qb / w, Nf = (2 * qc) / w;
    const double den = E * Gg - Ff * Ff;
    const double s11 = (Lf * Gg - Mf * Ff) / den, s12 = (Mf * E - Lf * Ff) / den, s22 = (Nf * E - Mf * Ff) / den;
    const double tr2 = (s11 + s22) / 2;
    const double df = s11 - s22;
    const double disc = df * df + 4 * (s12 * s12);
    const double rt = sqrt(disc) / 2;
    const double k1 = rt - tr2;
    const double k2 = (0.0 - tr2) - rt;
    if (lane == 0) {
      if (out.k1) out.k1[v64] = (float)k1;
      if (out.k2) out.k2[v64] = (float)k2;
      if (out.ring_size) out.ring_size[v64] = n;
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        float *d = which ? out.d2 : out.d1;
        if (!d) continue;
        const double lam = which ? tr2 + rt : tr2 - rt;
        const bool first = fabs(s11 - lam) >= fabs(s22 - lam);      // the row of S - lambda I with the larger diagonal entry
        double u1 = first ? s12 : lam - s22;
        double u2 = first ? lam - s11 : s12;
        if (u1 < 0 || (u1 == 0 && u2 < 0)) {
          u1 = -u1;
          u2 = -u2;
        }
        double dx = u1 * e1x + u2 * e2x, dy = u1 * e1y + u2 * e2y, dz = u1 * e1z + u2 * e2z;
        const double ld = sqrt(dot3(dx, dy, dz, dx, dy, dz));
        if (disc > 0 && ld > 0) {
          dx = dx / ld; dy = dy / ld; dz = dz / ld;
        } else {      // an umbilic: the frame itself
          dx = which ? e2x : e1x; dy = which ? e2y : e1y; dz = which ? e2z : e1z;
        }
        d[3 * v64] = (float)dx;
        d[3 * v64 + 1] = (float)dy;
        d[3 * v64 + 2] = (float)dz;
      }
    }
  }
}

}  // namespace

extern "C" {

size_t sn_mesh_curvature_workspace_bytes(int64_t nV, int64_t nF) { return CurvWs(nullptr, nV < 0 ? 0 : nV, nF < 0 ? 0 : nF).bytes(); }

int sn_mesh_principal_curvature_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t radius, float *k1, float *k2,
                                    float *d1, float *d2, int32_t *ring_size, int32_t *status, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0 || radius < 1) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!status) return SN_E_NULL;
  if ((nF > 0 && (!V || !F)) || (nV > 0 && !V)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_curvature_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nV == 0) return launch_status();
  const CurvWs ws(workspace, nV, nF);
  const int *vptr, *inc;
  int *sums;
  const int st = sn_internal_incidence(F, nV, nF, workspace, status, SN_DESC_BAD_FACE, &vptr, &inc, &sums, s);
  if (st != SN_OK) return st;
  hipLaunchKernelGGL(curv_normals_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, ws.normal);
  const CurvOut out = {k1, k2, d1, d2, ring_size, status};
  hipLaunchKernelGGL(curv_fit_k, dim3(grid_for(nV, 1)), dim3(kWave), 0, s, V, F, nV, vptr, inc, ws.normal, (int)radius, out);
  return launch_status();
}

}  // extern "C"

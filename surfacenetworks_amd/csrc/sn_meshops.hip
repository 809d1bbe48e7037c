// sn_meshops.hip — device-side construction of the Dirac operators from (V, F)  (gfx950).
// fp64 geometry in the reference's operation order; FMA contraction is switched off for this file so that the
// results round to the same fp32 values as the numpy pipeline (src/utils/mesh.py:17-64).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sn_internal.h"
#include "sn_spmm.h"

namespace {

constexpr int kWG = 256;


// mesh.dist entry: sqrt(((V[a]-V[b])**2).sum())  — (dx² + dy²) + dz², as numpy sums three terms
__device__ __forceinline__ double edge_len(const float *__restrict__ V, int a, int b) {
  const double dx = (double)V[3 * a] - (double)V[3 * b];
  const double dy = (double)V[3 * a + 1] - (double)V[3 * b + 1];
  const double dz = (double)V[3 * a + 2] - (double)V[3 * b + 2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// mesh.area (Heron, 1e-6 floor), src/utils/mesh.py:67-80; also counts incident faces per vertex
__global__ __launch_bounds__(kWG) void face_area_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF,
                                                   double *__restrict__ Af, int *__restrict__ vcount) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    const double lij = edge_len(V, i, j), ljk = edge_len(V, j, k), lki = edge_len(V, k, i);
    const double s = ((lij + ljk) + lki) / 2;
    const double q = ((s * (s - lij)) * (s - ljk)) * (s - lki);
    Af[f] = q > 0 ? sqrt(q) : 1e-6;
    atomicAdd(&vcount[i], 1);
    atomicAdd(&vcount[j], 1);
    atomicAdd(&vcount[k], 1);
  }
}

// a face contributes its three corners only when its indices are three distinct vertices of the mesh
__device__ __forceinline__ bool face_ok(int i, int j, int k, int64_t nV) {
  return (unsigned)i < (unsigned)nV && (unsigned)j < (unsigned)nV && (unsigned)k < (unsigned)nV && i != j && j != k && k != i;
}

// ---- buckets by vertex: count into a zeroed ptr[0..nV], bucket_offsets, fill through the atomic cursor ------------------------
// A bucket holds codes CODE * face + corner.  KEY: the bucket of corner c is its own vertex (kCornerVertex: the side that starts
// there) or the lower end of the side c -> c + 1 (kLowerEnd).  FILTER: which faces take part.  The order inside a bucket is the
// order of the atomics: a reader that depends on it sorts the bucket (sort_run), the others say why they do not.
enum BucketKey { kCornerVertex, kLowerEnd };
enum BucketFilter { kEveryFace, kGoodFaces, kGoodKeptFaces };      // kGoodKeptFaces: face_ok and keep[f] != 0

template <BucketKey KEY>
__device__ __forceinline__ int bucket_of(const int (&v)[3], int c) {
  return KEY == kCornerVertex ? v[c] : min(v[c], v[(c + 1) % 3]);
}
// false: the face takes no part; *bad: because it failed face_ok (a face that is not kept is not looked at)
template <BucketFilter FILTER>
__device__ __forceinline__ bool bucket_takes(const int (&v)[3], const int *__restrict__ keep, int64_t f, int64_t nV, bool *bad) {
  *bad = false;
  if (FILTER == kEveryFace) return true;
  if (FILTER == kGoodKeptFaces && keep[f] == 0) return false;
  *bad = !face_ok(v[0], v[1], v[2], nV);
  return !*bad;
}

// status_bit is raised in *status (when there is one) for a face that fails face_ok
template <BucketKey KEY, BucketFilter FILTER>
__global__ __launch_bounds__(kWG) void bucket_count_k(const int *__restrict__ F, const int *__restrict__ keep, int64_t nF, int64_t nV,
                                                      int *__restrict__ count, int *__restrict__ status, int status_bit) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int v[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
    bool bad;
    if (!bucket_takes<FILTER>(v, keep, f, nV, &bad)) {
      if (bad && status) atomicOr(status, status_bit);
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(&count[bucket_of<KEY>(v, c)], 1);
  }
}
template <BucketKey KEY, BucketFilter FILTER, int CODE>
__global__ __launch_bounds__(kWG) void bucket_fill_k(const int *__restrict__ F, const int *__restrict__ keep, int64_t nF, int64_t nV,
                                                     int *__restrict__ cursor, int *__restrict__ bucket) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int v[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
    bool bad;
    if (!bucket_takes<FILTER>(v, keep, f, nV, &bad)) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) bucket[atomicAdd(&cursor[bucket_of<KEY>(v, c)], 1)] = (int)(CODE * f + c);
  }
}

// counts in ptr[0..nV) and a zero at nV -> the buckets' offsets, in place, and the cursor the fill advances (a copy)
inline int bucket_offsets(int *ptr, int *cursor, int *sums, int64_t nV, hipStream_t s) {
  sn_internal_scan_i32(ptr, nV + 1, ptr, sums, nullptr, 0, 0, s);
  const hipError_t e = sn_internal_copy2d(cursor, 0, ptr, 0, (int64_t)((size_t)(nV + 1) * sizeof(int)), 1, s);
  return e == hipSuccess ? SN_OK : (int)e;
}

// sort each vertex's list, write DiA's block columns, and Av_j = sum_{incident faces, ascending} Af/3 (mesh.py:43-45)
__global__ __launch_bounds__(kWG) void vertex_lists_k(const int *__restrict__ vptr, int64_t nV, int *__restrict__ inc,
                                                      const double *__restrict__ Af, double *__restrict__ Av,
                                                      int *__restrict__ dia_colind) {
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v < nV; v += (int64_t)gridDim.x * kWG) {
    const int b = vptr[v], e = vptr[v + 1];
    sort_run(inc, b, e);
    double a = 0;
    for (int i = b; i < e; ++i) {
      a += Af[inc[i] >> 2] / 3;
      dia_colind[i] = inc[i] >> 2;
    }
    Av[v] = a;
  }
}

__global__ __launch_bounds__(kWG) void vertex_sort_k(const int *__restrict__ vptr, int64_t nV, int *__restrict__ inc) {
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v < nV; v += (int64_t)gridDim.x * kWG) sort_run(inc, vptr[v], vptr[v + 1]);
}

// the 4x4 block  -Q(0,e)/(2Af)  (mesh.py:28-33,55-58), row-major, as doubles
__device__ __forceinline__ void dirac_block(const float *__restrict__ V, const int *__restrict__ F, int64_t f, int c,
                                            double Af, double *m /*16*/) {
  const int a = F[3 * f + (c + 1) % 3], b = F[3 * f + (c + 2) % 3];
  const double ex = (double)V[3 * a] - (double)V[3 * b];
  const double ey = (double)V[3 * a + 1] - (double)V[3 * b + 1];
  const double ez = (double)V[3 * a + 2] - (double)V[3 * b + 2];
  const double sc = 2 * Af;
  // Q(0,b,c,d) = [[0,-b,-c,-d],[b,0,-d,c],[c,d,0,-b],[d,-c,b,0]];  entry = -(q)/(2Af)
  const double q[16] = {0.0, -ex, -ey, -ez, ex, 0.0, -ez, ey, ey, ez, 0.0, -ex, ez, -ey, ex, 0.0};
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = -q[i] / sc;
}

// Di (block row = face) and DiAT (same structure, blocks = (DiA block)^T = D_block * Af/Av)
__global__ __launch_bounds__(kWG) void di_fill_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF,
                                                 const double *__restrict__ Af, const double *__restrict__ Av,
                                                 int *__restrict__ di_rowptr, int *__restrict__ di_colind,
                                                 float *__restrict__ di_vals, float *__restrict__ diat_vals) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f <= nF; f += (int64_t)gridDim.x * kWG) {
    di_rowptr[f] = (int)(3 * f);
    if (f == nF) break;
    int c0 = 0, c1 = 1, c2 = 2;                        // corners ordered by vertex id (block columns ascending)
    int v0 = F[3 * f], v1 = F[3 * f + 1], v2 = F[3 * f + 2];
#define SN_SWAP(a, b, x, y) if (a > b) { int t = a; a = b; b = t; t = x; x = y; y = t; }
    SN_SWAP(v0, v1, c0, c1) SN_SWAP(v1, v2, c1, c2) SN_SWAP(v0, v1, c0, c1)
#undef SN_SWAP
    const int vs[3] = {v0, v1, v2}, cs[3] = {c0, c1, c2};
    const double af = Af[f];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      double m[16];
      dirac_block(V, F, f, cs[s], af, m);
      const int64_t o = 3 * f + s;
      di_colind[o] = vs[s];
      const double av = Av[vs[s]];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        di_vals[16 * o + i] = (float)m[i];
        diat_vals[16 * o + i] = (float)((m[i] * af) / av);      // (mat.T * Af / Av) transposed back
      }
    }
  }
}

// DiA (block row = vertex) = D_block^T * Af/Av, and DiT = D_block^T (same structure)
__global__ __launch_bounds__(kWG) void dia_fill_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                  const int *__restrict__ vptr, const int *__restrict__ inc,
                                                  const double *__restrict__ Af, const double *__restrict__ Av,
                                                  int *__restrict__ dia_rowptr, float *__restrict__ dia_vals,
                                                  float *__restrict__ dit_vals) {
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v <= nV; v += (int64_t)gridDim.x * kWG) {
    dia_rowptr[v] = vptr[v];
    if (v == nV) break;
    const double av = Av[v];
    for (int o = vptr[v]; o < vptr[v + 1]; ++o) {
      const int64_t f = inc[o] >> 2;
      const int c = inc[o] & 3;
      const double af = Af[f];
      double m[16];
      dirac_block(V, F, f, c, af, m);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double t = m[4 * k + r];                          // transpose
          dit_vals[16 * (int64_t)o + 4 * r + k] = (float)t;
          dia_vals[16 * (int64_t)o + 4 * r + k] = (float)((t * af) / av);
        }
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Cotangent Laplacian, vertex-centric.  Thread i walks its incident faces (ascending face id) and builds, for every
// neighbour j, W[i,j] (row i's value) and W[j,i] (row j's value, needed for the column sum d_i) from the same face data,
// exactly as the reference's permutation loop does:  (-l_pq^2 + l_qr^2 + l_rp^2) / (8 a + 1e-6)  for (p,q,r) = (i,j,k).
// ------------------------------------------------------------------------------------------------
constexpr int kMaxDeg = SN_LAP_MAX_DEGREE;

template <bool FILL>
__global__ __launch_bounds__(kWG) void laplacian_rows_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                        const int *__restrict__ vptr, const int *__restrict__ inc,
                                                        const double *__restrict__ Af, int *__restrict__ rowptr,
                                                        int *__restrict__ colind, float *__restrict__ vals,
                                                        int *__restrict__ status_flag) {
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < nV; i += (int64_t)gridDim.x * kWG) {
    const int b = vptr[i], e = vptr[i + 1];
    if (e - b > kMaxDeg) {
      if (status_flag) atomicExch(status_flag, 1);
      if constexpr (!FILL) rowptr[i] = 1;
      continue;
    }
    int nb[2 * kMaxDeg];          // neighbour ids (with duplicates), in face order
    double wij[2 * kMaxDeg];      // contribution to W[i, nb]
    double wji[2 * kMaxDeg];      // contribution to W[nb, i]
    int n = 0;
    double A = 0;
    for (int o = b; o < e; ++o) {
      const int64_t f = inc[o] >> 2;
      const int c = inc[o] & 3;
      const int j = F[3 * f + (c + 1) % 3], k = F[3 * f + (c + 2) % 3];
      const double lij = edge_len(V, (int)i, j), ljk = edge_len(V, j, k), lki = edge_len(V, k, (int)i);
      const double a2 = lij * lij, b2 = ljk * ljk, c2 = lki * lki;
      const double den = 8 * Af[f] + 1e-6;
      // permutations (i,j,k): W[i,j];  (i,k,j): W[i,k];  (j,i,k): W[j,i];  (k,i,j): W[k,i]
      nb[n] = j; wij[n] = ((-a2 + b2) + c2) / den; wji[n] = ((-a2 + c2) + b2) / den; ++n;
      nb[n] = k; wij[n] = ((-c2 + b2) + a2) / den; wji[n] = ((-c2 + a2) + b2) / den; ++n;
      const double t = Af[f] / 3 / 4;
      A += t;
      A += t;
    }
    sort_run(nb, 0, n, wij, wji);      // by neighbour id; stable: keeps face order among duplicates
    // merge duplicates; d_i = sum over neighbours (ascending) of W[nb, i]; entries with W[i,nb] == 0 are dropped
    const double ainv = 1 / (A + 1e-9);
    double d = 0;
    int cnt = 0;
    int out = FILL ? rowptr[i] : 0;
    bool diag_done = false;
    for (int x = 0; x < n;) {
      const int kn = nb[x];
      double w = 0, wt = 0;
      while (x < n && nb[x] == kn) { w += wij[x]; wt += wji[x]; ++x; }
      if (wt != 0) d += wt;
      if (w != 0) {
        if constexpr (FILL) {
          if (!diag_done && kn > i) { ++out; diag_done = true; }          // leave the diagonal slot, filled below
          colind[out] = kn;
          vals[out] = (float)(ainv * (0 - w));
          ++out;
        }
        ++cnt;
      }
    }
    if constexpr (FILL) {
      // diagonal position: after the neighbours smaller than i
      int pos = rowptr[i];
      for (int x = 0, seen = -1; x < n; ++x) {
        if (nb[x] == seen) continue;
        seen = nb[x];
        double w = 0;
        for (int y = x; y < n && nb[y] == seen; ++y) w += wij[y];
        if (w != 0 && seen < i) ++pos;
      }
      colind[pos] = (int)i;
      vals[pos] = (float)(ainv * d);
    } else {
      rowptr[i] = cnt + 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Geodesic (edge-path) distance matrices: all-pairs shortest paths on a CSR graph, fp32 (definition: sn_spmm.h).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWG) void edge_lengths_csr_k(const float *__restrict__ V, const int *__restrict__ rowptr,
                                                          const int *__restrict__ colind, int64_t n, float *__restrict__ w) {
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v < n; v += (int64_t)gridDim.x * kWG)
    for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
      const int u = colind[e];
      w[e] = ((unsigned)u < (unsigned)n) ? (float)edge_len(V, (int)v, u) : INFINITY;   // a column outside the mesh: no edge
    }
}

constexpr int kApspLds = 160 * 1024;      // the CU's whole LDS: one workgroup may take it all
constexpr int kApspHead = 16;             // three rotating "changed" flags, padded so that the vectors stay 16-byte aligned
constexpr int kApspMaxN = (kApspLds - kApspHead) / 4;
constexpr int kApspMaxWG = 1024;

// S: sources per workgroup — the largest of {8, 4, 2, 1} whose S distance vectors fit the LDS
inline int apsp_group(int64_t n) {
  for (int S = 8; S > 1; S >>= 1)
    if (S * n <= kApspMaxN) return S;
  return n <= kApspMaxN ? 1 : 0;
}
// threads per workgroup: 16 waves when the vectors leave room for one workgroup per CU, 8 for two, 4 for more (then
// several small workgroups share the CU and none of them leaves it with one or two waves)
inline int apsp_threads(int64_t n) {
  const int S = apsp_group(n);
  if (!S) return 0;
  const int64_t per_cu = kApspLds / (kApspHead + 4 * S * (n > 0 ? n : 1));
  return per_cu <= 1 ? 1024 : per_cu == 2 ? 512 : 256;
}

// Pull sweeps to the fixed point of d[v] = min(d[v], min_u fl(d[u] + w_uv)).  d[v*S + j]: distance from source s0 + j, in
// LDS; the owner of v (thread v mod blockDim) is the only writer of d[v*S..]; a neighbour's word is read either old or new,
// both are lengths of real paths, and fp32 addition of w >= 0 is monotone, so the fixed point does not depend on the order.
// At most n sweeps whatever the arrays hold (NaN and negative weights included): sweep k settles every k-hop path.
template <int S>
__global__ __launch_bounds__(kApspMaxWG) void graph_apsp_k(const int *__restrict__ rowptr, const int *__restrict__ colind,
                                                            const float *__restrict__ w, int n, int src_begin, int src_count,
                                                            float *__restrict__ out, int64_t ldo, int *__restrict__ unreached,
                                                            int *__restrict__ sweeps) {
  extern __shared__ __align__(16) unsigned char apsp_lds[];
  int *flag = reinterpret_cast<int *>(apsp_lds);
  float *d = reinterpret_cast<float *>(apsp_lds + kApspHead);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int s0 = src_begin + (int)blockIdx.x * S;
  const int ns = min(S, src_begin + src_count - s0);           // the last group of a window may be partial
  for (int i = tid; i < n * S; i += nt) d[i] = INFINITY;
  if (tid < 3) flag[tid] = 0;
  __syncthreads();
  if (tid < ns) d[(s0 + tid) * S + tid] = 0.0f;
  __syncthreads();
  int it = 0;
  if (colind != nullptr)
    for (; it < n; ++it) {
      if (tid == 0) flag[(it + 1) % 3] = 0;                    // read last before the previous barrier, set next after this one
      bool changed = false;
      for (int v = tid; v < n; v += nt) {
        float cur[S], best[S];
#pragma unroll
        for (int j = 0; j < S; ++j) best[j] = cur[j] = d[v * S + j];
        const int eb = rowptr[v], ee = rowptr[v + 1];
        for (int e = eb; e < ee; ++e) {
          const int u = colind[e];
          const float we = w[e];
          if ((unsigned)u >= (unsigned)n) continue;            // never index LDS by a column the graph does not have
#pragma unroll
          for (int j = 0; j < S; ++j) best[j] = fminf(best[j], d[u * S + j] + we);
        }
#pragma unroll
        for (int j = 0; j < S; ++j)
          if (best[j] < cur[j]) {
            d[v * S + j] = best[j];
            changed = true;
          }
      }
      if (changed) flag[it % 3] = 1;
      __syncthreads();
      if (!flag[it % 3]) break;
    }
  if (sweeps != nullptr && tid == 0) sweeps[blockIdx.x] = it < n ? it + 1 : n;
  bool inf_left = false;
  for (int j = 0; j < ns; ++j) {
    float *row = out + (int64_t)(s0 - src_begin + j) * ldo;
    for (int v = tid; v < n; v += nt) {
      const float x = d[v * S + j];
      inf_left |= (x == INFINITY);
      __builtin_nontemporal_store(x, row + v);
    }
  }
  if (inf_left && unreached != nullptr) atomicOr(unreached, 1);
}

// G[i][j] = G[j][i] = min(G[i][j], G[j][i]) in place: block (bi <= bj) holds tiles (bi,bj) and (bj,bi) in LDS, then writes both
constexpr int kSymTile = 32;
__global__ __launch_bounds__(kWG) void symmetrize_min_k(float *__restrict__ G, int64_t n, int64_t ld) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  __shared__ float a[kSymTile][kSymTile + 1], b[kSymTile][kSymTile + 1];
  const int tx = threadIdx.x % kSymTile, ty = threadIdx.x / kSymTile;
  const int64_t i0 = (int64_t)bi * kSymTile, j0 = (int64_t)bj * kSymTile;
  for (int r = ty; r < kSymTile; r += kWG / kSymTile) {
    a[r][tx] = (i0 + r < n && j0 + tx < n) ? G[(i0 + r) * ld + j0 + tx] : INFINITY;
    b[r][tx] = (j0 + r < n && i0 + tx < n) ? G[(j0 + r) * ld + i0 + tx] : INFINITY;
  }
  __syncthreads();
  for (int r = ty; r < kSymTile; r += kWG / kSymTile) {
    if (i0 + r < n && j0 + tx < n) G[(i0 + r) * ld + j0 + tx] = fminf(a[r][tx], b[tx][r]);
    if (bi != bj && j0 + r < n && i0 + tx < n) G[(j0 + r) * ld + i0 + tx] = fminf(b[r][tx], a[tx][r]);
  }
}

template <int S>
int apsp_launch(const int *rowptr, const int *colind, const float *w, int n, int src_begin, int src_count, float *out,
                int64_t ldo, int *unreached, int *sweeps, hipStream_t s) {
  const size_t lds = (size_t)kApspHead + (size_t)4 * S * n;
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void *>(graph_apsp_k<S>), hipFuncAttributeMaxDynamicSharedMemorySize, kApspLds);
  if (attr != hipSuccess) return (int)attr;
  hipLaunchKernelGGL((graph_apsp_k<S>), dim3((unsigned)((src_count + S - 1) / S)), dim3(apsp_threads(n)), lds, s, rowptr, colind, w,
                     n, src_begin, src_count, out, ldo, unreached, sweeps);
  return launch_status();
}

// ------------------------------------------------------------------------------------------------
// Geodesic distance matrices that cross triangles: first-order Eikonal sweeps (definition: sn_spmm.h).
// ------------------------------------------------------------------------------------------------
struct MeshCorner {      // (v; a, b): the record of the header, 40 bytes
  int a, b;
  float la, lb;
  double c, sb, h;
};
static_assert(sizeof(MeshCorner) == SN_MESH_CORNER_BYTES, "corner record layout");

// the records of the good faces, scattered through the cursor of their corner-vertex buckets
__global__ __launch_bounds__(kWG) void corner_fill_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF, int64_t nV,
                                                     int *__restrict__ cursor, MeshCorner *__restrict__ rec) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int idx[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
    if (!face_ok(idx[0], idx[1], idx[2], nV)) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int v = idx[k], a = idx[(k + 1) % 3], b = idx[(k + 2) % 3];
      const double ex = (double)V[3 * a] - (double)V[3 * b], ey = (double)V[3 * a + 1] - (double)V[3 * b + 1],
                   ez = (double)V[3 * a + 2] - (double)V[3 * b + 2];
      const double qx = (double)V[3 * b] - (double)V[3 * v], qy = (double)V[3 * b + 1] - (double)V[3 * v + 1],
                   qz = (double)V[3 * b + 2] - (double)V[3 * v + 2];
      const double nx = qy * ez - qz * ey, ny = qz * ex - qx * ez, nz = qx * ey - qy * ex;
      MeshCorner r;
      r.a = a;
      r.b = b;
      r.la = (float)edge_len(V, v, a);
      r.lb = (float)edge_len(V, v, b);
      r.c = sqrt((ex * ex + ey * ey) + ez * ez);
      r.sb = ((qx * ex + qy * ey) + qz * ez) / r.c;
      r.h = sqrt((nx * nx + ny * ny) + nz * nz) / r.c;
      rec[atomicAdd(&cursor[v], 1)] = r;
    }
  }
}

// graph_apsp_k with a richer candidate set: thread t owns vertices t, t + threads, ... and loops over their corners; a
// corner's constants are loaded once and applied to all S sources.  Same LDS layout, flags, barrier and single-writer rule.
// A neighbour's word is read old or new; both are upper bounds that some path realises, so what a sweep writes is one too,
// and a sweep that changed nothing has read only final values: the result is a fixed point of the header's update.
template <int S>
__global__ __launch_bounds__(kApspMaxWG) void mesh_geodesics_k(const int *__restrict__ cptr, const MeshCorner *__restrict__ rec, int n,
                                                                int src_begin, int src_count, float *__restrict__ out, int64_t ldo,
                                                                int *__restrict__ flags, int *__restrict__ sweeps) {
  extern __shared__ __align__(16) unsigned char apsp_lds[];
  int *flag = reinterpret_cast<int *>(apsp_lds);
  float *d = reinterpret_cast<float *>(apsp_lds + kApspHead);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int s0 = src_begin + (int)blockIdx.x * S;
  const int ns = min(S, src_begin + src_count - s0);
  for (int i = tid; i < n * S; i += nt) d[i] = INFINITY;
  if (tid < 3) flag[tid] = 0;
  __syncthreads();
  if (tid < ns) d[(s0 + tid) * S + tid] = 0.0f;
  __syncthreads();
  int it = 0;
  if (rec != nullptr)
    for (; it < n; ++it) {
      if (tid == 0) flag[(it + 1) % 3] = 0;
      bool changed = false;
      for (int v = tid; v < n; v += nt) {
        float cur[S], best[S];
#pragma unroll
        for (int j = 0; j < S; ++j) best[j] = cur[j] = d[v * S + j];
        const int cb = cptr[v], ce = cptr[v + 1];
        for (int e = cb; e < ce; ++e) {
          const MeshCorner k = rec[e];
          if ((unsigned)k.a >= (unsigned)n || (unsigned)k.b >= (unsigned)n) continue;      // never index LDS by a vertex the mesh does not have
          const bool tri = k.c > 0 && k.h > 0;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float da = d[k.a * S + j], db = d[k.b * S + j];
            float cand = fminf(da + k.la, db + k.lb);
            const double delta = (double)da - (double)db;
            if (tri && fabs(delta) < k.c) {                       // false for a NaN or infinite delta
              const double r = sqrt((k.c - delta) * (k.c + delta));
              const double m = -(k.h * delta);
              if (k.sb * r <= m && m <= (k.sb + k.c) * r) cand = fminf(cand, (float)((double)db + (k.h * r - k.sb * delta) / k.c));
            }
            best[j] = fminf(best[j], cand);
          }
        }
#pragma unroll
        for (int j = 0; j < S; ++j)
          if (best[j] < cur[j]) {
            d[v * S + j] = best[j];
            changed = true;
          }
      }
      if (changed) flag[it % 3] = 1;
      __syncthreads();
      if (!flag[it % 3]) break;
    }
  if (sweeps != nullptr && tid == 0) sweeps[blockIdx.x] = it < n ? it + 1 : n;
  bool inf_left = false;
  for (int j = 0; j < ns; ++j) {
    float *row = out + (int64_t)(s0 - src_begin + j) * ldo;
    for (int v = tid; v < n; v += nt) {
      const float x = d[v * S + j];
      inf_left |= (x == INFINITY);
      __builtin_nontemporal_store(x, row + v);
    }
  }
  if (flags != nullptr) {
    if (inf_left) atomicOr(flags, 1);
    if (it == n && tid == 0) atomicOr(flags, 2);                  // the n-th sweep still changed something
  }
}

template <int S>
int mesh_geodesics_launch(const int *cptr, const MeshCorner *rec, int n, int src_begin, int src_count, float *out, int64_t ldo,
                          int *flags, int *sweeps, hipStream_t s) {
  const size_t lds = (size_t)kApspHead + (size_t)4 * S * n;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(mesh_geodesics_k<S>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, kApspLds);
  if (attr != hipSuccess) return (int)attr;
  hipLaunchKernelGGL((mesh_geodesics_k<S>), dim3((unsigned)((src_count + S - 1) / S)), dim3(apsp_threads(n)), lds, s, cptr, rec, n,
                     src_begin, src_count, out, ldo, flags, sweeps);
  return launch_status();
}

// ------------------------------------------------------------------------------------------------
// Intrinsic Delaunay triangulation by edge flips, and the Laplacian on it (definition: sn_spmm.h).  The state is keyed by face
// sides (code 3 f + s).  No LDS and no corner table on purpose: the working set is 1-2 MB at FAUST size and the access is
// pointer chasing through the glue map.
// ------------------------------------------------------------------------------------------------
constexpr int kIdtRefused = SN_IDT_BAD_FACE | SN_IDT_NON_MANIFOLD | SN_IDT_ORIENTATION;
typedef unsigned long long idt_claim_t;

// The sides are bucketed by the vertex they start at (kCornerVertex over the good faces).
// twin of the side a -> b: the one side b -> a in b's bucket.  The order inside a bucket (atomic cursor) does not matter: a
// twin is stored only when it is the only candidate.
__global__ __launch_bounds__(kWG) void glue_twin_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF, int64_t nV,
                                                   const int *__restrict__ ptr, const int *__restrict__ bucket, int *__restrict__ G,
                                                   double *__restrict__ l, int *__restrict__ status) {
  for (int64_t c = (int64_t)blockIdx.x * kWG + threadIdx.x; c < 3 * nF; c += (int64_t)gridDim.x * kWG) {
    const int64_t f = c / 3;
    const int s = (int)(c - 3 * f);
    const int idx[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
    if (!face_ok(idx[0], idx[1], idx[2], nV)) {
      G[c] = -1;
      if (l) l[c] = 0;
      continue;
    }
    const int a = F[c], b = F[3 * f + (s + 1) % 3];
    if (l) l[c] = edge_len(V, a, b);
    int opp = 0, same = 0, twin = -1;
    for (int e = ptr[b]; e < ptr[b + 1]; ++e) {
      const int d = bucket[e];
      if (F[3 * (d / 3) + (d % 3 + 1) % 3] == a) { ++opp; twin = d; }
    }
    for (int e = ptr[a]; e < ptr[a + 1]; ++e) {
      const int d = bucket[e];
      if (d != (int)c && F[3 * (d / 3) + (d % 3 + 1) % 3] == b) ++same;
    }
    if (1 + opp + same > 2) atomicOr(status, SN_IDT_NON_MANIFOLD);
    else if (same) atomicOr(status, SN_IDT_ORIENTATION);
    G[c] = (opp == 1 && same == 0) ? twin : -1;
  }
}

// cot of the angle opposite side s of face f, (b^2 + c^2 - a^2) / (4 A), A by Heron; false for a degenerate face
__device__ __forceinline__ bool idt_cot(const double *l, int f, int s, double *cot) {
  const double a = l[3 * f + s], b = l[3 * f + (s + 1) % 3], c = l[3 * f + (s + 2) % 3];
  const double h = ((a + b) + c) / 2;
  const double q = ((h * (h - a)) * (h - b)) * (h - c);
  if (!(q > 0)) return false;
  *cot = ((b * b + c * c) - a * a) / (4 * sqrt(q));
  return true;
}

// Claim word of side c in a round: [20 bits: 0xFFFFF - round | 12 bits: hash(c, round) | 32 bits: c].  A later round's word is
// smaller than any stale one; within a round the order is a per-round shuffle of the side codes, unique because c is in it.
// With the bare code as the priority the losers form chains along the face numbering (a side waits for a smaller one that is
// itself waiting): 1569 rounds on torus_grid(65, 106, jitter=0.8) against 27 with the shuffle (LABNOTES.md#intrinsic).
constexpr int kIdtMaxRounds = 1 << 20;
__device__ __forceinline__ idt_claim_t idt_claim_word(unsigned round, int c) {
  unsigned h = (unsigned)c * 2654435761u + round * 40503u;
  h = (h ^ (h >> 15)) * 2246822519u;
  return ((idt_claim_t)(0xFFFFFu - round) << 44) | ((idt_claim_t)(h >> 20) << 32) | (unsigned)c;
}

// First launch of a round: one thread per interior side with c < G[c].  A non-Delaunay side writes its word by integer min into
// the claim of its two faces and of the up to four faces across their outer sides.  Reads l and G, writes neither.
__global__ __launch_bounds__(kWG) void idt_claim_k(const double *__restrict__ l, const int *__restrict__ G, int64_t nS,
                                                   idt_claim_t *__restrict__ claim, unsigned round, int last,
                                                   int *__restrict__ counters, int *__restrict__ status) {
  if (*status & kIdtRefused) return;
  for (int64_t c64 = (int64_t)blockIdx.x * kWG + threadIdx.x; c64 < nS; c64 += (int64_t)gridDim.x * kWG) {
    const int c = (int)c64, p = G[c];
    if (p <= c || (int64_t)p >= nS) continue;
    const int f = c / 3, g = p / 3, s = c % 3, t = p % 3;
    if (f == g) continue;                              // a face glued to itself along this edge: always Delaunay, never flipped
    double cf, cg;
    const bool okf = idt_cot(l, f, s, &cf), okg = idt_cot(l, g, t, &cg);
    if (!okf || !okg) {
      atomicOr(status, SN_IDT_DEGENERATE);
      continue;
    }
    if (!(cf + cg < SN_IDT_THRESHOLD)) continue;
    const idt_claim_t w = idt_claim_word(round, c);
    atomicMin(&claim[f], w);
    atomicMin(&claim[g], w);
    const int outer[4] = {3 * f + (s + 1) % 3, 3 * f + (s + 2) % 3, 3 * g + (t + 1) % 3, 3 * g + (t + 2) % 3};
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int q = G[outer[x]];
      if (q >= 0 && (int64_t)q < nS) atomicMin(&claim[q / 3], w);
    }
    atomicAdd(&counters[0], 1);
    if (last) atomicOr(status, SN_IDT_NOT_CONVERGED);
  }
}

// Second launch: the side that holds every one of its claims flips; it is then the only thread of the round that reads or
// writes those faces (a face is written only by the holder of its claim, and the claims are not written here).
__global__ __launch_bounds__(kWG) void idt_flip_k(int *F, double *l, int *G, int64_t nS, const idt_claim_t *__restrict__ claim,
                                                  unsigned round, int *__restrict__ counters, const int *__restrict__ status) {
  if (*status & kIdtRefused) return;
  for (int64_t c64 = (int64_t)blockIdx.x * kWG + threadIdx.x; c64 < nS; c64 += (int64_t)gridDim.x * kWG) {
    const int c = (int)c64, f = c / 3, s = c % 3;
    const idt_claim_t w = idt_claim_word(round, c);
    if (claim[f] != w) continue;                       // only a side that claimed in this round can find its own word
    const int p = G[c];
    if (p < 0 || (int64_t)p >= nS) continue;
    const int g = p / 3, t = p % 3;
    if (claim[g] != w) continue;
    const int s1 = (s + 1) % 3, s2 = (s + 2) % 3, t1 = (t + 1) % 3, t2 = (t + 2) % 3;
    const int oldc[4] = {3 * f + s1, 3 * f + s2, 3 * g + t1, 3 * g + t2};
    const int newc[4] = {3 * g + 1, 3 * f, 3 * f + 1, 3 * g};
    int part[4];
    bool held = true;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      part[x] = G[oldc[x]];
      if (part[x] >= 0 && (int64_t)part[x] < nS && claim[part[x] / 3] != w) held = false;
    }
    if (!held) continue;
    // f = (i, j, k), g = (j, i, m)  ->  f = (k, i, m), g = (m, j, k)
    const int i = F[3 * f + s], j = F[3 * f + s1], k = F[3 * f + s2], m = F[3 * g + t2];
    const double a = l[3 * f + s], ljk = l[3 * f + s1], lki = l[3 * f + s2], lim = l[3 * g + t1], lmj = l[3 * g + t2];
    // i at the origin, j at (a, 0), k above and m below the axis
    const double a2 = a * a;
    const double xk = ((a2 + lki * lki) - ljk * ljk) / (2 * a);
    const double xm = ((a2 + lim * lim) - lmj * lmj) / (2 * a);
    const double yk = sqrt(fmax((lki - xk) * (lki + xk), 0.0));
    const double ym = -sqrt(fmax((lim - xm) * (lim + xm), 0.0));
    const double dx = xk - xm, dy = yk - ym;
    const double lkm = sqrt(dx * dx + dy * dy);
#pragma unroll
    for (int x = 0; x < 4; ++x)                        // a partner that is itself one of the four outer sides moves with it
#pragma unroll
      for (int y = 0; y < 4; ++y)
        if (G[oldc[x]] == oldc[y]) part[x] = newc[y];
    F[3 * f] = k; F[3 * f + 1] = i; F[3 * f + 2] = m;
    F[3 * g] = m; F[3 * g + 1] = j; F[3 * g + 2] = k;
    l[3 * f] = lki; l[3 * f + 1] = lim; l[3 * f + 2] = lkm;
    l[3 * g] = lmj; l[3 * g + 1] = ljk; l[3 * g + 2] = lkm;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int q = part[x];
      G[newc[x]] = q;
      if (q >= 0 && (int64_t)q < nS && q / 3 != f && q / 3 != g) G[q] = newc[x];
    }
    G[3 * f + 2] = 3 * g + 2;
    G[3 * g + 2] = 3 * f + 2;
    atomicAdd(&counters[1], 1);
  }
}

// ---- Laplacian of (F', l'): contributions, [caller sorts the keys], heads + scan + row pointers, masses, entries -------------
constexpr int64_t kIdtNoKey = INT64_MAX;
__device__ __forceinline__ int64_t idt_key(int64_t row, int64_t col, int64_t nV, int64_t nFk, int64_t f, int slot) {
  return ((row * nV + col) * nFk + f) * 16 + slot;
}

// item < nF: the 12 contributions of a face (slot 2n: W[F[p], F[q]] of permutation n, slot 2n + 1: its mirror for the column
// sum of F[p], with the mass a/3/4);  item >= nF: the diagonal seed of vertex item - nF (value 0, mass 0, slot 12 of face 0)
__global__ __launch_bounds__(kWG) void idt_contrib_k(const int *__restrict__ F, const double *__restrict__ l, int64_t nV, int64_t nF,
                                                     int64_t *__restrict__ keys, double *__restrict__ cval,
                                                     double *__restrict__ cmass, int *__restrict__ status) {
  const int64_t nFk = nF > 0 ? nF : 1;
  for (int64_t it = (int64_t)blockIdx.x * kWG + threadIdx.x; it < nF + nV; it += (int64_t)gridDim.x * kWG) {
    if (it >= nF) {
      const int64_t v = it - nF, o = 12 * nF + v;
      keys[o] = idt_key(v, v, nV, nFk, 0, 12);
      cval[o] = 0;
      cmass[o] = 0;
      continue;
    }
    const int64_t f = it;
    const int idx[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
    const bool ok = (unsigned)idx[0] < (unsigned)nV && (unsigned)idx[1] < (unsigned)nV && (unsigned)idx[2] < (unsigned)nV;
    if (!ok) {
      if (status) atomicOr(status, SN_IDT_BAD_FACE);
      for (int x = 0; x < 12; ++x) { keys[12 * f + x] = kIdtNoKey; cval[12 * f + x] = 0; cmass[12 * f + x] = 0; }
      continue;
    }
    const double lij = l[3 * f], ljk = l[3 * f + 1], lki = l[3 * f + 2];
    const double h = ((lij + ljk) + lki) / 2;
    const double q = ((h * (h - lij)) * (h - ljk)) * (h - lki);
    const double ar = q > 0 ? sqrt(q) : 1e-6;
    const double den = 8 * ar + 1e-6, mass = ar / 3 / 4;
    const double e01 = lij * lij, e12 = ljk * ljk, e20 = lki * lki;
    // squared length between local corners x, y: index x + y - 1 of {e01, e20, e12}
    const double e2[3] = {e01, e20, e12};
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int pp = perms[n][0], qq = perms[n][1], rr = perms[n][2];
      const double epq = e2[pp + qq - 1], eqr = e2[qq + rr - 1], erp = e2[rr + pp - 1];
      const int64_t row = idx[pp], col = idx[qq], o = 12 * f + 2 * n;
      const bool loop = row == col;                    // a self-edge: W[i,i] cancels in D - W, only its mass counts
      keys[o] = loop ? kIdtNoKey : idt_key(row, col, nV, nFk, f, 2 * n);
      cval[o] = loop ? 0.0 : ((-epq + eqr) + erp) / den;
      cmass[o] = 0;
      keys[o + 1] = idt_key(row, row, nV, nFk, f, 2 * n + 1);
      cval[o + 1] = loop ? 0.0 : ((-epq + erp) + eqr) / den;
      cmass[o + 1] = mass;
    }
  }
}

// head[t] = 1 where sorted position t starts a new (row, col); head[N] = 0 so that the exclusive scan ends in the entry count
__global__ __launch_bounds__(kWG) void idt_heads_k(const int64_t *__restrict__ sk, int64_t N, int64_t span, int *__restrict__ head) {
  for (int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x; t <= N; t += (int64_t)gridDim.x * kWG)
    head[t] = (t < N && sk[t] != kIdtNoKey && (t == 0 || sk[t - 1] / span != sk[t] / span)) ? 1 : 0;
}

// rowptr[r] = entries before the first sorted key of row r (binary search)
__global__ __launch_bounds__(kWG) void idt_rowptr_k(const int64_t *__restrict__ sk, int64_t N, int64_t nV, int64_t span,
                                                    const int *__restrict__ hs, int *__restrict__ rowptr) {
  for (int64_t r = (int64_t)blockIdx.x * kWG + threadIdx.x; r <= nV; r += (int64_t)gridDim.x * kWG) {
    const int64_t want = r * nV * span;
    int64_t lo = 0, hi = N;
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (sk[mid] < want) lo = mid + 1; else hi = mid;
    }
    rowptr[r] = hs[lo];
  }
}

// serial sums over the run of one (row, col) in sorted order: MASS = false writes the entry, MASS = true the vertex mass
template <bool MASS>
__global__ __launch_bounds__(kWG) void idt_entries_k(const int64_t *__restrict__ sk, const int64_t *__restrict__ order, int64_t N,
                                                     int64_t nV, int64_t span, const int *__restrict__ hs,
                                                     const double *__restrict__ contrib, double *__restrict__ A,
                                                     int *__restrict__ colind, float *__restrict__ vals) {
  for (int64_t t = (int64_t)blockIdx.x * kWG + threadIdx.x; t < N; t += (int64_t)gridDim.x * kWG) {
    if (sk[t] == kIdtNoKey) continue;
    const int64_t ent = sk[t] / span;
    if (t > 0 && sk[t - 1] / span == ent) continue;
    const int64_t row = ent / nV, col = ent - row * nV;
    if (MASS && row != col) continue;
    double sum = 0;
    for (int64_t u = t; u < N && sk[u] / span == ent; ++u) {
      const int64_t src = order[u];
      if ((uint64_t)src < (uint64_t)N) sum += contrib[src];
    }
    if constexpr (MASS) {
      A[row] = sum;
    } else {
      const double ainv = 1 / (A[row] + 1e-9);
      const int e = hs[t];
      colind[e] = (int)col;
      vals[e] = (float)(row == col ? ainv * sum : ainv * (0 - sum));
    }
  }
}

// ---- workspace layouts: one description each (SnCarver), run by the *_workspace_bytes query without a workspace and by the
// entry point with it.  nV, nF >= 0. ----
struct BucketWs {      // ptr[nV + 1], cursor[nV + 1], bucket[3 nF], the scan's scratch
  int *ptr = nullptr, *cursor = nullptr, *bucket = nullptr, *sums = nullptr;
  BucketWs() = default;
  BucketWs(SnCarver &c, int64_t nV, int64_t nF)
      : ptr(c.take<int>(nV + 1)), cursor(c.take<int>(nV + 1)), bucket(c.take<int>(3 * nF)), sums(c.take_scan(nV + 1)) {}
};
struct DiracWs {       // the Dirac builder's; the Laplacian builder shares it and leaves Av alone
  SnCarver c;
  double *Af, *Av;
  BucketWs b;
  DiracWs(void *w, int64_t nV, int64_t nF) : c(w), Af(c.take<double>(nF)), Av(c.take<double>(nV)), b(c, nV, nF) {}
};
struct CornersWs {
  SnCarver c;
  int *cursor, *sums;
  CornersWs(void *w, int64_t nV) : c(w), cursor(c.take<int>(nV + 1)), sums(c.take_scan(nV + 1)) {}
};
struct MeshBucketWs {  // glue, descriptors, cot Laplacian
  SnCarver c;
  BucketWs b;
  MeshBucketWs(void *w, int64_t nV, int64_t nF) : c(w), b(c, nV, nF) {}
};
struct IdtLapWs {
  SnCarver c;
  double *cval, *cmass, *A;
  int *hs, *sums;
  IdtLapWs(void *w, int64_t nV, int64_t nF)
      : c(w), cval(c.take<double>(12 * nF + nV)), cmass(c.take<double>(12 * nF + nV)), A(c.take<double>(nV)),
        hs(c.take<int>(12 * nF + nV + 1)), sums(c.take_scan(12 * nF + nV + 1)) {}
};
struct ComponentsWs {  // the winner word and the label counter; edge mode: the sides' buckets
  SnCarver c;
  unsigned long long *acc;
  BucketWs b;
  ComponentsWs(void *w, int64_t nV, int64_t nF, bool edge) : c(w), acc(c.take<unsigned long long>(2)) {
    if (edge) b = BucketWs(c, nV, nF);
  }
};
struct CompactWs {     // one scratch for both scans
  SnCarver c;
  int *vpos, *fpos, *sums;
  CompactWs(void *w, int64_t nV, int64_t nF)
      : c(w), vpos(c.take<int>(nV + 1)), fpos(c.take<int>(nF + 1)), sums(c.take_scan((nV > nF ? nV : nF) + 1)) {}
};
struct OrientWs {
  SnCarver c;
  BucketWs b;
  int *conflict;
  OrientWs(void *w, int64_t nV, int64_t nF) : c(w), b(c, nV, nF), conflict(c.take<int>(nF)) {}
};
template <class T>
inline size_t one_slice_bytes(int64_t count) {      // a workspace that is one array: the entry point takes it as it comes
  SnCarver c(nullptr);
  c.take<T>(count);
  return c.bytes;
}
inline int64_t at_least_0(int64_t n) { return n < 0 ? 0 : n; }

// ------------------------------------------------------------------------------------------------
// Mesh clean-up: component labels by a concurrent union-find, and compaction by two scans (definition: sn_spmm.h).
// A node is a vertex (SN_CC_VERTEX) or a face (SN_CC_EDGE).  parent[x] <= x always: a link is one CAS that turns a root into
// the child of a smaller root, and path halving only replaces a parent by a grandparent.  So every chain strictly decreases,
// the root of a class is its minimum, and nobody ever waits: a CAS fails only because another thread's link succeeded.
// Loads and stores of parent[] are relaxed atomics of device scope, so that a retry reads what the winning CAS wrote.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x.  A chain has at most n nodes; one step past that bound reports SN_CC_INTERNAL and returns -1.
template <bool HALVE>
__device__ __forceinline__ int cc_find(int *parent, int x, int n, int *status) {
  for (int step = 0; step <= n; ++step) {
    const int p = cc_load(parent + x);
    if (p == x) return x;
    if ((unsigned)p >= (unsigned)n) break;               // not a value this file writes
    const int g = cc_load(parent + p);
    if (g == p) return p;
    if ((unsigned)g >= (unsigned)n) break;
    if (HALVE) cc_store(parent + x, g);                  // x is no root and never becomes one again: no CAS targets it
    x = g;
  }
  atomicOr(status, SN_CC_INTERNAL);
  return -1;
}

// join the classes of a and b.  Every pass but the last follows a link made by somebody else, and a class is linked at most
// once as the larger root: at most n passes.
__device__ __forceinline__ void cc_unite(int *parent, int a, int b, int n, int *status) {
  for (int pass = 0; pass <= n; ++pass) {
    a = cc_find<true>(parent, a, n, status);
    b = cc_find<true>(parent, b, n, status);
    if (a < 0 || b < 0 || a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
  }
  atomicOr(status, SN_CC_INTERNAL);
}

__global__ __launch_bounds__(kWG) void cc_init_k(int *__restrict__ parent, int *__restrict__ count, int64_t n) {
  for (int64_t x = (int64_t)blockIdx.x * kWG + threadIdx.x; x < n; x += (int64_t)gridDim.x * kWG) {
    parent[x] = (int)x;
    count[x] = 0;
  }
}

// vertex mode: the three vertices of a good face are one class
__global__ __launch_bounds__(kWG) void cc_vertex_union_k(const int *__restrict__ F, int64_t nF, int64_t nV, int *parent,
                                                         int *__restrict__ status) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    if (!face_ok(i, j, k, nV)) {
      atomicOr(status, SN_CC_BAD_FACE);
      continue;
    }
    cc_unite(parent, i, j, (int)nV, status);
    cc_unite(parent, j, k, (int)nV, status);
  }
}

// edge mode: the sides of the good faces, bucketed under the lower of their two vertices (kLowerEnd: orientation does not
// matter; the orientation of the repair section buckets only the kept faces).
// A side joins its face to the face of the first side of its bucket on the same upper vertex: a star per edge, whatever the
// number of faces on it.  The order inside a bucket (atomic cursor) picks the centre of the star, not the partition.
__global__ __launch_bounds__(kWG) void cc_edge_union_k(const int *__restrict__ F, int64_t nF, int64_t nV, const int *__restrict__ ptr,
                                                       const int *__restrict__ bucket, int *parent, int *__restrict__ status) {
  for (int64_t c = (int64_t)blockIdx.x * kWG + threadIdx.x; c < 3 * nF; c += (int64_t)gridDim.x * kWG) {
    const int64_t f = c / 3;
    const int s = (int)(c - 3 * f);
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    if (!face_ok(i, j, k, nV)) continue;
    const int a = s == 0 ? i : s == 1 ? j : k, b = s == 0 ? j : s == 1 ? k : i;
    const int lo = min(a, b), hi = max(a, b);
    for (int e = ptr[lo]; e < ptr[lo + 1]; ++e) {
      const int d = bucket[e];
      if ((unsigned)d >= (unsigned)(3 * nF)) continue;
      const int g = d / 3, t = d - 3 * g;
      if (max(F[d], F[3 * g + (t + 1) % 3]) != hi) continue;       // (a bucketed side belongs to a good face: its min is lo)
      if (g != (int)f) cc_unite(parent, (int)f, g, (int)nF, status);
      break;
    }
  }
}

// vlabel[v] = root of v, in place (a reader meets the old parent or the root: both are ancestors)
__global__ __launch_bounds__(kWG) void cc_flatten_k(int *parent, int64_t n, int *__restrict__ status) {
  for (int64_t x = (int64_t)blockIdx.x * kWG + threadIdx.x; x < n; x += (int64_t)gridDim.x * kWG) {
    const int r = cc_find<false>(parent, (int)x, (int)n, status);
    cc_store(parent + x, r < 0 ? (int)x : r);
  }
}

// flabel and the histogram.  VERTEX: flabel[f] = vlabel[F[f][0]] (flattened by the launch before);  else flabel is the face
// forest itself and f looks up its own root.
template <bool VERTEX>
__global__ __launch_bounds__(kWG) void cc_face_labels_k(const int *__restrict__ F, int64_t nF, int64_t nV, const int *vlabel,
                                                        int *flabel, int *__restrict__ count, int *__restrict__ status) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    int r = -1;
    if (face_ok(i, j, k, nV)) {
      r = VERTEX ? vlabel[i] : cc_find<false>(flabel, (int)f, (int)nF, status);
      if ((unsigned)r < (unsigned)(VERTEX ? nV : nF)) atomicAdd(&count[r], 1);
      else r = (int)(VERTEX ? i : f);                             // only after SN_CC_INTERNAL
    }
    if (VERTEX) flabel[f] = r;
    else if (r >= 0) cc_store(flabel + f, r);                     // a bad face stays its own root until cc_bad_labels_k
  }
}
__global__ __launch_bounds__(kWG) void cc_bad_labels_k(const int *__restrict__ F, int64_t nF, int64_t nV, int *__restrict__ flabel) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG)
    if (!face_ok(F[3 * f], F[3 * f + 1], F[3 * f + 2], nV)) flabel[f] = -1;
}

// acc[0]: max over the labels of (count << 32) | (0x7fffffff - label) — the largest count, the smallest label on a tie;
// acc[1]: the number of labels that have a face.  One pair of atomics per wave.
typedef unsigned long long cc_word_t;
__global__ __launch_bounds__(kWG) void cc_winner_k(const int *__restrict__ count, int64_t n, cc_word_t *__restrict__ acc) {
  cc_word_t best = 0;
  int used = 0;
  for (int64_t l = (int64_t)blockIdx.x * kWG + threadIdx.x; l < n; l += (int64_t)gridDim.x * kWG) {
    const int c = count[l];
    if (c > 0) {
      const cc_word_t w = ((cc_word_t)(unsigned)c << 32) | (cc_word_t)(0x7fffffffu - (unsigned)l);
      best = w > best ? w : best;
      ++used;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const cc_word_t o = __shfl_down(best, d, 64);
    best = o > best ? o : best;
    used += __shfl_down(used, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && used > 0) {
    atomicMax(&acc[0], best);
    atomicAdd(&acc[1], (cc_word_t)used);
  }
}
__global__ void cc_summary_k(const cc_word_t *__restrict__ acc, int *__restrict__ summary) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const cc_word_t w = acc[0];
  summary[0] = (int)acc[1];
  summary[1] = w ? (int)(0x7fffffffu - (unsigned)(w & 0xffffffffu)) : -1;
  summary[2] = (int)(w >> 32);
}

// ---- compaction: fmark[f] = face f stays, vmark[v] = a staying face uses v (plain stores of 1), both with one slot past the
// end so that the exclusive scans end in the totals ----
__global__ __launch_bounds__(kWG) void compact_mark_k(const int *__restrict__ F, const int *__restrict__ keep, int64_t nF, int64_t nV,
                                                      int *__restrict__ fmark, int *__restrict__ vmark) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f <= nF; f += (int64_t)gridDim.x * kWG) {
    if (f == nF) {
      fmark[f] = 0;
      break;
    }
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    const bool stay = keep[f] != 0 && face_ok(i, j, k, nV);
    fmark[f] = stay ? 1 : 0;
    if (stay) vmark[i] = vmark[j] = vmark[k] = 1;
  }
}
__global__ __launch_bounds__(kWG) void compact_vertices_k(const float *__restrict__ V, int64_t nV, const int *__restrict__ vpos,
                                                          int *__restrict__ I, int *__restrict__ J, float *__restrict__ Vnew,
                                                          const int *__restrict__ fpos, int64_t nF, int *__restrict__ sizes) {
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v <= nV; v += (int64_t)gridDim.x * kWG) {
    if (v == nV) {
      sizes[0] = vpos[nV];
      sizes[1] = fpos[nF];
      break;
    }
    const int o = vpos[v];
    const bool stay = vpos[v + 1] != o;
    I[v] = stay ? o : -1;
    if (!stay) continue;
    J[o] = (int)v;
    if (V) {
      Vnew[3 * (int64_t)o] = V[3 * v];
      Vnew[3 * (int64_t)o + 1] = V[3 * v + 1];
      Vnew[3 * (int64_t)o + 2] = V[3 * v + 2];
    }
  }
}
__global__ __launch_bounds__(kWG) void compact_faces_k(const int *__restrict__ F, int64_t nF, const int *__restrict__ fpos,
                                                       const int *__restrict__ vpos, int *__restrict__ Fsrc, int *__restrict__ Fnew) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int o = fpos[f];
    if (fpos[f + 1] == o) continue;                      // a staying face passed face_ok: its indices address vpos
    Fsrc[o] = (int)f;
    Fnew[3 * (int64_t)o] = vpos[F[3 * f]];
    Fnew[3 * (int64_t)o + 1] = vpos[F[3 * f + 1]];
    Fnew[3 * (int64_t)o + 2] = vpos[F[3 * f + 2]];
  }
}
__global__ __launch_bounds__(kWG) void label_mask_k(const int *__restrict__ flabel, int64_t nF, const int *__restrict__ label,
                                                    int *__restrict__ keep) {
  const int want = *label;
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG)
    keep[f] = (want >= 0 && flabel[f] == want) ? 1 : 0;
}

// exclusive scan of a[0..n) in place on stream s
inline void scan_in_place(int *a, int64_t n, int *sums, hipStream_t s) { sn_internal_scan_i32(a, n, a, sums, nullptr, 0, 0, s); }

// ------------------------------------------------------------------------------------------------
// Mesh repair: weld, duplicate faces, orientation (definition: sn_spmm.h, "Mesh repair").
// Weld and duplicate faces share one scheme: an open-addressing table of ids at load factor <= 0.5.  A slot is claimed by one
// atomicCAS(empty -> id) and from then on holds ids of ONE key only: a probe compares its own key with the key of the id it
// finds, moves on when they differ and does atomicMin(slot, id) when they agree.  Slots are never emptied, so every member of a
// class stops at the same slot, whatever the order, and after the launch that slot holds the smallest id of the class.  Which
// slot a class sits in depends on the order; what is read from it does not.  A class of k coincident members costs k atomics
// on one word, not k^2 comparisons.
// ------------------------------------------------------------------------------------------------
constexpr int kRepairEmpty = -1;
constexpr int64_t kRepairMaxNodes = (int64_t)1 << 30;      // table of at most 2^31 slots; the parity bit of the orientation forest

struct RepairKey { int64_t a, b, c; };
__device__ __forceinline__ bool key_eq(const RepairKey &x, const RepairKey &y) { return x.a == y.a && x.b == y.b && x.c == y.c; }
__device__ __forceinline__ uint32_t key_slot(const RepairKey &k, uint32_t mask) {
  uint64_t h = (uint64_t)k.a * 0x9E3779B97F4A7C15ull;
  h = (h ^ (h >> 29)) + (uint64_t)k.b;
  h *= 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 31)) + (uint64_t)k.c;
  h *= 0x94D049BB133111EBull;
  return (uint32_t)(h >> 32) & mask;
}

// weld key of vertex v; false: v is unweldable.  tol == 0: the fp32 values themselves, -0.0 as +0.0 (one bit pattern per value);
// tol > 0: rint((double)x / tol), round-half-even, as int64, quotients outside +-2^62 (an infinite one among them) refused.
// weld == 0: nothing is welded and only a non-finite coordinate refuses.
__device__ __forceinline__ bool weld_key(const float *__restrict__ V, int64_t v, double tol, int weld, RepairKey *key) {
  int64_t q[3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = V[3 * v + c];
    q[c] = 0;
    if (!isfinite(x)) ok = false;
    else if (!weld) continue;
    else if (tol > 0) {
      const double r = rint((double)x / tol);
      if (!(fabs(r) <= 0x1p62)) ok = false;
      else q[c] = (int64_t)r;
    } else {
      q[c] = (int64_t)__float_as_uint(x == 0.0f ? 0.0f : x);
    }
  }
  key->a = q[0], key->b = q[1], key->c = q[2];
  return ok;
}
// key of face f: its three vertex ids in ascending order; false: f is bad
__device__ __forceinline__ bool face_key(const int *__restrict__ F, int64_t f, int64_t nV, RepairKey *key) {
  int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
  if (!face_ok(i, j, k, nV)) return false;
  int t;
  if (i > j) t = i, i = j, j = t;
  if (j > k) t = j, j = k, k = t;
  if (i > j) t = i, i = j, j = t;
  key->a = i, key->b = j, key->c = k;
  return true;
}

// one wave64 sum, then one atomicAdd per wave
__device__ __forceinline__ void wave_count(int v, int *dst) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// FACES: the ids are faces of F and the key is face_key; else vertices of V and weld_key.  The probe loops are bounded by the
// table size (the table has at least twice as many slots as ids, so an empty slot is always met first): SN_REPAIR_INTERNAL.
template <bool FACES>
__device__ __forceinline__ bool repair_key(const float *__restrict__ V, const int *__restrict__ F, int64_t x, int64_t nV, double tol,
                                           RepairKey *key) {
  return FACES ? face_key(F, x, nV, key) : weld_key(V, x, tol, 1, key);
}
template <bool FACES>
__global__ __launch_bounds__(kWG) void repair_insert_k(const float *__restrict__ V, const int *__restrict__ F, int64_t n, int64_t nV,
                                                       double tol, int *table, uint32_t mask, int *__restrict__ status) {
  for (int64_t x = (int64_t)blockIdx.x * kWG + threadIdx.x; x < n; x += (int64_t)gridDim.x * kWG) {
    RepairKey mine, other;
    if (!repair_key<FACES>(V, F, x, nV, tol, &mine)) continue;
    uint32_t h = key_slot(mine, mask);
    bool done = false;
    for (uint32_t probe = 0; probe <= mask && !done; ++probe, h = (h + 1) & mask) {
      int cur = cc_load(table + h);
      if (cur == kRepairEmpty) {
        cur = atomicCAS(table + h, kRepairEmpty, (int)x);
        if (cur == kRepairEmpty) {
          done = true;
          break;
        }
      }
      if ((unsigned)cur >= (unsigned)n || !repair_key<FACES>(V, F, cur, nV, tol, &other)) break;       // not a value this file writes
      if (key_eq(mine, other)) {
        atomicMin(table + h, (int)x);
        done = true;
      }
    }
    if (!done) atomicOr(status, SN_REPAIR_INTERNAL);
  }
}
// the slot of x's class, read after repair_insert_k has finished: the smallest id of the class (x itself after SN_REPAIR_INTERNAL)
template <bool FACES>
__device__ __forceinline__ int repair_lookup(const float *__restrict__ V, const int *__restrict__ F, int64_t x, int64_t n, int64_t nV,
                                             double tol, const RepairKey &mine, const int *__restrict__ table, uint32_t mask,
                                             int *__restrict__ status) {
  uint32_t h = key_slot(mine, mask);
  for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
    const int cur = table[h];
    RepairKey other;
    if ((unsigned)cur >= (unsigned)n || !repair_key<FACES>(V, F, cur, nV, tol, &other)) break;
    if (key_eq(mine, other)) return cur;
  }
  atomicOr(status, SN_REPAIR_INTERNAL);
  return (int)x;
}

__global__ __launch_bounds__(kWG) void weld_rep_k(const float *__restrict__ V, int64_t nV, double tol, int weld,
                                                  const int *__restrict__ table, uint32_t mask, int *__restrict__ rep,
                                                  int *__restrict__ counts, int *__restrict__ status) {
  int welded = 0;
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v < nV; v += (int64_t)gridDim.x * kWG) {
    RepairKey mine;
    int r = (int)v;
    if (weld && weld_key(V, v, tol, 1, &mine)) r = repair_lookup<false>(V, nullptr, v, nV, nV, tol, mine, table, mask, status);
    rep[v] = r;
    welded += r != (int)v;
  }
  wave_count(welded, counts);
}
// F through the representative; an unweldable vertex is written as -1, so that every later step sees its faces as bad; an index
// outside 0..nV-1 stays what it is
__global__ __launch_bounds__(kWG) void weld_faces_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF, int64_t nV,
                                                    double tol, int weld, const int *__restrict__ rep, int *__restrict__ Fw,
                                                    int *__restrict__ status) {
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < 3 * nF; e += (int64_t)gridDim.x * kWG) {
    const int v = F[e];
    int out = v;
    if ((unsigned)v < (unsigned)nV) {
      RepairKey key;
      if (weld_key(V, v, tol, weld, &key)) out = rep[v];
      else {
        out = -1;
        atomicOr(status, SN_REPAIR_NONFINITE);
      }
    }
    Fw[e] = out;
  }
}

// keep[f] = f is good and (with unique) the smallest face id on its unordered vertex triple.  counts = {bad faces, duplicate
// faces, kept faces whose fp64 squared double-area is exactly 0}
__global__ __launch_bounds__(kWG) void unique_keep_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF, int64_t nV,
                                                     int unique, const int *__restrict__ table, uint32_t mask, int *__restrict__ keep,
                                                     int *__restrict__ counts, int *__restrict__ status) {
  int bad = 0, dup = 0, flat = 0;
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    RepairKey mine;
    int stay = 0;
    if (!face_key(F, f, nV, &mine)) {
      ++bad;
    } else {
      stay = !unique || repair_lookup<true>(nullptr, F, f, nF, nV, 0.0, mine, table, mask, status) == (int)f;
      dup += !stay;
      if (stay && V) {
        const int a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
        const double ux = (double)V[3 * b] - (double)V[3 * a], uy = (double)V[3 * b + 1] - (double)V[3 * a + 1],
                     uz = (double)V[3 * b + 2] - (double)V[3 * a + 2];
        const double wx = (double)V[3 * c] - (double)V[3 * a], wy = (double)V[3 * c + 1] - (double)V[3 * a + 1],
                     wz = (double)V[3 * c + 2] - (double)V[3 * a + 2];
        const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
        flat += ((cx * cx + cy * cy) + cz * cz) == 0.0;
      }
    }
    keep[f] = stay;
  }
  if (bad) atomicOr(status, SN_REPAIR_BAD_FACE);
  wave_count(bad, counts);
  wave_count(dup, counts + 1);
  wave_count(flat, counts + 2);
}

// ---- orientation: the union-find of cc_unite with the parity to the parent in bit 0, w[x] = (parent << 1) | parity ----
// A root is w[x] == x << 1.  A link is one CAS on a root, the larger under the smaller; halving stores (grandparent, parity
// to it) into a non-root.  The parity between a node and any of its ancestors is fixed by the links once made, so every word
// a reader meets is a valid (ancestor, parity to it) pair.  Returns the root, *par = parity of x to it; -1 past the bound.
template <bool HALVE>
__device__ __forceinline__ int or_find(int *w, int x, int n, int *par, int *status) {
  int acc = 0;
  for (int step = 0; step <= n; ++step) {
    const int wx = cc_load(w + x), p = wx >> 1;
    if (wx == x << 1) {
      *par = acc;
      return x;
    }
    if ((unsigned)p >= (unsigned)n) break;
    const int wp = cc_load(w + p), g = wp >> 1;
    if (wp == p << 1) {
      *par = acc ^ (wx & 1);
      return p;
    }
    if ((unsigned)g >= (unsigned)n) break;
    const int q = (wx ^ wp) & 1;
    if (HALVE) cc_store(w + x, (g << 1) | q);
    acc ^= q;
    x = g;
  }
  atomicOr(status, SN_REPAIR_INTERNAL);
  return -1;
}
// faces a and b must end with flip[a] ^ flip[b] == p.  In one class already: a disagreement flags the root met (or_resolve_k
// carries the flag to the final root).
__device__ __forceinline__ void or_unite(int *w, int *conflict, int a, int b, int p, int n, int *status) {
  for (int pass = 0; pass <= n; ++pass) {
    int pa, pb;
    a = or_find<true>(w, a, n, &pa, status);
    b = or_find<true>(w, b, n, &pb, status);
    if (a < 0 || b < 0) return;
    p ^= pa ^ pb;                                                  // now between the two roots
    if (a == b) {
      if (p) cc_store(conflict + a, 1);
      return;
    }
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(w + hi, hi << 1, (lo << 1) | p) == hi << 1) return;
  }
  atomicOr(status, SN_REPAIR_INTERNAL);
}
__global__ __launch_bounds__(kWG) void or_init_k(int *__restrict__ w, int *__restrict__ conflict, int64_t n) {
  for (int64_t x = (int64_t)blockIdx.x * kWG + threadIdx.x; x < n; x += (int64_t)gridDim.x * kWG) {
    w[x] = (int)x << 1;
    conflict[x] = 0;
  }
}
// One thread per side of a kept face.  It counts the sides of its bucket on its own edge, itself included: exactly two is a
// link, made by the side with the lower code; three and more link nothing and the lowest code counts the edge.
__global__ __launch_bounds__(kWG) void or_link_k(const int *__restrict__ F, const int *__restrict__ keep, int64_t nF, int64_t nV,
                                                 const int *__restrict__ ptr, const int *__restrict__ bucket, int *w, int *conflict,
                                                 int *__restrict__ counts, int *__restrict__ status) {
  int edges = 0;
  for (int64_t c = (int64_t)blockIdx.x * kWG + threadIdx.x; c < 3 * nF; c += (int64_t)gridDim.x * kWG) {
    const int64_t f = c / 3;
    const int s = (int)(c - 3 * f);
    if (keep[f] == 0) continue;
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    if (!face_ok(i, j, k, nV)) continue;
    const int a = s == 0 ? i : s == 1 ? j : k, b = s == 0 ? j : s == 1 ? k : i;
    const int lo = min(a, b), hi = max(a, b);
    int m = 0, other = -1, other_from = -1, first = INT_MAX;
    for (int e = ptr[lo]; e < ptr[lo + 1]; ++e) {
      const int d = bucket[e];
      if ((unsigned)d >= (unsigned)(3 * nF)) continue;
      const int g = d / 3, t = d - 3 * g;
      const int from = F[d], to = F[3 * g + (t + 1) % 3];
      if (max(from, to) != hi) continue;                           // (a bucketed side belongs to a good face: its min is lo)
      ++m;
      first = min(first, d);
      if (d != (int)c) other = d, other_from = from;
    }
    if (m == 2 && (int)c < other) or_unite(w, conflict, (int)f, other / 3, other_from == a ? 1 : 0, (int)nF, status);
    else if (m > 2 && first == (int)c) ++edges;
  }
  if (edges) atomicOr(status, SN_REPAIR_NONMANIFOLD);
  wave_count(edges, counts);
}
// w[f] = (root << 1) | parity in place (still a valid pair), and a flagged face flags its root
__global__ __launch_bounds__(kWG) void or_resolve_k(int *w, int *conflict, int64_t nF, int *__restrict__ status) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    int par;
    const int r = or_find<false>(w, (int)f, (int)nF, &par, status);
    if (r < 0) continue;
    cc_store(w + f, (r << 1) | par);
    if (r != (int)f && cc_load(conflict + f)) cc_store(conflict + r, 1);
  }
}
// label, flip and the oriented faces; counts[1..2] = {classes without a consistent winding, classes}
__global__ __launch_bounds__(kWG) void or_finish_k(const int *__restrict__ F, const int *__restrict__ keep, int64_t nF, int64_t nV,
                                                   int *label, const int *__restrict__ conflict, int *__restrict__ flip,
                                                   int *__restrict__ Fout, int *__restrict__ counts, int *__restrict__ status) {
  int classes = 0, twisted = 0;
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    const bool in = keep[f] != 0 && face_ok(i, j, k, nV);
    const int wf = label[f], r = wf >> 1;
    int turn = 0;
    if (in && (unsigned)r < (unsigned)nF) {
      const int bad = conflict[r];
      turn = bad ? 0 : (wf & 1);
      classes += r == (int)f;
      twisted += r == (int)f && bad;
    }
    label[f] = in ? r : -1;
    flip[f] = turn;
    if (Fout) {
      Fout[3 * f] = i;
      Fout[3 * f + 1] = turn ? k : j;
      Fout[3 * f + 2] = turn ? j : k;
    }
  }
  if (twisted) atomicOr(status, SN_REPAIR_NONORIENTABLE);
  wave_count(twisted, counts + 1);
  wave_count(classes, counts + 2);
}

inline uint32_t repair_table_slots(int64_t n) {      // a power of two >= 2 n, n <= 2^30
  uint32_t t = 2;
  while ((int64_t)t < 2 * n) t <<= 1;
  return t;
}

// ------------------------------------------------------------------------------------------------
// Per-vertex normals, mass and curvature, and the libigl-convention Laplacian (definition: sn_spmm.h, "Mesh descriptors").
// Every per-face quantity is a function of the face alone, so a corner recomputes it from the three positions it has loaded
// anyway instead of reading a 64-byte record another pass wrote: same bits, one gather less (LABNOTES.md#descriptors).
// ------------------------------------------------------------------------------------------------
struct FaceGeom {      // n_f and dbl_f from the first vertex, and the dot products d at the corners i, j, k
  double nx, ny, nz, dbl, d0, d1, d2;
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}
__device__ __forceinline__ double pick3(double x0, double x1, double x2, int c) { return c == 0 ? x0 : c == 1 ? x1 : x2; }
__device__ __forceinline__ int pick3i(int x0, int x1, int x2, int c) { return c == 0 ? x0 : c == 1 ? x1 : x2; }

// of a face that passed face_ok
__device__ __forceinline__ FaceGeom face_geom(const float *__restrict__ V, int i, int j, int k) {
  const double ix = V[3 * i], iy = V[3 * i + 1], iz = V[3 * i + 2];
  const double jx = V[3 * j], jy = V[3 * j + 1], jz = V[3 * j + 2];
  const double kx = V[3 * k], ky = V[3 * k + 1], kz = V[3 * k + 2];
  const double ax = jx - ix, ay = jy - iy, az = jz - iz;       // P_j - P_i
  const double bx = kx - ix, by = ky - iy, bz = kz - iz;       // P_k - P_i
  FaceGeom g;
  g.nx = ay * bz - az * by;
  g.ny = az * bx - ax * bz;
  g.nz = ax * by - ay * bx;
  g.dbl = sqrt(dot3(g.nx, g.ny, g.nz, g.nx, g.ny, g.nz));
  g.d0 = dot3(ax, ay, az, bx, by, bz);                                                  // (i; j, k)
  g.d1 = dot3(kx - jx, ky - jy, kz - jz, ix - jx, iy - jy, iz - jz);                    // (j; k, i)
  g.d2 = dot3(ix - kx, iy - ky, iz - kz, jx - kx, jy - ky, jz - kz);                    // (k; i, j)
  return g;
}

// the corner (v; a, b) = corner c of a face that is neither bad nor flat
struct CornerTerms {
  double ux, uy, uz, wx, wy, wz;      // u = P_a - P_v, w = P_b - P_v
  double dv, cota, cotb, af, vor;     // vor: the corner's term of M_voronoi
};
__device__ __forceinline__ CornerTerms corner_terms(const float *__restrict__ V, int v, int a, int b, const FaceGeom &g, int c) {
  const double px = V[3 * v], py = V[3 * v + 1], pz = V[3 * v + 2];
  CornerTerms t;
  t.ux = (double)V[3 * a] - px; t.uy = (double)V[3 * a + 1] - py; t.uz = (double)V[3 * a + 2] - pz;
  t.wx = (double)V[3 * b] - px; t.wy = (double)V[3 * b + 1] - py; t.wz = (double)V[3 * b + 2] - pz;
  t.dv = pick3(g.d0, g.d1, g.d2, c);
  t.cota = pick3(g.d1, g.d2, g.d0, c) / g.dbl;
  t.cotb = pick3(g.d2, g.d0, g.d1, c) / g.dbl;
  t.af = g.dbl / 2;
  if (g.d0 < 0 || g.d1 < 0 || g.d2 < 0) {
    t.vor = t.dv < 0 ? t.af / 2 : t.af / 4;
  } else {
    const double uu = dot3(t.ux, t.uy, t.uz, t.ux, t.uy, t.uz), ww = dot3(t.wx, t.wy, t.wz, t.wx, t.wy, t.wz);
    t.vor = (uu * t.cotb + ww * t.cota) / 8;
  }
  return t;
}

// counts the corners of the good faces per vertex, raises the bad / flat bits, writes the face outputs that are wanted
__global__ __launch_bounds__(kWG) void desc_face_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nF, int64_t nV,
                                                   int *__restrict__ count, float *__restrict__ face_area,
                                                   float *__restrict__ face_normal, int *__restrict__ status) {
  for (int64_t f = (int64_t)blockIdx.x * kWG + threadIdx.x; f < nF; f += (int64_t)gridDim.x * kWG) {
    const int i = F[3 * f], j = F[3 * f + 1], k = F[3 * f + 2];
    float a = 0.f, x = 0.f, y = 0.f, z = 0.f;
    if (!face_ok(i, j, k, nV)) {
      atomicOr(status, SN_DESC_BAD_FACE);
    } else {
      atomicAdd(&count[i], 1);
      atomicAdd(&count[j], 1);
      atomicAdd(&count[k], 1);
      const FaceGeom g = face_geom(V, i, j, k);
      if (!(g.dbl > 0)) {
        atomicOr(status, SN_DESC_FLAT_FACE);
      } else {
        a = (float)(g.dbl / 2);
        x = (float)(g.nx / g.dbl); y = (float)(g.ny / g.dbl); z = (float)(g.nz / g.dbl);
      }
    }
    if (face_area) face_area[f] = a;
    if (face_normal) { face_normal[3 * f] = x; face_normal[3 * f + 1] = y; face_normal[3 * f + 2] = z; }
  }
}

// N / |N| componentwise, or zero and the flag
__device__ __forceinline__ void desc_put_normal(float *__restrict__ out, int64_t v, double x, double y, double z, int *flags) {
  const double len = sqrt(dot3(x, y, z, x, y, z));
  const bool ok = len > 0;
  if (!ok) *flags |= SN_DESC_NO_NORMAL;
  out[3 * v] = ok ? (float)(x / len) : 0.f;
  out[3 * v + 1] = ok ? (float)(y / len) : 0.f;
  out[3 * v + 2] = ok ? (float)(z / len) : 0.f;
}

// one thread per vertex streams over its sorted incidence list (codes 3 f + c, ascending): no bound on the list's length
__global__ __launch_bounds__(kWG) void desc_vertex_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                     const int *__restrict__ vptr, const int *__restrict__ inc,
                                                     float *__restrict__ n_area, float *__restrict__ n_uniform,
                                                     float *__restrict__ n_angle, float *__restrict__ mass_bary,
                                                     float *__restrict__ mass_voronoi, float *__restrict__ gauss,
                                                     float *__restrict__ mean, int *__restrict__ status) {
  const bool want_angle = n_angle != nullptr || gauss != nullptr;
  for (int64_t v = (int64_t)blockIdx.x * kWG + threadIdx.x; v < nV; v += (int64_t)gridDim.x * kWG) {
    double nax = 0, nay = 0, naz = 0, nux = 0, nuy = 0, nuz = 0, ngx = 0, ngy = 0, ngz = 0;
    double px = 0, py = 0, pz = 0, mb = 0, mv = 0, th = 0;
    for (int o = vptr[v]; o < vptr[v + 1]; ++o) {
      const int64_t f = inc[o] / 3;
      const int c = inc[o] % 3;
      const int idx[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
      const FaceGeom g = face_geom(V, idx[0], idx[1], idx[2]);
      if (!(g.dbl > 0)) continue;
      const CornerTerms t = corner_terms(V, (int)v, pick3i(idx[1], idx[2], idx[0], c), pick3i(idx[2], idx[0], idx[1], c), g, c);
      const double hx = g.nx / g.dbl, hy = g.ny / g.dbl, hz = g.nz / g.dbl;
      nax += g.nx; nay += g.ny; naz += g.nz;
      nux += hx; nuy += hy; nuz += hz;
      if (want_angle) {
        const double a = atan2(g.dbl, t.dv);
        th += a;
        ngx += a * hx; ngy += a * hy; ngz += a * hz;
      }
      mb += t.af / 3;
      mv += t.vor;
      const double ha = 0.5 * t.cota, hb = 0.5 * t.cotb;
      px += hb * t.ux + ha * t.wx;
      py += hb * t.uy + ha * t.wy;
      pz += hb * t.uz + ha * t.wz;
    }
    int flags = 0;
    if (n_area) desc_put_normal(n_area, v, nax, nay, naz, &flags);
    if (n_uniform) desc_put_normal(n_uniform, v, nux, nuy, nuz, &flags);
    if (n_angle) desc_put_normal(n_angle, v, ngx, ngy, ngz, &flags);
    if (mass_bary) mass_bary[v] = (float)mb;
    if (mass_voronoi) mass_voronoi[v] = (float)mv;
    if (gauss) gauss[v] = (float)(2 * 3.141592653589793 - th);
    if (mean) {
      const double len = sqrt(dot3(px, py, pz, px, py, pz));
      const double s = dot3(px, py, pz, nax, nay, naz) > 0 ? -1.0 : 1.0;
      mean[v] = mv > 0 ? (float)((s * len) / (2 * mv)) : 0.f;
    }
    if (flags) atomicOr(status, flags);
  }
}

// an entry of the libigl-convention Laplacian rounded to fp32, with the reference's clamp when one is given
__device__ __forceinline__ float cot_entry(double x, int clamp, float hack, int *flags) {
  float v = (float)x;
  if (clamp && !(fabsf(v) <= 1e10f)) {      // not finite, or past 1e10 either way
    v = hack;
    *flags |= SN_DESC_CLAMPED;
  }
  return v;
}

// L = M^-1 C by rows, the frame of laplacian_rows_k: neighbour lists in registers, hence its degree limit.  PENCIL: the same
// sums left in fp64 and undivided, S = -C into vals64 and the mass into mass64 (sn_mesh_cot_pencil_f64)
template <bool FILL, bool PENCIL = false>
__global__ __launch_bounds__(kWG) void cot_laplacian_rows_k(const float *__restrict__ V, const int *__restrict__ F, int64_t nV,
                                                            const int *__restrict__ vptr, const int *__restrict__ inc, int voronoi,
                                                            int clamp, float hack, int *__restrict__ rowptr,
                                                            int *__restrict__ colind, float *__restrict__ vals,
                                                            int *__restrict__ status, double *__restrict__ vals64 = nullptr,
                                                            double *__restrict__ mass64 = nullptr) {
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < nV; i += (int64_t)gridDim.x * kWG) {
    const int b = vptr[i], e = vptr[i + 1];
    if (e - b > kMaxDeg) {
      atomicOr(status, SN_DESC_DEGREE);
      if constexpr (!FILL) rowptr[i] = 1;
      continue;
    }
    int nb[2 * kMaxDeg];          // neighbour ids (with duplicates), in face order
    double cw[2 * kMaxDeg];       // contribution to C[i, nb]
    int n = 0;
    double M = 0;
    for (int o = b; o < e; ++o) {
      const int64_t f = inc[o] / 3;
      const int c = inc[o] % 3;
      const int idx[3] = {F[3 * f], F[3 * f + 1], F[3 * f + 2]};
      const FaceGeom g = face_geom(V, idx[0], idx[1], idx[2]);
      if (!(g.dbl > 0)) continue;
      const int va = pick3i(idx[1], idx[2], idx[0], c), vb = pick3i(idx[2], idx[0], idx[1], c);
      const CornerTerms t = corner_terms(V, (int)i, va, vb, g, c);
      nb[n] = va; cw[n] = 0.5 * t.cotb; ++n;             // the edge i-a lies opposite b
      nb[n] = vb; cw[n] = 0.5 * t.cota; ++n;
      M += voronoi ? t.vor : t.af / 3;
    }
    sort_run(nb, 0, n, cw);                              // by neighbour id, stable
    if constexpr (!FILL) {
      int cnt = 0;
      for (int x = 0; x < n; ++x) cnt += (x == 0 || nb[x] != nb[x - 1]);
      rowptr[i] = cnt + 1;
    } else {
      double S = 0;
      int out = rowptr[i], dpos = -1, flags = 0;
      for (int x = 0; x < n;) {
        const int kn = nb[x];
        double C = 0;
        while (x < n && nb[x] == kn) C += cw[x++];
        S += C;
        if (dpos < 0 && kn > i) dpos = out++;            // the diagonal slot, filled below
        colind[out] = kn;
        if constexpr (PENCIL) vals64[out] = 0 - C; else vals[out] = cot_entry(C / M, clamp, hack, &flags);
        ++out;
      }
      if (dpos < 0) dpos = out;
      colind[dpos] = (int)i;
      if constexpr (PENCIL) {
        vals64[dpos] = S;
        mass64[i] = M;
      } else {
        vals[dpos] = cot_entry((0 - S) / M, clamp, hack, &flags);
      }
      if (flags) atomicOr(status, flags);
    }
  }
}

// ptr / bucket of the good faces (codes 3 f + c, ascending per vertex) after desc_face_k has counted into a zeroed ptr
inline int incidence_build(const int *F, int64_t nV, int64_t nF, const BucketWs &b, hipStream_t s) {
  const int st = bucket_offsets(b.ptr, b.cursor, b.sums, nV, s);
  if (st != SN_OK) return st;
  if (nF > 0)
    hipLaunchKernelGGL((bucket_fill_k<kCornerVertex, kGoodFaces, 3>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, (const int *)nullptr, nF, nV,
                       b.cursor, b.bucket);
  if (nV > 0) hipLaunchKernelGGL(vertex_sort_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, b.ptr, nV, b.bucket);
  return SN_OK;
}

}  // namespace

// the by-vertex incidence of the good faces for the builders of other translation units (sn_internal.h)
size_t sn_internal_incidence_bytes(int64_t nV, int64_t nF) { return MeshBucketWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes; }

int sn_internal_incidence(const int *F, int64_t nV, int64_t nF, void *workspace, int *status, int bad_face_bit, const int **ptr,
                          const int **inc, int **sums, hipStream_t s) {
  const BucketWs b = MeshBucketWs(workspace, nV, nF).b;
  const hipError_t e = sn_internal_fill(b.ptr, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF > 0)
    hipLaunchKernelGGL((bucket_count_k<kCornerVertex, kGoodFaces>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F,
                       (const int *)nullptr, nF, nV, b.ptr, status, bad_face_bit);
  const int st = incidence_build(F, nV, nF, b, s);
  *ptr = b.ptr;
  *inc = b.bucket;
  *sums = b.sums;
  return st;
}

extern "C" {

size_t sn_dirac_workspace_bytes(int64_t nV, int64_t nF) {
  return DiracWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes;
}

int sn_dirac_bsr4_from_mesh(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t *di_rowptr,
                            int32_t *di_colind, float *di_vals, float *diat_vals, int32_t *dia_rowptr,
                            int32_t *dia_colind, float *dia_vals, float *dit_vals, void *workspace,
                            size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (4 * nV + 1 > INT_MAX || 12 * nF > INT_MAX) return SN_E_RANGE;
  if (!di_rowptr || !dia_rowptr) return SN_E_NULL;
  if (nF > 0 && (!V || !F || !di_colind || !di_vals || !diat_vals || !dia_colind || !dia_vals || !dit_vals)) return SN_E_NULL;
  if (workspace_bytes < sn_dirac_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DiracWs ws(workspace, nV, nF);
  double *Af = ws.Af, *Av = ws.Av;
  int *vptr = ws.b.ptr, *inc = ws.b.bucket;      // the faces are not validated on this path: codes 4 f + c of every face
  const hipError_t e = sn_internal_fill(vptr, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF > 0) hipLaunchKernelGGL(face_area_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, V, F, nF, Af, vptr);
  const int st = bucket_offsets(vptr, ws.b.cursor, ws.b.sums, nV, s);
  if (st != SN_OK) return st;
  if (nF > 0)
    hipLaunchKernelGGL((bucket_fill_k<kCornerVertex, kEveryFace, 4>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, (const int *)nullptr, nF, nV,
                       ws.b.cursor, inc);
  if (nV > 0) hipLaunchKernelGGL(vertex_lists_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, vptr, nV, inc, Af, Av, dia_colind);
  hipLaunchKernelGGL(di_fill_k, dim3(grid_for(nF + 1, kWG)), dim3(kWG), 0, s, V, F, nF, Af, Av, di_rowptr, di_colind, di_vals, diat_vals);
  hipLaunchKernelGGL(dia_fill_k, dim3(grid_for(nV + 1, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, Af, Av, dia_rowptr, dia_vals, dit_vals);
  return launch_status();
}

size_t sn_laplacian_workspace_bytes(int64_t nV, int64_t nF) { return sn_dirac_workspace_bytes(nV, nF); }

int sn_laplacian_csr_from_mesh(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase,
                               int32_t *rowptr, int32_t *colind, float *vals, int32_t *status_flag,
                               void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();      // a stale error left by an earlier runtime call of this thread is not ours to report
  if (nV < 0 || nF < 0 || (phase != 0 && phase != 1)) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!rowptr) return SN_E_NULL;
  if (nF > 0 && (!V || !F)) return SN_E_NULL;
  if (phase == 1 && nV > 0 && (!colind || !vals)) return SN_E_NULL;
  if (workspace_bytes < sn_laplacian_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DiracWs ws(workspace, nV, nF);
  double *Af = ws.Af;
  int *vptr = ws.b.ptr, *inc = ws.b.bucket;
  if (phase == 0) {
    hipError_t e = sn_internal_fill(vptr, 0, (size_t)(nV + 1) * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (status_flag) {
      e = sn_internal_fill(status_flag, 0, sizeof(int), s);
      if (e != hipSuccess) return (int)e;
    }
    if (nF > 0) hipLaunchKernelGGL(face_area_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, V, F, nF, Af, vptr);
    const int st = bucket_offsets(vptr, ws.b.cursor, ws.b.sums, nV, s);
    if (st != SN_OK) return st;
    if (nF > 0)
      hipLaunchKernelGGL((bucket_fill_k<kCornerVertex, kEveryFace, 4>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, (const int *)nullptr, nF,
                         nV, ws.b.cursor, inc);
    if (nV > 0) hipLaunchKernelGGL(vertex_sort_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, vptr, nV, inc);
    e = sn_internal_fill(rowptr + nV, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (nV > 0)
      hipLaunchKernelGGL((laplacian_rows_k<false>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, Af, rowptr,
                         (int *)nullptr, (float *)nullptr, status_flag);
    scan_in_place(rowptr, nV + 1, ws.b.sums, s);
  } else if (nV > 0) {
    hipLaunchKernelGGL((laplacian_rows_k<true>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, Af, rowptr, colind,
                       vals, (int *)nullptr);
  }
  return launch_status();
}

int sn_edge_lengths_csr_f32(const float *V, const int32_t *rowptr, const int32_t *colind, int64_t n, float *w, void *stream) {
  (void)hipGetLastError();
  if (n < 0) return SN_E_SHAPE;
  if (n + 1 > INT_MAX) return SN_E_RANGE;
  if (n == 0) return SN_OK;
  if (!V || !rowptr) return SN_E_NULL;
  if (!colind != !w) return SN_E_NULL;
  if (!colind) return SN_OK;                                     // a pattern without entries
  hipLaunchKernelGGL(edge_lengths_csr_k, dim3(grid_for(n, kWG)), dim3(kWG), 0, static_cast<hipStream_t>(stream), V, rowptr, colind, n, w);
  return launch_status();
}

int64_t sn_graph_apsp_max_vertices(void) { return kApspMaxN; }
int32_t sn_graph_apsp_group(int64_t n) { return n < 0 ? 0 : apsp_group(n); }
int32_t sn_graph_apsp_threads(int64_t n) { return n < 0 ? 0 : apsp_threads(n); }

int sn_graph_apsp_sweeps_f32(const int32_t *rowptr, const int32_t *colind, const float *w, int64_t n, int64_t src_begin,
                             int64_t src_count, float *out, int64_t ldo, int32_t *unreached, int32_t *sweeps, void *stream) {
  (void)hipGetLastError();
  if (n < 0 || src_begin < 0 || src_count < 0 || src_begin + src_count > n) return SN_E_SHAPE;
  if (n > kApspMaxN) return SN_E_UNSUPPORTED;                    // S = 1 no longer fits the LDS: nothing is launched
  if (src_count == 0) return SN_OK;
  if (!rowptr || !out) return SN_E_NULL;
  if (!colind != !w) return SN_E_NULL;                           // both NULL: a graph without entries
  if (ldo < n) return SN_E_LD;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int ni = (int)n, sb = (int)src_begin, sc = (int)src_count;
  switch (apsp_group(n)) {
    case 8: return apsp_launch<8>(rowptr, colind, w, ni, sb, sc, out, ldo, unreached, sweeps, s);
    case 4: return apsp_launch<4>(rowptr, colind, w, ni, sb, sc, out, ldo, unreached, sweeps, s);
    case 2: return apsp_launch<2>(rowptr, colind, w, ni, sb, sc, out, ldo, unreached, sweeps, s);
    default: return apsp_launch<1>(rowptr, colind, w, ni, sb, sc, out, ldo, unreached, sweeps, s);
  }
}

int sn_graph_apsp_f32(const int32_t *rowptr, const int32_t *colind, const float *w, int64_t n, int64_t src_begin,
                      int64_t src_count, float *out, int64_t ldo, int32_t *unreached, void *stream) {
  return sn_graph_apsp_sweeps_f32(rowptr, colind, w, n, src_begin, src_count, out, ldo, unreached, nullptr, stream);
}

int sn_symmetrize_min_f32(float *G, int64_t n, int64_t ld, void *stream) {
  (void)hipGetLastError();
  if (n < 0) return SN_E_SHAPE;
  if (n == 0) return SN_OK;
  if (!G) return SN_E_NULL;
  if (ld < n) return SN_E_LD;
  const int64_t nt = (n + kSymTile - 1) / kSymTile;
  if (nt > 65535) return SN_E_RANGE;
  hipLaunchKernelGGL(symmetrize_min_k, dim3((unsigned)nt, (unsigned)nt), dim3(kWG), 0, static_cast<hipStream_t>(stream), G, n, ld);
  return launch_status();
}

size_t sn_mesh_corners_workspace_bytes(int64_t nV) {
  return CornersWs(nullptr, at_least_0(nV)).c.bytes;
}

int sn_mesh_corners_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t *cptr, void *corners,
                        int32_t *status_flag, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!cptr) return SN_E_NULL;
  if (nF > 0 && (!V || !F || !corners)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_corners_workspace_bytes(nV) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CornersWs ws(workspace, nV);
  hipError_t e = sn_internal_fill(cptr, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (status_flag) {
    e = sn_internal_fill(status_flag, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
  }
  if (nF > 0)      // (the flag of this entry point is 1)
    hipLaunchKernelGGL((bucket_count_k<kCornerVertex, kGoodFaces>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, (const int *)nullptr, nF, nV,
                       cptr, status_flag, 1);
  const int st = bucket_offsets(cptr, ws.cursor, ws.sums, nV, s);
  if (st != SN_OK) return st;
  if (nF > 0)
    hipLaunchKernelGGL(corner_fill_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, V, F, nF, nV, ws.cursor, static_cast<MeshCorner *>(corners));
  return launch_status();
}

int sn_mesh_geodesics_sweeps_f32(const int32_t *cptr, const void *corners, int64_t n, int64_t src_begin, int64_t src_count,
                                 float *out, int64_t ldo, int32_t *flags, int32_t *sweeps, void *stream) {
  (void)hipGetLastError();
  if (n < 0 || src_begin < 0 || src_count < 0 || src_begin + src_count > n) return SN_E_SHAPE;
  if (n > kApspMaxN) return SN_E_UNSUPPORTED;                    // S = 1 no longer fits the LDS: nothing is launched
  if (src_count == 0) return SN_OK;
  if (!cptr || !out) return SN_E_NULL;
  if (ldo < n) return SN_E_LD;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const MeshCorner *rec = static_cast<const MeshCorner *>(corners);
  const int ni = (int)n, sb = (int)src_begin, sc = (int)src_count;
  switch (apsp_group(n)) {
    case 8: return mesh_geodesics_launch<8>(cptr, rec, ni, sb, sc, out, ldo, flags, sweeps, s);
    case 4: return mesh_geodesics_launch<4>(cptr, rec, ni, sb, sc, out, ldo, flags, sweeps, s);
    case 2: return mesh_geodesics_launch<2>(cptr, rec, ni, sb, sc, out, ldo, flags, sweeps, s);
    default: return mesh_geodesics_launch<1>(cptr, rec, ni, sb, sc, out, ldo, flags, sweeps, s);
  }
}

int sn_mesh_geodesics_f32(const int32_t *cptr, const void *corners, int64_t n, int64_t src_begin, int64_t src_count,
                          float *out, int64_t ldo, int32_t *flags, void *stream) {
  return sn_mesh_geodesics_sweeps_f32(cptr, corners, n, src_begin, src_count, out, ldo, flags, nullptr, stream);
}

size_t sn_mesh_glue_workspace_bytes(int64_t nV, int64_t nF) {
  return MeshBucketWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes;
}

int sn_mesh_glue_i32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t *G, double *l, int32_t *status,
                     void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!status) return SN_E_NULL;
  if (nF > 0 && (!F || !G)) return SN_E_NULL;
  if (!V != !l && nF > 0) return SN_E_NULL;                      // the lengths need the coordinates, and nothing else does
  if (workspace_bytes < sn_mesh_glue_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const BucketWs b = MeshBucketWs(workspace, nV, nF).b;
  hipError_t e = sn_internal_fill(b.ptr, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF == 0) return SN_OK;
  hipLaunchKernelGGL((bucket_count_k<kCornerVertex, kGoodFaces>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F,
                     (const int *)nullptr, nF, nV, b.ptr, status, SN_IDT_BAD_FACE);
  const int st = bucket_offsets(b.ptr, b.cursor, b.sums, nV, s);
  if (st != SN_OK) return st;
  hipLaunchKernelGGL((bucket_fill_k<kCornerVertex, kGoodFaces, 3>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, (const int *)nullptr, nF, nV,
                     b.cursor, b.bucket);
  hipLaunchKernelGGL(glue_twin_k, dim3(grid_for(3 * nF, kWG)), dim3(kWG), 0, s, V, F, nF, nV, b.ptr, b.bucket, G, l, status);
  return launch_status();
}

size_t sn_mesh_idt_workspace_bytes(int64_t nF) { return one_slice_bytes<idt_claim_t>(at_least_0(nF)); }

int sn_mesh_idt_rounds_f64(int32_t *Fp, double *lp, int32_t *G, int64_t nF, int32_t round_begin, int32_t round_count,
                           int32_t max_rounds, int32_t *counters, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream) {
  (void)hipGetLastError();
  if (nF < 0 || round_begin < 0 || round_count < 0 || max_rounds < 0 || (int64_t)round_begin + round_count > max_rounds)
    return SN_E_SHAPE;
  if (3 * nF > INT_MAX || max_rounds > kIdtMaxRounds) return SN_E_RANGE;
  if (!status || (round_count > 0 && !counters)) return SN_E_NULL;
  if (nF > 0 && (!Fp || !lp || !G)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_idt_workspace_bytes(nF) || !workspace) return SN_E_WORKSPACE;
  if (round_count == 0) return SN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  idt_claim_t *claim = static_cast<idt_claim_t *>(workspace);
  hipError_t e = sn_internal_fill(counters + 2 * (int64_t)round_begin, 0, (size_t)round_count * 2 * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF == 0) return SN_OK;
  if (round_begin == 0) {
    e = sn_internal_fill(claim, 0xff, (size_t)nF * sizeof(idt_claim_t), s);
    if (e != hipSuccess) return (int)e;
  }
  const int64_t nS = 3 * nF;
  for (int r = round_begin; r < round_begin + round_count; ++r) {
    hipLaunchKernelGGL(idt_claim_k, dim3(grid_for(nS, kWG)), dim3(kWG), 0, s, lp, G, nS, claim, (unsigned)r, r == max_rounds - 1 ? 1 : 0,
                       counters + 2 * (int64_t)r, status);
    hipLaunchKernelGGL(idt_flip_k, dim3(grid_for(nS, kWG)), dim3(kWG), 0, s, Fp, lp, G, nS, claim, (unsigned)r, counters + 2 * (int64_t)r,
                       status);
  }
  return launch_status();
}

int64_t sn_mesh_idt_laplacian_items(int64_t nV, int64_t nF) { return nV < 0 || nF < 0 ? 0 : 12 * nF + nV; }

size_t sn_mesh_idt_laplacian_workspace_bytes(int64_t nV, int64_t nF) {
  return IdtLapWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes;
}

int sn_mesh_idt_laplacian_f32(const int32_t *Fp, const double *lp, int64_t nV, int64_t nF, int32_t phase, int64_t *keys,
                              const int64_t *order, int32_t *rowptr, int32_t *colind, float *vals, int32_t *status,
                              void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0 || phase < 0 || phase > 2) return SN_E_SHAPE;
  const int64_t N = 12 * nF + nV, nFk = nF > 0 ? nF : 1, span = 16 * nFk;
  if (nV + 1 > INT_MAX || N + 1 > INT_MAX) return SN_E_RANGE;
  if ((long double)nV * (long double)nV * (long double)span >= 9.0e18L) return SN_E_RANGE;      // the sort key is one int64
  if (workspace_bytes < sn_mesh_idt_laplacian_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  if (N > 0 && !keys) return SN_E_NULL;
  if (nF > 0 && (!Fp || !lp)) return SN_E_NULL;
  if (phase > 0 && ((N > 0 && !order) || !rowptr)) return SN_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const IdtLapWs ws(workspace, nV, nF);
  if (phase == 0) {
    if (N > 0) hipLaunchKernelGGL(idt_contrib_k, dim3(grid_for(nF + nV, kWG)), dim3(kWG), 0, s, Fp, lp, nV, nF, keys, ws.cval, ws.cmass, status);
  } else if (phase == 1) {
    hipLaunchKernelGGL(idt_heads_k, dim3(grid_for(N + 1, kWG)), dim3(kWG), 0, s, keys, N, span, ws.hs);
    scan_in_place(ws.hs, N + 1, ws.sums, s);
    hipLaunchKernelGGL(idt_rowptr_k, dim3(grid_for(nV + 1, kWG)), dim3(kWG), 0, s, keys, N, nV, span, ws.hs, rowptr);
  } else if (N > 0) {
    if (!colind || !vals) return SN_E_NULL;
    hipLaunchKernelGGL((idt_entries_k<true>), dim3(grid_for(N, kWG)), dim3(kWG), 0, s, keys, order, N, nV, span, ws.hs, ws.cmass, ws.A,
                       (int *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL((idt_entries_k<false>), dim3(grid_for(N, kWG)), dim3(kWG), 0, s, keys, order, N, nV, span, ws.hs, ws.cval, ws.A,
                       colind, vals);
  }
  return launch_status();
}

size_t sn_mesh_components_workspace_bytes(int64_t nV, int64_t nF, int32_t mode) {
  return ComponentsWs(nullptr, at_least_0(nV), at_least_0(nF), mode == SN_CC_EDGE).c.bytes;
}

int sn_mesh_components_i32(const int32_t *F, int64_t nV, int64_t nF, int32_t mode, int32_t *vlabel, int32_t *flabel,
                           int32_t *count, int32_t *summary, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0 || (mode != SN_CC_EDGE && mode != SN_CC_VERTEX)) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  const bool vertex = mode == SN_CC_VERTEX;
  const int64_t n = vertex ? nV : nF;
  if (!summary || !status) return SN_E_NULL;
  if (nF > 0 && (!F || !flabel)) return SN_E_NULL;
  if (n > 0 && !count) return SN_E_NULL;
  if (vertex && nV > 0 && !vlabel) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_components_workspace_bytes(nV, nF, mode) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const ComponentsWs ws(workspace, nV, nF, !vertex);
  cc_word_t *acc = ws.acc;
  hipError_t e = sn_internal_fill(acc, 0, 2 * sizeof(cc_word_t), s);
  if (e != hipSuccess) return (int)e;
  e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  int *parent = vertex ? vlabel : flabel;
  if (n > 0) hipLaunchKernelGGL(cc_init_k, dim3(grid_for(n, kWG)), dim3(kWG), 0, s, parent, count, n);
  if (vertex) {
    if (nF > 0) hipLaunchKernelGGL(cc_vertex_union_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, nF, nV, parent, status);
    if (nV > 0) hipLaunchKernelGGL(cc_flatten_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, parent, nV, status);
    if (nF > 0) hipLaunchKernelGGL((cc_face_labels_k<true>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, nF, nV, vlabel, flabel, count, status);
  } else if (nF > 0) {
    const BucketWs &b = ws.b;
    e = sn_internal_fill(b.ptr, 0, (size_t)(nV + 1) * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((bucket_count_k<kLowerEnd, kGoodFaces>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F,
                       (const int *)nullptr, nF, nV, b.ptr, status, SN_CC_BAD_FACE);
    const int st = bucket_offsets(b.ptr, b.cursor, b.sums, nV, s);
    if (st != SN_OK) return st;
    hipLaunchKernelGGL((bucket_fill_k<kLowerEnd, kGoodFaces, 3>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, (const int *)nullptr, nF, nV,
                       b.cursor, b.bucket);
    hipLaunchKernelGGL(cc_edge_union_k, dim3(grid_for(3 * nF, kWG)), dim3(kWG), 0, s, F, nF, nV, b.ptr, b.bucket, parent, status);
    hipLaunchKernelGGL((cc_face_labels_k<false>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, nF, nV, (const int *)nullptr, flabel, count, status);
    hipLaunchKernelGGL(cc_bad_labels_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, nF, nV, flabel);
  }
  if (n > 0) hipLaunchKernelGGL(cc_winner_k, dim3(grid_for(n, kWG)), dim3(kWG), 0, s, count, n, acc);
  hipLaunchKernelGGL(cc_summary_k, dim3(1), dim3(64), 0, s, acc, summary);
  return launch_status();
}

int sn_mesh_label_mask_i32(const int32_t *flabel, int64_t nF, const int32_t *label, int32_t *keep, void *stream) {
  (void)hipGetLastError();
  if (nF < 0) return SN_E_SHAPE;
  if (3 * nF > INT_MAX) return SN_E_RANGE;
  if (nF == 0) return SN_OK;
  if (!flabel || !label || !keep) return SN_E_NULL;
  hipLaunchKernelGGL(label_mask_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, static_cast<hipStream_t>(stream), flabel, nF, label, keep);
  return launch_status();
}

size_t sn_mesh_compact_workspace_bytes(int64_t nV, int64_t nF) {
  return CompactWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes;
}

int sn_mesh_compact_i32(const float *V, const int32_t *F, const int32_t *keep, int64_t nV, int64_t nF, int32_t *I, int32_t *J,
                        int32_t *Fsrc, int32_t *Fnew, float *Vnew, int32_t *sizes, void *workspace, size_t workspace_bytes,
                        void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!sizes) return SN_E_NULL;
  if (nF > 0 && (!F || !keep || !Fsrc || !Fnew)) return SN_E_NULL;
  if (nV > 0 && (!I || !J)) return SN_E_NULL;
  if (nV > 0 && !V != !Vnew) return SN_E_NULL;                     // the coordinates are copied when both are given
  if (workspace_bytes < sn_mesh_compact_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CompactWs ws(workspace, nV, nF);
  int *vpos = ws.vpos, *fpos = ws.fpos, *sums = ws.sums;
  hipError_t e = sn_internal_fill(vpos, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(compact_mark_k, dim3(grid_for(nF + 1, kWG)), dim3(kWG), 0, s, F, keep, nF, nV, fpos, vpos);
  scan_in_place(fpos, nF + 1, sums, s);
  scan_in_place(vpos, nV + 1, sums, s);
  hipLaunchKernelGGL(compact_vertices_k, dim3(grid_for(nV + 1, kWG)), dim3(kWG), 0, s, V, nV, vpos, I, J, Vnew, fpos, nF, sizes);
  if (nF > 0) hipLaunchKernelGGL(compact_faces_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, nF, fpos, vpos, Fsrc, Fnew);
  return launch_status();
}

size_t sn_mesh_descriptors_workspace_bytes(int64_t nV, int64_t nF) {
  return MeshBucketWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes;
}

int sn_mesh_descriptors_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, float *face_area, float *face_normal,
                            float *n_area, float *n_uniform, float *n_angle, float *mass_bary, float *mass_voronoi,
                            float *gauss, float *mean, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!status) return SN_E_NULL;
  const bool per_vertex = n_area || n_uniform || n_angle || mass_bary || mass_voronoi || gauss || mean;
  if ((nF > 0 && (!V || !F)) || (nV > 0 && per_vertex && !V)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_descriptors_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const BucketWs b = MeshBucketWs(workspace, nV, nF).b;
  int *vptr = b.ptr, *inc = b.bucket;
  hipError_t e = sn_internal_fill(vptr, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF > 0) hipLaunchKernelGGL(desc_face_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, V, F, nF, nV, vptr, face_area, face_normal, status);
  if (per_vertex && nV > 0) {
    const int st = incidence_build(F, nV, nF, b, s);
    if (st != SN_OK) return st;
    hipLaunchKernelGGL(desc_vertex_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, n_area, n_uniform, n_angle, mass_bary,
                       mass_voronoi, gauss, mean, status);
  }
  return launch_status();
}

size_t sn_mesh_cot_laplacian_workspace_bytes(int64_t nV, int64_t nF) { return sn_mesh_descriptors_workspace_bytes(nV, nF); }

}  // extern "C"

namespace {

// both phases of sn_mesh_cot_laplacian_f32 (vals) and of sn_mesh_cot_pencil_f64 (vals64 and mass64) after their argument checks
int cot_rows_phases(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase, int voronoi, int32_t clamp, double hack,
                    int32_t *rowptr, int32_t *colind, float *vals, double *vals64, double *mass64, int32_t *status, void *workspace,
                    void *stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const BucketWs b = MeshBucketWs(workspace, nV, nF).b;
  int *vptr = b.ptr, *inc = b.bucket;
  if (phase == 0) {
    hipError_t e = sn_internal_fill(vptr, 0, (size_t)(nV + 1) * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    e = sn_internal_fill(status, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (nF > 0)
      hipLaunchKernelGGL(desc_face_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, V, F, nF, nV, vptr, (float *)nullptr, (float *)nullptr, status);
    const int st = incidence_build(F, nV, nF, b, s);
    if (st != SN_OK) return st;
    e = sn_internal_fill(rowptr + nV, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (nV > 0)
      hipLaunchKernelGGL((cot_laplacian_rows_k<false>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, voronoi, 0, 0.f, rowptr,
                         (int *)nullptr, (float *)nullptr, status);
    scan_in_place(rowptr, nV + 1, b.sums, s);
  } else if (nV > 0 && vals64) {
    hipLaunchKernelGGL((cot_laplacian_rows_k<true, true>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, voronoi, 0, 0.f,
                       rowptr, colind, (float *)nullptr, status, vals64, mass64);
  } else if (nV > 0) {
    hipLaunchKernelGGL((cot_laplacian_rows_k<true>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, F, nV, vptr, inc, voronoi, clamp != 0,
                       (float)hack, rowptr, colind, vals, status);
  }
  return launch_status();
}

}  // namespace

extern "C" {

int sn_mesh_cot_laplacian_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase, int32_t mass, int32_t clamp,
                              double hack, int32_t *rowptr, int32_t *colind, float *vals, int32_t *status, void *workspace,
                              size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0 || (phase != 0 && phase != 1)) return SN_E_SHAPE;
  if (mass != SN_DESC_MASS_BARYCENTRIC && mass != SN_DESC_MASS_VORONOI) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!rowptr || !status) return SN_E_NULL;
  if ((nF > 0 || nV > 0) && (!V || (nF > 0 && !F))) return SN_E_NULL;
  if (phase == 1 && nV > 0 && (!colind || !vals)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_cot_laplacian_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  return cot_rows_phases(V, F, nV, nF, phase, mass == SN_DESC_MASS_VORONOI, clamp, hack, rowptr, colind, vals, nullptr, nullptr, status,
                         workspace, stream);
}

int sn_mesh_cot_pencil_f64(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t phase, int32_t *rowptr, int32_t *colind,
                           double *S, double *mass, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0 || (phase != 0 && phase != 1)) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!rowptr || !status) return SN_E_NULL;
  if ((nF > 0 || nV > 0) && (!V || (nF > 0 && !F))) return SN_E_NULL;
  if (phase == 1 && nV > 0 && (!colind || !S || !mass)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_cot_laplacian_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  return cot_rows_phases(V, F, nV, nF, phase, 1, 0, 0.0, rowptr, colind, nullptr, S, mass, status, workspace, stream);
}

size_t sn_mesh_weld_workspace_bytes(int64_t nV) {
  if (nV < 0 || nV > kRepairMaxNodes) nV = 0;
  return one_slice_bytes<int>(repair_table_slots(nV));
}

int sn_mesh_weld_f32(const float *V, const int32_t *F, int64_t nV, int64_t nF, double tol, int32_t weld, int32_t *rep, int32_t *Fw,
                     int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0 || !(tol >= 0) || !(tol <= 1.7976931348623157e308)) return SN_E_SHAPE;
  if (nV > kRepairMaxNodes || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!counts || !status) return SN_E_NULL;
  if (nV > 0 && (!V || !rep)) return SN_E_NULL;
  if (nF > 0 && (!F || !Fw)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_weld_workspace_bytes(nV) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int *table = static_cast<int *>(workspace);
  const uint32_t slots = repair_table_slots(nV);
  hipError_t e = sn_internal_fill(counts, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nV > 0) {
    if (weld) {
      e = sn_internal_fill(table, 0xff, (size_t)slots * sizeof(int), s);                    // kRepairEmpty in every slot
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL((repair_insert_k<false>), dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, (const int *)nullptr, nV, nV, tol, table,
                         slots - 1, status);
    }
    hipLaunchKernelGGL(weld_rep_k, dim3(grid_for(nV, kWG)), dim3(kWG), 0, s, V, nV, tol, (int)weld, table, slots - 1, rep, counts, status);
  }
  if (nF > 0) hipLaunchKernelGGL(weld_faces_k, dim3(grid_for(3 * nF, kWG)), dim3(kWG), 0, s, V, F, nF, nV, tol, (int)weld, rep, Fw, status);
  return launch_status();
}

size_t sn_mesh_unique_faces_workspace_bytes(int64_t nF) {
  if (nF < 0 || nF > kRepairMaxNodes) nF = 0;
  return one_slice_bytes<int>(repair_table_slots(nF));
}

int sn_mesh_unique_faces_i32(const float *V, const int32_t *F, int64_t nV, int64_t nF, int32_t unique, int32_t *keep,
                             int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || 3 * nF > INT_MAX) return SN_E_RANGE;
  if (!counts || !status) return SN_E_NULL;
  if (nF > 0 && (!F || !keep)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_unique_faces_workspace_bytes(nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int *table = static_cast<int *>(workspace);
  const uint32_t slots = repair_table_slots(nF);
  hipError_t e = sn_internal_fill(counts, 0, 3 * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF == 0) return launch_status();
  if (unique) {
    e = sn_internal_fill(table, 0xff, (size_t)slots * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((repair_insert_k<true>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, (const float *)nullptr, F, nF, nV, 0.0, table,
                       slots - 1, status);
  }
  hipLaunchKernelGGL(unique_keep_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, V, F, nF, nV, (int)unique, table, slots - 1, keep, counts,
                     status);
  return launch_status();
}

size_t sn_mesh_orient_workspace_bytes(int64_t nV, int64_t nF) {
  return OrientWs(nullptr, at_least_0(nV), at_least_0(nF)).c.bytes;
}

int sn_mesh_orient_i32(const int32_t *F, const int32_t *keep, int64_t nV, int64_t nF, int32_t *flip, int32_t *label, int32_t *Fout,
                       int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
  (void)hipGetLastError();
  if (nV < 0 || nF < 0) return SN_E_SHAPE;
  if (nV + 1 > INT_MAX || nF >= kRepairMaxNodes) return SN_E_RANGE;        // a face id and its parity bit share one int32
  if (!counts || !status) return SN_E_NULL;
  if (nF > 0 && (!F || !keep || !flip || !label)) return SN_E_NULL;
  if (workspace_bytes < sn_mesh_orient_workspace_bytes(nV, nF) || !workspace) return SN_E_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const OrientWs ws(workspace, nV, nF);
  const BucketWs &b = ws.b;
  int *conflict = ws.conflict;
  hipError_t e = sn_internal_fill(counts, 0, 3 * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  e = sn_internal_fill(status, 0, sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  if (nF == 0) return launch_status();
  e = sn_internal_fill(b.ptr, 0, (size_t)(nV + 1) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(or_init_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, label, conflict, nF);
  hipLaunchKernelGGL((bucket_count_k<kLowerEnd, kGoodKeptFaces>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, keep, nF, nV,
                     b.ptr, status, SN_REPAIR_BAD_FACE);
  const int st = bucket_offsets(b.ptr, b.cursor, b.sums, nV, s);
  if (st != SN_OK) return st;
  hipLaunchKernelGGL((bucket_fill_k<kLowerEnd, kGoodKeptFaces, 3>), dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, keep, nF, nV, b.cursor,
                     b.bucket);
  hipLaunchKernelGGL(or_link_k, dim3(grid_for(3 * nF, kWG)), dim3(kWG), 0, s, F, keep, nF, nV, b.ptr, b.bucket, label, conflict, counts, status);
  hipLaunchKernelGGL(or_resolve_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, label, conflict, nF, status);
  hipLaunchKernelGGL(or_finish_k, dim3(grid_for(nF, kWG)), dim3(kWG), 0, s, F, keep, nF, nV, label, conflict, flip, Fout, counts, status);
  return launch_status();
}

}  // extern "C"

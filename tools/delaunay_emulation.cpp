// Host emulation of surfacenetworks_amd/csrc/sn_delaunay.hip with ONE lane per workgroup: the kernel source itself, compiled by a
// host C++ compiler behind stub definitions of the HIP keywords.  The kernels are written as strided loops between barriers, so
// with a workgroup size of 1 every phase runs to its end before the next starts and the results are the device's (they do not
// depend on thread timing).  It checks the algorithm and, built with -fsanitize=address,undefined, every index — not the
// interplay of lanes.  tests/test_delaunay_emulation.py builds and runs it; by hand:
//   sed -e '/hip_runtime.h/d' -e 's/kWG = 256/kWG = 1/' surfacenetworks_amd/csrc/sn_delaunay.hip > /tmp/sn_delaunay_host.inc
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include -DSN_DELAUNAY_SOURCE='"/tmp/sn_delaunay_host.inc"' \
//       tools/delaunay_emulation.cpp -o /tmp/delaunay_emulation
// Usage: delaunay_emulation dt|digits IN OUT — little-endian int32 / int64 records, written and read by the test.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define __device__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __syncthreads() ((void)0)
struct dim3 {
  unsigned x;
  dim3(unsigned a) : x(a) {}
};
static struct { int x; } threadIdx = {0}, blockIdx = {0};
typedef int hipError_t;
typedef void *hipStream_t;
static const int hipSuccess = 0;
static int hipGetLastError() { return 0; }
static int atomicMin(int *p, int v) { const int o = *p; if (v < o) *p = v; return o; }
static int atomicOr(int *p, int v) { const int o = *p; *p |= v; return o; }
static int atomicAdd(int *p, int v) { const int o = *p; *p += v; return o; }
#define hipLaunchKernelGGL(k, g, b, sh, st, ...)                                       \
  do {                                                                                 \
    for (unsigned bb_ = 0; bb_ < (g).x; ++bb_) { blockIdx.x = (int)bb_; k(__VA_ARGS__); } \
  } while (0)
#include SN_DELAUNAY_SOURCE

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  int rc;
  if (!strcmp(argv[1], "dt")) {                // header: B, Nmax, max_rounds; count[B]; P[B][Nmax][2]
    const std::vector<int64_t> h = take<int64_t>(in, 3);
    const int64_t B = h[0], N = h[1];
    std::vector<int32_t> count = take<int32_t>(in, B), P = take<int32_t>(in, B * N * 2);
    std::vector<int32_t> F(B * N * 6), nF(B), status(B), counts(B * 4);
    rc = sn_delaunay2d_i32(P.data(), count.data(), B, N, (int32_t)h[2], F.data(), nF.data(), status.data(), counts.data(), nullptr);
    put(out, nF); put(out, status); put(out, counts); put(out, F);
  } else {                                     // header: B, rows, cols, R, min_points, min_det, seed, image_base; images
    const std::vector<int64_t> h = take<int64_t>(in, 8);
    const int64_t B = h[0], N = sn_poisson_disc_cells(h[2] - 1, h[1] - 1, h[3]);
    if (N < 0) return 3;
    std::vector<uint8_t> img = take<uint8_t>(in, B * h[1] * h[2]);
    std::vector<int32_t> P(B * N * 2), count(B), F(B * N * 6), nF(B), status(B), attempts(B), counts(B * 4), steps(B);
    std::vector<float> V(B * N * 3);
    rc = sn_mesh_digits_u8(img.data(), B, (int32_t)h[1], (int32_t)h[2], (uint64_t)h[6], h[7], h[3], (int32_t)h[4], h[5],
                           SN_MESHDIGITS_MAX_ATTEMPTS, 4096, N, P.data(), count.data(), V.data(), F.data(), nF.data(), status.data(),
                           attempts.data(), counts.data(), nullptr);
    put(out, count); put(out, nF); put(out, status); put(out, attempts); put(out, P); put(out, V); put(out, F);
    if (rc == 0) rc = sn_poisson_disc_i32((uint64_t)h[6], h[7], 0, h[2] - 1, h[1] - 1, h[3], B, N, P.data(), count.data(), steps.data(), nullptr);
    put(out, count); put(out, steps);
  }
  fclose(out);
  return rc == 0 ? 0 : 4;
}

// zk_point_grid.h -- the uniform bin grid over a 2-D point set, shared by the searches that walk it (the cells of
// zk_voronoi.hip, the nearest neighbours of zk_knn.hip).  The single owner of:
//
//   points       load_points_kernel: (N, 2) ZK_F64 as they are or ZK_I32 widened exactly, to double2; a NaN or inf raises
//                ERR_NONFINITE in the caller's flag word.
//   side         grid_side: G = ceil(sqrt(N / 2)) bins per axis (about two points a bin on a uniform set), at most MAX_GRID.
//   frame        zk_grid_frame: origin, bin side and G, in device memory.  The CONSUMER's kernel chooses it (the frames
//                differ); every point must lie in [x0, x0 + h G] x [y0, y0 + h G] up to rounding, which bin_of clamps.  Its
//                bin_x / bin_y / key are the only statement of the binning rule: the sort key and the searches call them.
//   bins         build_point_grid: keys by bin_key_kernel, a radix sort of (key, index) pairs (rocPRIM), then
//                bin_start_kernel: bin starts are lower bounds in the sorted keys, and the points are gathered into bin order.
//                It leaves spts, sidx and bin_start (G G + 1 entries) for the search.
//
// Loading and building are two steps: a caller may read the flag, or return, before any frame exists.
//
// This header is compiled under each includer's flags, and zk_knn.o is built with -ffp-contract=off where zk_voronoi.o is
// not.  The device expressions here are subtract, divide, floor, compare and integer arithmetic only: nothing of the shape
// a * b + c that contraction could fuse, so both objects bin alike.  Keep it so; a frame kernel, a clip or a distance does not
// belong here.  Everything has internal linkage: each object keeps its own device copy.
#pragma once

#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int MAX_GRID = 4096;                       // bins per axis at most (bin keys fit 24 bits)

enum { ERR_NONFINITE = 1 };                          // the flag bit of load_points_kernel

inline int grid_side(int64_t n) {
  int g = (int)ceil(sqrt((double)n / 2));
  return g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g);
}

__device__ inline int bin_of(double u, int g) {
  const double f = floor(u);
  return f >= (double)(g - 1) ? g - 1 : (f > 0 ? (int)f : 0);      // NaN goes to 0
}

struct zk_grid_frame {
  double x0, y0, h;                                  // grid origin and bin side
  int g;                                             // bins per axis
  __device__ int bin_x(double x) const { return bin_of((x - x0) / h, g); }
  __device__ int bin_y(double y) const { return bin_of((y - y0) / h, g); }
  __device__ unsigned key(double2 p) const { return (unsigned)(bin_y(p.y) * g + bin_x(p.x)); }
};

__global__ __launch_bounds__(256) void load_points_kernel(const void* __restrict__ in, int dtype, long long n, double2* __restrict__ pts,
                                                          int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x, y;
  if (dtype == ZK_I32) {
    x = (double)((const int*)in)[2 * i];
    y = (double)((const int*)in)[2 * i + 1];
  } else {
    x = ((const double*)in)[2 * i];
    y = ((const double*)in)[2 * i + 1];
  }
  if (!(fabs(x) <= 1.7976931348623157e308) || !(fabs(y) <= 1.7976931348623157e308)) atomicOr(flag, ERR_NONFINITE);
  pts[i] = make_double2(x, y);
}

__global__ __launch_bounds__(256) void bin_key_kernel(const double2* __restrict__ pts, long long n, const zk_grid_frame* __restrict__ fi,
                                                      unsigned* __restrict__ keys, int* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const zk_grid_frame f = *fi;
  keys[i] = f.key(pts[i]);
  idx[i] = (int)i;
}

// bin_start[b] = first sorted point of bin b, b in [0, bins]; spts = the points in sorted order
__global__ __launch_bounds__(256) void bin_start_kernel(const unsigned* __restrict__ skeys, const int* __restrict__ sidx,
                                                        const double2* __restrict__ pts, long long n, long long bins,
                                                        int* __restrict__ bin_start, double2* __restrict__ spts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i <= bins) {
    long long lo = 0, hi = n;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((long long)skeys[mid] < i) lo = mid + 1;
      else hi = mid;
    }
    bin_start[i] = (int)lo;
  }
  if (i < n) spts[i] = pts[sidx[i]];
}

// what a search reads, and the buffers behind it
struct point_grid {
  const double2* spts = nullptr;                     // the points in bin order
  const int* sidx = nullptr;                         // their indices in the caller's order
  const int* bin_start = nullptr;                    // g * g + 1 entries
  dev_buf keys, idx, bin, sorted;
};

// Bins the n loaded points `pts` by the frame `frame` (device memory, written on `s` before this call) with g = grid_side(n).
int build_point_grid(point_grid* gr, temp_store& tmp, const double2* pts, int64_t n, int g, const zk_grid_frame* frame, hipStream_t s) {
  int rc;
  const long long bins = (long long)g * g;
  int key_bits = 1;
  while (((long long)1 << key_bits) < bins) ++key_bits;
  if ((rc = gr->keys.alloc(sizeof(unsigned) * 2 * (size_t)n)) || (rc = gr->idx.alloc(sizeof(int) * 2 * (size_t)n)) ||
      (rc = gr->bin.alloc(sizeof(int) * (size_t)(bins + 1))) || (rc = gr->sorted.alloc(sizeof(double2) * (size_t)n)))
    return rc;
  unsigned *k_in = gr->keys.as<unsigned>(), *k_out = k_in + n;
  int *i_in = gr->idx.as<int>(), *i_out = i_in + n;
  hipLaunchKernelGGL(bin_key_kernel, dim3(blocks_of(n)), dim3(256), 0, s, pts, (long long)n, frame, k_in, i_in);
  ZK_HIP(hipGetLastError());
  if ((rc = zk_prim(tmp, [&](void* p, size_t& b) { return rocprim::radix_sort_pairs(p, b, k_in, k_out, i_in, i_out, (size_t)n, 0, key_bits, s); })))
    return rc;
  const long long span = bins + 1 > n ? bins + 1 : n;
  hipLaunchKernelGGL(bin_start_kernel, dim3(blocks_of(span)), dim3(256), 0, s, k_out, i_out, pts, (long long)n, bins, gr->bin.as<int>(),
                     gr->sorted.as<double2>());
  gr->spts = gr->sorted.as<double2>();
  gr->sidx = i_out;
  gr->bin_start = gr->bin.as<int>();
  return 0;
}

}  // namespace

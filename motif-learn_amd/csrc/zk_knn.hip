// zk_knn.hip -- the passes over the data of the reference's graph/vnn.py estimate_d on the device: a 12-nearest-neighbour
// distance matrix and the reductions its Otsu / Li thresholds are made of.  Built with -ffp-contract=off, as zk_refine.hip is.
//
// A. zk_knn_distances.  The k <= 12 smallest Euclidean distances of every point to the points of the set, itself included
//   (column 0 is 0), ascending.
//   frame        one workgroup: the bounding box of the points (min / max are order-free), with square bins over it.
//   bins         the point grid of zk_point_grid.h over that box.
//   search       one lane per point in bin order.  The running list of 12 distances lives in registers (an insertion network
//                unrolled over the 12 slots, no run-time index).  Bins are visited in rings of growing Chebyshev distance r
//                around the point's own bin; every point not yet seen lies outside the box of the rings searched, so the
//                search ends at the first ring where the k-th best is no farther than the nearest side of that box that is
//                not a side of the grid (less a relative slack of 1e-9 of the grid's side, far past any rounding of the
//                binning), or when the rings have covered the grid.  Distances are sqrt(dx * dx + dy * dy) in float64, not
//                fused.
//
// B. zk_knn_stats.  One reduction per call over the (N, 12) distance matrix dd, for the eleven nested samples
//   d_k = dd[:, 1:k], k = 2 .. 12 (element (i, j) belongs to every k > j):
//   ZK_KNN_RANGES   min of column 1 and max of columns 1 .. 11 (rows are ascending: the range of d_k is [min col 1, max col k-1])
//   ZK_KNN_HIST     the eleven 256-bin histograms of np.histogram(d_k, bins=256) in one pass: 11 x 256 int32 counters in LDS,
//                   merged into global counters with integer atomics.  The bin of a value is NumPy's own rule (zk_np_bins.h):
//                   the index (v - first) / (last - first) * 256 truncated, 256 folded into 255, one step down when
//                   v < edges[index], one step up when v >= edges[index + 1] and the bin is not the last; the edges are the
//                   caller's (np.linspace).
//   ZK_KNN_SIDES    with w = v - shift and eleven thresholds t_k: the number of w > t_k, their sum and the sum of the rest, per
//                   k.  Sums go through a fixed tree (a strided sequential sum per lane, wave shuffles, the four waves of a
//                   workgroup in order, then the workgroups in order): no floating-point atomics, two runs agree bit for bit.
//   ZK_KNN_GAPS     the smallest positive difference between two values of w = v - shift within each d_k: a radix sort of the
//                   float64 bit patterns (w >= 0, so they order as integers) and a minimum over adjacent differences
//                   (atomicMin on the bit pattern: order-free).
//   The scalar rules on these few hundred numbers (Otsu's argmax, Li's iteration, the score) are the host's (graph.py).
#include <math.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "zk_internal.h"
#include "zk_np_bins.h"
#include "zk_point_grid.h"
#include "zk_scratch.h"

namespace {

typedef unsigned long long u64;

constexpr int KNN = 12;                              // columns of the distance matrix
constexpr int NK = 11;                               // the samples d_2 .. d_12
constexpr int RED_BLOCKS = 512;                      // workgroups of a reduction at most
constexpr double SLACK = 1e-9;
constexpr double DBL_BIG = 1.7976931348623157e308;

// ---------------------------------------------------------------------------------------------------------------------
// A. nearest-neighbour distances
// ---------------------------------------------------------------------------------------------------------------------

// one workgroup: the bounding box and the grid over it
__global__ __launch_bounds__(1024) void knn_frame_kernel(const double2* __restrict__ pts, long long n, int g, zk_grid_frame* __restrict__ out) {
  __shared__ double s[4][1024];
  const int t = threadIdx.x;
  double xlo = DBL_BIG, xhi = -DBL_BIG, ylo = DBL_BIG, yhi = -DBL_BIG;
  for (long long i = t; i < n; i += 1024) {
    xlo = fmin(xlo, pts[i].x);
    xhi = fmax(xhi, pts[i].x);
    ylo = fmin(ylo, pts[i].y);
    yhi = fmax(yhi, pts[i].y);
  }
  s[0][t] = xlo;
  s[1][t] = xhi;
  s[2][t] = ylo;
  s[3][t] = yhi;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (t < d) {
      s[0][t] = fmin(s[0][t], s[0][t + d]);
      s[1][t] = fmax(s[1][t], s[1][t + d]);
      s[2][t] = fmin(s[2][t], s[2][t + d]);
      s[3][t] = fmax(s[3][t], s[3][t + d]);
    }
    __syncthreads();
  }
  if (t == 0) {
    zk_grid_frame f;
    const double span = fmax(s[1][0] - s[0][0], s[3][0] - s[2][0]);
    f.x0 = s[0][0];
    f.y0 = s[2][0];
    f.h = span > 0 && span <= DBL_BIG ? span / (double)g : 1.0;
    f.g = g;
    *out = f;
  }
}

// the running list: best[0] <= ... <= best[11]; d takes its place and the largest falls out (no run-time index: registers)
__device__ inline void insert12(double (&best)[KNN], double d) {
#pragma unroll
  for (int j = 0; j < KNN; ++j) {
    const double lo = fmin(best[j], d), hi = fmax(best[j], d);
    best[j] = lo;
    d = hi;
  }
}

__device__ inline void scan_range(const double2* __restrict__ spts, int lo, int hi, double px, double py, double (&best)[KNN]) {
  for (int m = lo; m < hi; ++m) {
    const double dx = spts[m].x - px, dy = spts[m].y - py;
    insert12(best, sqrt(dx * dx + dy * dy));
  }
}

__global__ __launch_bounds__(64) void knn_kernel(const double2* __restrict__ spts, const int* __restrict__ sidx,
                                                 const int* __restrict__ bin_start, long long n, const zk_grid_frame* __restrict__ fi, int k,
                                                 const int* __restrict__ flag, double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
  if (t >= n || (*flag & ERR_NONFINITE)) return;     // set before this launch; with a NaN no search would ever stop
  const zk_grid_frame f = *fi;
  const int g = f.g;
  const double px = spts[t].x, py = spts[t].y;
  double best[KNN];
#pragma unroll
  for (int j = 0; j < KNN; ++j) best[j] = INFINITY;
  const int bx = f.bin_x(px), by = f.bin_y(py);
  int reach = bx > g - 1 - bx ? bx : g - 1 - bx;
  reach = by > reach ? by : reach;
  reach = g - 1 - by > reach ? g - 1 - by : reach;
  const double e = SLACK * f.h * g;
  for (int r = 0; r <= reach; ++r) {
    if (r > 0) {                                     // the points not yet seen lie outside the box of the rings before r
      double kth = best[0];
#pragma unroll
      for (int j = 1; j < KNN; ++j) kth = j == k - 1 ? best[j] : kth;
      double bound = INFINITY;                       // distance to the nearest side of that box that is not a side of the grid
      if (bx - r + 1 > 0) bound = fmin(bound, px - (f.x0 + f.h * (bx - r + 1)));
      if (bx + r < g) bound = fmin(bound, f.x0 + f.h * (bx + r) - px);
      if (by - r + 1 > 0) bound = fmin(bound, py - (f.y0 + f.h * (by - r + 1)));
      if (by + r < g) bound = fmin(bound, f.y0 + f.h * (by + r) - py);
      if (kth <= bound - e) break;
    }
    const int xlo = bx - r > 0 ? bx - r : 0, xhi = bx + r < g - 1 ? bx + r : g - 1;
    if (by - r >= 0) scan_range(spts, bin_start[(by - r) * g + xlo], bin_start[(by - r) * g + xhi + 1], px, py, best);
    if (r > 0 && by + r <= g - 1) scan_range(spts, bin_start[(by + r) * g + xlo], bin_start[(by + r) * g + xhi + 1], px, py, best);
    const int ylo = by - r + 1 > 0 ? by - r + 1 : 0, yhi = by + r - 1 < g - 1 ? by + r - 1 : g - 1;
    for (int y = ylo; y <= yhi; ++y) {
      if (bx - r >= 0) scan_range(spts, bin_start[y * g + bx - r], bin_start[y * g + bx - r + 1], px, py, best);
      if (r > 0 && bx + r <= g - 1) scan_range(spts, bin_start[y * g + bx + r], bin_start[y * g + bx + r + 1], px, py, best);
    }
  }
  double* row = out + (long long)sidx[t] * k;
#pragma unroll
  for (int j = 0; j < KNN; ++j)
    if (j < k) row[j] = best[j];
}

int check_knn(const void* pts, int dtype, int64_t n, int k, const void* out) {
  if (dtype != ZK_F64 && dtype != ZK_I32) return zk_fail(ZK_E_BADARG, "knn_distances: points are ZK_F64 or ZK_I32");
  if (k < 1 || k > KNN) return zk_fail(ZK_E_BADARG, "knn_distances: needs 1 <= k <= 12");
  if (n < k) return zk_fail(ZK_E_BADARG, "knn_distances: needs k <= n_points (every point has k neighbours, itself included)");
  if (n >= ((int64_t)1 << 26)) return zk_fail(ZK_E_BADARG, "knn_distances: needs n_points < 2^26");
  if (!pts || !out) return zk_fail(ZK_E_BADARG, "knn_distances: null pointer");
  return 0;
}

int knn_call(const void* points, int dtype, int64_t n, int k, double* out, hipStream_t s) {
  int rc;
  const int g = grid_side(n);
  temp_store tmp;
  point_grid grid;
  dev_buf d_pts, d_frame;
  dev_flag flag;
  if ((rc = d_pts.alloc(sizeof(double2) * (size_t)n)) || (rc = flag.arm(s)) || (rc = d_frame.alloc(sizeof(zk_grid_frame)))) return rc;
  hipLaunchKernelGGL(load_points_kernel, dim3(blocks_of(n)), dim3(256), 0, s, points, dtype, (long long)n, d_pts.as<double2>(), flag.word());
  hipLaunchKernelGGL(knn_frame_kernel, dim3(1), dim3(1024), 0, s, d_pts.as<double2>(), (long long)n, g, d_frame.as<zk_grid_frame>());
  if ((rc = build_point_grid(&grid, tmp, d_pts.as<double2>(), n, g, d_frame.as<zk_grid_frame>(), s))) return rc;
  hipLaunchKernelGGL(knn_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, grid.spts, grid.sidx, grid.bin_start, (long long)n,
                     d_frame.as<zk_grid_frame>(), k, flag.word(), out);
  ZK_HIP(hipGetLastError());
  int flags;
  if ((rc = flag.read(s, &flags))) return rc;        // the working buffers go with this call
  if (flags & ERR_NONFINITE) return zk_fail(ZK_E_BADARG, "knn_distances: a point is not finite");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// B. reductions over the distance matrix
// ---------------------------------------------------------------------------------------------------------------------

// what one reduction carries per lane: NV values, joined by add / min / max
enum { JOIN_ADD = 0, JOIN_MIN = 1, JOIN_MAX = 2 };

__device__ inline double join(double a, double b, int how) { return how == JOIN_ADD ? a + b : (how == JOIN_MIN ? fmin(a, b) : fmax(a, b)); }

// The lanes' values v[0 .. NV) through a fixed tree: shuffles within a wave, the four waves in order; lane 0 of the workgroup
// writes part[block][NV].  how(j) says how value j is joined.
template <int NV, class How>
__device__ inline void block_reduce(double (&v)[NV], double* __restrict__ part, How how) {
  __shared__ double w[4][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double a = v[j];
    for (int d = 32; d > 0; d >>= 1) a = join(a, __shfl_down(a, d, 64), how(j));
    if (lane == 0) w[wave][j] = a;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int j = threadIdx.x;
    double a = w[0][j];
    for (int q = 1; q < 4; ++q) a = join(a, w[q][j], how(j));
    part[(long long)blockIdx.x * NV + j] = a;
  }
}

// out[j] = part[0][j] (+) part[1][j] (+) ... in order
template <class How>
__global__ __launch_bounds__(64) void final_reduce_kernel(const double* __restrict__ part, int blocks, int nv, double* __restrict__ out, How how) {
  const int j = threadIdx.x;
  if (j >= nv) return;
  double a = part[j];
  for (int b = 1; b < blocks; ++b) a = join(a, part[(long long)b * nv + j], how(j));
  out[j] = a;
}

struct how_ranges {
  __device__ int operator()(int j) const { return j == 0 ? JOIN_MIN : JOIN_MAX; }
};
struct how_add {
  __device__ int operator()(int) const { return JOIN_ADD; }
};

// v[0] = min of column 1, v[j] = max of column j, j = 1 .. 11
__global__ __launch_bounds__(256) void ranges_kernel(const double* __restrict__ dd, long long n, double* __restrict__ part) {
  double v[KNN];
  v[0] = INFINITY;
#pragma unroll
  for (int j = 1; j < KNN; ++j) v[j] = -INFINITY;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    v[0] = fmin(v[0], dd[i * KNN + 1]);
#pragma unroll
    for (int j = 1; j < KNN; ++j) v[j] = fmax(v[j], dd[i * KNN + j]);
  }
  block_reduce<KNN>(v, part, how_ranges());
}

// params: shift, t[11].  v[3 c] = count of w > t_c, v[3 c + 1] = their sum, v[3 c + 2] = the sum of the rest, c = k - 2
__global__ __launch_bounds__(256) void sides_kernel(const double* __restrict__ dd, long long n, const double* __restrict__ params,
                                                    double* __restrict__ part) {
  double v[3 * NK];
#pragma unroll
  for (int j = 0; j < 3 * NK; ++j) v[j] = 0;
  const double shift = params[0];
  double t[NK];
#pragma unroll
  for (int c = 0; c < NK; ++c) t[c] = params[1 + c];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
#pragma unroll
    for (int j = 1; j < KNN; ++j) {
      const double w = dd[i * KNN + j] - shift;
#pragma unroll
      for (int c = j - 1; c < NK; ++c) {             // column j belongs to d_k for k = c + 2 > j
        const bool above = w > t[c];
        v[3 * c] += above ? 1.0 : 0.0;
        v[3 * c + 1] += above ? w : 0.0;
        v[3 * c + 2] += above ? 0.0 : w;
      }
    }
  }
  block_reduce<3 * NK>(v, part, how_add());
}

// params: first, last[11], edges[11][257]
__global__ __launch_bounds__(256) void hist_kernel(const double* __restrict__ dd, long long n, const double* __restrict__ params,
                                                   u64* __restrict__ counts) {
  __shared__ int h[NK * BINS];
  for (int q = threadIdx.x; q < NK * BINS; q += 256) h[q] = 0;
  __syncthreads();
  const double first = params[0];
  const double* edges = params + 1 + NK;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    for (int j = 1; j < KNN; ++j) {
      const double v = dd[i * KNN + j];
      for (int c = j - 1; c < NK; ++c) atomicAdd(&h[c * BINS + np_bin(v, first, params[1 + c], edges + c * (BINS + 1))], 1);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < NK * BINS; q += 256)
    if (h[q]) atomicAdd(counts + q, (u64)h[q]);
}

// keys[i * cols + (j - 1)] = bits of dd[i][j] - shift, j = 1 .. cols
__global__ __launch_bounds__(256) void gap_keys_kernel(const double* __restrict__ dd, long long n, int cols, double shift, u64* __restrict__ keys) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * cols) return;
  const long long i = t / cols;
  const int j = (int)(t - i * cols) + 1;
  const double w = dd[i * KNN + j] - shift;
  keys[t] = (u64)__double_as_longlong(w > 0 ? w : 0.0);    // w >= 0 by contract; -0.0 and a contract broken go to +0.0
}

__global__ __launch_bounds__(256) void gap_min_kernel(const u64* __restrict__ sorted, long long m, u64* __restrict__ best) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t + 1 >= m) return;
  const double gap = __longlong_as_double((long long)sorted[t + 1]) - __longlong_as_double((long long)sorted[t]);
  if (gap > 0) atomicMin(best, (u64)__double_as_longlong(gap));
}

int params_len(int op) {
  return op == ZK_KNN_RANGES ? 0 : (op == ZK_KNN_HIST ? 1 + NK + NK * (BINS + 1) : (op == ZK_KNN_SIDES ? 1 + NK : 1));
}

int check_stats(const void* dd, int64_t n, int op, const double* params, const int64_t* counts, const double* sums) {
  if (op != ZK_KNN_RANGES && op != ZK_KNN_HIST && op != ZK_KNN_SIDES && op != ZK_KNN_GAPS) return zk_fail(ZK_E_BADARG, "knn_stats: unknown op");
  if (n < 1 || n >= ((int64_t)1 << 26) || !dd) return zk_fail(ZK_E_BADARG, "knn_stats: needs a distance matrix of 1 <= n_points < 2^26 rows");
  if (params_len(op) && !params) return zk_fail(ZK_E_BADARG, "knn_stats: this op needs params_host");
  if ((op == ZK_KNN_HIST || op == ZK_KNN_SIDES) && !counts) return zk_fail(ZK_E_BADARG, "knn_stats: this op needs counts_host");
  if (op != ZK_KNN_HIST && !sums) return zk_fail(ZK_E_BADARG, "knn_stats: this op needs sums_host");
  if (op == ZK_KNN_HIST)
    for (int c = 0; c < NK; ++c)
      if (!(params[1 + c] > params[0])) return zk_fail(ZK_E_BADARG, "knn_stats: a histogram needs last > first");
  return 0;
}

int stats_call(const double* dd, int64_t n, int op, const double* params, int64_t* counts, double* sums, hipStream_t s) {
  int rc;
  dev_buf d_params, d_part, d_out;
  const int np = params_len(op);
  if (np) {
    if ((rc = d_params.alloc(sizeof(double) * np))) return rc;
    ZK_HIP(hipMemcpyAsync(d_params.p, params, sizeof(double) * np, hipMemcpyHostToDevice, s));
  }
  const long long want = (n + 255) / 256;
  const int blocks = (int)(want < RED_BLOCKS ? want : RED_BLOCKS);
  if (op == ZK_KNN_RANGES || op == ZK_KNN_SIDES) {
    const int nv = op == ZK_KNN_RANGES ? KNN : 3 * NK;
    double host[3 * NK];
    if ((rc = d_part.alloc(sizeof(double) * nv * blocks)) || (rc = d_out.alloc(sizeof(double) * nv))) return rc;
    if (op == ZK_KNN_RANGES) {
      hipLaunchKernelGGL(ranges_kernel, dim3(blocks), dim3(256), 0, s, dd, (long long)n, d_part.as<double>());
      hipLaunchKernelGGL(final_reduce_kernel<how_ranges>, dim3(1), dim3(64), 0, s, d_part.as<double>(), blocks, nv, d_out.as<double>(), how_ranges());
    } else {
      hipLaunchKernelGGL(sides_kernel, dim3(blocks), dim3(256), 0, s, dd, (long long)n, d_params.as<double>(), d_part.as<double>());
      hipLaunchKernelGGL(final_reduce_kernel<how_add>, dim3(1), dim3(64), 0, s, d_part.as<double>(), blocks, nv, d_out.as<double>(), how_add());
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(host, d_out.p, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    if (op == ZK_KNN_RANGES) {
      for (int j = 0; j < KNN; ++j) sums[j] = host[j];
    } else {
      for (int c = 0; c < NK; ++c) {
        counts[c] = (int64_t)host[3 * c];            // an integer below 2^53: exact
        sums[2 * c] = host[3 * c + 1];
        sums[2 * c + 1] = host[3 * c + 2];
      }
    }
    return 0;
  }
  if (op == ZK_KNN_HIST) {
    if ((rc = d_out.alloc(sizeof(u64) * NK * BINS))) return rc;
    ZK_HIP(hipMemsetAsync(d_out.p, 0, sizeof(u64) * NK * BINS, s));
    hipLaunchKernelGGL(hist_kernel, dim3(blocks), dim3(256), 0, s, dd, (long long)n, d_params.as<double>(), d_out.as<u64>());
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(counts, d_out.p, sizeof(u64) * NK * BINS, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    return 0;
  }
  // ZK_KNN_GAPS: one sort per sample
  dev_buf d_keys;
  temp_store tmp;
  const size_t most = (size_t)n * NK;
  if ((rc = d_keys.alloc(sizeof(u64) * 2 * most)) || (rc = d_out.alloc(sizeof(u64) * NK))) return rc;
  ZK_HIP(hipMemsetAsync(d_out.p, 0xff, sizeof(u64) * NK, s));
  u64 *k_in = d_keys.as<u64>(), *k_out = k_in + most;
  const auto sort = [&](size_t m) { return [=](void* p, size_t& b) { return rocprim::radix_sort_keys(p, b, k_in, k_out, m, 0, 64, s); }; };
  size_t bytes = 0;                                  // one allocation, sized by the largest sample, serves the eleven sorts
  if ((rc = zk_prim_bytes(&bytes, sort(most))) || (rc = tmp.ensure(bytes))) return rc;
  for (int c = 0; c < NK; ++c) {
    const long long m = (long long)n * (c + 1);
    hipLaunchKernelGGL(gap_keys_kernel, dim3(blocks_of(m)), dim3(256), 0, s, dd, (long long)n, c + 1, params[0], k_in);
    if ((rc = zk_prim(tmp, sort((size_t)m)))) return rc;
    hipLaunchKernelGGL(gap_min_kernel, dim3(blocks_of(m)), dim3(256), 0, s, k_out, m, d_out.as<u64>() + c);
    ZK_HIP(hipGetLastError());
  }
  u64 host[NK];
  ZK_HIP(hipMemcpyAsync(host, d_out.p, sizeof(u64) * NK, hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < NK; ++c) {
    double gap = INFINITY;                           // all ones (never lowered): no two distinct values
    if (host[c] != ~(u64)0) memcpy(&gap, &host[c], sizeof(double));
    sums[c] = gap;
  }
  return 0;
}

}  // namespace


extern "C" int zk_knn_distances_dev(int device, const void* points_dev, int points_dtype, int64_t n_points, int k, double* out_dev,
                                    void* hip_stream) {
  int rc = check_knn(points_dev, points_dtype, n_points, k, out_dev);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return knn_call(points_dev, points_dtype, n_points, k, out_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_knn_distances(int device, const void* points_host, int points_dtype, int64_t n_points, int k, double* out_host) {
  int rc = check_knn(points_host, points_dtype, n_points, k, out_host);
  if (rc) return rc;
  if (points_dtype == ZK_F64)                        // the values are checked before anything is launched
    for (int64_t q = 0; q < 2 * n_points; ++q)
      if (!(fabs(((const double*)points_host)[q]) <= DBL_BIG)) return zk_fail(ZK_E_BADARG, "knn_distances: a point is not finite");
  ZK_ON_DEVICE(device);
  const size_t pts_bytes = (points_dtype == ZK_I32 ? sizeof(int32_t) : sizeof(double)) * 2 * (size_t)n_points,
               out_bytes = sizeof(double) * (size_t)k * (size_t)n_points;
  dev_buf d_pts, d_out;
  if ((rc = d_pts.upload(points_host, pts_bytes)) || (rc = d_out.alloc(out_bytes)) ||
      (rc = knn_call(d_pts.p, points_dtype, n_points, k, d_out.as<double>(), (hipStream_t)0)))
    return rc;
  return d_out.download(out_host, out_bytes);
}

extern "C" int zk_knn_stats_dev(int device, const double* dd_dev, int64_t n_points, int op, const double* params_host, int64_t* counts_host,
                                double* sums_host, void* hip_stream) {
  int rc = check_stats(dd_dev, n_points, op, params_host, counts_host, sums_host);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return stats_call(dd_dev, n_points, op, params_host, counts_host, sums_host, (hipStream_t)hip_stream);
}

extern "C" int zk_knn_stats(int device, const double* dd_host, int64_t n_points, int op, const double* params_host, int64_t* counts_host,
                            double* sums_host) {
  int rc = check_stats(dd_host, n_points, op, params_host, counts_host, sums_host);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  dev_buf d_dd;
  if ((rc = d_dd.upload(dd_host, sizeof(double) * KNN * (size_t)n_points))) return rc;
  return stats_call(d_dd.as<double>(), n_points, op, params_host, counts_host, sums_host, (hipStream_t)0);
}

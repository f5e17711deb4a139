// zk_datasets.hip -- device side of mtflearn.datasets: the rasteriser of the reference's datasets/_tapered_gaussian.py
// (add_tapered_gaussian, what HoneyCombLattice.to_image draws with) and the uncut Gaussians of get_zps_test_patches /
// generate_data_gn.  The frame is added to in place.
//
// The reference adds point 0, then point 1, ... to the frame, and a float32 frame rounds at every add.  The order is part
// of the result, so this is a gather: every pixel adds its own contributions in ascending point index, in float64, a
// float32 frame rounded after every add.  No floating-point atomics anywhere: two runs agree bit for bit.
//
//   with a cutoff   the frame is cut into TILE x TILE pixel tiles.  count: one lane per point adds 1 (integer atomic) to
//                   every tile its clipped pixel box overlaps.  scan: exclusive int64 offsets.  fill: the same lanes with
//                   the same predicate write their point index into the tile's list, at a slot handed out by an integer
//                   atomic (so the order inside a list is arbitrary).  gather: one workgroup per tile sorts its list
//                   ascending (a bitonic network in LDS up to SORT_CAP entries, in place in global memory beyond), then
//                   takes it in ascending windows of WINDOW points staged in LDS (centre, amplitude, clipped box), each
//                   lane walking the window for its own pixel.
//                   The host knows the points, so it sizes the lists before anything is launched (the same box predicate,
//                   compiled from the same function): when all lists together would pass the budget the points are cut
//                   into ascending index ranges rendered one after the other, which keeps the order by construction.
//   without         every point reaches every pixel of its frame: no lists, the workgroup of a tile walks the frame's own
//                   point range in windows.  Frames are batched (gridDim.z).
#pragma clang fp contract(off)

#include <float.h>
#include <math.h>

#include <algorithm>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int TILE = 16;                  // pixels per tile side; TILE * TILE lanes per workgroup
constexpr int THREADS = TILE * TILE;
constexpr int WINDOW = THREADS;           // points staged per pass over a list: one per lane
constexpr int SORT_CAP = 1024;            // list entries sorted in LDS; longer lists are sorted in place in global memory
constexpr int64_t DEFAULT_BUDGET = (int64_t)1 << 24;   // list entries (int32) per point range: 64 MiB

enum { MODE_UNCUT = 0, MODE_CUT = 1, MODE_TAPER = 2 };

struct point {
  double x, y, a;
};

// The pixels a point may touch: [floor(x - R), ceil(x + R)] x [floor(y - R), ceil(y + R)] cut to the frame, as inclusive
// int bounds; false when nothing is left (or a coordinate is not finite).  Host and device evaluate the same expressions
// (one rounding per operation, this file is compiled without contraction), so the host's list sizes are the device's.
__host__ __device__ inline bool clipped_box(double x, double y, double R, int H, int W, int& x0, int& x1, int& y0, int& y1) {
  if (!(fabs(x) <= DBL_MAX) || !(fabs(y) <= DBL_MAX)) return false;
  const double fx0 = fmax(floor(x - R), 0.0), fx1 = fmin(ceil(x + R), (double)(W - 1));
  const double fy0 = fmax(floor(y - R), 0.0), fy1 = fmin(ceil(y + R), (double)(H - 1));
  if (!(fx0 <= fx1) || !(fy0 <= fy1)) return false;
  x0 = (int)fx0;
  x1 = (int)fx1;
  y0 = (int)fy0;
  y1 = (int)fy1;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// binning
// ---------------------------------------------------------------------------------------------------------------------

// FILL = false: counts[tile] += 1 for every tile the box of point p0 + i overlaps.  FILL = true: the same walk, writing the
// point index to list[offsets[tile] + slot], the slot from the tile's cursor.
template <bool FILL>
__global__ __launch_bounds__(256) void bin_kernel(const point* __restrict__ pts, long long p0, long long n, double R, int H, int W,
                                                  int tiles_x, unsigned* __restrict__ counts, const long long* __restrict__ offsets,
                                                  int* __restrict__ list, long long capacity) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const point p = pts[p0 + i];
  int x0, x1, y0, y1;
  if (!clipped_box(p.x, p.y, R, H, W, x0, x1, y0, y1)) return;
  for (int ty = y0 / TILE; ty <= y1 / TILE; ++ty)
    for (int tx = x0 / TILE; tx <= x1 / TILE; ++tx) {
      const long long tile = (long long)ty * tiles_x + tx;
      const unsigned slot = atomicAdd(&counts[tile], 1u);
      if (FILL) {
        const long long at = offsets[tile] + slot;
        if (at < capacity) list[at] = (int)(p0 + i);
      }
    }
}

// offsets[0 .. n] = exclusive sums of counts[0 .. n) in int64; one workgroup of 1024 lanes, each with a contiguous share.
__global__ __launch_bounds__(1024) void scan_kernel(const unsigned* __restrict__ counts, long long n, long long* __restrict__ offsets) {
  __shared__ long long part[1024];
  const int t = threadIdx.x;
  const long long share = (n + 1023) / 1024, lo = std::min<long long>(n, t * share), hi = std::min<long long>(n, lo + share);
  long long sum = 0;
  for (long long i = lo; i < hi; ++i) sum += counts[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const long long add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long run = part[t] - sum;
  for (long long i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (t == 1023) offsets[n] = part[1023];
}

// ---------------------------------------------------------------------------------------------------------------------
// the gather
// ---------------------------------------------------------------------------------------------------------------------

// Ascending sort of v[0 .. n) by the whole workgroup: the bitonic network in its all-ascending form (every merge opens with
// a mirror step), laid over the next power of two with the missing tail read as +infinity.  An exchange whose upper end is
// past n would leave both ends where they are, so it is skipped: no padding is stored.  v is LDS or global memory.
__device__ void sort_ascending(int* v, long long n) {
  long long P = 1;
  while (P < n) P <<= 1;
  const long long half = P >> 1;
  for (long long k = 2; k <= P; k <<= 1) {
    const long long h = k >> 1;
    for (long long p = threadIdx.x; p < half; p += THREADS) {
      const long long base = (p / h) * k, q = p % h, a = base + q, b = base + k - 1 - q;
      if (b < n) {
        const int va = v[a], vb = v[b];
        if (va > vb) {
          v[a] = vb;
          v[b] = va;
        }
      }
    }
    __syncthreads();
    for (long long j = k >> 2; j >= 1; j >>= 1) {
      for (long long p = threadIdx.x; p < half; p += THREADS) {
        const long long a = (p / j) * 2 * j + p % j, b = a + j;
        if (b < n) {
          const int va = v[a], vb = v[b];
          if (va > vb) {
            v[a] = vb;
            v[b] = va;
          }
        }
      }
      __syncthreads();
    }
  }
}

struct staged {
  double x[WINDOW], y[WINDOW], a[WINDOW];
  int x0[WINDOW], x1[WINDOW], y0[WINDOW], y1[WINDOW];
};

// one more contribution to the accumulator, in the reference's own operations and order
template <typename T, int MODE>
__device__ __forceinline__ void add_point(T& acc, double px, double py, double x, double y, double a, double R, double sigma2) {
  const double dx = px - x, dy = py - y;
  const double d2 = dx * dx + dy * dy;
  double w;
  if (MODE == MODE_UNCUT) {
    w = a * exp(-d2 / sigma2);                      // sigma2 holds 2 sigma^2 here
  } else {
    const double r = sqrt(d2);
    if (!(r <= R)) return;
    w = a * exp(-0.5 * (r * r) / sigma2);
    if (MODE == MODE_TAPER) {
      const double t = r / R;
      w = w * (1.0 - 3.0 * (t * t) + 2.0 * (t * t * t));
    }
  }
  acc = (T)((double)acc + w);
}

template <typename T, int MODE>
__global__ __launch_bounds__(THREADS) void gather_kernel(T* frame, int H, int W, int tiles_x, const point* __restrict__ pts,
                                                         const long long* __restrict__ offsets, int* list, long long capacity,
                                                         double R, double sigma2) {
  __shared__ int s_idx[SORT_CAP];
  __shared__ staged s;
  const long long tile = blockIdx.x;
  const long long beg = offsets[tile], L = std::min(offsets[tile + 1], capacity) - beg;
  if (L <= 0) return;                               // the same for the whole workgroup
  const int tid = threadIdx.x;
  int* lst = list + beg;
  const bool in_lds = L <= SORT_CAP;
  if (in_lds) {
    for (int i = tid; i < (int)L; i += THREADS) s_idx[i] = lst[i];
    __syncthreads();
    sort_ascending(s_idx, L);
  } else {
    sort_ascending(lst, L);
  }
  __syncthreads();
  const int X = (int)(tile % tiles_x) * TILE + tid % TILE, Y = (int)(tile / tiles_x) * TILE + tid / TILE;
  const bool mine = X < W && Y < H;
  const double px = (double)X, py = (double)Y;
  T acc = 0;
  if (mine) acc = frame[(long long)Y * W + X];
  for (long long w0 = 0; w0 < L; w0 += WINDOW) {
    const int n = (int)std::min<long long>(WINDOW, L - w0);
    if (tid < n) {
      const point p = pts[in_lds ? s_idx[w0 + tid] : lst[w0 + tid]];
      s.x[tid] = p.x;
      s.y[tid] = p.y;
      s.a[tid] = p.a;
      int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
      (void)clipped_box(p.x, p.y, R, H, W, x0, x1, y0, y1);
      s.x0[tid] = x0;
      s.x1[tid] = x1;
      s.y0[tid] = y0;
      s.y1[tid] = y1;
    }
    __syncthreads();
    if (mine)
      for (int j = 0; j < n; ++j)
        if (X >= s.x0[j] && X <= s.x1[j] && Y >= s.y0[j] && Y <= s.y1[j]) add_point<T, MODE>(acc, px, py, s.x[j], s.y[j], s.a[j], R, sigma2);
    __syncthreads();
  }
  if (mine) frame[(long long)Y * W + X] = acc;
}

// no cutoff: frame b (blockIdx.z) takes its own points [offsets[b], offsets[b + 1]) in order, everywhere
template <typename T>
__global__ __launch_bounds__(THREADS) void uncut_kernel(T* frames, int H, int W, const point* __restrict__ pts,
                                                        const long long* __restrict__ offsets, double two_sigma2) {
  __shared__ double s_x[WINDOW], s_y[WINDOW], s_a[WINDOW];
  const int tid = threadIdx.x, b = blockIdx.z;
  const long long beg = offsets[b], L = offsets[b + 1] - beg;
  const int X = blockIdx.x * TILE + tid % TILE, Y = blockIdx.y * TILE + tid / TILE;
  const bool mine = X < W && Y < H;
  const double px = (double)X, py = (double)Y;
  T* frame = frames + (long long)b * H * W;
  T acc = 0;
  if (mine) acc = frame[(long long)Y * W + X];
  for (long long w0 = 0; w0 < L; w0 += WINDOW) {
    const int n = (int)std::min<long long>(WINDOW, L - w0);
    if (tid < n) {
      const point p = pts[beg + w0 + tid];
      s_x[tid] = p.x;
      s_y[tid] = p.y;
      s_a[tid] = p.a;
    }
    __syncthreads();
    if (mine)
      for (int j = 0; j < n; ++j) add_point<T, MODE_UNCUT>(acc, px, py, s_x[j], s_y[j], s_a[j], 0.0, two_sigma2);
    __syncthreads();
  }
  if (mine && L > 0) frame[(long long)Y * W + X] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------

template <typename T>
void launch_gather(int mode, T* frame, int H, int W, int tiles_x, long long tiles, const point* pts, const long long* offsets,
                   int* list, long long capacity, double R, double sigma2, hipStream_t s) {
  if (mode == MODE_TAPER)
    hipLaunchKernelGGL((gather_kernel<T, MODE_TAPER>), dim3((unsigned)tiles), dim3(THREADS), 0, s, frame, H, W, tiles_x, pts, offsets,
                       list, capacity, R, sigma2);
  else
    hipLaunchKernelGGL((gather_kernel<T, MODE_CUT>), dim3((unsigned)tiles), dim3(THREADS), 0, s, frame, H, W, tiles_x, pts, offsets,
                       list, capacity, R, sigma2);
}

int render_run(void* frame, int dtype, int64_t H, int64_t W, int64_t batch, const double* points, const double* amplitudes,
               const int64_t* point_offsets, int64_t n, double sigma, double r_factor, int taper, int64_t budget, hipStream_t s) {
  if (n == 0) return 0;
  std::vector<point> host(n);
  for (int64_t i = 0; i < n; ++i) host[i] = {points[2 * i], points[2 * i + 1], amplitudes[i]};
  dev_buf d_pts;
  int rc;
  if ((rc = d_pts.alloc(sizeof(point) * (size_t)n))) return rc;
  ZK_HIP(hipMemcpyAsync(d_pts.p, host.data(), sizeof(point) * (size_t)n, hipMemcpyHostToDevice, s));
  const int tiles_x = (int)((W + TILE - 1) / TILE), tiles_y = (int)((H + TILE - 1) / TILE);

  if (r_factor <= 0) {                              // no cutoff (checked: taper is off)
    std::vector<long long> off(batch + 1);
    for (int64_t b = 0; b <= batch; ++b) off[b] = point_offsets ? point_offsets[b] : (b ? n : 0);
    dev_buf d_off;
    if ((rc = d_off.alloc(sizeof(long long) * off.size()))) return rc;
    ZK_HIP(hipMemcpyAsync(d_off.p, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, s));
    const double two_sigma2 = 2 * (sigma * sigma);
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)batch);
    if (dtype == ZK_F32)
      hipLaunchKernelGGL((uncut_kernel<float>), grid, dim3(THREADS), 0, s, (float*)frame, (int)H, (int)W, d_pts.as<point>(),
                         d_off.as<long long>(), two_sigma2);
    else
      hipLaunchKernelGGL((uncut_kernel<double>), grid, dim3(THREADS), 0, s, (double*)frame, (int)H, (int)W, d_pts.as<point>(),
                         d_off.as<long long>(), two_sigma2);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(s));                // the staging buffers go with this call
    return 0;
  }

  const double R = r_factor * sigma, sigma2 = sigma * sigma;
  const int mode = taper ? MODE_TAPER : MODE_CUT;
  const long long tiles = (long long)tiles_x * tiles_y;
  if (budget <= 0) budget = DEFAULT_BUDGET;
  // list entries per point, then ascending ranges [p0, p1) of at most `budget` entries (a single point may pass it)
  std::vector<int64_t> cuts{0};
  int64_t in_range = 0, largest = 0;
  for (int64_t i = 0; i < n; ++i) {
    int x0, x1, y0, y1;
    int64_t c = 0;
    if (clipped_box(host[i].x, host[i].y, R, (int)H, (int)W, x0, x1, y0, y1))
      c = (int64_t)(x1 / TILE - x0 / TILE + 1) * (y1 / TILE - y0 / TILE + 1);
    if (in_range + c > budget && i > cuts.back()) {
      largest = std::max(largest, in_range);
      cuts.push_back(i);
      in_range = 0;
    }
    in_range += c;
  }
  largest = std::max(largest, in_range);
  cuts.push_back(n);
  if (largest == 0) return 0;                       // nothing reaches the frame

  dev_buf d_counts, d_offsets, d_list;
  if ((rc = d_counts.alloc(sizeof(unsigned) * (size_t)tiles)) || (rc = d_offsets.alloc(sizeof(long long) * (size_t)(tiles + 1))) ||
      (rc = d_list.alloc(sizeof(int) * (size_t)largest)))
    return rc;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    const long long p0 = cuts[c], np = cuts[c + 1] - p0;
    const unsigned blocks = (unsigned)((np + 255) / 256);
    ZK_HIP(hipMemsetAsync(d_counts.p, 0, sizeof(unsigned) * (size_t)tiles, s));
    hipLaunchKernelGGL((bin_kernel<false>), dim3(blocks), dim3(256), 0, s, d_pts.as<point>(), p0, np, R, (int)H, (int)W, tiles_x,
                       d_counts.as<unsigned>(), (const long long*)nullptr, (int*)nullptr, 0LL);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, d_counts.as<unsigned>(), tiles, d_offsets.as<long long>());
    ZK_HIP(hipMemsetAsync(d_counts.p, 0, sizeof(unsigned) * (size_t)tiles, s));
    hipLaunchKernelGGL((bin_kernel<true>), dim3(blocks), dim3(256), 0, s, d_pts.as<point>(), p0, np, R, (int)H, (int)W, tiles_x,
                       d_counts.as<unsigned>(), d_offsets.as<long long>(), d_list.as<int>(), (long long)largest);
    if (dtype == ZK_F32)
      launch_gather<float>(mode, (float*)frame, (int)H, (int)W, tiles_x, tiles, d_pts.as<point>(), d_offsets.as<long long>(),
                           d_list.as<int>(), (long long)largest, R, sigma2, s);
    else
      launch_gather<double>(mode, (double*)frame, (int)H, (int)W, tiles_x, tiles, d_pts.as<point>(), d_offsets.as<long long>(),
                            d_list.as<int>(), (long long)largest, R, sigma2, s);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(s));                  // the lists go with this call
  return 0;
}

int check_render(const void* frame, int dtype, int64_t H, int64_t W, int64_t batch, const double* points, const double* amplitudes,
                 const int64_t* point_offsets, int64_t n, double sigma, double r_factor, int taper) {
  if (dtype != ZK_F32 && dtype != ZK_F64) return zk_fail(ZK_E_BADARG, "dtype must be ZK_F32 or ZK_F64");
  if (H < 1 || W < 1 || H >= ((int64_t)1 << 31) - TILE || W >= ((int64_t)1 << 31) - TILE)
    return zk_fail(ZK_E_BADARG, "bad frame shape (needs 1 <= height, width < 2^31 - 16)");
  if ((W + TILE - 1) / TILE * ((H + TILE - 1) / TILE) >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "the frame has 2^31 tiles or more");
  if (n < 0 || n >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "bad point count (needs 0 <= n < 2^31)");
  if (!frame || (n && (!points || !amplitudes))) return zk_fail(ZK_E_BADARG, "null pointer");
  if (!(sigma > 0) || !(sigma <= DBL_MAX)) return zk_fail(ZK_E_BADARG, "sigma must be positive and finite");
  if (!(fabs(r_factor) <= DBL_MAX)) return zk_fail(ZK_E_BADARG, "r_factor must be finite");
  if (taper && !(r_factor > 0)) return zk_fail(ZK_E_BADARG, "the taper needs a cutoff: r_factor > 0");
  if (r_factor > 0) {
    if (batch != 1) return zk_fail(ZK_E_BADARG, "batch > 1 only without a cutoff (taper = 0, r_factor <= 0)");
  } else {
    if (batch < 1 || batch > 65535) return zk_fail(ZK_E_BADARG, "needs 1 <= batch <= 65535");
    if (batch > 1 && !point_offsets) return zk_fail(ZK_E_BADARG, "batch > 1 needs point_offsets");
    if ((H + TILE - 1) / TILE > 65535) return zk_fail(ZK_E_BADARG, "without a cutoff the frame height is at most 65535 tiles of 16 rows");
  }
  if (point_offsets) {
    if (point_offsets[0] != 0 || point_offsets[batch] != n) return zk_fail(ZK_E_BADARG, "point_offsets must run from 0 to n_points");
    for (int64_t b = 0; b < batch; ++b)
      if (point_offsets[b] > point_offsets[b + 1]) return zk_fail(ZK_E_BADARG, "point_offsets must not decrease");
  }
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_render_gaussians_dev(int device, void* frame_dev, int dtype, int64_t height, int64_t width, int64_t batch,
                                       const double* points_host, const double* amplitudes_host, const int64_t* point_offsets_host,
                                       int64_t n_points, double sigma, double r_factor, int taper, int64_t list_budget,
                                       void* hip_stream) {
  int rc = check_render(frame_dev, dtype, height, width, batch, points_host, amplitudes_host, point_offsets_host, n_points, sigma,
                        r_factor, taper);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return render_run(frame_dev, dtype, height, width, batch, points_host, amplitudes_host, point_offsets_host, n_points, sigma,
                    r_factor, taper, list_budget, (hipStream_t)hip_stream);
}

extern "C" int zk_render_gaussians(int device, void* frame_host, int dtype, int64_t height, int64_t width, int64_t batch,
                                   const double* points_host, const double* amplitudes_host, const int64_t* point_offsets_host,
                                   int64_t n_points, double sigma, double r_factor, int taper, int64_t list_budget) {
  int rc = check_render(frame_host, dtype, height, width, batch, points_host, amplitudes_host, point_offsets_host, n_points, sigma,
                        r_factor, taper);
  if (rc) return rc;
  if (n_points == 0) return 0;
  ZK_ON_DEVICE(device);
  const size_t bytes = (size_t)batch * height * width * (dtype == ZK_F64 ? 8 : 4);
  dev_buf d_frame;
  if ((rc = d_frame.upload(frame_host, bytes))) return rc;
  if ((rc = render_run(d_frame.p, dtype, height, width, batch, points_host, amplitudes_host, point_offsets_host, n_points, sigma,
                       r_factor, taper, list_budget, (hipStream_t)0)))
    return rc;
  return d_frame.download(frame_host, bytes);
}

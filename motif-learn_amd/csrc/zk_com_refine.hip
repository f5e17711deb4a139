// zk_com_refine.hip -- the reference's thresholded centroid refinement (features/_keypoint.py, com_refine) on the device: a
// size x size window is cut at every key point, thresholded with Li's rule or with Otsu's, what lies below the threshold
// counts as zero, and the point moves to the centroid of what is left.  A file of its own beside zk_refine.hip, built with the same
// -ffp-contract=off: every product and sum below is rounded once.  The window's corner is zk_point_window.h's, the histogram's
// bin rule zk_np_bins.h's.
//
// One launch, one workgroup per window, no global scratch and no floating-point atomics.  A window of at most 256 pixels
// (size <= 16) is worked on by ONE WAVE (a workgroup of 64 lanes: four pixels a lane at most), a larger one by a workgroup of
// FOUR WAVES (256 lanes: 16 pixels a lane at 64 x 64); the choice depends on size alone, so the same window takes the same
// reduction tree in every call.  The window is read from the frame once, widened to float64 into LDS, and everything else
// works from LDS:
//   range        min and max (order-free).  Equal: the threshold is that value, no iteration.
//   Otsu         np.histogram(w, 256) and skimage's rule on it, as tests/thresholds_reference.py states it: the 257 edges of
//                np.linspace (edge k = k * step + min, product and sum rounded separately, the last edge set to max), integer
//                LDS counters under NumPy's bin rule, then the two np.cumsum of counts * centres -- SEQUENTIAL in bin order:
//                lane 0 walks the bins upwards and lane 1 downwards in the same loop -- and the class variance of every split
//                in parallel; the first maximum is found as the maximum and then the smallest index that attains it.  The
//                result is a bin centre, bit-equal to NumPy's.
//   Li           v = w - min.  The tolerance is half the smallest gap between distinct values: a bitonic sort of v in LDS,
//                padded with +inf to a power of two, and a minimum over adjacent differences.  From the mean of v, every step
//                takes the count and the sums of v > t and of the rest through the fixed tree below; mean_back == 0 ends the
//                loop, otherwise t = (mean_back - mean_fore) / (log(mean_back) - log(mean_fore)); the loop ends when
//                |t - t_prev| > tolerance is false (a NaN from an empty side ends it and stays, as in NumPy).  The published loop
//                has no bound; here a window still running after 1000 steps raises a flag and writes nothing.
//   centroid     values w < t count as zero (false for a NaN t: nothing is zeroed): s = sum(w), sr = sum(w * (double)row),
//                sc = sum(w * (double)col) with window-local indices, out = (sc / s, sr / s); 0 / 0 = NaN is kept.
// The fixed tree: a lane adds its pixels i = lane, lane + lanes, ... in that order, the 64 lanes of a wave are joined by
// shuffles (32, 16, .. 1), the waves in order.  Two runs agree bit for bit.
//
// A window that leaves the frame raises the error flag and writes nothing.  In point mode (zk_com_refine_points_dev) the corner
// is rint(point) - size / 2 and the result (centroid - size / 2.0) + point, the two rounded operations of the host wrapper.
// LDS: 8 bytes a pixel, plus 8 bytes a padded pixel for Li's sort or 8200 bytes of Otsu's tables: 66 KiB at most.  The
// loads of a window are rows of `size` neighbouring pixels; what binds the kernel has not been measured beyond whole-call times.
#include <math.h>

#include "zk_np_bins.h"
#include "zk_point_window.h"

namespace {

constexpr int MIN_SIZE = 2, MAX_SIZE = 64;           // the side of a window
constexpr int WAVE_AREA = 256;                       // windows up to this many pixels take one wave, larger ones four
constexpr int LI_MAX_ITERATIONS = 1000;

enum { ERR_LI = 2 };                                 // beside ERR_WINDOW in the flag word

struct op_add {
  __device__ double operator()(double a, double b) const { return a + b; }
};
struct op_min {
  __device__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct op_max {
  __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

// The lanes' values through the fixed tree; every lane returns with the joined values.  red holds 3 x 4 doubles.
template <int NT, int NV, class Op>
__device__ inline void block_all(double (&a)[NV], double* red, Op op) {
#pragma unroll
  for (int j = 0; j < NV; ++j)
    for (int d = 32; d > 0; d >>= 1) a[j] = op(a[j], __shfl_down(a[j], d, 64));
  if (NT == 64) {
#pragma unroll
    for (int j = 0; j < NV; ++j) a[j] = __shfl(a[j], 0, 64);
    return;
  }
  __syncthreads();                                   // whoever still reads red from the call before
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < NV; ++j) red[j * 4 + (threadIdx.x >> 6)] = a[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double r = red[j * 4];
    for (int q = 1; q < NT / 64; ++q) r = op(r, red[j * 4 + q]);
    a[j] = r;
  }
}

template <int NT, class Op>
__device__ inline double block_all1(double v, double* red, Op op) {
  double a[1] = {v};
  block_all<NT, 1>(a, red, op);
  return a[0];
}

// Otsu's threshold of the window w[0 .. area) with lo < hi.  tab: 257 edges, 256 + 256 cumulative sums, 256 + 256 counters.
template <int NT>
__device__ inline double otsu_threshold(const double* w, int area, double lo, double hi, double* tab, double* red) {
  const int t = threadIdx.x;
  double *edge = tab, *fwd = tab + BINS + 1, *bwd = fwd + BINS;
  int *hist = (int*)(bwd + BINS), *below = hist + BINS;
  const double step = (hi - lo) / (double)BINS;
  for (int k = t; k <= BINS; k += NT) {
    edge[k] = k == BINS ? hi : (double)k * step + lo;
    if (k < BINS) hist[k] = 0;
  }
  __syncthreads();
  for (int i = t; i < area; i += NT) atomicAdd(&hist[np_bin(w[i], lo, hi, edge)], 1);
  __syncthreads();
  if (t < 2) {                                       // np.cumsum is sequential: lane 0 upwards, lane 1 downwards
    double acc = 0;
    int seen = 0;
    for (int q = 0; q < BINS; ++q) {
      const int j = t ? BINS - 1 - q : q, c = hist[j];
      const double term = (double)c * ((edge[j] + edge[j + 1]) / 2);
      acc = q ? acc + term : term;
      seen += c;
      if (t) {
        bwd[j] = acc;
      } else {
        fwd[j] = acc;
        below[j] = seen;
      }
    }
  }
  __syncthreads();
  double var[BINS / NT], best = -1;                  // split k = t + NT * q of this lane (a variance is never negative)
#pragma unroll
  for (int q = 0; q < BINS / NT; ++q) {
    const int k = t + NT * q;
    var[q] = -1;
    if (k >= BINS - 1) continue;
    const int w1 = below[k], w2 = area - w1;         // both at least 1: the first bin holds the minimum, the last the maximum
    const double d = fwd[k] / (double)w1 - bwd[k + 1] / (double)w2;
    var[q] = (double)((long long)w1 * w2) * (d * d);
    best = fmax(best, var[q]);
  }
  best = block_all1<NT>(best, red, op_max());
  double first = (double)BINS;
#pragma unroll
  for (int q = 0; q < BINS / NT; ++q)
    if (var[q] == best) first = fmin(first, (double)(t + NT * q));
  first = block_all1<NT>(first, red, op_min());
  const int k = first < (double)(BINS - 1) ? (int)first : 0;               // a NaN variance everywhere (NaN pixels): np.argmax gives 0
  return (edge[k] + edge[k + 1]) / 2;
}

// Li's threshold of the window (lo < hi), less lo.  sorted: room for `padded` doubles.  Returns false when the loop did not end.
template <int NT>
__device__ inline bool li_threshold(const double* w, int area, int padded, double lo, double* sorted, double* red, double* t_out,
                                    int* iterations_out) {
  const int t = threadIdx.x;
  for (int i = t; i < padded; i += NT) sorted[i] = i < area ? w[i] - lo : INFINITY;
  __syncthreads();
  for (int k = 2; k <= padded; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < padded; i += NT) {
        const int l = i ^ j;
        if (l > i) {
          const double a = sorted[i], b = sorted[l];
          if ((a > b) == ((i & k) == 0)) {
            sorted[i] = b;
            sorted[l] = a;
          }
        }
      }
      __syncthreads();
    }
  double gap = INFINITY, sum = 0;
  for (int i = t; i < area; i += NT) {
    if (i + 1 < area) {
      const double g = sorted[i + 1] - sorted[i];
      if (g > 0) gap = fmin(gap, g);
    }
    sum += w[i] - lo;
  }
  const double tolerance = block_all1<NT>(gap, red, op_min()) / 2;
  double now = block_all1<NT>(sum, red, op_add()) / (double)area, before = -2 * tolerance;
  int iterations = 0;
  bool ended = true;
  while (fabs(now - before) > tolerance) {
    if (iterations == LI_MAX_ITERATIONS) {
      ended = false;
      break;
    }
    before = now;
    ++iterations;
    double side[3] = {0, 0, 0};                      // count of v > t, their sum, the sum of the rest
    for (int i = t; i < area; i += NT) {
      const double v = w[i] - lo;
      const bool fore = v > before;
      side[0] += fore ? 1.0 : 0.0;
      side[1] += fore ? v : 0.0;
      side[2] += fore ? 0.0 : v;
    }
    block_all<NT, 3>(side, red, op_add());
    const double mean_fore = side[1] / side[0], mean_back = side[2] / ((double)area - side[0]);
    if (mean_back == 0) break;
    now = (mean_back - mean_fore) / (log(mean_back) - log(mean_fore));
  }
  *t_out = now;
  *iterations_out = iterations;
  return ended;
}

template <typename T, int NT>
__global__ __launch_bounds__(NT) void com_refine_kernel(const T* __restrict__ img, long long H, long long W, const void* __restrict__ pts,
                                                        int pts_dtype, int size, int padded, int otsu, double* __restrict__ out,
                                                        double* __restrict__ thresholds, int* __restrict__ iterations,
                                                        int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double red[12];
  const int t = threadIdx.x, area = size * size;
  const long long n = blockIdx.x;
  double *w = lds, *work = lds + area;
  // the corner of the window: uniform over the workgroup, so every exit below is taken by all lanes
  const point_window at = window_at(pts, pts_dtype, n, size, H, W);
  if (!at.inside) {
    if (t == 0) atomicOr(flag, ERR_WINDOW);
    return;
  }
  double range[2] = {INFINITY, -INFINITY};
  for (int i = t; i < area; i += NT) {
    const double v = (double)img[(at.y0 + i / size) * W + at.x0 + i % size];
    w[i] = v;
    range[0] = fmin(range[0], v);
    range[1] = fmax(range[1], v);
  }
  __syncthreads();
  const double lo = block_all1<NT>(range[0], red, op_min()), hi = block_all1<NT>(range[1], red, op_max());
  double level = lo;
  int steps = 0;
  if (lo != hi) {
    if (otsu) {
      level = otsu_threshold<NT>(w, area, lo, hi, work, red);
    } else {
      double above;
      if (!li_threshold<NT>(w, area, padded, lo, work, red, &above, &steps)) {
        if (t == 0) atomicOr(flag, ERR_LI);
        return;
      }
      level = above + lo;
    }
  }
  double sums[3] = {0, 0, 0};
  for (int i = t; i < area; i += NT) {
    const double v = w[i] < level ? 0.0 : w[i];
    sums[0] += v;
    sums[1] += v * (double)(i / size);
    sums[2] += v * (double)(i % size);
  }
  block_all<NT, 3>(sums, red, op_add());
  if (t == 0) {
    double x = sums[2] / sums[0], y = sums[1] / sums[0];
    if (pts_dtype != CORNERS) {
      x = (x - (double)size / 2) + at.px;
      y = (y - (double)size / 2) + at.py;
    }
    out[2 * n] = x;
    out[2 * n + 1] = y;
    if (thresholds) thresholds[n] = level;
    if (iterations) iterations[n] = steps;
  }
}

int check_com(const char* who, const void* img, int dtype, int64_t H, int64_t W, const void* pts, int64_t n, int64_t size, int threshold,
              const void* out) {
  int rc;
  if ((rc = check_frame(who, img, dtype, H, W, n))) return rc;
  const std::string name(who);
  if (size < MIN_SIZE || size > MAX_SIZE) return zk_fail(ZK_E_BADARG, name + ": needs 2 <= size <= 64");
  if (threshold != ZK_THRESHOLD_LI && threshold != ZK_THRESHOLD_OTSU) return zk_fail(ZK_E_BADARG, name + ": unknown threshold");
  return check_pointers(who, n, pts && out);
}

template <typename T, int NT>
int com_launch(const void* img, int64_t H, int64_t W, const void* pts, int pts_dtype, int64_t n, int size, int padded, int otsu,
               size_t lds, double* out, double* thresholds, int* iterations, int* flag, hipStream_t s) {
  if (lds + 1024 > 64 * 1024)                        // with the static words beside it the tile may pass 64 KiB
    ZK_HIP(hipFuncSetAttribute((const void*)com_refine_kernel<T, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((com_refine_kernel<T, NT>), dim3((unsigned)n), dim3(NT), lds, s, (const T*)img, (long long)H, (long long)W, pts,
                     pts_dtype, size, padded, otsu, out, thresholds, iterations, flag);
  ZK_HIP(hipGetLastError());
  return 0;
}

int com_call(const char* who, const void* img, int dtype, int64_t H, int64_t W, const void* pts, int pts_dtype, int64_t n, int size,
             int threshold, double* out, double* thresholds, int* iterations, hipStream_t s) {
  if (n == 0) return 0;
  int rc, flags;
  dev_flag flag;
  if ((rc = flag.arm(s))) return rc;
  const int area = size * size, otsu = threshold == ZK_THRESHOLD_OTSU;
  int padded = 2;
  while (padded < area) padded <<= 1;
  const size_t tables = sizeof(double) * (3 * BINS + 1) + sizeof(int) * 2 * BINS;
  const size_t lds = sizeof(double) * area + (otsu ? tables : sizeof(double) * padded);
  if (area <= WAVE_AREA)
    rc = dtype == ZK_F32 ? com_launch<float, 64>(img, H, W, pts, pts_dtype, n, size, padded, otsu, lds, out, thresholds, iterations, flag.word(), s)
                         : com_launch<double, 64>(img, H, W, pts, pts_dtype, n, size, padded, otsu, lds, out, thresholds, iterations, flag.word(), s);
  else
    rc = dtype == ZK_F32 ? com_launch<float, 256>(img, H, W, pts, pts_dtype, n, size, padded, otsu, lds, out, thresholds, iterations, flag.word(), s)
                         : com_launch<double, 256>(img, H, W, pts, pts_dtype, n, size, padded, otsu, lds, out, thresholds, iterations, flag.word(), s);
  if (rc || (rc = flag.read(s, &flags))) return rc;
  if (flags & ERR_WINDOW) return window_fail(who);
  if (flags & ERR_LI) return zk_fail(ZK_E_BADARG, std::string(who) + ": Li's iteration has not ended after 1000 steps in a window");
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_com_refine_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const int32_t* corners_dev,
                                 int64_t n, int64_t size, int threshold, double* centroids_dev, double* thresholds_dev,
                                 int32_t* iterations_dev, void* hip_stream) {
  int rc = check_com("com_refine", image_dev, image_dtype, H, W, corners_dev, n, size, threshold, centroids_dev);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return com_call("com_refine", image_dev, image_dtype, H, W, corners_dev, CORNERS, n, (int)size, threshold, centroids_dev, thresholds_dev,
                  iterations_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_com_refine_points_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const void* points_dev,
                                        int points_dtype, int64_t n, int64_t size, int threshold, double* out_dev, void* hip_stream) {
  int rc = check_com("com_refine_points", image_dev, image_dtype, H, W, points_dev, n, size, threshold, out_dev);
  if (rc) return rc;
  if (points_dtype != ZK_I32 && points_dtype != ZK_F64) return zk_fail(ZK_E_BADARG, "com_refine_points: points are ZK_F64 or ZK_I32");
  ZK_ON_DEVICE(device);
  return com_call("com_refine_points", image_dev, image_dtype, H, W, points_dev, points_dtype, n, (int)size, threshold, out_dev, nullptr,
                  nullptr, (hipStream_t)hip_stream);
}

extern "C" int zk_com_refine(int device, const void* image_host, int image_dtype, int64_t H, int64_t W, const int32_t* corners_host,
                             int64_t n, int64_t size, int threshold, double* centroids_out, double* thresholds_out,
                             int32_t* iterations_out) {
  int rc = check_com("com_refine", image_host, image_dtype, H, W, corners_host, n, size, threshold, centroids_out);
  if (rc) return rc;
  if (!corners_inside(corners_host, n, size, H, W)) return window_fail("com_refine");   // before anything is launched
  if (n == 0) return 0;
  ZK_ON_DEVICE(device);
  const size_t count = (size_t)n;
  const size_t img_bytes = zk_elem_size(image_dtype) * (size_t)H * (size_t)W, corner_bytes = sizeof(int32_t) * 2 * count,
               cen_bytes = sizeof(double) * 2 * count, thr_bytes = sizeof(double) * count, it_bytes = sizeof(int32_t) * count;
  dev_buf d_img, d_corners, d_cen, d_thr, d_it;      // the three results are computed whether or not the caller takes them
  if ((rc = d_img.upload(image_host, img_bytes)) || (rc = d_corners.upload(corners_host, corner_bytes)) || (rc = d_cen.alloc(cen_bytes)) ||
      (rc = d_thr.alloc(thr_bytes)) || (rc = d_it.alloc(it_bytes)) ||
      (rc = com_call("com_refine", d_img.p, image_dtype, H, W, d_corners.p, CORNERS, n, (int)size, threshold, d_cen.as<double>(),
                     d_thr.as<double>(), d_it.as<int>(), (hipStream_t)0)) ||
      (rc = d_cen.download(centroids_out, cen_bytes)) || (rc = d_thr.download(thresholds_out, thr_bytes)))
    return rc;
  return d_it.download(iterations_out, it_bytes);
}

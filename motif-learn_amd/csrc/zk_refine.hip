// zk_refine.hip -- the sub-pixel centroid refinement of the reference's features/_keypoint.py (center_of_mass_refine) on the
// device, the first of the two steps its notebooks take between key points and bonds (the second, the passes over the data
// of estimate_d, is zk_knn.hip).
//
// zk_refine_points.  The reference paints one label image in point order and reduces every label with SciPy's center_of_mass.
// Here:
//   owner        an int32 image, zeroed, then atomicMax(label) over every pixel of every (2 size + 1)^2 box, label = index + 1:
//                the last painter of a pixel is the largest label (integer atomics: the image does not depend on the order
//                the lanes arrive in).  A box that leaves the frame raises the error flag and paints nothing.
//   sums         one lane per point walks its own box in raveled (row-major) order and adds, for the pixels it owns, the value,
//                value * (double)row and value * (double)col into three float64 sums, each product rounded once (the file is
//                compiled with -ffp-contract=off): the order and the operations of np.bincount over the raveled frame, which
//                is what SciPy's label sums are.  In disk mode the last painter's box corners painted 0 in the reference, so
//                a pixel counts only when the owner is this point AND the pixel lies in this point's disk; whoever was
//                painted over stays painted over.  x = sum(value * col) / sum(value), y likewise with row; a point that owns
//                nothing gives 0 / 0 = NaN, as SciPy does.
// A box holds a few hundred pixels at most and neighbouring lanes read neighbouring boxes only by chance (the points come
// in the caller's order): the loads are not coalesced.  What binds the kernel has not been measured beyond whole-call times.
#include "zk_point_window.h"

namespace {

constexpr int MAX_SIZE = 64;                         // half-width of a refinement box at most

enum { ERR_BOX = 1 };                                // the box rule is not the window rule of zk_point_window.h: a flag bit of its own

__device__ inline bool box_inside(int x, int y, int size, long long H, long long W) {
  return (long long)x - size >= 0 && (long long)x + size < W && (long long)y - size >= 0 && (long long)y + size < H;
}

// one lane per (point, box pixel)
__global__ __launch_bounds__(256) void paint_kernel(const int* __restrict__ pts, long long n, int size, long long H, long long W,
                                                    int* __restrict__ owner, int* __restrict__ flag) {
  const int side = 2 * size + 1;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)side * side;
  if (t >= n * per) return;
  const long long i = t / per;
  const int e = (int)(t - i * per), x = pts[2 * i], y = pts[2 * i + 1];
  if (!box_inside(x, y, size, H, W)) {
    if (e == 0) atomicOr(flag, ERR_BOX);
    return;
  }
  const long long row = (long long)y - size + e / side, col = (long long)x - size + e % side;
  atomicMax(owner + row * W + col, (int)(i + 1));
}

template <typename T>
__global__ __launch_bounds__(64) void centroid_kernel(const T* __restrict__ img, const int* __restrict__ pts, long long n, int size,
                                                      int disk, long long H, long long W, const int* __restrict__ owner,
                                                      double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const int x = pts[2 * i], y = pts[2 * i + 1], label = (int)(i + 1);
  double s = 0, sr = 0, sc = 0;
  if (box_inside(x, y, size, H, W)) {
    for (int dy = -size; dy <= size; ++dy) {
      const long long row = (long long)y + dy;
      for (int dx = -size; dx <= size; ++dx) {
        const long long col = (long long)x + dx;
        if (owner[row * W + col] != label) continue;
        if (disk && dx * dx + dy * dy > size * size) continue;
        const double v = (double)img[row * W + col];
        s += v;
        sr += v * (double)row;
        sc += v * (double)col;
      }
    }
  }
  out[2 * i] = sc / s;
  out[2 * i + 1] = sr / s;
}

int check_refine(const void* img, int dtype, int64_t H, int64_t W, const void* pts, int64_t n, int64_t size, int mode, const void* out) {
  int rc;
  if ((rc = check_frame("refine_points", img, dtype, H, W, n))) return rc;   // n < 2^24: the reference's label image has the frame's type
  if (size < 0 || size > MAX_SIZE) return zk_fail(ZK_E_BADARG, "refine_points: needs 0 <= size <= 64");
  if (mode != ZK_REFINE_BOX && mode != ZK_REFINE_DISK) return zk_fail(ZK_E_BADARG, "refine_points: unknown mode");
  return check_pointers("refine_points", n, pts && out);
}

int box_fail() {
  return zk_fail(ZK_E_BADARG, "refine_points: a box leaves the frame (every point needs size <= x < W - size, size <= y < H - size)");
}

int refine_call(const void* img, int dtype, int64_t H, int64_t W, const int* pts, int64_t n, int size, int mode, double* out,
                hipStream_t s) {
  if (n == 0) return 0;
  int rc, flags;
  dev_buf d_owner;
  dev_flag flag;
  if ((rc = d_owner.alloc(sizeof(int) * (size_t)H * (size_t)W)) || (rc = flag.arm(s))) return rc;
  ZK_HIP(hipMemsetAsync(d_owner.p, 0, sizeof(int) * (size_t)H * (size_t)W, s));
  const long long per = (long long)(2 * size + 1) * (2 * size + 1);
  hipLaunchKernelGGL(paint_kernel, dim3(blocks_of(n * per)), dim3(256), 0, s, pts, (long long)n, size, (long long)H, (long long)W,
                     d_owner.as<int>(), flag.word());
  const dim3 grid((unsigned)((n + 63) / 64));
  if (dtype == ZK_F32)
    hipLaunchKernelGGL(centroid_kernel<float>, grid, dim3(64), 0, s, (const float*)img, pts, (long long)n, size, mode == ZK_REFINE_DISK,
                       (long long)H, (long long)W, d_owner.as<int>(), out);
  else
    hipLaunchKernelGGL(centroid_kernel<double>, grid, dim3(64), 0, s, (const double*)img, pts, (long long)n, size, mode == ZK_REFINE_DISK,
                       (long long)H, (long long)W, d_owner.as<int>(), out);
  ZK_HIP(hipGetLastError());
  if ((rc = flag.read(s, &flags))) return rc;        // the owner image goes with this call
  return flags & ERR_BOX ? box_fail() : 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_refine_points_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const int32_t* points_dev,
                                    int64_t n_points, int64_t size, int mode, double* out_dev, void* hip_stream) {
  int rc = check_refine(image_dev, image_dtype, H, W, points_dev, n_points, size, mode, out_dev);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return refine_call(image_dev, image_dtype, H, W, points_dev, n_points, (int)size, mode, out_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_refine_points(int device, const void* image_host, int image_dtype, int64_t H, int64_t W, const int32_t* points_host,
                                int64_t n_points, int64_t size, int mode, double* out_host) {
  int rc = check_refine(image_host, image_dtype, H, W, points_host, n_points, size, mode, out_host);
  if (rc) return rc;
  for (int64_t i = 0; i < n_points; ++i) {           // the boxes are checked before anything is launched
    const int64_t x = points_host[2 * i], y = points_host[2 * i + 1];
    if (x - size < 0 || x + size >= W || y - size < 0 || y + size >= H) return box_fail();
  }
  if (n_points == 0) return 0;
  ZK_ON_DEVICE(device);
  const size_t img_bytes = zk_elem_size(image_dtype) * (size_t)H * (size_t)W, pts_bytes = sizeof(int32_t) * 2 * (size_t)n_points,
               out_bytes = sizeof(double) * 2 * (size_t)n_points;
  dev_buf d_img, d_pts, d_out;
  if ((rc = d_img.upload(image_host, img_bytes)) || (rc = d_pts.upload(points_host, pts_bytes)) || (rc = d_out.alloc(out_bytes)) ||
      (rc = refine_call(d_img.p, image_dtype, H, W, d_pts.as<int>(), n_points, (int)size, mode, d_out.as<double>(), (hipStream_t)0)))
    return rc;
  return d_out.download(out_host, out_bytes);
}

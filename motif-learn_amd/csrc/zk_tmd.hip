// zk_tmd.hip -- device side of mtflearn.datasets.TMDImageSimulator (the reference's datasets/_tmd_simulator.py): a batch of
// float32 frames, each the sum of its *layers* (species).  A layer is a delta image -- its atoms' scales added at their
// rounded positions -- blurred by a separable kernel and multiplied by an amplitude.
//
//   delta stage   link: one lane per point takes its pixel (rint of the coordinates, off-frame points dropped) and pushes its
//                 index on that pixel's list (an integer exchange on the pixel's head, the previous head kept as the point's
//                 `next`): the lists live in the delta image itself, whose words are heads (-1: empty) until the next kernel.
//                 sum: one lane per pixel walks its list once per entry, each time taking the smallest index above the last
//                 one, and adds the scales in that -- ascending -- order in float32, as np.add.at does.  Then the word is the
//                 pixel's float.  No floating-point atomics: the order the lists were built in does not reach the result.
//   blur stage    one workgroup per TW x TH output tile of one frame, layer after layer: the column pass (axis 0) of the tile's
//                 rows over the tile's columns plus a halo of r on either side goes to LDS, the row pass (axis 1) reads it from
//                 there.  Both in float64 and in SciPy's order of operations (correlate1d of a symmetric kernel):
//                 t = c w[0], then t += (left + right) w[j] for j = r .. 1.
//                   ZK_TMD_FFT       zeros outside the frame; the intermediate stays float64; total = float32(float64(total) + A t)
//                                    -- fftconvolve(delta, A exp(-(x^2 + y^2) / 2 sigma^2), 'same') without the transform's error;
//                   ZK_TMD_GAUSSIAN  SciPy's 'reflect' (folded again when r >= n); each pass is stored as float32; then
//                                    total = total + float32(A) * blurred in float32 -- A * gaussian_filter(delta, sigma).
// A frame's result depends on its own layers only: alone or in a batch, host or resident entry, the bits are the same.
#pragma clang fp contract(off)

#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int TW = 64, TH = 4, THREADS = TW * TH;
constexpr int R_MAX = 960;                // TH rows of TW + 2 r float64 stay within 64 KiB of LDS

struct point {
  double x, y, scale;
};

struct layer {
  long long p0, p1;                       // its points
  long long w0;                           // its half kernel in the weight array
  double amp;
  int r;
};

// SciPy's 'reflect' boundary: period 2n, the second half mirrored
__device__ __forceinline__ int reflect_index(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// ---------------------------------------------------------------------------------------------------------------------
// delta stage
// ---------------------------------------------------------------------------------------------------------------------

// blockIdx.y: the layer.  head: (L, H, W) int32, -1 everywhere before the launch.
__global__ __launch_bounds__(256) void link_kernel(const point* __restrict__ pts, const layer* __restrict__ layers, int H, int W,
                                                   int* __restrict__ head, int* __restrict__ next) {
  const layer ly = layers[blockIdx.y];
  const long long i = ly.p0 + (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= ly.p1) return;
  const double x = rint(pts[i].x), y = rint(pts[i].y);
  if (!(x >= 0.0 && x < (double)W && y >= 0.0 && y < (double)H)) return;
  const long long pix = ((long long)blockIdx.y * H + (long long)y) * W + (long long)x;
  next[i] = atomicExch(&head[pix], (int)i);
}

// One lane per pixel of the (L, H, W) image: the head word becomes the float32 sum of the listed scales, ascending index.
__global__ __launch_bounds__(256) void sum_kernel(const point* __restrict__ pts, const int* __restrict__ next, int* words, long long n) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= n) return;
  const int first = words[pix];
  float acc = 0.0f;
  int last = -1;
  while (first >= 0) {
    int best = INT_MAX;
    for (int k = first; k >= 0; k = next[k])
      if (k > last && k < best) best = k;
    if (best == INT_MAX) break;
    acc = acc + (float)pts[best].scale;
    last = best;
  }
  words[pix] = __float_as_int(acc);
}

// ---------------------------------------------------------------------------------------------------------------------
// blur stage
// ---------------------------------------------------------------------------------------------------------------------

template <bool FFT>
__global__ __launch_bounds__(THREADS) void blur_kernel(const float* __restrict__ delta, float* __restrict__ frames, int H, int W,
                                                       const layer* __restrict__ layers, const int* __restrict__ frame_layers,
                                                       const double* __restrict__ weights) {
  extern __shared__ double mid[];                    // [TH][TW + 2 r] of the layer at hand
  const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW, b = blockIdx.z;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, X = x0 + tx, Y = y0 + ty;
  const bool mine = X < W && Y < H;
  float total = 0.0f;
  for (int l = frame_layers[b]; l < frame_layers[b + 1]; ++l) {
    const layer ly = layers[l];
    const int r = ly.r, span = TW + 2 * r;
    const double* w = weights + ly.w0;
    const float* d = delta + (long long)l * H * W;
    for (int e = tid; e < TH * span; e += THREADS) {
      const int row = e / span, c = e - row * span, y = y0 + row, xl = x0 - r + c;
      double t = 0.0;
      if (FFT) {
        if (y < H && xl >= 0 && xl < W) {
          const float* col = d + xl;
          t = (double)col[(long long)y * W] * w[0];
          for (int j = r; j >= 1; --j) {
            const double up = y - j >= 0 ? (double)col[(long long)(y - j) * W] : 0.0;
            const double dn = y + j < H ? (double)col[(long long)(y + j) * W] : 0.0;
            t += (up + dn) * w[j];
          }
        }
      } else if (y < H) {
        const float* col = d + reflect_index(xl, W);
        t = (double)col[(long long)y * W] * w[0];
        if (y - r >= 0 && y + r < H) {
          for (int j = r; j >= 1; --j) t += ((double)col[(long long)(y - j) * W] + (double)col[(long long)(y + j) * W]) * w[j];
        } else {
          for (int j = r; j >= 1; --j)
            t += ((double)col[(long long)reflect_index(y - j, H) * W] + (double)col[(long long)reflect_index(y + j, H) * W]) * w[j];
        }
        t = (double)(float)t;                        // gaussian_filter1d's float32 output of axis 0
      }
      mid[e] = t;
    }
    __syncthreads();
    if (mine) {
      const double* line = mid + ty * span + tx + r;
      double t = line[0] * w[0];
      for (int j = r; j >= 1; --j) t += (line[-j] + line[j]) * w[j];
      if (FFT) total = (float)((double)total + ly.amp * t);
      else total = total + (float)ly.amp * (float)t;
    }
    __syncthreads();
  }
  if (mine) frames[((long long)b * H + Y) * W + X] = total;
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------

struct job {
  int64_t B, H, W, L;
  const int32_t* layer_frame;
  const int64_t* point_offsets;
  const double* points;
  const double* amps;
  const int64_t* weight_offsets;
  const double* weights;
  int mode;
};

int check_job(const void* frames, const void* masks, int dtype, const job& j) {
  if (dtype != ZK_F32) return zk_fail(ZK_E_BADARG, "zk_tmd_render: dtype must be ZK_F32");
  if (j.mode != ZK_TMD_FFT && j.mode != ZK_TMD_GAUSSIAN) return zk_fail(ZK_E_BADARG, "zk_tmd_render: mode must be ZK_TMD_FFT or ZK_TMD_GAUSSIAN");
  if (j.B < 1 || j.B > 65535) return zk_fail(ZK_E_BADARG, "zk_tmd_render: needs 1 <= batch <= 65535");
  if (j.H < 1 || j.W < 1 || j.H > (int64_t)65535 * TH || j.W >= ((int64_t)1 << 30))
    return zk_fail(ZK_E_BADARG, "zk_tmd_render: bad frame shape (needs 1 <= height <= 262140, 1 <= width < 2^30)");
  if (j.L < 0 || j.L > 65535) return zk_fail(ZK_E_BADARG, "zk_tmd_render: needs 0 <= n_layers <= 65535");
  const bool blur = j.weights != nullptr || j.weight_offsets != nullptr;
  if (blur && (!j.weights || !j.weight_offsets || !j.amps || !frames)) return zk_fail(ZK_E_BADARG, "zk_tmd_render: null pointer");
  if (!blur && !masks) return zk_fail(ZK_E_BADARG, "zk_tmd_render: null pointer (without weights there is nothing to write but the masks)");
  if (j.L && (!j.layer_frame || !j.point_offsets)) return zk_fail(ZK_E_BADARG, "zk_tmd_render: null pointer");
  if (j.L == 0) return 0;
  if (j.point_offsets[0] != 0) return zk_fail(ZK_E_BADARG, "zk_tmd_render: point_offsets must start at 0");
  for (int64_t l = 0; l < j.L; ++l) {
    if (j.point_offsets[l] > j.point_offsets[l + 1]) return zk_fail(ZK_E_BADARG, "zk_tmd_render: point_offsets must not decrease");
    if (j.layer_frame[l] < 0 || j.layer_frame[l] >= j.B) return zk_fail(ZK_E_BADARG, "zk_tmd_render: a layer's frame is outside the batch");
    if (l && j.layer_frame[l] < j.layer_frame[l - 1])
      return zk_fail(ZK_E_BADARG, "zk_tmd_render: the layers of a frame must be consecutive (layer_frame must not decrease)");
  }
  const int64_t n = j.point_offsets[j.L];
  if (n >= ((int64_t)1 << 31) - 1) return zk_fail(ZK_E_BADARG, "zk_tmd_render: bad point count (needs n < 2^31 - 1)");
  if (n && !j.points) return zk_fail(ZK_E_BADARG, "zk_tmd_render: null pointer");
  for (int64_t i = 0; i < 3 * n; ++i)
    if (!(fabs(j.points[i]) <= DBL_MAX)) return zk_fail(ZK_E_BADARG, "zk_tmd_render: points and scales must be finite");
  if ((double)j.L * (double)j.H * (double)j.W >= 9.0e18) return zk_fail(ZK_E_BADARG, "zk_tmd_render: the delta images are too large");
  if (!blur) return 0;
  if (j.weight_offsets[0] != 0) return zk_fail(ZK_E_BADARG, "zk_tmd_render: weight_offsets must start at 0");
  for (int64_t l = 0; l < j.L; ++l) {
    const int64_t r = j.weight_offsets[l + 1] - j.weight_offsets[l] - 1;
    if (r < 0) return zk_fail(ZK_E_BADARG, "zk_tmd_render: every layer needs a half kernel w[0 .. r] with r >= 0 (weight_offsets must increase)");
    if (r > R_MAX) return zk_fail(ZK_E_BADARG, "zk_tmd_render: a kernel radius above 960 is not supported");
    if (!(fabs(j.amps[l]) <= DBL_MAX)) return zk_fail(ZK_E_BADARG, "zk_tmd_render: amplitudes must be finite");
  }
  for (int64_t i = 0; i < j.weight_offsets[j.L]; ++i)
    if (!(fabs(j.weights[i]) <= DBL_MAX)) return zk_fail(ZK_E_BADARG, "zk_tmd_render: weights must be finite");
  return 0;
}

// frames: (B, H, W) float32 on the device, written whole (may be null without weights); masks: (L, H, W) float32 on the device
// or null.  Synchronises the stream before it returns: the staging buffers go with this call.
int run_job(float* frames, float* masks, const job& j, hipStream_t s) {
  const bool blur = j.weights != nullptr;
  const long long plane = (long long)j.H * j.W;
  int rc;
  if (j.L == 0) {
    if (blur) ZK_HIP(hipMemsetAsync(frames, 0, sizeof(float) * (size_t)(j.B * plane), s));
    ZK_HIP(hipStreamSynchronize(s));
    return 0;
  }
  const int64_t n = j.point_offsets[j.L];
  std::vector<layer> layers(j.L);
  std::vector<int> frame_layers(j.B + 1, 0);
  long long most = 0;
  int r_max = 0;
  for (int64_t l = 0; l < j.L; ++l) {
    layer& ly = layers[l];
    ly.p0 = j.point_offsets[l];
    ly.p1 = j.point_offsets[l + 1];
    ly.w0 = blur ? j.weight_offsets[l] : 0;
    ly.r = blur ? (int)(j.weight_offsets[l + 1] - j.weight_offsets[l] - 1) : 0;
    ly.amp = blur ? j.amps[l] : 0.0;
    most = std::max(most, ly.p1 - ly.p0);
    r_max = std::max(r_max, ly.r);
    frame_layers[j.layer_frame[l] + 1] += 1;
  }
  for (int64_t b = 0; b < j.B; ++b) frame_layers[b + 1] += frame_layers[b];

  dev_buf d_layers, d_frame_layers, d_weights, d_pts, d_next, d_delta;
  if ((rc = d_layers.alloc(sizeof(layer) * layers.size())) || (rc = d_frame_layers.alloc(sizeof(int) * frame_layers.size())) ||
      (rc = d_pts.alloc(sizeof(point) * (size_t)n)) || (rc = d_next.alloc(sizeof(int) * (size_t)n)))
    return rc;
  ZK_HIP(hipMemcpyAsync(d_layers.p, layers.data(), sizeof(layer) * layers.size(), hipMemcpyHostToDevice, s));
  ZK_HIP(hipMemcpyAsync(d_frame_layers.p, frame_layers.data(), sizeof(int) * frame_layers.size(), hipMemcpyHostToDevice, s));
  if (n) ZK_HIP(hipMemcpyAsync(d_pts.p, j.points, sizeof(point) * (size_t)n, hipMemcpyHostToDevice, s));
  if (blur) {
    const size_t bytes = sizeof(double) * (size_t)j.weight_offsets[j.L];
    if ((rc = d_weights.alloc(bytes))) return rc;
    ZK_HIP(hipMemcpyAsync(d_weights.p, j.weights, bytes, hipMemcpyHostToDevice, s));
  }
  float* delta = masks;
  const size_t delta_bytes = sizeof(float) * (size_t)(j.L * plane);
  if (!delta) {
    if ((rc = d_delta.alloc(delta_bytes))) return rc;
    delta = d_delta.as<float>();
  }

  ZK_HIP(hipMemsetAsync(delta, 0xFF, delta_bytes, s));        // every head -1
  if (most)
    hipLaunchKernelGGL(link_kernel, dim3(blocks_of(most), (unsigned)j.L), dim3(256), 0, s, d_pts.as<point>(), d_layers.as<layer>(),
                       (int)j.H, (int)j.W, (int*)delta, d_next.as<int>());
  const long long words = j.L * plane;
  for (long long at = 0; at < words; at += (long long)1 << 38) {       // 2^30 blocks per launch
    const long long part = std::min(words - at, (long long)1 << 38);
    hipLaunchKernelGGL(sum_kernel, dim3(blocks_of(part)), dim3(256), 0, s, d_pts.as<point>(), d_next.as<int>(), (int*)delta + at, part);
  }
  ZK_HIP(hipGetLastError());
  if (blur) {
    const dim3 grid((unsigned)((j.W + TW - 1) / TW), (unsigned)((j.H + TH - 1) / TH), (unsigned)j.B);
    const size_t lds = sizeof(double) * TH * (TW + 2 * (size_t)r_max);
    if (j.mode == ZK_TMD_FFT)
      hipLaunchKernelGGL((blur_kernel<true>), grid, dim3(THREADS), lds, s, delta, frames, (int)j.H, (int)j.W, d_layers.as<layer>(),
                         d_frame_layers.as<int>(), d_weights.as<double>());
    else
      hipLaunchKernelGGL((blur_kernel<false>), grid, dim3(THREADS), lds, s, delta, frames, (int)j.H, (int)j.W, d_layers.as<layer>(),
                         d_frame_layers.as<int>(), d_weights.as<double>());
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_tmd_render_dev(int device, void* frames_dev, void* masks_dev, int dtype, int64_t batch, int64_t height, int64_t width,
                                 int64_t n_layers, const int32_t* layer_frame_host, const int64_t* point_offsets_host,
                                 const double* points_host, const double* amplitudes_host, const int64_t* weight_offsets_host,
                                 const double* weights_host, int mode, void* hip_stream) {
  const job j{batch, height, width, n_layers, layer_frame_host, point_offsets_host, points_host, amplitudes_host, weight_offsets_host,
              weights_host, mode};
  const int rc = check_job(frames_dev, masks_dev, dtype, j);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return run_job((float*)frames_dev, (float*)masks_dev, j, (hipStream_t)hip_stream);
}

extern "C" int zk_tmd_render(int device, void* frames_host, void* masks_host, int dtype, int64_t batch, int64_t height, int64_t width,
                             int64_t n_layers, const int32_t* layer_frame_host, const int64_t* point_offsets_host,
                             const double* points_host, const double* amplitudes_host, const int64_t* weight_offsets_host,
                             const double* weights_host, int mode) {
  const job j{batch, height, width, n_layers, layer_frame_host, point_offsets_host, points_host, amplitudes_host, weight_offsets_host,
              weights_host, mode};
  int rc = check_job(frames_host, masks_host, dtype, j);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  const bool blur = weights_host != nullptr;
  const size_t frame_bytes = sizeof(float) * (size_t)(batch * height * width), mask_bytes = sizeof(float) * (size_t)(n_layers * height * width);
  dev_buf d_frames, d_masks;
  if (blur && (rc = d_frames.alloc(frame_bytes))) return rc;
  if (masks_host && (rc = d_masks.alloc(mask_bytes))) return rc;
  if ((rc = run_job(d_frames.as<float>(), d_masks.as<float>(), j, (hipStream_t)0))) return rc;
  if (blur && (rc = d_frames.download(frames_host, frame_bytes))) return rc;   // without weights no frame is rendered
  return d_masks.download(masks_host, mask_bytes);
}

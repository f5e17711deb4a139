// zk_background.hip -- device side of mtflearn.background (reference background/): the slowly varying background under
// the atomic columns, removed ahead of local_max.
//
//   opening       scipy.ndimage.grey_opening(image, (ky, kx)), mode 'reflect': a flat minimum filter (erosion) and then a
//                 flat maximum filter (dilation), each separable.  Erosion window along an axis of size k: [i - k/2,
//                 i - k/2 + k - 1]; dilation (SciPy shifts its origin by one on an even axis): [i - (k - 1 - k/2), ...].
//                 Each 1-D pass is van Herk / Gil-Werman over segments of k outputs (about three comparisons per pixel
//                 whatever k); the passes along x run on a transposed copy so that every pass reads along columns,
//                 coalesced.  Exact by construction.
//   baseline      num_iters rounds of gaussian_filter (column pass, then row pass) and np.minimum(., image), float64.
//                 Every tap follows SciPy's summation order for symmetric weights (t = x0 w0; t += (x[-j] + x[+j]) w[j]
//                 for j = r .. 1), products and sums unfused (fp contract off below): bit for bit SciPy's.
//   rolling ball  skimage.restoration.rolling_ball restated (parity unpinned: scikit-image is not a dependency):
//                 background(p) = min over ball offsets o of img[p + o] + diff[o], +inf outside the frame; a grey erosion
//                 with a non-flat ball.  Each workgroup streams the input rows its 16 x 256 output tile needs through LDS;
//                 each wave walks only the chords of the ball (dx in [-w(dy), w(dy)]) of the rows it holds, the diff table
//                 read with wave-uniform loads.  One add and one min per tap, float32 for float32 images and float64
//                 otherwise: the same rounding as the host restatement in any order.
//
// Residual (all three, optional): image - background in the background's type, then max(., 0) when clip is set.
// Edges: SciPy's 'reflect' (dcba|abcd), folded again and again when a window or radius exceeds the frame.
// NaN / inf pixels: the baseline is np.minimum's (a NaN on either side stays a NaN) and the residual NumPy's subtraction and
// np.clip; the rolling ball skips a NaN sum as scikit-image's `if min_value > tmp` does (no finite sum at all: +inf); the
// opening is exact on +-inf and unspecified on NaN (as SciPy's own min / max queue is).
// Long axes: every kernel that puts rows on grid.y strides over it (grid_y below), so a frame of one column is served.
#pragma clang fp contract(off)

#include <math.h>

#include <algorithm>
#include <limits>
#include <type_traits>
#include <vector>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int RB_NX = 4;                 // outputs per lane along x, 64 apart (conflict-free LDS reads)
constexpr int RB_TY = 4;                 // output rows per wave
constexpr int RB_WAVES = 4;
constexpr int RB_TW = 64 * RB_NX, RB_TH = RB_WAVES * RB_TY;
constexpr int RB_MAX_R = 1536;           // two staged rows of (RB_TW + 2 R) float64 stay within 64 KiB of LDS

// SciPy's 'reflect' boundary: period 2n, the second half mirrored
__device__ __forceinline__ int reflect_index(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

template <bool MAX, typename T>
__device__ __forceinline__ T pick(T a, T b) {
  if constexpr (MAX) return b > a ? b : a;
  else return b < a ? b : a;
}

// The y extent of a grid is 16 bits wide: more row blocks than that are strided over by the kernel (for (...; += gridDim.y ...)).
inline unsigned grid_y(long long blocks) { return (unsigned)std::min<long long>(blocks, 65535); }

// ---------------------------------------------------------------------------------------------------------------------
// opening
// ---------------------------------------------------------------------------------------------------------------------

// One 1-D min (MAX false) / max filter along the columns of an (H, W) image: out[y][x] = op over
// in[y - a .. y - a + k - 1][x].  A thread owns a segment of k output rows of one column: windows starting in
// [B, B + k - 1] (B = s - a) split at c = B + k - 1 into a suffix op over in[e .. c] and a prefix op over in[c + 1 .. e + k - 1].
// The suffix results are parked in `out` and completed by the prefix walk.  in != out.
template <typename T, bool MAX>
__global__ __launch_bounds__(256) void vh_column_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int k, int a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  if (x >= W) return;
  for (long long seg = (long long)blockIdx.y * 4 + (threadIdx.x >> 6); seg * k < H; seg += (long long)gridDim.y * 4) {
    const long long s = seg * k;
    const long long B = s - a;
    T run = in[(long long)reflect_index((int)(B + k - 1), H) * W + x];
    if (k - 1 + s < H) out[(s + k - 1) * W + x] = run;
    for (int j = k - 2; j >= 0; --j) {
      run = pick<MAX>(run, in[(long long)reflect_index((int)(B + j), H) * W + x]);
      if (s + j < H) out[(s + j) * W + x] = run;
    }
    T pre = run;  // overwritten at j = 1
    for (int j = 1; j < k && s + j < H; ++j) {
      const T v = in[(long long)reflect_index((int)(B + k - 1 + j), H) * W + x];
      pre = j == 1 ? v : pick<MAX>(pre, v);
      const long long o = (s + j) * W + x;
      out[o] = pick<MAX>(out[o], pre);
    }
  }
}

// (H, W) -> (W, H)
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W) {
  __shared__ T tile[64][65];
  const int bx = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (long long by = (long long)blockIdx.y * 64; by < H; by += (long long)gridDim.y * 64) {
    for (int r = ty; r < 64; r += 4) {
      const long long y = by + r;
      const int x = bx + tx;
      if (y < H && x < W) tile[r][tx] = in[y * W + x];
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
      const int x = bx + r;
      const long long y = by + tx;
      if (x < W && y < H) out[(long long)x * H + y] = tile[tx][r];
    }
    __syncthreads();  // the tile is refilled by the next block of rows
  }
}

template <typename T, bool MAX>
int column_pass(const T* in, T* out, int H, int W, int k, int a, hipStream_t s) {
  const long long segs = (H + (long long)k - 1) / k;
  hipLaunchKernelGGL((vh_column_kernel<T, MAX>), dim3(blocks_of(W, 64), grid_y(blocks_of(segs, 4))), dim3(256), 0, s, in, out, H, W, k, a);
  ZK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int transpose(const T* in, T* out, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel<T>, dim3(blocks_of(W, 64), grid_y(blocks_of(H, 64))), dim3(256), 0, s, in, out, H, W);
  ZK_HIP(hipGetLastError());
  return 0;
}

// erosion (axis 0, then axis 1), then dilation (axis 1, then axis 0; min / max filters are exact in any axis order)
template <typename T>
int opening_core(const void* img_v, int H, int W, int ky, int kx, void* bg_v, hipStream_t s) {
  // a window of 2n or more covers a whole period of the reflected line: every such window gives the same result
  ky = (int)std::min<long long>(ky, 2LL * H);
  kx = (int)std::min<long long>(kx, 2LL * W);
  const T* img = (const T*)img_v;
  T* bg = (T*)bg_v;
  const size_t bytes = (size_t)H * W * sizeof(T);
  if (ky == 1 && kx == 1) {
    ZK_HIP(hipMemcpyAsync(bg, img, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  dev_buf s1, s2;
  int rc;
  if ((rc = s1.alloc(bytes)) || (kx > 1 && (rc = s2.alloc(bytes)))) return rc;
  T* S1 = s1.as<T>();
  T* S2 = s2.as<T>();
  const T* cur = img;
  if (ky > 1) {
    if ((rc = column_pass<T, false>(img, S1, H, W, ky, ky / 2, s))) return rc;
    cur = S1;
  }
  if (kx > 1) {
    if ((rc = transpose<T>(cur, S2, H, W, s)) || (rc = column_pass<T, false>(S2, S1, W, H, kx, kx / 2, s)) ||
        (rc = column_pass<T, true>(S1, S2, W, H, kx, kx - 1 - kx / 2, s)) || (rc = transpose<T>(S2, ky > 1 ? S1 : bg, W, H, s)))
      return rc;
  }
  if (ky > 1 && (rc = column_pass<T, true>(S1, bg, H, W, ky, ky - 1 - ky / 2, s))) return rc;
  ZK_HIP(hipStreamSynchronize(s));  // the scratch is freed on return
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// baseline
// ---------------------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void widen_kernel(const T* __restrict__ in, double* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = (double)in[i];
}

// One gaussian_filter1d pass of radius r (weights w[0..r], w[0] the centre) along x (ALONG_X) or y, SciPy's order of
// operations; WITH_MIN: then np.minimum(., img).  One output per thread, lanes along x (coalesced either way).
template <bool ALONG_X, bool WITH_MIN>
__global__ __launch_bounds__(256) void gauss_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                    const double* __restrict__ img, int H, int W, const double* __restrict__ w, int r) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  if (x >= W) return;
  for (long long yy = (long long)blockIdx.y * 4 + (threadIdx.x >> 6); yy < H; yy += (long long)gridDim.y * 4) {
    const int y = (int)yy;
    const int n = ALONG_X ? W : H, i = ALONG_X ? x : y;
    const long long stride = ALONG_X ? 1 : W;
    const double* line = ALONG_X ? in + (long long)y * W : in + x;
    double t = line[i * stride] * w[0];
    if (i - r >= 0 && i + r < n) {
      for (int j = r; j >= 1; --j) t += (line[(i - j) * stride] + line[(i + j) * stride]) * w[j];
    } else {
      for (int j = r; j >= 1; --j)
        t += (line[(long long)reflect_index(i - j, n) * stride] + line[(long long)reflect_index(i + j, n) * stride]) * w[j];
    }
    const long long o = (long long)y * W + x;
    if (WITH_MIN) {
      const double v = img[o];
      t = (v < t || v != v) ? v : t;  // np.minimum: a NaN on either side stays a NaN
    }
    out[o] = t;
  }
}

template <typename T>
int baseline_core(const void* img_v, int H, int W, const double* wy_host, int ry, const double* wx_host, int rx, int iters,
                  double* bg, hipStream_t s) {
  const long long n = (long long)H * W;
  dev_buf d_img, d_tmp, d_w;
  int rc;
  if ((rc = d_tmp.alloc((size_t)n * 8)) || (rc = d_w.alloc((size_t)(ry + rx + 2) * 8))) return rc;
  const double* img;
  if constexpr (std::is_same<T, double>::value) {
    img = (const double*)img_v;
  } else {
    if ((rc = d_img.alloc((size_t)n * 8))) return rc;
    hipLaunchKernelGGL(widen_kernel<T>, dim3(std::min<unsigned>(blocks_of(n, 256), 2048)), dim3(256), 0, s, (const T*)img_v,
                       d_img.as<double>(), n);
    ZK_HIP(hipGetLastError());
    img = d_img.as<double>();
  }
  double* wy = d_w.as<double>();
  double* wx = wy + ry + 1;
  ZK_HIP(hipMemcpyAsync(wy, wy_host, (size_t)(ry + 1) * 8, hipMemcpyHostToDevice, s));
  ZK_HIP(hipMemcpyAsync(wx, wx_host, (size_t)(rx + 1) * 8, hipMemcpyHostToDevice, s));
  const dim3 grid(blocks_of(W, 64), grid_y(blocks_of(H, 4)));
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL((gauss_kernel<false, false>), grid, dim3(256), 0, s, it ? bg : img, d_tmp.as<double>(), nullptr, H, W, wy, ry);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL((gauss_kernel<true, true>), grid, dim3(256), 0, s, d_tmp.as<double>(), bg, img, H, W, wx, rx);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// rolling ball
// ---------------------------------------------------------------------------------------------------------------------

// The smallest of acc and the sums s (and s2), a NaN sum skipped, as v_min / v_min3: no operand is ever a signalling NaN (acc is
// +inf or an earlier minimum, a sum the result of an add), so the instruction keeps the other operands where one is a NaN, which
// is fmin().  Spelled as the instruction because fmin() makes the compiler quiet acc again on every tap (a canonicalising v_max
// per v_min).
__device__ __forceinline__ float min_skip_nan(float acc, float s) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(acc), "v"(s));
  return r;
}
__device__ __forceinline__ double min_skip_nan(double acc, double s) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(acc), "v"(s));
  return r;
}
__device__ __forceinline__ float min_skip_nan(float acc, float s, float s2) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(acc), "v"(s), "v"(s2));
  return r;
}
__device__ __forceinline__ double min_skip_nan(double acc, double s, double s2) { return min_skip_nan(min_skip_nan(acc, s), s2); }

// diff: (2R + 2) rows of 2R + 1 (+inf off the ball; the last row all +inf); chord[dy + R]: the half-width of row dy, -1 when it is empty.
// Lane l of wave v owns outputs (y0 + v RB_TY + t, x0 + l + 64 u); LDS holds two staged input rows of columns
// x0 - R .. x0 + RB_TW + R - 1 (+inf off the frame); rows off the frame are skipped (+inf contributes nothing).  A workgroup
// takes the tiles y0 = (blockIdx.y + i gridDim.y) RB_TH in turn.
template <typename T, typename A>
__global__ __launch_bounds__(256) void rolling_ball_kernel(const T* __restrict__ img, T* __restrict__ out, int H, int W, int R,
                                                           const A* __restrict__ diff, const int* __restrict__ chord) {
  extern __shared__ __align__(16) unsigned char rb_lds[];
  A* rows = (A*)rb_lds;
  const int LW = RB_TW + 2 * R, PW = 2 * R + 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x0 = blockIdx.x * RB_TW;
  const A inf = std::numeric_limits<A>::infinity();
  auto stage = [&](int yi, A* dst) {
    const T* src = img + (long long)yi * W;
    for (int c = threadIdx.x; c < LW; c += 256) {
      const int gx = x0 - R + c;
      dst[c] = (gx >= 0 && gx < W) ? (A)src[gx] : inf;
    }
  };
  for (long long tile = blockIdx.y; tile * RB_TH < H; tile += gridDim.y) {
    const int y0 = (int)(tile * RB_TH);
    const int yw = y0 + wave * RB_TY;
    A acc[RB_TY][RB_NX];
#pragma unroll
    for (int t = 0; t < RB_TY; ++t)
#pragma unroll
      for (int u = 0; u < RB_NX; ++u) acc[t][u] = inf;

    const int yi_lo = max(y0 - R, 0), yi_hi = min(y0 + RB_TH - 1 + R, H - 1);
    stage(yi_lo, rows);  // the last tile's reads ended at its closing barrier
    __syncthreads();
    for (int yi = yi_lo, b = 0; yi <= yi_hi; ++yi, b ^= 1) {
      if (yi < yi_hi) stage(yi + 1, rows + (b ^ 1) * LW);
      const A* row = rows + b * LW + R + lane;  // row[dx + 64 u] = input (yi, x0 + lane + 64 u + dx)
      int wm = -1;
      int base[RB_TY];  // diff row offset + R of each output row; the all-inf row when its ball row is empty or off the ball
#pragma unroll
      for (int t = 0; t < RB_TY; ++t) {
        const int dy = yi - (yw + t);
        const int w = (dy >= -R && dy <= R && yw + t < H) ? chord[dy + R] : -1;
        base[t] = (w >= 0 ? dy + R : PW) * PW + R;
        wm = max(wm, w);
      }
      // branch-free over the rows: a row outside its chord adds +inf (the table is +inf there), which min ignores; a -inf pixel
      // there gives -inf + inf = NaN, which it skips
      // the tap at dx, and with PAIR the one at dx + 1: skimage keeps the smaller of the two; a NaN sum is skipped
      auto tap = [&](int dx, auto pair) {
        constexpr bool PAIR = decltype(pair)::value;
        A v[RB_NX], v2[RB_NX];
#pragma unroll
        for (int u = 0; u < RB_NX; ++u) {
          v[u] = row[dx + 64 * u];
          if constexpr (PAIR) v2[u] = row[dx + 1 + 64 * u];
        }
#pragma unroll
        for (int t = 0; t < RB_TY; ++t) {
          const A d = diff[base[t] + dx];
#pragma unroll
          for (int u = 0; u < RB_NX; ++u) {
            if constexpr (PAIR) acc[t][u] = min_skip_nan(acc[t][u], v[u] + d, v2[u] + diff[base[t] + dx + 1]);
            else acc[t][u] = min_skip_nan(acc[t][u], v[u] + d);
          }
        }
      };
      // the 2 wm + 1 taps two at a time (written out: the compiler does not unroll a loop around the v_min above by itself)
      for (int dx = -wm; dx < wm; dx += 2) tap(dx, std::true_type());
      if (wm >= 0) tap(wm, std::false_type());
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < RB_TY; ++t) {
      const int y = yw + t;
      if (y >= H) continue;
#pragma unroll
      for (int u = 0; u < RB_NX; ++u) {
        const int x = x0 + lane + 64 * u;
        if (x < W) out[(long long)y * W + x] = (T)acc[t][u];  // integer types: truncation, as astype
      }
    }
  }
}

// skimage's ball_kernel(radius, 2) and intensity difference, in the arithmetic type A
template <typename A>
void ball_tables(double radius, int R, std::vector<A>& diff, std::vector<int>& chord) {
  const int PW = 2 * R + 1;
  const double r2 = radius * radius;
  diff.assign((size_t)(PW + 1) * PW, std::numeric_limits<A>::infinity());
  chord.assign(PW, -1);
  const A centre = (A)sqrt(std::max(r2, 0.0));
  for (int dy = -R; dy <= R; ++dy)
    for (int dx = -R; dx <= R; ++dx) {
      const double ss = (double)dy * dy + (double)dx * dx;
      if (sqrt(ss) > radius) continue;
      const A kern = (A)sqrt(std::max(r2 - ss, 0.0));
      diff[(size_t)(dy + R) * PW + dx + R] = centre - kern;
      chord[dy + R] = std::max(chord[dy + R], std::abs(dx));
    }
}

template <typename T, typename A>
int rolling_ball_core(const void* img, int H, int W, double radius, void* bg, hipStream_t s) {
  const int R = (int)ceil(radius);
  std::vector<A> diff;
  std::vector<int> chord;
  ball_tables<A>(radius, R, diff, chord);
  dev_buf d_diff, d_chord;
  int rc;
  if ((rc = d_diff.alloc(diff.size() * sizeof(A))) || (rc = d_chord.alloc(chord.size() * sizeof(int)))) return rc;
  ZK_HIP(hipMemcpyAsync(d_diff.p, diff.data(), diff.size() * sizeof(A), hipMemcpyHostToDevice, s));
  ZK_HIP(hipMemcpyAsync(d_chord.p, chord.data(), chord.size() * sizeof(int), hipMemcpyHostToDevice, s));
  const size_t lds = (size_t)2 * (RB_TW + 2 * R) * sizeof(A);
  hipLaunchKernelGGL((rolling_ball_kernel<T, A>), dim3(blocks_of(W, RB_TW), grid_y(blocks_of(H, RB_TH))), dim3(256), lds, s, (const T*)img,
                     (T*)bg, H, W, R, d_diff.as<A>(), d_chord.as<int>());
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(s));  // the tables are freed on return
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// residual
// ---------------------------------------------------------------------------------------------------------------------

// res = TO(img) - bg in TO (integer types wrap as NumPy's do), then max(res, 0) under clip
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void residual_kernel(const TI* __restrict__ img, const TO* __restrict__ bg, TO* __restrict__ res,
                                                       long long n, int clip) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    TO d = (TO)((TO)img[i] - bg[i]);
    if (clip && d < (TO)0) d = (TO)0;
    res[i] = d;
  }
}

template <typename TI, typename TO>
int residual(const void* img, const void* bg, void* res, long long n, int clip, hipStream_t s) {
  hipLaunchKernelGGL((residual_kernel<TI, TO>), dim3(std::min<unsigned>(blocks_of(n, 256), 2048)), dim3(256), 0, s, (const TI*)img,
                     (const TO*)bg, (TO*)res, n, clip);
  ZK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------------------------------------

enum method { M_OPENING, M_ROLLING_BALL, M_BASELINE };

struct args {
  int method;
  int ky = 1, kx = 1;              // opening
  double radius = 0.0;             // rolling ball
  const double* wy = nullptr;      // baseline
  const double* wx = nullptr;
  int ry = 0, rx = 0, iters = 1;
};

template <typename T>
int run_typed(const args& a, const void* img, int H, int W, int clip, void* bg, void* res, hipStream_t s) {
  const long long n = (long long)H * W;
  int rc;
  if (a.method == M_BASELINE) {
    if ((rc = baseline_core<T>(img, H, W, a.wy, a.ry, a.wx, a.rx, a.iters, (double*)bg, s))) return rc;
    return res ? residual<T, double>(img, bg, res, n, clip, s) : 0;
  }
  if (a.method == M_OPENING) rc = opening_core<T>(img, H, W, a.ky, a.kx, bg, s);
  else if constexpr (std::is_same<T, float>::value) rc = rolling_ball_core<T, float>(img, H, W, a.radius, bg, s);
  else rc = rolling_ball_core<T, double>(img, H, W, a.radius, bg, s);
  if (rc) return rc;
  return res ? residual<T, T>(img, bg, res, n, clip, s) : 0;
}

int run(const args& a, const void* img, int dtype, int H, int W, int clip, void* bg, void* res, hipStream_t s) {
  return zk_with_elem(dtype, [&](auto e) { return run_typed<typename decltype(e)::type>(a, img, H, W, clip, bg, res, s); });
}

int check_common(int dtype, int64_t H, int64_t W, const void* img, const void* bg) {
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (H <= 0 || W <= 0 || H * W >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "bad image shape (needs 0 < height * width < 2^31)");
  if (!img || !bg) return zk_fail(ZK_E_BADARG, "null pointer");
  return 0;
}

int check_method(const args& a) {
  if (a.method == M_OPENING && (a.ky < 1 || a.kx < 1)) return zk_fail(ZK_E_BADARG, "opening sizes must be >= 1");
  if (a.method == M_ROLLING_BALL && !(a.radius > 0.0 && a.radius <= RB_MAX_R))
    return zk_fail(ZK_E_BADARG, "rolling-ball radius must be in (0, 1536]");
  if (a.method == M_BASELINE) {
    if (!a.wy || !a.wx || a.ry < 0 || a.rx < 0) return zk_fail(ZK_E_BADARG, "baseline needs weights and radii >= 0");
    if (a.iters < 1) return zk_fail(ZK_E_BADARG, "num_iters must be >= 1");
  }
  return 0;
}

int run_dev(int device, const args& a, const void* img, int dtype, int64_t H, int64_t W, int clip, void* bg, void* res, void* stream) {
  int rc = check_common(dtype, H, W, img, bg);
  if (rc || (rc = check_method(a))) return rc;
  ZK_ON_DEVICE(device);
  return run(a, img, dtype, (int)H, (int)W, clip, bg, res, (hipStream_t)stream);
}

int run_host(int device, const args& a, const void* img_host, int dtype, int64_t H, int64_t W, int clip, void* bg_host, void* res_host) {
  int rc = check_common(dtype, H, W, img_host, bg_host);
  if (rc || (rc = check_method(a))) return rc;
  ZK_ON_DEVICE(device);
  const size_t in_bytes = (size_t)H * W * zk_elem_size(dtype);
  const size_t out_bytes = a.method == M_BASELINE ? (size_t)H * W * 8 : in_bytes;
  dev_buf d_img, d_bg, d_res;                        // d_res stays null without a res_host
  if ((rc = d_img.upload(img_host, in_bytes)) || (rc = d_bg.alloc(out_bytes)) || (res_host && (rc = d_res.alloc(out_bytes)))) return rc;
  if ((rc = run(a, d_img.p, dtype, (int)H, (int)W, clip, d_bg.p, d_res.p, (hipStream_t)0)) || (rc = d_bg.download(bg_host, out_bytes)))
    return rc;
  return d_res.download(res_host, out_bytes);
}

args opening_args(int64_t size_y, int64_t size_x) {
  args a;
  a.method = M_OPENING;
  a.ky = (int)std::max<int64_t>(std::min<int64_t>(size_y, 1 << 30), 0);
  a.kx = (int)std::max<int64_t>(std::min<int64_t>(size_x, 1 << 30), 0);
  return a;
}

args rolling_ball_args(double radius) {
  args a;
  a.method = M_ROLLING_BALL;
  a.radius = radius;
  return a;
}

args baseline_args(const double* wy, int64_t ry, const double* wx, int64_t rx, int64_t iters) {
  args a;
  a.method = M_BASELINE;
  a.wy = wy;
  a.wx = wx;
  a.ry = (int)std::max<int64_t>(std::min<int64_t>(ry, 1 << 30), -1);
  a.rx = (int)std::max<int64_t>(std::min<int64_t>(rx, 1 << 30), -1);
  a.iters = (int)std::max<int64_t>(std::min<int64_t>(iters, 1 << 30), 0);
  return a;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_background_opening(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t size_y,
                                     int64_t size_x, int clip, void* background_host, void* residual_host) {
  return run_host(device, opening_args(size_y, size_x), image_host, dtype, height, width, clip, background_host, residual_host);
}

extern "C" int zk_background_opening_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t size_y,
                                         int64_t size_x, int clip, void* background_dev, void* residual_dev, void* hip_stream) {
  return run_dev(device, opening_args(size_y, size_x), image_dev, dtype, height, width, clip, background_dev, residual_dev, hip_stream);
}

extern "C" int zk_background_rolling_ball(int device, const void* image_host, int dtype, int64_t height, int64_t width, double radius,
                                          int clip, void* background_host, void* residual_host) {
  return run_host(device, rolling_ball_args(radius), image_host, dtype, height, width, clip, background_host, residual_host);
}

extern "C" int zk_background_rolling_ball_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width,
                                              double radius, int clip, void* background_dev, void* residual_dev, void* hip_stream) {
  return run_dev(device, rolling_ball_args(radius), image_dev, dtype, height, width, clip, background_dev, residual_dev, hip_stream);
}

extern "C" int zk_background_baseline(int device, const void* image_host, int dtype, int64_t height, int64_t width,
                                      const double* weights_y, int64_t radius_y, const double* weights_x, int64_t radius_x,
                                      int64_t num_iters, int clip, double* background_host, double* residual_host) {
  return run_host(device, baseline_args(weights_y, radius_y, weights_x, radius_x, num_iters), image_host, dtype, height, width, clip,
                  background_host, residual_host);
}

extern "C" int zk_background_baseline_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width,
                                          const double* weights_y, int64_t radius_y, const double* weights_x, int64_t radius_x,
                                          int64_t num_iters, int clip, double* background_dev, double* residual_dev, void* hip_stream) {
  return run_dev(device, baseline_args(weights_y, radius_y, weights_x, radius_x, num_iters), image_dev, dtype, height, width, clip,
                 background_dev, residual_dev, hip_stream);
}

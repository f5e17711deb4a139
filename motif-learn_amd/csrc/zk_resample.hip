// zk_resample.hip -- zk_scan_resample: every frame of a (Z, H, W) stack sampled at (y + dy[z, x], x + dx[z, y]) through its own
// B-spline interpolant of order 0, 1 or 3 (the reference's apply_scan_noise, denoise/_noise_models.py:28-57, frame by frame).
//
//   order 3   prefilter_rows_kernel   stack -> plane A: tiles of 64 rows x 56 columns (+ 32 on either side) cross LDS, one lane
//                                     per row walks its segment (zk_spline3_segment), loads and stores stay whole rows;
//             prefilter_cols_kernel   plane A -> plane B: one lane per column and 128-row segment, coalesced across lanes;
//   any order gather_kernel           one output per lane, lanes along x, (order + 1)^2 taps folded by the mode.
//
// A segment warms up over the extended signal, so it reads samples its neighbours own: the passes go from one plane to the
// next, never in place.  The two float64 planes (16 B per pixel) are the whole scratch; a stack that needs more than the budget
// goes in runs of whole frames, and since no kernel looks across frames the run length cannot show in the result.
// Nothing here is fused by the compiler (-ffp-contract=off, csrc/Makefile): the tap sums are the reference's expressions.
#include <algorithm>
#include <type_traits>

#include "zk_interp.h"
#include "zk_ring.h"
#include "zk_scratch.h"

namespace {

constexpr int ROW_TILE = 64;                                  // rows of a tile: one per lane of the wave that filters it
constexpr int ROW_SEG = 56;                                   // columns a tile produces
constexpr int ROW_SPAN = ROW_SEG + 2 * ZK_SPLINE_WARMUP;      // columns it holds
constexpr int ROW_PITCH = ROW_SPAN + 1;                       // odd: the lanes of the filter pass spread over the banks
constexpr int COL_SEG = 128;                                  // rows of a column segment
constexpr size_t DEFAULT_BUDGET = (size_t)256 << 20;          // input + output + scratch of one run

zk_device_bytes g_budget;  // zk_scan_resample_set_chunk; 0: DEFAULT_BUDGET

// ---------------------------------------------------------------------------------------------------------------------
// order 3: the prefilter
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void prefilter_rows_kernel(const T* __restrict__ in, double* __restrict__ out, int H, int W, int mode) {
  __shared__ double tile[ROW_TILE * ROW_PITCH];
  const int tid = threadIdx.x;
  const long long x0 = (long long)blockIdx.x * ROW_SEG, y0 = (long long)blockIdx.y * ROW_TILE;
  const long long frame = (long long)blockIdx.z * H * W;
  const int rows = (int)min((long long)ROW_TILE, H - y0), cols = (int)min((long long)ROW_SEG, W - x0);
  for (int e = tid; e < rows * ROW_SPAN; e += 256) {
    const int r = e / ROW_SPAN, k = e - r * ROW_SPAN;
    const long long x = zk_fold_index(x0 - ZK_SPLINE_WARMUP + k, W, mode);
    tile[r * ROW_PITCH + k] = ZK_SPLINE_GAIN * (double)in[frame + (y0 + r) * W + x];
  }
  __syncthreads();
  if (tid < rows) {
    double* line = tile + tid * ROW_PITCH + ZK_SPLINE_WARMUP;  // line[i]: column x0 + i
    zk_spline3_segment(
        0, cols, [&](long long i) { return line[i]; }, [&](long long i, double v) { line[i] = v; }, [&](long long i) { return line[i]; });
  }
  __syncthreads();
  for (int e = tid; e < rows * cols; e += 256) {
    const int r = e / cols, k = e - r * cols;
    out[frame + (y0 + r) * W + x0 + k] = tile[r * ROW_PITCH + ZK_SPLINE_WARMUP + k];
  }
}

__global__ __launch_bounds__(256) void prefilter_cols_kernel(const double* __restrict__ in, double* __restrict__ out, int H, int W, int mode) {
  const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  const long long a = (long long)blockIdx.y * COL_SEG, b = min((long long)H, a + COL_SEG);
  const double* src = in + (long long)blockIdx.z * H * W + x;
  double* dst = out + (long long)blockIdx.z * H * W + x;
  zk_spline3_segment(
      a, b, [&](long long i) { return ZK_SPLINE_GAIN * src[zk_fold_index(i, H, mode) * W]; }, [&](long long i, double v) { dst[i * W] = v; },
      [&](long long i) { return dst[i * W]; });
}

// ---------------------------------------------------------------------------------------------------------------------
// the gather
// ---------------------------------------------------------------------------------------------------------------------
// blockIdx.x = row * blocks_per_row + block of the row, blockIdx.y = frame.  The x shift is one number per row and the y shift
// one per lane; both coordinates are formed per lane as the float64 sums x + dx and y + dy, the reference's operands.
template <typename TSRC, typename TOUT, int ORDER>
__global__ __launch_bounds__(256) void gather_kernel(const TSRC* __restrict__ src, const double* __restrict__ dx, const double* __restrict__ dy,
                                                     TOUT* __restrict__ out, int H, int W, int blocks_per_row, int mode) {
  const long long y = blockIdx.x / blocks_per_row;
  const long long x = (long long)(blockIdx.x - y * blocks_per_row) * 256 + threadIdx.x;
  if (x >= W) return;
  const long long z = blockIdx.y;
  const double cx = (double)x + dx[z * H + y], cy = (double)y + dy[z * W + x];
  const TSRC* frame = src + z * H * W;
  TOUT* dst = out + (z * H + y) * W + x;
  if (mode == ZK_EXT_CONSTANT && (cx < 0.0 || cx > (double)(W - 1) || cy < 0.0 || cy > (double)(H - 1))) {
    *dst = (TOUT)0.0;
    return;
  }
  const double ux = zk_map_coordinate(cx, W, mode), uy = zk_map_coordinate(cy, H, mode);
  double wx[ORDER + 1], wy[ORDER + 1];
  const long long ix = zk_spline_taps(ux, ORDER, wx), iy = zk_spline_taps(uy, ORDER, wy);
  long long fx[ORDER + 1];
#pragma unroll
  for (int i = 0; i <= ORDER; ++i) fx[i] = zk_fold_index(ix + i, W, mode);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j <= ORDER; ++j) {
    const long long fy = zk_fold_index(iy + j, H, mode);
#pragma unroll
    for (int i = 0; i <= ORDER; ++i) {
      const double v = (fy < 0 || fx[i] < 0) ? 0.0 : (double)frame[fy * W + fx[i]];
      acc += v * wy[j] * wx[i];
    }
  }
  *dst = (TOUT)acc;
}

template <typename TSRC, typename TOUT>
int launch_gather(const TSRC* src, const double* dx, const double* dy, TOUT* out, int64_t nz, int H, int W, int order, int mode, hipStream_t s) {
  const int bpr = (int)blocks_of(W, 256);
  const dim3 grid((unsigned)((int64_t)bpr * H), (unsigned)nz);
  if (order == 0) hipLaunchKernelGGL((gather_kernel<TSRC, TOUT, 0>), grid, dim3(256), 0, s, src, dx, dy, out, H, W, bpr, mode);
  else if (order == 1) hipLaunchKernelGGL((gather_kernel<TSRC, TOUT, 1>), grid, dim3(256), 0, s, src, dx, dy, out, H, W, bpr, mode);
  else hipLaunchKernelGGL((gather_kernel<TSRC, TOUT, 3>), grid, dim3(256), 0, s, src, dx, dy, out, H, W, bpr, mode);
  ZK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct job {
  int dtype, order, mode;
  int64_t Z, H, W;
  size_t pixels() const { return (size_t)H * W; }
  size_t in_frame() const { return pixels() * zk_elem_size(dtype); }
  size_t out_frame() const { return pixels() * (dtype == ZK_F32 ? 4 : 8); }
  size_t scratch_frame() const { return order == 3 ? pixels() * 16 : 0; }
};

int check_job(const job& j, const void* stack, const void* dx, const void* dy, const void* out) {
  if (!zk_is_elem(j.dtype)) return zk_fail(ZK_E_BADARG, "scan_resample: dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (j.Z < 1 || j.H < 1 || j.W < 1) return zk_fail(ZK_E_BADARG, "scan_resample: Z, H and W must be positive");
  // grid.y of the row prefilter carries H / 64 and grid.x of the gather H * ceil(W / 256)
  if (j.H > ((int64_t)1 << 21) || j.W > ((int64_t)1 << 21) || j.Z >= ((int64_t)1 << 31) || j.Z * j.H * j.W >= ((int64_t)1 << 40) ||
      blocks_of(j.W, 256) * j.H >= ((int64_t)1 << 31))
    return zk_fail(ZK_E_BADARG, "scan_resample: needs H, W <= 2^21, H * ceil(W / 256) < 2^31, Z < 2^31 and fewer than 2^40 samples");
  if (j.order != 0 && j.order != 1 && j.order != 3) return zk_fail(ZK_E_BADARG, "scan_resample: order must be 0, 1 or 3");
  if (j.mode < ZK_RESAMPLE_REFLECT || j.mode > ZK_RESAMPLE_CONSTANT) return zk_fail(ZK_E_BADARG, "scan_resample: mode must be one of ZK_RESAMPLE_*");
  if (j.order == 3 && j.mode != ZK_RESAMPLE_REFLECT && j.mode != ZK_RESAMPLE_MIRROR && j.mode != ZK_RESAMPLE_GRID_WRAP)
    return zk_fail(ZK_E_BADARG, "scan_resample: order 3 takes ZK_RESAMPLE_REFLECT, ZK_RESAMPLE_MIRROR or ZK_RESAMPLE_GRID_WRAP");
  if (!stack || !dx || !dy || !out) return zk_fail(ZK_E_BADARG, "scan_resample: null pointer");
  return 0;
}

size_t budget_of(int device) { return g_budget.get(device, DEFAULT_BUDGET); }

// frames per run: what `bytes` holds at `unit` bytes a frame, at least one, at most the launch's grid.y
int64_t frames_per_run(size_t bytes, size_t unit, int64_t Z) {
  int64_t n = unit ? (int64_t)(bytes / unit) : Z;
  n = std::max<int64_t>(n, 1);
  return std::min<int64_t>(std::min<int64_t>(n, Z), 65535);
}

// nz frames, all operands on the device; scratch holds nz * 16 * H * W bytes at order 3
template <typename T, typename TOUT>
int run_frames(const job& j, const T* in, const double* dx, const double* dy, TOUT* out, int64_t nz, double* scratch, hipStream_t s) {
  const int H = (int)j.H, W = (int)j.W;
  if (j.order != 3) return launch_gather<T, TOUT>(in, dx, dy, out, nz, H, W, j.order, j.mode, s);
  double* a = scratch;
  double* b = scratch + (size_t)nz * j.pixels();
  hipLaunchKernelGGL(prefilter_rows_kernel<T>, dim3(blocks_of(W, ROW_SEG), blocks_of(H, ROW_TILE), (unsigned)nz), dim3(256), 0, s, in, a, H, W, j.mode);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(prefilter_cols_kernel, dim3(blocks_of(W, 256), blocks_of(H, COL_SEG), (unsigned)nz), dim3(256), 0, s, a, b, H, W, j.mode);
  ZK_HIP(hipGetLastError());
  return launch_gather<double, TOUT>(b, dx, dy, out, nz, H, W, 3, j.mode, s);
}

// the whole stack in runs of `per` frames
template <typename T, typename TOUT>
int run_typed(const job& j, const void* in_v, const double* dx, const double* dy, void* out_v, int64_t nz, int64_t per, double* scratch, hipStream_t s) {
  const T* in = (const T*)in_v;
  TOUT* out = (TOUT*)out_v;
  for (int64_t z0 = 0; z0 < nz; z0 += per) {
    const int64_t n = std::min<int64_t>(per, nz - z0);
    const int rc = run_frames<T, TOUT>(j, in + (size_t)z0 * j.pixels(), dx + z0 * j.H, dy + z0 * j.W, out + (size_t)z0 * j.pixels(), n, scratch, s);
    if (rc) return rc;
  }
  return 0;
}

int run_dev(const job& j, const void* in, const double* dx, const double* dy, void* out, int64_t nz, int64_t per, double* scratch, hipStream_t s) {
  return zk_with_elem(j.dtype, [&](auto e) {
    using T = typename decltype(e)::type;  // float32 comes back as float32, every other format as float64
    using TOUT = typename std::conditional<std::is_same<T, float>::value, float, double>::type;
    return run_typed<T, TOUT>(j, in, dx, dy, out, nz, per, scratch, s);
  });
}

zk_device_stage g_host[ZK_DEVICE_TABLE];  // the staging of the host entry point (zk_ring.h)

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_scan_resample_set_chunk(int device, int64_t budget_bytes) {
  return g_budget.set(device, budget_bytes, "bad arguments");
}

extern "C" int zk_scan_resample_dev(int device, const void* stack_dev, int dtype, int64_t Z, int64_t H, int64_t W, const double* dx_dev,
                                    const double* dy_dev, int order, int mode, void* out_dev, void* scratch_dev, int64_t scratch_bytes,
                                    void* hip_stream) {
  const job j{dtype, order, mode, Z, H, W};
  int rc = check_job(j, stack_dev, dx_dev, dy_dev, out_dev);
  if (rc) return rc;
  if (scratch_dev && (scratch_bytes < 0 || (size_t)scratch_bytes < j.scratch_frame()))
    return zk_fail(ZK_E_BADARG, "scan_resample: the scratch must hold one frame's two float64 planes (16 H W bytes at order 3)");
  if ((rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  hipStream_t s = (hipStream_t)hip_stream;
  if (order != 3 || scratch_dev) {  // nothing of the library's own to release: enqueued and left running
    const int64_t per = frames_per_run(scratch_dev ? (size_t)scratch_bytes : 0, j.scratch_frame(), Z);
    return run_dev(j, stack_dev, dx_dev, dy_dev, out_dev, Z, per, (double*)scratch_dev, s);
  }
  const int64_t per = frames_per_run(budget_of(device), j.scratch_frame(), Z);
  dev_buf scratch;
  if ((rc = scratch.alloc((size_t)per * j.scratch_frame())) || (rc = run_dev(j, stack_dev, dx_dev, dy_dev, out_dev, Z, per, scratch.as<double>(), s)))
    return rc;
  ZK_HIP(hipStreamSynchronize(s));  // the scratch is freed on return
  return 0;
}

extern "C" int zk_scan_resample(int device, const void* stack_host, int dtype, int64_t Z, int64_t H, int64_t W, const double* dx_host,
                                const double* dy_host, int order, int mode, void* out_host) {
  const job j{dtype, order, mode, Z, H, W};
  int rc = check_job(j, stack_host, dx_host, dy_host, out_host);
  if (rc || (rc = zk_check_device(device, ZK_DEVICE_TABLE))) return rc;
  ZK_ON_DEVICE(device);
  std::lock_guard<std::mutex> guard(g_host[device].lock);
  zk_stage* h = &g_host[device].stage;
  if ((rc = zk_stage_create(h))) return rc;
  zk_ring* r = &h->ring;
  const size_t in_unit = j.in_frame(), out_unit = j.out_frame();
  const zk_chunks ch = zk_chunk_plan(budget_of(device), in_unit + out_unit + j.scratch_frame(), 1, Z);
  const int64_t per = std::min<int64_t>(ch.chunk, 65535);  // frames of one launch
  dev_buf shifts, scratch;
  if ((rc = shifts.alloc((size_t)Z * (H + W) * 8)) || (order == 3 && (rc = scratch.alloc((size_t)per * j.scratch_frame())))) return rc;
  double* d_dx = shifts.as<double>();
  double* d_dy = d_dx + (size_t)Z * H;
  ZK_HIP(hipMemcpyAsync(d_dx, dx_host, (size_t)Z * H * 8, hipMemcpyHostToDevice, h->stream));
  ZK_HIP(hipMemcpyAsync(d_dy, dy_host, (size_t)Z * W * 8, hipMemcpyHostToDevice, h->stream));
  rc = zk_ring_run(
      r, h->stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, (size_t)ch.chunk * out_unit);
        if (!e) e = zk_ring_up(r, h->stream, c, slot, r->d_in[slot], (const char*)stack_host + (size_t)ch.first(c) * in_unit, (size_t)ch.count(c) * in_unit);
        return e ? e
                 : run_dev(j, r->d_in[slot], d_dx + ch.first(c) * H, d_dy + ch.first(c) * W, r->d_out[slot], ch.count(c), per, scratch.as<double>(),
                           h->stream);
      },
      [&](int64_t c, int slot) -> int { return zk_ring_down(r, slot, (char*)out_host + (size_t)ch.first(c) * out_unit, (size_t)ch.count(c) * out_unit); });
  zk_stage_trim(h, ZK_STAGE_KEEP_STACKS);
  return rc;  // zk_ring_run has drained every stream: shifts and scratch may go
}

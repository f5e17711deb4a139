// zk_utils.hip -- device side of mtflearn.utils (reference utils/_preprocessing_image.py, utils/_clip_image.py): the passes over
// the pixels of normalize_image / normalize_image_robust / standardize_image / percentile_clip / value_clip.  Everything
// scalar (np.isclose, eps, NumPy's percentile interpolation, the clip decision) stays with the caller.
//
// The image is flat: n elements of ZK_F32 / ZK_F64 / ZK_U8 / ZK_U16 / ZK_I16, each converted to float32 as it is read
// (round to nearest, ndarray.astype(np.float32)).
//
//   stats        min / max over the finite elements, the count of the others, and sum x, sum |x|, sum x^2 (or sum (x - c)^2)
//                over the finite ones in float64.  Every lane, then every workgroup, then one last workgroup adds its terms in
//                a fixed order, each partial sum carried as an unevaluated pair (two-sum), so the result is the correctly
//                rounded sum up to a few 2^-100 of sum |terms| and repeats bit for bit.  No floating-point atomics.
//   order stats  up to 16 ranks of the ascending sort, exact: radix select over the order-preserving uint32 image of the
//                float32 bits, four sweeps of eight bits.  A sweep counts, per distinct prefix still alive among the ranks (a
//                "slot"; an element matches at most one), the next digit of the matching elements: per-workgroup histograms in
//                LDS (slots x 256 counters, 16 KiB at most), merged into a global table with integer atomics, so the counts do
//                not depend on the order of arrival.  One small workgroup then walks each rank down its slot's counts and
//                rebuilds the slots.  Lanes of a wave that count the same bin are added as one (a constant frame, or the
//                handful of exponent bins a real frame fills in the first sweep, would otherwise serialise on one counter).
//                In deviation mode the sorted values are |x - c| in float32, never stored.
//   map          the elementwise passes: rescale and clip (float32, one operation at a time, nothing fused: NumPy's results
//                bit for bit), divide and standardise (float64 per element, rounded once).
#pragma clang fp contract(off)

#include <math.h>

#include <algorithm>
#include <type_traits>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

constexpr int MAX_RANKS = 16;
constexpr int SWEEP_BLOCKS = 1024;  // 4 workgroups per CU; a workgroup's share of a 2048^2 frame is 4096 elements

// Read-only sweep of p[0 .. n): f(value, have) once per element, 16 bytes per lane per request where the address allows (the
// fewer than two vectors of elements off the 16-byte grid at either end are read one by one).  Every lane of a wave makes the same
// number of calls, so f may use wave-wide operations: a lane past its last element calls with have = false.
template <typename T, typename F>
__device__ __forceinline__ void sweep(const T* __restrict__ p, long long n, F&& f) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec __attribute__((ext_vector_type(V)));
  long long head = (long long)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T));
  if (head > n) head = n;
  const long long nv = (n - head) / V;
  const int lane = threadIdx.x & 63;
  const long long wave0 = (long long)blockIdx.x * blockDim.x + threadIdx.x - lane, step = (long long)gridDim.x * blockDim.x;
  const vec* pv = (const vec*)(p + head);
  for (long long i0 = wave0; i0 < nv; i0 += step) {
    const long long i = i0 + lane;
    const bool have = i < nv;
    vec v = {};
    if (have) v = pv[i];
#pragma unroll
    for (int j = 0; j < V; ++j) f(v[j], have);
  }
  const long long tail0 = head + nv * V, loose = head + (n - tail0);
  for (long long i0 = wave0; i0 < loose; i0 += step) {
    const long long i = i0 + lane;
    const bool have = i < loose;
    f(have ? p[i < head ? i : tail0 + (i - head)] : T(0), have);
  }
}

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN
__device__ __forceinline__ bool finite_f64(double x) { return fabs(x) <= 1.7976931348623157e+308; }

// ---------------------------------------------------------------------------------------------------------------------
// stats
// ---------------------------------------------------------------------------------------------------------------------

// an unevaluated sum hi + lo, |lo| <= ulp(hi) / 2
struct dd {
  double hi, lo;
};

__device__ __forceinline__ void dd_add(dd& a, double x) {  // Knuth's two-sum, the error kept in lo
  const double s = a.hi + x;
  const double b = s - a.hi;
  const double e = (a.hi - (s - b)) + (x - b);
  a.hi = s;
  a.lo += e;
}

__device__ __forceinline__ dd dd_join(dd a, dd b) {
  const double s = a.hi + b.hi;
  const double t = s - a.hi;
  const double e = ((a.hi - (s - t)) + (b.hi - t)) + (a.lo + b.lo);
  dd r;
  r.hi = s + e;
  r.lo = e - (r.hi - s);
  return r;
}

struct stats_part {
  float mn, mx;
  unsigned long long nonfinite;
  dd s[3];
};

__device__ __forceinline__ stats_part stats_join(const stats_part& a, const stats_part& b) {
  stats_part r;
  r.mn = b.mn < a.mn ? b.mn : a.mn;
  r.mx = b.mx > a.mx ? b.mx : a.mx;
  r.nonfinite = a.nonfinite + b.nonfinite;
#pragma unroll
  for (int k = 0; k < 3; ++k) r.s[k] = dd_join(a.s[k], b.s[k]);
  return r;
}

__device__ __forceinline__ stats_part stats_shfl_down(const stats_part& a, int d) {
  stats_part r;
  r.mn = __shfl_down(a.mn, d);
  r.mx = __shfl_down(a.mx, d);
  r.nonfinite = __shfl_down(a.nonfinite, d);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.s[k].hi = __shfl_down(a.s[k].hi, d);
    r.s[k].lo = __shfl_down(a.s[k].lo, d);
  }
  return r;
}

// the workgroup's 256 parts, joined in a fixed tree (lanes by halving, then the four waves in order); valid in thread 0
__device__ __forceinline__ stats_part stats_block_join(stats_part v, stats_part* lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = stats_join(v, stats_shfl_down(v, d));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) v = stats_join(v, lds[w]);
  return v;
}

__device__ __forceinline__ stats_part stats_empty() {
  stats_part v;
  v.mn = INFINITY;
  v.mx = -INFINITY;
  v.nonfinite = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) v.s[k] = dd{0.0, 0.0};
  return v;
}

// CENTERED: s[0] = sum (x - c)^2 only.  WIDE (float64 images): the sums take the elements as they are, not narrowed to float32
// (what np.mean / np.std of a float64 image see); min / max are float32 either way, over the elements finite in float32.
template <typename T, bool CENTERED, bool WIDE>
__global__ __launch_bounds__(256) void stats_kernel(const T* __restrict__ img, long long n, double c, stats_part* __restrict__ parts) {
  __shared__ stats_part lds[4];
  stats_part v = stats_empty();
  sweep(img, n, [&](T raw, bool have) {
    if (!have) return;
    const float xf = (float)raw;
    const double x = WIDE ? (double)raw : (double)xf;
    if (!(WIDE ? finite_f64(x) : finite_f32(xf))) {
      ++v.nonfinite;
      return;
    }
    if (!WIDE || finite_f32(xf)) {  // a finite float64 past the float32 range is summed, and left out of the float32 min / max
      v.mn = xf < v.mn ? xf : v.mn;
      v.mx = xf > v.mx ? xf : v.mx;
    }
    if (CENTERED) {
      const double d = x - c;
      dd_add(v.s[0], d * d);
    } else {
      dd_add(v.s[0], x);
      dd_add(v.s[1], fabs(x));
      dd_add(v.s[2], x * x);
    }
  });
  v = stats_block_join(v, lds);
  if (threadIdx.x == 0) parts[blockIdx.x] = v;
}

struct stats_result {
  float mn, mx;
  long long nonfinite;
  double s[3];
};

__global__ __launch_bounds__(256) void stats_final_kernel(const stats_part* __restrict__ parts, int n_parts, stats_result* __restrict__ out) {
  __shared__ stats_part lds[4];
  stats_part v = stats_empty();
  for (int i = threadIdx.x; i < n_parts; i += 256) v = stats_join(v, parts[i]);
  v = stats_block_join(v, lds);
  if (threadIdx.x == 0) {
    out->mn = v.mn;
    out->mx = v.mx;
    out->nonfinite = (long long)v.nonfinite;
    for (int k = 0; k < 3; ++k) out->s[k] = v.s[k].hi;
  }
}

unsigned sweep_blocks(long long n, int dtype) {
  const long long per_block = 256LL * (16 / (long long)zk_elem_size(dtype));
  return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, SWEEP_BLOCKS));
}

template <typename T>
void launch_stats(const void* img, long long n, int mode, double c, stats_part* parts, unsigned blocks, hipStream_t s) {
  const bool centered = mode & ZK_STATS_CENTERED;
  if constexpr (std::is_same<T, double>::value) {
    if (mode & ZK_STATS_WIDE) {
      if (centered) hipLaunchKernelGGL((stats_kernel<T, true, true>), dim3(blocks), dim3(256), 0, s, (const T*)img, n, c, parts);
      else hipLaunchKernelGGL((stats_kernel<T, false, true>), dim3(blocks), dim3(256), 0, s, (const T*)img, n, c, parts);
      return;
    }
  }
  if (centered) hipLaunchKernelGGL((stats_kernel<T, true, false>), dim3(blocks), dim3(256), 0, s, (const T*)img, n, c, parts);
  else hipLaunchKernelGGL((stats_kernel<T, false, false>), dim3(blocks), dim3(256), 0, s, (const T*)img, n, c, parts);
}

int stats_run(const void* img, int dtype, long long n, int mode, double c, float* minmax, int64_t* n_nonfinite, double* sums,
              hipStream_t s) {
  const unsigned blocks = sweep_blocks(n, dtype);
  dev_buf d_parts, d_out;
  int rc;
  if ((rc = d_parts.alloc(blocks * sizeof(stats_part))) || (rc = d_out.alloc(sizeof(stats_result)))) return rc;
  stats_part* parts = d_parts.as<stats_part>();
  zk_with_elem(dtype, [&](auto e) { launch_stats<typename decltype(e)::type>(img, n, mode, c, parts, blocks, s); });
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(256), 0, s, parts, (int)blocks, d_out.as<stats_result>());
  ZK_HIP(hipGetLastError());
  stats_result r;
  ZK_HIP(hipMemcpyAsync(&r, d_out.p, sizeof(r), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  minmax[0] = r.mn;
  minmax[1] = r.mx;
  *n_nonfinite = r.nonfinite;
  for (int k = 0; k < 3; ++k) sums[k] = r.s[k];
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// order statistics
// ---------------------------------------------------------------------------------------------------------------------

// uint32 image of a float32 whose unsigned order is the float order (-0.0 just below +0.0), and back
__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct select_state {
  uint32_t hist[MAX_RANKS][256];  // counts of the running sweep, per slot; zero between sweeps
  uint32_t slot_prefix[MAX_RANKS];  // the digits fixed so far (the high 8 * sweep bits of the key) of each live slot
  int n_slots;
  int n_ranks;
  int slot_of[MAX_RANKS];           // per rank
  uint32_t prefix[MAX_RANKS];       // per rank: as slot_prefix
  uint32_t remaining[MAX_RANKS];    // per rank: its rank among the elements that share its prefix
};

__global__ __launch_bounds__(256) void select_init_kernel(select_state* __restrict__ st, const uint32_t* __restrict__ ranks, int n_ranks) {
  for (int i = threadIdx.x; i < MAX_RANKS * 256; i += 256) (&st->hist[0][0])[i] = 0;
  if (threadIdx.x < MAX_RANKS) {
    const int k = threadIdx.x;
    st->slot_of[k] = 0;
    st->prefix[k] = 0;
    st->remaining[k] = k < n_ranks ? ranks[k] : 0;
    st->slot_prefix[k] = 0;
  }
  if (threadIdx.x == 0) {
    st->n_slots = 1;
    st->n_ranks = n_ranks;
  }
}

// one count of `bin` per lane with `live` set; lanes of the wave on the same bin as its first live lane are added as one (twice)
__device__ __forceinline__ void count_bin(uint32_t* __restrict__ hist, bool live, uint32_t bin) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long m = __ballot(live);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t b = (uint32_t)__shfl((int)bin, leader);
    const bool same = live && bin == b;
    const unsigned long long sm = __ballot(same);
    if (lane == leader) atomicAdd(&hist[b], (uint32_t)__popcll(sm));
    live = live && !same;
  }
  if (live) atomicAdd(&hist[bin], 1u);
}

// sweep `pass` (0 .. 3): digit = bits [24 - 8 pass, 32 - 8 pass) of the key, counted under the slot whose prefix the higher bits equal
template <typename T, bool DEVIATION>
__global__ __launch_bounds__(256) void select_count_kernel(const T* __restrict__ img, long long n, float c, int pass,
                                                           select_state* __restrict__ st) {
  __shared__ uint32_t hist[MAX_RANKS * 256];
  __shared__ uint32_t slot_prefix[MAX_RANKS];
  const int n_slots = st->n_slots;
  for (int i = threadIdx.x; i < n_slots * 256; i += 256) hist[i] = 0;
  if (threadIdx.x < MAX_RANKS) slot_prefix[threadIdx.x] = threadIdx.x < n_slots ? st->slot_prefix[threadIdx.x] : 0xffffffffu;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  sweep(img, n, [&](T raw, bool have) {
    float x = (float)raw;
    if (DEVIATION) x = fabsf(x - c);
    const uint32_t key = key_of(x);
    const uint32_t high = pass ? key >> (shift + 8) : 0;
    int slot = -1;
    for (int k = 0; k < n_slots; ++k)
      if (slot_prefix[k] == high) slot = k;
    const bool live = have && slot >= 0;
    count_bin(hist, live, live ? (uint32_t)slot * 256 + ((key >> shift) & 255u) : 0);
  });
  __syncthreads();
  uint32_t* g = &st->hist[0][0];
  for (int i = threadIdx.x; i < n_slots * 256; i += 256)
    if (hist[i]) atomicAdd(&g[i], hist[i]);
}

// after a sweep: each rank steps down its slot's counts to its digit, then the slots are rebuilt from the distinct prefixes and
// the table is cleared for the next sweep
__global__ __launch_bounds__(256) void select_step_kernel(select_state* __restrict__ st, int pass, float* __restrict__ values) {
  const int n_ranks = st->n_ranks;
  if (threadIdx.x < n_ranks) {
    const int k = threadIdx.x;
    const uint32_t* h = st->hist[st->slot_of[k]];
    uint32_t rem = st->remaining[k];
    int d = 0;
    for (; d < 255 && rem >= h[d]; ++d) rem -= h[d];
    st->prefix[k] = (st->prefix[k] << 8) | (uint32_t)d;
    st->remaining[k] = rem;
    if (pass == 3) values[k] = value_of(st->prefix[k]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MAX_RANKS * 256; i += 256) (&st->hist[0][0])[i] = 0;
  if (threadIdx.x == 0) {
    int n_slots = 0;
    for (int k = 0; k < n_ranks; ++k) {
      int s = 0;
      while (s < n_slots && st->slot_prefix[s] != st->prefix[k]) ++s;
      if (s == n_slots) st->slot_prefix[n_slots++] = st->prefix[k];
      st->slot_of[k] = s;
    }
    st->n_slots = n_slots;
  }
}

template <typename T>
void launch_count(const void* img, long long n, int deviation, float c, int pass, select_state* st, unsigned blocks, hipStream_t s) {
  if (deviation) hipLaunchKernelGGL((select_count_kernel<T, true>), dim3(blocks), dim3(256), 0, s, (const T*)img, n, c, pass, st);
  else hipLaunchKernelGGL((select_count_kernel<T, false>), dim3(blocks), dim3(256), 0, s, (const T*)img, n, c, pass, st);
}

int order_stats_run(const void* img, int dtype, long long n, int mode, float c, const int64_t* ranks, int n_ranks, float* values,
                    hipStream_t s) {
  uint32_t r32[MAX_RANKS];
  for (int k = 0; k < n_ranks; ++k) r32[k] = (uint32_t)ranks[k];
  const unsigned blocks = sweep_blocks(n, dtype);
  dev_buf d_state, d_io;
  int rc;
  if ((rc = d_state.alloc(sizeof(select_state))) || (rc = d_io.alloc(MAX_RANKS * 8))) return rc;
  select_state* st = d_state.as<select_state>();
  uint32_t* d_ranks = d_io.as<uint32_t>();
  float* d_values = (float*)(d_ranks + MAX_RANKS);
  ZK_HIP(hipMemcpyAsync(d_ranks, r32, n_ranks * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(256), 0, s, st, d_ranks, n_ranks);
  ZK_HIP(hipGetLastError());
  for (int pass = 0; pass < 4; ++pass) {
    zk_with_elem(dtype, [&](auto e) { launch_count<typename decltype(e)::type>(img, n, mode, c, pass, st, blocks, s); });
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(select_step_kernel, dim3(1), dim3(256), 0, s, st, pass, d_values);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipMemcpyAsync(values, d_values, n_ranks * sizeof(float), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// elementwise
// ---------------------------------------------------------------------------------------------------------------------

struct map_params {
  float a, b, c, d;   // float32 operations
  double mean, std;   // standardise; mean is also the divisor of ZK_MAP_DIVIDE
};

// OP ZK_MAP_RESCALE      a + (x - b) * c / d       (vmin, x_min, span, scale)
//    ZK_MAP_DIVIDE       x / norm in float64 (norm = params[0] as given), rounded once to float32
//    ZK_MAP_CLIP         min(max(x, a), b) as np.clip orders it (NaN stays NaN; a > b gives b)
//    ZK_MAP_STANDARDIZE  (x - mean) / std in float64, x as stored, rounded once to TO
template <typename TI, typename TO, int OP>
__global__ __launch_bounds__(256) void map_kernel(const TI* __restrict__ img, TO* __restrict__ out, long long n, map_params p, int keep) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const TI raw = img[i];
    if constexpr (OP == ZK_MAP_STANDARDIZE) {
      const double x = (double)raw;
      const double d = x - p.mean;
      out[i] = (keep && !finite_f64(x)) ? (TO)x : (TO)(d / p.std);
    } else {
      const float x = (float)raw;
      float r;
      if constexpr (OP == ZK_MAP_RESCALE) {
        const float t0 = x - p.b;
        const float t1 = t0 * p.c;
        const float t2 = t1 / p.d;
        r = p.a + t2;
      } else if constexpr (OP == ZK_MAP_DIVIDE) {
        r = (float)((double)x / p.mean);
      } else {
        const float t = x < p.a ? p.a : x;
        r = t > p.b ? p.b : t;
      }
      out[i] = (keep && !finite_f32(x)) ? x : r;
    }
  }
}

template <typename TI, typename TO, int OP>
void launch_map_op(const void* img, void* out, long long n, const map_params& p, int keep, hipStream_t s) {
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 2048));
  hipLaunchKernelGGL((map_kernel<TI, TO, OP>), dim3(blocks), dim3(256), 0, s, (const TI*)img, (TO*)out, n, p, keep);
}

template <typename TI>
void launch_map(const void* img, void* out, long long n, int op, const map_params& p, int keep, hipStream_t s) {
  switch (op) {
    case ZK_MAP_RESCALE: launch_map_op<TI, float, ZK_MAP_RESCALE>(img, out, n, p, keep, s); break;
    case ZK_MAP_DIVIDE: launch_map_op<TI, float, ZK_MAP_DIVIDE>(img, out, n, p, keep, s); break;
    case ZK_MAP_CLIP: launch_map_op<TI, float, ZK_MAP_CLIP>(img, out, n, p, keep, s); break;
    default:
      if constexpr (std::is_same<TI, float>::value) launch_map_op<TI, float, ZK_MAP_STANDARDIZE>(img, out, n, p, keep, s);
      else launch_map_op<TI, double, ZK_MAP_STANDARDIZE>(img, out, n, p, keep, s);
  }
}

size_t map_out_size(int dtype, int op) { return (op == ZK_MAP_STANDARDIZE && dtype != ZK_F32) ? 8 : 4; }

int map_run(const void* img, int dtype, long long n, int op, const double* params, int keep, void* out, hipStream_t s) {
  map_params p;
  p.a = (float)params[0];
  p.b = (float)params[1];
  p.c = (float)params[2];
  p.d = (float)params[3];
  p.mean = params[0];
  p.std = params[1];
  zk_with_elem(dtype, [&](auto e) { launch_map<typename decltype(e)::type>(img, out, n, op, p, keep, s); });
  ZK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// checks and the host-buffer forms
// ---------------------------------------------------------------------------------------------------------------------

int check_image(const void* img, int dtype, int64_t n) {
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (n < 1 || n >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "bad element count (needs 1 <= n < 2^31)");
  if (!img) return zk_fail(ZK_E_BADARG, "null pointer");
  return 0;
}

int check_stats(int mode, const float* minmax, const int64_t* n_nonfinite, const double* sums) {
  if (mode & ~(ZK_STATS_CENTERED | ZK_STATS_WIDE)) return zk_fail(ZK_E_BADARG, "mode must be a combination of ZK_STATS_CENTERED and ZK_STATS_WIDE");
  if (!minmax || !n_nonfinite || !sums) return zk_fail(ZK_E_BADARG, "null pointer");
  return 0;
}

int check_order(int64_t n, int mode, const int64_t* ranks, int n_ranks, const float* values) {
  if (mode != ZK_ORDER_VALUES && mode != ZK_ORDER_DEVIATIONS) return zk_fail(ZK_E_BADARG, "mode must be ZK_ORDER_VALUES or ZK_ORDER_DEVIATIONS");
  if (n_ranks < 1 || n_ranks > MAX_RANKS) return zk_fail(ZK_E_BADARG, "needs 1 <= n_ranks <= 16");
  if (!ranks || !values) return zk_fail(ZK_E_BADARG, "null pointer");
  for (int k = 0; k < n_ranks; ++k)
    if (ranks[k] < 0 || ranks[k] >= n) return zk_fail(ZK_E_BADARG, "every rank must be in [0, n)");
  return 0;
}

int check_map(int op, const double* params, const void* out) {
  if (op < ZK_MAP_RESCALE || op > ZK_MAP_STANDARDIZE) return zk_fail(ZK_E_BADARG, "op must be one of ZK_MAP_*");
  if (!params || !out) return zk_fail(ZK_E_BADARG, "null pointer");
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_image_stats_dev(int device, const void* image_dev, int dtype, int64_t n, int mode, double center, float* minmax_host,
                                  int64_t* n_nonfinite_host, double* sums_host, void* hip_stream) {
  int rc = check_image(image_dev, dtype, n);
  if (rc || (rc = check_stats(mode, minmax_host, n_nonfinite_host, sums_host))) return rc;
  ZK_ON_DEVICE(device);
  return stats_run(image_dev, dtype, n, mode, center, minmax_host, n_nonfinite_host, sums_host, (hipStream_t)hip_stream);
}

extern "C" int zk_image_stats(int device, const void* image_host, int dtype, int64_t n, int mode, double center, float* minmax_host,
                              int64_t* n_nonfinite_host, double* sums_host) {
  int rc = check_image(image_host, dtype, n);
  if (rc || (rc = check_stats(mode, minmax_host, n_nonfinite_host, sums_host))) return rc;
  ZK_ON_DEVICE(device);
  dev_buf d_img;
  if ((rc = d_img.upload(image_host, (size_t)n * zk_elem_size(dtype)))) return rc;
  return stats_run(d_img.p, dtype, n, mode, center, minmax_host, n_nonfinite_host, sums_host, (hipStream_t)0);
}

extern "C" int zk_image_order_stats_dev(int device, const void* image_dev, int dtype, int64_t n, int mode, float center,
                                        const int64_t* ranks_host, int n_ranks, float* values_host, void* hip_stream) {
  int rc = check_image(image_dev, dtype, n);
  if (rc || (rc = check_order(n, mode, ranks_host, n_ranks, values_host))) return rc;
  ZK_ON_DEVICE(device);
  return order_stats_run(image_dev, dtype, n, mode, center, ranks_host, n_ranks, values_host, (hipStream_t)hip_stream);
}

extern "C" int zk_image_order_stats(int device, const void* image_host, int dtype, int64_t n, int mode, float center,
                                    const int64_t* ranks_host, int n_ranks, float* values_host) {
  int rc = check_image(image_host, dtype, n);
  if (rc || (rc = check_order(n, mode, ranks_host, n_ranks, values_host))) return rc;
  ZK_ON_DEVICE(device);
  dev_buf d_img;
  if ((rc = d_img.upload(image_host, (size_t)n * zk_elem_size(dtype)))) return rc;
  return order_stats_run(d_img.p, dtype, n, mode, center, ranks_host, n_ranks, values_host, (hipStream_t)0);
}

extern "C" int zk_image_map_dev(int device, const void* image_dev, int dtype, int64_t n, int op, const double* params_host,
                                int keep_nonfinite, void* out_dev, void* hip_stream) {
  int rc = check_image(image_dev, dtype, n);
  if (rc || (rc = check_map(op, params_host, out_dev))) return rc;
  ZK_ON_DEVICE(device);
  return map_run(image_dev, dtype, n, op, params_host, keep_nonfinite, out_dev, (hipStream_t)hip_stream);
}

extern "C" int zk_image_map(int device, const void* image_host, int dtype, int64_t n, int op, const double* params_host,
                            int keep_nonfinite, void* out_host) {
  int rc = check_image(image_host, dtype, n);
  if (rc || (rc = check_map(op, params_host, out_host))) return rc;
  ZK_ON_DEVICE(device);
  const size_t out_bytes = (size_t)n * map_out_size(dtype, op);
  dev_buf d_img, d_out;
  if ((rc = d_img.upload(image_host, (size_t)n * zk_elem_size(dtype))) || (rc = d_out.alloc(out_bytes))) return rc;
  if ((rc = map_run(d_img.p, dtype, n, op, params_host, keep_nonfinite, d_out.p, (hipStream_t)0))) return rc;
  return d_out.download(out_host, out_bytes);
}

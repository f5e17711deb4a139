// zk_peaks.hip -- device side of local_max (reference features/_local_max_v2.py): key-point detection ahead of
// zk_transform_points.
//
//   candidates   skimage.feature.peak_local_max(image, min_distance=1, threshold_abs=t): pixels equal to the maximum of
//                their 3 x 3 neighbourhood, strictly above t, off the 1-px border; none at all in a constant image
//   NaN          neither the reference nor scikit-image defines it; the rule here (tests/local_max_oracle.py restates it):
//                the minimum (the default threshold) and the constant-image test are taken over the non-NaN pixels, an image
//                with no non-NaN pixel has no candidates, a NaN pixel is never a candidate (v > t is false) and a NaN
//                neighbour never outranks a pixel (NaN > v is false): NaN acts as -inf in the 3 x 3 maximum, and only there
//   suppression  filter_peaks_by_distance: candidates visited in descending intensity, a kept one drops every other
//                candidate at Euclidean distance <= min_distance
//
// Pipeline (one call, every step on the device):
//   1. min / max of the image (one pass; the min is the default threshold, min == max is the constant-image rule)
//   2. candidate flags, compacted to a raster-ordered list of pixel indices (rocPRIM select)
//   3. stable radix sort of that list by descending value (rocPRIM radix_sort_pairs on order-preserving value bits):
//      the position in the sorted list is a candidate's PRIORITY, ties broken by raster order.  An int32 rank image
//      (-1 where there is no candidate) serves the neighbour look-ups.
//   4. suppression as a fixed point over priorities.  An undecided candidate becomes SUPPRESSED as soon as a
//      higher-priority candidate within r is KEPT, and KEPT once every higher-priority candidate within r is
//      SUPPRESSED; otherwise it waits.  By induction on priority every decision is the one the sequential loop makes,
//      and the highest-priority undecided candidate always resolves, so the iteration ends.  A workgroup iterates its
//      64 x 16 tile to a local fixed point in LDS (halo of r, read-only); launches repeat only for what waits on a
//      neighbouring tile.  Radii whose halo does not fit LDS take one global round per launch instead.
//   5. the KEPT candidates in priority order (rocPRIM select) -> (x, y) int32 pairs.
#include <math.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

// suppression states; SUPPRESSED / KEPT double as the 0 / 1 flags of the final selection
enum : uint8_t { PK_SUPPRESSED = 0, PK_KEPT = 1, PK_UNDECIDED = 2 };

constexpr int TILE_W = 64, TILE_H = 16, TILE_THREADS = 256;
constexpr size_t TILE_LDS_MAX = 60 * 1024;  // + 4 KiB of static LDS: within the 64 KiB of a workgroup
constexpr int ROUNDS_PER_CHECK = 4;  // suppression launches between two reads of the undecided counter

thread_local int64_t g_last_launches = 0;

// order-preserving unsigned images of the value bits (-0.0 folded onto +0.0, which compares equal to it)
__device__ __forceinline__ unsigned long long ordered64(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unordered64(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ unsigned int ordered32(float v) {
  const unsigned int b = __float_as_uint(v + 0.0f);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// mm[0] = ordered key of the minimum (initialised to all ones), mm[1] of the maximum (initialised to zero); NaN is skipped
template <typename T>
__global__ __launch_bounds__(256) void minmax_kernel(const T* __restrict__ img, long long n, unsigned long long* __restrict__ mm) {
  unsigned long long lo = ~0ull, hi = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double v = (double)img[i];
    if (v != v) continue;
    const unsigned long long k = ordered64(v);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long a = __shfl_down(lo, o), b = __shfl_down(hi, o);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    if (lo != ~0ull) atomicMin(&mm[0], lo);
    if (hi != 0ull) atomicMax(&mm[1], hi);
  }
}

// flag[i] = 1 for a candidate: interior pixel, no 3 x 3 neighbour greater, value > threshold, image not constant
template <typename T>
__global__ __launch_bounds__(256) void candidate_kernel(const T* __restrict__ img, int H, int W, const unsigned long long* __restrict__ mm,
                                                        int has_threshold, double threshold, uint8_t* __restrict__ flag) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long long i = (long long)y * W + x;
  uint8_t f = 0;
  const unsigned long long lo = mm[0], hi = mm[1];
  if (x >= 1 && x < W - 1 && y >= 1 && y < H - 1 && lo != ~0ull && lo != hi) {
    const double v = (double)img[i];
    const double t = has_threshold ? threshold : unordered64(lo);
    if (v > t) {
      bool top = true;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
          if ((double)img[i + (long long)dy * W + dx] > v) top = false;
      f = top ? 1 : 0;
    }
  }
  flag[i] = f;
}

// sort keys: ascending order of the key = descending value (float32-exact sources use the 32-bit float image)
template <typename T, typename K>
__global__ __launch_bounds__(256) void key_kernel(const T* __restrict__ img, const int32_t* __restrict__ pix, int n, K* __restrict__ key) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if constexpr (sizeof(K) == 8)
    key[j] = ~ordered64((double)img[pix[j]]);
  else
    key[j] = ~ordered32((float)img[pix[j]]);
}

__global__ __launch_bounds__(256) void rank_kernel(const int32_t* __restrict__ pix_sorted, int n, int32_t* __restrict__ rank_img,
                                                   uint8_t* __restrict__ state) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  rank_img[pix_sorted[k]] = k;
  state[k] = PK_UNDECIDED;
}

// One workgroup per TILE_W x TILE_H tile, iterated to a local fixed point in LDS.  LDS holds the rank and state of every
// pixel of the tile plus a halo of floor(r) (rank -1 off the image), and the disk offsets as linear LDS offsets.
// Halo states are a read-only snapshot: what waits on an undecided halo candidate waits for the next launch.
// States only ever go from UNDECIDED to a final value, so reading another tile's state mid-launch, old or new, is safe.
__global__ __launch_bounds__(TILE_THREADS) void suppress_tile_kernel(const int32_t* __restrict__ rank_img, int H, int W, int Rx, int Ry,
                                                                     const int32_t* __restrict__ offsets, int n_off,
                                                                     uint8_t* __restrict__ state, uint8_t* __restrict__ tile_done,
                                                                     unsigned int* __restrict__ undecided) {
  const int tiles_x = (W + TILE_W - 1) / TILE_W;
  const int tile = blockIdx.x;
  if (tile_done[tile]) return;
  const int tx0 = (tile % tiles_x) * TILE_W, ty0 = (tile / tiles_x) * TILE_H;
  const int LW = TILE_W + 2 * Rx, LH = TILE_H + 2 * Ry, cells = LW * LH;
  extern __shared__ int32_t lds[];
  int32_t* l_rank = lds;
  int32_t* l_off = lds + cells;
  volatile uint8_t* l_st = (volatile uint8_t*)(l_off + n_off);
  __shared__ int32_t own[TILE_W * TILE_H];
  __shared__ int n_own, changed, remaining;

  if (threadIdx.x == 0) {
    n_own = 0;
    remaining = 0;
  }
  for (int o = threadIdx.x; o < n_off; o += TILE_THREADS) l_off[o] = offsets[o];
  for (int c = threadIdx.x; c < cells; c += TILE_THREADS) {
    const int gy = ty0 - Ry + c / LW, gx = tx0 - Rx + c % LW;
    int32_t rk = -1;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) rk = rank_img[(long long)gy * W + gx];
    l_rank[c] = rk;
    l_st[c] = rk >= 0 ? state[rk] : PK_SUPPRESSED;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < TILE_W * TILE_H; t += TILE_THREADS) {
    const int i = t / TILE_W, j = t % TILE_W;
    if (ty0 + i >= H || tx0 + j >= W) continue;
    const int c = (Ry + i) * LW + Rx + j;
    if (l_rank[c] >= 0 && l_st[c] == PK_UNDECIDED) own[atomicAdd(&n_own, 1)] = c;
  }
  __syncthreads();
  const int n = n_own;
  if (n == 0) {
    if (threadIdx.x == 0) tile_done[tile] = 1;
    return;
  }
  do {
    __syncthreads();
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += TILE_THREADS) {
      const int c = own[e];
      if (l_st[c] != PK_UNDECIDED) continue;
      const int32_t rk = l_rank[c];
      bool waits = false, drop = false;
      for (int o = 0; o < n_off; ++o) {
        const int nc = c + l_off[o];
        const int32_t nr = l_rank[nc];
        if (nr >= 0 && nr < rk) {
          const uint8_t s = l_st[nc];
          if (s == PK_KEPT) {
            drop = true;
            break;
          }
          if (s == PK_UNDECIDED) waits = true;
        }
      }
      if (drop) {
        l_st[c] = PK_SUPPRESSED;
        changed = 1;
      } else if (!waits) {
        l_st[c] = PK_KEPT;
        changed = 1;
      }
    }
    __syncthreads();
  } while (changed);
  int left = 0;
  for (int e = threadIdx.x; e < n; e += TILE_THREADS) {
    const int c = own[e];
    const uint8_t s = l_st[c];
    if (s == PK_UNDECIDED) ++left;
    else state[l_rank[c]] = s;
  }
  if (left) atomicAdd(&remaining, left);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (remaining) atomicAdd(undecided, (unsigned int)remaining);
    else tile_done[tile] = 1;
  }
}

// Radii whose halo does not fit LDS: one global round per launch, one thread per undecided candidate.
__global__ __launch_bounds__(256) void suppress_global_kernel(const int32_t* __restrict__ rank_img, const int32_t* __restrict__ pix_sorted,
                                                              int n, int H, int W, const int2* __restrict__ offsets, int n_off,
                                                              uint8_t* state, unsigned int* __restrict__ undecided) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  volatile uint8_t* st = state;
  if (st[k] != PK_UNDECIDED) return;
  const int p = pix_sorted[k], y = p / W, x = p % W;
  bool waits = false, drop = false;
  for (int o = 0; o < n_off; ++o) {
    const int gx = x + offsets[o].x, gy = y + offsets[o].y;
    if (gx < 0 || gx >= W || gy < 0 || gy >= H) continue;
    const int32_t nr = rank_img[(long long)gy * W + gx];
    if (nr >= 0 && nr < k) {
      const uint8_t s = st[nr];
      if (s == PK_KEPT) {
        drop = true;
        break;
      }
      if (s == PK_UNDECIDED) waits = true;
    }
  }
  if (drop) st[k] = PK_SUPPRESSED;
  else if (!waits) st[k] = PK_KEPT;
  else atomicAdd(undecided, 1u);
}

__global__ __launch_bounds__(256) void points_kernel(const int32_t* __restrict__ kept_pix, int n, int W, int32_t* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int p = kept_pix[j];
  out[2 * j] = p % W;
  out[2 * j + 1] = p / W;
}

template <typename T>
int launch_front(const void* img, int H, int W, unsigned long long* mm, int has_threshold, double threshold, uint8_t* flag,
                 hipStream_t s) {
  const long long n = (long long)H * W;
  ZK_HIP(hipMemsetAsync(mm, 0xff, 8, s));
  ZK_HIP(hipMemsetAsync(mm + 1, 0, 8, s));
  hipLaunchKernelGGL(minmax_kernel<T>, dim3(std::min<unsigned>(blocks_of(n), 1024)), dim3(256), 0, s, (const T*)img, n, mm);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(candidate_kernel<T>, dim3(blocks_of(W, 64), blocks_of(H, 4)), dim3(256), 0, s, (const T*)img, H, W,
                     (const unsigned long long*)mm, has_threshold, threshold, flag);
  ZK_HIP(hipGetLastError());
  return 0;
}

// stable sort of the raster-ordered candidate list by descending value -> pix_sorted
template <typename T, typename K>
int sort_candidates(const void* img, const int32_t* pix, int n, int32_t* pix_sorted, void* keys, void* temp, size_t temp_bytes,
                    hipStream_t s) {
  K* k_in = (K*)keys;
  K* k_out = k_in + n;
  hipLaunchKernelGGL((key_kernel<T, K>), dim3(blocks_of(n)), dim3(256), 0, s, (const T*)img, pix, n, k_in);
  ZK_HIP(hipGetLastError());
  size_t bytes = temp_bytes;
  ZK_HIP(rocprim::radix_sort_pairs(temp, bytes, k_in, k_out, pix, pix_sorted, n, 0, 8 * (unsigned)sizeof(K), s));
  return 0;
}

template <typename K>
size_t sort_temp_bytes(int n) {
  size_t bytes = 0;
  (void)zk_prim_bytes(&bytes, [&](void* p, size_t& b) {
    return rocprim::radix_sort_pairs(p, b, (K*)nullptr, (K*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, n, 0, 8 * (unsigned)sizeof(K),
                                     (hipStream_t)0);
  });
  return bytes;
}

// The whole pipeline on a resident image.  Writes min(n, capacity) (x, y) int32 rows to points_dev, n to *n_found.
int local_max_core(const void* img, int dtype, int H, int W, double r, int has_threshold, double threshold, int32_t* points_dev,
                   int64_t capacity, int64_t* n_found, hipStream_t s) {
  g_last_launches = 0;
  const long long npx = (long long)H * W;
  dev_buf d_mm, d_flag, d_count;
  temp_store tmp;
  int rc;
  if ((rc = d_mm.alloc(16)) || (rc = d_flag.alloc((size_t)npx)) || (rc = d_count.alloc(8))) return rc;
  rc = zk_with_elem(dtype, [&](auto e) {
    return launch_front<typename decltype(e)::type>(img, H, W, d_mm.as<unsigned long long>(), has_threshold, threshold, d_flag.as<uint8_t>(), s);
  });
  if (rc) return rc;

  // raster-ordered candidate list (the count crosses to the host: it sizes everything after)
  dev_buf d_pix;
  if ((rc = d_pix.alloc((size_t)npx * 4))) return rc;
  if ((rc = zk_prim(tmp, [&](void* p, size_t& b) {
         return rocprim::select(p, b, rocprim::counting_iterator<int32_t>(0), d_flag.as<uint8_t>(), d_pix.as<int32_t>(),
                                d_count.as<unsigned int>(), (size_t)npx, s);
       })))
    return rc;
  unsigned int n_cand = 0;
  ZK_HIP(hipMemcpyAsync(&n_cand, d_count.p, 4, hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  *n_found = 0;
  if (n_cand == 0) return 0;
  const int n = (int)n_cand;

  // priorities
  const bool wide = dtype == ZK_F64;
  const size_t key_size = wide ? 8 : 4;
  dev_buf d_keys, d_sorted, d_rank, d_state, d_temp2;
  const size_t sort_bytes = wide ? sort_temp_bytes<unsigned long long>(n) : sort_temp_bytes<unsigned int>(n);
  // the kept candidates in priority order (run after the suppression); one allocation serves the sort and this select
  const auto select_kept = [&](void* p, size_t& b) {
    return rocprim::select(p, b, d_sorted.as<int32_t>(), d_state.as<uint8_t>(), d_pix.as<int32_t>(), d_count.as<unsigned int>(), (size_t)n, s);
  };
  size_t kept_bytes = 0;
  if ((rc = zk_prim_bytes(&kept_bytes, select_kept))) return rc;
  size_t temp2_bytes = std::max(sort_bytes, kept_bytes);
  if ((rc = d_keys.alloc((size_t)n * 2 * key_size)) || (rc = d_sorted.alloc((size_t)n * 4)) || (rc = d_rank.alloc((size_t)npx * 4)) ||
      (rc = d_state.alloc((size_t)n)) || (rc = d_temp2.alloc(temp2_bytes)))
    return rc;
  rc = zk_with_elem(dtype, [&](auto e) {
    using T = typename decltype(e)::type;  // float64 pixels sort by 64-bit keys, every other format by 32-bit ones (key_size above)
    using K = typename std::conditional<std::is_same<T, double>::value, unsigned long long, unsigned int>::type;
    return sort_candidates<T, K>(img, d_pix.as<int32_t>(), n, d_sorted.as<int32_t>(), d_keys.p, d_temp2.p, sort_bytes, s);
  });
  if (rc) return rc;
  ZK_HIP(hipMemsetAsync(d_rank.p, 0xff, (size_t)npx * 4, s));
  hipLaunchKernelGGL(rank_kernel, dim3(blocks_of(n)), dim3(256), 0, s, d_sorted.as<int32_t>(), n, d_rank.as<int32_t>(), d_state.as<uint8_t>());
  ZK_HIP(hipGetLastError());

  // disk offsets dx^2 + dy^2 <= r^2 (the point itself excluded), as the reference's inclusive ball query
  // (offsets longer than the image is wide / tall never meet a pixel: the scan stops at the image's extent)
  const int Rx = (int)std::min<double>(floor(r), (double)(W - 1)), Ry = (int)std::min<double>(floor(r), (double)(H - 1));
  const double r2 = r * r;
  const int LW = TILE_W + 2 * Rx, LH = TILE_H + 2 * Ry;
  std::vector<int2> off2;
  std::vector<int32_t> off_lin;
  for (long long dy = -Ry; dy <= Ry; ++dy)
    for (long long dx = -Rx; dx <= Rx; ++dx)
      if ((dx || dy) && (double)(dx * dx + dy * dy) <= r2) {
        off2.push_back(make_int2((int)dx, (int)dy));
        off_lin.push_back((int32_t)(dy * LW + dx));
      }
  const int n_off = (int)off2.size();
  const size_t tile_lds = (size_t)LW * LH * 5 + (size_t)n_off * 4;
  const bool tiled = tile_lds <= TILE_LDS_MAX;
  const int tiles = blocks_of(W, TILE_W) * blocks_of(H, TILE_H);
  constexpr int N_COUNTERS = ROUNDS_PER_CHECK;
  dev_buf d_off, d_done, d_undecided;
  if ((rc = d_off.alloc((size_t)std::max(n_off, 1) * 8)) || (rc = d_done.alloc((size_t)tiles)) ||
      (rc = d_undecided.alloc(N_COUNTERS * 4)))
    return rc;
  if (n_off) {
    if (tiled) ZK_HIP(hipMemcpyAsync(d_off.p, off_lin.data(), (size_t)n_off * 4, hipMemcpyHostToDevice, s));
    else ZK_HIP(hipMemcpyAsync(d_off.p, off2.data(), (size_t)n_off * 8, hipMemcpyHostToDevice, s));
  }
  ZK_HIP(hipMemsetAsync(d_done.p, 0, (size_t)tiles, s));
  // every launch resolves at least the highest-priority undecided candidate: n launches bound the loop
  for (long long launch = 0;;) {
    for (int c = 0; c < N_COUNTERS; ++c, ++launch) {
      unsigned int* counter = d_undecided.as<unsigned int>() + c;
      ZK_HIP(hipMemsetAsync(counter, 0, 4, s));
      if (tiled)
        hipLaunchKernelGGL(suppress_tile_kernel, dim3(tiles), dim3(TILE_THREADS), tile_lds, s, d_rank.as<int32_t>(), H, W, Rx, Ry,
                           d_off.as<int32_t>(), n_off, d_state.as<uint8_t>(), d_done.as<uint8_t>(), counter);
      else
        hipLaunchKernelGGL(suppress_global_kernel, dim3(blocks_of(n)), dim3(256), 0, s, d_rank.as<int32_t>(), d_sorted.as<int32_t>(),
                           n, H, W, d_off.as<int2>(), n_off, d_state.as<uint8_t>(), counter);
      ZK_HIP(hipGetLastError());
    }
    unsigned int left = 0;
    ZK_HIP(hipMemcpyAsync(&left, d_undecided.as<unsigned int>() + N_COUNTERS - 1, 4, hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    g_last_launches = launch;
    if (left == 0) break;
    if (launch > (long long)n + N_COUNTERS) return zk_fail(ZK_E_BADARG, "local_max: suppression made no progress");
  }

  ZK_HIP(select_kept(d_temp2.p, temp2_bytes));
  unsigned int n_kept = 0;
  ZK_HIP(hipMemcpyAsync(&n_kept, d_count.p, 4, hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  *n_found = n_kept;
  const int64_t n_out = std::min<int64_t>(n_kept, capacity);
  if (n_out > 0 && points_dev) {
    hipLaunchKernelGGL(points_kernel, dim3(blocks_of(n_out)), dim3(256), 0, s, d_pix.as<int32_t>(), (int)n_out, W, points_dev);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(s));
  return 0;
}

int check_args(int dtype, int64_t H, int64_t W, const void* img, double r, int64_t capacity, const void* out, const int64_t* n_found) {
  if (!zk_is_elem(dtype)) return zk_fail(ZK_E_BADARG, "dtype must be one of ZK_F32, ZK_F64, ZK_U8, ZK_U16, ZK_I16");
  if (H <= 0 || W <= 0 || H * W >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "bad image shape (needs 0 < height * width < 2^31)");
  if (!img || !n_found) return zk_fail(ZK_E_BADARG, "null pointer");
  if (!(r >= 0.0) || !isfinite(r)) return zk_fail(ZK_E_BADARG, "min_distance must be a finite number >= 0");
  if (capacity < 0 || (capacity > 0 && !out)) return zk_fail(ZK_E_BADARG, "capacity > 0 needs an output array");
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_local_max_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, double min_distance,
                                int has_threshold, double threshold, int32_t* points_dev, int64_t capacity, int64_t* n_found_host,
                                void* hip_stream) {
  int rc = check_args(dtype, height, width, image_dev, min_distance, capacity, points_dev, n_found_host);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  return local_max_core(image_dev, dtype, (int)height, (int)width, min_distance, has_threshold, threshold, points_dev, capacity,
                        n_found_host, (hipStream_t)hip_stream);
}

extern "C" int zk_local_max(int device, const void* image_host, int dtype, int64_t height, int64_t width, double min_distance,
                            int has_threshold, double threshold, int64_t* points_host, int64_t capacity, int64_t* n_found) {
  int rc = check_args(dtype, height, width, image_host, min_distance, capacity, points_host, n_found);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  const size_t img_bytes = (size_t)height * width * zk_elem_size(dtype);
  dev_buf d_img, d_pts;
  if ((rc = d_img.upload(image_host, img_bytes)) || (rc = d_pts.alloc((size_t)std::max<int64_t>(capacity, 1) * 8))) return rc;
  if ((rc = local_max_core(d_img.p, dtype, (int)height, (int)width, min_distance, has_threshold, threshold, d_pts.as<int32_t>(),
                           capacity, n_found, (hipStream_t)0)))
    return rc;
  const int64_t n_out = std::min(*n_found, capacity);
  if (n_out > 0) {
    std::vector<int32_t> pts((size_t)n_out * 2);
    if ((rc = d_pts.download(pts.data(), pts.size() * 4))) return rc;   // the points found, widened to int64 below
    for (size_t i = 0; i < pts.size(); ++i) points_host[i] = pts[i];
  }
  return 0;
}

extern "C" int64_t zk_local_max_last_launches(void) { return g_last_launches; }

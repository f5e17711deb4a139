// zk_rows.h -- the resident (N, D) float64 moment matrix and what its consumers share (not part of the public ABI):
// the container, the tile loader of the row kernels, and the host helpers of a pass (defined in zk_rows.hip).  Included by
// zk_rows.hip (container, column statistics), zk_kmeans.hip, zk_mixture.hip and zk_graph.hip.
//
// Common shape of the row kernels: a workgroup is ONE wave that owns tiles of 64 consecutive rows.  A tile is 64*D
// contiguous doubles = 32*D granules of 16 B: the LDS-DMA engine copies it as it lies (global_load_lds_dwordx4, 1 KiB per
// instruction, no VGPRs) into one of the wave's two LDS buffers while the wave computes on the other (tile_pipe).  Then
// lane r walks row r (stride D doubles: conflict-free for odd D, i.e. for n_max 8 / 12 moment matrices) while everything
// that is not a matrix element -- centre coordinates, Cholesky factors, column means -- is wave-uniform and arrives through
// scalar loads (as in the moment kernels).  Column sums per cluster are built the other way round (lane = column, the row's label wave-uniform) with
// LDS floating-point adds into a wave-private table.  Per-workgroup partial results are written out and summed by a second
// kernel in a fixed order: results do not depend on scheduling (bit-identical from run to run on the same device).
#pragma once

#include "zk_internal.h"
#include "zk_fold.h"  // ZK_CONST / zk_const

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>

struct zk_rows {
  int device = 0;
  int n_cu = 256;
  int64_t N = 0;
  int D = 0;
  const double* X = nullptr;
  bool own = false;
  hipStream_t stream = nullptr;
  double* d_mean = nullptr;      // [D] the centring shift (column means; zeros until zk_rows_center)
  double* d_xsq = nullptr;       // [N] squared norms of the centred rows
  void* d_tab = nullptr;         // wave-uniform operand tables of the current call
  size_t tab_bytes = 0;
  void* d_part = nullptr;        // per-workgroup partial results
  size_t part_bytes = 0;
  void* d_red = nullptr;         // reduced results
  size_t red_bytes = 0;
  void* d_seed[2] = {nullptr, nullptr};  // k-means++: (t, N) candidate distance rows, ping-pong
  size_t seed_bytes[2] = {0, 0};
  int seed_cur = 0;              // buffer that holds the current closest-distance row
  const double* d_closest = nullptr;
  int seed_t = 0;                // candidates of the last zk_kmeans_seed_step ...
  int seed_last = -1;            // ... and the buffer their distance rows are in
  int32_t* d_labels = nullptr;   // [N]
  void* d_resp = nullptr;        // (k, N) responsibilities
  size_t resp_bytes = 0;
  unsigned long long* d_count = nullptr;  // [4] integer counters
  std::vector<double> h_buf;
  void* h_pin = nullptr;         // page-locked staging of the operand tables (up) and the reduced results (down)
  size_t pin_bytes = 0;
  hipEvent_t ev_up = nullptr;    // the last table upload has left the staging buffer
  void* h_res = nullptr;         // page-locked landing area of the reduced results (+ 8 bytes for a counter)
  size_t res_bytes = 0;
  bool profile = false;          // HIP events around the main kernel of zk_kmeans_step / zk_gmm_estep / zk_gmm_moments
  hipEvent_t ev[2] = {nullptr, nullptr};
  double last_kernel_ms = 0.0;
};

constexpr int TILE = 64;

#define ZK_GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define ZK_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// The wave's stream of tiles t = blockIdx.x, + gridDim.x, ...: acquire() returns tile t in LDS (row r at [r * D]) once its
// DMA has landed and puts the DMA of the next tile in flight into the other buffer; advance() moves on.  Only tiles that lie
// wholly inside the matrix are moved by DMA (whole 16-B granules); the ragged last tile is copied with ordinary loads, rows
// past the end as zeros.
struct tile_pipe {
  const double* X;
  long long N, t, step;
  int D, lane, cur, nbuf;
  double* buf;
  // nbuf = 2: the next tile's DMA flies under this tile's arithmetic; 1: half the LDS, more waves per CU (kernels whose
  // arithmetic, not the stream, sets the pace)
  __device__ __forceinline__ tile_pipe(const double* X_, long long N_, int D_, double* lds, int lane_, int nbuf_ = 2)
      : X(X_), N(N_), t(blockIdx.x), step(gridDim.x), D(D_), lane(lane_), cur(0), nbuf(nbuf_), buf(lds) {
    if (nbuf == 2 && live()) issue(t, buf);
  }
  __device__ __forceinline__ bool live() const { return t * TILE < N; }
  __device__ __forceinline__ int rows() const { return (int)(N - t * TILE < TILE ? N - t * TILE : TILE); }
  __device__ __forceinline__ void issue(long long tt, double* dst) {
    if ((tt + 1) * TILE > N) return;
    const char* src = (const char*)(X + tt * TILE * D);
    const int n_gran = 32 * D;
    for (int q = 0; q * 64 < n_gran; ++q) {
      const int g = q * 64 + lane;
      if (g < n_gran) __builtin_amdgcn_global_load_lds(ZK_GLOBAL_PTR(src + (long long)g * 16), ZK_LDS_PTR((char*)dst + q * 1024), 16, 0, 2);
    }
  }
  __device__ __forceinline__ const double* acquire() {
    double* now = buf + cur * TILE * D;
    if (nbuf == 1) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the buffer is no longer read
      issue(t, now);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // tile t has landed; the other buffer is no longer read
    if ((t + 1) * TILE > N) {
      const long long base = t * TILE * D, total = N * D;
#pragma unroll 8
      for (int q = 0; q < D; ++q) {
        const long long e = base + (long long)q * TILE + lane;
        now[q * TILE + lane] = e < total ? X[e] : 0.0;
      }
      __syncthreads();
    }
    const long long nt = t + step;
    if (nbuf == 2 && nt * TILE < N) issue(nt, buf + (cur ^ 1) * TILE * D);
    return now;
  }
  __device__ __forceinline__ void advance() {
    t += step;
    if (nbuf == 2) cur ^= 1;
  }
};

// v of the lane a DPP control names (quad_perm / row mirrors: lanes of the same row of 16), for a double
template <int CTRL>
__device__ __forceinline__ double zk_dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- host helpers of a pass (zk_rows.hip) --------------------------------------------------------------------------
// the operand tables of a pass, built in m->h_buf: uploaded asynchronously, ordered before the pass's kernels on the matrix's
// stream; h_buf is left empty
int zk_upload_tab(zk_rows* m);
// fixed-order sum of the per-workgroup partial results ([n_blocks][n] in d_part) -> host, with d_count[0] when asked for;
// synchronises the stream
int zk_reduce_to_host(zk_rows* m, int n_blocks, int n, double* host_out, unsigned long long* counter_out = nullptr);
// HIP events around the main kernel of a pass while zk_rows_profile is on; zk_rows_prof_read after the stream has been synchronised
int zk_rows_prof_begin(zk_rows* m);
int zk_rows_prof_end(zk_rows* m);
int zk_rows_prof_read(zk_rows* m);
// the label array, allocated on first use; `unset`: a new one starts at -1, as sklearn's labels_old (a pass that counts changes)
int zk_rows_need_labels(zk_rows* m, bool unset);
int zk_check_lds(size_t bytes);  // refuses more than a CU's 160 KiB

// A single-wave row pass: tile buffers (one or two), LDS bytes (tiles + `extra_lds`) and the persistent grid.
struct zk_row_plan {
  int nbuf = 0;
  size_t lds = 0;
  int grid = 0;
};
int zk_plan_row_pass(const zk_rows* m, size_t extra_lds, zk_row_plan* p);

template <typename K>
int zk_allow_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024) ZK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}

// raise the kernel's LDS limit where needed, launch, collect the launch error
template <typename K, typename... A>
int zk_launch_lds(K kernel, const zk_rows* m, dim3 grid, dim3 block, size_t lds, A... args) {
  const int rc = zk_allow_lds(kernel, lds);
  if (rc) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, m->stream, args...);
  ZK_HIP(hipGetLastError());
  return 0;
}

// the same between the profile events: the main kernel of a pass
template <typename K, typename... A>
int zk_launch_profiled(K kernel, zk_rows* m, dim3 grid, dim3 block, size_t lds, A... args) {
  int rc = zk_rows_prof_begin(m);
  if (rc || (rc = zk_launch_lds(kernel, m, grid, block, lds, args...))) return rc;
  return zk_rows_prof_end(m);
}

// the same for a planned single-wave row kernel: every one of them starts with (X, N, D, nbuf)
template <typename K, typename... A>
int zk_launch_row_pass(K kernel, const zk_rows* m, const zk_row_plan& p, A... args) {
  return zk_launch_lds(kernel, m, dim3(p.grid), dim3(64), p.lds, m->X, (long long)m->N, m->D, p.nbuf, args...);
}

// f(std::integral_constant<int, V>) for the V among Vs that equals v: picks the template instance a run-time size asks for
template <int... Vs, class F>
int zk_with_int(int v, F f) {
  int rc = 0;
  const bool found = ((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return found ? rc : zk_fail(ZK_E_BADARG, "no kernel instance for this size");
}

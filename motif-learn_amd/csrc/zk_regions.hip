// zk_regions.hip -- device side of mtflearn.graph: the faces ("regions") of a planar lattice graph, what the reference's
// graph/find_regions.py walks wedge by wedge on the host.  Points (N, 2) float64 and directed edges (E, 2) int64 go in;
// the polygons (CSR offsets + vertices), their sizes and centres and the graph of neighbouring polygons come out.
//
// Everything is one lane per directed edge or per wedge, integers all the way except the angles and the centres:
//
//   grown edge   i0 = first argmin of x; node N at (x_i0 - 1, y_i0) with the edges (i0, N) and (N, i0).  It dangles in the
//                outer face, so that face dies at it.
//   edge sort    keys (i << 32) | j, radix-sorted (rocPRIM, as zk_peaks.hip sorts its candidates) and deduplicated; the
//                CSR row starts are lower bounds of (i << 32) in the unique keys.
//   angles       theta = fmod(atan2(dy, dx) + 2 pi, 2 pi) per edge in float64; each lane counts the entries of its own row
//                that order before it by (theta, j), which is its slot in the row: no cap on the degree.
//   wedges       row (js[t - 1], i, js[t]) per slot of a row with d >= 2 neighbours, (js[0], -1, js[0]) for d == 1 and
//                (i, -1, -1) for d == 0; keys (col0 << 32) | (col1 + 1) with col2 as payload, radix-sorted.  The array has
//                M + N + 1 entries (M unique edges, one possible isolated row per node); unused entries carry an all-ones
//                key, sort to the end and are dead ends.
//   successor    of (a, b, c), b != -1: the row with key (b, c), by binary search; none = dead end.  The map is injective,
//                so the wedges fall into simple paths (no polygon) and cycles (one polygon each).
//   labelling    pointer doubling in ping-pong buffers: after ceil(log2 W) rounds a wedge whose pointer never met a dead end
//                lies on a cycle, and it carries the smallest wedge index of that cycle.
//   ranking      the cycle is cut in front of its smallest wedge and the distance to the cut is doubled the same way;
//                the smallest wedge's own distance is the cycle's length k, the others sit at k - distance.
//   compaction   exclusive scans number the cycle minima ascending (the reference's polygon order), turn the lengths into
//                offsets and number the adjacency pairs; col0 of every cycle wedge lands at offsets[face] + rank.
//   centres      one lane per face adds its vertices' coordinates in vertex order and divides by k: what
//                nodes[region].mean(axis=0) does, bit for bit.
//   adjacency    a wedge (a, b, .) is the half-edge a -> b of its face; for a < b with both half-edges on cycles the pair
//                (face of a -> b, face of b -> a) is emitted, in ascending wedge order.
//
// Only integer atomics (one error flag); two runs agree byte for byte.
#pragma clang fp contract(off)

#include <math.h>

#include <algorithm>
#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "zk_internal.h"
#include "zk_scratch.h"

namespace {

typedef unsigned long long u64;

constexpr u64 PAD_KEY = ~0ull;                       // unused wedge slots and rejected edges: sorts last, matches nothing
constexpr double TWO_PI = 2 * 3.141592653589793;     // the reference's 2 * np.pi

// what the count phase leaves for the fill phase
struct regions_state {
  int device = 0;
  int64_t F = 0, V = 0, A = 0;
  dev_buf offsets, vertices, ks, centers, adjacency;   // int64 (F + 1), int64 (V), int64 (F), float64 (F, 2), int64 (A, 2)
};

// doubling rounds that cover any path or cycle of up to w wedges: the smallest r with 2^r >= w
inline int rounds_for(long long w) {
  int r = 0;
  while (((long long)1 << r) < w) ++r;
  return r;
}

// first index in a[0 .. n) with a[index] >= key
__device__ __forceinline__ long long lower_bound(const u64* __restrict__ a, long long n, u64 key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// np.argmin of the x column: the first minimum, a NaN counting as smaller than every number (the first NaN wins)
__device__ __forceinline__ bool argmin_before(double xa, long long ia, double xb, long long ib) {
  const bool na = xa != xa, nb = xb != xb;
  if (na != nb) return na;
  if (!na && xa != xb) return xa < xb;
  return ia < ib;
}

// ext[0 .. n) are the caller's points (copied before this launch); writes the grown node ext[n] and *i0.  One workgroup.
__global__ __launch_bounds__(1024) void grow_kernel(double2* __restrict__ ext, long long n, int* __restrict__ i0) {
  __shared__ double sx[1024];
  __shared__ long long si[1024];
  const int t = threadIdx.x;
  double bx = 0;
  long long bi = -1;
  for (long long i = t; i < n; i += 1024) {
    const double x = ext[i].x;
    if (bi < 0 || argmin_before(x, i, bx, bi)) {
      bx = x;
      bi = i;
    }
  }
  sx[t] = bx;
  si[t] = bi;
  __syncthreads();
  for (int d = 512; d > 0; d >>= 1) {
    if (t < d && si[t + d] >= 0 && (si[t] < 0 || argmin_before(sx[t + d], si[t + d], sx[t], si[t]))) {
      sx[t] = sx[t + d];
      si[t] = si[t + d];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double2 p = ext[si[0]];
    ext[n] = make_double2(p.x - 1, p.y);
    *i0 = (int)si[0];
  }
}

// keys[0 .. e) from the caller's pairs, keys[e], keys[e + 1] the grown edge.  A pair out of [0, n) or a self-loop raises the flag.
__global__ __launch_bounds__(256) void edge_key_kernel(const long long* __restrict__ ijs, long long e, long long n,
                                                       const int* __restrict__ i0, u64* __restrict__ keys, int* __restrict__ flag) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < e) {
    const long long i = ijs[2 * k], j = ijs[2 * k + 1];
    if (i < 0 || i >= n || j < 0 || j >= n || i == j) {
      atomicOr(flag, 1);
      keys[k] = PAD_KEY;
    } else {
      keys[k] = ((u64)i << 32) | (u64)j;
    }
  } else if (k == e) {
    keys[k] = ((u64)*i0 << 32) | (u64)n;
  } else if (k == e + 1) {
    keys[k] = ((u64)n << 32) | (u64)*i0;
  }
}

// row[i] = first unique edge of node i, i in [0, nodes]; row[nodes] = m
__global__ __launch_bounds__(256) void row_kernel(const u64* __restrict__ ukeys, long long m, long long nodes, int* __restrict__ row) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i > nodes) return;
  row[i] = (int)lower_bound(ukeys, m, (u64)i << 32);
}

__global__ __launch_bounds__(256) void theta_kernel(const u64* __restrict__ ukeys, long long m, const double2* __restrict__ ext,
                                                    double* __restrict__ theta) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const double2 pi = ext[ukeys[k] >> 32], pj = ext[ukeys[k] & 0xffffffffull];
  const double dx = pj.x - pi.x, dy = pj.y - pi.y;
  theta[k] = fmod(atan2(dy, dx) + TWO_PI, TWO_PI);
}

// sorted[row start + (entries of the row ordered before k by (theta, j))] = j of edge k
__global__ __launch_bounds__(256) void angular_sort_kernel(const u64* __restrict__ ukeys, long long m, const int* __restrict__ row,
                                                           const double* __restrict__ theta, int* __restrict__ sorted) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const int i = (int)(ukeys[k] >> 32), j = (int)(ukeys[k] & 0xffffffffull);
  const int s = row[i], e = row[i + 1];
  const double th = theta[k];
  int before = 0;
  for (int u = s; u < e; ++u) {
    const double tu = theta[u];
    const int ju = (int)(ukeys[u] & 0xffffffffull);
    before += (tu < th || (tu == th && ju < j)) ? 1 : 0;
  }
  sorted[s + before] = j;
}

// slots [0, m): the wedge of edge slot k; slots [m, m + nodes): the isolated row of node k - m, or padding
__global__ __launch_bounds__(256) void wedge_kernel(const u64* __restrict__ ukeys, long long m, long long nodes,
                                                    const int* __restrict__ row, const int* __restrict__ sorted, u64* __restrict__ wkeys,
                                                    int* __restrict__ wlast) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m + nodes) return;
  if (k < m) {
    const int i = (int)(ukeys[k] >> 32);
    const int s = row[i], d = row[i + 1] - s, t = (int)k - s;
    if (d >= 2) {
      const int prev = sorted[s + (t == 0 ? d - 1 : t - 1)];
      wkeys[k] = ((u64)prev << 32) | (u64)(i + 1);
      wlast[k] = sorted[k];
    } else {
      wkeys[k] = (u64)sorted[s] << 32;             // col1 = -1
      wlast[k] = sorted[s];
    }
  } else {
    const long long i = k - m;
    wkeys[k] = row[i + 1] == row[i] ? (u64)i << 32 : PAD_KEY;
    wlast[k] = -1;
  }
}

// succ[w] = index of the row (col1, col2) of wedge w, -1 at a dead end; the doubling starts from it
__global__ __launch_bounds__(256) void successor_kernel(const u64* __restrict__ wkeys, const int* __restrict__ wlast, long long w_n,
                                                        int* __restrict__ succ, int* __restrict__ ptr, int* __restrict__ mn) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n) return;
  const u64 key = wkeys[w];
  int nx = -1;
  if (key != PAD_KEY && (key & 0xffffffffull) != 0) {
    const u64 want = (((key & 0xffffffffull) - 1) << 32) | (u64)(wlast[w] + 1);
    const long long at = lower_bound(wkeys, w_n, want);
    if (at < w_n && wkeys[at] == want) nx = (int)at;
  }
  succ[w] = nx;
  ptr[w] = nx;
  mn[w] = (int)w;
}

// one doubling round of the labelling: the pointer jumps twice as far, the minimum covers twice as many wedges
__global__ __launch_bounds__(256) void label_round_kernel(const int* __restrict__ ptr_in, const int* __restrict__ mn_in, long long w_n,
                                                          int* __restrict__ ptr_out, int* __restrict__ mn_out) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n) return;
  const int p = ptr_in[w];
  int m = mn_in[w], q = -1;
  if (p >= 0) {
    m = min(m, mn_in[p]);
    q = ptr_in[p];
  }
  ptr_out[w] = q;
  mn_out[w] = m;
}

// cut every cycle in front of its smallest wedge: nxt = successor, or -1 when the successor is the smallest; dist = 1
__global__ __launch_bounds__(256) void rank_init_kernel(const int* __restrict__ succ, const int* __restrict__ ptr, const int* __restrict__ mn,
                                                        long long w_n, int* __restrict__ nxt, int* __restrict__ dist) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n) return;
  const bool on = ptr[w] >= 0;
  nxt[w] = on && succ[w] != mn[w] ? succ[w] : -1;
  dist[w] = on ? 1 : 0;
}

__global__ __launch_bounds__(256) void rank_round_kernel(const int* __restrict__ nxt_in, const int* __restrict__ dist_in, long long w_n,
                                                         int* __restrict__ nxt_out, int* __restrict__ dist_out) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n) return;
  const int p = nxt_in[w];
  int d = dist_in[w], q = -1;
  if (p >= 0) {
    d += dist_in[p];
    q = nxt_in[p];
  }
  nxt_out[w] = q;
  dist_out[w] = d;
}

// is_min[w] = 1 for the smallest wedge of a cycle (is_min has w_n + 1 entries, the last 0: its scan ends in the face count)
__global__ __launch_bounds__(256) void min_flag_kernel(const int* __restrict__ ptr, const int* __restrict__ mn, long long w_n,
                                                       int* __restrict__ is_min) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w > w_n) return;
  is_min[w] = (w < w_n && ptr[w] >= 0 && mn[w] == (int)w) ? 1 : 0;
}

// ks[face] = length of the cycle (ks has w_n + 1 zeroed entries: its scan gives the offsets and ends in the vertex count)
__global__ __launch_bounds__(256) void ks_kernel(const int* __restrict__ is_min, const int* __restrict__ fid, const int* __restrict__ dist,
                                                 long long w_n, long long* __restrict__ ks) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n || !is_min[w]) return;
  ks[fid[w]] = dist[w];
}

__global__ __launch_bounds__(256) void vertices_kernel(const u64* __restrict__ wkeys, const int* __restrict__ ptr, const int* __restrict__ mn,
                                                       const int* __restrict__ fid, const int* __restrict__ dist,
                                                       const long long* __restrict__ offsets, long long w_n, long long* __restrict__ vertices) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n || ptr[w] < 0) return;
  const int m = mn[w];
  const long long rank = (int)w == m ? 0 : dist[m] - dist[w];
  vertices[offsets[fid[m]] + rank] = (long long)(wkeys[w] >> 32);
}

// pair[w] = 1 when wedge w = (a, b, .) with a < b and its reverse half-edge (b, a, .) both lie on cycles; partner[w] = the reverse
__global__ __launch_bounds__(256) void pair_flag_kernel(const u64* __restrict__ wkeys, const int* __restrict__ ptr, long long w_n,
                                                        int* __restrict__ pair, int* __restrict__ partner) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w > w_n) return;
  int flag = 0, other = -1;
  if (w < w_n && ptr[w] >= 0) {
    const u64 a = wkeys[w] >> 32, b1 = wkeys[w] & 0xffffffffull;   // b1 = b + 1 >= 1 on a cycle
    if (a + 1 < b1) {
      const u64 want = ((b1 - 1) << 32) | (a + 1);
      const long long at = lower_bound(wkeys, w_n, want);
      if (at < w_n && wkeys[at] == want && ptr[at] >= 0) {
        flag = 1;
        other = (int)at;
      }
    }
  }
  pair[w] = flag;
  if (w < w_n) partner[w] = other;
}

__global__ __launch_bounds__(256) void adjacency_kernel(const int* __restrict__ pair, const int* __restrict__ partner, const int* __restrict__ pos,
                                                        const int* __restrict__ mn, const int* __restrict__ fid, long long w_n,
                                                        long long* __restrict__ adjacency) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= w_n || !pair[w]) return;
  adjacency[2 * (long long)pos[w]] = fid[mn[w]];
  adjacency[2 * (long long)pos[w] + 1] = fid[mn[partner[w]]];
}

// centers[f] = the face's vertex coordinates added one after the other in vertex order, divided by k
__global__ __launch_bounds__(256) void centers_kernel(const double2* __restrict__ ext, const long long* __restrict__ offsets,
                                                      const long long* __restrict__ vertices, long long faces, double2* __restrict__ centers) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= faces) return;
  const long long lo = offsets[f], hi = offsets[f + 1];
  double x = 0, y = 0;
  for (long long v = lo; v < hi; ++v) {
    const double2 p = ext[vertices[v]];
    x += p.x;
    y += p.y;
  }
  const double k = (double)(hi - lo);
  centers[f] = make_double2(x / k, y / k);
}

// ---------------------------------------------------------------------------------------------------------------------
// the launch sequence
// ---------------------------------------------------------------------------------------------------------------------

int regions_count(regions_state* st, const double* pts, int64_t n, const long long* ijs, int64_t e, hipStream_t s) {
  if (n == 0) return 0;
  int rc;
  temp_store tmp;
  const long long nodes = n + 1, e2 = e + 2;

  // grown edge, edge keys, sort, deduplicate
  dev_buf d_ext, d_small, d_keys, d_ukeys;
  if ((rc = d_ext.alloc(sizeof(double2) * (size_t)nodes)) || (rc = d_small.alloc(64)) ||
      (rc = d_keys.alloc(sizeof(u64) * 2 * (size_t)e2)) || (rc = d_ukeys.alloc(sizeof(u64) * (size_t)e2)))
    return rc;
  int* d_i0 = d_small.as<int>();                    // [0] i0, [1] error flag, [2] unique edges
  ZK_HIP(hipMemsetAsync(d_small.p, 0, 64, s));
  ZK_HIP(hipMemcpyAsync(d_ext.p, pts, sizeof(double2) * (size_t)n, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(grow_kernel, dim3(1), dim3(1024), 0, s, d_ext.as<double2>(), (long long)n, d_i0);
  u64 *k_in = d_keys.as<u64>(), *k_out = k_in + e2;
  hipLaunchKernelGGL(edge_key_kernel, dim3(blocks_of(e2)), dim3(256), 0, s, ijs, (long long)e, (long long)n, d_i0, k_in, d_i0 + 1);
  ZK_HIP(hipGetLastError());
  if ((rc = zk_prim(tmp, [&](void* p, size_t& b) { return rocprim::radix_sort_keys(p, b, k_in, k_out, (size_t)e2, 0, 64, s); })) ||
      (rc = zk_prim(tmp, [&](void* p, size_t& b) {
         return rocprim::unique(p, b, k_out, d_ukeys.as<u64>(), (unsigned int*)(d_i0 + 2), (size_t)e2, rocprim::equal_to<u64>(), s);
       })))
    return rc;
  int small[3] = {0, 0, 0};
  ZK_HIP(hipMemcpyAsync(small, d_small.p, sizeof(small), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  if (small[1]) return zk_fail(ZK_E_BADARG, "find_regions: an edge is out of [0, n_points) or joins a node to itself");
  const long long m = small[2], w_n = m + nodes;
  if (m < 2 || m > e2 || w_n >= ((long long)1 << 31)) return zk_fail(ZK_E_BADARG, "find_regions: bad unique edge count");

  // rows, angles, the angular order, wedges
  dev_buf d_row, d_theta, d_sorted, d_wkeys, d_wlast;
  if ((rc = d_row.alloc(sizeof(int) * (size_t)(nodes + 1))) || (rc = d_theta.alloc(sizeof(double) * (size_t)m)) ||
      (rc = d_sorted.alloc(sizeof(int) * (size_t)m)) || (rc = d_wkeys.alloc(sizeof(u64) * 2 * (size_t)w_n)) ||
      (rc = d_wlast.alloc(sizeof(int) * 2 * (size_t)w_n)))
    return rc;
  const u64* uk = d_ukeys.as<u64>();
  hipLaunchKernelGGL(row_kernel, dim3(blocks_of(nodes + 1)), dim3(256), 0, s, uk, m, nodes, d_row.as<int>());
  hipLaunchKernelGGL(theta_kernel, dim3(blocks_of(m)), dim3(256), 0, s, uk, m, d_ext.as<double2>(), d_theta.as<double>());
  hipLaunchKernelGGL(angular_sort_kernel, dim3(blocks_of(m)), dim3(256), 0, s, uk, m, d_row.as<int>(), d_theta.as<double>(),
                     d_sorted.as<int>());
  u64 *wk_in = d_wkeys.as<u64>(), *wk = wk_in + w_n;
  int *wl_in = d_wlast.as<int>(), *wl = wl_in + w_n;
  hipLaunchKernelGGL(wedge_kernel, dim3(blocks_of(w_n)), dim3(256), 0, s, uk, m, nodes, d_row.as<int>(), d_sorted.as<int>(), wk_in, wl_in);
  ZK_HIP(hipGetLastError());
  if ((rc = zk_prim(tmp, [&](void* p, size_t& b) { return rocprim::radix_sort_pairs(p, b, wk_in, wk, wl_in, wl, (size_t)w_n, 0, 64, s); })))
    return rc;

  // successor, cycle labels, ranks
  dev_buf d_succ, d_ptr, d_mn, d_nxt, d_dist;
  if ((rc = d_succ.alloc(sizeof(int) * (size_t)w_n)) || (rc = d_ptr.alloc(sizeof(int) * 2 * (size_t)w_n)) ||
      (rc = d_mn.alloc(sizeof(int) * 2 * (size_t)w_n)) || (rc = d_nxt.alloc(sizeof(int) * 2 * (size_t)w_n)) ||
      (rc = d_dist.alloc(sizeof(int) * 2 * (size_t)w_n)))
    return rc;
  const unsigned wb = blocks_of(w_n);
  const int rounds = rounds_for(w_n);
  int *ptr = d_ptr.as<int>(), *ptr2 = ptr + w_n, *mn = d_mn.as<int>(), *mn2 = mn + w_n;
  hipLaunchKernelGGL(successor_kernel, dim3(wb), dim3(256), 0, s, wk, wl, w_n, d_succ.as<int>(), ptr, mn);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(label_round_kernel, dim3(wb), dim3(256), 0, s, ptr, mn, w_n, ptr2, mn2);
    std::swap(ptr, ptr2);
    std::swap(mn, mn2);
  }
  int *nxt = d_nxt.as<int>(), *nxt2 = nxt + w_n, *dist = d_dist.as<int>(), *dist2 = dist + w_n;
  hipLaunchKernelGGL(rank_init_kernel, dim3(wb), dim3(256), 0, s, d_succ.as<int>(), ptr, mn, w_n, nxt, dist);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(rank_round_kernel, dim3(wb), dim3(256), 0, s, nxt, dist, w_n, nxt2, dist2);
    std::swap(nxt, nxt2);
    std::swap(dist, dist2);
  }
  ZK_HIP(hipGetLastError());

  // faces in ascending order of their smallest wedge, lengths, offsets, vertices, adjacency
  dev_buf d_flag, d_fid, d_pair, d_partner, d_pos, d_ks, d_adj;
  if ((rc = d_flag.alloc(sizeof(int) * (size_t)(w_n + 1))) || (rc = d_fid.alloc(sizeof(int) * (size_t)(w_n + 1))) ||
      (rc = d_pair.alloc(sizeof(int) * (size_t)(w_n + 1))) || (rc = d_partner.alloc(sizeof(int) * (size_t)w_n)) ||
      (rc = d_pos.alloc(sizeof(int) * (size_t)(w_n + 1))) || (rc = d_ks.alloc(sizeof(long long) * (size_t)(w_n + 1))) ||
      (rc = st->offsets.alloc(sizeof(long long) * (size_t)(w_n + 1))) || (rc = st->vertices.alloc(sizeof(long long) * (size_t)w_n)))
    return rc;
  hipLaunchKernelGGL(min_flag_kernel, dim3(blocks_of(w_n + 1)), dim3(256), 0, s, ptr, mn, w_n, d_flag.as<int>());
  if ((rc = exclusive_sum<int>(tmp, d_flag.as<int>(), d_fid.as<int>(), (size_t)(w_n + 1), s))) return rc;
  ZK_HIP(hipMemsetAsync(d_ks.p, 0, sizeof(long long) * (size_t)(w_n + 1), s));
  hipLaunchKernelGGL(ks_kernel, dim3(wb), dim3(256), 0, s, d_flag.as<int>(), d_fid.as<int>(), dist, w_n, d_ks.as<long long>());
  if ((rc = exclusive_sum<long long>(tmp, d_ks.as<long long>(), st->offsets.as<long long>(), (size_t)(w_n + 1), s))) return rc;
  hipLaunchKernelGGL(vertices_kernel, dim3(wb), dim3(256), 0, s, wk, ptr, mn, d_fid.as<int>(), dist, st->offsets.as<long long>(), w_n,
                     st->vertices.as<long long>());
  hipLaunchKernelGGL(pair_flag_kernel, dim3(blocks_of(w_n + 1)), dim3(256), 0, s, wk, ptr, w_n, d_pair.as<int>(), d_partner.as<int>());
  if ((rc = exclusive_sum<int>(tmp, d_pair.as<int>(), d_pos.as<int>(), (size_t)(w_n + 1), s))) return rc;
  ZK_HIP(hipGetLastError());

  // the counts cross to the host: they size what the caller allocates
  int faces = 0, pairs = 0;
  long long verts = 0;
  ZK_HIP(hipMemcpyAsync(&faces, d_fid.as<int>() + w_n, sizeof(int), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipMemcpyAsync(&pairs, d_pos.as<int>() + w_n, sizeof(int), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipMemcpyAsync(&verts, st->offsets.as<long long>() + w_n, sizeof(long long), hipMemcpyDeviceToHost, s));
  ZK_HIP(hipStreamSynchronize(s));
  st->F = faces;
  st->V = verts;
  st->A = pairs;
  if ((rc = st->ks.alloc(sizeof(long long) * (size_t)faces)) || (rc = st->centers.alloc(sizeof(double2) * (size_t)faces)) ||
      (rc = st->adjacency.alloc(sizeof(long long) * 2 * (size_t)pairs)))
    return rc;
  if (faces) {
    ZK_HIP(hipMemcpyAsync(st->ks.p, d_ks.p, sizeof(long long) * (size_t)faces, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(centers_kernel, dim3(blocks_of(faces)), dim3(256), 0, s, d_ext.as<double2>(), st->offsets.as<long long>(),
                       st->vertices.as<long long>(), (long long)faces, st->centers.as<double2>());
  }
  if (pairs)
    hipLaunchKernelGGL(adjacency_kernel, dim3(wb), dim3(256), 0, s, d_pair.as<int>(), d_partner.as<int>(), d_pos.as<int>(), mn,
                       d_fid.as<int>(), w_n, st->adjacency.as<long long>());
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(s));                  // the working buffers go with this call
  return 0;
}

// copies what the count phase left to the caller's arrays (device or host memory, by `kind`)
int regions_fill(const regions_state* st, int64_t* offsets, int64_t* vertices, int64_t* ks, double* centers, int64_t* adjacency,
                 hipMemcpyKind kind, hipStream_t s) {
  if (offsets) {
    if (st->offsets.p) ZK_HIP(hipMemcpyAsync(offsets, st->offsets.p, sizeof(int64_t) * (size_t)(st->F + 1), kind, s));
    else if (kind == hipMemcpyDeviceToDevice) ZK_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), s));
    else offsets[0] = 0;
  }
  if (vertices && st->V) ZK_HIP(hipMemcpyAsync(vertices, st->vertices.p, sizeof(int64_t) * (size_t)st->V, kind, s));
  if (ks && st->F) ZK_HIP(hipMemcpyAsync(ks, st->ks.p, sizeof(int64_t) * (size_t)st->F, kind, s));
  if (centers && st->F) ZK_HIP(hipMemcpyAsync(centers, st->centers.p, sizeof(double) * 2 * (size_t)st->F, kind, s));
  if (adjacency && st->A) ZK_HIP(hipMemcpyAsync(adjacency, st->adjacency.p, sizeof(int64_t) * 2 * (size_t)st->A, kind, s));
  ZK_HIP(hipStreamSynchronize(s));                  // the state is freed next
  return 0;
}

int check_regions(const void* pts, int64_t n, const void* ijs, int64_t e, void** state, const int64_t* counts) {
  if (!state) return zk_fail(ZK_E_BADARG, "find_regions: null state pointer");
  if (*state) return 0;                             // fill phase: the inputs are not read again
  if (!counts) return zk_fail(ZK_E_BADARG, "find_regions: the count phase needs counts_host");
  if (n < 0 || e < 0 || n + e + 4 >= ((int64_t)1 << 31)) return zk_fail(ZK_E_BADARG, "find_regions: needs 0 <= n_points + n_edges + 4 < 2^31");
  if ((n && !pts) || (e && !ijs)) return zk_fail(ZK_E_BADARG, "find_regions: null pointer");
  if (n == 0 && e != 0) return zk_fail(ZK_E_BADARG, "find_regions: edges without points");
  return 0;
}

// both phases on resident inputs; `kind` says where the fill phase's arrays live
int regions_call(int device, const double* pts, int64_t n, const int64_t* ijs, int64_t e, void** state, int64_t* counts, int64_t* offsets,
                 int64_t* vertices, int64_t* ks, double* centers, int64_t* adjacency, hipMemcpyKind kind, hipStream_t s) {
  if (!*state) {
    regions_state* st = new (std::nothrow) regions_state;
    if (!st) return zk_fail(ZK_E_BADARG, "find_regions: out of host memory");
    st->device = device;
    const int rc = regions_count(st, pts, n, (const long long*)ijs, e, s);
    if (rc) {
      delete st;
      return rc;
    }
    counts[0] = st->F;
    counts[1] = st->V;
    counts[2] = st->A;
    *state = st;
    return 0;
  }
  regions_state* st = (regions_state*)*state;
  const int rc = regions_fill(st, offsets, vertices, ks, centers, adjacency, kind, s);
  delete st;
  *state = nullptr;
  return rc;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
extern "C" int zk_find_regions_dev(int device, const double* points_dev, int64_t n_points, const int64_t* edges_dev, int64_t n_edges,
                                   void** state, int64_t* counts_host, int64_t* offsets_dev, int64_t* vertices_dev, int64_t* ks_dev,
                                   double* centers_dev, int64_t* adjacency_dev, void* hip_stream) {
  int rc = check_regions(points_dev, n_points, edges_dev, n_edges, state, counts_host);
  if (rc) return rc;
  ZK_ON_DEVICE(*state ? ((regions_state*)*state)->device : device);
  return regions_call(device, points_dev, n_points, edges_dev, n_edges, state, counts_host, offsets_dev, vertices_dev, ks_dev, centers_dev,
                      adjacency_dev, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream);
}

extern "C" int zk_find_regions(int device, const double* points_host, int64_t n_points, const int64_t* edges_host, int64_t n_edges,
                               void** state, int64_t* counts_host, int64_t* offsets_host, int64_t* vertices_host, int64_t* ks_host,
                               double* centers_host, int64_t* adjacency_host) {
  int rc = check_regions(points_host, n_points, edges_host, n_edges, state, counts_host);
  if (rc) return rc;
  if (!*state)                                      // the values are checked before anything is launched
    for (int64_t k = 0; k < n_edges; ++k) {
      const int64_t i = edges_host[2 * k], j = edges_host[2 * k + 1];
      if (i < 0 || i >= n_points || j < 0 || j >= n_points || i == j)
        return zk_fail(ZK_E_BADARG, "find_regions: an edge is out of [0, n_points) or joins a node to itself");
    }
  ZK_ON_DEVICE(*state ? ((regions_state*)*state)->device : device);
  const size_t pts_bytes = sizeof(double) * 2 * (size_t)n_points, ijs_bytes = sizeof(int64_t) * 2 * (size_t)n_edges;
  dev_buf d_pts, d_ijs;                              // the second call of a pair (*state set) reads neither
  if (!*state && n_points && ((rc = d_pts.upload(points_host, pts_bytes)) || (rc = d_ijs.upload(edges_host, ijs_bytes)))) return rc;
  return regions_call(device, d_pts.as<double>(), n_points, d_ijs.as<int64_t>(), n_edges, state, counts_host, offsets_host, vertices_host,
                      ks_host, centers_host, adjacency_host, hipMemcpyDeviceToHost, (hipStream_t)0);
}

// zk_kmeans.hip -- k-means on the resident moment matrix (zk_rows.h):
//   kmeans_lbs(X, n)   reference clustering/_clustering_functions.py:8-22  (sklearn KMeans(n, random_state).fit(X).labels_)
// k-means++ seeding, the Lloyd pass and the own-distance pass of the empty-cluster relocation; scikit-learn's control flow
// between the passes is restated in mtflearn_amd/clustering.py.
#include "zk_rows.h"

namespace {

// dots of the centred row with KC wave-uniform vectors: ct is [D][KP] (vector index fastest)
template <int KC>
__device__ __forceinline__ void dots(const double* __restrict__ row, int D, const ZK_CONST double* cm, const ZK_CONST double* ct,
                                     int KP, double (&d)[KC]) {
#pragma unroll
  for (int c = 0; c < KC; ++c) d[c] = 0.0;
  for (int i = 0; i < D; ++i) {
    const double v = row[i] - cm[i];
    const ZK_CONST double* c = ct + (long long)i * KP;
#pragma unroll
    for (int cc = 0; cc < KC; ++cc) d[cc] = __builtin_fma(v, c[cc], d[cc]);
  }
}

// ---- k-means++ seeding step (sklearn/cluster/_kmeans.py _kmeans_plusplus): squared distances of every row to TP <= 8
// candidate rows, d = max(0, (-2 x.c + |c|^2) + |x|^2) as sklearn's _euclidean_distances builds them, folded with the
// closest distance so far; out[c][r]; part[block][c] = potential of candidate c over the block's rows ----------------
template <int TP>
__global__ __launch_bounds__(64) void seed_kernel(const double* __restrict__ X, long long N, int D, int nbuf,
                                                  const double* __restrict__ mean, const double* __restrict__ Ct,
                                                  const double* __restrict__ cc, int t, const double* __restrict__ xsq,
                                                  const double* __restrict__ closest, double* __restrict__ out,
                                                  double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  const ZK_CONST double* cm = zk_const(mean);
  const ZK_CONST double* ct = zk_const(Ct);
  const ZK_CONST double* ccc = zk_const(cc);
  double pot[TP];
#pragma unroll
  for (int c = 0; c < TP; ++c) pot[c] = 0.0;
  for (tile_pipe pipe(X, N, D, lds, lane, nbuf); pipe.live(); pipe.advance()) {
    const double* row = pipe.acquire() + lane * D;
    const long long r = pipe.t * TILE + lane;
    const bool live = r < N;
    const double xs = live ? xsq[r] : 0.0;
    const double prev = closest && live ? closest[r] : std::numeric_limits<double>::infinity();
    double d[TP];
    dots<TP>(row, D, cm, ct, TP, d);
#pragma unroll
    for (int c = 0; c < TP; ++c) {
      double v = __builtin_fma(-2.0, d[c], ccc[c]) + xs;
      v = v > 0.0 ? v : 0.0;
      v = v < prev ? v : prev;
      if (live && c < t) {
        __builtin_nontemporal_store(v, out + (long long)c * N + r);
        pot[c] += v;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < TP; ++c) {
    const double s = wave_sum(pot[c]);
    if (lane == 0) part[(long long)blockIdx.x * TP + c] = s;
  }
}

// sums of consecutive blocks of 1024 elements (for searchsorted(cumsum(a), v))
__global__ __launch_bounds__(256) void blocksum_kernel(const double* __restrict__ a, long long n, double* __restrict__ bsum) {
  __shared__ double w[4];
  const long long base = (long long)blockIdx.x * 1024;
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long i = base + q * 256 + threadIdx.x;
    s += i < n ? a[i] : 0.0;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

// ---- one Lloyd iteration (sklearn _k_means_lloyd.pyx lloyd_iter_chunked_dense): label = first argmin_c (|c|^2 - 2 x.c);
// with `update`: part[block][c][0..D-1] = sum of the centred rows of cluster c, [D] = their number -----------------------
template <int KC>
__device__ __forceinline__ void lloyd_chunk(const double* __restrict__ row, int D, const ZK_CONST double* cm, const ZK_CONST double* ct,
                                            const ZK_CONST double* cs, int KP, int c0, double& best, int& bl) {
  double d[KC];
  dots<KC>(row, D, cm, ct + c0, KP, d);
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const double sc = __builtin_fma(-2.0, d[c], cs[c0 + c]);
    if (sc < best) best = sc, bl = c0 + c;
  }
}

// sum over the rows in `mask` (wave-uniform) of column j of the tile, centred by mj; j == D: their number.  Four rows per
// step: four scalar bit extractions and LDS reads, one wait, then the adds in row order.
__device__ __forceinline__ double masked_column_sum(const double* __restrict__ tile, int D, int j, double mj, unsigned long long mask) {
  const double* col = tile + (j < D ? j : D - 1);
  const int n_rows = __builtin_popcountll(mask);
  int n = n_rows;
  double acc = 0.0;
  auto next = [&]() {
    const int r = __builtin_ctzll(mask);
    mask &= mask - 1;
    return col[r * D];
  };
  for (; n >= 4; n -= 4) {
    const double v0 = next(), v1 = next(), v2 = next(), v3 = next();
    acc += v0 - mj;
    acc += v1 - mj;
    acc += v2 - mj;
    acc += v3 - mj;
  }
  for (; n > 0; --n) acc += next() - mj;
  return j == D ? (double)n_rows : acc;
}

// KMAX > 0: k <= KMAX, the per-cluster column sums live in registers (lane = column; the rows of cluster c are the set bits
// of ballot(label == c), walked by a scalar loop); KMAX = 0: any k, LDS floating-point adds into a wave-private table
// (an LDS f64 atomic costs ~280 cycles per wave: 2.4x the whole pass at k = 6, so only where the registers do not reach).
// Tried: two waves per tile, both computing the labels (no exchange) and splitting the clusters of the column sums by
// parity, one tile buffer per pair (twelve waves per CU): 0.48 vs 0.47 ms per call at (4 M x 45, k = 6), 0.75 vs 0.83 at
// (2 M x 91, k = 12) -- the redundant distance pass and the two barriers per tile eat what the occupancy gives.  Not kept.
template <int KMAX>
__global__ __launch_bounds__(64) void lloyd_kernel(const double* __restrict__ X, long long N, int D, int nbuf,
                                                   const double* __restrict__ mean, const double* __restrict__ Ct,
                                                   const double* __restrict__ csq, int KP, int k, int32_t* __restrict__ labels,
                                                   int update, double* __restrict__ part, unsigned long long* __restrict__ changed) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* sums = lds + nbuf * TILE * D;
  const int D1 = D + 1;
  const int lane = threadIdx.x;
  const ZK_CONST double* cm = zk_const(mean);
  const ZK_CONST double* ct = zk_const(Ct);
  const ZK_CONST double* cs = zk_const(csq);
  if (KMAX == 0 && update)
    for (int e = lane; e < k * D1; e += 64) sums[e] = 0.0;
  const int j0 = lane, j1 = lane + 64;
  const double m0 = j0 < D ? mean[j0] : 0.0, m1 = j1 < D ? mean[j1] : 0.0;
  constexpr int KA = KMAX > 0 ? KMAX : 1;
  double acc0[KA], acc1[KA];
#pragma unroll
  for (int c = 0; c < KA; ++c) acc0[c] = acc1[c] = 0.0;
  unsigned long long nchg = 0;
  for (tile_pipe pipe(X, N, D, lds, lane, nbuf); pipe.live(); pipe.advance()) {
    const double* tile = pipe.acquire();
    const double* row = tile + lane * D;
    double best = std::numeric_limits<double>::infinity();
    int bl = 0;
    int c0 = 0;
    for (; c0 + 8 <= KP; c0 += 8) lloyd_chunk<8>(row, D, cm, ct, cs, KP, c0, best, bl);
    if (c0 < KP) lloyd_chunk<4>(row, D, cm, ct, cs, KP, c0, best, bl);
    const long long r = pipe.t * TILE + lane;
    const bool live = r < N;
    if (live) {
      nchg += labels[r] != bl;
      labels[r] = bl;
    }
    if (update) {
      const int rows = pipe.rows();
      if constexpr (KMAX > 0) {
        const unsigned long long valid = rows == TILE ? ~0ull : (1ull << rows) - 1;
#pragma unroll
        for (int c = 0; c < KMAX; ++c) {
          const unsigned long long mask = __ballot(bl == c) & valid;
          if (j0 <= D) acc0[c] += masked_column_sum(tile, D, j0, m0, mask);
          if (D >= 64 && j1 <= D) acc1[c] += masked_column_sum(tile, D, j1, m1, mask);
        }
      } else {
        // lane = column; the label of row rr is lane rr's `bl`.  Eight rows per step: their reads first, then the adds
        for (int r0 = 0; r0 < rows; r0 += 8) {
          double v0[8], v1[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            v0[u] = j0 < D ? tile[(r0 + u) * D + j0] : m0 + 1.0;
            v1[u] = j1 < D ? tile[(r0 + u) * D + j1] : m1 + 1.0;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (r0 + u < rows) {
              const int l = __builtin_amdgcn_readlane(bl, r0 + u);
              double* dst = sums + l * D1;
              if (j0 <= D) (void)__hip_atomic_fetch_add(dst + j0, v0[u] - m0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
              if (j1 <= D) (void)__hip_atomic_fetch_add(dst + j1, v1[u] - m1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (update) {
    double* out = part + (long long)blockIdx.x * k * D1;
    if constexpr (KMAX > 0) {
#pragma unroll
      for (int c = 0; c < KMAX; ++c)
        if (c < k) {
          if (j0 <= D) out[c * D1 + j0] = acc0[c];
          if (j1 <= D) out[c * D1 + j1] = acc1[c];
        }
    } else {
      for (int e = lane; e < k * D1; e += 64) out[e] = sums[e];
    }
  }
  if (__ballot(nchg != 0) && nchg) atomicAdd(changed, nchg);
}

// dist[r] = sum_j ((x_rj - mean_j) - centre[label_r][j])^2  (sklearn _relocate_empty_clusters_dense)
__global__ __launch_bounds__(64) void owndist_kernel(const double* __restrict__ X, long long N, int D, int nbuf,
                                                     const double* __restrict__ mean, const double* __restrict__ centers,
                                                     const int32_t* __restrict__ labels, double* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  const ZK_CONST double* cm = zk_const(mean);
  for (tile_pipe pipe(X, N, D, lds, lane, nbuf); pipe.live(); pipe.advance()) {
    const double* row = pipe.acquire() + lane * D;
    const long long r = pipe.t * TILE + lane;
    if (r < N) {
      const double* c = centers + (long long)labels[r] * D;
      double s = 0.0;
      for (int i = 0; i < D; ++i) {
        const double v = (row[i] - cm[i]) - c[i];
        s += v * v;
      }
      dist[r] = s;
    }
  }
}

}  // namespace

// operand table of wave-uniform vectors: [D][KP] (vector index fastest), then their KP squared norms (+inf beyond n)
static void pack_vectors(const double* v, int n, int D, int KP, bool pad_inf, std::vector<double>& h) {
  h.assign((size_t)D * KP + KP, 0.0);
  for (int c = 0; c < n; ++c) {
    double s = 0.0;
    for (int i = 0; i < D; ++i) {
      const double x = v[(size_t)c * D + i];
      h[(size_t)i * KP + c] = x;
      s += x * x;
    }
    h[(size_t)D * KP + c] = s;
  }
  if (pad_inf)
    for (int c = n; c < KP; ++c) h[(size_t)D * KP + c] = std::numeric_limits<double>::infinity();
}

// One seeding step: the centred candidate rows cand (t, D) with their squared norms cand_sq (t) -- the caller fetched them
// with zk_rows_fetch and took the norms the way scikit-learn does -- against every row; with use_closest the distances are
// folded with the current closest-distance row.  pot_out[c] = sum_r dist[c][r].
extern "C" int zk_kmeans_seed_step(zk_rows* m, const double* cand, const double* cand_sq, int t, int use_closest, double* pot_out) {
  if (!m || !cand || !cand_sq || !pot_out) return zk_fail(ZK_E_BADARG, "null pointer");
  if (t < 1 || t > 8) return zk_fail(ZK_E_BADARG, "1 to 8 candidates per seeding step");
  if (!m->d_xsq) return zk_fail(ZK_E_BADARG, "zk_rows_center first");
  if (use_closest && !m->d_closest) return zk_fail(ZK_E_BADARG, "no closest-distance row yet");
  ZK_ON_DEVICE(m->device);
  const int TP = t <= 4 ? 4 : 8;
  pack_vectors(cand, t, m->D, TP, false, m->h_buf);
  for (int c = 0; c < t; ++c) m->h_buf[(size_t)m->D * TP + c] = cand_sq[c];
  int rc = zk_upload_tab(m);
  if (rc) return rc;
  zk_row_plan p;
  if ((rc = zk_plan_row_pass(m, 0, &p))) return rc;
  const int dst = use_closest ? 1 - m->seed_cur : m->seed_cur;
  if ((rc = zk_ensure(&m->d_seed[dst], &m->seed_bytes[dst], (size_t)8 * m->N * sizeof(double)))) return rc;
  if ((rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)p.grid * TP * sizeof(double)))) return rc;
  const double* tab = (const double*)m->d_tab;
  const double* closest = use_closest ? m->d_closest : nullptr;
  rc = zk_with_int<4, 8>(TP, [&](auto tp) {
    return zk_launch_row_pass(seed_kernel<tp>, m, p, (const double*)m->d_mean, tab, tab + (size_t)m->D * TP, t, (const double*)m->d_xsq,
                              closest, (double*)m->d_seed[dst], (double*)m->d_part);
  });
  if (rc) return rc;
  double pot[8];
  if ((rc = zk_reduce_to_host(m, p.grid, TP, pot))) return rc;
  for (int c = 0; c < t; ++c) pot_out[c] = pot[c];
  m->seed_t = t;
  m->seed_last = dst;  // seed_cur changes when zk_kmeans_seed_pick adopts one of these rows
  return 0;
}

// Adopt candidate `which` of the last step as the closest-distance row, then idx_out[i] = searchsorted(cumsum(closest),
// vals[i]) (side 'left', clipped to N - 1) for the next step's draws (n_vals may be 0).
extern "C" int zk_kmeans_seed_pick(zk_rows* m, int which, const double* vals, int n_vals, int64_t* idx_out) {
  if (!m || m->seed_last < 0 || which < 0 || which >= m->seed_t) return zk_fail(ZK_E_BADARG, "no seeding step to pick from");
  if (n_vals < 0 || (n_vals > 0 && (!vals || !idx_out))) return zk_fail(ZK_E_BADARG, "bad arguments");
  ZK_ON_DEVICE(m->device);
  m->seed_cur = m->seed_last;
  m->d_closest = (const double*)m->d_seed[m->seed_cur] + (size_t)which * m->N;
  if (n_vals == 0) return 0;
  const long long nb = (m->N + 1023) / 1024;
  int rc = zk_ensure(&m->d_red, &m->red_bytes, (size_t)nb * sizeof(double));
  if (rc) return rc;
  hipLaunchKernelGGL(blocksum_kernel, dim3((unsigned)nb), dim3(256), 0, m->stream, m->d_closest, (long long)m->N, (double*)m->d_red);
  ZK_HIP(hipGetLastError());
  std::vector<double> bs(nb), cum(nb), blk(1024);
  ZK_HIP(hipMemcpyAsync(bs.data(), m->d_red, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  ZK_HIP(hipStreamSynchronize(m->stream));
  double run = 0.0;
  for (long long b = 0; b < nb; ++b) cum[b] = (run += bs[b]);
  for (int i = 0; i < n_vals; ++i) {
    long long b = std::lower_bound(cum.begin(), cum.end(), vals[i]) - cum.begin();
    long long found = m->N;  // past the end: clipped below
    while (b < nb && found == m->N) {
      const long long first = b * 1024, cnt = std::min<long long>(1024, m->N - first);
      ZK_HIP(hipMemcpy(blk.data(), m->d_closest + first, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost));
      double s = b ? cum[b - 1] : 0.0;
      for (long long e = 0; e < cnt; ++e) {
        s += blk[e];
        if (s >= vals[i]) {
          found = first + e;
          break;
        }
      }
      ++b;
    }
    idx_out[i] = std::min<long long>(found, m->N - 1);
  }
  return 0;
}

// One Lloyd pass with the centred centres (k, D): labels are rewritten on the device; with `update` sums_out (k, D) = sum
// of the centred rows of each cluster and counts_out (k); n_changed_out = rows whose label changed.
extern "C" int zk_kmeans_step(zk_rows* m, const double* centers, int k, int update, double* sums_out, double* counts_out,
                              int64_t* n_changed_out) {
  if (!m || !centers || !n_changed_out || (update && (!sums_out || !counts_out))) return zk_fail(ZK_E_BADARG, "null pointer");
  if (k < 1 || k > 256) return zk_fail(ZK_E_BADARG, "1 to 256 clusters");
  ZK_ON_DEVICE(m->device);
  const int KP = (k + 3) & ~3, D1 = m->D + 1;
  pack_vectors(centers, k, m->D, KP, true, m->h_buf);
  int rc = zk_upload_tab(m);
  if (rc) return rc;
  const int kmax = k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 0;  // per-cluster sums in registers up to 16 clusters
  const size_t sums_lds = update && !kmax ? (size_t)k * D1 * sizeof(double) : 0;
  zk_row_plan p;
  if ((rc = zk_plan_row_pass(m, sums_lds, &p)) || (rc = zk_rows_need_labels(m, true))) return rc;
  if (update && (rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)p.grid * k * D1 * sizeof(double)))) return rc;
  ZK_HIP(hipMemsetAsync(m->d_count, 0, sizeof(unsigned long long), m->stream));
  const double* tab = (const double*)m->d_tab;
  if ((rc = zk_rows_prof_begin(m))) return rc;
  rc = zk_with_int<4, 8, 16, 0>(kmax, [&](auto km) {
    return zk_launch_row_pass(lloyd_kernel<km>, m, p, (const double*)m->d_mean, tab, tab + (size_t)m->D * KP, KP, k, m->d_labels, update,
                              (double*)m->d_part, m->d_count);
  });
  if (rc || (rc = zk_rows_prof_end(m))) return rc;
  unsigned long long chg = 0;
  if (update) {
    std::vector<double> red((size_t)k * D1);
    if ((rc = zk_reduce_to_host(m, p.grid, k * D1, red.data(), &chg))) return rc;  // sums and the changed-label count: one wait
    for (int c = 0; c < k; ++c) {
      for (int j = 0; j < m->D; ++j) sums_out[(size_t)c * m->D + j] = red[(size_t)c * D1 + j];
      counts_out[c] = red[(size_t)c * D1 + m->D];
    }
  } else {
    ZK_HIP(hipMemcpyAsync(&chg, m->d_count, sizeof(chg), hipMemcpyDeviceToHost, m->stream));
    ZK_HIP(hipStreamSynchronize(m->stream));
  }
  *n_changed_out = (int64_t)chg;
  return zk_rows_prof_read(m);
}

// squared distance of every centred row to the centre of its label (k, D) -> host (N): the empty-cluster relocation
extern "C" int zk_kmeans_own_distance(zk_rows* m, const double* centers, int k, double* dist_host) {
  if (!m || !centers || !dist_host || k < 1) return zk_fail(ZK_E_BADARG, "bad arguments");
  if (!m->d_labels) return zk_fail(ZK_E_BADARG, "no labels yet");
  ZK_ON_DEVICE(m->device);
  m->h_buf.assign(centers, centers + (size_t)k * m->D);
  int rc = zk_upload_tab(m);
  if (rc) return rc;
  zk_row_plan p;
  if ((rc = zk_plan_row_pass(m, 0, &p))) return rc;
  const int dst = 1 - m->seed_cur;  // the seeding scratch is free by now
  if ((rc = zk_ensure(&m->d_seed[dst], &m->seed_bytes[dst], (size_t)m->N * sizeof(double)))) return rc;
  if ((rc = zk_launch_row_pass(owndist_kernel, m, p, (const double*)m->d_mean, (const double*)m->d_tab, (const int32_t*)m->d_labels,
                               (double*)m->d_seed[dst])))
    return rc;
  ZK_HIP(hipMemcpyAsync(dist_host, m->d_seed[dst], (size_t)m->N * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  ZK_HIP(hipStreamSynchronize(m->stream));
  return 0;
}

// zk_rows.hip -- the resident moment matrix (zk_rows.h): the container, its column statistics, row fetch, labels and
// profiling entry points, and the host helpers every pass over it shares (operand-table upload, fixed-order reduction).
// The clustering passes themselves are in zk_kmeans.hip and zk_mixture.hip; the (N, D) float64 matrix stays in HBM, every
// pass over it is a kernel, and the decisions between passes (random draws, centre updates, D x D Cholesky factors,
// convergence tests) are scikit-learn's own control flow restated in the Python wrapper (mtflearn_amd/clustering.py).
#include "zk_rows.h"

namespace {

// ---- column statistics: part[block][D] = sum over the block's rows of (x - shift) or (x - shift)^2 ---------------------
__global__ __launch_bounds__(64) void colsum_kernel(const double* __restrict__ X, long long N, int D, int nbuf,
                                                    const double* __restrict__ shift, int square, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  const int j0 = lane, j1 = lane + 64;
  const double m0 = shift && j0 < D ? shift[j0] : 0.0, m1 = shift && j1 < D ? shift[j1] : 0.0;
  double a0 = 0.0, a1 = 0.0;
  for (tile_pipe pipe(X, N, D, lds, lane, nbuf); pipe.live(); pipe.advance()) {
    const double* tile = pipe.acquire();
    const int rows = pipe.rows();
    for (int r = 0; r < rows; ++r) {
      if (j0 < D) {
        const double v = tile[r * D + j0] - m0;
        a0 += square ? v * v : v;
      }
      if (j1 < D) {
        const double v = tile[r * D + j1] - m1;
        a1 += square ? v * v : v;
      }
    }
  }
  if (j0 < D) part[(long long)blockIdx.x * D + j0] = a0;
  if (j1 < D) part[(long long)blockIdx.x * D + j1] = a1;
}

// out[g][i] = sum over the blocks b of group g (b = g * group ... , ascending) of part[b][i]
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ part, int n_blocks, int n, int group,
                                                     double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b0 = blockIdx.y * group, b1 = b0 + group < n_blocks ? b0 + group : n_blocks;
  double s = 0.0;
  for (int b = b0; b < b1; ++b) s += part[(long long)b * n + i];
  out[(long long)blockIdx.y * n + i] = s;
}

// xsq[r] = sum_j (x_rj - mean_j)^2 (row_norms of the centred matrix); count[0] += rows whose norm is not finite
__global__ __launch_bounds__(64) void rownorm_kernel(const double* __restrict__ X, long long N, int D, int nbuf,
                                                     const double* __restrict__ mean, double* __restrict__ xsq,
                                                     unsigned long long* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  const ZK_CONST double* cm = zk_const(mean);
  unsigned long long bad = 0;
  for (tile_pipe pipe(X, N, D, lds, lane, nbuf); pipe.live(); pipe.advance()) {
    const double* row = pipe.acquire() + lane * D;
    double s = 0.0;
    for (int i = 0; i < D; ++i) {
      const double v = row[i] - cm[i];
      s = __builtin_fma(v, v, s);
    }
    const long long r = pipe.t * TILE + lane;
    if (r < N) {
      xsq[r] = s;
      bad += !(s <= 1.7976931348623157e308);
    }
  }
  const unsigned long long any = __ballot(bad != 0);
  if (any && bad) atomicAdd(count, bad);
}

// ---- host helpers ------------------------------------------------------------------------------------------------
// Waves per CU matter more than overlap inside a wave (4 M x 45, two buffers / 3 waves -> one buffer / 6 waves per CU: Lloyd
// pass with sums 0.67 -> 0.46 ms, labels only 0.45 -> 0.31, seeding 0.41 -> 0.36): two tile buffers (the next tile's DMA under
// this tile's arithmetic) only while eight waves still fit a CU's 160 KiB, else one
int tile_bufs(const zk_rows* m, size_t extra = 0) {
  return 8 * ((size_t)2 * TILE * m->D * sizeof(double) + extra + 512) <= 160 * 1024 ? 2 : 1;
}
size_t tile_lds(const zk_rows* m, int nbuf) { return (size_t)nbuf * TILE * m->D * sizeof(double); }

// persistent single-wave workgroups: as many per CU as the LDS tile allows (at most 8), never more than tiles
int row_grid(const zk_rows* m, size_t lds_bytes) {
  // (LDS is handed out in 512-byte granules: a 64 x 45 tile of doubles is exactly 45 of them, and SEVEN fit a CU's 160 KiB)
  int per_cu = (int)((160 * 1024) / ((lds_bytes + 511) & ~(size_t)511));
  per_cu = std::max(1, std::min(per_cu, 8));
  const long long tiles = (m->N + TILE - 1) / TILE;
  return (int)std::min<long long>(tiles, (long long)per_cu * m->n_cu);
}

// page-locked staging area of at least `need` bytes (tables are a few KiB to ~100 KiB)
int ensure_pinned(zk_rows* m, size_t need) {
  if (m->pin_bytes >= need) return 0;
  if (m->ev_up) ZK_HIP(hipEventSynchronize(m->ev_up));
  if (m->h_pin) (void)hipHostFree(m->h_pin);
  m->h_pin = nullptr;
  m->pin_bytes = 0;
  const size_t want = need < 65536 ? 65536 : need;
  ZK_HIP(hipHostMalloc(&m->h_pin, want, hipHostMallocDefault));
  m->pin_bytes = want;
  if (!m->ev_up) ZK_HIP(hipEventCreateWithFlags(&m->ev_up, hipEventDisableTiming));
  return 0;
}

}  // namespace

int zk_check_lds(size_t bytes) {
  if (bytes > 160 * 1024) return zk_fail(ZK_E_BADARG, "too many features / clusters for one 160-KiB LDS tile");
  return 0;
}

int zk_plan_row_pass(const zk_rows* m, size_t extra_lds, zk_row_plan* p) {
  p->nbuf = tile_bufs(m, extra_lds);
  p->lds = tile_lds(m, p->nbuf) + extra_lds;
  const int rc = zk_check_lds(p->lds);
  if (rc) return rc;
  p->grid = row_grid(m, p->lds);
  return 0;
}

// the operand tables of a pass: staged in page-locked memory, so the copy is asynchronous and ordered before the pass's kernels on
// the stream -- no synchronisation here (round 3; a pageable source plus hipStreamSynchronize cost every pass ~25 us of its
// ~100 us of host overhead).  The staging buffer is reused once the previous upload has left it (ev_up).
int zk_upload_tab(zk_rows* m) {
  std::vector<double>& h = m->h_buf;
  const size_t bytes = h.size() * sizeof(double);
  int rc = zk_ensure(&m->d_tab, &m->tab_bytes, bytes);
  if (rc) return rc;
  if ((rc = ensure_pinned(m, bytes))) return rc;
  ZK_HIP(hipEventSynchronize(m->ev_up));  // (complete long ago: every pass ends with a synchronised read-back)
  memcpy(m->h_pin, h.data(), bytes);
  h.clear();
  ZK_HIP(hipMemcpyAsync(m->d_tab, m->h_pin, bytes, hipMemcpyHostToDevice, m->stream));
  ZK_HIP(hipEventRecord(m->ev_up, m->stream));
  return 0;
}

// fixed-order sum of the per-workgroup partial results ([n_blocks][n] in d_part) -> host; two levels (groups of 32 blocks,
// then the groups) so that thousands of partials do not become one thread's serial loop
int zk_reduce_to_host(zk_rows* m, int n_blocks, int n, double* host_out, unsigned long long* counter_out) {
  const int group = 32, n_groups = (n_blocks + group - 1) / group;
  {  // results land in page-locked memory: the copies are asynchronous and ONE synchronisation ends the pass
    const size_t need = (size_t)n * sizeof(double) + sizeof(unsigned long long);
    if (m->res_bytes < need) {
      if (m->h_res) (void)hipHostFree(m->h_res);
      m->h_res = nullptr;
      m->res_bytes = 0;
      const size_t want = need < 16384 ? 16384 : need;
      ZK_HIP(hipHostMalloc(&m->h_res, want, hipHostMallocDefault));
      m->res_bytes = want;
    }
  }
  int rc = zk_ensure(&m->d_red, &m->red_bytes, (size_t)(n_groups + 1) * n * sizeof(double));
  if (rc) return rc;
  double* fin = (double*)m->d_red;
  double* mid = fin + n;
  if (n_groups > 1) {
    hipLaunchKernelGGL(reduce_kernel, dim3((n + 255) / 256, n_groups), dim3(256), 0, m->stream, (const double*)m->d_part, n_blocks, n,
                       group, mid);
    hipLaunchKernelGGL(reduce_kernel, dim3((n + 255) / 256, 1), dim3(256), 0, m->stream, (const double*)mid, n_groups, n, n_groups, fin);
  } else {
    hipLaunchKernelGGL(reduce_kernel, dim3((n + 255) / 256, 1), dim3(256), 0, m->stream, (const double*)m->d_part, n_blocks, n, n_blocks,
                       fin);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(m->h_res, fin, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  if (counter_out)
    ZK_HIP(hipMemcpyAsync((char*)m->h_res + (size_t)n * sizeof(double), m->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          m->stream));
  ZK_HIP(hipStreamSynchronize(m->stream));
  memcpy(host_out, m->h_res, (size_t)n * sizeof(double));
  if (counter_out) memcpy(counter_out, (char*)m->h_res + (size_t)n * sizeof(double), sizeof(unsigned long long));
  return 0;
}

int zk_rows_prof_begin(zk_rows* m) {
  if (m->profile) ZK_HIP(hipEventRecord(m->ev[0], m->stream));
  return 0;
}
int zk_rows_prof_end(zk_rows* m) {
  if (m->profile) ZK_HIP(hipEventRecord(m->ev[1], m->stream));
  return 0;
}
int zk_rows_prof_read(zk_rows* m) {  // after the stream has been synchronised
  if (m->profile) {
    float ms = 0.f;
    ZK_HIP(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]));
    m->last_kernel_ms = ms;
  }
  return 0;
}

int zk_rows_need_labels(zk_rows* m, bool unset) {
  if (m->d_labels) return 0;
  ZK_HIP(hipMalloc((void**)&m->d_labels, (size_t)m->N * sizeof(int32_t)));
  if (unset) ZK_HIP(hipMemsetAsync(m->d_labels, 0xff, (size_t)m->N * sizeof(int32_t), m->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the resident matrix
// ------------------------------------------------------------------------------------------------------------------
static int rows_init(zk_rows* m) {
  ZK_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  (void)hipDeviceGetAttribute(&m->n_cu, hipDeviceAttributeMultiprocessorCount, m->device);
  ZK_HIP(hipMalloc((void**)&m->d_mean, (size_t)m->D * sizeof(double)));
  ZK_HIP(hipMemsetAsync(m->d_mean, 0, (size_t)m->D * sizeof(double), m->stream));
  ZK_HIP(hipMalloc((void**)&m->d_count, 4 * sizeof(unsigned long long)));
  ZK_HIP(hipMemsetAsync(m->d_count, 0, 4 * sizeof(unsigned long long), m->stream));
  return 0;
}

extern "C" int zk_rows_destroy(zk_rows* m) {
  if (!m) return 0;
  ZK_ON_DEVICE(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  if (m->own && m->X) (void)hipFree((void*)m->X);
  void* bufs[] = {m->d_mean, m->d_xsq, m->d_tab, m->d_part, m->d_red, m->d_seed[0], m->d_seed[1], m->d_labels, m->d_resp, m->d_count};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (hipEvent_t e : m->ev)
    if (e) (void)hipEventDestroy(e);
  if (m->ev_up) (void)hipEventDestroy(m->ev_up);
  if (m->h_pin) (void)hipHostFree(m->h_pin);
  if (m->h_res) (void)hipHostFree(m->h_res);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
  return 0;
}

static int rows_new(int device, const double* X_dev, int64_t N, int D, bool own, zk_rows** out) {
  zk_rows* m = new zk_rows;
  m->device = device;
  m->N = N;
  m->D = D;
  m->X = X_dev;
  m->own = own;
  const int rc = rows_init(m);
  if (rc) {
    m->own = false;
    zk_rows_destroy(m);
    return rc;
  }
  *out = m;
  return 0;
}

static int rows_args(const void* X, int64_t N, int D, zk_rows** out) {
  if (!X || !out) return zk_fail(ZK_E_BADARG, "null pointer");
  if (N <= 0 || D <= 0 || D > 127) return zk_fail(ZK_E_BADARG, "need 1 <= D <= 127 features and N > 0 rows");
  *out = nullptr;
  return 0;
}

extern "C" int zk_rows_adopt(int device, const double* X_dev, int64_t N, int D, zk_rows** out) {
  int rc = rows_args(X_dev, N, D, out);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  // every pass runs on the object's own non-blocking stream, which is not ordered against whatever stream is still
  // writing the matrix (zk_transform_patches_dev is asynchronous): wait for the producer here, once
  ZK_HIP(hipDeviceSynchronize());
  return rows_new(device, X_dev, N, D, false, out);
}

extern "C" int zk_rows_create(int device, const double* X_host, int64_t N, int D, zk_rows** out) {
  int rc = rows_args(X_host, N, D, out);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  double* d = nullptr;
  const size_t bytes = (size_t)N * D * sizeof(double);
  ZK_HIP(hipMalloc((void**)&d, bytes));
  // in pieces of 256 MiB on a stream of its own, as the host pipeline of zk_host.hip does: 1.46 GB from a pageable NumPy array
  // in 26 ms (56 GB/s, the PCIe link rate; the first call of a process adds the HIP runtime's start-up, ~0.15 s)
  hipStream_t up = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
  const size_t piece = (size_t)256 << 20;
  for (size_t off = 0; off < bytes && e == hipSuccess; off += piece)
    e = hipMemcpyAsync((char*)d + off, (const char*)X_host + off, std::min(piece, bytes - off), hipMemcpyHostToDevice, up);
  if (e == hipSuccess) e = hipStreamSynchronize(up);
  if (up) (void)hipStreamDestroy(up);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return zk_hip_fail(e, "hipMemcpy(X)");
  }
  rc = rows_new(device, d, N, D, true, out);
  if (rc) (void)hipFree(d);
  return rc;
}

extern "C" const double* zk_rows_data(const zk_rows* m) { return m ? m->X : nullptr; }

// Column sums of the matrix (first pass of numpy.mean).
extern "C" int zk_rows_colsum(zk_rows* m, double* sums_out) {
  if (!m || !sums_out) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(m->device);
  zk_row_plan p;
  int rc = zk_plan_row_pass(m, 0, &p);
  if (rc || (rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)p.grid * m->D * sizeof(double)))) return rc;
  if ((rc = zk_launch_row_pass(colsum_kernel, m, p, (const double*)nullptr, 0, (double*)m->d_part))) return rc;
  return zk_reduce_to_host(m, p.grid, m->D, sums_out);
}

// `mean` (D) becomes the centring shift of every later k-means call (scikit-learn subtracts the column means before
// clustering; with several ranks it is the mean over all of them); sqsum_out[j] = sum_r (x_rj - mean_j)^2 (second pass of
// numpy.var), the squared norms of the centred rows stay on the device, n_bad_out = rows with a non-finite element.
extern "C" int zk_rows_center_at(zk_rows* m, const double* mean, double* sqsum_out, int64_t* n_bad_out) {
  if (!m || !mean || !sqsum_out || !n_bad_out) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(m->device);
  zk_row_plan p;
  int rc = zk_plan_row_pass(m, 0, &p);
  if (rc || (rc = zk_ensure(&m->d_part, &m->part_bytes, (size_t)p.grid * m->D * sizeof(double)))) return rc;
  ZK_HIP(hipMemcpyAsync(m->d_mean, mean, (size_t)m->D * sizeof(double), hipMemcpyHostToDevice, m->stream));
  ZK_HIP(hipStreamSynchronize(m->stream));
  if ((rc = zk_launch_row_pass(colsum_kernel, m, p, (const double*)m->d_mean, 1, (double*)m->d_part))) return rc;
  if ((rc = zk_reduce_to_host(m, p.grid, m->D, sqsum_out))) return rc;
  if (!m->d_xsq) ZK_HIP(hipMalloc((void**)&m->d_xsq, (size_t)m->N * sizeof(double)));
  ZK_HIP(hipMemsetAsync(m->d_count, 0, sizeof(unsigned long long), m->stream));
  if ((rc = zk_launch_row_pass(rownorm_kernel, m, p, (const double*)m->d_mean, m->d_xsq, m->d_count))) return rc;
  unsigned long long bad = 0;
  ZK_HIP(hipMemcpyAsync(&bad, m->d_count, sizeof(bad), hipMemcpyDeviceToHost, m->stream));
  ZK_HIP(hipStreamSynchronize(m->stream));
  *n_bad_out = (int64_t)bad;
  return 0;
}

// Column means (mean_out) and population variances about them (var_out), two passes as numpy.mean / numpy.var, of THIS
// matrix alone (= zk_rows_colsum, division, zk_rows_center_at, division).
extern "C" int zk_rows_center(zk_rows* m, double* mean_out, double* var_out, int64_t* n_bad_out) {
  if (!m || !mean_out || !var_out || !n_bad_out) return zk_fail(ZK_E_BADARG, "null pointer");
  int rc = zk_rows_colsum(m, mean_out);
  if (rc) return rc;
  for (int j = 0; j < m->D; ++j) mean_out[j] /= (double)m->N;
  if ((rc = zk_rows_center_at(m, mean_out, var_out, n_bad_out))) return rc;
  for (int j = 0; j < m->D; ++j) var_out[j] /= (double)m->N;
  return 0;
}

// rows idx[0..n) of the matrix, minus the centring shift when `centred`, to the host
extern "C" int zk_rows_fetch(zk_rows* m, const int64_t* idx, int n, int centred, double* rows_out) {
  if (!m || !idx || !rows_out || n < 0) return zk_fail(ZK_E_BADARG, "bad arguments");
  ZK_ON_DEVICE(m->device);
  for (int i = 0; i < n; ++i) {
    if (idx[i] < 0 || idx[i] >= m->N) return zk_fail(ZK_E_BADARG, "row index out of range");
    ZK_HIP(hipMemcpyAsync(rows_out + (size_t)i * m->D, m->X + idx[i] * m->D, (size_t)m->D * sizeof(double), hipMemcpyDeviceToHost,
                          m->stream));
  }
  ZK_HIP(hipStreamSynchronize(m->stream));
  if (centred) {
    std::vector<double> mean(m->D);
    ZK_HIP(hipMemcpy(mean.data(), m->d_mean, (size_t)m->D * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < m->D; ++j) rows_out[(size_t)i * m->D + j] -= mean[j];
  }
  return 0;
}

// HIP-event timing of the main kernel of the next zk_kmeans_step calls (bench.py's roofline of the Lloyd pass)
extern "C" int zk_rows_profile(zk_rows* m, int enable) {
  if (!m) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(m->device);
  if (enable && !m->ev[0]) {
    ZK_HIP(hipEventCreate(&m->ev[0]));
    ZK_HIP(hipEventCreate(&m->ev[1]));
  }
  m->profile = enable != 0;
  return 0;
}
extern "C" double zk_rows_last_kernel_ms(const zk_rows* m) { return m ? m->last_kernel_ms : 0.0; }

// forget the labels (a new run starts from labels_old = -1)
extern "C" int zk_rows_reset_labels(zk_rows* m) {
  if (!m) return zk_fail(ZK_E_BADARG, "null pointer");
  ZK_ON_DEVICE(m->device);
  if (m->d_labels) ZK_HIP(hipMemsetAsync(m->d_labels, 0xff, (size_t)m->N * sizeof(int32_t), m->stream));
  return 0;
}

extern "C" int zk_rows_labels(zk_rows* m, int32_t* labels_host) {
  if (!m || !labels_host) return zk_fail(ZK_E_BADARG, "null pointer");
  if (!m->d_labels) return zk_fail(ZK_E_BADARG, "no labels yet");
  ZK_ON_DEVICE(m->device);
  ZK_HIP(hipMemcpyAsync(labels_host, m->d_labels, (size_t)m->N * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
  ZK_HIP(hipStreamSynchronize(m->stream));
  return 0;
}

extern "C" const int32_t* zk_rows_labels_dev(const zk_rows* m) { return m ? m->d_labels : nullptr; }

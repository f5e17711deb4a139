// zk_synth.hip -- linear synthesis out = C . T on the matrix cores: the device side of ZPs.inverse_transform (no reference
// counterpart: the reference cannot go back from moments to patches).
//
//   C   (N, P)   float64, row-major: one row of coefficients per output patch
//   T   (P, X)   float64, resident: the synthesis table (X = K^2 pixels; for the Zernike inverse G^-1 diag(s) B or diag(s) B,
//                computed by the caller), its P padded with zero rows to a multiple of 4 at upload
//   out (N, X)   float64 or float32, rounded once from the float64 accumulator
//
// The mirror image of the batch transform: a thin product whose cost is the N X output stream.  v_mfma_f64_16x16x4_f64 with
//   A[i][k] = C[row 16 rb + i][4 step + k]   lane (i = lane & 15, k = lane >> 4), from the workgroup's coefficient tile in LDS
//   B[k][j] = T[4 step + k][col 16 cb + j]   lane (k = lane >> 4, j = lane & 15), from global memory: the table (360 KiB at
//                                            (32 px, n_max 8), 2.9 MiB at (64, 12)) stays in L2 and is reread from there
//   D[i][j]  : lane holds (row (lane >> 4) + 4 q, col lane & 15), q = 0 .. 3
// workgroup = 4 waves = 64 rows x 256 columns, wave = 64 rows (4 blocks of 16) x 64 columns (4 blocks of 16): a B operand
// feeds 4 MFMAs, an A operand 4, and a step's B loads are issued a step ahead of its MFMAs.  The 16 lanes that share an
// output row write one contiguous 128-B segment (64 B for float32 output), non-temporally.  P above ZK_SYNTH_KC goes through
// the tile in slices of ZK_SYNTH_KC coefficients with the accumulators kept.
// No atomics, and a row's sum does not depend on where the row lies in the batch: two runs, and two chunkings, agree bit for bit.
#include <new>

#include "zk_ring.h"

#define ZK_SYNTH_ROWS 64
#define ZK_SYNTH_COLS 256
#define ZK_SYNTH_KC 96                    // coefficients of a row held in LDS at a time
#define ZK_SYNTH_PITCH (ZK_SYNTH_KC + 2)  // doubles; pitch = 2 mod 32: the 32 lanes (i, k < 2) of a half-wave read 32 different bank pairs

struct zk_synth {
  int device = 0;
  int n_funcs = 0;
  int p_pad = 0;          // n_funcs rounded up to a multiple of 4
  int64_t n_pixels = 0;
  double* d_table = nullptr;  // (p_pad, n_pixels)
  size_t host_chunk = 0;      // bytes of coefficients + output per chunk of the host variant; 0 = default
  zk_stage stage;             // the host variant (zk_ring.h): its kernel stream; coefficients up, patches down
};

namespace {

template <typename TOUT>
__global__ __launch_bounds__(256) void zk_synth_kernel(const double* __restrict__ coeffs, const double* __restrict__ table,
                                                       TOUT* __restrict__ out, long long n_rows, int n_funcs, int p_pad,
                                                       long long n_pixels) {
  typedef double v4d __attribute__((ext_vector_type(4)));
  __shared__ double tile[ZK_SYNTH_ROWS * ZK_SYNTH_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int li = lane & 15, kr = lane >> 4;
  const long long row0 = (long long)blockIdx.y * ZK_SYNTH_ROWS;
  const long long col0 = (long long)blockIdx.x * ZK_SYNTH_COLS + wave * 64;
  const bool live = col0 < n_pixels;  // wave-uniform; a wave past the last column keeps the barriers and its share of the staging
  bool col_ok[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) col_ok[cb] = col0 + 16 * cb + li < n_pixels;

  v4d acc[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = v4d{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < p_pad; k0 += ZK_SYNTH_KC) {
    const int kc = p_pad - k0 < ZK_SYNTH_KC ? p_pad - k0 : ZK_SYNTH_KC;  // a multiple of 4
    if (k0) __syncthreads();                                             // every wave is done with the slice before
    // rows past the batch and coefficients past n_funcs are zero; a wave takes every fourth row of the tile, its lanes the row's
    // consecutive coefficients (with one slice the rows of a tile are one contiguous run of the matrix)
#pragma unroll 4
    for (int r = wave; r < ZK_SYNTH_ROWS; r += 4) {
      const long long row = row0 + r;
      for (int c = lane; c < kc; c += 64) {
        double v = 0.0;
        if (row < n_rows && k0 + c < n_funcs) v = coeffs[row * n_funcs + k0 + c];
        tile[r * ZK_SYNTH_PITCH + c] = v;
      }
    }
    __syncthreads();
    if (live) {
      const double* __restrict__ tp = table + (long long)(k0 + kr) * n_pixels + col0 + li;
      const double* __restrict__ ap = tile + li * ZK_SYNTH_PITCH + kr;
      double b[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) b[cb] = col_ok[cb] ? tp[16 * cb] : 0.0;
      for (int ks = 0; ks < kc; ks += 4) {
        double bn[4] = {0.0, 0.0, 0.0, 0.0};
        if (ks + 4 < kc) {
          const double* __restrict__ tn = tp + (long long)(ks + 4) * n_pixels;
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) bn[cb] = col_ok[cb] ? tn[16 * cb] : 0.0;
        }
        double a[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) a[rb] = ap[rb * 16 * ZK_SYNTH_PITCH + ks];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rb], b[cb], acc[rb][cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) b[cb] = bn[cb];
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long row = row0 + 16 * rb + kr + 4 * q;
      if (row < n_rows) {
        TOUT* __restrict__ dst = out + row * n_pixels + col0 + li;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (col_ok[cb]) __builtin_nontemporal_store((TOUT)acc[rb][cb][q], dst + 16 * cb);
      }
    }
}

template <typename TOUT>
int launch_t(const zk_synth* s, const double* coeffs, int64_t n_rows, TOUT* out, hipStream_t stream) {
  const unsigned col_groups = (unsigned)((s->n_pixels + ZK_SYNTH_COLS - 1) / ZK_SYNTH_COLS);
  const int64_t round_max = (int64_t)65535 * ZK_SYNTH_ROWS;  // grid.y
  for (int64_t first = 0; first < n_rows; first += round_max) {
    const int64_t n = n_rows - first < round_max ? n_rows - first : round_max;
    dim3 grid(col_groups, (unsigned)((n + ZK_SYNTH_ROWS - 1) / ZK_SYNTH_ROWS));
    hipLaunchKernelGGL(zk_synth_kernel<TOUT>, grid, dim3(256), 0, stream, coeffs + first * s->n_funcs, s->d_table,
                       out + first * s->n_pixels, (long long)n, s->n_funcs, s->p_pad, (long long)s->n_pixels);
    ZK_HIP(hipGetLastError());
  }
  return 0;
}

int launch(const zk_synth* s, const double* coeffs, int64_t n_rows, int out_dtype, void* out, hipStream_t stream) {
  if (out_dtype == ZK_F32) return launch_t<float>(s, coeffs, n_rows, (float*)out, stream);
  return launch_t<double>(s, coeffs, n_rows, (double*)out, stream);
}

int check_apply(const zk_synth* s, const void* coeffs, int64_t n_rows, int out_dtype, const void* out, const char* where) {
  if (!s) return zk_fail(ZK_E_BADARG, "null synthesis object");
  if (out_dtype != ZK_F32 && out_dtype != ZK_F64) return zk_fail(ZK_E_BADARG, "out_dtype must be ZK_F32 or ZK_F64");
  if (n_rows < 0) return zk_fail(ZK_E_BADARG, "negative row count");
  if (n_rows > 0 && (!coeffs || !out)) return zk_fail(ZK_E_BADARG, std::string("null ") + where + " pointer");
  return 0;
}

void release(zk_synth* s) {
  zk_stage_destroy(&s->stage);
  if (s->d_table) (void)hipFree(s->d_table);
  delete s;
}

int build(zk_synth* s, const double* table_host) {
  const size_t live = (size_t)s->n_funcs * s->n_pixels * sizeof(double), all = (size_t)s->p_pad * s->n_pixels * sizeof(double);
  ZK_HIP(hipMalloc((void**)&s->d_table, all));
  ZK_HIP(hipMemcpy(s->d_table, table_host, live, hipMemcpyHostToDevice));
  if (all > live) ZK_HIP(hipMemset((char*)s->d_table + live, 0, all - live));
  const int rc = zk_stage_create(&s->stage);
  if (rc) return rc;
  ZK_HIP(hipDeviceSynchronize());  // the table is in place before any stream of any caller reads it
  return 0;
}

}  // namespace

extern "C" int zk_synth_create(int device, int n_funcs, int64_t n_pixels, const double* table_host, zk_synth** out) {
  if (!out) return zk_fail(ZK_E_BADARG, "out is null");
  *out = nullptr;
  if (n_funcs < 1 || n_funcs > 4096) return zk_fail(ZK_E_BADARG, "n_funcs must be between 1 and 4096");
  if (n_pixels < 1 || n_pixels > ((int64_t)1 << 24)) return zk_fail(ZK_E_BADARG, "n_pixels must be between 1 and 2^24");
  if (!table_host) return zk_fail(ZK_E_BADARG, "null table pointer");
  int rc = zk_check_device(device);
  if (rc) return rc;
  ZK_ON_DEVICE(device);
  zk_synth* s = new (std::nothrow) zk_synth();
  if (!s) return zk_fail(ZK_E_NOMEM, "out of host memory");
  s->device = device;
  s->n_funcs = n_funcs;
  s->p_pad = (n_funcs + 3) & ~3;
  s->n_pixels = n_pixels;
  if ((rc = build(s, table_host))) {
    release(s);
    return rc;
  }
  *out = s;
  return 0;
}

extern "C" int zk_synth_destroy(zk_synth* s) {
  if (!s) return 0;
  ZK_ON_DEVICE(s->device);
  (void)hipStreamSynchronize(s->stage.stream);
  release(s);  // waits for the copy streams
  return 0;
}

extern "C" int zk_synth_set_host_chunk(zk_synth* s, int64_t chunk_bytes) {
  if (!s || chunk_bytes < 0) return zk_fail(ZK_E_BADARG, "bad arguments");
  s->host_chunk = (size_t)chunk_bytes;
  return 0;
}

extern "C" int zk_synth_apply_dev(zk_synth* s, const double* coeffs_dev, int64_t n_rows, int out_dtype, void* out_dev, void* hip_stream) {
  const int rc = check_apply(s, coeffs_dev, n_rows, out_dtype, out_dev, "device");
  if (rc) return rc;
  if (n_rows == 0) return 0;
  ZK_ON_DEVICE(s->device);
  return launch(s, coeffs_dev, n_rows, out_dtype, out_dev, (hipStream_t)hip_stream);  // exactly the caller's stream
}

extern "C" int zk_synth_apply(zk_synth* s, const double* coeffs_host, int64_t n_rows, int out_dtype, void* out_host) {
  int rc = check_apply(s, coeffs_host, n_rows, out_dtype, out_host, "host");
  if (rc) return rc;
  if (n_rows == 0) return 0;
  ZK_ON_DEVICE(s->device);
  zk_ring* r = &s->stage.ring;
  const hipStream_t stream = s->stage.stream;
  const size_t in_unit = (size_t)s->n_funcs * sizeof(double), out_unit = (size_t)s->n_pixels * zk_elem_size(out_dtype);
  const size_t budget = s->host_chunk ? s->host_chunk : (size_t)256 << 20;
  const zk_chunks ch = zk_chunk_plan(budget, in_unit + out_unit, ZK_SYNTH_ROWS, n_rows);  // whole row tiles
  rc = zk_ring_run(
      r, stream, ch.n_chunks,
      [&](int64_t c, int slot) -> int {
        int e = zk_ring_slot(r, slot, (size_t)ch.chunk * in_unit, (size_t)ch.chunk * out_unit);
        if (!e) e = zk_ring_up(r, stream, c, slot, r->d_in[slot], coeffs_host + (size_t)ch.first(c) * s->n_funcs, (size_t)ch.count(c) * in_unit);
        return e ? e : launch(s, (const double*)r->d_in[slot], ch.count(c), out_dtype, r->d_out[slot], stream);
      },
      [&](int64_t c, int slot) -> int {
        return zk_ring_down(r, slot, (char*)out_host + (size_t)ch.first(c) * out_unit, (size_t)ch.count(c) * out_unit);
      });
  zk_stage_trim(&s->stage, ZK_STAGE_KEEP_ROWS);  // callers hold one object per table, several at a time
  return rc;
}

/*
 * zernike_hip.h -- C ABI of libzernike_hip.so, the MI355X (gfx950) implementation of
 * motif-learn's per-patch Zernike-moment hot path.
 *
 * The reference (jiadongdan/motif-learn, pure Python) has no native interface; its boundary is
 * the Python class `mtflearn.features.ZPs`.  Each entry point below replaces the arithmetic of
 * one reference method and is what a maintainer would bind with ctypes from inside that method
 * (binding stub: INTEGRATION.md):
 *
 *   zk_plan_create            <- ZPs.__init__ keeps `self.polynomials`            (_zps.py:48-50)
 *   zk_transform_patches      <- ZPs._transform_dot_product                       (_zps.py:146-157)
 *   zk_transform_frame        <- ZPs._transform_fft_convolve                      (_zps.py:159-193)
 *   zk_*_dev                  <- same, operands already resident in HBM (bench / multi-GPU)
 *   zk_transform_points       <- KeyPoints.extract_patches + ZPs.transform        (_keypoint.py:60-78)
 *   zk_frame_maps             <- zmoments.to_complex / rot_maps / mirror_map      (_zmoments.py:300-316, 420-493)
 *   zk_autocorr_mean, zk_polar_profile        <- estimate_patch_size, radial_profile  (_patch_size.py:48-100, 221-302)
 *   zk_power_spectra, zk_denoise_fft          <- _get_cumulative_energy, denoise_fft   (_estimate_n_max.py:8-86,
 *                                                                                      denoise/_denoise_fft.py:4-47)
 *   zk_circular_autocorr, zk_char_length      <- compute_autocorrelation, get_characteristic_length (_window_size.py:16-46)
 *   zk_char_length_fft                        <- get_characteristic_length_fft                      (_window_size.py:65-80)
 *   zk_shifted_magnitude, zk_angular_average  <- fft_power_spectrum, angular_average                (_fft_related.py:4-66)
 *   zk_comm_*, zk_allgather_rows              (no counterpart: the multi-GPU exchange of north_star)
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative code
 *     (-hipError_t for runtime failures, ZK_E_* for argument errors) and never throws;
 *     zk_last_error_string() describes the most recent failure on the calling thread.
 *   - the caller owns every host buffer; inputs are read-only, outputs are C-contiguous
 *     float64; no pointer is retained after the call returns.  Device memory owned by the
 *     library lives inside the plan and is released by zk_plan_destroy().
 *   - a plan is bound to one device and is not thread-safe (one stream per plan).  Every entry point
 *     leaves the calling thread's current HIP device as it found it.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails.
 */
#ifndef ZERNIKE_HIP_H
#define ZERNIKE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_ABI_VERSION 2

/* element type of the image / patch operand */
#define ZK_F32 0
#define ZK_F64 1
/* Narrow detector formats, accepted by the HOST-buffer entry points only (zk_transform_patches / _frame / _points,
 * zk_frame_maps): the bytes cross PCIe as they are (1-2 B per pixel instead of 4) and are widened to float32 on the
 * device, which is exact -- the moments equal those of NumPy's float64 promotion of the same integers
 * (reference _zps.py:151-155 upcasts whatever dtype it is given). */
#define ZK_U8  2
#define ZK_U16 3
#define ZK_I16 4
#define ZK_I32 5  /* int32 key points, what zk_local_max writes: accepted by zk_voronoi_cells and zk_knn_distances only */

/* argument-error codes (runtime failures are -hipError_t, i.e. -1 .. -1999) */
#define ZK_E_BADARG   (-10001)
#define ZK_E_NODEVICE (-10002)
#define ZK_E_NOMEM    (-10003)
#define ZK_E_COMM     (-10004)  /* RCCL unavailable, rendezvous failed or a collective returned an error */
#define ZK_E_FFT      (-10005)  /* hipFFT unavailable or a transform failed */

/* kernel selection, for tests and A/B measurements.  Default ZK_PATH_AUTO = the fastest family that restates the reference
 * to SURVEY 8c's criterion (elementwise rtol 1e-6, floor 1e-12 max|Z| up to n_max 12, 1e-11 above) on the reference's own
 * outputs: the polynomial kernels (SEPARABLE / STREAM) for full Zernike sets up to n_max 16, the plain sum on the matrix
 * cores (DIRECT) from n_max 17 and for every other set of >= 92 functions, else FOLDED / GENERIC. */
#define ZK_PATH_AUTO      0
#define ZK_PATH_GENERIC   1  /* any size / n_max / dtype: unfolded direct summation, one output per lane, ~1e-16 of the definition */
#define ZK_PATH_FOLDED    2  /* frame only: mirror-folded direct summation (4x fewer FMAs), ~1e-15            */
#define ZK_PATH_SEPARABLE 3  /* mirror-folded row-separable sums (Legendre products), ~1e-13; fastest.  Full
                                Zernike sets up to n_max 24 (17-24: one pass per mirror-parity class; ~1e-9 at 20, ~3e-8 at 24,
                                which is the rounding of the reference's own float64 basis there) */
#define ZK_PATH_STREAM    4  /* patches only: row-separable sums over the contiguous pixel stream of a patch,
                                whole 128-B lines whatever the patch size; AUTO prefers it where the row-pair
                                kernel of ZK_PATH_SEPARABLE would issue half-line requests */
#define ZK_PATH_DIRECT    5  /* sets of >= 92 functions (n_max >= 13), windows of 16 .. 512 px: the plain sum over the CALLER'S
                                basis values as a float64 GEMM on the matrix cores (v_mfma_f64_16x16x4_f64) -- the reference's
                                own arithmetic (np.dot, _zps.py:155), ~1e-15, at any order.  Dense mode multiplies window pixel
                                (r, c) with (-1)^n V(K-1-r, K-1-c), which is what the reference's convolution + sign fix does
                                (_zps.py:165-178; equal to V(r, c) for an exactly point-symmetric basis), whenever the set is
                                point-symmetric to 1e-6.  SEPARABLE stays available as an explicit opt-in above n_max 16:
                                2-6x faster, ~1e-10 (n_max 20) .. 1e-9 (n_max 24) of max|Z| from the reference's result */

typedef struct zk_plan zk_plan;

/* Library / device discovery. */
int         zk_abi_version(void);
int         zk_device_count(void);            /* >= 0, or a negative code               */
const char* zk_last_error_string(void);

/*
 * Create a plan for one (size, n_poly) basis on `device`.
 *   basis : host, (n_poly, size, size) float64, C order -- ZPs.polynomials      (_zps.py:90)
 *   n, m  : host, (n_poly) int32 radial order / azimuthal frequency per basis function, in
 *           the order of `basis`                                                  (_zps.py:74-81)
 * The plan uploads the disk-masked basis, pre-divided by the reference's normalising area
 * pi*size^2/4 (_zps.py:154,177).  When (n, m, basis) is the reference's full real Zernike set
 * it also builds the mirror-folded table and the row-separable (Legendre) tables of the fast
 * kernels, after verifying that they reproduce `basis` at every pixel of the disk.
 */
int  zk_plan_create(int size, int n_poly, const int32_t* n, const int32_t* m,
                    const double* basis, int device, zk_plan** out);
void zk_plan_destroy(zk_plan* plan);

/* Introspection: 1 if `path` (ZK_PATH_*) is available for `mode` (0 patches, 1 frame) and `dtype`. */
int zk_plan_has_path(const zk_plan* plan, int mode, int dtype, int path);
/* 1 if the plan has the single-kernel form of zk_transform_points (ZK_OP_POINTS: full Zernike set, n_max <= 16) /
 * the kernels behind zk_frame_maps (ZK_OP_MAPS: full Zernike set, n_max <= 40; fused in one kernel up to 16, moments into a
 * scratch matrix + a planes kernel above)
 * for `dtype`.  (No reference counterpart: the reference composes these from ZPs.transform.) */
#define ZK_OP_POINTS 1
#define ZK_OP_MAPS   2
int zk_plan_supports(const zk_plan* plan, int op, int dtype);
/* Number of pixels inside the unit disk (rho <= 1 as evaluated by the caller's basis). */
int zk_plan_disk_pixels(const zk_plan* plan);
/* The family (ZK_PATH_*, never AUTO) a transform of `n_units` patches (mode 0) / of a frame (mode 1) would run on with the
 * plan's current setting: what ZK_PATH_AUTO resolves to, or the forced path; -1 if a forced path is unavailable. */
int zk_plan_resolved_path(const zk_plan* plan, int mode, int dtype, int64_t n_units);
/* Force a kernel family (ZK_PATH_*); a forced path that is unavailable makes transforms fail. */
int zk_plan_set_path(zk_plan* plan, int path);

/*
 * Batch of patches (reference _zps.py:146-157):
 *   out[p, j] = sum_{r,c} patches[p, r, c] * basis[j, r, c] / (pi size^2 / 4)
 *   patches : (N, size, size) of `dtype`, C order;  out : (N, n_poly) float64.
 * Host variant copies in/out through staging buffers owned by the plan, on the plan's stream,
 * and returns when the result is in out_host.  The *_dev variants enqueue the kernel on exactly
 * `hip_stream` (a hipStream_t; NULL = HIP's default stream) and return without synchronising.
 */
int zk_transform_patches(zk_plan* plan, const void* patches_host, int dtype, int64_t n_patches,
                         double* out_host);
int zk_transform_patches_dev(zk_plan* plan, const void* patches_dev, int dtype,
                             int64_t n_patches, double* out_dev, void* hip_stream);

/*
 * Dense frame (reference _zps.py:159-193, i.e. fftconvolve(mode='same') * (-1)^n / area):
 *   out[j, i, k] = (-1)^n[j] * sum_{r,c} pad(image)[i - ea + r, k - ea + c] * basis[j, size-1-r, size-1-c] / (pi size^2/4)
 *   with eb = (size-1)/2, ea = size-1-eb and zero padding outside the image -- the convolution and the sign fix
 *   of the reference written out.  For a point-symmetric basis (V(-x, -y) = (-1)^n V(x, y): every Zernike set in exact
 *   arithmetic) this is the inner product of the window with basis[j]; the reference's float64 basis is point-symmetric
 *   only up to rounding (1e-13 of max|V| at n_max 10, 1e-8 at 24, 8e-4 at 36), and the kernels that sum the caller's own
 *   numbers (ZK_PATH_GENERIC, ZK_PATH_DIRECT) follow the formula above to the letter; the polynomial kernels
 *   (ZK_PATH_SEPARABLE / FOLDED, verified Zernike sets only) evaluate the exactly symmetric polynomial.
 *   image : (H, W) of `dtype`;  out : (n_poly, H, W) float64 (moment-major, as the reference).
 * The *_dev variant computes output rows [row0, row0+n_rows) only and writes them to
 * out_dev laid out as (n_poly, n_rows, W) -- the row-band shard of one GPU; the image operand
 * is always the whole frame.
 */
int zk_transform_frame(zk_plan* plan, const void* image_host, int dtype, int64_t height,
                       int64_t width, double* out_host);
int zk_transform_frame_dev(zk_plan* plan, const void* image_dev, int dtype, int64_t height,
                           int64_t width, int64_t row0, int64_t n_rows, double* out_dev,
                           void* hip_stream);

/*
 * Row band written IN PLACE into a larger array: as zk_transform_frame_dev, but plane j of the band starts
 * at out_dev + j * plane_stride (doubles).  With out_dev = full + row0 * W and plane_stride = H * W the
 * band lands inside the full (n_poly, H, W) array -- the layout zk_allgather_rows reassembles without a copy.
 */
int zk_transform_frame_dev_strided(zk_plan* plan, const void* image_dev, int dtype, int64_t height,
                                   int64_t width, int64_t row0, int64_t n_rows, double* out_dev,
                                   int64_t plane_stride, void* hip_stream);

/*
 * Moments of the size x size windows at given positions of a frame: the device form of "cut patches at
 * key points, then transform the batch" (reference features/_keypoint.py:60-78 + _zps.py:146-157)
 * without materialising the (N, size, size) batch.
 *   points : (n_points, 2) int32 (x, y) = (column, row); the window is
 *            image[y - size/2 : y - size/2 + size, x - size/2 : x - size/2 + size]  (pixels outside the
 *            frame read as zero; the reference's KeyPoints drops such points beforehand)
 *   out    : (n_points, n_poly) float64
 * Plans with the key-point kernel (zk_plan_supports(plan, ZK_OP_POINTS, dtype): full Zernike set, n_max <= 16)
 * read the windows straight from the frame; the others cut them on the device into a plan-owned batch
 * (<= 1 GiB at a time) and run the batch path on it.
 */
int zk_transform_points(zk_plan* plan, const void* image_host, int dtype, int64_t height, int64_t width,
                        const int32_t* points_host, int64_t n_points, double* out_host);
int zk_transform_points_dev(zk_plan* plan, const void* image_dev, int dtype, int64_t height, int64_t width,
                            const int32_t* points_dev, int64_t n_points, double* out_dev, void* hip_stream);

/*
 * Fused dense pipeline: frame -> per-pixel symmetry maps, without writing the (n_poly, H, W) moments
 * to memory (reference notebook-3 tail: zmoments.to_complex / rot_maps / mirror_map,
 * _zmoments.py:300-316, 420-493).  Any of the three outputs may be NULL.
 *   abs_out    : (N_c, n_rows, W)      |Z_{n,m} + i Z_{n,-m}| of the raw moments, (n, m>=0) in the
 *                                      order of to_complex(), N_c = number of (n, |m|) pairs
 *   rot_out    : (n_folds, n_rows, W)  zmoments.rot_maps(folds, p, m_unselect); n_folds <= 8
 *   mirror_out : (n_rows, W)           zmoments.mirror_map(theta, p, m_unselect)
 *   m_unselect : |m| values to drop (must contain 0; reference default (0, 1));  p_norm: 2, or 0 for None
 *   theta      : host, n_theta angles in radians (reference default linspace(0, 2 pi, 360, endpoint=False))
 * Needs the row-separable tables (zk_plan_has_path(plan, 1, dtype, ZK_PATH_SEPARABLE)); otherwise fails
 * and the caller composes zk_transform_frame with the host-side container methods.
 * The *_dev variant returns without synchronising, except on the FIRST call with a new (folds, m_unselect, theta)
 * option set: that call uploads a small table with a blocking copy (the plan keeps the tables of the 8 most
 * recently used option sets, so a launch in flight never sees its table overwritten).
 */
int zk_frame_maps(zk_plan* plan, const void* image_host, int dtype, int64_t height, int64_t width,
                  const int32_t* folds, int n_folds, const int32_t* m_unselect, int n_unselect, int p_norm,
                  const double* theta, int n_theta, double* rot_host, double* abs_host, double* mirror_host);
int zk_frame_maps_dev(zk_plan* plan, const void* image_dev, int dtype, int64_t height, int64_t width,
                      int64_t row0, int64_t n_rows, const int32_t* folds, int n_folds,
                      const int32_t* m_unselect, int n_unselect, int p_norm, const double* theta, int n_theta,
                      double* rot_dev, double* abs_dev, double* mirror_dev, void* hip_stream);

/*
 * The same tail on a BATCH of moment vectors -- zmoments.to_complex / rot_maps / mirror_map on rank-2 data (reference
 * _zmoments.py:300-316, 420-493), e.g. the moments at key points:
 *   moments (N, n_poly) row-major ->  rot (N, n_folds), abs (N, N_c), mirror (N)   (any output may be NULL)
 * zk_points_maps = zk_transform_points followed by that tail with the (N, n_poly) matrix never leaving the device
 * (the reference's notebook flow KeyPoints.extract_patches -> ZPs.transform -> rot_maps).  Full Zernike sets, n_max <= 40.
 */
int zk_moment_maps(zk_plan* plan, const double* moments_host, int64_t n_rows, const int32_t* folds, int n_folds,
                   const int32_t* m_unselect, int n_unselect, int p_norm, const double* theta, int n_theta,
                   double* rot_host, double* abs_host, double* mirror_host);
int zk_moment_maps_dev(zk_plan* plan, const double* moments_dev, int64_t n_rows, const int32_t* folds, int n_folds,
                       const int32_t* m_unselect, int n_unselect, int p_norm, const double* theta, int n_theta,
                       double* rot_dev, double* abs_dev, double* mirror_dev, void* hip_stream);
int zk_points_maps(zk_plan* plan, const void* image_host, int dtype, int64_t height, int64_t width,
                   const int32_t* points_host, int64_t n_points, const int32_t* folds, int n_folds,
                   const int32_t* m_unselect, int n_unselect, int p_norm, const double* theta, int n_theta,
                   double* rot_host, double* abs_host, double* mirror_host);

/* As zk_frame_maps_dev with every output plane `plane_stride` doubles apart (see zk_transform_frame_dev_strided);
 * rot_dev / abs_dev / mirror_dev point at the first row of the band inside their full arrays. */
int zk_frame_maps_dev_strided(zk_plan* plan, const void* image_dev, int dtype, int64_t height, int64_t width,
                              int64_t row0, int64_t n_rows, const int32_t* folds, int n_folds,
                              const int32_t* m_unselect, int n_unselect, int p_norm, const double* theta,
                              int n_theta, double* rot_dev, double* abs_dev, double* mirror_dev,
                              int64_t plane_stride, void* hip_stream);

/*
 * Kernel timing with HIP events on the stream the kernels are launched on.
 * zk_plan_profile(plan, 1) brackets every subsequent kernel launch with an event pair;
 * zk_plan_profile_read() synchronises, returns the launch count and summed kernel
 * milliseconds since the last read, and resets the counters.
 */
int zk_plan_profile(zk_plan* plan, int enable);
int zk_plan_profile_read(zk_plan* plan, int64_t* launches, double* total_ms);
/* Same, launch by launch: the first `cap` kernel times (ms, in launch order) since the last read go to ms_out; *n_out =
 * the number of launches RECORDED since the last read -- larger than `cap` when the list handed back is incomplete (the
 * rest is dropped; bench.py: minimum / median / maximum of the timed steps). */
int zk_plan_profile_read_launches(zk_plan* plan, double* ms_out, int64_t cap, int64_t* n_out);

/*
 * Host staging of the host-buffer entry points (zk_transform_patches / _frame / _points, zk_frame_maps): the
 * job is cut into chunks of at most `chunk_bytes` of input + output (default 256 MiB, ZK_HOST_CHUNK_MB in the
 * environment), each chunk goes host -> pinned ring -> device -> kernel -> pinned ring -> host with the
 * three stages of consecutive chunks overlapping on three streams; the device footprint is bounded by the
 * ring, whatever the job size.  zk_plan_release_staging frees the ring and every grown staging buffer
 * (they are re-created on demand).
 */
int zk_plan_set_host_chunk(zk_plan* plan, int64_t chunk_bytes);
int zk_plan_release_staging(zk_plan* plan);
/* Page-locked host memory (hipHostMalloc, portable): arrays in it move over PCIe by DMA at link speed and
 * without blocking the calling thread; free with zk_host_free. */
int zk_host_alloc(int64_t bytes, void** out_host);
int zk_host_free(void* host);

/* ------------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, units sharded with no data-path collective, ONE exchange step that
 * reassembles the result on every rank (north_star "a single RCCL all-gather over xGMI").
 * The reference has no counterpart (single-process NumPy).  RCCL is loaded on first use (dlopen of the
 * librccl.so.1 already in the process, else the one next to the HIP runtime in use, else the system's), so
 * the library itself has no link-time dependency on it.
 *
 * A communicator owns one RCCL communicator and one HIP stream of its own.  Collectives are ORDERED AFTER
 * everything enqueued so far on the `hip_stream` argument (the producer's stream) but RUN on the
 * communicator's stream, so kernels enqueued later on `hip_stream` overlap with the transfer;
 * zk_comm_join(comm, hip_stream) makes `hip_stream` wait for every collective issued so far.  Nothing here
 * synchronises the host except zk_comm_allgather_host and the init / destroy calls.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct zk_comm zk_comm;
#define ZK_COMM_ID_BYTES 128

/* Rendezvous.  Any of the three: (a) the caller moves the 128-byte id from rank 0 to the others itself;
 * (b) ranks of one node meet through a file: rank 0 writes the id to `path` (atomically), the others poll it,
 * rank 0 removes it once everyone has joined; (c) rank 0 listens on host:port and hands the id to each peer. */
int zk_comm_unique_id(void* id_out /* ZK_COMM_ID_BYTES */);
int zk_comm_init_rank(int device, int rank, int world, const void* id, zk_comm** out);
int zk_comm_init_file(int device, int rank, int world, const char* path, double timeout_s, zk_comm** out);
int zk_comm_init_tcp(int device, int rank, int world, const char* host, int port, double timeout_s, zk_comm** out);
int zk_comm_destroy(zk_comm* comm);
int zk_comm_rank(const zk_comm* comm);
int zk_comm_world(const zk_comm* comm);

/*
 * In-place all-gather of row blocks.  `full_dev` is the same-shaped (n_planes, H, W) float64 array on every
 * rank; rank r owns rows [r * rows_per_rank, min((r + 1) * rows_per_rank, H)) of every plane (the blocks of
 * shard_bounds: equal, the tail ranks possibly short or empty).  On entry each rank holds valid data in rows
 * [row_off, row_off + n_rows) of ITS block (clipped to the block); on completion those rows of EVERY block are
 * valid on every rank.  row_off = 0, n_rows = rows_per_rank gathers whole blocks; smaller windows are the
 * chunks of a pipelined gather (kernel of chunk c+1 overlapping the transfer of chunk c).
 *   moment matrix of a patch batch (N, n_poly):      n_planes = 1, H = N, W = n_poly
 *   dense moments / symmetry maps (planes, H, W):    rows of the frame
 *   a batch of frames (F, n_poly, H, W):             n_planes = 1, H = F, W = n_poly * H * W
 * Whole equal blocks of a single plane go through ncclAllGather (in place); everything else is one grouped
 * ncclSend / ncclRecv per peer and plane -- on the fully connected xGMI mesh that is the direct exchange
 * (every link carries one block, no ring forwarding).  ZK_COMM_ALGO=p2p|allgather|bcast in the environment
 * forces one form (bcast: one grouped ncclBroadcast per owner).
 */
int zk_allgather_rows(zk_comm* comm, double* full_dev, int64_t n_planes, int64_t height, int64_t width,
                      int64_t rows_per_rank, int64_t row_off, int64_t n_rows, void* hip_stream);

/*
 * The schedule of zk_allgather_rows as data.  zk_allgather_rows is two parts: this PURE planner (no GPU, no
 * RCCL, no communicator: callable on any machine) and an executor that hands the list, in order, to RCCL.
 * One zk_xfer is one RCCL call on the (n_planes, H, W) array seen as a flat run of doubles:
 *   ZK_XFER_SEND       ncclSend(full + offset, count, peer)
 *   ZK_XFER_RECV       ncclRecv(full + offset, count, peer)
 *   ZK_XFER_ALLGATHER  ncclAllGather(send = full + offset, recv = full + offset - rank * count, count per rank); peer -1
 *   ZK_XFER_BCAST      ncclBroadcast(full + offset, in place, count, root = peer)
 * Entries with the same `group` are issued between one ncclGroupStart / ncclGroupEnd (groups are numbered from 0,
 * ascending along the list).  Contract of a plan set (what tests/test_comm_plan.py checks for every rank of a world):
 * within a group the sends of rank a to rank b and the receives of b from a are equally many and pairwise of
 * equal count IN ORDER (RCCL matches point-to-point calls between two ranks in issue order); a rank's receives
 * are exactly the other ranks' windows, once each, disjoint from one another and from its own window; collective
 * entries (ALLGATHER / BCAST) appear on every rank in the same order with the same root and count.
 * `algo`: ZK_COMM_AUTO (whole equal blocks of one plane -> ALLGATHER, else P2P), ZK_COMM_P2P, ZK_COMM_ALLGATHER
 * (falls back to P2P when the blocks are not whole and equal), ZK_COMM_BCAST.
 * Writes at most `cap` entries to `out` (may be NULL with cap 0) and the number the plan HAS to *n_out.
 */
typedef struct zk_xfer {
  int32_t op;     /* ZK_XFER_* */
  int32_t peer;   /* destination (SEND), source (RECV), root (BCAST), -1 (ALLGATHER) */
  int32_t group;  /* ncclGroupStart / End bracket this entry belongs to */
  int32_t plane;  /* plane index the run lies in (information only; offset already includes it) */
  int64_t offset; /* first element, in doubles from full_dev */
  int64_t count;  /* elements */
} zk_xfer;
enum { ZK_XFER_SEND = 1, ZK_XFER_RECV = 2, ZK_XFER_ALLGATHER = 3, ZK_XFER_BCAST = 4 };
enum { ZK_COMM_AUTO = 0, ZK_COMM_P2P = 1, ZK_COMM_ALLGATHER = 2, ZK_COMM_BCAST = 3 };
#define ZK_COMM_PLANES_PER_GROUP 16
int zk_allgather_rows_plan(int rank, int world, int64_t n_planes, int64_t height, int64_t width, int64_t rows_per_rank,
                           int64_t row_off, int64_t n_rows, int algo, zk_xfer* out, int64_t cap, int64_t* n_out);
int zk_comm_join(zk_comm* comm, void* hip_stream);
/* Blocking all-gather of the same number of host bytes from every rank (timings, checksums, the k x D sums of a sharded
 * k-means step; doubles as a barrier).  Up to 64 MiB per rank. */
int zk_comm_allgather_host(zk_comm* comm, const void* send_host, void* recv_host, int64_t bytes_per_rank);

/* ------------------------------------------------------------------------------------------------------
 * Parameter pickers: the device side of the two reference routines that choose (size, n_max) for ZPs
 * (SURVEY 8f rank 3).  Host buffers in, host buffers out, blocking; no plan involved.  The FFTs are hipFFT's
 * (bound at run time: the library loads without it); the reference uses scipy / numpy FFTs at the same places.
 *
 *   zk_autocorr_mean  <- the loop of estimate_patch_size (features/_patch_size.py:268-279): for each window
 *                        image[y:y+window, x:x+window] (origins as (y, x) pairs), standardise_image (zero mean, unit
 *                        population std; a constant window fails with the reference's message), then
 *                        scipy.signal.correlate(p, p, mode='same', method='fft'); out = mean over the windows,
 *                        (window, window) float64, zero lag at [window/2, window/2].
 *   zk_polar_profile  <- radial_profile (features/_patch_size.py:48-100): skimage.transform.warp_polar(data,
 *                        center=(h/2, w/2), scaling='linear') aggregated over its 360 angles (method 0 mean, 1 max,
 *                        2 sum) -> (batch, zk_polar_radii(h, w)) float64.  scikit-image is not available in the
 *                        build image: the resampling restates its published algorithm (see zk_pickers.hip).
 *   zk_power_spectra  <- _get_cumulative_energy up to the radial profile (features/_estimate_n_max.py:42-65):
 *                        |fftshift(fft2(patch * outer(w, w)))|^2 for every window; window_1d may be NULL.
 *   zk_denoise_fft    <- denoise_fft (denoise/_denoise_fft.py:4-47): keep the ceil(p H W) Fourier coefficients of
 *                        largest power (exact selection; among coefficients that tie at the cut-off an arbitrary
 *                        subset survives, as with numpy.argpartition), inverse transform, real part.
 * ------------------------------------------------------------------------------------------------------ */
int zk_autocorr_mean(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t window,
                     const int32_t* origins_yx, int n_windows, int standardize, double* out_host);
int64_t zk_polar_radii(int64_t h, int64_t w);
int zk_polar_profile(int device, const double* data_host, int64_t batch, int64_t h, int64_t w, int64_t center_row,
                     int64_t center_col /* negative: (h/2, w/2) */, int method, double* out_host);
int zk_power_spectra(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t size,
                     const int32_t* origins_yx, int n_windows, const double* window_1d, double* out_host);
int zk_denoise_fft(int device, const void* image_host, int dtype, int64_t height, int64_t width, double p,
                   double* out_host);
/* skimage.restoration.estimate_sigma of a 2-D image, as estimate_n_max uses it (_estimate_n_max.py:109): median of the
 * non-zero |db2 diagonal detail coefficients| (PyWavelets dwtn, mode 'symmetric') / 0.6745 -- restated from scikit-image /
 * PyWavelets, which are not installed here (parity unpinned).  Coefficients and the median's order statistics on the device. */
int zk_wavelet_sigma(int device, const void* image_host, int dtype, int64_t height, int64_t width, double* sigma_out);

/* ------------------------------------------------------------------------------------------------------
 * Window-size estimators and the angular spectrum average (reference features/_window_size.py, _fft_related.py): what a
 * user runs before ZPs to choose `size`, here for a whole stack (batch, height, width) of ZK_F32 / ZK_F64 frames in one
 * call -- 1 .. 65535 frames of at most 16384 x 16384, any height and width.  Host buffers in, host buffers out, blocking;
 * hipFFT as above.  All arithmetic is float64.
 *
 *   zk_circular_autocorr  <- compute_autocorrelation (_window_size.py:16-27): |fftshift(ifft2(F conj F))| of every frame,
 *                            standardised first when asked (a constant frame fails with the reference's message): the
 *                            CIRCULAR autocorrelation, not the zero-padded one of zk_autocorr_mean.  out (batch, h, w).
 *   zk_shifted_magnitude  <- fft_power_spectrum (_fft_related.py:4-7): |fftshift(fft2(frame))| (the magnitude, as in the
 *                            reference), log(. + 1) of it with use_log (get_characteristic_length_fft's map).
 *   zk_char_length_fft    <- get_characteristic_length_fft (_window_size.py:65-80) up to `ind`: the shifted (log) magnitude,
 *                            its first maximum in C order (numpy.argmax) as centre (i, j), the 360-angle MEAN polar profile
 *                            of zk_polar_profile about it cut to [0:min(i, radii)], minus its SNIP baseline (niter sweeps),
 *                            scipy.ndimage.uniform_filter1d(size) with reflected edges, and the first maximum of that:
 *                            ind (batch), -1 for an empty profile (the caller returns height / ind).
 *   zk_char_length        <- get_characteristic_length (_window_size.py:36-46): scipy.signal.correlate(f, f, 'same', 'fft')
 *                            of the (standardised) frame -- the path of zk_autocorr_mean, rectangular -- its first maximum
 *                            as centre, the cut mean polar profile, and the first peak of scipy.signal.find_peaks without
 *                            conditions (plateaus at their midpoint): peaks (batch), -1 where there is none.
 *                          Both: centres (batch, 2) int32 (row, col), profiles (batch, zk_polar_radii(h, w)) with zeros
 *                            from the cut on, smoothed (the filtered profile, same layout); each may be NULL.
 *   zk_angular_average    <- angular_average (_fft_related.py:12-66) of float64 maps: per frame and bin, the SUM and the
 *                            COUNT of the pixels with edges[i] <= theta < edges[i + 1], theta = degrees(atan2(dy, dx)) mod
 *                            360 about (h / 2, w / 2), inside r <= min(h / 2, w / 2) with use_mask.  edges: the caller's
 *                            numpy.linspace(0, 360, num_bins + 1) (num_bins + 1 increasing values); membership is NumPy's
 *                            (the multiples of 45 degrees are exact), counts are exact, sums are float64 atomics and vary
 *                            in their last bits with the order of arrival.  The mean is sum / count on the caller's side.
 * ------------------------------------------------------------------------------------------------------ */
int zk_circular_autocorr(int device, const void* images_host, int dtype, int64_t batch, int64_t height, int64_t width,
                         int standardize, double* out_host);
int zk_shifted_magnitude(int device, const void* images_host, int dtype, int64_t batch, int64_t height, int64_t width,
                         int use_log, double* out_host);
int zk_char_length_fft(int device, const void* images_host, int dtype, int64_t batch, int64_t height, int64_t width, int niter,
                       int size, int use_log, int32_t* centres_host, double* profiles_host, double* smoothed_host,
                       int32_t* ind_host);
int zk_char_length(int device, const void* images_host, int dtype, int64_t batch, int64_t height, int64_t width,
                   int standardize, int32_t* centres_host, double* profiles_host, int32_t* peaks_host);
int zk_angular_average(int device, const double* spectra_host, int64_t batch, int64_t height, int64_t width,
                       const double* edges_host, int64_t num_bins, int use_mask, double* sums_host, int64_t* counts_host);

/* ------------------------------------------------------------------------------------------------------
 * Key-point detection: the device side of local_max (reference features/_local_max_v2.py), the step ahead of
 * zk_transform_points.  No plan involved; blocking.
 *
 *   candidates   pixels equal to the maximum of their 3 x 3 neighbourhood and > threshold, off the 1-px border
 *                (skimage.feature.peak_local_max(image, min_distance=1, threshold_abs=threshold)); a constant image has
 *                none.  has_threshold 0: the threshold is the image's minimum (computed on the device).  Otherwise
 *                `threshold` is compared with the exact value of every pixel as float64: the caller rounds it the way
 *                NumPy's comparison would (a Python float against a float32 image: to float32 first).
 *   suppression  candidates in descending intensity, ties in raster order (row, then column); a kept candidate drops
 *                every other one at dx^2 + dy^2 <= min_distance^2 (filter_peaks_by_distance; the reference's tie order
 *                is not stable).
 *   points       (x, y) = (column, row) of the kept candidates in that order.
 * dtype: ZK_F32 / ZK_F64 / ZK_U8 / ZK_U16 / ZK_I16 (the narrow formats are widened exactly on the device), C-contiguous
 * (height, width).  Both calls write min(n, capacity) rows and always report n in n_found: call again with capacity n
 * when it was short.  zk_local_max_dev writes int32 rows in the layout zk_transform_points_dev reads and runs on
 * hip_stream (it synchronises it: n crosses to the host).
 * zk_local_max_last_launches: suppression launches of the calling thread's last call (tools and tests).
 * ------------------------------------------------------------------------------------------------------ */
int zk_local_max(int device, const void* image_host, int dtype, int64_t height, int64_t width, double min_distance,
                 int has_threshold, double threshold, int64_t* points_host /* (cap, 2) x, y */, int64_t capacity,
                 int64_t* n_found);
int zk_local_max_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, double min_distance,
                     int has_threshold, double threshold, int32_t* points_dev /* zk_transform_points_dev layout */,
                     int64_t capacity, int64_t* n_found_host, void* hip_stream);
int64_t zk_local_max_last_launches(void);

/* ------------------------------------------------------------------------------------------------------
 * Background removal: the device side of the reference's background/ subpackage, the step ahead of local_max.  No plan
 * involved.  dtype: ZK_F32 / ZK_F64 / ZK_U8 / ZK_U16 / ZK_I16, C-contiguous (height, width).  Edges follow SciPy's
 * 'reflect' mode (dcba|abcd), folded again and again when a window or a radius exceeds the frame.
 *
 *   opening       scipy.ndimage.grey_opening(image, size=(size_y, size_x)) (background/_morphology.py): a flat minimum
 *                 filter of window [i - k/2, i - k/2 + k - 1] per axis, then a flat maximum filter of window
 *                 [i - (k - 1 - k/2), i + k/2] (SciPy's dilation origin, shifted by one on an even axis).  Sizes >= 1; an
 *                 axis of size 1 is left alone.  Background in the image's dtype, exact.
 *   rolling ball  skimage.restoration.rolling_ball(image, radius) (background/_rolling_ball.py), restated from scikit-image's
 *                 published algorithm (parity unpinned: scikit-image is not a dependency): offsets o in [-R, R]^2 with
 *                 R = ceil(radius) and |o| <= radius, diff[o] = k(0) - k(o) with k(o) = sqrt(max(radius^2 - |o|^2, 0));
 *                 background(p) = min over o of img[p + o] + diff[o], +inf outside the frame.  Arithmetic in float32 for
 *                 ZK_F32 and float64 otherwise, cast back to the image's dtype (integers truncate).  0 < radius <= 1536.
 *   baseline      background/_baseline.py: num_iters rounds of gaussian_filter (axis 0, then axis 1) and np.minimum(., image),
 *                 float64 throughout.  weights_y / weights_x: radius + 1 values w[0..r] of scipy.ndimage's symmetric kernel,
 *                 w[0] the centre (radius 0 with w[0] = 1 for an axis SciPy skips); each tap in SciPy's order,
 *                 t = x[0] w[0], then t += (x[-j] + x[+j]) w[j] for j = r .. 1, unfused: bit for bit SciPy's.
 *
 * residual (optional, NULL to skip): image - background in the background's type (NumPy's wrap-around for integers), then
 * max(., 0) when clip is non-zero.  Opening and rolling ball write background and residual in the image's dtype, baseline in
 * float64.  The _dev variants take device pointers and run on hip_stream (they synchronise it once their scratch is
 * released); nothing crosses to the host.  Any 0 < height * width < 2^31 is served, a single row or column included (the
 * kernels stride over the y extent of their grids).
 *
 * NaN / inf pixels: the baseline is SciPy's arithmetic and np.minimum (a NaN on either side stays a NaN); the rolling ball
 * skips a NaN sum, as scikit-image's `if min_value > tmp` does (a NaN or +inf pixel is passed over, a -inf pixel takes the
 * outputs whose ball holds it, an output with NaN sums only is +inf); the opening is exact on +-inf and unspecified on NaN
 * (as SciPy's own min / max queue is); the residual is NumPy's subtraction (inf - inf = NaN) and np.clip (NaN stays NaN).
 * ------------------------------------------------------------------------------------------------------ */
int zk_background_opening(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t size_y,
                          int64_t size_x, int clip, void* background_host, void* residual_host);
int zk_background_opening_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t size_y,
                              int64_t size_x, int clip, void* background_dev, void* residual_dev, void* hip_stream);
int zk_background_rolling_ball(int device, const void* image_host, int dtype, int64_t height, int64_t width, double radius,
                               int clip, void* background_host, void* residual_host);
int zk_background_rolling_ball_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, double radius,
                                   int clip, void* background_dev, void* residual_dev, void* hip_stream);
int zk_background_baseline(int device, const void* image_host, int dtype, int64_t height, int64_t width, const double* weights_y,
                           int64_t radius_y, const double* weights_x, int64_t radius_x, int64_t num_iters, int clip,
                           double* background_host, double* residual_host);
int zk_background_baseline_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width,
                               const double* weights_y /* host */, int64_t radius_y, const double* weights_x /* host */,
                               int64_t radius_x, int64_t num_iters, int clip, double* background_dev, double* residual_dev,
                               void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Image normalisation and clipping: the device side of the reference's utils/ subpackage (_preprocessing_image.py,
 * _clip_image.py), the first step of every workflow.  No plan involved.  The image is flat: n elements (1 <= n < 2^31) of
 * ZK_F32 / ZK_F64 / ZK_U8 / ZK_U16 / ZK_I16, C-contiguous in any shape, each converted to float32 as it is read (round to
 * nearest, ndarray.astype(np.float32)).  These calls do the passes over the pixels; everything scalar (np.isclose, eps,
 * NumPy's percentile interpolation, the decision to clip) is the caller's, on the few numbers that come back.
 *
 *   zk_image_stats        minmax[2]: min and max over the finite elements (+inf, -inf when there is none); *n_nonfinite: the
 *                         count of NaN / inf elements; sums[3]: sum x, sum |x|, sum x^2 over the finite elements in float64.
 *                         mode & ZK_STATS_CENTERED: sums[0] = sum (x - center)^2 instead (the second pass of a two-pass
 *                         variance), sums[1] = sums[2] = 0.  mode & ZK_STATS_WIDE: the sums (and the finite test) of a ZK_F64
 *                         image take its elements as they are, not narrowed (np.mean / np.std of a float64 image).
 *                         An element finite in float64 and past the float32 range is then summed and counted finite, and
 *                         left out of min / max.
 *                         Per-lane, per-workgroup and final partial sums are joined in a fixed tree, each carried as an
 *                         unevaluated pair of doubles: the result is the rounded exact sum to a few 2^-100 of sum |terms| and
 *                         two runs agree bit for bit (no floating-point atomics).
 *   zk_image_order_stats  values[i] = element ranks[i] (zero-based, 0 <= rank < n, at most 16 of them, any order, repeats
 *                         allowed) of the ascending sort of the converted elements (ZK_ORDER_VALUES) or of |x - center|
 *                         computed in float32 (ZK_ORDER_DEVIATIONS: the second median of a MAD; the deviations are never
 *                         stored).  Exact: a radix select on the order-preserving uint32 image of the float32 bits, every rank
 *                         refined in the same four sweeps, counts merged with integer atomics (the same result every run).
 *                         -0.0 sorts just below +0.0 (they compare equal: either may come back).  NaN elements sort by
 *                         their bits (after +inf with the sign clear); their place is not pinned.
 *   zk_image_map          out[i] = f(x[i]), one operation at a time, nothing fused:
 *                           ZK_MAP_RESCALE      p0 + (x - p1) * p2 / p3  in float32, in that order (vmin, x_min, span, scale):
 *                                               NumPy's float32 result bit for bit
 *                           ZK_MAP_CLIP         np.clip(x, p0, p1)       in float32 (NaN stays NaN; p0 > p1 gives p1)
 *                           ZK_MAP_DIVIDE       x / p0                   in float64, rounded once to float32
 *                           ZK_MAP_STANDARDIZE  (x - p0) / p1            in float64 on the element as stored, rounded once
 *                         params: four doubles (the float32 operations take them rounded to float32).  out is float32, except
 *                         ZK_MAP_STANDARDIZE of a non-ZK_F32 image: float64.  keep_nonfinite: NaN / inf elements are copied
 *                         to the output as they are.
 *
 * The _dev variants take device pointers (image, out) and run on hip_stream; ranks, params and every scalar result are host
 * memory (stats and order stats synchronise the stream: their results cross to the host).
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_STATS_CENTERED 1
#define ZK_STATS_WIDE 2
#define ZK_ORDER_VALUES 0
#define ZK_ORDER_DEVIATIONS 1
#define ZK_MAP_RESCALE 0
#define ZK_MAP_DIVIDE 1
#define ZK_MAP_CLIP 2
#define ZK_MAP_STANDARDIZE 3
int zk_image_stats(int device, const void* image_host, int dtype, int64_t n, int mode, double center, float* minmax_host,
                   int64_t* n_nonfinite_host, double* sums_host);
int zk_image_stats_dev(int device, const void* image_dev, int dtype, int64_t n, int mode, double center, float* minmax_host,
                       int64_t* n_nonfinite_host, double* sums_host, void* hip_stream);
int zk_image_order_stats(int device, const void* image_host, int dtype, int64_t n, int mode, float center,
                         const int64_t* ranks_host, int n_ranks, float* values_host);
int zk_image_order_stats_dev(int device, const void* image_dev, int dtype, int64_t n, int mode, float center,
                             const int64_t* ranks_host, int n_ranks, float* values_host, void* hip_stream);
int zk_image_map(int device, const void* image_host, int dtype, int64_t n, int op, const double* params_host, int keep_nonfinite,
                 void* out_host);
int zk_image_map_dev(int device, const void* image_dev, int dtype, int64_t n, int op, const double* params_host,
                     int keep_nonfinite, void* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Rasterising Gaussian atoms: the device side of the reference's datasets/ subpackage (_tapered_gaussian.py, what
 * HoneyCombLattice.to_image draws with, and the uncut Gaussians of _zps_test_data.py / _generate_data_gn.py).  No plan
 * involved.  frame: ZK_F32 / ZK_F64, C-contiguous (batch, height, width), ADDED TO IN PLACE.  points: n_points pairs (x, y)
 * of float64 in pixel coordinates (x the column, y the row; centres may lie outside the frame and may be negative);
 * amplitudes: n_points float64.  Both are HOST arrays in either form.
 *
 *   r_factor > 0   add_tapered_gaussian, to the letter.  With R = r_factor * sigma, point (x0, y0) touches the pixels of
 *                  [floor(x0 - R), ceil(x0 + R)] x [floor(y0 - R), ceil(y0 + R)] cut to the frame (nothing left: the point is
 *                  skipped); with dx = X - x0, dy = Y - y0, r = sqrt(dx * dx + dy * dy), the pixels with r <= R receive
 *                    taper = 1:  A * exp(-0.5 * (r * r) / sigma^2) * (1 - 3 t^2 + 2 t^3),  t = r / R
 *                    taper = 0:  A * exp(-0.5 * (r * r) / sigma^2)
 *                  in float64, one rounding per operation, nothing fused.  At r = R the taper is exactly 0.  The pixels of
 *                  the box outside the disc, to which the reference adds 0.0, are left alone: the one visible difference
 *                  is that a -0.0 pixel there stays -0.0.  batch must be 1.
 *   r_factor <= 0  no cutoff (taper must be 0): every pixel of the frame receives A * exp(-(dx * dx + dy * dy) / (2 sigma^2)),
 *                  the squared distance as it is, no sqrt.  batch frames of equal shape, frame b taking the points
 *                  point_offsets[b] .. point_offsets[b + 1] (batch + 1 ascending int64 from 0 to n_points, host memory;
 *                  NULL with batch = 1: all points).
 *
 * Order is part of the contract: every pixel adds its contributions in ascending point index, and a ZK_F32 frame rounds
 * after every add, acc = (float)((double)acc + w), as the reference's in-place += does.  It is a gather (per-tile point
 * lists built with integer atomics and sorted), so two runs agree bit for bit; no floating-point atomics.
 * list_budget: the most list entries (one per point and 16 x 16 pixel tile its box overlaps) built at once, <= 0 for the
 * default of 2^24; past it the points are rendered as consecutive index ranges, which changes no result.
 * The _dev variant takes the frame as a device pointer, runs on hip_stream and synchronises it before it returns (its point
 * and list buffers live for the call).
 * ------------------------------------------------------------------------------------------------------ */
int zk_render_gaussians(int device, void* frame_host, int dtype, int64_t height, int64_t width, int64_t batch,
                        const double* points_host, const double* amplitudes_host, const int64_t* point_offsets_host,
                        int64_t n_points, double sigma, double r_factor, int taper, int64_t list_budget);
int zk_render_gaussians_dev(int device, void* frame_dev, int dtype, int64_t height, int64_t width, int64_t batch,
                            const double* points_host, const double* amplitudes_host, const int64_t* point_offsets_host,
                            int64_t n_points, double sigma, double r_factor, int taper, int64_t list_budget, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Faces of a planar lattice graph: the device side of the reference's graph/ subpackage (find_regions.py, and the centres,
 * ring sizes and region adjacency that planar_graph.py derives from its result).  No plan involved.
 * points: n_points pairs (x, y) of float64; edges: n_edges directed pairs (i, j) of int64 with values in [0, n_points) and
 * i != j (anything else: ZK_E_BADARG; the host variant checks before anything is launched, the _dev variant on the device).
 * Duplicated pairs collapse; pairs are NOT symmetrised: a pair given in one direction is a neighbour in one direction.
 * Needs n_points + n_edges + 4 < 2^31.
 *
 * What is computed, in the reference's terms: a node is grown at (x - 1, y) of the first point of smallest x, joined to it in
 * both directions; every node's neighbours are sorted by theta = fmod(atan2(dy, dx) + 2 pi, 2 pi) ascending (float64, ties by
 * ascending j) into js[0 .. d); rows ("wedges") (js[t - 1], i, js[t]) for d >= 2, (js[0], -1, js[0]) for d == 1 and
 * (i, -1, -1) for d == 0 are sorted by column 0, then column 1; the successor of (a, b, c) with b != -1 is the row starting
 * (b, c), a row without one is a dead end.  Every cycle of the successor map is one polygon; polygons are ordered by their
 * smallest sorted row, and polygon entry t is column 0 of the cycle's t-th row counted from that smallest row.
 *
 * The output sizes are not known beforehand, so a call has two phases, told apart by *state:
 *   count   *state == NULL.  Runs the whole computation, keeps the results on the device behind *state, and writes
 *           counts_host[0 .. 3) = {F polygons, V vertices of all polygons together, A adjacency pairs}.  The five output
 *           pointers are not touched.  Both phases synchronise the stream (the counts cross to the host; the state is freed).
 *   fill    *state != NULL.  Copies to the non-NULL outputs, frees the state and sets *state = NULL (call it with five NULL
 *           outputs to just free).  points / edges / counts_host are not read.
 *             offsets    int64 (F + 1)  polygon f is vertices[offsets[f] .. offsets[f + 1])
 *             vertices   int64 (V)
 *             ks         int64 (F)      offsets[f + 1] - offsets[f]
 *             centers    float64 (F, 2) the polygon's points added one after the other in vertex order, divided by k:
 *                                       bit-equal to NumPy's nodes[region].mean(axis=0)
 *             adjacency  int64 (A, 2)   for every bond a < b whose half-edges a -> b and b -> a both lie on polygons, the
 *                                       pair (polygon of a -> b, polygon of b -> a), equal entries included, in ascending
 *                                       order of the sorted row (a, b, .)
 * Integer work apart from the angles and the centres, no floating-point atomics: two runs agree byte for byte.
 * zk_find_regions takes and fills host arrays; zk_find_regions_dev takes and fills device arrays on hip_stream.
 * ------------------------------------------------------------------------------------------------------ */
int zk_find_regions(int device, const double* points_host, int64_t n_points, const int64_t* edges_host, int64_t n_edges,
                    void** state, int64_t* counts_host, int64_t* offsets_host, int64_t* vertices_host, int64_t* ks_host,
                    double* centers_host, int64_t* adjacency_host);
int zk_find_regions_dev(int device, const double* points_dev, int64_t n_points, const int64_t* edges_dev, int64_t n_edges,
                        void** state, int64_t* counts_host, int64_t* offsets_dev, int64_t* vertices_dev, int64_t* ks_dev,
                        double* centers_dev, int64_t* adjacency_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Voronoi neighbours of a point set and the bonds the reference's graph/vnn.py (vnn_graph) keeps of them: the step between key
 * points and zk_find_regions.  No plan involved.
 * points: n_points pairs of ZK_F64, or of ZK_I32 (the (x, y) pairs zk_local_max writes, widened exactly on the device); the
 * result does not depend on which column is x.  Needs n_points < 2^26 - 4 and pad > 0.
 *
 * The diagram is that of the points plus four corner points centre + (-+v, -+v) in the order (-,-) (+,-) (+,+) (-,+), with
 * centre = mean of the points and v = max |p - centre| (1 + pad) over both coordinates (the reference's add_corner_points;
 * centre and v are reduced on the device in float64 in a fixed order, so they may differ from NumPy's by rounding).  Every
 * point clips its own cell, a convex polygon of at most 32 vertices, against the corners and then against the points of a
 * uniform grid of bins in rings of growing distance, until no point farther away can reach the cell.
 *
 *   mode ZK_VORONOI_NEIGHBOURS  rows (i, j) for every point i and every point j whose cells share a ridge of positive length,
 *                               with ridge[m] = that length as computed in the cell of i and edge[m] = hypot(p_j - p_i).
 *                               dmax and threshold are ignored.
 *   mode ZK_VORONOI_GRAPH       vnn_graph: with R_i the neighbours of i (corner points included) at less than dmax, the entry
 *                               (i, j) is kept when j is a point of R_i and L_ij / sum over R_i of L_ik >= threshold; the rows
 *                               are the pairs kept in either direction, in both directions.  Needs dmax > 0, threshold > 0;
 *                               ridge / edge are not written.
 * Rows are sorted by i, then j.
 *
 * Errors (ZK_E_BADARG, nothing returned, the library stays usable): a non-finite coordinate (the host variant checks before
 * anything is launched, the _dev variant on the device; finite coordinates so large that their sum or the starting square of a
 * cell overflows, near 1e307, count as non-finite), two coincident points, a cell that needs more than 32 vertices (a point
 * with more than 32 Voronoi neighbours, or with nearly as many: cells are clipped in bin order and may pass their final size
 * on the way), a cell that is convex only up to rounding (nearly coincident points).
 * Memory: the count phase stages 32 rows per point on the device, 128 B a point in graph mode and 640 B in neighbour mode
 * (43 GB at the limit on n_points), freed when it returns.
 *
 * The number of rows is not known beforehand, so a call has two phases, told apart by *state, as zk_find_regions:
 *   count   *state == NULL.  Runs the whole computation, keeps the rows on the device behind *state and writes
 *           counts_host[0] = M rows.  The three output pointers are not touched.  Both phases synchronise the stream.
 *   fill    *state != NULL.  Copies to the non-NULL outputs ijs int64 (M, 2), ridge float64 (M), edge float64 (M), frees the
 *           state and sets *state = NULL.  The other arguments are not read.
 * No floating-point atomics, every sum in a fixed order: two runs agree byte for byte.
 * zk_voronoi_cells takes and fills host arrays; zk_voronoi_cells_dev takes and fills device arrays on hip_stream.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_VORONOI_NEIGHBOURS 0
#define ZK_VORONOI_GRAPH      1
int zk_voronoi_cells(int device, const void* points_host, int points_dtype, int64_t n_points, double pad, int mode, double dmax,
                     double threshold, void** state, int64_t* counts_host, int64_t* ijs_host, double* ridge_host, double* edge_host);
int zk_voronoi_cells_dev(int device, const void* points_dev, int points_dtype, int64_t n_points, double pad, int mode, double dmax,
                         double threshold, void** state, int64_t* counts_host, int64_t* ijs_dev, double* ridge_dev, double* edge_dev,
                         void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Sub-pixel refinement of key points: the reference's center_of_mass_refine (features/_keypoint.py:12-23), the step between
 * zk_local_max and zk_voronoi_cells.  No plan involved.
 * image: (H, W) of ZK_F32 or ZK_F64.  points: n_points int32 pairs (x, y), what zk_local_max writes.  out: float64 (n_points, 2),
 * rows (x, y).  mode: ZK_REFINE_BOX (the (2 size + 1)^2 box) or ZK_REFINE_DISK (its pixels with dx^2 + dy^2 <= size^2).
 *
 * What is computed: the regions are painted in point order into one label image, so a pixel belongs to the LAST point whose box
 * covers it; in disk mode the corners of that last box paint 0 and such a pixel belongs to nobody, even where an earlier disk
 * covered it.  Per point three float64 sums over its pixels in raveled (row-major) order -- value, value * (double)row,
 * value * (double)col, each product rounded once -- and x = sum(value * col) / sum(value), y = sum(value * row) / sum(value):
 * bit-equal to scipy.ndimage.center_of_mass on that label image.  A point left with no pixels gives NaN, NaN (0 / 0).
 *
 * Errors (ZK_E_BADARG, nothing returned): a dtype other than the two float types, n_points >= 2^24 (the reference's label image
 * has the frame's type), size outside [0, 64], a box that leaves the frame (every point needs size <= x < W - size and
 * size <= y < H - size; the host variant checks before anything is launched, the _dev variant on the device, where such a point
 * paints and reads nothing).
 * Memory: an int32 owner image of H x W, freed when the call returns.  Integer atomics only: two runs agree byte for byte.
 * zk_refine_points takes and fills host arrays; zk_refine_points_dev takes and fills device arrays on hip_stream, which is
 * synchronised before it returns (the error flag crosses to the host).
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_REFINE_BOX  0
#define ZK_REFINE_DISK 1
int zk_refine_points(int device, const void* image_host, int image_dtype, int64_t H, int64_t W, const int32_t* points_host,
                     int64_t n_points, int64_t size, int mode, double* out_host);
int zk_refine_points_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const int32_t* points_dev,
                         int64_t n_points, int64_t size, int mode, double* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Thresholded centroid refinement of key points: the reference's com_refine (features/_keypoint.py:26-43).  No plan involved.
 * image: (H, W) of ZK_F32 or ZK_F64.  corners: n int32 pairs (x0, y0); window i is image[y0 : y0 + size, x0 : x0 + size],
 * 2 <= size <= 64, widened to float64.  threshold: ZK_THRESHOLD_LI or ZK_THRESHOLD_OTSU, both defined on that float64 window:
 *   Otsu  np.histogram(window, 256) (np.linspace's edges, NumPy's bin rule) and the centre of the bin that maximises the
 *         between-class variance, the cumulative sums taken sequentially in bin order as np.cumsum does; the first maximum.
 *   Li    v = window - min; from mean(v), t <- (mean_back - mean_fore) / (log(mean_back) - log(mean_fore)) over v > t and the
 *         rest, until two iterates differ by no more than half the smallest gap between distinct values, or mean_back == 0; a NaN
 *         from an empty side ends the loop and stays.  thresholds = t + min.  A window still running after 1000 steps is an error.
 *   A window of one value has that value as its threshold and no iteration.
 * Values below the threshold count as zero (none when it is NaN); centroids (n, 2) float64 holds
 * (sum(w * col) / sum(w), sum(w * row) / sum(w)) with window-local indices and every product rounded once; 0 / 0 = NaN is kept.
 * thresholds (n float64) and iterations (n int32: Li's steps, 0 for Otsu) may be NULL.  Sums go through a fixed tree that depends on
 * size alone: no floating-point atomics, two runs agree bit for bit.  Parity with scikit-image is not pinned (it bins a float32
 * window in float32).
 *
 * zk_com_refine_points_dev takes key points instead, ZK_I32 or ZK_F64 pairs (x, y): the corner is rint(point) - size / 2 and
 * out = (centroid - size / 2.0) + point, both on the device.
 *
 * Errors (ZK_E_BADARG, nothing returned): a dtype other than the two float types, n >= 2^24, size outside [2, 64], an unknown
 * threshold, a window that leaves the frame (the host variant checks before anything is launched, the _dev variants on the
 * device, where such a window reads and writes nothing).  No per-window global memory.  zk_com_refine takes and fills host
 * arrays; the _dev variants take and fill device arrays on hip_stream, which is synchronised before they return (the error flag
 * crosses to the host).
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_THRESHOLD_LI   0
#define ZK_THRESHOLD_OTSU 1
int zk_com_refine(int device, const void* image_host, int image_dtype, int64_t H, int64_t W, const int32_t* corners_host, int64_t n,
                  int64_t size, int threshold, double* centroids_out, double* thresholds_out, int32_t* iterations_out);
int zk_com_refine_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const int32_t* corners_dev, int64_t n,
                      int64_t size, int threshold, double* centroids_dev, double* thresholds_dev, int32_t* iterations_dev,
                      void* hip_stream);
int zk_com_refine_points_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const void* points_dev,
                             int points_dtype, int64_t n, int64_t size, int threshold, double* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Gaussian fits of key points: a least-squares fit of a 2-D Gaussian to the window of every key point.  No plan involved, and
 * no counterpart in the reference: this section is the definition.
 * image: (H, W) of ZK_F32 or ZK_F64.  corners: n int32 pairs (cx, cy); window i is image[cy : cy + size, cx : cx + size],
 * 3 <= size <= 32, widened to float64.  mask: ZK_GAUSS_BOX fits every pixel of the window, ZK_GAUSS_DISK (odd size only) the
 * pixels with (row - r)^2 + (col - r)^2 <= r^2, r = size / 2 (integer division).  The fitted pixels must outnumber the parameters.
 *
 * Model, in window coordinates, dx = col - x0, dy = row - y0:
 *   ZK_GAUSS_ELLIPTICAL  f = g + A exp(-(a dx^2 + 2 b dx dy + c dy^2) / 2), parameters p = (A, x0, y0, a, b, c, g)
 *   ZK_GAUSS_CIRCULAR    the same with b = 0 and c = a, parameters p = (A, x0, y0, a, g)
 * (the entries of the precision matrix, not widths and an angle: the problem stays regular where the column is round).
 * With r_i = pixel_i - f_i, J the derivatives of f, the sums J^T J, J^T r and rss = sum r_i^2 run over the fitted pixels.
 *
 * Start: g = the minimum of the fitted pixels, A = their maximum less that minimum, x0 = y0 = size / 2 (integer division: the pixel
 * the key point rounds to, so the fit is a function of the window alone and a point gives the same result through either entry
 * point), a = c = 1 / sigma0^2, b = 0, lambda = 1e-3.  The sums of the start are taken first; that is not an iteration.
 * Iteration (Levenberg-Marquardt with Marquardt's scaling), until a stop below:
 *   1. if `max_iter` iterations have been made, stop with status 1; otherwise this is one more iteration;
 *   2. solve (J^T J + lambda diag(J^T J)) delta = J^T r by Cholesky; trial = p + delta;
 *   3. the trial is ACCEPTED when no pivot failed (every pivot > 0), every entry of the trial is finite, the form is positive
 *      definite (a > 0, c > 0, a c - b^2 > 0), the centre lies in [-0.5, size - 0.5] on both axes, and rss(trial) <= rss(p);
 *   4. accepted: p = trial, lambda = max(lambda / 10, 1e-12), and if |delta_k| <= tol (|p_k| + 1) for every parameter (p the
 *      accepted trial) stop with status 0;
 *   5. otherwise: p stays, lambda = lambda * 10, and if lambda > 1e12 stop with status 2.
 * status: ZK_GAUSS_CONVERGED 0; ZK_GAUSS_MAX_ITER 1; ZK_GAUSS_STALLED 2 (lambda passed 1e12, or the fitted pixels are all
 * equal: then the start is returned with no iteration and rss 0); ZK_GAUSS_NOT_FINITE 3 (a fitted pixel is NaN or inf: the eight
 * outputs are NaN, no iteration).  Status 1 and 2 return the last accepted parameters.  iterations counts every pass through 1.
 *
 * params (n, 8) float64: x = (double)cx + x0, y = (double)cy + y0 (one rounded addition each), A, sigma_major = 1 / sqrt(l1),
 * sigma_minor = 1 / sqrt(l2) with l1 <= l2 the eigenvalues of [[a, b], [b, c]] (l2 = (a + c) / 2 + sqrt(((a - c) / 2)^2 + b^2),
 * l1 = (a c - b^2) / l2; the circular model: both are 1 / sqrt(a)), theta = atan2(-2 b, c - a) / 2, the angle of the major axis
 * from the x axis towards y, in (-pi/2, pi/2] (0 for the circular model; -2 b is formed as 0 - 2 b, so b = 0 gives 0 or pi/2,
 * never -pi/2), g, rss.
 * iterations and status: n int32 each.
 *
 * One kernel launch for all points, one wave a point, the window in registers, no global scratch; the lanes' sums are joined in
 * an order that depends on size alone and there are no floating-point atomics, so two runs and the two entry points agree bit
 * for bit.  zk_gauss_fit takes and fills host arrays and checks every window before anything is launched.
 * zk_gauss_fit_points_dev takes device arrays on hip_stream and key points, ZK_I32 or ZK_F64 pairs (x, y): the corner is
 * rint(point) - size / 2, computed on the device; a window that leaves the frame raises a flag there and nothing is written for
 * that point.  The stream is synchronised before it returns (the flag crosses to the host).
 *
 * Errors (ZK_E_BADARG, nothing returned): a dtype other than the two float types, n >= 2^24, size outside [3, 32], an unknown
 * model or mask, the disk with an even size, no more fitted pixels than parameters (the disk at size 3), sigma0 not positive and
 * finite, tol negative or not finite, max_iter outside [1, 10000], a window that leaves the frame.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_GAUSS_CIRCULAR   0
#define ZK_GAUSS_ELLIPTICAL 1
#define ZK_GAUSS_BOX  0
#define ZK_GAUSS_DISK 1
#define ZK_GAUSS_CONVERGED  0
#define ZK_GAUSS_MAX_ITER   1
#define ZK_GAUSS_STALLED    2
#define ZK_GAUSS_NOT_FINITE 3
int zk_gauss_fit(int device, const void* image_host, int image_dtype, int64_t H, int64_t W, const int32_t* corners_host, int64_t n,
                 int64_t size, int model, int mask, double sigma0, double tol, int64_t max_iter, double* params_out,
                 int32_t* iterations_out, int32_t* status_out);
int zk_gauss_fit_points_dev(int device, const void* image_dev, int image_dtype, int64_t H, int64_t W, const void* points_dev,
                            int points_dtype, int64_t n, int64_t size, int model, int mask, double sigma0, double tol, int64_t max_iter,
                            double* params_dev, int32_t* iterations_dev, int32_t* status_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * The device passes of the reference's estimate_d (graph/vnn.py:18-40): the bond length vnn_graph cuts at when no dmax is given.
 * No plan involved.
 *
 * zk_knn_distances: out float64 (n_points, k), the k smallest Euclidean distances sqrt(dx * dx + dy * dy) (float64, not fused) of
 * every point to the points of the set, itself included (column 0 is 0; a coincident point adds another 0), ascending.
 * points as for zk_voronoi_cells (ZK_F64 or ZK_I32 pairs).  Needs 1 <= k <= 12, k <= n_points < 2^26, finite points
 * (ZK_E_BADARG otherwise).  Points are binned on a uniform grid and every point searches rings of bins until its k-th best is
 * no farther than anything an unvisited ring can hold.
 *
 * zk_knn_stats: one reduction over dd, the (n_points, 12) matrix zk_knn_distances writes at k = 12, for the eleven nested
 * samples d_k = dd[:, 1:k], k = 2 .. 12 (index c = k - 2 below).  params_host / counts_host / sums_host are HOST arrays:
 *   ZK_KNN_RANGES  sums[0] = min of column 1, sums[j] = max of column j, j = 1 .. 11: d_k spans [sums[0], sums[k - 1]].
 *   ZK_KNN_HIST    params = {first, last[11], edges[11][257]}; counts[c][256] = np.histogram(d_k, bins=256)[0] under NumPy's own
 *                  rule: index (v - first) / (last_c - first) * 256 truncated, 256 folded into 255, one down when
 *                  v < edges[index], one up when v >= edges[index + 1] outside the last bin.  Needs last_c > first.
 *   ZK_KNN_SIDES   params = {shift, t[11]}; with w = v - shift: counts[c] = number of w > t_c in d_k, sums[2 c] = their sum,
 *                  sums[2 c + 1] = the sum of the others.  Fixed summation tree, no floating-point atomics.
 *   ZK_KNN_GAPS    params = {shift}, shift <= every value; sums[c] = the smallest positive difference between two values
 *                  w = v - shift of d_k (a radix sort of the bit patterns and adjacent differences), +inf when all are equal.
 * Both calls synchronise the stream.  The _dev variants take device arrays (points, out, dd) on hip_stream.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_KNN_RANGES 0
#define ZK_KNN_HIST   1
#define ZK_KNN_SIDES  2
#define ZK_KNN_GAPS   3
int zk_knn_distances(int device, const void* points_host, int points_dtype, int64_t n_points, int k, double* out_host);
int zk_knn_distances_dev(int device, const void* points_dev, int points_dtype, int64_t n_points, int k, double* out_dev,
                         void* hip_stream);
int zk_knn_stats(int device, const double* dd_host, int64_t n_points, int op, const double* params_host, int64_t* counts_host,
                 double* sums_host);
int zk_knn_stats_dev(int device, const double* dd_dev, int64_t n_points, int op, const double* params_host, int64_t* counts_host,
                     double* sums_host, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Patch-SVD / patch-PCA denoising: the device side of the reference's denoise/ subpackage (_denoise_svd.py,
 * _denoise_svd_memory_view.py), the step ahead of background removal.  No plan involved.
 *
 * A is the implicit (N, D) matrix whose row w = a * n_cols + b is the patch_h x patch_w window of the frame at origin
 * (row_origins[a], col_origins[b]), flattened row-major: D = patch_h * patch_w, N = n_rows * n_cols.  The origin lists are
 * HOST arrays in every form, strictly ascending, every window inside the frame (checked); A is never formed.  image: dtype
 * ZK_F32 / ZK_F64 / ZK_U8 / ZK_U16 / ZK_I16, C-contiguous (height, width), widened to float64 as it is read; every other
 * operand and result is float64, C-contiguous.
 *
 *   zk_windows_apply        Y (N, n_columns) = (A - 1 mean^T) Q, Q (D, n_columns); mean (D) may be NULL (no centring).
 *   zk_windows_apply_t      Z (D, n_columns) = A^T Y, Y (N, n_columns).
 *   zk_windows_moments      over the DENSE grid (every origin, step 1): mean (D) of the windows and their covariance
 *                           cov (D, D) = (A - 1 mean^T)^T (A - 1 mean^T) / (N - 1) (divided by 1 when N == 1), computed from
 *                           the products of the mean-centred frame with its own shifts (about 2 D height width products).
 *                           Patches of at most 48 x 48.
 *   zk_windows_reconstruct  out (height, width) = sum over the windows w on each pixel of (Y[w, :] V + mean)[d] / (number
 *                           of windows on the pixel), d the pixel's place in window w; Y (N, n_components), V (n_components, D);
 *                           mean may be NULL.  With V == NULL, Y is an explicit (N, patch_h, patch_w) batch of patches and
 *                           n_components is ignored.  The windows of a pixel are added rows of the grid first, ascending (the
 *                           reference's loop order); a pixel under no window is 0 / 0 = NaN.
 *
 * No atomics: every sum has a fixed order, two calls give the same bits.  The _dev forms take device pointers for the image,
 * the operands and the results, run on hip_stream and synchronise it before they return (their tables and scratch are
 * released); nothing but the origin lists crosses from the host.
 * ------------------------------------------------------------------------------------------------------ */
int zk_windows_apply(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                     const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins, int64_t n_cols, const double* Q_host,
                     int64_t n_columns, const double* mean_host, double* Y_host);
int zk_windows_apply_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                         const int32_t* row_origins /* host */, int64_t n_rows, const int32_t* col_origins /* host */, int64_t n_cols,
                         const double* Q_dev, int64_t n_columns, const double* mean_dev, double* Y_dev, void* hip_stream);
int zk_windows_apply_t(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                       const int32_t* row_origins, int64_t n_rows, const int32_t* col_origins, int64_t n_cols, const double* Y_host,
                       int64_t n_columns, double* Z_host);
int zk_windows_apply_t_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t patch_h,
                           int64_t patch_w, const int32_t* row_origins /* host */, int64_t n_rows,
                           const int32_t* col_origins /* host */, int64_t n_cols, const double* Y_dev, int64_t n_columns,
                           double* Z_dev, void* hip_stream);
int zk_windows_moments(int device, const void* image_host, int dtype, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                       double* mean_host, double* cov_host);
int zk_windows_moments_dev(int device, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t patch_h,
                           int64_t patch_w, double* mean_dev, double* cov_dev, void* hip_stream);
int zk_windows_reconstruct(int device, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w, const int32_t* row_origins,
                           int64_t n_rows, const int32_t* col_origins, int64_t n_cols, const double* Y_host, int64_t n_components,
                           const double* V_host, const double* mean_host, double* out_host);
int zk_windows_reconstruct_dev(int device, int64_t height, int64_t width, int64_t patch_h, int64_t patch_w,
                               const int32_t* row_origins /* host */, int64_t n_rows, const int32_t* col_origins /* host */,
                               int64_t n_cols, const double* Y_dev, int64_t n_components, const double* V_dev,
                               const double* mean_dev, double* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * First downstream consumer of the moment matrix: the two streaming passes of
 *   pca(X, n_components)   reference features/_dimension_reduction.py:3-6 (sklearn PCA(n).fit_transform(X))
 * on a float64 matrix X (N, D), D <= 127 (45 moments at n_max 8).
 *   zk_gram[_dev]     G (D+1, D+1) = [X | 1]^T [X | 1]: X^T X with the column sums in the last row / column and N in
 *                     the corner -- everything the covariance needs, one pass over X.
 *   zk_project[_dev]  Y (N, k) = (X - mean) components^T, k <= 16.
 * The D x D eigen-problem between them is solved on the host (LAPACK, as scikit-learn's "covariance_eigh" solver does).
 * The host-buffer zk_gram leaves X on the device and hands the copy back (X_dev_out) for zk_project, which frees it
 * when free_x is non-zero.
 * ------------------------------------------------------------------------------------------------------ */
int zk_gram(int device, const double* X_host, int64_t n_rows, int n_features, double* gram_host, void** X_dev_out);
int zk_project(int device, const void* X_dev, int64_t n_rows, int n_features, const double* mean_host,
               const double* components_host, int n_components, double* Y_host, int free_x);
int zk_gram_dev(int device, const double* X_dev, int64_t n_rows, int n_features, double* gram_dev, void* hip_stream);
int zk_project_dev(int device, const double* X_dev, int64_t n_rows, int n_features, const double* mean_dev,
                   const double* components_dev, int n_components, double* Y_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Clustering consumers of the moment matrix, csrc/zk_rows.hip, zk_kmeans.hip, zk_mixture.hip:
 *   kmeans_lbs(X, n)   reference clustering/_clustering_functions.py:8-22  (sklearn KMeans(n, random_state).fit(X).labels_)
 *   gmm_lbs(X, n)      reference clustering/_clustering_functions.py:25-33 (sklearn GaussianMixture(n, type).fit(X).predict(X))
 * zk_rows = a float64 matrix (N, D), D <= 127, resident on one device together with the work buffers of these passes.
 * Every pass over the matrix is one call here; what happens between passes (random draws, centre updates, D x D Cholesky
 * factors, convergence tests) is scikit-learn's control flow, restated by the caller (mtflearn_amd/clustering.py).
 * Results do not depend on scheduling: per-workgroup partial sums are reduced in a fixed order.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct zk_rows zk_rows;
int zk_rows_create(int device, const double* X_host, int64_t n_rows, int n_features, zk_rows** out); /* uploads a copy */
/* borrows X_dev (the caller keeps it alive and unchanged for the object's lifetime).  The passes run on a stream of the
 * object's own; zk_rows_adopt therefore waits (hipDeviceSynchronize) for whatever is still writing X_dev -- e.g. an
 * asynchronous zk_transform_patches_dev on the caller's stream -- before it returns. */
int zk_rows_adopt(int device, const double* X_dev, int64_t n_rows, int n_features, zk_rows** out);
int zk_rows_destroy(zk_rows* rows);
const double* zk_rows_data(const zk_rows* rows);                 /* the device matrix */
/* Column means and population variances (two passes, as numpy.mean / numpy.var); the means become the centring shift of
 * the k-means calls (scikit-learn subtracts them before clustering); n_bad_out = rows with a non-finite element. */
int zk_rows_center(zk_rows* rows, double* mean_out, double* var_out, int64_t* n_bad_out);
/* The two halves of zk_rows_center for a matrix whose rows are spread over several ranks: local column sums; then, with the
 * mean over ALL ranks, the local sums of squared deviations (and the centring shift, row norms, finiteness count). */
int zk_rows_colsum(zk_rows* rows, double* sums_out);
int zk_rows_center_at(zk_rows* rows, const double* mean, double* sqsum_out, int64_t* n_bad_out);
int zk_rows_fetch(zk_rows* rows, const int64_t* idx, int n, int centred, double* rows_out);   /* (n, D) to the host */
int zk_rows_reset_labels(zk_rows* rows);                         /* labels := -1 (a new k-means run) */
int zk_rows_labels(zk_rows* rows, int32_t* labels_host);         /* (N) labels of the last k-means / E step */
const int32_t* zk_rows_labels_dev(const zk_rows* rows);
/* k-means++ seeding (sklearn _kmeans_plusplus): squared distances of every centred row to t <= 8 candidate rows
 * (cand (t, D) centred, cand_sq their squared norms), max(0, (-2 x.c + |c|^2) + |x|^2), folded with the closest distance
 * so far when use_closest; pot_out[c] = their sum over the rows.  zk_kmeans_seed_pick adopts candidate `which` as the
 * closest-distance row and returns searchsorted(cumsum(closest), vals) clipped to N - 1 (n_vals may be 0). */
int zk_kmeans_seed_step(zk_rows* rows, const double* cand, const double* cand_sq, int t, int use_closest, double* pot_out);
int zk_kmeans_seed_pick(zk_rows* rows, int which, const double* vals, int n_vals, int64_t* idx_out);
/* One Lloyd pass (sklearn lloyd_iter_chunked_dense) with the centred centres (k, D), k <= 256: label = first argmin_c
 * (|c|^2 - 2 x.c); with `update` sums_out (k, D) = sum of the centred rows per cluster, counts_out (k);
 * n_changed_out = rows whose label changed. */
int zk_kmeans_step(zk_rows* rows, const double* centers, int k, int update, double* sums_out, double* counts_out,
                   int64_t* n_changed_out);
int zk_kmeans_own_distance(zk_rows* rows, const double* centers, int k, double* dist_host);   /* |x - c[label]|^2, (N) */
/* HIP-event time of the Lloyd kernel inside the zk_kmeans_step calls that follow (measurement aid of bench.py). */
int zk_rows_profile(zk_rows* rows, int enable);
double zk_rows_last_kernel_ms(const zk_rows* rows);
/* Gaussian mixture (sklearn _estimate_log_gaussian_prob / _estimate_log_prob_resp / _estimate_gaussian_parameters):
 * E step with upper-triangular precision Cholesky factors (k, D, D), means (k, D), log-determinants and log weights (k):
 * responsibilities (k, N) and labels (first argmax) stay on the device, lse_sum_out = sum_r logsumexp_c; the M step's
 * sums of `count` (1 to 3) consecutive components about `shift` in one pass over the matrix: gram_out (count, D+1, D+1), each
 * sum_r resp[c][r] [x_r - shift | 1]^T [x_r - shift | 1]. */
int zk_gmm_estep(zk_rows* rows, const double* prec_chol, const double* means, const double* log_det, const double* log_w, int k,
                 int want_resp, double* lse_sum_out);
int zk_gmm_resp_from_labels(zk_rows* rows, int k);               /* one-hot of the current labels */
int zk_gmm_moments(zk_rows* rows, int component, int count, const double* shift, double* gram_out);  /* count 1..8 per pass (1..3 with more than 47 features) */
/* The same sums with unit weights (the Gram matrix about `shift` with the column sums and N: what a covariance needs). */
int zk_rows_gram(zk_rows* rows, const double* shift, double* gram_out);

/* ------------------------------------------------------------------------------------------------------
 * The manifold consumer: ForceGraph8, reference manifold/force_relaxed.py:285-366 (csrc/zk_graph.hip).
 *   zk_rows_knn_correlation  compute_graph's neighbour search (:67-74: sklearn NearestNeighbors(metric='correlation'), brute
 *                            force) on the resident matrix: ind_out / dist_out (N, k), self first, sorted by distance; with
 *                            P_out also calculate_asymmetric_Pij (:17-52) for the given local_connectivity / perplexity.
 *   zk_force_layout_stage    optimize_stage (:236-266), the strictly sequential force-directed sweep over the graph's pairs
 *                            with its tau_rand_int negative sampling: HOST code here as in the reference (numba), operation
 *                            for operation; xy (n_nodes, 2) and rng_state (3) are updated in place, log_out (optional) receives
 *                            xy after every sweep.  force_params = (N, M, alpha, beta).
 * ------------------------------------------------------------------------------------------------------ */
int zk_rows_knn_correlation(zk_rows* rows, int n_neighbors, int local_connectivity, double perplexity, int64_t* ind_out,
                            double* dist_out, double* P_out);
/* numpy.random.RandomState.choice(n, p = uniform) from its one uniform draw u (host arithmetic, no n-sized arrays): the first
 * seed of scikit-learn's k-means++. */
int zk_uniform_choice_index(int64_t n, double u, int64_t* index_out);
/* test hooks of the above: the same index by plain sequential additions (and the last cumulative sum), and the float64 sum of
 * `steps` sequential additions of c -- what numpy.cumsum of a constant array holds at index steps - 1 -- by the jumping method */
int zk_uniform_choice_index_sequential(int64_t n, double u, int64_t* index_out, double* last_out);
double zk_repeated_sum_f64(double c, int64_t steps);
int zk_force_layout_stage(double* xy, int64_t n_nodes, const int64_t* node1, const int64_t* node2, const double* weight,
                          int64_t n_pairs, const int64_t* nbrs_ind, int n_neighbors, int64_t num_iterations,
                          const double* force_params, int num_negative_samples, double learning_rate, int64_t* rng_state,
                          double* log_out);

/* ------------------------------------------------------------------------------------------------------
 * Linear synthesis out = C . T: the device side of ZPs.inverse_transform, patches back from moments (csrc/zk_synth.hip; the
 * reference has no counterpart).  Independent of zk_plan: any table.
 *   table  : host, (n_funcs, n_pixels) float64, C order; uploaded once (its rows padded with zeros to a multiple of 4) and
 *            resident for the object's lifetime.  1 <= n_funcs <= 4096, 1 <= n_pixels <= 2^24.
 *   coeffs : (n_rows, n_funcs) float64, C order
 *   out    : (n_rows, n_pixels) of out_dtype (ZK_F32 | ZK_F64): out[p, x] = sum_j coeffs[p, j] table[j, x], accumulated in
 *            float64 on the matrix cores (v_mfma_f64_16x16x4_f64) and rounded once.  A zero table column gives +0.0.
 * For the Zernike inverse the table is G^-1 diag(s) B (least squares; G = B B^T / area the Gram matrix of the masked basis B)
 * or diag(s) B (the textbook sum), computed by the caller in float64 (mtflearn_amd/features/zernike_polys.py).
 * No atomics, and a row's sum does not depend on its place in the batch: two runs, and two chunkings, agree bit for bit.
 *
 * zk_synth_apply cuts the rows into chunks of at most `chunk_bytes` of coefficients + output (default 256 MiB,
 * zk_synth_set_host_chunk; at least 64 rows) and moves chunk c host -> device -> kernel -> device -> host through three device
 * slots on three streams of the object's own, consecutive chunks overlapping, straight from / into the caller's arrays
 * (page-locked arrays, zk_host_alloc, move by DMA without blocking the calling thread); it returns when out_host is complete.
 * zk_synth_apply_dev enqueues on exactly `hip_stream` (NULL = HIP's default stream) and does not synchronise.
 * n_rows == 0 succeeds and launches nothing.  The object is bound to one device and is not thread-safe.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct zk_synth zk_synth;
int zk_synth_create(int device, int n_funcs, int64_t n_pixels, const double* table_host, zk_synth** out);
int zk_synth_destroy(zk_synth* s);
int zk_synth_set_host_chunk(zk_synth* s, int64_t chunk_bytes);   /* staging size of the host variant */
int zk_synth_apply(zk_synth* s, const double* coeffs_host, int64_t n_rows, int out_dtype /* ZK_F32 | ZK_F64 */, void* out_host);
int zk_synth_apply_dev(zk_synth* s, const double* coeffs_dev, int64_t n_rows, int out_dtype, void* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Rotation alignment of moment rows to templates, and the per-row rotation (csrc/zk_align.hip; the reference has only the
 * scalar-angle zmoments.rotate and never searches the angle).  Independent of zk_plan: any PAIRED label set -- every
 * (n, m > 0) comes with (n, -m); full ZPs sets and zmoments.select()ed sets qualify -- with n <= 40.
 *   rows      : (n_rows, n_poly) float64, C order, real moments with labels n, m (n_poly int32 each, any order);
 *               pair k = (n, |m|) is the complex moment z_k = x_{n,+m} + i x_{n,-m}
 *   templates : host, (n_templates, n_poly) float64 in the same real form, 1 <= n_templates <= 64
 *   select    : host, (n_poly) int32 0 / 1 or NULL (all): the moments that count; both members of a pair alike
 *   c_m       = sum over the selected pairs with |m_k| = m of z_k conj(t_k)
 *   f(theta)  = sum_m Re(c_m exp(-i m theta)) = <rotate(z, theta), t> over the selected real moments, so that
 *               |rotate(z, theta) - t|^2 = |z|^2 + |t|^2 - 2 f(theta); theta in the convention of zmoments.rotate
 *               (Z^c_{n,m} -> Z^c_{n,m} exp(-i m theta)): rotating the row by `angle` brings it onto the template.
 * Grid: f on theta_j = j * ((360 / symmetry) / n_theta) degrees, j < n_theta (numpy.linspace(0, 360 / symmetry, n_theta,
 * endpoint=False)), 1 <= n_theta <= 4096, 1 <= symmetry <= 360; the first maximum wins.  trig_host (optional): the caller's
 * (n_theta, 2 trig_m) table, row j = cos(m theta_j), m = 1 .. trig_m, then sin(m theta_j), with trig_m >= the largest
 * selected |m|; NULL: computed by the library with libm.  Tables stay on the device, the eight most recently used per
 * device: only the first call with a new option set uploads (and synchronises).
 * Refinement: newton_iters (0 .. 16) Newton steps on f' from the grid maximum theta_0, a step only where f'' < 0, every
 * iterate clamped to theta_0 +- one grid step, the result wrapped into [0, 360 / symmetry); it is kept only if f there is
 * >= the grid maximum, else theta_0 stays: score >= max over the grid always.
 *   angle : (n_rows, n_templates) float64 degrees;  score : (n_rows, n_templates) float64 = f(angle)
 *   best  : (n_rows) int32: key ZK_ALIGN_DISTANCE: the first argmin_t fma(-2, score, w_t), w_t = |t|^2 over the selection;
 *           ZK_ALIGN_COSINE: the first argmax_t score * w_t, w_t = 1 / |t|.  key_values_host (n_templates): the w_t, or NULL
 *           (summed by the library in column order).  Any of the three outputs may be NULL.
 * zk_rotate_rows: out[r] = row r rotated by angles[r] degrees, (a, b) -> (a cos m t + b sin m t, b cos m t - a sin m t) per
 * (n, +-m) pair, m = 0 columns copied; out == rows (in place) is allowed and gives the same bits.
 * Everything is checked before any device call; a refused argument is ZK_E_BADARG with a message.  n_rows == 0 succeeds and
 * launches nothing.  No atomics: a row's results do not depend on the launch geometry, on its place in the batch or on the
 * chunking.  The host variants move chunks of at most `chunk_bytes` of input + output (default 256 MiB,
 * zk_align_set_host_chunk; at least 256 rows) through the staging ring of the device and return when the outputs are complete.
 * The *_dev variants enqueue on exactly `hip_stream` (NULL = HIP's default stream) and do not synchronise (templates, labels
 * and key values travel through a page-locked slot of the library's, four calls deep).  Calls are serialised per process.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_ALIGN_DISTANCE 0
#define ZK_ALIGN_COSINE   1
int zk_align_rows(int device, const double* rows_host, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                  const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                  int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                  double* angle_out, double* score_out, int32_t* best_out);
int zk_align_rows_dev(int device, const double* rows_dev, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                      const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                      int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                      double* angle_dev, double* score_dev, int32_t* best_dev, void* hip_stream);
int zk_align_set_host_chunk(int device, int64_t chunk_bytes);   /* staging size of the two host variants */
int zk_rotate_rows(int device, const double* rows_host, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                   const double* angles_host, double* out_host);
int zk_rotate_rows_dev(int device, const double* rows_dev, int64_t n_rows, int n_poly, const int32_t* n, const int32_t* m,
                       const double* angles_dev, double* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * The same alignment for the PLANE layout of the dense path, and the frame route built on it: for every pixel of a frame, which
 * template it looks like, at what rotation and how well (csrc/zk_align.hip; no reference counterpart).
 *   planes : (n_poly, .) float64, moment j of pixel i at planes[j * plane_stride + i], plane_stride >= n_pixels (doubles)
 *   angle, score : (n_templates, .) float64, template t of pixel i at [t * out_plane_stride + i], out_plane_stride >= n_pixels
 *   best   : (n_pixels) int32;  norm2 : (n_pixels) float64 = sum_j s_j x_j^2 over the selected real moments, one fma chain in
 *            ascending column order: with it score becomes a distance (norm2 + |t|^2 - 2 score) or a cosine
 *            (score / sqrt(norm2 |t|^2)).  Any of the four outputs may be NULL.
 * Options, grid, refinement and the best rule are those of zk_align_rows, and so are the bits: the two kernels instantiate one
 * body on two operand layouts, so pixel i of the planes gets exactly what row i of the transposed matrix gets.  Refused with
 * ZK_E_BADARG and a message, before any device call: plane_stride < n_pixels, out_plane_stride < n_pixels, and everything
 * zk_align_rows refuses.  n_pixels == 0 succeeds and launches nothing.  No atomics: a pixel's results do not depend on the launch
 * geometry, on its position, on the strides or on the banding.  zk_align_planes moves chunks of pixels (zk_align_set_host_chunk)
 * through the device's staging ring, a chunk of the operand as n_poly strided pieces; zk_align_planes_dev enqueues on exactly
 * `hip_stream` and does not synchronise (same page-locked slot and table cache as zk_align_rows_dev).
 *
 * zk_frame_align(_dev): output rows [row0, row0 + n_rows) of the maps of a frame, with the plan's labels (which must be a
 * paired set).  The plan's dense transform -- whatever zk_transform_frame_dev resolves for it -- writes a band of rows into the
 * plan's scratch matrix, the planes kernel turns the band into its part of the maps, band after band on one stream: the
 * (n_poly, H, W) moments never exist.  A band holds at most 1 GiB of moments (zk_align_set_band_bytes(device, bytes): less; 0: the
 * default), at least one row, whole multiples of 8 rows where it holds that many.  Zero-padded border positions are computed like
 * any other, as the dense transform returns them.  Outputs: (n_templates, n_rows, W) with out_plane_stride >= n_rows * W between
 * templates, (n_rows, W) for best and norm2; with out = full + row0 * W and out_plane_stride = H * W the band lands inside
 * whole-frame maps.  The *_dev form takes ZK_F32 / ZK_F64 frames on the device, the host form also the narrow formats; calls on
 * one plan share its scratch matrix and are not concurrent.
 * ------------------------------------------------------------------------------------------------------ */
int zk_align_planes(int device, const double* planes_host, int64_t n_pixels, int64_t plane_stride, int n_poly, const int32_t* n,
                    const int32_t* m, const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                    int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                    double* angle_out, double* score_out, int32_t* best_out, double* norm2_out, int64_t out_plane_stride);
int zk_align_planes_dev(int device, const double* planes_dev, int64_t n_pixels, int64_t plane_stride, int n_poly, const int32_t* n,
                        const int32_t* m, const double* templates_host, int n_templates, const int32_t* select, int n_theta,
                        int symmetry, int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                        double* angle_dev, double* score_dev, int32_t* best_dev, double* norm2_dev, int64_t out_plane_stride,
                        void* hip_stream);
int zk_frame_align(zk_plan* plan, const void* image_host, int dtype, int64_t height, int64_t width, int64_t row0, int64_t n_rows,
                   const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                   int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                   double* angle_host, double* score_host, int32_t* best_host, double* norm2_host, int64_t out_plane_stride);
int zk_frame_align_dev(zk_plan* plan, const void* image_dev, int dtype, int64_t height, int64_t width, int64_t row0, int64_t n_rows,
                       const double* templates_host, int n_templates, const int32_t* select, int n_theta, int symmetry,
                       int newton_iters, int key, const double* trig_host, int trig_m, const double* key_values_host,
                       double* angle_dev, double* score_dev, int32_t* best_dev, double* norm2_dev, int64_t out_plane_stride,
                       void* hip_stream);
int zk_align_set_band_bytes(int device, int64_t bytes);   /* moments per band of zk_frame_align; 0: the default */

/* ---------------------------------------------------------------------------------------------------------
 * mtflearn.eels (reference eels/_baseline_correction.py): the baseline of every spectrum of a spectrum image.
 *
 * The operand is (outer, length, inner) of `dtype` (the five image formats, widened exactly to float64 on the device): `length`
 * is the energy axis and each of the outer * inner other indices is one spectrum.  outer == 1 is the native energy-major
 * layout (E, H, W); any other operand is transposed on the device on the way in and out.  baseline (and signal = data -
 * baseline, NULL to skip) are float64 in the operand's layout; iterations (NULL to skip) is (outer, inner) int32.
 *
 *   zk_eels_snip  v = log(log(sqrt(y + 1) + 1) + 1); for pp = 1 .. niter: v[e] = min(v[e], (v[e + pp] + v[e - pp]) / 2) on
 *                 pp <= e < length - pp, every pass from the values of the pass before (a pass with 2 pp >= length changes
 *                 nothing); baseline = (exp(exp(v) - 1) - 1)^2 - 1.  float64 throughout, niter >= 0.
 *   zk_eels_pls   (W + lam D^T D) z = W y, D the differences of `order` (1 .. 3), by a band LDL^T per spectrum:
 *     ZK_EELS_WHITTAKER  one solve with the caller's weights: (length) float64 used for every spectrum
 *                        (weights_per_spectrum == 0) or one weight per sample in the operand's layout (!= 0);
 *     ZK_EELS_ALS        order 2; w = 1, then `itermax` solves with w = param (y > z), 1 - param (y < z), 0 (y == z);
 *     ZK_EELS_ARPLS      order 2; w = 1; per solve d = y - z, m / s the mean / population standard deviation of d[d < 0],
 *                        wt = 1 / (1 + exp(2 (d - (2 s - m)) / s)); stop when |w - wt| / |w| < param, else w = wt;
 *     ZK_EELS_AIRPLS     w = 1; solve i = 1 ..: dssn = |sum d[d < 0]|; stop when dssn < 0.001 sum |y| or i == itermax; else
 *                        w = 0 where d >= 0, exp(i |d| / dssn) where d < 0, and w[0] = w[length - 1] = exp(i max d[d < 0] / dssn).
 *   iterations: the solves a spectrum took (ALS: itermax).  Not pinned: non-finite samples, SNIP input below -1, a spectrum
 *   without a negative residual; every loop is bounded by itermax.
 *
 * One spectrum per lane, no atomics: a spectrum's numbers depend neither on its neighbours nor on the chunking, and the host
 * and the _dev form give the same bits.  The scratch planes (order + 1 float64 per sample and a few more) are cut over the
 * spectra to stay under zk_eels_set_chunk's bytes (0: the default, 1 GiB; at least 64 spectra per chunk).  Everything is
 * checked before any device call; a refused argument is ZK_E_BADARG with a message.  The _dev variants take device pointers
 * (the weights included), run on hip_stream and synchronise it once their scratch is released.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_EELS_WHITTAKER 0
#define ZK_EELS_ALS       1
#define ZK_EELS_ARPLS     2
#define ZK_EELS_AIRPLS    3
int zk_eels_snip(int device, const void* data_host, int dtype, int64_t outer, int64_t length, int64_t inner, int niter,
                 double* baseline_host, double* signal_host);
int zk_eels_snip_dev(int device, const void* data_dev, int dtype, int64_t outer, int64_t length, int64_t inner, int niter,
                     double* baseline_dev, double* signal_dev, void* hip_stream);
int zk_eels_pls(int device, const void* data_host, int dtype, int64_t outer, int64_t length, int64_t inner, int mode, int order,
                double lam, double param, int itermax, const double* weights_host, int weights_per_spectrum,
                double* baseline_host, double* signal_host, int32_t* iterations_host);
int zk_eels_pls_dev(int device, const void* data_dev, int dtype, int64_t outer, int64_t length, int64_t inner, int mode, int order,
                    double lam, double param, int itermax, const double* weights_dev, int weights_per_spectrum,
                    double* baseline_dev, double* signal_dev, int32_t* iterations_dev, void* hip_stream);
int zk_eels_set_chunk(int device, int64_t scratch_bytes);   /* cap of the scratch planes of the four calls above */

/* ---------------------------------------------------------------------------------------------------------
 * Scan-jitter resampling (reference denoise/_noise_models.py:28-57, apply_scan_noise), and the library's general
 * interpolation primitive (csrc/zk_interp.h).
 *
 *   out[z, y, x] = S_z(y + dy[z, x], x + dx[z, y])
 *
 * S_z is the B-spline interpolant of `order` (0: nearest, floor(c + 0.5); 1; 3) of frame z ALONE, extended by `mode` as
 * scipy.ndimage.map_coordinates extends it; the coordinate sums are formed in float64 and so is everything after them.  The
 * stack is (Z, H, W) of `dtype`; the result is float32 for ZK_F32, float64 for every other type (the integer formats are widened
 * exactly).  dx is (Z, H) and dy is (Z, W), float64; no coordinate array exists on either side.
 *   ZK_RESAMPLE_REFLECT        d c b a | a b c d | d c b a      ZK_RESAMPLE_GRID_WRAP       a b c d | a b c d | a b c d
 *   ZK_RESAMPLE_MIRROR         d c b | a b c d | c b a          ZK_RESAMPLE_GRID_CONSTANT   0 0 0 0 | a b c d | 0 0 0 0
 *   ZK_RESAMPLE_NEAREST        a a a a | a b c d | d d d d      ZK_RESAMPLE_CONSTANT        a coordinate outside [0, n - 1] on
 *                                                                                           either axis gives 0 as a whole
 * Taps are folded in the modulo form, so a shift of any number of image sizes is right.  Order 3 is offered for REFLECT,
 * MIRROR and GRID_WRAP: its prefilter (pole sqrt(3) - 2, gain 6 per axis, rows then columns) starts each segment from 32
 * samples of the extended signal, |pole|^32 < 1 ulp, i.e. it is the exact interpolant on an axis of any length -- where the
 * reference's 3-D call differs (it also filters along z and, for REFLECT, starts from a series cut at the axis length).
 *
 * Frames are independent: a frame alone, in a stack, in another run length, and the host and _dev forms give the same bits.
 * Order 3 needs two float64 planes per frame in flight (16 H W bytes).  zk_scan_resample streams whole frames through a staging
 * ring, input + output + scratch of one run staying under zk_scan_resample_set_chunk's bytes (0: the default, 256 MiB; at
 * least one frame).  zk_scan_resample_dev takes device pointers and runs on hip_stream; with scratch_dev (at least one frame's
 * planes; runs are sized to scratch_bytes) or below order 3 it allocates nothing and does not synchronise, otherwise it takes
 * its planes under the same cap and synchronises the stream before it releases them.  Everything is checked before any device
 * call; a refused argument is ZK_E_BADARG with a message.  Not pinned: non-finite samples or shifts.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_RESAMPLE_REFLECT       0
#define ZK_RESAMPLE_MIRROR        1
#define ZK_RESAMPLE_NEAREST       2
#define ZK_RESAMPLE_GRID_WRAP     3
#define ZK_RESAMPLE_GRID_CONSTANT 4
#define ZK_RESAMPLE_CONSTANT      5
int zk_scan_resample(int device, const void* stack_host, int dtype, int64_t Z, int64_t H, int64_t W, const double* dx_host,
                     const double* dy_host, int order, int mode, void* out_host);
int zk_scan_resample_dev(int device, const void* stack_dev, int dtype, int64_t Z, int64_t H, int64_t W, const double* dx_dev,
                         const double* dy_dev, int order, int mode, void* out_dev, void* scratch_dev, int64_t scratch_bytes,
                         void* hip_stream);
int zk_scan_resample_set_chunk(int device, int64_t budget_bytes);

/* ------------------------------------------------------------------------------------------------------
 * mtflearn.datasets.TMDImageSimulator (datasets/_tmd_simulator.py): a batch of float32 frames (batch, height, width), each the
 * sum of its layers (species) in the order given.  Layer l belongs to frame layer_frame[l] (the layers of a frame are
 * consecutive: layer_frame does not decrease; a frame without layers is zero), owns the points
 * [point_offsets[l], point_offsets[l + 1]) of the (n, 3) float64 array of (x, y, scale), and has an amplitude and a half kernel
 * w[0 .. r] = weights[weight_offsets[l] .. weight_offsets[l + 1]), centre first (r >= 0, at most 960).
 *
 *   delta image     float32: the scale of every point (rounded to float32) added at (rint(y), rint(x)) -- default rounding
 *                   mode, as np.round -- in ascending point index with a float32 rounding per add, as np.add.at; a point
 *                   whose pixel is off the frame is dropped.
 *   blur            the column pass (axis 0), then the row pass, each in float64 in SciPy's order of operations for a
 *                   symmetric kernel: t = c w[0], then t += (left + right) w[j] for j = r .. 1.
 *     ZK_TMD_FFT        zeros outside the frame, a float64 intermediate, frame = float32(float64(frame) + amplitude * t):
 *                       the exact fftconvolve(delta, amplitude * outer(g, g), 'same') for g[j] = w[|j|].
 *     ZK_TMD_GAUSSIAN   'reflect' (d c b a | a b c d | d c b a, folded again when r >= n), each pass stored as float32,
 *                       frame = frame + float32(amplitude) * t in float32: amplitude * scipy.ndimage.gaussian_filter(delta).
 *
 * masks, when not NULL, receives the delta images as (n_layers, height, width) float32.  With weights and weight_offsets both
 * NULL there is no blur: only the masks are written and frames may be NULL.  dtype is ZK_F32.  No floating-point atomics, and
 * a frame's result depends on its own layers only: alone, in a batch, from either entry point and on a second run the bits
 * are the same.  The metadata and the points are host arrays in both forms; zk_tmd_render_dev takes frames and masks on the
 * device, runs on hip_stream and synchronises it before it returns (its staging goes with the call).  Everything is checked
 * before any device call; a refused argument is ZK_E_BADARG with a message.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_TMD_FFT      0
#define ZK_TMD_GAUSSIAN 1
int zk_tmd_render(int device, void* frames_host, void* masks_host, int dtype, int64_t batch, int64_t height, int64_t width,
                  int64_t n_layers, const int32_t* layer_frame_host, const int64_t* point_offsets_host, const double* points_host,
                  const double* amplitudes_host, const int64_t* weight_offsets_host, const double* weights_host, int mode);
int zk_tmd_render_dev(int device, void* frames_dev, void* masks_dev, int dtype, int64_t batch, int64_t height, int64_t width,
                      int64_t n_layers, const int32_t* layer_frame_host, const int64_t* point_offsets_host, const double* points_host,
                      const double* amplitudes_host, const int64_t* weight_offsets_host, const double* weights_host, int mode,
                      void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Stack registration (no reference counterpart): the rigid drift of every frame of a (B, H, W) stack against a reference frame
 * to 1 / upsample of a pixel (Guizar-Sicairos, Thurman, Fienup, Opt. Lett. 33, 156 (2008)), and the ordered mean of a stack.
 *
 * shifts[b] = (dy, dx) is the translation that, applied to frame b, registers it onto the reference (scikit-image's sign): for
 * frame_b(y, x) = ref(y - s_y, x - s_x) it is (-s_y, -s_x).  Everything is float64; the integer formats are widened exactly.
 *   spectra      F = fft2(frame * w), R = fft2(ref * w); w[y, x] = wy[y] * wx[x], all 1 (ZK_REGISTER_WINDOW_NONE) or the periodic
 *                Hann window 0.5 - 0.5 cos(2 pi i / n) per axis (ZK_REGISTER_WINDOW_HANN).
 *   cross power  P = R conj(F); with ZK_REGISTER_NORM_PHASE P is divided by max(|P|, 100 eps max|P|), max|P| per frame.
 *   correlation  c = real(ifft2(P)).
 *   coarse peak  (y0, x0): the first maximum of c in flat FFT-layout order over the lags whose wrapped values
 *                (numpy.fft.fftfreq(n, 1 / n)) satisfy |ly| <= max_shift and |lx| <= max_shift; max_shift -1: every lag.  A
 *                lattice image correlates at every lattice vector: max_shift says how far drift can have gone.
 *   upsample 1   the coarse lag is the shift and peak its c.
 *   upsample u   S = ceil(1.5 u), off = S / 2 (integer), ys[j] = y0 + (j - off) / u and xs[i] = x0 + (i - off) / u in float64,
 *                C = real(Ey P Ex) / (H W) with Ey[j, k] = exp(+2 pi i ys[j] fftfreq(H)[k]) and Ex[k, i] = exp(+2 pi i
 *                fftfreq(W)[k] xs[i]); the shift is (ys[j], xs[i]) -- these float64 expressions, bit for bit -- of the first
 *                maximum of C in row-major order, and peak that C.  It is not clamped to max_shift again.  The phases are formed
 *                from the integer k (y0 u + j - off) reduced modulo u H before it meets 2 pi / (u H).
 * Ties go to the smaller flat index.  The reference is frame ref_index of the stack (ZK_REGISTER_REF_INDEX), the (H, W) frame
 * `ref` of ref_dtype (ZK_REGISTER_REF_FRAME), or for frame b the frame b - 1 (ZK_REGISTER_REF_PREVIOUS: frame 0 meets itself and
 * the rows are the pairwise shifts; the caller sums them).  shifts is (B, 2), peak (B).  corr (B, H, W) and up (B, S, S), when
 * not NULL, receive c / (H W)-normalised as above and C (up needs upsample > 1): the planes the answer was read from, for tests.
 * Frames go in runs whose complex fields stay under 1 GiB; no kernel looks across frames, no atomics are used, and a frame
 * alone, in a stack, in the host and the _dev form and on a second run gives the same bits.  2 <= H, W <= 16384, upsample in
 * 1 .. 1000.  Not defined: non-finite samples (nothing scans for them).
 *
 * zk_stack_mean: out[y, x] = (stack[0, y, x] + stack[1, y, x] + ... in ascending order) / B in float64: one division, no atomics.
 *
 * The host forms stream through a staging ring (frames for the shifts, runs of pixels for the mean).  The _dev forms take
 * device pointers and run on hip_stream; zk_register_shifts_dev synchronises it before it releases its fields,
 * zk_stack_mean_dev allocates nothing and does not synchronise.  Everything is checked before any device call; a refused
 * argument is ZK_E_BADARG with a message.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_REGISTER_REF_INDEX    0
#define ZK_REGISTER_REF_FRAME    1
#define ZK_REGISTER_REF_PREVIOUS 2
#define ZK_REGISTER_NORM_NONE    0
#define ZK_REGISTER_NORM_PHASE   1
#define ZK_REGISTER_WINDOW_NONE  0
#define ZK_REGISTER_WINDOW_HANN  1
int zk_register_shifts(int device, const void* stack_host, int dtype, int64_t B, int64_t H, int64_t W, int ref_mode, int64_t ref_index,
                       const void* ref_host, int ref_dtype, int upsample, int64_t max_shift, int normalization, int window,
                       double* shifts_host, double* peak_host, double* corr_host, double* up_host);
int zk_register_shifts_dev(int device, const void* stack_dev, int dtype, int64_t B, int64_t H, int64_t W, int ref_mode, int64_t ref_index,
                           const void* ref_dev, int ref_dtype, int upsample, int64_t max_shift, int normalization, int window,
                           double* shifts_dev, double* peak_dev, double* corr_dev, double* up_dev, void* hip_stream);
int zk_stack_mean(int device, const void* stack_host, int dtype, int64_t B, int64_t H, int64_t W, double* out_host);
int zk_stack_mean_dev(int device, const void* stack_dev, int dtype, int64_t B, int64_t H, int64_t W, double* out_dev, void* hip_stream);

/* ------------------------------------------------------------------------------------------------------
 * Geometric phase analysis (no reference counterpart): the strain and rotation maps of every frame of a (B, H, W) stack from
 * the phases of two Bragg spots (Hytch, Snoeck, Kilaas, Ultramicroscopy 74, 131 (1998)).
 *
 * g (2, 2) on the host: the rows g_k = (gy, gx) are the two Bragg vectors in cycles per pixel; sigma the mask width in cycles
 * per pixel.  Everything is float64; the integer formats are widened exactly.  Axis index a and j: 0 = y, 1 = x.
 *   spectrum     F = fft2(frame * w), w all 1 (ZK_GPA_WINDOW_NONE) or the separable periodic Hann window of the registration
 *                (ZK_GPA_WINDOW_HANN).
 *   planes       M_k[ky, kx] = exp(-(dy^2 + dx^2) / (2 sigma^2)), dy = fftfreq(H)[ky] - gy wrapped to the nearest representative
 *                (dy -= rint(dy)), dx likewise; H_k = ifft2(F M_k) with its 1 / (H W); amplitude_k = |H_k|.
 *   gradient     dP_k/dx = arg(H_k[y, x + 1] conj(H_k[y, x - 1]) c2x_k) / 2 inside, arg(H_k[y, 1] conj(H_k[y, 0]) c1x_k) in the
 *                first and arg(H_k[y, W - 1] conj(H_k[y, W - 2]) c1x_k) in the last column, c1x_k = exp(-2 pi i gx_k) and c2x_k =
 *                exp(-4 pi i gx_k) formed once on the host; y likewise with gy_k.  arg is atan2(imaginary, real): the wrapped
 *                phase is never unwrapped and never demodulated by a position-dependent factor, so no rounding grows with y, x.
 *   reference    (y0, y1, x0, x1), a half-open rectangle inside the frame, or NULL.  m[k][a] = the mean of dP_k/dr_a over the
 *                rectangle (a float64 sum in a fixed tree, divided once; no atomics); dP_k/dr_a -= m[k][a];
 *                G = g + m / (2 pi), the refined Bragg vectors.  NULL: m = 0, G = g.
 *   strain       e[j][a] = du_j/dr_a = -(1 / 2 pi) sum_k inv(G)[j][k] dP_k/dr_a; exx = e[x][x], eyy = e[y][y],
 *                exy = (e[x][y] + e[y][x]) / 2, rotation = (e[y][x] - e[x][y]) / 2 in radians.  A frame I0(r - u(r)) gives
 *                e = grad u to first order.
 *   phase        arg(H_k exp(-2 pi i t)), t = gy y + gx x reduced by t -= floor(t): for display only.
 * maps (4, B, H, W): exx, eyy, exy, rotation.  amp (B, 2, H, W).  g_out (B, 2, 2): G.  phase (B, 2, H, W) and planes
 * (B, 2, H, W) complex float64 (H_k itself, for tests) when not NULL.  Frames go in runs whose three complex fields stay under
 * 1 GiB (zk_gpa_set_run_bytes(device, bytes): another budget; 0: the default); no kernel looks across frames, and a frame
 * alone, in a stack, in runs of any length, in the host and the _dev form and on a second run gives the same bits.
 * 4 <= H, W <= 16384; |g components| <= 0.5; the rows of g non-zero and |det g| > 1e-6 |g_1| |g_2|; sigma finite and > 0.
 * Not defined: non-finite samples (nothing scans for them).
 *
 * zk_gpa streams the frames through a staging ring; zk_gpa_dev takes device pointers, runs on hip_stream and synchronises it
 * before it releases its fields.  g and reference are host pointers in both.  Everything is checked before any device call;
 * a refused argument is ZK_E_BADARG with a message.
 * ------------------------------------------------------------------------------------------------------ */
#define ZK_GPA_WINDOW_NONE 0
#define ZK_GPA_WINDOW_HANN 1
int zk_gpa(int device, const void* stack_host, int dtype, int64_t B, int64_t H, int64_t W, const double* g, double sigma, int window,
           const int64_t* reference, double* maps_host, double* amp_host, double* g_out_host, double* phase_host, void* planes_host);
int zk_gpa_dev(int device, const void* stack_dev, int dtype, int64_t B, int64_t H, int64_t W, const double* g, double sigma, int window,
               const int64_t* reference, double* maps_dev, double* amp_dev, double* g_out_dev, double* phase_dev, void* planes_dev,
               void* hip_stream);
int zk_gpa_set_run_bytes(int device, int64_t bytes);      /* the complex fields of one run of zk_gpa(_dev); 0: the default */

/* Device memory for callers that have no allocator of their own (a NumPy / C user of the *_dev entry points). */
int zk_device_malloc(int device, int64_t bytes, void** out_dev);
int zk_device_free(int device, void* dev);
int zk_device_copy(int device, void* dst, const void* src, int64_t bytes, int kind /* 1 H2D, 2 D2H, 3 D2D */);
int zk_device_synchronize(int device);

/* What this GPU sustains on a plain stream over a caller's buffers, measured with HIP events (bench.py prints it beside the
 * batch kernel's figure, so that a slow box, an unlucky physical placement, or the cost of mixing reads and writes shows as
 * such).  `bytes` of src_dev are read in 256-KiB groups (rounded down):
 *   dst_dev == NULL                          every wave reads contiguous 16-KiB stages through the LDS-DMA engine
 *                                            (global_load_lds nt, the batch kernel's own load instruction) and discards them;
 *   dst_dev != NULL, store_per_group == 0    a 16-B-per-lane copy src -> dst (non-temporal loads and stores);
 *   dst_dev != NULL, store_per_group  > 0    the read stream above, and after each group its wave writes store_per_group
 *                                            bytes (a multiple of 16) to dst_dev + group * store_per_group as 1-KiB
 *                                            non-temporal runs: the batch kernel's traffic mix without its arithmetic
 *                                            (23040 = 64 patches x 45 moments per 256 KiB of float32 32-px patches).
 * *ms_out = average over `reps` launches after one warm-up. */
int zk_hbm_probe(int device, const void* src_dev, void* dst_dev, int64_t bytes, int64_t store_per_group, int reps, double* ms_out);

/* The shader clock while other work runs on the device (measurement aid of bench.py; no reference counterpart): start puts ONE
 * wave on a stream of its own that samples the shader-clock counter against the constant 100-MHz counter and then naps until
 * stop is called or `max_ms` (<= 2000) have passed; stop returns the mean clock in GHz over the `ms` the wave was resident.
 * The FP64-bound kernels of this library run at 1.7-2.2 GHz of the nominal 2.4 (power management), so their rates are stated
 * against the measured clock as well as the nominal one. */
long long zk_debug_strip3_launches(void);  /* launches of the opt-in dense kernel zk_frame_strip3_kernel (ZK_STRIP_V3=1) so far: tests */
typedef struct zk_clock_monitor zk_clock_monitor;
int zk_clock_monitor_start(int device, double max_ms, zk_clock_monitor** out);
int zk_clock_monitor_stop(zk_clock_monitor* monitor, double* ghz_out, double* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* ZERNIKE_HIP_H */

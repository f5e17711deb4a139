#!/usr/bin/env python3
"""The reference notebooks' two Zernike flows on a synthetic frame, through the drop-in API.

  notebook 2 (batch):  key points -> patches -> ZPs.fit_transform(patches) -> rotation-invariant |Z_nm| -> rot_maps
  notebook 3 (dense):  ZPs.fit_transform(frame) -> rot_maps / mirror_map / |Z_nm| maps
  jittered series:     rendered frames -> apply_scan_noise (scan distortion) -> denoise_svd, resident
  defect frames:       TMDImageSimulator stack in one call -> scan noise -> Poisson noise -> local_max, against pts / labels
  resident chain:      lattice rendered on the device -> denoise -> background removal -> local maxima -> moments at them
  refined chain:       the same key points -> sub-pixel centroids -> bond length -> Voronoi bonds -> polygons, all resident
  motifs:              k-means centres of the key-point moments -> ZPs.inverse_transform -> the motif each class stands for
  matching:            kmeans_aligned templates -> ZPs.align_maps -> cosine map from score, norm2, |t| -> local_max
  strain:              a lattice displaced by a known field -> pick_g -> gpa against a reference rectangle -> strain maps

Only the import line differs from the reference (`from mtflearn import ZPs`).  Needs an MI355X.
Run:  python motif-learn_amd/examples/notebook_flows.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mtflearn_amd import ZPs                         # reference: from mtflearn import ZPs
from mtflearn_amd.synthetic import honeycomb_frame


def main():
    frame = honeycomb_frame(1024, seed=7)            # float32 STEM-like frame (the notebooks load a .npy here)
    size, n_max = 32, 10
    zps = ZPs(n_max=n_max, size=size)

    # ---- notebook 2: patches at key points -------------------------------------------------------
    rng = np.random.default_rng(0)
    pts = rng.uniform(size, 1024 - size, size=(5000, 2))                 # stand-in for the peak finder
    ipts = np.rint(pts).astype(int)
    patches = np.array([frame[y - 16:y + 16, x - 16:x + 16] for x, y in ipts])   # KeyPoints.extract_patches
    t = time.perf_counter()
    zm = zps.fit_transform(patches)                                        # (5000, 66) float64, on the GPU
    print(f"batch  : {patches.shape} -> {zm.data.shape} in {1e3 * (time.perf_counter() - t):.1f} ms")
    invariants = np.abs(zm.to_complex().data)                              # rotation-invariant features
    folds = zm.rot_maps([2, 3, 4, 6])                                      # (5000, 4) symmetry scores
    print("         |Z_nm| features", invariants.shape, " rot_maps", folds.shape,
          " dominant fold of patch 0:", [2, 3, 4, 6][int(np.argmax(folds[0]))])
    same = zps.transform_at(frame, pts)                                    # no patch batch at all (extension)
    print("         transform_at == transform(patches):", np.allclose(same.data, zm.data, rtol=1e-9, atol=1e-13))

    # ---- notebook 3: dense symmetry maps -----------------------------------------------------------
    t = time.perf_counter()
    zf = zps.fit_transform(frame)                                          # (66, 1024, 1024) float64
    print(f"dense  : {frame.shape} -> {zf.data.shape} in {1e3 * (time.perf_counter() - t):.1f} ms")
    rot = zf.rot_maps([2, 3, 4, 6])                                        # reference call, NumPy on the host
    t = time.perf_counter()
    maps = zps.symmetry_maps(frame, n_folds=[2, 3, 4, 6])                  # same maps, fused on the GPU
    print(f"fused  : rot_maps + |Z_nm| + mirror_map in {1e3 * (time.perf_counter() - t):.1f} ms;"
          f" max |rot - host rot| = {np.nanmax(np.abs(maps['rot_maps'] - rot)):.2e}")
    valid = zf.valid_mask
    print("         valid (un-padded) positions:", int(valid.sum()), "of", valid.size)

    # ---- the front of the chain, device-resident: the notebooks' input frame is a denoised one -------------------
    from mtflearn_amd import _native
    from mtflearn_amd.datasets import HoneyCombLattice                     # reference: from mtflearn.datasets import ...
    from mtflearn_amd.distributed import (denoise_svd_device, honeycomb_image_device, local_max_device, points_moments_device,
                                          remove_background_device)
    t = time.perf_counter()
    lattice = HoneyCombLattice(size=1024, l=12, seed=7)
    dev = honeycomb_image_device(lattice)                                  # born on the device: only the site coordinates go up
    clean = denoise_svd_device(dev, size, n_components=8)                  # reference: denoise_svd(frame, 32, 8)
    residual, _ = remove_background_device(clean, "opening", 3 * size + 1)
    peaks = local_max_device(residual, 5.0)                                # (N, 2) int32 (x, y) on the device
    keep = peaks.numpy()
    keep = keep[(keep.min(axis=1) >= size // 2) & (keep[:, 0] < 1024 - size // 2) & (keep[:, 1] < 1024 - size // 2)]
    moments = points_moments_device(zps._device_plan(), clean, _native.DeviceArray.from_numpy(keep.astype(np.int32)))
    print(f"chain  : render -> denoise -> background -> local_max -> moments {moments.shape} in {1e3 * (time.perf_counter() - t):.1f} ms")
    sites = np.concatenate(lattice.get_points())                           # the frame's atoms are known: check the peaks
    inner = keep[(keep.min(axis=1) >= 2 * size) & (keep.max(axis=1) < 1024 - 2 * size)]
    dist = np.hypot(inner[:, None, 0] - sites[None, :, 0], inner[:, None, 1] - sites[None, :, 1]).min(axis=1)
    print(f"         {len(inner)} interior peaks, farthest from a lattice site: {dist.max():.2f} px")

    # ---- a jittered series of the same lattice: render -> scan noise -> denoise, the frames never on the host ------------
    from mtflearn_amd.denoise import DenoiseSVD, _jitter, apply_scan_noise
    from mtflearn_amd.resident import scan_noise_device
    t = time.perf_counter()
    frames = _native.DeviceArray((4, 1024, 1024), np.float32)             # the rendered frame is float32
    for k in range(4):                                                     # four exposures of one lattice
        _native.check(_native.load().zk_device_copy(0, frames[k].data_ptr(), dev.data_ptr(), dev.nbytes, 3), "zk_device_copy")
    dx, dy = _jitter(7, frames.shape, 1.0, 0.3)                            # the reference's draws: Z (H + W) numbers go up
    jittered = scan_noise_device(frames, _native.DeviceArray.from_numpy(dx), _native.DeviceArray.from_numpy(dy), order=3)
    cleaned = [denoise_svd_device(jittered[k], size, n_components=8) for k in range(4)]
    print(f"jitter : 4 frames -> scan noise (order 3) -> denoise_svd in {1e3 * (time.perf_counter() - t):.1f} ms, all resident")
    host = apply_scan_noise(frames.numpy(), jx=1.0, jy=0.3, seed=7, order=3)   # reference: apply_scan_noise(frames, 1.0, 0.3, 7, 3)
    print("         host call == resident call:", np.array_equal(host, jittered.numpy()),
          "; DenoiseSVD on the host copy:", DenoiseSVD(host[0], 8, size, None).run().shape)

    # ---- labelled defect frames: simulators -> one device call -> scan noise -> shot noise -> key points against the labels ----
    from mtflearn_amd.datasets import TMDImageSimulator, apply_poisson_noise  # reference: from mtflearn.datasets import ...
    from mtflearn_amd.resident import tmd_frames_device
    t = time.perf_counter()
    sims = []
    for k, theta in enumerate((0.0, 10.0, 20.0, 30.0)):
        sim = TMDImageSimulator(size=(512, 512), a=30, theta=theta)
        sim.add_random_vacancies('X', num_single=6, num_double=6, seed=k)
        sim.add_random_dopants('TM', num_dopants=8, seed=k)
        sims.append(sim)
    stack = tmd_frames_device(sims, consistent_defects=True)               # (4, 512, 512) float32, resident; labels in sims[k].pts / .lbs
    dx, dy = _jitter(3, stack.shape, 0.4, 0.2)
    shaken = scan_noise_device(stack, _native.DeviceArray.from_numpy(dx), _native.DeviceArray.from_numpy(dy), order=1)
    noisy = apply_poisson_noise(shaken.numpy(), counts_per_pixel=400, seed=1)  # the draw is NumPy's: host
    found = local_max_device(_native.DeviceArray.from_numpy(noisy[0]), 6.0, 0.15).numpy()
    print(f"defects: 4 simulators -> tmd_frames_device -> scan noise -> Poisson -> local_max in {1e3 * (time.perf_counter() - t):.1f} ms")
    sim = sims[0]
    names = sorted(set(sim.labels.tolist()))                               # lbs indexes the sorted labels of the whole lattice
    inner = (sim.pts.min(axis=1) >= 8) & (sim.pts.max(axis=1) < 504)
    near = np.hypot(sim.pts[inner, None, 0] - found[None, :, 0], sim.pts[inner, None, 1] - found[None, :, 1]).min(axis=1)
    for name in names:
        of_kind = sim.labels[inner] == name
        print(f"         frame 0, {name:>2}: {int(of_kind.sum()):4d} interior sites, {int((near[of_kind] <= 2.0).sum()):4d} with a peak within 2 px"
              + ("  (a double vacancy leaves nothing to find)" if name == "v2" else ""))
    print("         defect counts of frame 0:", {str(k): int(v) for k, v in sim.get_defect_counts().items()}, "; lbs:", np.bincount(sim.lbs).tolist())

    # ---- a multi-frame acquisition: one simulator, eight jittered exposures -> register -> average -> denoise, no frame on the host ----
    from mtflearn_amd.resident import register_stack_device
    t = time.perf_counter()
    series = tmd_frames_device([sims[0]] * 8, consistent_defects=True)     # (8, 512, 512) float32, resident
    dx, dy = _jitter(5, series.shape, 0.0, 0.0)
    drift = np.random.default_rng(5).uniform(-2.5, 2.5, (8, 2))            # a rigid drift per frame on top of the row jitter
    drift[0] = 0.0
    dx += _jitter(6, series.shape, 0.3, 0.0)[0] + drift[:, 1:2]
    dy += drift[:, 0:1]
    moved = scan_noise_device(series, _native.DeviceArray.from_numpy(dx), _native.DeviceArray.from_numpy(dy), order=3, mode="grid-wrap")
    reg = register_stack_device(moved, reference=0, upsample=100, max_shift=8)   # max_shift: a lattice correlates at every lattice vector
    averaged = denoise_svd_device(reg.mean, size, n_components=8)
    print(f"series : 8 exposures -> scan noise -> register_stack_device -> denoise_svd in {1e3 * (time.perf_counter() - t):.1f} ms, all resident")
    print("         drift found, worst error against the drawn one: "
          f"{np.abs(reg.shifts.numpy() - drift).max():.3f} px; averaged frame {averaged.shape}")

    # ---- the refined chain: key points -> centroids -> estimate_d -> bonds -> polygons, nothing but scalars on the host ------
    from mtflearn_amd.distributed import estimate_d_device, find_regions_device, refine_points_device, vnn_graph_device
    t = time.perf_counter()
    d_keep = _native.DeviceArray.from_numpy(keep.astype(np.int32))
    atoms = refine_points_device(clean, d_keep, size=3)                    # reference: KeyPoints.refine(r=3); (N, 2) float64 (x, y)
    dmax = estimate_d_device(atoms, threshold="otsu")                      # reference: estimate_d(pts)
    bonds = vnn_graph_device(atoms, dmax)                                  # vnn_graph_device(atoms) alone estimates with Li, as the reference
    offsets, vertices, ks, centers, adjacency = find_regions_device(atoms, bonds)
    print(f"refined: refine -> estimate_d ({dmax:.2f} px) -> vnn_graph {bonds.shape} -> find_regions in {1e3 * (time.perf_counter() - t):.1f} ms;"
          f" {int((ks.numpy() == 6).sum())} hexagons of {len(ks)} polygons")
    moved = atoms.numpy() - keep
    print(f"         centroids moved the key points by at most {np.abs(moved).max():.2f} px")
    from mtflearn_amd.distributed import com_refine_device
    cut = com_refine_device(clean, d_keep, 9)                              # reference: com_refine(pts, img, 9); Li per window, 'otsu' on request
    print(f"         thresholded centroids (9 x 9 windows, Li) differ from the plain ones by at most {np.nanmax(np.abs(cut.numpy() - atoms.numpy())):.2f} px")
    from mtflearn_amd import resident
    fit, steps, status = resident.gaussian_fit_device(clean, d_keep, 9, model="circular")   # a 2-D Gaussian per column: (N, 8) x, y, A, widths, angle, g, rss
    fit = fit.numpy()
    print(f"         Gaussian fits (9 x 9, circular): {int((status.numpy() == 0).sum())} of {len(fit)} converged in at most {int(steps.numpy().max())} steps,"
          f" median width {np.median(fit[:, 3]):.2f} px, amplitude {np.median(fit[:, 2]):.3g}; centres differ from the centroids by at most"
          f" {np.nanmax(np.abs(fit[:, :2] - atoms.numpy())):.2f} px")

    # ---- back from moments: what does each k-means class look like? ------------------------------------------------
    from mtflearn_amd.clustering import DeviceRows, kmeans_fit
    from mtflearn_amd.distributed import inverse_transform_device
    t = time.perf_counter()
    with DeviceRows.adopt(moments.data_ptr(), *moments.shape, device=moments.device.index) as rows:
        labels, centres, _ = kmeans_fit(rows, 4, random_state=0)           # (4, 66) centres; the moment matrix stays on the device
    d_centres = _native.DeviceArray.from_numpy(centres)
    motifs = inverse_transform_device(zps, d_centres).numpy()              # (4, 32, 32): least-squares inverse, exact in the basis' span
    threefold = inverse_transform_device(zps, d_centres, m_select=(0, 3, 6)).numpy()   # the same centres, their 3-fold part only
    print(f"motifs : k-means centres {centres.shape} -> patches {motifs.shape} in {1e3 * (time.perf_counter() - t):.1f} ms;"
          f" class sizes {np.bincount(labels, minlength=4).tolist()}")
    share = np.linalg.norm(threefold.reshape(4, -1), axis=1) / np.linalg.norm(motifs.reshape(4, -1), axis=1)
    print("         share of each motif carried by |m| in (0, 3, 6):", np.round(share, 2).tolist())
    print("         same patches from the host call:", np.array_equal(motifs, zps.inverse_transform(centres)))

    # ---- the same classes with the rotation taken out: aligned k-means, sharp motifs ----------------------------------
    from mtflearn_amd.clustering import kmeans_aligned
    X = moments.numpy()
    t = time.perf_counter()
    a_labels, a_centres, a_angles, a_inertia, a_iter = kmeans_aligned(X, zps.n, zps.m, 4, init=centres)
    a_motifs = zps.inverse_transform(a_centres)                            # beside `motifs`: one orientation per class
    print(f"         aligned k-means from the plain centres: {a_iter} iterations in {1e3 * (time.perf_counter() - t):.1f} ms, class sizes"
          f" {np.bincount(a_labels, minlength=4).tolist()}, aligned motifs {a_motifs.shape}; orientation per atom in [0, 360):"
          f" {np.round(a_angles[:4], 1).tolist()} ...")

    # ---- finding the motifs: the aligned centres as templates, every pixel of the frame matched against them -----------------
    from mtflearn_amd.features import local_max
    t = time.perf_counter()
    found_maps = zps.align_maps(clean.numpy(), a_centres, key="cosine")    # angle / score (4, H, W), best (H, W), norm2 (H, W)
    t_norm2 = (a_centres ** 2).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):                   # cosine of a pixel's moments with its best template, rotated
        cosine = np.take_along_axis(found_maps.score, found_maps.best[None].astype(np.int64), axis=0)[0] / np.sqrt(
            found_maps.norm2 * t_norm2[found_maps.best])
    cosine = np.where(np.isfinite(cosine) & zps._valid_mask(*cosine.shape), cosine, 0.0)
    sites_found = local_max(cosine, 5.0, threshold=0.9)                    # (N, 2) (x, y): where a learned motif sits
    print(f"match  : align_maps of {cosine.shape} against {a_centres.shape[0]} templates -> cosine map -> local_max in"
          f" {1e3 * (time.perf_counter() - t):.1f} ms; {len(sites_found)} matches above 0.9, per class"
          f" {np.bincount(found_maps.best[sites_found[:, 1], sites_found[:, 0]], minlength=a_centres.shape[0]).tolist()}")

    # ---- strain: how the lattice is deformed -- geometric phase analysis of a frame with a known displacement bump ---------------
    from mtflearn_amd import strain
    yy, xx = np.meshgrid(np.arange(512.0), np.arange(512.0), indexing="ij")
    lattice_g = np.array([[0.0, 1 / 16], [1 / 16 * np.sqrt(3) / 2, -1 / 32]])   # a hexagonal pair, 16 px period
    bump = 0.4 * np.exp(-((yy - 300) ** 2 + (xx - 330) ** 2) / (2 * 40.0 ** 2))  # u = (0, bump): atoms pushed along x
    strained = sum(np.cos(2 * np.pi * (gy * yy + gx * (xx - bump))) for gy, gx in (*lattice_g, lattice_g[0] + lattice_g[1])).astype(np.float32)
    t = time.perf_counter()
    g = strain.pick_g(strained)                                            # the two strongest independent Bragg spots
    res = strain.gpa(strained, g, reference=(32, 160, 32, 160), window="hann")
    truth = np.gradient(bump, axis=1)                                      # exx = d u_x / dx
    inner = (slice(64, 448), slice(64, 448))
    print(f"strain : pick_g -> gpa of {strained.shape} in {1e3 * (time.perf_counter() - t):.1f} ms; g {np.round(res.g, 4).tolist()};"
          f" exx in [{res.exx[inner].min():.4f}, {res.exx[inner].max():.4f}] against the field's [{truth.min():.4f}, {truth.max():.4f}],"
          f" worst |exx - truth| inside {np.abs(res.exx - truth)[inner].max():.1e}, |rotation| <= {np.abs(res.rotation[inner]).max():.4f} rad")


if __name__ == "__main__":
    main()

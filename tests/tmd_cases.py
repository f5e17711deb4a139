"""The case table of the TMDImageSimulator tests: shared by tests/make_golden_tmd.py (which runs the reference's class on it)
and by tests/test_tmd_cpu.py / tests/test_gpu_tmd.py (which run mtflearn_amd's).  The smallest shapes at which each piece can
still go wrong:

    A  (64, 80)  a = 30   theta = 0     the defaults; not square, a width that is no multiple of the 64-pixel tile
    B  (96, 64)  a = 31   theta = 0     X sites on half-integer x: round-half-even decides the pixel
    C  (64, 64)  a = 7.5  theta = 17.3  overlapping kernels; random vacancies and dopants (the reference's index mix-up)
    D  (24, 20)  a = 0.7  theta = 5     several atoms per pixel with different scales: the order of the float32 adds shows
    E  (20, 56)  a = 9    theta = 40    three species, sigma = 6: halos of 18 (FFT) and 24 (Gaussian, above the frame height)
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tmd_golden.npz")

CASES = {
    "A": dict(size=(64, 80), a=30, theta=0.0),
    "B": dict(size=(96, 64), a=31, theta=0.0),
    "C": dict(size=(64, 64), a=7.5, theta=17.3),
    "D": dict(size=(24, 20), a=0.7, theta=5.0),
    "E": dict(size=(20, 56), a=9, theta=40.0,
              basis=[(0.0, 0.0, 'TM'), (1 / 3, 1 / 3, 'X'), (2 / 3, 2 / 3, 'Y')],
              species_params={'TM': {'sigma': 6.0, 'A': 1.0}}),
}
MODES = {"fft": True, "gauss": False}
D_INTENSITIES = (0.8, 0.3, 0.55, 0.1, 0.7)          # no two neighbours in the cycle alike: colliding atoms differ
PTS_ALL_IN_FULL = 5000                              # sites: above it the golden holds the digest of pts_all only
DEFAULT_PARAMS = {'sigma': 2.0, 'A': 1.0}


def build(cls, name, use_fft):
    """An instance of ``cls`` (the reference's class or mtflearn_amd's) for case ``name``, its defects in place."""
    sim = cls(use_fft=use_fft, **CASES[name])
    if name == "C":
        sim.add_random_vacancies('X', 3, 3, seed=1)
        sim.add_random_dopants('TM', 4, seed=2)
    if name == "D":                                  # per-species indices, straight into the list simulate() reads
        coords = sim.generate_lattice()
        for label in ('TM', 'X'):
            for k in range(0, len(coords[label]), 2):
                sim.dopants.append((label, k, D_INTENSITIES[(k // 2) % len(D_INTENSITIES)]))
    return sim


def species_of(name):
    """Species in order of first appearance in the basis."""
    basis = CASES[name].get("basis") or [(0.0, 0.0, 'TM'), (1 / 3, 1 / 3, 'X')]
    return list(dict.fromkeys(b[2] for b in basis))


def params_of(name, label):
    table = CASES[name].get("species_params") or {'TM': {'sigma': 2.0, 'A': 1.0}, 'X': {'sigma': 1.5, 'A': 0.6}}
    return table.get(label, DEFAULT_PARAMS)


def digest(array):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(array).tobytes()).digest(), dtype=np.uint8)


def host_record(sim):
    """What a simulator's host side leaves behind after ``simulate``, as arrays (the golden's ``<case>/...`` entries)."""
    out = {"pts_all_sha256": digest(sim.pts_all), "pts_all_shape": np.array(sim.pts_all.shape), "pts": sim.pts,
           "labels": np.asarray(sim.labels), "lbs": np.asarray(sim.lbs)}
    if len(sim.pts_all) <= PTS_ALL_IN_FULL:
        out["pts_all"] = sim.pts_all
    for label, indices in sim.filtered_indices.items():
        out[f"filtered/{label}"] = np.asarray(indices, dtype=np.int64)
    for kind, entries in (("vacancies", sim.vacancies), ("dopants", sim.dopants)):
        out[f"{kind}/label"] = np.array([e[0] for e in entries], dtype="U8")
        out[f"{kind}/index"] = np.array([e[1] for e in entries], dtype=np.int64)
        out[f"{kind}/scale"] = np.array([e[2] for e in entries], dtype=np.float64)
    counts = sim.get_defect_counts()
    out["counts/keys"] = np.array(sorted(counts), dtype="U8")
    out["counts/values"] = np.array([counts[k] for k in sorted(counts)], dtype=np.int64)
    return out


def load_golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}

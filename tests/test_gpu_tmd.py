"""GPU checks of mtflearn_amd.datasets.TMDImageSimulator (csrc/zk_tmd.hip) on the cases of tests/tmd_cases.py.

    masks            the reference's, array_equal, in every case and mode;
    Gaussian mode    the reference's image, array_equal, for up to two species; for three (case E, whose recorded walk was
                     Y, TM, X) within S spacing32(peak): the only freedom is the order of S float32 adds of identical terms;
    FFT mode         max |ours - E| <= (S / 2) spacing32(peak) + 1e-12 peak, E the exact float64 convolution (tests/tmd_oracle.py)
                     and peak its maximum: each of the S accumulations rounds once -- and against the reference
                     max |ours - golden| <= e_ref + the same, e_ref = max |golden - E| computed here from the golden and E;
    reproducibility  a frame alone, in a batch of other simulators, through zk_tmd_render, through tmd_frames_device and run
                     twice: identical bits; `out=` is written into, and return_masks leaves the image as it is.

tests/test_tmd_cpu.py shows on the CPU that the oracle is the reference where the reference is exact."""
import numpy as np
import pytest

import tmd_cases as tc
import tmd_oracle as to
from mtflearn_amd import _native, datasets, resident

pytestmark = pytest.mark.gpu
VARIANTS = [(name, mode) for name in tc.CASES for mode in tc.MODES]


@pytest.fixture(scope="module")
def golden():
    return tc.load_golden()


@pytest.fixture(scope="module")
def rendered():
    """Every case and mode once: ``(simulator, image, {label: mask})``, left unchanged by the tests that share it."""
    out = {}
    for name, mode in VARIANTS:
        sim = tc.build(datasets.TMDImageSimulator, name, tc.MODES[mode])
        image, masks = sim.simulate(return_masks=True)
        out[name, mode] = (sim, image, masks)
    return out


def reference_order(golden, name, mode):
    return [str(s) for s in golden[f"{name}/{mode}/species"]]


@pytest.mark.parametrize("name,mode", VARIANTS)
def test_masks_equal_the_reference(golden, rendered, name, mode):
    sim, image, masks = rendered[name, mode]
    assert list(masks) == tc.species_of(name) and image.dtype == np.float32 and image.shape == tuple(sim.size)
    for k, label in enumerate(reference_order(golden, name, mode)):
        assert masks[label].dtype == np.float32
        np.testing.assert_array_equal(masks[label], golden[f"{name}/{mode}/masks"][k], err_msg=f"{name}/{mode}/{label}")


@pytest.mark.parametrize("name", list(tc.CASES))
def test_gaussian_mode_against_the_reference(golden, rendered, name):
    _, image, _ = rendered[name, "gauss"]
    want = golden[f"{name}/gauss/image"]
    n_species = len(tc.species_of(name))
    worst = np.abs(image.astype(np.float64) - want).max()
    print(f"case {name} gauss: max |ours - reference| = {worst:.3e}")
    if n_species <= 2:
        np.testing.assert_array_equal(image, want)
    else:
        assert worst <= n_species * float(np.spacing(np.float32(want.max())))


@pytest.mark.parametrize("name", list(tc.CASES))
def test_gaussian_mode_equals_the_oracle_in_our_order(golden, rendered, name):
    """Bit for bit in every case, three species included: the oracle adds them in order of first appearance, as we do."""
    _, image, masks = rendered[name, "gauss"]
    species = tc.species_of(name)
    np.testing.assert_array_equal(image, to.gauss_image([masks[s] for s in species], [tc.params_of(name, s) for s in species]))


@pytest.mark.parametrize("name", list(tc.CASES))
def test_fft_mode_against_the_exact_convolution(golden, rendered, name):
    _, image, _ = rendered[name, "fft"]
    order = reference_order(golden, name, "fft")
    E = to.exact_image(list(golden[f"{name}/fft/masks"]), [tc.params_of(name, s) for s in order])
    bound = to.fft_bound(E, len(order))
    ours = np.abs(image.astype(np.float64) - E).max()
    e_ref = np.abs(golden[f"{name}/fft/image"].astype(np.float64) - E).max()
    against = np.abs(image.astype(np.float64) - golden[f"{name}/fft/image"]).max()
    print(f"case {name} fft: max |ours - E| = {ours:.3e} (bound {bound:.3e}); e_ref = {e_ref:.3e}; max |ours - reference| = {against:.3e}")
    assert ours <= bound
    assert against <= e_ref + bound


def test_consistent_defects(rendered):
    """Case C with the labelled atoms dimmed: the oracle's masks, its Gaussian image bit for bit, E within the FFT bound --
    and not the default frame."""
    species = tc.species_of("C")
    params = [tc.params_of("C", s) for s in species]
    for mode, use_fft in tc.MODES.items():
        sim = tc.build(datasets.TMDImageSimulator, "C", use_fft)
        image, masks = sim.simulate(return_masks=True, consistent_defects=True)
        site_labels = np.tile(np.array([b[2] for b in sim.basis]), len(sim.pts_all) // len(sim.basis))
        want = []
        for label in species:
            atoms = sim._cached_coords[label]
            own = np.flatnonzero(site_labels == label)
            want.append(to.delta(sim.size, atoms, to.scales(len(atoms), label, sim.vacancies, sim.dopants, own)))
            np.testing.assert_array_equal(masks[label], want[-1])
        assert not np.array_equal(image, rendered["C", mode][1])
        if use_fft:
            E = to.exact_image(want, params)
            assert np.abs(image.astype(np.float64) - E).max() <= to.fft_bound(E, len(species))
        else:
            np.testing.assert_array_equal(image, to.gauss_image(want, params))
        # every labelled defect on the frame is dimmed where the labels say
        marked = sim.pts[np.isin(sim.labels, ["v1", "v2", "D"])]
        assert len(marked) == 10
        stack = sum(masks[s] for s in species)                 # at a = 7.5 no two atoms share a pixel
        for x, y in marked:
            row, col = int(np.round(y)), int(np.round(x))
            if row < 64 and col < 64:                          # a site within half a pixel of the far edge rounds off the frame
                assert stack[row, col] < 1.0


@pytest.mark.parametrize("mode", list(tc.MODES))
def test_same_bits_alone_batched_host_entry_and_twice(rendered, mode):
    build =lambda name: tc.build(datasets.TMDImageSimulator, name, tc.MODES[mode])
    sims = [build("C"), datasets.TMDImageSimulator(size=(64, 64), a=11, theta=3.0, use_fft=tc.MODES[mode]), build("C")]
    alone, alone_masks = rendered["C", mode][1], rendered["C", mode][2]
    frames, masks = resident.tmd_frames_device(sims, return_masks=True)
    assert frames.shape == (3, 64, 64) and masks.shape == (3, 2, 64, 64) and masks.dtype == np.float32
    frames, masks = frames.numpy(), masks.numpy()
    for b in (0, 2):
        np.testing.assert_array_equal(frames[b], alone)
        for k, label in enumerate(tc.species_of("C")):
            np.testing.assert_array_equal(masks[b, k], alone_masks[label])
    assert not np.array_equal(frames[1], alone)
    np.testing.assert_array_equal(frames[1], sims[1].simulate())
    again = resident.tmd_frames_device(sims)                  # a second run, without masks
    np.testing.assert_array_equal(again.numpy(), frames)
    # out= is written into and returned
    out = _native.DeviceArray((3, 64, 64), np.float32, _native.default_device())
    assert resident.tmd_frames_device(sims, out=out) is out
    np.testing.assert_array_equal(out.numpy(), frames)
    # the host entry point, handed the same layers
    layers = []
    for b, sim in enumerate(sims):
        layers += [(b,) + layer[1:] for layer in sim._layers()]
    host, host_masks = np.full((3, 64, 64), np.nan, np.float32), np.full((6, 64, 64), np.nan, np.float32)
    datasets._tmd_render_host(host, host_masks, layers, True, tc.MODES[mode])
    np.testing.assert_array_equal(host, frames)
    np.testing.assert_array_equal(host_masks.reshape(3, 2, 64, 64), masks)


def test_torch_out_and_masks():
    torch = pytest.importorskip("torch")
    sims = [tc.build(datasets.TMDImageSimulator, "A", True), tc.build(datasets.TMDImageSimulator, "A", True)]
    out = torch.full((2, 64, 80), float("nan"), dtype=torch.float32, device="cuda")
    got, masks = resident.tmd_frames_device(sims, return_masks=True, out=out)
    assert got is out and isinstance(masks, torch.Tensor) and tuple(masks.shape) == (2, 2, 64, 80)
    want = sims[0].simulate()
    np.testing.assert_array_equal(out.cpu().numpy()[0], want)
    np.testing.assert_array_equal(out.cpu().numpy()[1], want)


def test_place_atoms_delta_and_edge_frames(golden):
    sim = tc.build(datasets.TMDImageSimulator, "D", True)
    atoms = sim._cached_coords["TM"]
    scales = to.scales(len(atoms), "TM", sim.vacancies, sim.dopants)
    k = reference_order(golden, "D", "fft").index("TM")
    np.testing.assert_array_equal(sim.place_atoms_delta(atoms, scales), golden["D/fft/masks"][k])
    # half-integer positions round to even; -0.4 rounds to pixel 0; everything else is off the frame
    tiny = datasets.TMDImageSimulator(size=(3, 5))
    positions = np.array([[0.5, 0.5], [1.5, 2.5], [-0.4, -0.5], [4.49, 2.49], [4.5, 2.0], [2.0, 2.5], [-0.51, 1.0], [1e300, 1.0]])
    values = np.array([1.0, 0.5, 0.25, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=np.float32)
    np.testing.assert_array_equal(tiny.place_atoms_delta(positions, values), to.delta((3, 5), positions[:7], values[:7]))
    # a frame one pixel wide and one of a single pixel, both modes: radius far above the frame
    for size in ((7, 1), (1, 1)):
        for use_fft in (True, False):
            one = datasets.TMDImageSimulator(size=size, a=2.0, use_fft=use_fft)
            image, masks = one.simulate(return_masks=True)
            species = ["TM", "X"]
            params = [tc.params_of("A", s) for s in species]
            if use_fft:
                E = to.exact_image([masks[s] for s in species], params)
                assert np.abs(image - E).max() <= to.fft_bound(E, 2)
            else:
                np.testing.assert_array_equal(image, to.gauss_image([masks[s] for s in species], params))

"""The kernels of csrc/zk_regions.hip past the sizes the reference's goldens reach, against the host walk of
tests/regions_oracle.py (held to the reference by tests/test_regions_cpu.py, which also proves these inputs): cycles either side
of 2^10 and 2^12 wedges, a dead-end path longer than any cycle, a row of 700 for the angular sort's linear count, and a tied
minimum x that the argmin sweep meets in different lanes and strides.

Criteria, those of tests/test_gpu_regions.py, no tolerance: ``np.array_equal`` on ``offsets`` / ``vertices`` / ``ks``, byte
equality on ``centers``, set equality on the symmetrised adjacency.  Every case asserts its own conditioning when it is built."""
import numpy as np
import pytest

import regions_cases as rc
import regions_oracle as oracle
from mtflearn_amd import _native, distributed, graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracles():
    """The host walk of every case, computed once."""
    return {name: oracle.regions(*case) for name, case in rc.kernel_cases().items()}


def same_as_oracle(name, ref, offsets, vertices, ks, centers, adjacency):
    for key, got, want in (("offsets", offsets, ref[0]), ("vertices", vertices, ref[1]), ("ks", ks, ref[2])):
        assert got.dtype == np.int64 and np.array_equal(got, want), (name, key)
    assert centers.dtype == np.float64 and centers.shape == ref[3].shape and centers.tobytes() == ref[3].tobytes(), (name, "centers")
    assert adjacency.dtype == np.int64 and adjacency.ndim == 2 and adjacency.shape[1] == 2
    assert oracle.symmetrised(adjacency) == oracle.symmetrised(ref[4]), (name, "adjacency")
    sizes, counts = np.unique(ks, return_counts=True)
    assert dict(zip(sizes.tolist(), counts.tolist())) == rc.KERNEL_EXPECTED_KS[name], name


def device_call(kind, pts, ijs):
    if kind == "host":
        return graph._regions_arrays(pts, ijs)
    out = distributed.find_regions_device(_native.DeviceArray.from_numpy(pts), _native.DeviceArray.from_numpy(ijs))
    return [a.numpy() for a in out]


@pytest.mark.parametrize("kind", ["host", "resident"])
@pytest.mark.parametrize("name", rc.KERNEL_NAMES)
def test_regions_equal_the_host_walk(oracles, name, kind):
    pts, ijs = rc.kernel_cases()[name]
    same_as_oracle(name, oracles[name], *device_call(kind, pts, ijs))


@pytest.mark.parametrize("kind", ["host", "resident"])
def test_first_of_a_tied_minimum_takes_the_grown_edge(kind):
    """Nodes 2500, 1030, 2047 and 2054 share the smallest x: lanes 452, 6, 1023 and again 6 of the argmin sweep, in strides 2, 1, 1
    and 2.  ``np.argmin`` takes 1030, the grown node's only neighbour.  The grown node never appears in ``vertices``, but its
    edge kills the outer face of the triangle it hangs on: that triangle (343, of nodes 1029 .. 1031) keeps one face where every
    other one keeps two.  A grown edge on 2047, 2054 or 2500 would leave triangle 343 both faces and take one from 682, 684 or
    833."""
    pts, ijs = rc.kernel_cases()["tied_min_triangles"]
    assert int(np.argmin(pts[:, 0])) == 1030 and (pts[:, 0] == pts[:, 0].min()).sum() == len(rc.TIED_TRIANGLE_NODES)
    offsets, vertices, ks, centers, adjacency = device_call(kind, pts, ijs)
    assert set(ks.tolist()) == {3}
    faces_of = np.bincount(vertices[offsets[:-1]] // 3, minlength=1000)       # faces per triangle, by any one vertex
    assert faces_of[1030 // 3] == 1
    assert np.array_equal(np.flatnonzero(faces_of != 2), [1030 // 3])
    assert len(adjacency) == 3 * 999                                         # the free triangles' two faces share their three bonds


def test_two_runs_give_identical_bytes():
    for name in ("ring_4093", "chain_5000", "tied_min_3000"):
        pts, ijs = rc.kernel_cases()[name]
        first, second = graph._regions_arrays(pts, ijs), graph._regions_arrays(pts, ijs)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), name

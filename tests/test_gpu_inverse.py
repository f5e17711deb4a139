"""``ZPs.inverse_transform`` / ``_native.Synthesis`` / ``distributed.inverse_transform_device`` on the GPU (csrc/zk_synth.hip).

Bounds, all elementwise and derived (tests/inverse_cases.py), none tuned:
  kernel against NumPy    |got - C @ T| <= 4 (P + 4) 2^-53 (|C| @ |T|): a P-term sum in any order on both sides; float32 output adds
                          2^-24 |C @ T|, its one rounding.
  round trip              X = C B -> transform -> inverse_transform: 1e-12 max|Z| max_x sum_j |T[j, x]| (the project's parity
                          floor of the forward transform, carried through the table) plus the kernel bound.
  partition of |m|        the outputs of the parts add up to the full output within the kernel bound itself, |T| the full table.
  linearity               inverse(a Z1 + Z2) against a R1 + R2 within the kernel bound itself, C = a Z1 + Z2.
The raw-table cases use tables without any symmetry, so a transposed MFMA operand cannot pass.  (100, 40) has more than 96
coefficients, which take the LDS tile in two slices."""
import numpy as np
import pytest

import inverse_cases as ic
from mtflearn_amd import _native, clustering, distributed

pytestmark = pytest.mark.gpu

TABLES = [(15, 64), (15, 81), (45, 289), (66, 1089), (91, 4096), (1, 1), (5, 7), (100, 40)]
ROWS = [1, 15, 16, 17, 257, 1000]


def raw_case(p, x):
    rng = np.random.default_rng(1000 * p + x)
    return rng.standard_normal((max(ROWS), p)), rng.standard_normal((p, x))


def within(got, ref, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print(f"{what}: max |err| {err.max() if err.size else 0.0:.3e}, worst err / bound {worst:.3f}")
    assert got.shape == ref.shape
    assert (err <= bound).all(), what


def on_stream(synth, coeffs, dtype):
    """``apply_dev`` on a stream that is not the default one."""
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = torch.from_numpy(np.ascontiguousarray(coeffs)).cuda()
        out = torch.empty((len(coeffs), synth.n_pixels), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
        assert stream.cuda_stream != 0
        synth.apply_dev(c.data_ptr(), len(coeffs), out.data_ptr(), _native.dtype_code(np.dtype(dtype)), stream.cuda_stream)
    stream.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("p,x", TABLES)
def test_kernel_against_numpy_with_an_arbitrary_table(p, x):
    c_all, t = raw_case(p, x)
    synth = _native.Synthesis.create(t)
    try:
        assert (synth.n_funcs, synth.n_pixels) == (p, x)
        for n in ROWS:
            c = c_all[:n]
            ref, bound = c @ t, ic.sum_bound(c, t)
            got64 = synth.apply(c)
            assert got64.dtype == np.float64
            within(got64, ref, bound, f"({p}, {x}) N={n} float64")
            got32 = synth.apply(c, np.float32)
            assert got32.dtype == np.float32
            within(got32, ref, bound + 2.0 ** -24 * np.abs(ref), f"({p}, {x}) N={n} float32")
            np.testing.assert_array_equal(got32, got64.astype(np.float32))        # rounded once from the float64 accumulator
            np.testing.assert_array_equal(synth.apply(c), got64)                  # two runs, bit for bit
            np.testing.assert_array_equal(synth.apply(c, np.float32), got32)
            np.testing.assert_array_equal(on_stream(synth, c, np.float64), got64)
            np.testing.assert_array_equal(on_stream(synth, c, np.float32), got32)
    finally:
        synth.close()


def test_chunking_changes_no_bit():
    p, x, n = 45, 1024, 1000
    rng = np.random.default_rng(7)
    c, t = rng.standard_normal((n, p)), rng.standard_normal((p, x))
    synth = _native.Synthesis.create(t)
    try:
        whole = {dt: synth.apply(c, dt) for dt in (np.float64, np.float32)}
        within(whole[np.float64], c @ t, ic.sum_bound(c, t), "unchunked")
        for dt, item in ((np.float64, 8), (np.float32, 4)):
            synth.set_host_chunk(384 * (8 * p + item * x))          # 384 rows a chunk: 384 + 384 + 232
            np.testing.assert_array_equal(synth.apply(c, dt), whole[dt])
            synth.set_host_chunk(1)                                 # the smallest chunk there is, 64 rows: 15 full and one of 40
            np.testing.assert_array_equal(synth.apply(c, dt), whole[dt])
        synth.set_host_chunk(0)
        empty = synth.apply(np.zeros((0, p)))
        assert empty.shape == (0, x) and empty.dtype == np.float64
    finally:
        synth.close()
    z = ic.zps(9, 4)
    for dt in (np.float64, np.float32):
        out = z.inverse_transform(np.zeros((0, len(z.n))), dtype=dt)
        assert out.shape == (0, 9, 9) and out.dtype == dt


def test_slots_freed_after_a_large_job_are_created_again():
    """Three full slots of 2048 rows (17 MiB each) are above what an object keeps between calls (32 MiB): the call frees them at
    its end, and the next call, large or small, stages through new ones.  A fourth, partial chunk reuses slot 0 before that."""
    table = ic.zps(32, 8)._synthesis_entry("lstsq", None)["table"]
    p, x = table.shape
    assert (p, x) == (45, 1024)
    n = 3 * 2048 + 100
    c = np.random.default_rng(11).standard_normal((n, p))
    synth = _native.Synthesis.create(table)
    try:
        whole = synth.apply(c)                                          # one chunk at the default budget
        within(whole, c @ table, ic.sum_bound(c, table), "one chunk")
        synth.set_host_chunk(2048 * 8 * (p + x))
        np.testing.assert_array_equal(synth.apply(c), whole)
        synth.set_host_chunk(0)
        np.testing.assert_array_equal(synth.apply(c[:100]), whole[:100])
    finally:
        synth.close()


@pytest.mark.parametrize("size,n_max,n", [(9, 4, 257), (17, 8, 257), (32, 8, 257), (33, 10, 257), (64, 12, 17)])
def test_round_trip_on_the_device(size, n_max, n):
    z = ic.zps(size, n_max)
    _, x = ic.span_patches(z, n, seed=size + n_max)
    zm = z.transform(x)
    back = z.inverse_transform(zm)
    assert back.shape == x.shape and back.dtype == np.float64
    table = z._synthesis_entry("lstsq", None)["table"]
    bound = 1e-12 * np.abs(zm.data).max() * np.abs(table).sum(axis=0)[None, :] + ic.sum_bound(zm.data, table)
    within(back.reshape(n, -1), x.reshape(n, -1), bound, f"round trip ({size}, {n_max})")
    outside = ~ic.basis(z).any(axis=0)
    flat = back.reshape(n, -1)[:, outside]
    assert outside.any() and not flat.any() and not np.signbit(flat).any()       # exactly +0.0 outside the disk
    back32 = z.inverse_transform(zm, dtype=np.float32)
    np.testing.assert_array_equal(back32, back.astype(np.float32))
    # the textbook sum is the other table, and misses these patches (why it is not the default)
    direct = z.inverse_transform(zm, method="direct")
    within(direct.reshape(n, -1), zm.data @ ic.numpy_table(z, "direct"), ic.sum_bound(zm.data, ic.numpy_table(z, "direct")), "direct")
    assert np.abs(direct - x).max() > 0.1 * np.abs(x).max()


def test_selection_and_linearity():
    z = ic.zps(33, 10)
    n = 257
    rng = np.random.default_rng(5)
    z1, z2 = rng.standard_normal((2, n, len(z.n)))
    full = z.inverse_transform(z1)
    parts = ic.m_partition(z)
    total = sum(z.inverse_transform(z1, m_select=p) for p in parts)
    table = z._synthesis_entry("lstsq", None)["table"]
    within(total.reshape(n, -1), full.reshape(n, -1), ic.sum_bound(z1, table), "partition of |m|")
    one = z.inverse_transform(z1, m_select=(0, 3, 6))
    picked = z._synthesis_entry("lstsq", (0, 3, 6))["table"]          # (pinned to NumPy's own table by tests/test_inverse_cpu.py)
    within(one.reshape(n, -1), z1 @ picked, ic.sum_bound(z1, picked), "m_select=(0, 3, 6) against its table")

    from mtflearn_amd.features.moments import zmoments
    zc = zmoments(z1, z.n, z.m, patch_size=z.size).to_complex()
    assert zc.is_complex
    np.testing.assert_array_equal(z.inverse_transform(zc), z.inverse_transform(zc.to_real()))
    np.testing.assert_array_equal(z.inverse_transform(zmoments(z1, z.n, z.m, patch_size=z.size)), full)

    a = -2.75
    mixed = z.inverse_transform(a * z1 + z2)
    within(mixed.reshape(n, -1), (a * full + z.inverse_transform(z2)).reshape(n, -1), ic.sum_bound(a * z1 + z2, table),
           "linearity")


@pytest.mark.parametrize("kind", ["native", "torch"])
def test_resident_chain_equals_the_host_call(kind):
    z = ic.zps(32, 8)
    _, x = ic.span_patches(z, 300, seed=11)
    moments = z.transform(x).data
    held = _native.DeviceArray.from_numpy(moments)
    with clustering.DeviceRows.adopt(held.data_ptr(), *moments.shape, device=0) as rows:
        _, centres, _ = clustering.kmeans_fit(rows, 4, random_state=0)
    assert centres.shape == (4, len(z.n))
    if kind == "native":
        centres_dev = _native.DeviceArray.from_numpy(centres)
        host = lambda a: a.numpy()
    else:
        import torch
        centres_dev = torch.from_numpy(np.ascontiguousarray(centres)).cuda()
        host = lambda a: (torch.cuda.synchronize(), a.cpu().numpy())[1]
    for kw in ({}, {"m_select": (0, 3, 6)}, {"dtype": np.float32}, {"method": "direct"}):
        got = distributed.inverse_transform_device(z, centres_dev, **kw)
        assert tuple(got.shape) == (4, 32, 32)
        np.testing.assert_array_equal(host(got), z.inverse_transform(centres, **kw))
    first = distributed.inverse_transform_device(z, centres_dev, n_rows=2)
    np.testing.assert_array_equal(host(first), z.inverse_transform(centres[:2]))
    assert tuple(distributed.inverse_transform_device(z, centres_dev, n_rows=0).shape) == (0, 32, 32)
    with pytest.raises(ValueError, match="float64 matrix of real Zernike moments"):
        distributed.inverse_transform_device(z, centres_dev[:, :3].contiguous() if kind == "torch" else _native.DeviceArray((4, 3), np.float64))

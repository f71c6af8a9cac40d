"""The test infrastructure behind tests/test_device_inputs_gpu.py, without a GPU: the vectorised Philox restatement against the
scalar one (itself pinned by the published known-answer vectors, tests/test_noise.py) up to and beyond the stream positions
where the high counter word changes, and the sensitivity of the exact `amp` comparison: with `dist_in = 'uniform'` the two
roundings of `1 + v * zin` and a single rounding (one fused multiply-add) must differ often enough for the comparison to tell
them apart."""
import numpy as np
import pytest

from oracle import device_inputs_cases as dc
from oracle import philox_numpy as ph

E34 = 1 << 34


@pytest.mark.parametrize('seed,offset,n', [(0, 0, 17), (12345, 3, 1000), ((7 << 32) | 9, (1 << 34) + 1, 259), (1, 5, 1)])
def test_uniform_vec_on_the_cases_of_the_kernel_test(seed, offset, n):
    got = ph.uniform_vec(seed, offset, n)
    assert got.dtype == np.float32 and got.shape == (n,)
    np.testing.assert_array_equal(got, ph.uniform(seed, offset, n))


@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_uniform_vec_across_the_first_change_of_the_high_counter_word(shift):
    """Element 2^34 is word 0 of block 2^32: the range holds blocks 2^32 - 1 and 2^32 at every offset % 4."""
    offset = E34 - 8 + shift
    assert offset % 4 == shift and offset // 4 < (1 << 32) - 1 < (1 << 32) <= (offset + 22) // 4
    np.testing.assert_array_equal(ph.uniform_vec(dc.SEED, offset, 23), ph.uniform(dc.SEED, offset, 23))
    assert ph.uniform_vec(dc.SEED, offset, 0).shape == (0,)


def test_uniform_vec_beyond_three_times_2_to_the_34():
    np.testing.assert_array_equal(ph.uniform_vec(dc.SEED, 3 * E34 + 7, 41), ph.uniform(dc.SEED, 3 * E34 + 7, 41))
    # (and where the high word is no longer a small number: block 2^36 + ...)
    np.testing.assert_array_equal(ph.uniform_vec(3, (1 << 38) - 6, 13), ph.uniform(3, (1 << 38) - 6, 13))


def test_restatement_of_the_noise_outputs():
    """`device_inputs_noise` is the stream cut as the header says, zin exact, amp the two-rounding expression in float32."""
    v = np.linspace(0.05, 0.9, 6).astype(np.float32)
    z, zin, amp = ph.device_inputs_noise(dc.SEED, E34 - 30, E34 - 5, v, False, 2, 3)
    np.testing.assert_array_equal(z.reshape(-1), ph.uniform(dc.SEED, E34 - 30, 72))
    u = ph.uniform(dc.SEED, E34 - 5, 12).astype(np.float64).reshape(2, 6)
    np.testing.assert_array_equal(zin.astype(np.float64), 2 * u - 1)                    # 2 u - 1 is exact in float32
    prod = (v.astype(np.float64)[None, :] * zin.astype(np.float64)).astype(np.float32)  # rounded once ...
    np.testing.assert_array_equal(amp, (1.0 + prod.astype(np.float64)).astype(np.float32))   # ... and once more
    _, sgn, amp_b = ph.device_inputs_noise(dc.SEED, E34 - 30, E34 - 5, v, True, 2, 3)
    np.testing.assert_array_equal(sgn, np.where(u < 0.5, 1.0, -1.0))
    np.testing.assert_array_equal(amp_b, ph.amp_rounded_once(v, sgn))                   # v * (+-1) is exact: one rounding
    assert ph.device_inputs_noise(dc.SEED, 0, 0, None, False, 2, 3)[1:] == (None, None)
    got = dc.noise(dc.ROWS[0], 'uniform', E34 - 30, E34 - 5)
    for a, b in zip(got, (z, zin, amp)):
        np.testing.assert_array_equal(a, b)


def _share(v, zin, amp):
    return float((ph.amp_rounded_once(v, zin) != amp).mean())


@pytest.mark.parametrize('row', dc.ROWS, ids=dc.row_id)
def test_exact_amp_comparison_tells_one_rounding_from_two(row):
    """For every `uniform` case of the GPU test at least 5 % of the amp elements differ between the two-rounding form and the
    exact 1 + v z rounded once (13 - 25 % is typical); the bernoulli cases cannot differ (the product is exact)."""
    for off_z, off_zin in dc.offsets(row):
        zin, amp = ph.signs_and_amp(dc.SEED, off_zin, dc.v_of(row), False, row.B, 2 * row.N)
        assert _share(dc.v_of(row), zin, amp) >= 0.05, (row, off_zin)
        zin, amp = ph.signs_and_amp(dc.SEED, off_zin, dc.v_of(row), True, row.B, 2 * row.N)
        assert _share(dc.v_of(row), zin, amp) == 0.0


@pytest.mark.parametrize('ssn_type', ['heteroin', 'deg-heteroin'])
def test_exact_path_comparison_of_the_generator_tells_one_rounding_from_two(ssn_type):
    v = dc.gen_v_per_neuron(ssn_type)
    for pos in dc.GEN_POSITIONS:
        zin, amp = ph.signs_and_amp(dc.GEN_SEED, pos + dc.GEN_MODELS * (2 * dc.GEN_SITES) ** 2, v, False, dc.GEN_MODELS,
                                    2 * dc.GEN_SITES)
        assert _share(v, zin, amp) >= 0.05, (ssn_type, pos)

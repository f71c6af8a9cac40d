"""The odd register row of the split tile in column pairs, and the 7-row transpose-reduce without a zero row.

The heavy waves of the fp32 NB = 1 split kernels at C = 25 (7 rows per lane: two packed row pairs and one odd row in VGPRs,
two rows in LDS) sum the odd row's 25 products in two halves -- even columns, odd columns, column 24 into the even half,
then one add -- and reduce 7 rows without forming a zero row 7.  Rows 4, 11, 18, ... of every heavy wave are odd rows.

Common setup: fp32, one stimulus per draw (NB = 1), B = 5 draws, through `ssnode.fixed_points_batch` with variant 3 (split
tile), the library's own choice (None) and variant 4 (whole tile in VGPRs, plain column order), at

    N    2N   kernel                                    what it exercises
    100  200  mixed, 3 heavy waves + light wave         exact columns
    99   198  mixed                                     ragged last column group: a column pair with one half masked
    86   172  mixed                                     light wave with 4 real rows, heavy waves full
    77   154  uniform solve_tile_kernel<float,7,25,2>   3 heavy waves, the last one partly empty

Test 1 (order-independent bits): W has integer entries in [-3, 3] (none zero in the odd rows, all rows distinct), r0 integers
in [1, 7], ext integers.  Every product and every partial sum of W r0 + ext is an integer below 2^24, exact in fp32 in any
order of summation (checked here with numpy: sum_c |W[i][c]| r0[c] + |ext[i]| < 2^24), so after one step variant 3 and the
library's choice must equal variant 4 bit for bit, and lie within RTOL32 of the fp64 oracle; asym_tanh and asym_power.  The
inputs are checked not to be vacuous: u = W r0 + ext has both signs and values on both sides of the soft bound's voltage.
Test 2 (seven steps on `new_JDS` weights from a random r0): every element within RTOL32 of the fp64 oracle, variants 3 and 4
within RTOL32 of each other.
Test 3 (reduce): row i of W is (i + 1) x ones, r0 = ones, ext = 0, asym_power without a rate bound: u_i = (i + 1) 2N exactly,
the rate is strictly increasing in i (neighbours differ by more than 1 % >> RTOL32), so a lane that ended with another row's
sum, or with the value lane 7 is left with, misses the oracle at RTOL32.
"""
import numpy as np
import pytest

from oracle import ssn_numpy as on
from test_solver_gpu import RTOL32, _oracle_batch
from test_solver_stop_gpu import _same_bits

pytestmark = pytest.mark.gpu
P = on.DEFAULT_PARAMS

B = 5
SIZES = [100, 99, 86, 77]
VARIANTS = [3, None, 4]
VIDS = ['v3', 'auto', 'v4']
IO_TYPES = ['asym_tanh', 'asym_power']
KSTEPS = 7

_INT = {}
_REAL = {}
_RAMP = {}


def _solve(W, ext, r0, variant, io_type, max_iter):
    from tc_gan_amd import ssnode
    free = dict(rate_stop_at=np.inf)
    res = ssnode.fixed_points_batch(W, ext, P['k'], P['n'], r0=r0, max_iter=max_iter, atol=0.0, dtype='float32',
                                    variant=variant, io_type=io_type, **free)
    assert (np.asarray(res.codes) == 1).all() and (np.asarray(res.steps) == max_iter).all()
    return np.asarray(res.x)


def _oracle(oracle_lib, W, ext, r0, io_type, max_iter):
    # (`hard` is the rate at which asym_power stops and the upper bound of asym_tanh's saturation)
    free = dict(hard=np.inf) if io_type == 'asym_power' else {}
    return _oracle_batch(oracle_lib, W.astype(np.float64), ext.astype(np.float64), io_type, max_iter, 0.0,
                         r0=r0.astype(np.float64), **free)[0]


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=RTOL32, atol=RTOL32 * 1e-2, err_msg=what)


# ------------------------------------------------------------------ 1. order-independent bits
def _int_inputs(N):
    M = 2 * N
    rs = np.random.RandomState(2000 + N)
    W = rs.randint(-3, 4, size=(B, M, M)).astype(np.float32)
    odd = np.arange(M) % 7 == 4                      # the odd row of every 7-row lane tile
    fill = rs.choice(np.array([-3., -2., -1., 1., 2., 3.], dtype=np.float32), size=W[:, odd].shape)
    W[:, odd] = np.where(W[:, odd] == 0, fill, W[:, odd])
    r0 = rs.randint(1, 8, size=(B, 1, M)).astype(np.float32)
    ext = rs.randint(-40, 41, size=(1, M)).astype(np.float32)
    return W, ext, r0


def _int_case(oracle_lib, N, io_type):
    key = (N, io_type)
    if key not in _INT:
        W, ext, r0 = _int_inputs(N)
        _INT[key] = dict(W=W, ext=ext, r0=r0, want=_oracle(oracle_lib, W, ext, r0, io_type, 1),
                         got={v: _solve(W, ext, r0, v, io_type, 1) for v in VARIANTS})
    return _INT[key]


@pytest.mark.parametrize('N', SIZES)
def test_integer_inputs_are_exact_in_any_order_and_not_vacuous(N):
    W, ext, r0 = _int_inputs(N)
    M = 2 * N
    assert (W[:, np.arange(M) % 7 == 4] != 0).all()
    for b in range(B):
        assert len({row.tobytes() for row in W[b]}) == M, 'all rows distinct'
    bound = np.einsum('bij,bj->bi', np.abs(W).astype(np.float64), r0[:, 0].astype(np.float64)) + np.abs(ext)
    assert bound.max() < 2 ** 24
    u = np.einsum('bij,bj->bi', W.astype(np.float64), r0[:, 0].astype(np.float64)) + ext
    v0 = on.rate_to_volt(P['rate_soft_bound'], P['k'], P['n'])
    for rows in (slice(0, N), slice(N, M)):
        assert (u[:, rows] < 0).any() and ((u[:, rows] > 0) & (u[:, rows] < v0)).any() and (u[:, rows] > v0).any()
    rows4 = u[:, np.arange(M) % 7 == 4]
    assert (rows4 < 0).any() and ((rows4 > 0) & (rows4 < v0)).any() and (rows4 > v0).any()


@pytest.mark.parametrize('io_type', IO_TYPES)
@pytest.mark.parametrize('variant', [3, None], ids=['v3', 'auto'])
@pytest.mark.parametrize('N', SIZES)
def test_one_step_on_integers_equals_the_all_register_kernel_bit_for_bit(oracle_lib, N, variant, io_type):
    c = _int_case(oracle_lib, N, io_type)
    assert np.isfinite(c['got'][4]).all()
    _close(c['got'][4], c['want'], 'variant 4 against the fp64 oracle')
    _close(c['got'][variant], c['want'], 'against the fp64 oracle')
    _same_bits(c['got'][variant], c['got'][4], 'against variant 4 (plain column order)')


# ------------------------------------------------------------------ 2. seven steps on the real weights
def _real_case(oracle_lib, N):
    if N not in _REAL:
        jds = on.new_JDS()
        rs = np.random.RandomState(3000 + N)
        W = np.stack([on.generate_weight(N, jds['J'], jds['D'], jds['S'], z) for z in rs.rand(B, 2 * N, 2 * N)]).astype(np.float32)
        ext = (on.stimulus_input([1.0], np.linspace(-.5, .5, N), P['smoothness'], contrasts=[1.0]) * 20.0).astype(np.float32)
        r0 = (rs.rand(B, 1, 2 * N) * 20 + 0.05).astype(np.float32)
        _REAL[N] = dict(want=_oracle(oracle_lib, W, ext, r0, 'asym_tanh', KSTEPS),
                        got={v: _solve(W, ext, r0, v, 'asym_tanh', KSTEPS) for v in VARIANTS})
    return _REAL[N]


@pytest.mark.parametrize('variant', VARIANTS, ids=VIDS)
@pytest.mark.parametrize('N', SIZES)
def test_seven_steps_on_the_real_weights_match_the_fp64_oracle_in_every_row(oracle_lib, N, variant):
    c = _real_case(oracle_lib, N)
    assert np.isfinite(c['got'][variant]).all()
    _close(c['got'][variant], c['want'], 'against the fp64 oracle')
    _close(c['got'][variant], c['got'][4], 'against variant 4')
    _close(c['got'][4], c['got'][variant], 'variant 4 against this one')


# ------------------------------------------------------------------ 3. reduce
def _ramp_case(oracle_lib, N):
    if N not in _RAMP:
        M = 2 * N
        W = np.ascontiguousarray(np.broadcast_to((np.arange(M, dtype=np.float32) + 1)[None, :, None], (B, M, M)))
        ext = np.zeros((1, M), dtype=np.float32)
        r0 = np.ones((B, 1, M), dtype=np.float32)
        _RAMP[N] = dict(want=_oracle(oracle_lib, W, ext, r0, 'asym_power', 1),
                        got={v: _solve(W, ext, r0, v, 'asym_power', 1) for v in VARIANTS})
    return _RAMP[N]


@pytest.mark.parametrize('variant', VARIANTS, ids=VIDS)
@pytest.mark.parametrize('N', SIZES)
def test_every_finishing_lane_holds_its_own_row(oracle_lib, N, variant):
    c = _ramp_case(oracle_lib, N)
    want, got = c['want'], c['got'][variant]
    for rows in (slice(0, N), slice(N, 2 * N)):
        assert (np.diff(want[..., rows], axis=-1) > 50 * RTOL32 * want[..., rows][..., :-1]).all(), 'rows must be told apart'
    assert np.isfinite(got).all()
    _close(got, want, 'against the fp64 oracle')

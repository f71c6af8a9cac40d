"""The Wasserstein distances of the scorer (tc_gan_amd/analyzers/distdiff.py with wasserstein=True), the parts that need no GPU:
the exact restatement of the kernel's weighted sum (tests/wasserstein_cases.py) against known answers and against scipy, the
case KS cannot tell apart, the host logic (directions, refusals, wdist.csv, the arguments distdiff.json keeps) and the generated
code of csrc/ssn_wdist.hip (no spills, no scratch)."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_distdiff import CFG, THETA, ks_numerators
from wasserstein_cases import (block_sum_in_order, lattice, project_rows, w1_columns, w1_distance, w1_exact, wnum_bound,
                               wnum_in_kernel_order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')


# ---- 1. the restatement against known answers ----------------------------------------------------------------------------

def test_restatement_gives_the_known_answers():
    x = [0.0, 1.0, 3.0]
    assert w1_exact(x, [5.0, 6.0, 8.0]) == (45, 3, 3) and w1_distance(x, [5.0, 6.0, 8.0]) == 5
    assert w1_exact(x, x) == (0, 3, 3)
    assert w1_distance(x, [0.5, 1.5, 3.5]) == Fraction(1, 2)
    assert w1_distance([5.0, 6.0, 8.0], x) == 5                                   # symmetric
    # ties inside a sample and across the two: F_x - F_t = 2/3 - 1/4 on [1, 2), 2/3 - 3/4 on [2, 3), 1 - 3/4 on [3, 4)
    assert w1_exact([1.0, 1.0, 3.0], [1.0, 2.0, 2.0, 4.0]) == (5 + 1 + 3, 3, 4)
    assert w1_distance([1.0, 1.0, 3.0], [1.0, 2.0, 2.0, 4.0]) == Fraction(3, 4)
    # n != m: one point against two
    assert w1_exact([2.0], [0.0, 4.0]) == (4, 1, 2) and w1_distance([2.0], [0.0, 4.0]) == 2
    assert w1_distance([0.0] * 5, [3.0] * 2) == 3                                 # two point masses
    # non-finite values are left out; an empty side gives 0 and no distance
    assert w1_exact([np.nan, 0.0, np.inf, 1.0, -np.inf, 3.0], [5.0, np.nan, 6.0, 8.0]) == (45, 3, 3)
    assert w1_exact([np.nan], [1.0]) == (0, 0, 1) and w1_distance([np.nan], [1.0]) is None
    assert w1_exact([1.0], []) == (0, 1, 0)
    # the inputs are taken as float32
    assert w1_exact([0.1], [0.0])[0] == Fraction(float(np.float32(0.1)))


def test_restatement_equals_scipy_on_seeded_pairs():
    wasserstein_distance = pytest.importorskip('scipy.stats').wasserstein_distance
    rs = np.random.RandomState(17)
    worst = 0.0
    for i in range(200):
        n, m = int(rs.choice([1, 2, 5, 30, 128, 400])), int(rs.choice([1, 3, 32, 257, 1000]))
        if i % 3 == 0:
            x, t = rs.randn(n), rs.randn(m)
        elif i % 3 == 1:
            x, t = np.maximum(rs.randn(n), 0), np.maximum(rs.randn(m), 0)          # rectified: heavy ties at zero
        else:
            x, t = rs.randint(0, 8, n).astype(float), rs.randint(0, 8, m).astype(float)
        x, t = x.astype('float32'), t.astype('float32')
        worst = max(worst, abs(float(w1_distance(x, t)) - wasserstein_distance(x.astype('float64'), t.astype('float64'))))
    print('largest difference to scipy:', worst)
    assert worst <= 1e-12


def test_w1_tells_apart_what_ks_cannot():
    """Two generated columns on one side of the truth: the same KS numerator (KSD = 1), W1 apart by the shift."""
    rs = np.random.RandomState(3)
    t = lattice(rs, (50, 1))
    near = lattice(rs, (30, 1)) + 64 + 5
    far = near + 5
    x = np.concatenate([near, far], axis=1)
    num, n, m = ks_numerators(x, np.repeat(t, 2, axis=1))
    assert list(num) == [30 * 50] * 2 and list(n) == [30] * 2 and list(m) == [50] * 2
    w_near, w_far = w1_distance(near, t), w1_distance(far, t)
    assert w_far - w_near == 5
    # (all of x above all of t: W1 is the difference of the means; the sums of multiples of 1/8 are exact in fp64)
    assert w_near == Fraction(float(near.astype('float64').sum())) / 30 - Fraction(float(t.astype('float64').sum())) / 50


def test_block_sum_in_order_adds_in_the_stated_order():
    """Powers of two that differ by more than 53 bits show who is added to whom: 1 + 2^-53 rounds back to 1 (ties to even), so a
    small term survives only where it meets another small term first."""
    tiny = 2.0 ** -53
    assert block_sum_in_order([]) == 0 and block_sum_in_order([3.0]) == 3
    assert block_sum_in_order(np.ones(1000)) == 1000
    one_thread = np.zeros(513)
    one_thread[[0, 256, 512]] = [1, tiny, tiny]                                   # thread 0: (1 + tiny) + tiny
    assert block_sum_in_order(one_thread) == 1
    one_thread[[0, 256, 512]] = [tiny, tiny, 1]                                   # (tiny + tiny) + 1
    assert block_sum_in_order(one_thread) == 1 + 2 * tiny
    lanes = np.zeros(64)
    lanes[[0, 32, 33]] = [1, tiny, tiny]                                          # off = 32 first: lane 0 takes lane 32 alone
    assert block_sum_in_order(lanes) == 1
    lanes[[0, 32, 33]] = [0, 0, 0]
    lanes[[0, 1, 33]] = [1, tiny, tiny]                                           # off = 32 joins lanes 1 and 33 before off = 1
    assert block_sum_in_order(lanes) == 1 + 2 * tiny
    lanes[[0, 1, 33]] = [0, 0, 0]
    lanes[[0, 1, 3]] = [1, tiny, tiny]                                            # off = 2 joins lanes 1 and 3 before off = 1
    assert block_sum_in_order(lanes) == 1 + 2 * tiny
    waves = np.zeros(256)
    waves[[0, 64, 128]] = [1, tiny, tiny]                                         # (wave 0 + wave 1) + wave 2
    assert block_sum_in_order(waves) == 1
    waves[[0, 64, 128]] = [tiny, tiny, 1]
    assert block_sum_in_order(waves) == 1 + 2 * tiny


@pytest.mark.parametrize('B,T', [(1, 1), (64, 7), (65, 50), (257, 50), (300, 7), (300, 700)])
def test_wnum_in_kernel_order_is_exact_on_a_lattice_and_within_the_bound_elsewhere(B, T):
    rs = np.random.RandomState(B + T)
    x, t = lattice(rs, (B,)), lattice(rs, (T,))
    if B >= 4:
        x[[0, B // 2, B - 1]] = [np.nan, np.inf, -np.inf]
    exact, n, m = w1_exact(x, t)
    assert n == (B - 3 if B >= 4 else B) and Fraction(float(wnum_in_kernel_order(x, t))) == exact
    assert wnum_in_kernel_order(t, t) == 0 and wnum_in_kernel_order(x, [np.nan]) == 0 and wnum_in_kernel_order([np.nan], t) == 0
    worst = Fraction(0)
    for _ in range(5):
        x, t = (rs.rand(B) * 40).astype('float32'), (rs.rand(T) * 40).astype('float32')
        x[rs.randint(B)] = t[rs.randint(T)]                                       # a value both hold
        exact, n, m = w1_exact(x, t)
        err, bound = abs(Fraction(float(wnum_in_kernel_order(x, t))) - exact), wnum_bound(exact, n, m)
        assert err <= bound
        worst = max(worst, err / bound if bound else 0)
    print('largest error of the restatement: {:.3g} of the bound'.format(float(worst)))


def test_projection_restatement_is_the_sequential_sum():
    rs = np.random.RandomState(5)
    x, theta = rs.randn(4, 9).astype('float32'), rs.randn(3, 9).astype('float32')
    want = np.empty((4, 3), dtype='float32')
    for r in range(4):
        for l in range(3):
            acc = Fraction(0)
            for c in range(9):
                acc = Fraction(float(acc + Fraction(float(x[r, c])) * Fraction(float(theta[l, c]))))   # one rounding: an fma
            want[r, l] = np.float32(float(acc))
    np.testing.assert_array_equal(project_rows(x, theta), want)


# ---- 2. host logic -------------------------------------------------------------------------------------------------------

def test_direction_table():
    from tc_gan_amd import clib
    from tc_gan_amd.analyzers.distdiff import slice_directions
    th = slice_directions(128, 80, 0)
    assert th.shape == (128, 80) and th.dtype == np.float32 and th.flags['C_CONTIGUOUS']
    g = np.random.RandomState(0).randn(128, 80)
    np.testing.assert_array_equal(th, (g / np.sqrt((g * g).sum(axis=1))[:, None]).astype('float32'))
    norms = np.sqrt((th.astype('float64') ** 2).sum(axis=1))
    assert np.abs(norms - 1).max() <= 80 * 2.0 ** -24                             # unit rows up to the rounding to float32
    np.testing.assert_array_equal(th, slice_directions(128, 80, 0))
    assert not np.array_equal(th, slice_directions(128, 80, 1))
    np.testing.assert_array_equal(np.abs(slice_directions(3, 1, 9)), 1)           # one column: the directions are +-1
    assert slice_directions(clib.W1_MAX_DIRECTIONS, 2).shape == (clib.W1_MAX_DIRECTIONS, 2)
    header = open(os.path.join(ROOT, 'include', 'ssnode_mi355x.h')).read()
    assert int(re.search(r'#define SSN_W1_MAX_DIRECTIONS (\d+)', header).group(1)) == clib.W1_MAX_DIRECTIONS


def test_direction_refusals_need_no_device():
    from tc_gan_amd import clib
    from tc_gan_amd.analyzers.distdiff import score_parameter_sets, slice_directions
    for bad in (0, -3, clib.W1_MAX_DIRECTIONS + 1):
        with pytest.raises(ValueError, match='directions'):
            slice_directions(bad, 16)
        for dynamics in ('fixed-time', 'fixed-point'):
            with pytest.raises(ValueError, match='directions'):
                score_parameter_sets(CFG, [THETA], np.zeros((8, 16)), draws=4, wasserstein=True, directions=bad, dynamics=dynamics)


def test_new_symbols_are_declared():
    from tc_gan_amd import clib
    for name in ('ssn_ks_w1_columns_f32', 'ssn_project_rows_f32'):
        assert name in clib.DECLARED_SYMBOLS and getattr(clib.libssnode, name).argtypes is not None
    assert 'ssn_wdist.hip' in open(os.path.join(CSRC, 'Makefile')).read()
    assert clib.libssnode.ssn_abi_version() == 1


def test_c_entry_points_refuse_from_the_arguments_alone():
    """Host checks in front of any HIP call: no device needed."""
    from tc_gan_amd import clib
    lib = clib.libssnode
    invalid = clib.SSN_ERR_BASE + 1                  # hipErrorInvalidValue
    assert lib.ssn_ks_w1_columns_f32(None, None, None, 1, 16385, 1, 1, None, None, None, None) == invalid
    assert '16384' in clib.last_error()
    assert lib.ssn_ks_w1_columns_f32(None, None, None, 1, 4, 1, 1, None, None, None, None) == invalid
    assert lib.ssn_ks_w1_columns_f32(None, None, None, -1, 4, 1, 1, None, None, None, None) == invalid
    assert lib.ssn_project_rows_f32(None, 4, 3, 3, None, clib.W1_MAX_DIRECTIONS + 1, None, None) == invalid
    assert '4096' in clib.last_error()
    assert lib.ssn_project_rows_f32(None, 4, 2, 3, None, 5, None, None) == invalid          # ldx < C
    assert lib.ssn_project_rows_f32(None, 4, 3, 3, None, 5, None, None) == invalid          # null pointers
    assert lib.ssn_project_rows_f32(None, -1, 3, 3, None, 5, None, None) == invalid
    # empty problems succeed
    assert lib.ssn_ks_w1_columns_f32(None, None, None, 0, 4, 7, 1, None, None, None, None) == 0
    assert lib.ssn_ks_w1_columns_f32(None, None, None, 3, 4, 0, 1, None, None, None, None) == 0
    assert lib.ssn_project_rows_f32(None, 0, 3, 3, None, 5, None, None) == 0
    assert lib.ssn_project_rows_f32(None, 4, 3, 3, None, 0, None, None) == 0


def _result():
    from tc_gan_amd.analyzers.distdiff import ksd_from_counts, w1_from_sums
    num = np.array([[0, 3, 0], [6, 1, 0]], dtype=np.int64)
    n = np.array([[2, 3, 0], [2, 3, 3]], dtype=np.int64)
    m = np.array([3, 2, 0], dtype=np.int64)
    wnum = np.array([[0.0, 0.1 * 6, 0.0], [7.5, 1.0 / 3.0, 0.0]])
    return dict(gen_step=np.array([10, 20]), stat=['a', 'b', 'c'], num=num, n=n, m=m, KSD=ksd_from_counts(num, n, m[None, :]),
                wnum=wnum, W1=w1_from_sums(wnum, n, m[None, :]), SW1=np.array([1.0 / 7.0, np.nan]),
                sliced=dict(directions=4, seed=0, n=np.array([3, 0]), m=5))


def test_w1_from_sums_and_the_long_table_round_trip(tmp_path):
    import pandas
    from tc_gan_amd.analyzers.distdiff import SLICED_STAT, wdist_table, write_long_table, write_wdist_table
    result = _result()
    np.testing.assert_array_equal(result['W1'], [[0.0, 0.1 * 6 / 6, np.nan], [7.5 / 6, 1.0 / 3.0 / 6, np.nan]])
    path = tmp_path / 'wdist.csv'
    write_wdist_table(str(path), result)
    back = pandas.read_csv(str(path), float_precision='round_trip')
    assert list(back.columns) == ['gen_step', 'stat', 'W1', 'n', 'm'] and len(back) == 2 * 4
    assert list(back['gen_step']) == [10] * 4 + [20] * 4 and list(back['stat']) == ['a', 'b', 'c', SLICED_STAT] * 2
    np.testing.assert_array_equal(back['W1'].to_numpy(), np.concatenate([result['W1'][0], [1.0 / 7.0], result['W1'][1], [np.nan]]))
    np.testing.assert_array_equal(back['n'].to_numpy(), [2, 3, 0, 3, 2, 3, 3, 0])
    np.testing.assert_array_equal(back['m'].to_numpy(), [3, 2, 0, 5] * 2)
    pandas.testing.assert_frame_equal(back, wdist_table(result).astype({'stat': back['stat'].dtype}), check_dtype=False)
    # the KS table does not change with the new keys in the result
    plain = {k: v for k, v in result.items() if k not in ('wnum', 'W1', 'SW1', 'sliced')}
    write_long_table(str(tmp_path / 'a.csv'), result)
    write_long_table(str(tmp_path / 'b.csv'), plain)
    assert (tmp_path / 'a.csv').read_bytes() == (tmp_path / 'b.csv').read_bytes()


def test_distdiff_json_arguments_do_not_change_with_the_new_options():
    from tc_gan_amd.analyzers.distdiff import make_parser, recorded_arguments
    new = ['--wasserstein', '--directions', '16', '--direction-seed', '3']
    ns = make_parser().parse_args(['somewhere'])
    assert ns.wasserstein is False and ns.directions == 128 and ns.direction_seed == 0
    for base in (['somewhere', '--draws', '8'], ['somewhere', '--dynamics', 'fixed-point', '--max-candidates', '12']):
        plain, on = make_parser().parse_args(base), make_parser().parse_args(base + new)
        assert on.wasserstein and on.directions == 16 and on.direction_seed == 3
        assert recorded_arguments(on) == recorded_arguments(plain)
        assert not {'wasserstein', 'directions', 'direction_seed'} & set(recorded_arguments(on))
    assert sorted(recorded_arguments(make_parser().parse_args(['somewhere'] + new))) == [
        'draws', 'gen_kernel', 'max_draws_per_launch', 'output', 'rundir', 'save_tuning_curves', 'seed', 'steps']
    assert sorted(recorded_arguments(make_parser().parse_args(['somewhere', '--dynamics', 'fixed-point'] + new))) == [
        'draws', 'dynamics', 'gen_kernel', 'max_candidates', 'max_draws_per_launch', 'output', 'rundir', 'save_tuning_curves', 'seed',
        'solver_dtype', 'steps']


def test_module_docstring_names_the_option():
    from tc_gan_amd.analyzers import distdiff
    assert '--wasserstein' in distdiff.__doc__ and 'wdist.csv' in distdiff.__doc__


# ---- 3. the generated code of csrc/ssn_wdist.hip -------------------------------------------------------------------------

def test_no_kernel_of_the_wasserstein_file_spills_or_uses_scratch(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_wdist.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_wdist.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)', text, re.S)
    names = sorted(n for n, _, _ in found)
    assert len(names) == 2 and any('ks_w1_columns_kernel' in n for n in names) and any('project_rows_kernel' in n for n in names)
    assert all(int(p) == 0 and int(s) == 0 for _, p, s in found), found

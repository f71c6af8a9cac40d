"""The sliced Wasserstein match of two samples of different sizes (csrc/ssn_swd_sizes.hip in libssnode_ext.so,
networks/sliced_wasserstein.py with swd_truth_batch), the parts that need no GPU: the restatement the GPU tests compare with
(tests/swd_sizes_cases.py) against scipy, against the equal-size restatement on replicated rows, against fp64 autograd, on a
lattice and at equal sizes; how far three deliberate errors move what is checked; the companion library's exports and refusals
and the frozen surface of libssnode.so; the generated code of the new kernel; the trainer's option and the command lines."""
import os
import re
import shutil
import subprocess
from fractions import Fraction
from math import gcd

import numpy as np
import pytest
import torch

import swd_cases as sc
import swd_sizes_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')

#: from one value each to the default run's 15 draws against its truth; coprime, common factor, n > m, n == m
SIZE_PAIRS = [(1, 1), (1, 7), (7, 1), (2, 3), (4, 6), (6, 4), (5, 5), (12, 18), (9, 64), (64, 9), (15, 1000)]


def _replicated(a, times):
    return np.repeat(a, times, axis=0)


# ---- 1. the restatement against other statements of the same distance ------------------------------------------------------

def test_restatement_equals_scipy_per_direction():
    wasserstein_distance = pytest.importorskip('scipy.stats').wasserstein_distance
    rs = np.random.RandomState(1)
    worst = 0.0
    for n, m in SIZE_PAIRS:
        x, y, theta = zc.generic_inputs(rs, n, m, 5, 3)
        got = zc.swd(x, y, theta, 1)
        for l in range(5):
            ref = wasserstein_distance(got['px'][:, l].astype('float64'), got['py'][:, l].astype('float64'))
            worst = max(worst, abs(float(got['loss_l'][l]) - ref))
    print('largest difference to scipy:', worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('power', [1, 2])
def test_restatement_equals_the_equal_size_match_on_replicated_rows(power):
    """Every x row m / g times and every y row n / g times (g = gcd) are two samples of n m / g rows with the same empirical
    measures: the rank matching of `swd_cases.match` on them is this coupling.  Equal as rationals."""
    rs = np.random.RandomState(2)
    for n, m in SIZE_PAIRS:
        x, y, theta = zc.generic_inputs(rs, n, m, 4, 3)
        got = zc.swd(x, y, theta, power)
        g = gcd(n, m)
        _, want = sc.match(_replicated(got['px'], m // g), _replicated(got['py'], n // g), power)
        assert got['loss_l'] == want, (n, m)


@pytest.mark.parametrize('power', [1, 2])
def test_restatement_equals_fp64_autograd_through_sort(power):
    """The restatement rounds the projections, the coefficients and the gradient to float32 (2^-24 = 6e-8 relative each) where
    autograd stays in fp64: loss within 1e-6 relative, gradient within 1e-6 of its largest entry.  Generic rows without ties."""
    rs = np.random.RandomState(3)
    worst = 0.0
    for n, m in ((7, 1), (2, 3), (12, 18), (15, 1000), (64, 9)):
        D, L = 5, 8
        x, y = rs.randn(n, D).astype('float32'), (rs.randn(m, D) + 0.5).astype('float32')
        theta = sc.generic_inputs(rs, 2, L, D)[2]
        theta[L // 2] = theta[0][::-1]                            # (no tied direction here)
        got = zc.swd(x, y, theta, power)
        g = gcd(n, m)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        tt = torch.tensor(theta, dtype=torch.float64)
        px, py = xt @ tt.T, torch.tensor(y, dtype=torch.float64) @ tt.T
        d = torch.sort(px, dim=0).values.repeat_interleave(m // g, dim=0) - torch.sort(py, dim=0).values.repeat_interleave(n // g, dim=0)
        loss = (d.abs() if power == 1 else d * d).mean()
        grad, = torch.autograd.grad(loss, xt)
        np.testing.assert_allclose(got['loss'], float(loss.detach()), rtol=1e-6)
        top = np.abs(grad.numpy()).max()
        worst = max(worst, np.abs(got['gx'] - grad.numpy()).max() / top)
        np.testing.assert_allclose(got['gx'], grad.numpy(), rtol=0, atol=1e-6 * top)
    print('largest gradient difference / largest entry:', worst)


@pytest.mark.parametrize('power', [1, 2])
def test_lattice_values_are_exact(power):
    """Every operation of the kernel order is exact on the lattice: its loss is the rational one, and the coefficients are the
    exact sums times the exact inv."""
    for n, m, L in ((1, 1, 1), (2, 8, 2), (64, 16, 4), (256, 1024, 2)):
        x, y, theta = zc.lattice_inputs(np.random.RandomState(10 + n), n, m, L, 6)
        got = zc.swd(x, y, theta, power)
        ordered = [zc.loss_in_kernel_order(got['px'][:, l], got['py'][:, l], power) for l in range(L)]
        assert [Fraction(float(v)) for v in ordered] == got['loss_l']
        i, j, w, _, _ = zc.coupling(n, m)
        for l in range(L):
            order = np.argsort(got['px'][:, l] + np.float32(0), kind='stable')
            d = got['px'][order, l].astype('float64')[i] - np.sort(got['py'][:, l]).astype('float64')[j]
            for rank in (0, n // 2, n - 1):
                sel = i == rank
                c = sum(int(wk) * Fraction(float(np.sign(dk) if power == 1 else 2.0 * dk)) for wk, dk in zip(w[sel], d[sel]))
                assert Fraction(float(got['coef'][order[rank], l])) == c / (L * n * m)


@pytest.mark.parametrize('power', [1, 2])
def test_equal_power_of_two_sizes_give_the_bits_of_the_equal_size_restatement(power):
    """n == m: every weight is n, a power of two, so the weighted terms, their sums and the division by n n are those of the
    rank matching scaled exactly."""
    for n, L in ((1, 1), (2, 2), (64, 4), (512, 2)):
        x, y, theta = sc.generic_inputs(np.random.RandomState(20 + n), n, L, 6)
        got, want = zc.swd(x, y, theta, power), sc.swd(x, y, theta, power)
        assert got['loss_l'] == want['loss_l']
        np.testing.assert_array_equal(got['coef'].view(np.uint32), want['coef'].view(np.uint32))
        for l in range(L):
            a = zc.loss_in_kernel_order(got['px'][:, l], got['py'][:, l], power)
            b = sc.loss_in_kernel_order(got['px'][:, l], got['py'][:, l], power)
            assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


@pytest.mark.parametrize('power', [1, 2])
def test_kernel_order_stays_within_the_bound_and_non_finite_columns_are_nan(power):
    worst = Fraction(0)
    for n, m in ((2, 3), (65, 64), (15, 1000), (300, 257), (1000, 1024)):
        x, y, theta = zc.generic_inputs(np.random.RandomState(100 + n), n, m, 3, 6)
        want = zc.swd(x, y, theta, power)
        for l in range(3):
            exact = want['loss_l'][l]
            err = abs(Fraction(float(zc.loss_in_kernel_order(want['px'][:, l], want['py'][:, l], power))) - exact)
            assert err <= zc.loss_bound(exact, n, m), (n, m, l)
            if exact:
                worst = max(worst, err / zc.loss_bound(exact, n, m))
    print('largest error of the kernel order: {:.3g} of the bound'.format(float(worst)))
    assert worst > 0                                              # (generic values do round: the order is exercised)
    px, py = np.ones((3, 2), dtype='float32'), np.zeros((5, 2), dtype='float32')
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            p = [px.copy(), py.copy()]
            p[side][1, 1] = bad
            coef, loss = zc.match(p[0], p[1], power)
            assert loss[1] is None and np.isnan(coef[:, 1]).all() and loss[0] == 1 and np.isfinite(coef[:, 0]).all()
            assert np.isnan(zc.loss_in_kernel_order(p[0][:, 1], p[1][:, 1], power))


# ---- 2. sensitivity: what a wrong restatement would move -----------------------------------------------------------------

def test_deliberate_errors_move_the_checked_quantities_far_beyond_their_tolerances():
    """The GPU tests hold coef to equality of bits (the least difference is one float32 ulp, 2^-23 relative) and loss_l to
    `loss_bound`.  Each error must move one of them by at least 1e6 ulps of coef's largest entry or 1e6 bounds."""
    rs = np.random.RandomState(4)
    n, m, L, D = 65, 64, 33, 6
    x, y, theta = zc.generic_inputs(rs, n, m, L, D)
    right = zc.swd(x, y, theta, 2)
    ulp = 2.0 ** -23
    top = np.abs(right['coef']).max()

    def loss_factor(wrong):
        return min(float(abs(a - b) / zc.loss_bound(a, n, m)) for a, b in zip(right['loss_l'], wrong['loss_l']) if a != 0)

    short = zc.swd(x, y, theta, 2, j_hi_short=True)
    moved = np.abs(short['coef'] - right['coef']).max() / top
    print('j_hi one short: loss_l moves by at least', loss_factor(short), 'bounds, coef by', moved / ulp, 'ulps')
    assert loss_factor(short) >= 1e6 and moved / ulp >= 1e6

    unit = zc.swd(x, y, theta, 2, unit_weights=True)
    moved = np.abs(unit['coef'] - right['coef']).max() / top
    print('weights all 1: loss_l moves by at least', loss_factor(unit), 'bounds, coef by', moved / ulp, 'ulps')
    assert loss_factor(unit) >= 1e6 and moved / ulp >= 1e6

    ranked = zc.swd(x, y, theta, 2, scatter='rank')
    moved = np.abs(ranked['coef'] - right['coef']).max() / top
    assert ranked['loss_l'] == right['loss_l']                    # (the loss cannot see the scatter: the coefficients do)
    print('scattered by rank: coef moves by', moved / ulp, 'ulps')
    assert moved / ulp >= 1e6
    assert np.abs(ranked['gx'] - right['gx']).max() / np.abs(right['gx']).max() / ulp >= 1e6


# ---- 3. the two libraries ---------------------------------------------------------------------------------------------------

def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    return sorted(set(re.findall(r'^\s*(?:int|long|size_t|double|const char \*|const char\*)\s*\*?\s*([a-z_0-9]+)\s*\(', text,
                                 flags=re.M)))


def _exported(library):
    out = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(ROOT, 'tc_gan_amd', 'ext', library)]).decode()
    return sorted(line.split()[-1].split('@')[0] for line in out.splitlines() if line.strip())


def test_companion_library_exports_its_header_and_nothing_else():
    from tc_gan_amd import clib
    names = _declared('ssnode_mi355x_ext.h')
    assert names == ['ssnx_abi_version', 'ssnx_last_error', 'ssnx_swd_match_sizes_f32']
    assert sorted(clib.EXT_DECLARED_SYMBOLS) == names == _exported('libssnode_ext.so')
    assert all(n.startswith('ssnx_') for n in names)
    assert clib.libssnode_ext.ssnx_abi_version() == 1
    assert len(clib.libssnode_ext.ssnx_swd_match_sizes_f32.argtypes) == 9
    header = open(os.path.join(ROOT, 'include', 'ssnode_mi355x_ext.h')).read()
    assert int(re.search(r'#define SSNX_SWD_MAX_TRUTH (\d+)', header).group(1)) == clib.SWD_MAX_TRUTH == clib.KS_MAX_DRAWS
    assert header.lstrip().startswith('/*') and 'after the surface of libssnode.so was pinned' in header.split('*/')[0]
    assert 'libssnode_ext.map' in open(os.path.join(ROOT, '.gitignore')).read()


def test_the_main_library_exports_its_header_as_before():
    from tc_gan_amd import clib
    names = _declared('ssnode_mi355x.h')
    assert _exported('libssnode.so') == names == sorted(clib.DECLARED_SYMBOLS)
    assert not [n for n in names if n.startswith('ssnx_')] and len(names) == 132
    assert not set(clib.EXT_DECLARED_SYMBOLS) & set(clib.DECLARED_SYMBOLS)


#: (n, m, L, power) with null pointers -> what ssnx_last_error says behind "ssnx_swd_match_sizes_f32: "
REFUSALS = [
    ((4097, 8, 3, 2), 'more than 4096 generated rows (their keys are sorted in 32 KiB of LDS)'),
    ((8, 16385, 3, 2), 'more than 16384 truth rows (their values are sorted in 64 KiB of LDS)'),
    ((8, 8, 4097, 2), 'more than 4096 directions'),
    ((-1, 8, 3, 2), 'a negative size'),
    ((8, -1, 3, 2), 'a negative size'),
    ((8, 8, -3, 2), 'a negative size'),
    ((8, 8, 3, 0), 'a power other than 1 or 2'),
    ((8, 8, 3, 3), 'a power other than 1 or 2'),
    ((0, 0, 0, -1), 'a power other than 1 or 2'),
    ((8, 0, 3, 2), 'no truth rows (m == 0) to match the generated rows with'),
    ((8, 9, 3, 2), 'invalid argument (null pointer)'),
    ((1, 1, 1, 1), 'invalid argument (null pointer)'),
]


@pytest.mark.parametrize('sizes, message', REFUSALS)
def test_the_match_refuses_from_the_arguments_alone(sizes, message):
    """Host checks in front of any HIP call: no device needed.  The message is the companion library's own."""
    from tc_gan_amd import clib
    n, m, L, power = sizes
    before = clib.last_error()
    rc = clib.libssnode_ext.ssnx_swd_match_sizes_f32(None, n, None, m, L, power, None, None, None)
    assert rc == clib.SSN_ERR_BASE + 1                                # hipErrorInvalidValue
    assert clib.ext_last_error() == 'ssnx_swd_match_sizes_f32: ' + message
    assert clib.last_error() == before                                # (the main library's string is not touched)
    with pytest.raises(clib.SSNLibraryError, match=re.escape(message)):
        clib.check_ext(rc, 'ssnx_swd_match_sizes_f32')


def test_empty_problems_succeed_and_write_nothing():
    from tc_gan_amd import clib
    for power in (1, 2):
        for n, m, L in ((0, 5, 3), (5, 7, 0), (0, 0, 0), (0, 0, 3), (5, 0, 0)):
            assert clib.libssnode_ext.ssnx_swd_match_sizes_f32(None, n, None, m, L, power, None, None, None) == 0
    clib.check_ext(0, 'nothing')


def _makefile_flags(stem):
    """What csrc/Makefile compiles `stem`.hip with: its CXXFLAGS (with ARCH expanded) and FLAGS_<stem> where it sets one."""
    makefile = open(os.path.join(CSRC, 'Makefile')).read()

    def value(name):
        found = re.search(r'^%s[ \t]*[?:]?=[ \t]*(.*)$' % re.escape(name), makefile, re.M)
        return found.group(1).strip() if found else ''
    flags = (value('CXXFLAGS') + ' ' + value('FLAGS_' + stem) + ' ' + value('EXTRA')).replace('$(ARCH)', value('ARCH'))
    assert '$(' not in flags, flags
    return flags.split()


def test_new_kernel_is_wave64_without_spills_or_scratch(tmp_path):
    """Metadata only, with the Makefile's flags.  Static LDS as designed: the four doubles of the ordered block sum and the
    flag of a non-finite column, 40 bytes, beside the dynamic 8 P(n) + 4 P(m) <= 96 KiB the launch asks for."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_swd_sizes.s'
    flags = _makefile_flags('ssn_swd_sizes')
    assert '-O3' in flags and '--offload-arch=gfx950' in flags and '-fPIC' in flags
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_swd_sizes.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)'
                       r'.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+).*?\.wavefront_size:\s+(\d+)', text, re.S)
    assert len(found) == 1 and 'swd_match_sizes_kernel' in found[0][1], found
    assert [int(v) for k, v in enumerate(found[0]) if k != 1] == [40, 0, 0, 0, 64], found
    source = open(os.path.join(CSRC, 'ssn_swd_sizes.hip')).read() + open(os.path.join(CSRC, 'ssn_swd_sizes_dev.h')).read()
    assert 'asm' not in source and 'atomicAdd' not in source
    makefile = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'ssn_swd_sizes.hip' in makefile and 'ssn_ext_capi.hip' in makefile
    assert 'ssn_swd_sizes' not in re.search(r'^SRCS\s+:=(.*)$', makefile, re.M).group(1)      # not linked into libssnode.so
    # the companion library's headers are its own: no object of libssnode.so depends on them
    assert re.search(r'^HDRS\s+:=\s*\$\(filter-out \$\(EXT_HDRS\)', makefile, re.M)
    ext_hdrs = re.search(r'^EXT_HDRS\s+:=(.*)$', makefile, re.M).group(1).split()
    assert {'ssn_ext_host.h', 'ssn_swd_sizes_dev.h'} <= set(ext_hdrs)
    for name in os.listdir(CSRC):
        if name.endswith(('.hip', '.h')) and name not in ('ssn_ext_capi.hip', 'ssn_swd_sizes.hip', 'ssn_swd_sizes_dev.h'):
            text = open(os.path.join(CSRC, name)).read()
            assert 'ssn_ext_host.h' not in text and 'ssn_swd_sizes_dev.h' not in text and 'mi355x_ext.h' not in text, name
            assert name == 'ssn_ext_host.h' or 'launch_swd_match_sizes' not in text, name


# ---- 4. the trainer's option and the command lines ---------------------------------------------------------------------

def test_defaults():
    from tc_gan_amd import clib
    from tc_gan_amd.networks.sliced_wasserstein import DEFAULT_PARAMS, BPTTSlicedWasserstein
    assert DEFAULT_PARAMS['swd_truth_batch'] == 0 and BPTTSlicedWasserstein.swd_truth_batch == 0
    assert clib.SWD_MAX_TRUTH == 16384 and clib.SWD_MAX_BATCH == 4096


def test_the_three_meanings_of_swd_truth_batch():
    from tc_gan_amd.networks.sliced_wasserstein import truth_minibatch_rows
    from tc_gan_amd.utils import random_minibatches
    # 0: the stream of a run without the option
    got = truth_minibatch_rows(0, 5, 20, seed=np.random.RandomState(3))
    want = random_minibatches(5, np.arange(20), seed=np.random.RandomState(3))
    for _ in range(9):
        np.testing.assert_array_equal(next(got), next(want))
    # M: minibatches of M rows on the same kind of stream
    got = truth_minibatch_rows(10, 5, 20, seed=np.random.RandomState(3))
    want = random_minibatches(10, np.arange(20), seed=np.random.RandomState(3))
    for _ in range(5):
        rows = next(got)
        assert rows.shape == (10,)
        np.testing.assert_array_equal(rows, next(want))
    # -1: the whole truth, no shuffle drawn, batchsize may exceed the truth
    rng = np.random.RandomState(3)
    state = rng.get_state()[1].copy()
    assert truth_minibatch_rows(-1, 1024, 300, seed=rng) is None
    np.testing.assert_array_equal(rng.get_state()[1], state)
    with pytest.raises(ValueError, match='batchsize = 1024 > len'):
        truth_minibatch_rows(0, 1024, 300, seed=rng)


def test_refusals_by_name():
    """The factory refuses a bad value before it builds the generator (no device needed); the whole truth is refused where it has
    more rows than the match takes."""
    from tc_gan_amd import clib
    from tc_gan_amd.networks.sliced_wasserstein import checked_truth_batch, make_sliced_wasserstein, truth_minibatch_rows
    for bad in (clib.SWD_MAX_TRUTH + 1, -2, 2.5, True):
        with pytest.raises(ValueError, match='swd_truth_batch = '):
            checked_truth_batch(bad)
        with pytest.raises(ValueError, match='swd_truth_batch = '):
            make_sliced_wasserstein(dict(swd_truth_batch=bad))
    assert [checked_truth_batch(v) for v in (-1, 0, 1, 256.0, clib.SWD_MAX_TRUTH)] == [-1, 0, 1, 256, clib.SWD_MAX_TRUTH]
    with pytest.raises(ValueError, match=r'swd_truth_batch = -1: the truth has 16385 rows'):
        truth_minibatch_rows(-1, 15, clib.SWD_MAX_TRUTH + 1)
    with pytest.raises(ValueError, match=r'swd_truth_batch = -1: the truth has 0 rows'):
        truth_minibatch_rows(-1, 15, 0)
    with pytest.raises(ValueError, match=r'swd_truth_batch = 301 > truth rows = 300'):      # (not random_minibatches' 'batchsize')
        truth_minibatch_rows(301, 15, 300)
    assert next(truth_minibatch_rows(300, 1024, 300, seed=0)).shape == (300,)


def test_swd_loss_grad_asks_for_unequal_sizes_by_name():
    """Without `unequal=True` a y of another row count is the shape error it was; the check comes before any launch."""
    from tc_gan_amd.networks.sliced_wasserstein import swd_loss_grad
    x, y, theta = torch.zeros(4, 3), torch.zeros(5, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError, match='unequal=True'):
        swd_loss_grad(x, y, theta, 2)
    with pytest.raises(ValueError, match='contiguous'):
        swd_loss_grad(x, torch.zeros(5, 4), theta, 2, unequal=True)
    with pytest.raises(ValueError, match='truth rows'):
        swd_loss_grad(x, torch.zeros(0, 3), theta, 2, unequal=True)


def test_command_line():
    from tc_gan_amd.run import bptt_swd, bptt_swd_ensemble, options
    with pytest.raises(SystemExit) as err:
        bptt_swd.make_parser().parse_args(['--help'])
    assert err.value.code == 0
    assert ['--swd-truth-batch'] == [f for o in options.options_of('s') for f in o['flags'] if 'truth-batch' in f]
    assert not [o for o in options.OPTIONS if '--swd-truth-batch' in o['flags']]          # the older scripts do not take it
    for given, want in (('-1', -1), ('0', 0), ('256', 256)):
        assert vars(bptt_swd.make_parser().parse_args(['--swd-truth-batch', given]))['swd_truth_batch'] == want
    with pytest.raises(SystemExit):
        bptt_swd.make_parser().parse_args(['--swd-truth-batch', 'all'])
    # the set equality tests/test_swd_ensemble.py asks for: ensemble options == solo options + members, given or not
    for extra in ([], ['--swd-truth-batch', '64']):
        solo = vars(bptt_swd.make_parser().parse_args(extra))
        ens = vars(bptt_swd_ensemble.make_parser().parse_args(extra + ['--members', 'm.json']))
        assert set(ens) == set(solo) | {'members'}


def test_help_names_the_option(capsys):
    from tc_gan_amd.run import bptt_swd
    with pytest.raises(SystemExit):
        bptt_swd.main(['--help'])
    text = capsys.readouterr().out
    assert '--swd-truth-batch' in text and 'whole truth' in text


def test_the_default_is_recorded_in_info_json(tmp_path, monkeypatch):
    """`main` hands the option to the run's config whether it was given or not (info.json is written from that config)."""
    from tc_gan_amd.run import bptt_swd
    seen = []
    monkeypatch.setattr(bptt_swd, 'do_learning', lambda learn, run_config, **kw: seen.append(dict(run_config)))
    bptt_swd.main([])
    bptt_swd.main(['--swd-truth-batch', '-1'])
    assert [c['swd_truth_batch'] for c in seen] == [0, -1]


def test_the_ensemble_refuses_the_option_by_name(tmp_path):
    from tc_gan_amd.networks import sliced_wasserstein_ensemble as swe
    from tc_gan_amd.run import bptt_swd_ensemble as bse
    assert 'swd_truth_batch' not in swe.MEMBER_KEYS | swe.SHARED_KEYS
    with pytest.raises(ValueError, match="unknown option 'swd_truth_batch'"):
        swe.validate_member_overrides([dict(swd_truth_batch=64)])
    for value in (-1, 64):
        with pytest.raises(ValueError, match='swd_truth_batch = {}'.format(value)):
            swe.ensemble_from_member_configs([dict(gen_kernel='tile', swd_truth_batch=value)])
        rc = vars(bse.make_parser().parse_args(['--members', 'm.json', '--swd-truth-batch', str(value),
                                                '--datastore', str(tmp_path / 'ens')]))
        rc.pop('members')
        with pytest.raises(ValueError, match='swd_truth_batch = {}'.format(value)):
            bse.prepare_datastores(rc, [dict(seed=1)])
        assert not (tmp_path / 'ens').exists()                     # refused before anything is written
    swe.refuse_truth_batch(dict(swd_truth_batch=0))
    swe.refuse_truth_batch({})

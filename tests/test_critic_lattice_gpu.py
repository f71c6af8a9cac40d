"""The bf16 critic bit for bit: every bf16 code path of the critic against oracle/critic_lattice.py on cases with nothing to round.

On a lattice case (every GEMM operand a bf16 number, every partial sum an fp32 number -- asserted case by case in
tests/test_critic_lattice.py) the fp64 oracle's answer is the answer of ANY correct arithmetic with bf16 operands and fp32
accumulation, in any order.  So there is no tolerance here: critic values, the stacked D values, mean D(xg), mean D(xd), the
WHOLE flat gradient, the generator side's input gradient and the accuracy must equal the oracle (operands rounded to bf16 where
the kernels round them) element by element -- `got == want` where want is 0, else |got - want| <= 2^-30 |want| (a wrong last
fp32 bit is 2^-24; the oracle's own fp64 noise is below 2^-50).  The penalty and the loss get rtol 1e-6: square root,
subtraction and square add an ulp each.

One child process per environment setting (the variables are read once per process):
    default                              critic_pack_kernel + critic_rows_kernel where the widths allow it, gemm_bf16_pipe_kernel
                                         (K >= 64), gemm_mfma_kernel<true> (K < 64), split-K slabs + splitk_reduce_kernel
    SSN_CRITIC_ROWS=0                    the layer-by-layer chain on the same GEMM kernels
    SSN_CRITIC_ROWS=0 SSN_GEMM_PIPE=0    every GEMM through gemm_mfma_kernel<true>
Each runs every case of `critic_lattice.CASES` in family A (lmd = 0) and B (lmd = 8, integer gradient norms) with
precision='bf16', and family A with precision='fp32' (products of lattice numbers are exact there too), and the tie case,
whose forward operands lie exactly half way between two bf16 numbers: only round-to-nearest-even gives the oracle's D.
The three settings must also agree among themselves bit for bit.

ONE site is not on the lattice, in ONE case: the case 'one' (widths <= 128, conditional, rectify) is computed by the fused
row-block kernels of ssn_critic_fused.hip whatever `precision` says, in fp32 throughout, and they consume the penalty's
upstream ghat = lmd * 2 (||g|| - 1) / ||g|| / np * g UNROUNDED: the quotient by ||g|| and the product with g round once each
(the bf16 paths round ghat to bf16 when they stage it, which restores the exact value).  With lmd = 8 the parameter gradients
downstream of ghat are therefore held to a bound derived from the operation count, not to exactness:
    |got - want| <= (2 + sum(dims[:-1]) + ng + nd + 2 np + 1) * 2^-24 * (sum of the |terms| of that gradient element)
-- 2 roundings in ghat, one per fused multiply-add of the second chain (its contractions run over dims[0..L-1]), one per row
of the weight-gradient sums (ng + nd rows, np rows for each of the two sweeps) and the final conversion; for 'one' that is 62
ulps of the term sum.  Bias gradients (no term from the penalty), D values, statistics and the input gradient stay exact.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import critic_lattice as cl  # noqa: E402

SETTINGS = {'default': {}, 'layers': {'SSN_CRITIC_ROWS': '0'}, 'general': {'SSN_CRITIC_ROWS': '0', 'SSN_GEMM_PIPE': '0'}}
RUNS = [('A', 'bf16'), ('B', 'bf16'), ('A', 'fp32')]


# ---------------------------------------------------------------------------------------------------------------
# the child: every case on the GPU, results into one .npz   (python tests/test_critic_lattice_gpu.py OUT.npz [case ...])
# ---------------------------------------------------------------------------------------------------------------
def _child_main(path, only=()):
    from tc_gan_amd.critic import Critic
    res = {}
    for name in (only or list(cl.CASES)):
        for family, precision in RUNS:
            case = cl.make_case(name, family)
            c = Critic(case['nx'], case['layers'], precision=precision, nonlinearity=case['nonlinearity'],
                       conditional=case['conditional'], hide_cell_type=case['hide_cell_type'])
            c.set_flat(np.concatenate([np.ravel(p) for p in case['params']]))
            xg, cg, xd, cd, xp, cp = (case[k] for k in ('xg', 'cg', 'xd', 'cd', 'xp', 'cp'))
            key = '%s_%s_%s_' % (name, family, precision)
            res[key + 'fwd'] = np.concatenate([c.forward(xg, cg).cpu().numpy(), c.forward(xd, cd).cpu().numpy()])
            res[key + 'stats'] = c.loss_grad(xg, cg, xd, cd, xp, cp, case['lmd']).cpu().numpy()
            res[key + 'flat'] = c.grads.cpu().numpy()
            res[key + 'dvals'] = c._dvals.cpu().numpy()
            gx, dmean = c.input_grad(xg, cg, scale=-1.0 / len(xg))
            res[key + 'gx'] = gx.cpu().numpy()
            res[key + 'gx_mean'] = dmean.cpu().numpy().reshape(1)
            res[key + 'accuracy'] = c.accuracy_device(xg, cg, xd, cd).cpu().numpy()
    if not only:
        tie = cl.make_tie_case()
        c = Critic(tie['nx'], tie['layers'], precision='bf16', conditional=False)
        c.set_flat(np.concatenate([np.ravel(p) for p in tie['params']]))
        res['tie_fwd'] = c.forward(tie['x'], None).cpu().numpy()
    np.savez(path, **res)


if __name__ == '__main__':
    _child_main(sys.argv[1], tuple(sys.argv[2:]))
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------
# the parent
# ---------------------------------------------------------------------------------------------------------------
_RESULTS = {}        # setting -> results of its child process, or the exception it ended with


def _gpu(setting):
    """Results of one child process under one environment setting: run once per session, whatever its end -- a child that
    failed is not started again, and after a child that was killed (a signal, the timeout) no other child is started."""
    if setting not in _RESULTS:
        killed = [s for s, r in _RESULTS.items() if isinstance(r, subprocess.TimeoutExpired) or
                  (isinstance(r, subprocess.CalledProcessError) and (r.returncode < 0 or r.returncode in (124, 134, 137, 139)))]
        if killed:
            _RESULTS[setting] = RuntimeError('not started: the child of setting %r was killed' % killed[0])
        else:
            env = {k: v for k, v in os.environ.items() if k not in ('SSN_CRITIC_ROWS', 'SSN_GEMM_PIPE')}
            env.update(SETTINGS[setting])
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, 'lattice.npz')
                try:
                    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
                    _RESULTS[setting] = dict(np.load(path))
                except (subprocess.SubprocessError, OSError) as ex:
                    _RESULTS[setting] = ex
    if isinstance(_RESULTS[setting], Exception):
        raise _RESULTS[setting]
    return _RESULTS[setting]


@functools.lru_cache(maxsize=None)
def _oracle(name, family):
    case = cl.make_case(name, family)
    return case, cl.evaluate(case, rounding='rne')


def _deviation(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return got, want, np.abs(got - want)


def _assert_exact(got, want, what, bound=None):
    """got == want where want == 0, else |got - want| <= 2^-30 |want| (+ `bound`, per element, where one is derived).
    Returns the number of elements held to exactness."""
    got, want, dev = _deviation(got, want)
    allowed = 2.0 ** -30 * np.abs(want) + (0.0 if bound is None else np.asarray(bound, dtype=np.float64).ravel())
    bad = dev > allowed
    print('%s: %d elements, %d differ, largest |got - want| %.3g (|want| up to %.3g)' % (what, want.size, int((dev > 0).sum()),
                                                                                     dev.max(), np.abs(want).max()))
    assert not bad.any(), '%s: %d of %d elements off, first at %d: got %r, want %r' % (
        what, int(bad.sum()), want.size, int(np.argmax(bad)), got[np.argmax(bad)], want[np.argmax(bad)])
    return int(want.size if bound is None else (np.asarray(bound).ravel() == 0).sum())


def _fused(case):
    """rectify, plain layers, conditional, every width <= 128, <= 2048 stacked rows -> ssn_critic_fused.hip."""
    rows = len(case['xg']) + len(case['xd']) + len(case['xp'])
    return case['conditional'] and case['nonlinearity'] == 'rectify' and max(case['layers']) <= 128 and rows <= 2048


@pytest.mark.parametrize('family,precision', RUNS, ids=['%s-%s' % r for r in RUNS])
@pytest.mark.parametrize('name', list(cl.CASES))
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_lattice_case_equals_the_oracle(setting, name, family, precision):
    """See the module docstring.  Exact: `Critic.forward` of xg and xd, `_dvals`, stats[0], stats[1], the whole flat gradient,
    `input_grad`'s gx and mean, `accuracy_device`.  rtol 1e-6: stats[2] (penalty), stats[3] (loss)."""
    got = _gpu(setting)
    case, want = _oracle(name, family)
    key = '%s_%s_%s_' % (name, family, precision)
    n = 0
    n += _assert_exact(got[key + 'fwd'], want['D'], 'forward')
    n += _assert_exact(got[key + 'dvals'], want['D'], '_dvals')
    n += _assert_exact(got[key + 'stats'][:2], want['stats'][:2], 'stats[0:2]')
    bound = None
    if _fused(case) and case['lmd'] != 0:
        dims = [case['nx'] + 3] + case['layers']
        ulps = 2 + sum(dims[:-1]) + len(case['xg']) + len(case['xd']) + 2 * len(case['xp']) + 1
        assert ulps == 62 or name != 'one'
        bound = ulps * 2.0 ** -24 * want['flat_abs']          # (0 for the biases: no term of the penalty, exact)
    n += _assert_exact(got[key + 'flat'], want['flat'], 'flat gradient', bound)
    n += _assert_exact(got[key + 'gx'], want['gx'], 'input gradient')
    n += _assert_exact(got[key + 'gx_mean'], want['gx_mean'], 'mean D of input_grad')
    n += _assert_exact(got[key + 'accuracy'], want['accuracy'], 'accuracy')
    print('%s: %d elements held to exactness' % (key, n))
    for i, what in ((2, 'penalty'), (3, 'loss')):
        g, w = float(got[key + 'stats'][i]), float(want['stats'][i])
        print('%s: got %r, want %r' % (what, g, w))
        assert abs(g - w) <= 1e-6 * abs(w), (what, g, w)


def test_the_three_settings_agree_bit_for_bit():
    ref = _gpu('default')
    for setting in ('layers', 'general'):
        other = _gpu(setting)
        assert sorted(other) == sorted(ref)
        for key, want in ref.items():
            np.testing.assert_array_equal(other[key], want, err_msg='%s: %s' % (setting, key))


@pytest.mark.parametrize('setting', ['default', 'layers'])
def test_tie_operands_round_to_nearest_even(setting):
    """x, W_1 and a good part of h_1 are exact ties between neighbouring bf16 numbers (tests/test_critic_lattice.py): D equals
    the oracle that rounds to nearest even -- and neither the truncating one nor the one that rounds away from zero -- in
    critic_rows_kernel (default) and in gemm_mfma_kernel<true> (the layer path; K = 8 and 32).  (No condition columns: a
    conditional critic of this width is computed by the fused fp32 kernels, which round nothing.)"""
    tie = cl.make_tie_case()
    want, _ = cl.tie_forward(tie, 'rne')
    got = _gpu(setting)['tie_fwd'].astype(np.float64)
    for mode in ('trunc', 'away', None):
        print('%s: %d of %d elements of D differ from the %s oracle' % (setting, int((got != cl.tie_forward(tie, mode)[0]).sum()), got.size, mode))
    np.testing.assert_array_equal(got, want)

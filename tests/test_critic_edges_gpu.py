"""The fp32 critic against the fp64 oracle at the edges of every kernel path: the cases, inputs, measures and tolerances of
oracle/critic_cases.py (what makes them meaningful is asserted without a GPU in tests/test_critic_cases.py).

One child process per environment setting (the library reads SSN_CRITIC_FUSED once per process):
    default               fused row-block kernels (RB = 4 / 8) up to 2048 stacked rows of conditional rectify nets <= 128 wide, the
                          GEMM chain (gemm_mfma_kernel<false>, split-K slabs + splitk_reduce_kernel) or the LayerNorm chain beyond
    SSN_CRITIC_FUSED=0    the fused-size cases on the chain that would otherwise never see them with these inputs
Each child runs every case through `Critic.loss_grad`, `forward`, `input_grad` and `accuracy_device` -- the nets up to 128 wide
also on one batch of 1030 rows (fused forward with RB = 8) and one of 2049 (chain) -- and writes one .npz; the parent compares
every tensor with the oracle: weight-gradient matrices element by element on the scale of the element's own row and column,
vectors / D values / input gradients relative to the tensor's largest element, loss and statistics relatively, each within four
times the deviation of the same oracle run in float32 (`critic_cases.tolerances`; per case and tensor kind, <= 1e-3).  Measured:
DESIGN.md section 1.

The path.  The library does not report which kernels computed a critic, so the table's path column is held two ways: against
the dispatch rule restated in the case module (tests/test_critic_cases.py), and here by what the two settings return -- a pass
the fused kernels take in the default setting (`loss_grad`, `forward`) comes back with other bits under SSN_CRITIC_FUSED=0
(another arithmetic: plain FMAs in another order against the fp32 MFMA), a pass they do not take comes back bit for bit the same.
A case that silently lands on another path fails `test_the_path_of_every_case`.  What the bits do NOT confirm on the device: a
fused `input_grad` pass (both backward chains add the products of an element of gx in the same order with fused multiply-adds,
so gx has the same bits either way) and a fused pass that returns fewer than 64 values (`forward` and `input_grad` of the 7 / 5 /
6 cases).  For those -- the RB = 8 form of `input_grad` at 1030 rows among them -- the path and the rows per workgroup are held by
the restated rule alone, and only their values by the oracle.
"""
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

from oracle import critic_cases as cc  # noqa: E402

SETTINGS = {'default': {}, 'chains': {'SSN_CRITIC_FUSED': '0'}}


# ---------------------------------------------------------------------------------------------------------------
# the child: every case on the GPU, results into one .npz   (python tests/test_critic_edges_gpu.py OUT.npz [case ...])
# ---------------------------------------------------------------------------------------------------------------
def _child_main(path, only=()):
    from tc_gan_amd.critic import Critic
    res = {}
    for c in cc.CASES:
        if only and c.name not in only:
            continue
        x = cc.inputs(c)
        crit = Critic(c.nx, list(c.layers), precision='fp32', normalization=list(c.norm), nonlinearity=c.nonlinearity,
                      conditional=c.conditional)
        crit.set_flat(cc.flat_params(c))
        key = c.name + '/'
        ng = c.batches[0]
        res[key + 'stats'] = crit.loss_grad(x['xg'], x['cg'], x['xd'], x['cd'], x['xp'], x['cp'], cc.LMD).cpu().numpy()
        res[key + 'grads'] = crit.grads.cpu().numpy()
        res[key + 'dvals'] = crit._dvals.cpu().numpy()
        res[key + 'fwd_p'] = crit.forward(x['xp'], x['cp']).cpu().numpy()
        gx, mean = crit.input_grad(x['xg'], x['cg'], scale=-1.0 / ng)
        res[key + 'gx'], res[key + 'gx_mean'] = gx.cpu().numpy(), mean.cpu().numpy().reshape(1)
        res[key + 'acc'] = crit.accuracy_device(x['xg'], x['cg'], x['xd'], x['cd']).cpu().numpy()
        if cc.has_extra(c):
            for n in cc.EXTRA:
                xe, ce = x['xe'][:n], None if x['ce'] is None else x['ce'][:n]
                res[key + 'fwd_%d' % n] = crit.forward(xe, ce).cpu().numpy()
                gx, mean = crit.input_grad(xe, ce, scale=-1.0 / n)
                res[key + 'gx_%d' % n], res[key + 'gxmean_%d' % n] = gx.cpu().numpy(), mean.cpu().numpy().reshape(1)
            a, b = cc.EXTRA
            xe, ce = x['xe'], x['ce']
            res[key + 'acc_%d' % a] = crit.accuracy_device(xe[:a], None if ce is None else ce[:a], xe[a:], None if ce is None else ce[a:]).cpu().numpy()
            res[key + 'acc_%d' % b] = crit.accuracy_device(xe, ce, x['xd'], x['cd']).cpu().numpy()
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
            env = {k: v for k, v in os.environ.items() if k != 'SSN_CRITIC_FUSED'}
            env.update(SETTINGS[setting])
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, 'edges.npz')
                try:
                    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=240)
                    _RESULTS[setting] = dict(np.load(path))
                except (subprocess.SubprocessError, OSError) as ex:
                    _RESULTS[setting] = ex
    if isinstance(_RESULTS[setting], Exception):
        raise _RESULTS[setting]
    return _RESULTS[setting]


def _of_case(res, c):
    return {k[len(c.name) + 1:]: v for k, v in res.items() if k.startswith(c.name + '/')}


@pytest.mark.parametrize('c', cc.CASES, ids=cc.case_id)
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_case_within_four_times_the_fp32_oracle(setting, c):
    """Every tensor of every pass of the case, in the case module's measures, within the case's tolerances."""
    got = _of_case(_gpu(setting), c)
    assert got, 'the child returned nothing for this case'
    assert all(np.isfinite(v).all() for v in got.values())
    errs, tol, dev32 = cc.errors(c, got), cc.tolerances(c), cc.fp32_oracle_deviation(c)
    bad = []
    for kind in cc.KINDS:
        for tensor, (err, where) in sorted(errs[kind].items()):
            print('%s %s %-12s %-6s %.3g   (fp32 oracle %.3g, tolerance %.3g)%s' % (
                setting, c.name, tensor, kind, err, dev32[kind], tol[kind], '   <-- element %d' % where if err > tol[kind] else ''))
            if not err <= tol[kind]:
                bad.append((tensor, kind, 'element %d' % where, err, tol[kind]))
    assert not bad, (setting, c.name, bad)


@pytest.mark.parametrize('c', cc.CASES, ids=cc.case_id)
def test_the_path_of_every_case(c):
    """See the module docstring: the passes the table sends to the fused kernels change their bits when those are switched off,
    every other pass does not -- `loss_grad` by its stacked rows, `forward` / `input_grad` by their batch."""
    a, b = _of_case(_gpu('default'), c), _of_case(_gpu('chains'), c)
    assert sorted(a) == sorted(b) and a

    def same(*keys):
        return all(np.array_equal(a[k], b[k]) for k in keys)

    assert cc.critic_path(c, cc.rows(c)) == c.path and (c.rb == cc.fused_rb(cc.rows(c)) if c.path == 'fused' else c.rb is None)
    passes = [('loss_grad', cc.rows(c), ('grads', 'stats', 'dvals')), ('forward', c.batches[2], ('fwd_p',)),
              ('input_grad', c.batches[0], ('gx', 'gx_mean'))]
    if cc.has_extra(c):
        passes += [('forward', n, ('fwd_%d' % n,)) for n in cc.EXTRA] + [('input_grad', n, ('gx_%d' % n, 'gxmean_%d' % n)) for n in cc.EXTRA]
    for what, nrows, keys in passes:
        fused = cc.critic_path(c, nrows) == 'fused'
        assert cc.critic_path(c, nrows, fused_enabled=False) != 'fused'
        if fused and (what == 'input_grad' or sum(a[k].size for k in keys) < 64):
            # a handful of values may agree by chance (`loss_grad` of the smallest case has 188), and gx does agree: both
            # backward chains add the products of an element in the same order with fused multiply-adds
            continue
        if fused:
            assert not same(*keys), '%s %s over %d rows: meant for the fused kernels, but SSN_CRITIC_FUSED=0 changes nothing' % (c.name, what, nrows)
        else:
            assert same(*keys), '%s %s over %d rows: not meant for the fused kernels, but SSN_CRITIC_FUSED=0 changes it' % (c.name, what, nrows)

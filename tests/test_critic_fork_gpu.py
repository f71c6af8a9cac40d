"""The forked chain path of `critic_loss_grad` against the single-stream one.

When every weight-gradient GEMM of both halves of an update is split over K, the layer-by-layer chain (ssn_critic.hip) runs the
penalty half on a second stream and the weight-gradient GEMMs and bias sums of both halves on a third; `SSN_CRITIC_PAR=0` keeps
everything on the caller's stream.  The slabs are added after the join in the order the GEMMs were issued, so statistics, D
values and EVERY gradient element are the same bit for bit.  The library reads `SSN_CRITIC_PAR` once per process: one child
process per setting, both with `SSN_CRITIC_ROWS=0` (bf16 stays off the row-block kernel, which does not fork), each running one
`loss_grad` and one one-call critic step (the `eps` form, whose one input launch lies in front of the fork) in fp32 and bf16.

The shape is the smallest that forks: conditional, nx = 8 (dims[0] = 11), layers [160, 160] (wider than the fused kernels take),
ng = nd = np = 512.  That it does fork -- and that the same net on 128 rows per input does not -- is asserted with the restated
`choose_splits` of oracle/critic_cases.py, so that a change of the rule that empties this test is noticed.
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

NX, LAYERS, ROWS, LMD = 8, (160, 160), 512, 10.0
PRECISIONS = ('fp32', 'bf16')
SETTINGS = {'forked': {}, 'one-stream': {'SSN_CRITIC_PAR': '0'}}


def _forks(dims, ng, nd, npn):
    """The condition of the side streams in `critic_loss_grad`: every weight-gradient GEMM of both halves is split over K --
    w_out and every layer at K = ng + nd, every layer at K = np."""
    bgd = ng + nd
    return (npn > 0 and bgd > 0 and cc.choose_splits(dims[-1], 1, bgd) > 1 and
            all(cc.choose_splits(a, b, bgd) > 1 and cc.choose_splits(a, b, npn) > 1 for a, b in zip(dims[:-1], dims[1:])))


# ---------------------------------------------------------------------------------------------------------------
# the child: both precisions on the GPU, results into one .npz   (python tests/test_critic_fork_gpu.py OUT.npz)
# ---------------------------------------------------------------------------------------------------------------
def _child_main(path):
    import torch
    from tc_gan_amd.critic import Critic, Updater
    res = {}
    for precision in PRECISIONS:
        rs = np.random.RandomState(41)
        c = Critic(NX, list(LAYERS), precision=precision, seed=5, conditional=True)
        xg, xd = (torch.as_tensor(rs.rand(ROWS, NX) * 5, device='cuda', dtype=torch.float32) for _ in range(2))
        xp = 0.25 * xg + 0.75 * xd
        cond = torch.as_tensor(np.stack([np.full(ROWS, 20.), rs.rand(ROWS) * 2 - 1, rs.randint(0, 2, ROWS)], 1),
                               device='cuda', dtype=torch.float32)
        eps = torch.as_tensor(rs.rand(ROWS), device='cuda', dtype=torch.float32)
        key = precision + '/'
        res[key + 'stats'] = c.loss_grad(xg, cond, xd, cond, xp, cond, LMD).cpu().numpy()
        res[key + 'grads'] = c.grads.cpu().numpy()
        res[key + 'dvals'] = c._dvals.cpu().numpy()
        xp2, tail = c.step(Updater(learning_rate=1e-3, update_name='adam-wgan'), xg, xd, cond, eps, LMD)
        res[key + 'step_stats'] = c.stats.cpu().numpy()
        res[key + 'step_grads'] = c.grads.cpu().numpy()
        res[key + 'step_dvals'] = c._dvals.cpu().numpy()
        res[key + 'step_xp'], res[key + 'step_tail'] = xp2.cpu().numpy(), tail.cpu().numpy()
        res[key + 'step_params'] = c.params.cpu().numpy()
    np.savez(path, **res)


if __name__ == '__main__':
    _child_main(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------
# the parent
# ---------------------------------------------------------------------------------------------------------------
_RESULTS = {}        # setting -> results of its child process, or the exception it ended with


def _gpu(setting):
    """Results of one child process under one setting: run once per session, whatever its end; after a child that did not end
    by itself with a result no other child is started."""
    if setting not in _RESULTS:
        failed = [s for s, r in _RESULTS.items() if isinstance(r, Exception)]
        if failed:
            _RESULTS[setting] = RuntimeError('not started: the child of setting %r failed' % failed[0])
        else:
            env = {k: v for k, v in os.environ.items() if k != 'SSN_CRITIC_PAR'}
            env.update(SETTINGS[setting], SSN_CRITIC_ROWS='0')
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, 'fork.npz')
                try:
                    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=120)
                    _RESULTS[setting] = dict(np.load(path))
                except (subprocess.SubprocessError, OSError) as ex:
                    _RESULTS[setting] = ex
    if isinstance(_RESULTS[setting], Exception):
        raise _RESULTS[setting]
    return _RESULTS[setting]


@pytest.mark.parametrize('precision', PRECISIONS)
def test_forked_chain_matches_the_single_stream(precision):
    dims = [NX + 3] + list(LAYERS)
    assert dims[0] == 11 and _forks(dims, ROWS, ROWS, ROWS)
    assert not _forks(dims, 128, 128, 128)                      # the control: K < 512, nothing is split, one stream
    want, got = _gpu('one-stream'), _gpu('forked')
    keys = [k for k in want if k.startswith(precision + '/')]
    assert len(keys) == 9 and sorted(want) == sorted(got)
    for k in keys:
        assert np.isfinite(want[k]).all() and np.abs(want[k]).max() > 0, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)

"""Which kernel a generator pass or a batched solve runs, by the library's own word: host arithmetic only
(`ssn_gen_forward_variant`, `ssn_solve_batch_variant_for`), no device.  The query IS the forward's decision, so these values pin
the dispatch itself; the expected numbers were read off the library before the rule was gathered into one place."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _variant(B, NB, M=16, kernel=0, seqlen=12, skip=4, save=False, **gen):
    from tc_gan_amd import clib, genops
    gp = genops.make_gen_params(seqlen=seqlen, skip_steps=skip, kernel=0, **gen)
    gp.kernel = kernel                                   # (raw: the refused codes never pass clib.gen_kernel_code)
    return clib.libssnode.ssn_gen_forward_variant(B, NB, M, seqlen, int(save), ctypes.byref(gp))


@pytest.fixture
def precision():
    """Sets the operand precision of the automatic choice for one test; the previous setting comes back afterwards."""
    from tc_gan_amd import clib
    before = clib.set_operand_precision('split')
    try:
        yield clib.set_operand_precision
    finally:
        clib.set_operand_precision(before)


def _child(env, calls):
    """The automatic or explicit choice for each (B, NB, kernel) of `calls` in a fresh process with `env` over the environment,
    minus the two switches (the library reads each of them once)."""
    code = ("import ctypes, json, sys\nsys.path.insert(0, %r)\nfrom tc_gan_amd import clib, genops\nout = []\n"
            "for B, NB, kernel in json.loads(sys.argv[1]):\n"
            "    gp = genops.make_gen_params(seqlen=12, skip_steps=4, kernel=kernel)\n"
            "    out.append(clib.libssnode.ssn_gen_forward_variant(B, NB, 16, 12, 0, ctypes.byref(gp)))\n"
            "print(json.dumps(out))\n" % ROOT)
    env = dict({k: v for k, v in os.environ.items() if k not in ('SSN_FWD_SPLIT', 'SSN_FWD_WIDE')}, **env)
    out = subprocess.run([sys.executable, '-c', code, json.dumps(calls)], check=True, env=env, timeout=300, stdout=subprocess.PIPE)
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


AUTO = [((3, 8), 1), ((48, 4), 1), ((257, 3), 1), ((95, 8), 1), ((96, 8), 5), ((191, 8), 5), ((192, 8), 4), ((256, 8), 4),
        ((257, 8), 8), ((129, 12), 8)]
FP32_OPERANDS = [((96, 8), 3), ((192, 8), 2), ((257, 8), 2)]


@pytest.mark.parametrize('shape,want', AUTO)
def test_automatic_choice_fills_the_chip(precision, shape, want):
    assert _variant(*shape) == want


@pytest.mark.parametrize('shape,want', FP32_OPERANDS)
def test_automatic_choice_on_fp32_operands(precision, shape, want):
    assert _variant(*shape, io_type='asym_power') == want       # no rate bound: the fp16-split forward does not apply
    precision('fp32')
    assert _variant(*shape) == want


def test_initial_operand_precision_from_the_environment():
    assert _child(dict(SSN_FWD_SPLIT='0'), [(B, NB, 0) for (B, NB), _ in FP32_OPERANDS]) == [want for _, want in FP32_OPERANDS]


def test_automatic_choice_leaves_the_split_kernels_where_they_do_not_apply(precision):
    assert _variant(300, 8, 200) == 8
    assert _variant(300, 8, 200, rate_hard_bound=4e4) == 2       # r 2^rshift would leave the fp16 range
    assert _variant(300, 8, 200, dt=20) == 2                     # dt > tau: no bound on the rates
    # trajectory stores address one draw's block with 32-bit byte offsets: NB T 2N < 2^29
    T = 2 ** 29 // 1600 + 1
    assert _variant(300, 8, 200, seqlen=T, save=True) == 1
    assert _variant(300, 8, 200, seqlen=T, save=False) == 8


@pytest.mark.parametrize('gen,NB,M,want', [
    (dict(io_type='asym_tanh'), 8, 16, [1, 2, 3, 4, 5, 6, -1, 8]),
    (dict(io_type='asym_power'), 8, 16, [1, 2, 3, -1, -1, -1, -1, -1]),
    (dict(io_type='asym_tanh'), 3, 16, [1, -1, -1, -1, -1, -1, -1, -1]),
    (dict(io_type='asym_tanh'), 8, 210, [1, -1, -1, -1, -1, -1, -1, -1]),   # the matrix-core kernels stop at 2N = 208
    (dict(io_type='asym_tanh'), 8, 2050, [-1] * 8)])
def test_explicit_codes(precision, gen, NB, M, want):
    assert [_variant(3, NB, M, kernel=k, **gen) for k in range(1, 9)] == want
    if M in (210, 2050):
        assert _variant(3, NB, M, kernel=0, **gen) == want[0]


@pytest.mark.parametrize('wide,want', [('0', [6, 6, 5, 6, 8]), ('3', [7, 7, 5, 6, 8])])
def test_forms_of_the_two_group_split_kernel(wide, want):
    assert _child(dict(SSN_FWD_WIDE=wide), [(192, 8, k) for k in (0, 4, 5, 6, 8)]) == want


def test_the_query_refuses_the_horizons_the_launch_refuses(precision):
    """(It used to answer 8 for both.)"""
    assert _variant(300, 8, 200, seqlen=0, skip=0) == -1
    assert _variant(300, 8, 200, seqlen=12, skip=12) == -1


def test_codes_that_name_no_kernel_are_refused(precision):
    """7, 9, -1: the query used to answer 1 for some of them, and the launch ran the tile kernels without a word."""
    for io_type in ('asym_tanh', 'asym_power'):
        for NB in (8, 3):
            assert [_variant(3, NB, kernel=k, io_type=io_type) for k in (7, 9, -1)] == [-1, -1, -1]


def test_solver_variants(precision):
    from tc_gan_amd import clib
    sp = clib.SolverParams(io_type=clib.IO_CODES['asym_tanh'], max_iter=100, k=0.01, n=2.2, tau_E=10., tau_I=1., dt=0.1, atol=1e-5,
                           rate_soft_bound=200., rate_hard_bound=1000.)

    def solve(B, NB, M, nbytes):
        return clib.libssnode.ssn_solve_batch_variant_for(B, NB, M, nbytes, ctypes.byref(sp))
    assert [solve(B, 8, 200, 4) for B in (3, 192, 257)] == [2, 6, 8]
    assert solve(257, 8, 104, 4) == 2
    assert [solve(B, 8, M, 8) for B, M in ((3, 200), (192, 200), (257, 200), (257, 104))] == [2, 2, 2, 2]

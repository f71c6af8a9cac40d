"""Host paths of the device MT19937 draw (csrc/ssn_mt19937.hip) that the draw-by-draw tests do not walk: the ring of buffer
sets with buffers that grow, the ring of tickets taken over while states of both kinds are pending, and calls the library
refuses.  Integer work throughout: every comparison is bit equality with numpy's own RandomState."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _at(seed, pos):
    """(device-continued generator, numpy twin) of `seed`, both moved to position `pos` of their current block."""
    from tc_gan_amd.utils import as_randomstate
    dev, host = as_randomstate(seed), np.random.RandomState(seed)
    for rs in (dev, host):
        st = rs.get_state()
        rs.set_state((st[0], st[1], pos) + tuple(st[3:]))
    return dev, host


def _same_state(dev, host):
    sd, sh = dev.get_state(), host.get_state()
    return sd[2] == sh[2] and np.array_equal(sd[1], sh[1])


@pytest.mark.parametrize('pos', [0, 623])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_back_to_back_draws_through_the_buffer_ring_with_growth(dtype, pos):
    """Five draws of one generator with no synchronisation between them: more draws than the library has buffer sets (3), the
    third and fourth larger than any before (1, 2, then 5 segments of 128 blocks: the sets' buffers grow while earlier
    kernels may still read them), the fifth a small draw in a set that has grown."""
    from tc_gan_amd.networks.ssn import device_rand
    dev, host = _at(7, pos)
    sizes = (1, 313, 128 * 312 + 1, 4 * 128 * 312 + 1, 313)
    got = [device_rand(dev, (n,), dtype) for n in sizes]
    torch.cuda.synchronize()
    for n, g in zip(sizes, got):
        want = host.rand(n)
        if dtype == torch.float32:
            want = want.astype('float32')
        assert np.array_equal(g.cpu().numpy(), want), n
    assert _same_state(dev, host)


def test_ticket_takeover_parks_states_of_both_kinds():
    """Twenty draws begun before any of their generators is used again (the library keeps eight tickets): ten leave the
    state in the caller's current block (5 doubles from position 0: the pending state is the key itself), ten leave it
    (the state is computed on the device).  The generators are then used in reverse order: the early ones get their
    states from where the takeover parked them."""
    from tc_gan_amd.networks.ssn import device_rand
    gens = []
    for s in range(10):
        gens.append((_at(100 + s, 0), (5,)))
        gens.append((_at(200 + s, 624), (3, 40, 40)))
    got = [device_rand(dev, shape, torch.float64) for (dev, _), shape in gens]
    for ((dev, host), shape), g in reversed(list(zip(gens, got))):
        assert np.array_equal(g.cpu().numpy(), host.rand(*shape)), shape
        assert np.array_equal(dev.choice(1000, 7), host.choice(1000, 7))
        assert np.array_equal(dev.rand(5), host.rand(5))
        assert _same_state(dev, host)


def _refused_calls(key, pos, out, tail_out, ticket):
    from tc_gan_amd import clib
    lib, st, tk = clib.libssnode, clib.stream_ptr(), ctypes.byref(ticket)
    jds = [(ctypes.c_float * 4)(1., 1., 1., 1.) for _ in range(3)]
    return {
        'pos = 625': lambda: lib.ssn_mt19937_random_sample_begin_f32(key.ctypes.data, 625, 21, 0, 21, out.data_ptr(), st, tk),
        'skip + count > total': lambda: lib.ssn_mt19937_random_sample_begin_f32(key.ctypes.data, pos, 21, 7, 15, out.data_ptr(), st, tk),
        'N = 0': lambda: lib.ssn_build_w_mt19937_begin_f32(key.ctypes.data, pos, 1, 0, 1, jds[0], jds[1], jds[2], out.data_ptr(),
                                                           None, 0, st, tk),
        'tail_kind = 3': lambda: lib.ssn_mt19937_random_sample_tail_begin_f32(key.ctypes.data, pos, 21, 0, 21, out.data_ptr(), 3, 7, 0, 7,
                                                                              tail_out.data_ptr(), st, tk),
    }


@pytest.mark.parametrize('case', ['pos = 625', 'skip + count > total', 'N = 0', 'tail_kind = 3'])
def test_refused_calls_leave_the_library_usable(case):
    """Host-side argument checks: the call returns non-zero, hands out no ticket, and the generator's next draw and state
    are numpy's."""
    from tc_gan_amd import clib
    from tc_gan_amd.networks.ssn import device_rand
    clib.require_gpu()
    dev, host = _at(31, 17)
    st = dev.get_state()
    key = np.ascontiguousarray(st[1], dtype=np.uint32)
    out = torch.zeros(64, device='cuda', dtype=torch.float32)
    tail_out = torch.zeros(64, device='cuda', dtype=torch.float32)
    ticket = ctypes.c_int(-1)
    assert _refused_calls(key, int(st[2]), out, tail_out, ticket)[case]() != 0
    assert ticket.value == -1
    got = device_rand(dev, (3, 7), torch.float32)
    assert np.array_equal(got.cpu().numpy(), host.rand(3, 7).astype('float32'))
    assert _same_state(dev, host)

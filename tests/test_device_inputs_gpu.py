"""The inputs of a device-noise forward in one call (`ssn_gen_inputs_philox_f32`; `gen_inputs_kernel`, csrc/ssn_aux.hip), held
to a known answer: the noise outputs to the Philox restatement (oracle/philox_numpy.py), W and ext to the separately pinned
kernels (`ssn_build_w_f32`, `ssn_stimulus_f32`, `ssn_stimulus_amp_f32`, `ssn_stimulus_hetero_f32`), the whole call to the three
calls the header says it stands for, and the slices of the ranks of a data-parallel job to the single call -- at the shapes
where a vector of four leaves a row, where the W and the stimulus range reach their caps of workgroups and stride, at every
alignment of the two stream offsets within the Philox blocks, and up to and across stream element 2^34, where the high word of
the counter first changes (oracle/device_inputs_cases.py).  Then the Python dispatch: a forward that takes the one-call path
and a forward on the materialised noise of the same slices give the same bits.

Every comparison is exact.  Every output lies inside a larger allocation filled with a sentinel, 16-byte aligned, and nothing
outside the outputs may change.

Out of scope: the cap of the zin / amp range (8192 workgroups) is reached only with B * 2N > 8.3 million, hence a W of several
GB; that range's stride is not exercised here."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import device_inputs_cases as dc
from oracle import ssn_numpy as on

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64                      # elements on either side: 256 bytes, so the buffer inside is as aligned as the allocation


class Guarded(object):
    """n float32 elements inside an allocation of n + 2 * GUARD filled with SENTINEL (no output of the call can be that number)."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape))
        self.whole = torch.full((self.n + 2 * GUARD,), SENTINEL, device='cuda', dtype=torch.float32)
        self.ptr = self.whole.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    @property
    def t(self):
        return self.whole[GUARD:GUARD + self.n].reshape(self.shape)

    def guards_intact(self):
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())


def _jds():
    jds = on.new_JDS()
    return [(ctypes.c_float * 4)(*np.asarray(jds[k], dtype='double').reshape(4)) for k in 'JDS']


def _dev(a):
    return torch.from_numpy(np.array(a)).to('cuda')                  # (a copy: the shared references are read-only)


def one_call(N, B, NB, bw, con, v, bernoulli, keep_z, off_z, off_zin):
    """`ssn_gen_inputs_philox_f32` into guarded buffers: dict of `Guarded` (z: None when not kept).  zin and amp are handed
    over even with v = NULL, where the call must leave them alone."""
    from tc_gan_amd import clib
    M = 2 * N
    out = dict(W=Guarded((B, M, M)), z=Guarded((B, M, M)) if keep_z else None, zin=Guarded((B, M)), amp=Guarded((B, M)),
               ext=Guarded((B, NB, M)))
    J, D, S = _jds()
    a = clib.GenInputs(seed=dc.SEED, off_z=off_z, off_zin=off_zin, J=J, D=D, S=S, bw=bw.data_ptr(), con=con.data_ptr(),
                       smoothness=dc.SMOOTHNESS, v=None if v is None else v.data_ptr(), bernoulli=int(bernoulli),
                       W=out['W'].ptr, z=out['z'].ptr if keep_z else None, zin=out['zin'].ptr, amp=out['amp'].ptr,
                       ext=out['ext'].ptr, B=B, NB=NB, N=N)
    clib.check(clib.libssnode.ssn_gen_inputs_philox_f32(ctypes.byref(a), clib.stream_ptr()), 'ssn_gen_inputs_philox_f32')
    torch.cuda.synchronize()
    return out


def three_calls(N, B, NB, bw, con, v, bernoulli, keep_z, off_z, off_zin):
    """The calls the header names, in its order: `ssn_philox_amp_f32`, `ssn_stimulus_amp_f32`, `ssn_build_w_philox_f32`."""
    from tc_gan_amd import clib
    lib = clib.libssnode
    M = 2 * N
    J, D, S = _jds()
    W, ext = (torch.full(s, SENTINEL, device='cuda') for s in ((B, M, M), (B, NB, M)))
    z = torch.full((B, M, M), SENTINEL, device='cuda') if keep_z else None
    zin = amp = None
    if v is not None:
        zin, amp = torch.full((B, M), SENTINEL, device='cuda'), torch.full((B, M), SENTINEL, device='cuda')
        clib.check(lib.ssn_philox_amp_f32(dc.SEED, off_zin, v.data_ptr(), zin.data_ptr(), amp.data_ptr(), B * M, M, int(bernoulli),
                                          clib.stream_ptr()), 'ssn_philox_amp_f32')
    clib.check(lib.ssn_stimulus_amp_f32(bw.data_ptr(), con.data_ptr(), ctypes.c_float(dc.SMOOTHNESS),
                                        None if amp is None else amp.data_ptr(), ext.data_ptr(), B, NB, N, clib.stream_ptr()),
               'ssn_stimulus_amp_f32')
    clib.check(lib.ssn_build_w_philox_f32(dc.SEED, off_z, J, D, S, W.data_ptr(), None if z is None else z.data_ptr(), B, N,
                                          clib.stream_ptr()), 'ssn_build_w_philox_f32')
    return dict(W=W, z=z, zin=zin, amp=amp, ext=ext)


def build_w(z, N):
    from tc_gan_amd import clib
    J, D, S = _jds()
    W = torch.full(tuple(z.shape), SENTINEL, device='cuda')
    clib.check(clib.libssnode.ssn_build_w_f32(z.data_ptr(), J, D, S, W.data_ptr(), int(z.shape[0]), N, clib.stream_ptr()), 'ssn_build_w_f32')
    return W


def stimulus(bw, con, N, amp=None, zin=None, v=None):
    """`ssn_stimulus_f32` (nothing given), `ssn_stimulus_amp_f32` (amp) or `ssn_stimulus_hetero_f32` with nv = 2N (zin and v)."""
    from tc_gan_amd import clib
    lib = clib.libssnode
    B, NB = bw.shape
    ext = torch.full((B, NB, 2 * N), SENTINEL, device='cuda')
    sm = ctypes.c_float(dc.SMOOTHNESS)
    if zin is not None:
        clib.check(lib.ssn_stimulus_hetero_f32(bw.data_ptr(), con.data_ptr(), sm, zin.data_ptr(), v.data_ptr(), 2 * N, ext.data_ptr(),
                                               B, NB, N, clib.stream_ptr()), 'ssn_stimulus_hetero_f32')
    elif amp is not None:
        clib.check(lib.ssn_stimulus_amp_f32(bw.data_ptr(), con.data_ptr(), sm, amp.data_ptr(), ext.data_ptr(), B, NB, N,
                                            clib.stream_ptr()), 'ssn_stimulus_amp_f32')
    else:
        clib.check(lib.ssn_stimulus_f32(bw.data_ptr(), con.data_ptr(), sm, ext.data_ptr(), B, NB, N, clib.stream_ptr()), 'ssn_stimulus_f32')
    return ext


def _mismatch(got, want):
    """'' when the tensors hold the same bits, else how many elements differ and the largest difference."""
    if torch.equal(got, want):
        return ''
    bad = got != want
    return '%d of %d differ (max |diff| %.3g)' % (int(bad.sum()), got.numel(), float((got.double() - want.double()).abs().max()))


@pytest.mark.parametrize('keep_z', [True, False], ids=['z-kept', 'z-null'])
@pytest.mark.parametrize('mode', dc.MODES)
@pytest.mark.parametrize('row', dc.ROWS, ids=dc.row_id)
def test_one_call_against_restatement_and_pinned_kernels(row, mode, keep_z):
    """At every pair of offsets of the row: z (when kept), zin and amp equal the restatement (amp in its two-rounding form);
    W equals `ssn_build_w_f32` of the returned z -- and of the restated z when z = NULL, so W does not depend on z being
    kept; ext equals `ssn_stimulus_f32` with v = NULL, else both `ssn_stimulus_amp_f32` of the returned amp and
    `ssn_stimulus_hetero_f32` of the returned zin; every output equals the three separate calls; nothing outside the outputs
    is written.  All checks of a case are evaluated and the ones that fail are named."""
    N, B, NB = row
    bw, con = (_dev(a) for a in dc.stimuli(row))
    v = None if mode == 'plain' else _dev(dc.v_of(row))
    failures = []
    for off_z, off_zin in dc.offsets(row):
        def check(name, got, want):
            bad = _mismatch(got, want)
            if bad:
                failures.append('off_z=%d off_zin=%d %s: %s' % (off_z, off_zin, name, bad))

        z_want, zin_want, amp_want = dc.noise(row, mode, off_z, off_zin)
        got = one_call(N, B, NB, bw, con, v, mode == 'bernoulli', keep_z, off_z, off_zin)
        for name, g in got.items():
            if g is not None and not g.guards_intact():
                failures.append('off_z=%d off_zin=%d: written outside %s' % (off_z, off_zin, name))
        z_dev = _dev(z_want)
        if keep_z:
            check('z vs restatement', got['z'].t, z_dev)
            check('W vs ssn_build_w_f32(returned z)', got['W'].t, build_w(got['z'].t.contiguous(), N))
        else:
            check('W vs ssn_build_w_f32(restated z)', got['W'].t, build_w(z_dev, N))
        if mode == 'plain':
            if not (got['zin'].untouched() and got['amp'].untouched()):
                failures.append('off_z=%d off_zin=%d: zin / amp written with v = NULL' % (off_z, off_zin))
            check('ext vs ssn_stimulus_f32', got['ext'].t, stimulus(bw, con, N))
        else:
            zin, amp = got['zin'].t.contiguous(), got['amp'].t.contiguous()
            check('zin vs restatement', zin, _dev(zin_want))
            check('amp vs two-rounding restatement', amp, _dev(amp_want))
            check('ext vs ssn_stimulus_amp_f32(returned amp)', got['ext'].t, stimulus(bw, con, N, amp=amp))
            check('ext vs ssn_stimulus_hetero_f32(returned zin, v)', got['ext'].t, stimulus(bw, con, N, zin=zin, v=v))
        sep = three_calls(N, B, NB, bw, con, v, mode == 'bernoulli', keep_z, off_z, off_zin)
        for name in ('W', 'ext') + (('z',) if keep_z else ()) + (('zin', 'amp') if v is not None else ()):
            check('%s vs the three separate calls' % name, got[name].t, sep[name])
    assert not failures, '\n'.join(failures)


def _world_cases():
    for row in dc.ROWS:
        for world in (2, 4):
            # (a draw of the row's B models when the ranks divide it, else of B models per rank)
            Bg = row.B if row.B % world == 0 else row.B * world
            M = 2 * row.N
            positions = [4 * 17 + 1]
            if row.N in (10, 101):
                positions.append(dc.E34 - (Bg * M * M // 2) // 4 * 4 - 3)         # the z draw across 2^34, misaligned
                positions.append(dc.E34 - Bg * M * M - Bg * M // 2 - 1)           # the zin draw across 2^34
            yield pytest.param(row, world, Bg, positions, id='%s-world%d' % (dc.row_id(row), world))


@pytest.mark.parametrize('mode', dc.MODES)
@pytest.mark.parametrize('row,world,Bg,positions', list(_world_cases()))
def test_rank_slices_compose(row, world, Bg, positions, mode):
    """Rows split over 2 and 4 ranks, each rank calling with the offsets `DeviceNoise.take` gives it for the z draw and then
    the zin draw (the order of `gen_noise`) and with its rows of bw and con: the concatenated outputs equal the single call."""
    from tc_gan_amd.networks.ssn import DeviceNoise
    N, NB, M = row.N, row.NB, 2 * row.N
    bw, con = (_dev(a) for a in dc.stimuli(row, Bg))
    v = None if mode == 'plain' else _dev(dc.v_of(row))
    names = ('W', 'z', 'ext') + (('zin', 'amp') if v is not None else ())
    failures = []
    for pos in positions:
        def run(rank, world):
            zg = DeviceNoise(dc.SEED, rank, world)
            zg.set_state(dict(seed=dc.SEED, position=pos))
            Bl = Bg // world
            off_z, off_zin = zg.take(Bl * M * M), zg.take(Bl * M)
            assert zg.position == pos + Bg * M * M + Bg * M
            rows = slice(rank * Bl, (rank + 1) * Bl)
            got = one_call(N, Bl, NB, bw[rows].contiguous(), con[rows].contiguous(), v, mode == 'bernoulli', True, off_z, off_zin)
            assert all(got[k].guards_intact() for k in names)
            return {k: got[k].t for k in names}

        whole = run(0, 1)
        parts = [run(r, world) for r in range(world)]
        for k in names:
            bad = _mismatch(torch.cat([p[k] for p in parts]), whole[k])
            if bad:
                failures.append('position %d %s: %s' % (pos, k, bad))
    assert not failures, '\n'.join(failures)


GEN_KW = dict(smoothness=dc.SMOOTHNESS, k=0.01, n=2.2, tau_E=10., tau_I=1., dt=0.1, io_type='asym_tanh', seqlen=30, skip_steps=20)


@pytest.mark.parametrize('position', dc.GEN_POSITIONS, ids=['start', 'z-across-2^34', 'zin-across-2^34'])
@pytest.mark.parametrize('dist_in', ['bernoulli', 'uniform'])
@pytest.mark.parametrize('ssn_type', ['default', 'heteroin', 'deg-heteroin'])
def test_both_paths_of_a_forward_give_the_same_bits(ssn_type, dist_in, position, monkeypatch):
    """`TuningCurveGenerator` with `z_device_seed`: `forward` on the `gen_noise` result (`PhiloxDraw` / `PhiloxAmp`: the
    one-call path, counted here) against `forward` on the materialised tensors of the same slices (`PhiloxDraw.materialize()`
    and the zin of `PhiloxAmp.materialize()`: `generate_weight_batch` and `stimulus_hetero_kernel`) -- tuning curve, time
    average and both penalties identical, and so is what the V gradient reads afterwards (the stored zin and the un-amplified
    stimulus), with the inputs themselves (W, z, ext)."""
    from tc_gan_amd import clib
    from tc_gan_amd.networks.ssn import PhiloxAmp, PhiloxDraw, TuningCurveGenerator
    calls = []
    real = clib.libssnode.ssn_gen_inputs_philox_f32
    monkeypatch.setattr(clib.libssnode, 'ssn_gen_inputs_philox_f32', lambda *a: calls.append(1) or real(*a))
    jds = on.new_JDS()
    N, B, NB = dc.GEN_SITES, dc.GEN_MODELS, dc.GEN_STIMULI
    rs = np.random.RandomState(5)
    bw, con = rs.rand(B, NB), rs.choice([5.0, 20.0], size=(B, NB))

    def make():
        gen = TuningCurveGenerator(num_sites=N, num_tcdom=NB, J=jds['J'], D=jds['D'], S=jds['S'], batchsize=B,
                                   probes=list(range(0, 2 * N, 3)), include_time_avg=True, z_device_seed=dc.GEN_SEED,
                                   ssn_type=ssn_type, dist_in=dist_in, **({} if ssn_type == 'default' else dict(V=dc.GEN_V[ssn_type])),
                                   **GEN_KW)
        gen._zgen.set_state(dict(seed=dc.GEN_SEED, position=position))
        return gen

    a = make()
    noise = a.gen_noise(None, stimulator_bandwidths=bw)
    assert isinstance(noise['model_zs'], PhiloxDraw) and noise['model_zs'].offset == position
    assert (ssn_type == 'default') == ('model_zs_in' not in noise)
    out_a = a.forward(save=True, stimulator_bandwidths=bw, stimulator_contrasts=con, **noise)
    assert len(calls) == 1
    b = make()
    mat = dict(model_zs=noise['model_zs'].materialize())
    if ssn_type != 'default':
        assert isinstance(noise['model_zs_in'], PhiloxAmp) and noise['model_zs_in'].offset == position + B * 4 * N * N
        mat['model_zs_in'] = noise['model_zs_in'].materialize()[0]
    out_b = b.forward(save=True, stimulator_bandwidths=bw, stimulator_contrasts=con, **mat)
    assert len(calls) == 1                                   # (the second forward went through the separate kernels)
    failures = []
    for name in out_a._fields:
        assert getattr(out_a, name).numel() > 0 and bool(torch.isfinite(getattr(out_a, name)).all())
        if _mismatch(getattr(out_a, name), getattr(out_b, name)):
            failures.append(name + ': ' + _mismatch(getattr(out_a, name), getattr(out_b, name)))
    if _mismatch(a.last_penalties, b.last_penalties):
        failures.append('penalties: ' + _mismatch(a.last_penalties, b.last_penalties))
    for name in ('zin', 'ext_base', 'ext', 'W', 'z'):
        sa, sb = a._saved[name], b._saved[name]
        assert (sa is None) == (sb is None) == (ssn_type == 'default' and name in ('zin', 'ext_base'))
        if sa is not None and _mismatch(sa, sb):
            failures.append('saved %s: %s' % (name, _mismatch(sa, sb)))
    assert not failures, '\n'.join(failures)

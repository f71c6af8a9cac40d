"""No GPU: the cases of oracle/ff_cases.py -- the restated index arithmetic, the conditions of every case, the oracle against
oracle/ff_torch.py and autograd, the sensitivity of the element-wise check to one wrong grid point, and the blind spots of
tests/test_ff_gpu.py as numbers."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import ff_cases as fc
from oracle import ff_torch as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = list(dict.fromkeys(fc._key(c) for c in fc.CASES))            # the input sets, in the order of the cases


def _cases_of(key):
    return [c for c in fc.CASES if fc._key(c) == key]


def _set_id(key):
    return fc.case_id(key._replace(entry='set', path=''))


def test_the_advance_restated_visits_every_point_at_its_coordinates():
    """`advance_trace` (the lattice kernels' incremental (bx, by, bz)) lands on divmod's coordinates at every (thread, sweep),
    visits every 16-byte group or point once, and the boxes carry as the case table says."""
    for box in list(fc.BOXES) + [9, 11, 18, 28, 32, 36]:
        for pts in ((4, 1) if box ** 3 % 4 == 0 else (1,)):
            tr = fc.advance_trace(box, pts)
            assert sorted(g for _, _, g, _, _, _ in tr) == list(range(0, box ** 3 - pts + 1, pts))
            assert all(xyz == fc.coords(box, g) for _, _, g, xyz, _, _ in tr), (box, pts)
    assert fc.carry_points(16, 4) == {}                               # four exact sweeps, no carry
    assert set(fc.carry_points(20, 4)) == set(fc.carry_points(40, 4)) == {'z', 'y', 'zy'}
    assert set(fc.carry_points(13, 1)) == {'z', 'y', 'zy'}


def test_a_16_byte_group_crosses_rows_but_never_planes():
    for box in range(1, 65):
        row, plane = fc.group_crossings(box)
        assert plane is None
        assert (row is not None) == (box % 4 == 2 and box > 1), box
    assert fc.group_crossings(6)[0] == (5, 6) and fc.group_crossings(14)[0] == (13, 14)


def test_named_points_of_the_production_box():
    p = fc.named_points(40, True)
    assert p['last'] == 63999 and p['first'] == 0 and p['last-group'] == 63996
    assert (p['vec-sweep0-end'], p['vec-sweep1-start'], p['scalar-sweep0-end'], p['scalar-sweep1-start']) == (1023, 1024, 255, 256)
    assert p['vec-ragged-sweep-start'] == 62 * 1024 and 64000 % 1024 != 0 and 64000 % 256 == 0
    assert p['ring-refill'] == 4 * 768 and [fc.coords(40, p['iz&3=%d' % k])[2] & 3 for k in (1, 2, 3)] == [1, 2, 3]
    assert 'ring-refill' in fc.named_points(16, True) and 'ring-refill' not in fc.named_points(12, True)
    for box in fc.BOXES:              # every named point of a box lies in one of its lattice groups, three indices per axis at most
        groups = fc.lattice_groups(box)
        assert sorted(g for grp in groups for g in grp.values()) == sorted(fc.named_points(box, True).values())
        assert all(len(set(fc.coords(box, g)[ax] for g in grp.values())) <= 3 for grp in groups for ax in range(3))


def test_the_case_table_covers_what_it_claims():
    cs = fc.CASES
    assert len(set(fc.case_id(c) for c in cs)) == len(cs)
    assert {c.box for c in cs} == {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 16, 20, 24, 40}
    assert {c.ni for c in cs} == {1, 20, 26, 27, 28, 32} and {c.nhid for c in cs} == {1, 3} and {c.a for c in cs} == {0.5, 1.0, 2.5}
    assert {0, 1, 255, 256, 257, 600} <= {c.ncon for c in cs}
    assert {c.stim for c in cs} == set(fc.STIM_KINDS)
    assert {(c.entry, c.path) for c in cs} == {('forward', 'generic'), ('forward', 'lattice'), ('forward_sparse', 'sparse-generic'),
                                               ('forward_sparse', 'sparse-lattice'), ('backward', 'generic'), ('backward_sparse', 'sparse-generic')}
    assert all(2 <= c.nsam <= 3 for c in cs)
    for box in fc.BOXES:              # every box runs every kernel it can reach
        paths = {c.path for c in cs if c.box == box}
        assert {'generic', 'lattice', 'sparse-generic'} <= paths and (('sparse-lattice' in paths) == (box % 4 == 0))
    # 27 stimuli off the lattice by one ulp or by their order take the generic kernels
    assert all(c.path in ('generic', 'sparse-generic') for c in cs if c.stim in ('lattice-ulp', 'lattice-perm'))
    # the launchers' constants, against the source text
    src = open(os.path.join(ROOT, 'tc_gan_amd', 'csrc', 'ssn_ff.hip')).read()
    assert 'constexpr int FF_MAX_NI = %d;' % fc.FF_MAX_NI in src
    assert 'lat && a.ni == 27 && a.box % 4 == 0 && G % 4 == 0 && ((uintptr_t)a.RF_w % 16) == 0' in src
    assert '#define FF_SPARSE_DEPTH 3' in src and 'v += 256' in src


@pytest.mark.parametrize('key', SETS, ids=_set_id)
def test_conditions(key):
    """Shares of the named points, distance from the kink, the predicted path of every entry point, float32-exact inputs;
    -1 slots mid-list and at the end; the exponent arguments that matter stay where float32 exponentials are accurate."""
    for c in _cases_of(key):
        fig = fc.conditions(c)
    x, o = fc.inputs(c), fc.oracle(c)
    assert fig['xarg'] < 30
    if c.ncon >= 8:
        idx = x['idx']
        filled = idx >= 0
        assert (~filled[:, :, -1]).any() and filled[:, :, -1].any() or c.nsam * c.nhid < 3      # lists of different lengths
        assert any((~filled[s, h, :np.nonzero(filled[s, h])[0][-1]]).any() for s in range(c.nsam) for h in range(c.nhid))    # a -1 mid-list
        assert all(len(set(idx[s, h][filled[s, h]])) == filled[s, h].sum() for s in range(c.nsam) for h in range(c.nhid))   # an index once
    if c.ncon >= len(x['anchors']) + 4:
        assert fc.fully_connected(c)
    if c.ncon > 256:                  # named points on both sides of the list's own sweep boundary and in its last filled slot
        named = {g for g, _ in x['named'].values()}
        edge = [x['idx'][s, h, t] for s in range(c.nsam) for h in range(c.nhid) for t in (255, 256) if x['idx'][s, h, t] >= 0]
        assert len(edge) >= 3 and all(g in named for g in edge)           # (lists that end before the boundary aside)
    ts = x['TH_sam']
    assert (np.isin(ts, fc._f32(fc.SPECIAL_TH))).sum() >= (ts.size + 1) // 2
    assert set(o['tol']) == {'den', 'q', 'out', 'dsig'} and max(o['tol'].values()) <= fc.TOLERANCE_CAP
    print(_set_id(key), {k: '%.1e' % v for k, v in o['tol'].items()}, 'kink %.1e' % fig['kink'], 'rounds %d' % fig['rounds'])


def test_special_threshold_samples_all_occur():
    seen = set()
    for key in SETS:
        if key.box <= 12:
            seen |= set(fc.inputs(_cases_of(key)[0])['TH_sam'].ravel())
    assert set(fc._f32(fc.SPECIAL_TH)) <= seen


@pytest.mark.parametrize('key', [k for k in SETS if k.box in (2, 5, 6, 12) and k.ncon == 40 or k.box == 2][:8], ids=_set_id)
def test_oracle_vs_ff_torch_and_autograd(key):
    """The numpy oracle against the torch restatement of the model script on the DENSE arrays (the scatter of the lists), and
    its directly written dsig against autograd with an RF_l, RF_d of its own per (sample, unit)."""
    c = _cases_of(key)[0]
    x, o = fc.inputs(c), fc.oracle(c)
    v = {k: torch.tensor(q, dtype=of.DT) for k, q in x['val'].items()}
    t = {k: torch.as_tensor(x[k], dtype=of.DT) for k in ('RF_w', 'FF_con', 'FF_str', 'TH_sam', 'stim')}
    pos = of.grid_positions(c.box)
    want = of.ff_output(v['RF_l'], v['RF_d'], v['TH'], v['TH_d'], v['J'], v['a'], t['RF_w'], t['FF_con'], t['FF_str'], t['TH_sam'], pos, t['stim'])
    np.testing.assert_allclose(o['out'], want.numpy(), rtol=1e-11, atol=1e-13)
    assert np.array_equal(o['out'] > 0, want.numpy() > 0)
    # dsig of the drive itself (TH far below: every output on), fed the oracle's own q, den
    gq = x['gq'][0]
    sp = fc.second_pass(o, gq[None], o['q'], np.broadcast_to(o['den'][:, :, None], o['q'].shape))
    for h in range(c.nhid):
        rl = (v['RF_l'] * torch.ones(c.nsam, 1, 1, dtype=of.DT)).requires_grad_(True)
        rd = (v['RF_d'] * torch.ones(c.nsam, 1, 1, dtype=of.DT)).requires_grad_(True)
        q = of.ff_output(rl, rd, torch.tensor(-1e3, dtype=of.DT), v['TH_d'], v['J'], v['a'], t['RF_w'], t['FF_con'][:, h:h + 1],
                         t['FF_str'][:, h:h + 1], t['TH_sam'][:, h:h + 1], pos, t['stim'])
        gl, gd = torch.autograd.grad((torch.as_tensor(gq[:, :, h:h + 1]) * q).sum(), [rl, rd])
        got = sp['dsig'][0][:, h]
        np.testing.assert_allclose(got[:, 0], gl.numpy().ravel(), rtol=1e-9, atol=1e-12 * np.abs(sp['scale']).max())
        np.testing.assert_allclose(got[:, 1], gd.numpy().ravel(), rtol=1e-9, atol=1e-12 * np.abs(sp['scale']).max())


@pytest.mark.parametrize('key', SETS, ids=_set_id)
def test_one_wrong_grid_point_exceeds_the_tolerance(key):
    """Every named point left out, reading its streams at g + 1, or placed at its neighbour's coordinates moves a checked element
    of the forward (den, q, out) and -- where the set runs a second pass -- of dsig by at least SENSITIVITY tolerances."""
    cases = _cases_of(key)
    c = cases[0]
    x, o = fc.inputs(c), fc.oracle(c)
    # (without a connection, and with the single grid point of box 1 where w - q = 0, dsig is zero whatever the point does)
    backward = any(k.entry.startswith('backward') for k in cases) and c.ncon > 0 and c.box > 1
    forward = any(k.entry.startswith('forward') for k in cases)
    least = {}
    for name, (g, _) in x['named'].items():
        for kind in fc.DEFECTS:
            if c.box == 1 and kind != 'dropped':
                continue                                   # (a single grid point has no neighbour)
            e = fc.errors(o, fc.defect(c, g, kind))
            fwd = max(float(e[k].max()) / o['tol'][k] for k in ('den', 'q', 'out') if o['tol'][k] > 0)
            if forward:
                assert fwd >= fc.SENSITIVITY, (name, kind, fwd)
                least['forward'] = min(least.get('forward', np.inf), fwd)
            if backward:
                bwd = float(e['dsig'].max()) / o['tol']['dsig']
                assert bwd >= fc.SENSITIVITY, (name, kind, bwd)
                least['backward'] = min(least.get('backward', np.inf), bwd)
    print(_set_id(key), {k: '%.0f' % v for k, v in least.items()})


def _script_inputs_share(box, seed=0):
    """Under the inputs of tests/test_ff_gpu.py (RF_l = 2, RF_d = 0.3, stimuli {-1, 0, 1}^3, RF_w ~ U(0, 1)): the largest share
    over the stimuli of a stimulus's denominator that the first / the last grid point / the last 16-byte group holds."""
    rs = np.random.RandomState(seed)
    pos, stim = of.grid_positions(box).numpy(), of.default_stimuli().numpy()
    sig = rs.rand(box ** 3) * 0.3 + 2.0
    e = np.exp(-((pos[None] - stim[:, None]) ** 2).sum(-1) / (2 * sig ** 2))
    sh = e / e.sum(axis=1, keepdims=True)
    return float(sh[:, 0].max()), float(sh[:, -1].max()), float(sh[:, -4:].sum(axis=1).max())


def test_the_gap_one_grid_point_is_below_the_old_tolerances():
    """What tests/test_ff_gpu.py cannot see: at box 40 the first and the last grid point hold about 1.2e-5 of a denominator and
    a whole 16-byte group 5e-5 -- below rtol 2e-5 on den (sparse against dense) and rtol 2e-4 on the outputs --, at box 12 the
    last point 4.3e-4 at the most.  On the inputs of this module the same point holds at least SHARE_MIN."""
    first, last, group = _script_inputs_share(40)
    assert 0.8e-5 < last < 1.6e-5 and 0.8e-5 < first < 1.6e-5 and group < 6e-5 < 2e-4
    assert last < 2e-5
    _, last12, _ = _script_inputs_share(12)
    assert 2e-4 < last12 < 5e-4
    c = next(k for k in fc.CASES if k.box == 40 and k.stim == 'free')
    assert fc.shares(c)['last'][0] >= fc.SHARE_MIN > 1000 * last


def test_the_gap_the_old_inputs_never_use_the_exponent():
    """Every FF test ran a = exp(As) = 1 (ff_model.START_PARAMS, never overridden in tests/test_ff_gpu.py), and drew TH_sam from
    uniform(-1, 1): |TH_sam|^a could ignore a.  Here a = 0.5, 1, 2.5 and TH_sam holds 0, +-1, +-1e-6."""
    model = open(os.path.join(ROOT, 'tc_gan_amd', 'ff_model.py')).read()
    assert re.search(r'START_PARAMS = dict\(.*\n? *As=np\.log\(1\.\)\)', model)
    old = open(os.path.join(ROOT, 'tests', 'test_ff_gpu.py')).read()
    assert 'As=' not in old and "'As':" not in old and 'rng.uniform(-1, 1' in model.replace('rs.', 'rng.')
    c = next(k for k in fc.CASES if k.a == 2.5 and k.box == 12)
    x, o = fc.inputs(c), fc.oracle(c)
    ts = x['TH_sam']
    with_a1 = x['val']['TH'] + np.sign(ts) * np.abs(ts) * x['val']['TH_d']
    moved = np.abs(with_a1 - o['thr']).max() / o['S'].max()
    assert moved > 1000 * o['tol']['out']


def test_the_gap_five_totals_hide_a_misplaced_dsig():
    """dsig written to the wrong (sample, unit) leaves the five parameter gradients unchanged: they are sums over (s, h)."""
    c = next(k for k in fc.CASES if k.entry == 'backward' and k.nhid == 3 and k.box == 12)
    o = fc.oracle(c)
    d = o['dsig'][0]
    swapped = d[::-1, ::-1]
    assert np.allclose(swapped.sum(axis=(0, 1)), d.sum(axis=(0, 1)), rtol=1e-12)
    assert fc.errors(o, dict(dsig=np.broadcast_to(swapped, o['dsig'].shape)))['dsig'].max() > 1000 * o['tol']['dsig']

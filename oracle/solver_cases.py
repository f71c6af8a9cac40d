"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The cases, inputs, fp64 results and the error measure that hold every kernel of the fixed-point solver (`ssn_solve_batch_*`:
streaming, register-stationary, the tile shapes, fp32 MFMA, fp16-split wide / alternating, two-draw) to the fp64 C oracle
ELEMENT BY ELEMENT (tests/test_solver_elementwise_gpu.py), and that tests/test_solver_cases.py checks without a GPU.

Why its own inputs: the stimulus of the other solver tests is centred on the ring, and from r = 0 the neurons at the ends of
the ring stay silent in every stimulus narrower than the ring (1e-22 ... 1e-14 after 300 steps).  Those neurons are the tail
rows and columns of every tile grid, the E / I boundary row N - 1 and the ragged last column group, and below the `atol` of
those tests they are not compared at all (tests/test_solver_cases.py::test_the_gap_* records that).  Here every neuron is
driven: ext uniform per draw, stimulus and neuron, a non-zero start state, a horizon short enough that no neuron has decayed
(every element of the end state holds >= 1e-3 of its (draw, stimulus) maximum), with asym_tanh the last draw driven into the
saturating branch, and the error of every element measured against that element alone -- no absolute term.
"""
import collections
import ctypes

import numpy as np

from . import ssn_numpy as on

P = on.DEFAULT_PARAMS
B = 3                       # an odd number of draws: the two-draw kernel is left with a lone one
DT = 8e-4
HORIZONS = (24, 7)          # an even and an odd number of steps: both parities of the two state buffers
T = max(HORIZONS)
SOFT, HARD = 200.0, 1000.0
RTOL = {'float32': 1e-4, 'float64': 1e-9}       # the project's RTOL32 (BASELINE's north star) and RTOL64

Case = collections.namedtuple('Case', 'dtype io_type M NB shared')

# ---------------------------------------------------------------------------------------------------------------- the cases
# fp32.  Tile grids (columns per column group C = 4, 8, 13, 19, 25, 26; ssn_tile.hip::launch_tile_nb):
#   30  a partly filled C = 4           58  C = 8 (odd N)                66  partly filled C = 13      104  top of C = 13
#   106 C = 19, split shape with 2 waves (no mixed kernel)              130  C = 19 mixed, last wave with 4 rows per lane
#   146, 152 C = 19 mixed with 5 rows per lane (152: top)               154  C = 25, split shape with 3 waves
#   198 C = 25 mixed, ragged last column group (and the half-real tail tile of the two-draw kernel)
#   200 top of C = 25                   202  C = 26, all-register only (odd N)                         208  top of the ladder
#   210 first size beyond the ladder (every variant but 0 refuses)      258, 402  streaming only
# The same sizes walk the register-stationary ladder (16 KCH >= 2N, KCH = 2, 4, 7, 10, 13) and the matrix-core ones (fp32
# MFMA: 104, 152, 200, 208; fp16-split and two-draw: 104, 152, 208).
# Stimuli: 1, 2, 3, 5 reach the tile / register-stationary templates 1, 2, 4 (5 = 4 + 1 at C <= 19, 2 + 2 + 1 above);
# 4, 5, 8, 9, 11 are the groupings of variants 5-8 (two groups of four per workgroup): second group absent, ragged, full,
# a lone stimulus in a second workgroup, a ragged first group in a second workgroup.  Every NB runs every variant that takes it.
_SIZES32 = [(30, (1, 2, 3, 5, 4, 11)), (58, (1, 2, 5, 9)), (66, (1, 3, 5, 8)), (104, (1, 2, 3, 5, 4, 8, 9, 11)),
            (106, (1, 2, 3, 5, 4, 9)), (130, (1, 3, 5, 11)), (146, (2, 5, 8)), (152, (1, 2, 3, 5, 4, 8, 9, 11)),
            (154, (1, 2, 3, 5, 4, 8, 9, 11)), (198, (1, 2, 3, 5, 4, 8, 9, 11)), (200, (1, 3, 8, 9)),
            (202, (1, 2, 3, 5, 4, 8, 9, 11)), (208, (2, 5, 4, 8, 11)), (210, (1, 3, 5, 4)), (258, (2, 8)), (402, (1, 5))]
# fp64 (variants 0, 1, 2): 20; 60 (C = 8); 104 top of the 7-row shapes; 106, 152 C = 19 with 4 rows per lane; 154, 204 C = 26 with one row
# of every lane's tile in LDS (204 is the reference's default N = 102); 210 streaming only
_SIZES64 = [(M, (1, 3, 5)) for M in (20, 60, 104, 106, 152, 154, 204, 210)]
_LINEAR32 = [(30, 5), (58, 5), (104, 5), (152, 5), (198, 5), (202, 5), (210, 5)]          # asym_linear: one size per grid
_LINEAR64 = [(20, 3), (104, 3), (152, 3), (204, 3)]
_SHARED32 = [(30, 5), (58, 9), (104, 8), (152, 5), (198, 9), (202, 5)]                    # stimuli shared by the draws, (NB, 2N)
_SHARED64 = [(20, 3), (152, 3), (204, 3)]

CASES = ([Case('float32', io, M, NB, False) for M, nbs in _SIZES32 for NB in nbs for io in ('asym_tanh', 'asym_power')]
         + [Case('float32', 'asym_linear', M, NB, False) for M, NB in _LINEAR32]
         + [Case('float32', 'asym_tanh', M, NB, True) for M, NB in _SHARED32]
         + [Case('float64', io, M, NB, False) for M, nbs in _SIZES64 for NB in nbs for io in ('asym_tanh', 'asym_power')]
         + [Case('float64', 'asym_linear', M, NB, False) for M, NB in _LINEAR64]
         + [Case('float64', 'asym_tanh', M, NB, True) for M, NB in _SHARED64])


def case_id(c):
    return '%s-%s-M%d-NB%d%s' % (c.dtype, c.io_type, c.M, c.NB, '-shared' if c.shared else '')


# ------------------------------------------------------------------------------------- which kernel a (case, variant) runs
VARIANTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, None)
REFUSAL = 'requested kernel variant has no instantiation for this size'       # ssn_capi.hip::solve_batch_impl


def _ladder(need, ladder):
    return next((x for x in ladder if need <= x), 0)


def tile_c(c):
    return _ladder((c.M + 7) // 8, (4, 8, 13, 19, 25, 26) if c.dtype == 'float32' else (4, 8, 13, 19, 26))


def regw_kch(c):
    return _ladder((c.M + 15) // 16, (2, 4, 7, 10, 13) if c.dtype == 'float32' else (2, 4, 7))


def mfma_mk(c, variant):
    return _ladder(c.M, (104, 152, 200, 208) if variant == 5 else (104, 152, 208))


def supported(c, variant):
    """Whether `ssn_solve_batch_*_variant` takes the shape (include/ssnode_mi355x.h; None is the library's own choice)."""
    if variant in (None, 0):
        return True
    if variant == 1:
        return regw_kch(c) != 0
    if variant in (2, 3, 4):
        return tile_c(c) != 0
    fp32 = c.dtype == 'float32' and c.NB >= 4 and c.M <= 208
    return fp32 if variant == 5 else fp32 and c.io_type == 'asym_tanh'


def variants(c):
    """The variants a case is run with: all that its dtype has, refusals included (the fp16-split ones with asym_tanh only:
    tests/test_solver_gpu.py holds their refusal of the unbounded functions)."""
    if c.dtype == 'float64':
        return (0, 1, 2, None)
    return tuple(v for v in VARIANTS if v not in (6, 7, 8) or c.io_type == 'asym_tanh')


def grouping(NB):
    """How variants 5-8 lay NB stimuli out, two groups of four per workgroup."""
    last = NB % 8
    kind = 'full' if last == 0 else 'group two absent' if last == 4 else 'group two ragged' if last > 4 else 'group one ragged'
    return kind if NB <= 8 else 'second workgroup, ' + ('one stimulus' if last == 1 else kind)


def kernel_of(c, variant):
    """(family, grid, shape) of the kernel a supported (case, variant) launches -- the launchers restated:
    ssn_capi.hip::solve_batch_impl, ssn_tile.hip::launch_tile_nb, ssn_solver.hip::launch_regw_nb, ssn_mfma*.hip, ssn_duo.hip.
    family: 'stream', 'regw', 'tile split', 'tile mixed', 'tile mixed6', 'tile all-register', 'mfma', 'wide', 'alternating',
    'duo' (fp64: 'fp64 stream', 'fp64 regw', 'fp64 tile'); grid: the step of the family's size ladder; shape: the stimuli per
    workgroup the template is instantiated for (tile, register-stationary), the rows per lane of the last wave (mixed), the
    rows of the four waves (mixed6) or the grouping of the stimuli (variants 5-8)."""
    assert supported(c, variant)
    fp32 = c.dtype == 'float32'
    if variant is None:                    # B = 3 is far from filling the chip: tile, register-stationary, streaming
        variant = 2 if tile_c(c) else 1 if regw_kch(c) else 0
    if variant == 0:
        return ('stream' if fp32 else 'fp64 stream'), ('2N <= 208' if c.M <= 208 else '2N > 208'), 1
    if variant == 1:
        k = regw_kch(c)
        nbt = (8 if c.NB >= 8 else 4 if c.NB >= 4 else 2 if c.NB >= 2 else 1) if fp32 else (2 if k < 7 and c.NB >= 2 else 1)
        return ('regw' if fp32 else 'fp64 regw'), k, nbt
    if variant in (2, 3, 4):
        C = tile_c(c)
        if not fp32:
            return 'fp64 tile', C, 1
        waves = (c.M + 55) // 56
        last_rows = c.M - 56 * (waves - 1)
        if variant != 4 and C in (19, 25):               # variants 2 and 3 are the same choice: split where instantiated
            if C == 25 and c.NB == 1 and c.M >= 170:     # (ssn_tile.hip: TILE_MIXED6_MIN_M)
                return 'tile mixed6', C, 'rows 56/48/48/48'
            if (C == 25 and waves == 4 and last_rows <= 32) or (C == 19 and waves == 3 and last_rows <= 40):
                return 'tile mixed', C, 'last wave %d rows per lane' % (4 if last_rows <= 32 else 5)
            return 'tile split', C, 1
        return 'tile all-register', C, 4 if C <= 19 and c.NB >= 4 else 2 if c.NB >= 2 else 1
    return {5: 'mfma', 6: 'wide', 7: 'alternating', 8: 'duo'}[variant], mfma_mk(c, variant), grouping(c.NB)


def ran(c, variant):
    """The two records a (case, variant) that ran to the end leaves for `coverage`."""
    k = kernel_of(c, variant)
    return [k, ('variant', c.dtype, variant, k[1])]


GROUPINGS = tuple(grouping(NB) for NB in (4, 5, 8, 9, 11))


def coverage():
    """What tests/test_solver_elementwise_gpu.py must have seen run to the end: every variant on every step of its size
    ladder, and every template instantiation and stimulus grouping of every kernel family."""
    C32, C64, KCH32, KCH64 = (4, 8, 13, 19, 25, 26), (4, 8, 13, 19, 26), (2, 4, 7, 10, 13), (2, 4, 7)
    both = ('2N <= 208', '2N > 208')
    need = [('variant', 'float32', v, C) for v in (2, 3, 4, None) for C in C32] + [('variant', 'float32', None, '2N > 208')]
    need += [('variant', 'float32', 1, k) for k in KCH32] + [('variant', 'float32', 0, g) for g in both]
    need += [('variant', 'float32', 5, mk) for mk in (104, 152, 200, 208)]
    need += [('variant', 'float32', v, mk) for v in (6, 7, 8) for mk in (104, 152, 208)]
    need += [('variant', 'float64', v, C) for v in (2, None) for C in C64] + [('variant', 'float64', None, '2N > 208')]
    need += [('variant', 'float64', 1, k) for k in KCH64] + [('variant', 'float64', 0, g) for g in both]
    need += [('stream', g, 1) for g in both] + [('fp64 stream', g, 1) for g in both]
    need += [('regw', k, nbt) for k in KCH32 for nbt in (1, 2, 4, 8)]
    need += [('fp64 regw', k, nbt) for k in KCH64 for nbt in ((1, 2) if k < 7 else (1,))]
    need += [('tile all-register', C, nbt) for C in C32 for nbt in ((1, 2, 4) if C <= 19 else (1, 2))]
    need += [('tile split', 19, 1), ('tile split', 25, 1), ('tile mixed', 19, 'last wave 4 rows per lane'),
             ('tile mixed', 19, 'last wave 5 rows per lane'), ('tile mixed', 25, 'last wave 4 rows per lane'),
             ('tile mixed6', 25, 'rows 56/48/48/48')]
    need += [('fp64 tile', C, 1) for C in C64]
    need += [('mfma', mk, g) for mk in (104, 152, 200, 208) for g in GROUPINGS]
    need += [(f, mk, g) for f in ('wide', 'alternating', 'duo') for mk in (104, 152, 208) for g in GROUPINGS]
    return need


# ------------------------------------------------------------------------------------------------------------------- inputs
def _rounded(a, dtype):
    return np.asarray(a, dtype='float64').astype(dtype).astype('float64')


def scale(c):
    """ext and r0 shrink beyond 2N = 104: the larger nets amplify transients, and at scale 1 the Euler loop run in float32
    on the CPU is itself 6.8e-5 (2N = 210) ... 0.3 (2N = 402) off the fp64 one."""
    return 1.0 if c.M <= 104 else 0.25


def saturated_draws(c):
    """(B,) bool: the draws whose stimuli reach the saturating branch of f -- the last one of the asym_tanh cases with stimuli
    per draw, up to 2N = 258 (at 2N = 402 the float32 CPU run of such a draw is 3.4e-4 off by itself)."""
    return np.arange(B) == (B - 1 if c.io_type == 'asym_tanh' and not c.shared and c.M <= 258 else -1)


SATURATED_EXT = (30.0, 80.0)
# Seed offsets of the cases whose first draw of inputs misses one of the conditions that tests/test_solver_cases.py asserts for
# every case -- or comes within a factor two of missing: the float32 run depends on the order in which a CPU's einsum adds.
# A case that misses gets another seed here; it is never dropped.
RESEED = {'float32-asym_tanh-M30-NB3': 1, 'float32-asym_tanh-M152-NB5': 1, 'float32-asym_tanh-M152-NB11': 1,
          'float32-asym_tanh-M154-NB4': 1, 'float32-asym_power-M154-NB9': 1, 'float32-asym_tanh-M198-NB4': 1,
          'float32-asym_power-M198-NB8': 1, 'float32-asym_tanh-M200-NB3': 3, 'float32-asym_power-M202-NB3': 1,
          'float32-asym_tanh-M202-NB8': 1, 'float32-asym_tanh-M208-NB2': 1, 'float32-asym_tanh-M208-NB8': 1,
          'float32-asym_tanh-M208-NB11': 3, 'float32-asym_power-M210-NB5': 1, 'float32-asym_tanh-M258-NB2': 1,
          'float32-asym_power-M402-NB5': 2, 'float32-asym_tanh-M152-NB5-shared': 1, 'float64-asym_tanh-M20-NB1': 4,
          'float64-asym_tanh-M20-NB3': 2, 'float64-asym_tanh-M20-NB5': 2, 'float64-asym_tanh-M152-NB5': 1,
          'float64-asym_power-M210-NB5': 1,
          # (a defect of tests/test_solver_cases.py::test_defects_are_seen that moves the row it concerns less than 100 x tol)
          'float32-asym_power-M58-NB9': 1, 'float32-asym_tanh-M66-NB3': 1, 'float32-asym_power-M66-NB8': 1,
          'float32-asym_tanh-M146-NB2': 1, 'float32-asym_tanh-M402-NB1': 1, 'float64-asym_tanh-M60-NB1': 2}
_INPUTS, _ORACLE, _TRAJ = {}, {}, {}


def inputs(c):
    """fp64 arrays that are exactly representable in the case's dtype: W = generate_weight(N, new_JDS, z) (B, M, M),
    ext (B, NB, M) -- or (NB, M) for a shared case -- and r0 (B, NB, M)."""
    if c in _INPUTS:
        return _INPUTS[c]
    _INPUTS.clear()                         # (one case at a time: the tests walk the cases in order)
    rs = np.random.RandomState(1000003 * RESEED.get(case_id(c), 0) + 1000 * c.M + 10 * c.NB + 3 * on.IO_CODES[c.io_type] + c.shared)
    N, s = c.M // 2, scale(c)
    jds = on.new_JDS()
    W = np.stack([on.generate_weight(N, jds['J'], jds['D'], jds['S'], z) for z in rs.rand(B, c.M, c.M)])
    ext = rs.uniform(2.0, 20.0, (B, c.NB, c.M)) * s
    r0 = rs.uniform(0.05, 20.0, (B, c.NB, c.M))
    sat = saturated_draws(c)
    r0[~sat] *= s                           # (the saturated draw starts from the unscaled state at every size)
    ext[sat] = rs.uniform(*SATURATED_EXT, size=(int(sat.sum()), c.NB, c.M))
    if c.shared:
        ext = ext[0]
    res = _INPUTS[c] = dict(W=_rounded(W, c.dtype), ext=_rounded(ext, c.dtype), r0=_rounded(r0, c.dtype))
    return res


def ext_per_draw(c, x=None):
    """The stimuli as (B, NB, M) whatever form the case passes them in."""
    ext = (x or inputs(c))['ext']
    return np.broadcast_to(ext, (B, c.NB, c.M)) if ext.ndim == 2 else ext


# ------------------------------------------------------------------------------------------------------------------ oracles
def step_factors(M, dtype='float64'):
    """dt / tau per neuron (E: i < N, I: the rest), computed in fp64 like the C oracle and the library's host code."""
    tau = np.where(np.arange(M) < M // 2, P['tau'][0], P['tau'][1])
    return (DT / tau).astype(dtype)


def io_fun(v, io_type, dtype='float64'):
    """`ssn_numpy.io_fun` with the default constants, evaluated in `dtype`."""
    dt = np.dtype(dtype).type
    k, n, r0, r1 = dt(P['k']), dt(P['n']), dt(SOFT), dt(HARD)
    v0 = dt(on.rate_to_volt(SOFT, P['k'], P['n']))
    if io_type == 'asym_power':
        return k * np.power(np.maximum(v, dt(0)), n)
    r_pow = k * np.power(np.clip(v, dt(0), v0), n)
    if io_type == 'asym_linear':
        return np.where(v <= v0, r_pow, r_pow + k * np.power(v0, n - dt(1)) * n * (v - v0))
    return np.where(v <= v0, r_pow, r0 + (r1 - r0) * np.tanh(n * r0 / (r1 - r0) * (v - v0) / v0))


def euler(W, ext, r0, io_type, steps=T, dtype='float64', eps=None, ext_of=None):
    """The Euler loop of ssnode.c restated in numpy, in fp64 or float32: the WHOLE trajectory (steps + 1, B, NB, M) from
    r0 on.  W (B, M, M), ext and r0 (B, NB, M).  `eps` replaces the per-neuron dt / tau (the defect runs of
    tests/test_solver_cases.py)."""
    W, ext, r = (np.asarray(a, dtype=dtype) for a in (W, ext, r0))
    eps = step_factors(W.shape[-1], dtype) if eps is None else np.asarray(eps, dtype=dtype)
    traj = np.empty((steps + 1,) + r.shape, dtype=dtype)
    traj[0] = r
    for t in range(steps):
        v = np.einsum('bij,bsj->bsi', W, r) + ext
        r = r + (-r + io_fun(v, io_type, dtype)) * eps
        assert r.dtype == np.dtype(dtype)
        traj[t + 1] = r
    return traj


def trajectory(c, dtype='float64'):
    """`euler` on a case's inputs, as fp64 arrays whatever `dtype` it ran in (the last case per dtype is cached)."""
    if _TRAJ.get(dtype, (None,))[0] != c:
        x = inputs(c)
        _TRAJ[dtype] = (c, euler(x['W'], ext_per_draw(c, x), x['r0'], c.io_type, dtype=dtype).astype('float64'))
    return _TRAJ[dtype][1]


def c_oracle(c, steps):
    """`oracle_solve_batch` (fp64 C) on a case's inputs for a fixed number of steps, atol = 0 and no rate stop: x, x_prev
    (the state one step earlier), codes, steps."""
    lib = on.load_oracle_lib()
    x = inputs(c)
    ext = ext_per_draw(c, x)
    r = np.ascontiguousarray(x['r0']).copy()
    scratch = np.full_like(r, np.nan)
    codes = np.full((B, c.NB), -1, dtype=np.int32)
    nsteps = np.full((B, c.NB), -1, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    hard = HARD if c.io_type == 'asym_tanh' else np.inf
    for b in range(B):                      # (the C driver shares the stimuli among its draws: one call per draw)
        lib.oracle_solve_batch(on.IO_CODES[c.io_type], 1, c.NB, c.M // 2, on.ptr(np.ascontiguousarray(x['W'][b])),
                               on.ptr(np.ascontiguousarray(ext[b])), P['k'], P['n'], on.ptr(r[b]), on.ptr(scratch[b]),
                               P['tau'][0], P['tau'][1], DT, steps, 0.0, SOFT, hard, codes[b].ctypes.data_as(ip),
                               nsteps[b].ctypes.data_as(ip))
    # code 1: the two buffers have changed roles `steps` times, so the newest state is in "r1" after an odd number of steps
    newest, prev = (scratch, r) if steps % 2 else (r, scratch)
    return newest, prev, codes, nsteps


def oracle(c):
    """{steps: (x, x_prev, codes, steps)} of the C oracle for every horizon (the last case is cached)."""
    if _ORACLE.get('case') != c:
        _ORACLE.clear()
        _ORACLE.update(case=c, res={k: c_oracle(c, k) for k in HORIZONS})
    return _ORACLE['res']


# ------------------------------------------------------------------------------------------------------------------ measure
def rel_err(got, want):
    """|got - want| / |want| element by element -- no absolute term, no element left out (the oracle is positive everywhere:
    tests/test_solver_cases.py)."""
    assert (want > 0).all()
    return np.abs(np.asarray(got, dtype='float64') - want) / want


def per_draw_max(err):
    """Largest figure per draw of an array (B, ...) or (steps, B, ...)."""
    return err.reshape(B, -1).max(axis=1)

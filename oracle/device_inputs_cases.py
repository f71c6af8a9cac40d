"""ORACLE -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The cases that hold the one-launch inputs of a device-noise forward (`ssn_gen_inputs_philox_f32`, `gen_inputs_kernel` of
tc_gan_amd/csrc/ssn_aux.hip) to the Philox restatement (`philox_numpy.device_inputs_noise`) and to the separately pinned
kernels, bit for bit (tests/test_device_inputs_gpu.py), and whose sensitivity tests/test_philox_inputs.py checks without a GPU.

The kernel cuts one grid in three ranges of workgroups: W (and z) in vectors of four elements that may straddle two Philox
blocks, the stimulus with 1 + v z formed again from the stream element of its (draw, neuron), and zin / amp one Philox block per
thread.  Each range strides once it reaches its cap of workgroups.  The 64-bit stream position is split into the two low counter
words in three different places, and the high word first changes at element 2^34 (block 2^32).
"""
import collections

import numpy as np

from . import philox_numpy as ph

SEED = (7 << 32) | 35                    # both key words non-zero; chosen with GEN_SEED so that every 'uniform' case tells
                                         # one rounding of 1 + v z from two (tests/test_philox_inputs.py)
SMOOTHNESS = 0.25 / 8                    # ssn_numpy.DEFAULT_PARAMS['smoothness']
E34 = 1 << 34                            # the first stream element whose block has a non-zero high counter word

# (N, B, NB): the smallest shapes at which each path can go wrong
Row = collections.namedtuple('Row', 'N B NB')
ROWS = [
    Row(3, 2, 1),           # 2N % 4 == 2: a vector of four runs over the end of a row
    Row(10, 3, 5),          # odd B, ragged NB; every alignment of the two offsets
    Row(101, 2, 8),         # 2N = 202, the paper's size, 2N % 4 == 2
    Row(100, 2, 8),         # 2N = 200, the benchmark's size
    Row(100, 108, 27),      # B (2N)^2 = 4 320 000 > 4 194 304 = 4 * 256 * 4096: the W range is capped at 4096 workgroups and
                            # strides; B NB 2N = 583 200 > 524 288 = 256 * 2048: the stimulus range is capped at 2048 and strides
]
MODES = ('plain', 'bernoulli', 'uniform')          # v = NULL; v with signs; v with 2 u - 1


def row_id(r):
    return 'N%d-B%d-NB%d' % r


def offsets(row):
    """The (off_z, off_zin) pairs of a row.  Low: all 16 combinations of off_z % 4 x off_zin % 4 for N = 10, four of them (each
    residue once on either side) for the others.  High (N = 10 and N = 101): the W range straddling element 2^34 at every
    off_z % 4 -- with a misalignment one thread's second block is block 2^32 -- together with off_zin = 2^34 - 5 (the amp range
    and the per-element counters of the stimulus range straddle it too), and both offsets at 3 * 2^34 + 7."""
    z0, zin0 = 4 * 17, 4 * 100000
    if row.N == 10:
        out = [(z0 + a, zin0 + b) for a in range(4) for b in range(4)]
    else:
        out = [(z0 + a, zin0 + b) for a, b in ((0, 0), (1, 2), (2, 3), (3, 1))]
    if row.N in (10, 101):
        half = (row.B * (2 * row.N) ** 2 // 2) // 4 * 4
        out += [(E34 - half + a, E34 - 5) for a in range(4)]
        out += [(3 * E34 + 7, 3 * E34 + 7)]
    return out


def v_of(row):
    return np.linspace(0.05, 0.9, 2 * row.N).astype(np.float32)


def stimuli(row, B=None):
    """bw uniform in [0, 1], con drawn from {5, 20} per (draw, stimulus); float32 [B][NB]."""
    B = row.B if B is None else B
    rs = np.random.RandomState(1000 * row.N + row.NB)
    bw = rs.rand(B, row.NB).astype(np.float32)
    con = rs.choice([5.0, 20.0], size=(B, row.NB)).astype(np.float32)
    return bw, con


_Z, _ZIN = {}, {}
_LARGE = 1 << 20


def noise(row, mode, off_z, off_zin, B=None):
    """`philox_numpy.device_inputs_noise` of a case: (z, zin, amp), zin = amp = None for 'plain'.  Computed once and never
    written to; of the draws above a million elements (17 MB for the large row) only the last one is kept."""
    B = row.B if B is None else B
    M = 2 * row.N
    zkey = (row.N, B, off_z)
    if zkey not in _Z:
        if B * M * M > _LARGE:
            for k in [k for k in _Z if k[1] * (2 * k[0]) ** 2 > _LARGE]:
                del _Z[k]
        _Z[zkey] = ph.uniform_vec(SEED, off_z, B * M * M).reshape(B, M, M)
        _Z[zkey].setflags(write=False)
    if mode == 'plain':
        return _Z[zkey], None, None
    akey = (row.N, B, off_zin, mode)
    if akey not in _ZIN:
        _ZIN[akey] = ph.signs_and_amp(SEED, off_zin, v_of(row), mode == 'bernoulli', B, M)
        for a in _ZIN[akey]:
            a.setflags(write=False)
    return (_Z[zkey],) + _ZIN[akey]


# The Python dispatch (`TuningCurveGenerator` with `z_device_seed`): 10 sites, 5 stimuli, 3 models, a short run.  A forward
# draws z (B * 2N * 2N elements) and then zin (B * 2N) from the generator's stream: position 0, a position that puts the z draw
# across element 2^34 (at an odd alignment), and one that puts the zin draw across it.
GEN_SITES, GEN_MODELS, GEN_STIMULI = 10, 3, 5
GEN_SEED = 24
GEN_V = {'default': None, 'heteroin': [0.35, 0.15], 'deg-heteroin': 0.45}
_GEN_Z = GEN_MODELS * (2 * GEN_SITES) ** 2
GEN_POSITIONS = [0, E34 - _GEN_Z // 2 - 1, E34 - _GEN_Z - GEN_MODELS * GEN_SITES + 1]


def gen_v_per_neuron(ssn_type):
    """V of a heterogeneous-input generator per neuron (first N neurons V_E, the others V_I; one value for both: 'deg-heteroin')."""
    return np.repeat(np.broadcast_to(np.asarray(GEN_V[ssn_type], dtype='float64'), 2), GEN_SITES).astype(np.float32)

"""The sliced Wasserstein match per condition cell (csrc/ssn_swd_cells.hip in libssnode_ext2.so,
networks/conditional_sliced_wasserstein.py, run/bptt_cswd.py), the parts that need no GPU: the restatement the GPU tests compare
with (tests/swd_cells_cases.py) against exact rationals, fp64 autograd, the one-cell case and a lattice; how far three deliberate
errors move what is checked; the second companion library's exports, refusals and build; the generated code's metadata; the
command line; the cell-id map and the trainer's refusals by name."""
import ctypes
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
import swd_cells_cases as cc
import swd_sizes_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')

#: cell sizes of one call: empty cells first, in the middle and last; one row; around the padding of 64
SIZES = [(5,), (0, 3, 0, 7, 0), (1, 2, 63, 64, 65, 0), (0, 9, 1)]


# ---- 1. the restatement against other statements of the same loss --------------------------------------------------------

@pytest.mark.parametrize('power', [1, 2])
def test_kernel_order_stays_within_the_bound_of_the_exact_rational_per_cell(power):
    worst = Fraction(0)
    for k, sizes in enumerate(SIZES):
        for m in (1, 7, 65):
            x, cells, y, theta = cc.generic_inputs(np.random.RandomState(10 * k + m), sizes, m, 3, 6)
            want = cc.swd_cells(x, cells, y, theta, power)
            ordered = cc.loss_cl_in_kernel_order(want['px'], want['cell_rows'], want['cell_start'], want['py'], power)
            for c, n in enumerate(sizes):
                for l in range(3):
                    exact = want['loss_cl'][c][l]
                    err = abs(Fraction(float(ordered[c, l])) - exact)
                    assert err <= zc.loss_bound(exact, n, m), (sizes, m, c, l)
                    if exact:
                        worst = max(worst, err / zc.loss_bound(exact, n, m))
                if n == 0:
                    assert (ordered[c] == 0).all() and not np.signbit(ordered[c]).any()
            # every row has one cell and one coefficient per direction; the tied direction has none
            assert (want['coef'][:, 1] == 0).all()
    print('largest error of the kernel order: {:.3g} of the bound'.format(float(worst)))
    assert worst > 0


@pytest.mark.parametrize('power', [1, 2])
def test_restatement_equals_fp64_autograd_of_the_weighted_loss(power):
    """sum_c (n_c / B) mean_l W_p^p through torch.sort, the quantile coupling written with repeated rows.  The restatement
    rounds the projections, the coefficients and the gradient to float32 where autograd stays in fp64: the tolerances of
    tests/test_swd_sizes.py for the same three roundings -- loss to 1e-6 relative, gradient to 1e-6 of its largest entry.
    Generic rows without ties."""
    rs = np.random.RandomState(3)
    worst = 0.0
    for sizes, m in (((7, 0, 2), 3), ((12, 5, 1), 18), ((0, 15), 100), ((64, 9, 3, 1), 9)):
        D, L, C, B = 5, 8, len(sizes), sum(sizes)
        cells = cc.interleaved_cells(rs, sizes)
        x, y = rs.randn(B, D).astype('float32'), (rs.randn(C, m, D) + 0.5).astype('float32')
        theta = sc.generic_inputs(rs, 2, L, D)[2]
        theta[L // 2] = theta[0][::-1]                            # (no tied direction here)
        got = cc.swd_cells(x, cells, y, theta, power)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        tt = torch.tensor(theta, dtype=torch.float64)
        loss = 0
        for c, n in enumerate(sizes):
            if n == 0:
                continue
            g = gcd(n, m)
            px = xt[torch.as_tensor(np.nonzero(cells == c)[0])] @ tt.T
            py = torch.tensor(y[c], dtype=torch.float64) @ tt.T
            d = torch.sort(px, dim=0).values.repeat_interleave(m // g, dim=0) - \
                torch.sort(py, dim=0).values.repeat_interleave(n // g, dim=0)
            loss = loss + (n / B) * (d.abs() if power == 1 else d * d).mean()
        grad, = torch.autograd.grad(loss, xt)
        np.testing.assert_allclose(got['swd'], float(loss.detach()), rtol=1e-6)
        top = np.abs(grad.numpy()).max()
        worst = max(worst, np.abs(got['gx'] - grad.numpy()).max() / top)
        np.testing.assert_allclose(got['gx'], grad.numpy(), rtol=0, atol=1e-6 * top)
        host, _ = cc.swd_in_host_order(cc.loss_cl_in_kernel_order(got['px'], got['cell_rows'], got['cell_start'], got['py'], power),
                                       got['cell_start'])
        np.testing.assert_allclose(host, got['swd'], rtol=(B + m + L + C + 8) * 2.0 ** -52)
    print('largest gradient difference / largest entry:', worst)


@pytest.mark.parametrize('power', [1, 2])
def test_one_cell_gives_the_bits_of_the_match_of_two_sizes(power):
    for n, m, L in ((1, 1, 1), (7, 1, 2), (2, 3, 3), (65, 64, 3), (15, 1000, 2)):
        x, y, theta = zc.generic_inputs(np.random.RandomState(n + m), n, m, L, 6)
        want = zc.swd(x, y, theta, power)
        got = cc.swd_cells(x, np.zeros(n, dtype=int), y[None], theta, power)
        np.testing.assert_array_equal(got['cell_rows'], np.arange(n))
        np.testing.assert_array_equal(got['coef'].view(np.uint32), want['coef'].view(np.uint32))
        assert got['loss_cl'] == [want['loss_l']]
        np.testing.assert_array_equal(got['gx'].view(np.uint32), want['gx'].view(np.uint32))


@pytest.mark.parametrize('power', [1, 2])
def test_lattice_values_are_exact(power):
    """Every operation of the kernel order is exact on the lattice: loss_cl is the rational one, the coefficients are the exact
    sums times the exact inv = 1 / (L B m), and the host's weighted mean is the exact one."""
    for sizes, m, L in (((1,), 1, 1), ((2, 0, 4, 2), 8, 2), ((64, 32, 16, 16), 16, 4), ((0, 256), 64, 2)):
        B = sum(sizes)
        x, cells, y, theta = cc.lattice_inputs(np.random.RandomState(10 + B), sizes, m, L, 6)
        got = cc.swd_cells(x, cells, y, theta, power)
        ordered = cc.loss_cl_in_kernel_order(got['px'], got['cell_rows'], got['cell_start'], got['py'], power)
        assert [[Fraction(float(v)) for v in row] for row in ordered] == got['loss_cl']
        assert Fraction(cc.swd_in_host_order(ordered, got['cell_start'])[0]) == \
            sum((Fraction(n, B * L) * sum(got['loss_cl'][c]) for c, n in enumerate(sizes)), Fraction(0))
        for c, n in enumerate(sizes):
            if n == 0:
                continue
            rows = got['cell_rows'][got['cell_start'][c]:got['cell_start'][c + 1]]
            i, j, w, _, _ = zc.coupling(n, m)
            for l in range(L):
                seg = got['px'][rows, l]
                order = np.argsort(seg + np.float32(0), kind='stable')
                d = seg[order].astype('float64')[i] - np.sort(got['py'][c][:, l]).astype('float64')[j]
                for rank in (0, n // 2, n - 1):
                    sel = i == rank
                    exact = sum(int(wk) * Fraction(float(np.sign(dk) if power == 1 else 2.0 * dk)) for wk, dk in zip(w[sel], d[sel]))
                    assert Fraction(float(got['coef'][rows[order[rank]], l])) == exact / (L * B * m)


def test_a_non_finite_value_is_nan_for_its_cell_and_direction_only():
    sizes, m, L = (3, 0, 4), 5, 2
    x, cells, y, theta = cc.generic_inputs(np.random.RandomState(8), sizes, m, L, 4)
    clean = cc.swd_cells(x, cells, y, theta, 2)
    rows2 = np.nonzero(cells == 2)[0]
    for bad in (np.nan, np.inf, -np.inf):
        for side in ('x', 'y'):
            px, py = clean['px'].copy(), clean['py'].copy()
            if side == 'x':
                px[rows2[1], 0] = bad
            else:
                py[2, 3, 0] = bad
            coef, loss_cl = cc.match_cells(px, clean['cell_rows'], clean['cell_start'], py, 2)
            assert loss_cl[2][0] is None and np.isnan(coef[rows2, 0]).all()
            assert loss_cl[0] == clean['loss_cl'][0] and loss_cl[2][1] == clean['loss_cl'][2][1] and loss_cl[1] == [0, 0]
            keep = np.ones_like(coef, dtype=bool)
            keep[rows2, 0] = False
            np.testing.assert_array_equal(coef[keep].view(np.uint32), clean['coef'][keep].view(np.uint32))


# ---- 2. sensitivity: what a wrong kernel or a wrong restatement would move -------------------------------------------------

def test_deliberate_errors_move_the_checked_quantities_far_beyond_their_tolerances():
    """The GPU tests hold coef to equality of bits (the least difference is one float32 ulp, 2^-23 relative) and loss_cl to
    `loss_bound`, at most (n_c + m + 4) 2^-52 relative (an empty cell's to +0 exactly).  Movements of the three errors, measured
    with this restatement here on the CPU: inv with n_c for B moves coef by 6.30e7 ulps of its largest entry; ties broken by
    global row, with every cell's rows arriving in descending order, by 4.02e6 ulps; an empty cell given the next cell's start
    moves that cell's loss_cl from +0 to at least 0.1015 in every direction but the tied one, 3.0e12 times the
    largest bound of any loss_cl of the case.  The smallest of the three, the tie-break's 4.02e6, is what every one is held to."""
    rs = np.random.RandomState(4)
    sizes, m, L, D = (65, 0, 9, 33), 64, 33, 6
    x, cells, y, theta = cc.generic_inputs(rs, sizes, m, L, D)
    right = cc.swd_cells(x, cells, y, theta, 2)
    ulp = 2.0 ** -23
    top = np.abs(right['coef']).max()
    moved = {}

    wrong = cc.swd_cells(x, cells, y, theta, 2, inv_per_cell=True)
    assert wrong['loss_cl'] == right['loss_cl']                   # (the loss cannot see the scale of the coefficients)
    moved['inv with n_c for B'] = np.abs(wrong['coef'] - right['coef']).max() / top / ulp

    # rows of every cell in DESCENDING order: the local index k then runs against the row index
    rows, start = right['cell_rows'].copy(), right['cell_start']
    for c in range(len(sizes)):
        rows[start[c]:start[c + 1]] = rows[start[c]:start[c + 1]][::-1]
    by_k = cc.match_cells(right['px'], rows, start, right['py'], 2)
    by_row = cc.match_cells(right['px'], rows, start, right['py'], 2, ties='row')
    assert by_k[1] == by_row[1] == right['loss_cl']
    moved['ties by global row'] = np.abs(by_row[0] - by_k[0]).max() / top / ulp
    # (with the rows ascending the two tie-breaks are the same: that is why the kernel may carry k)
    np.testing.assert_array_equal(cc.match_cells(right['px'], right['cell_rows'], start, right['py'], 2, ties='row')[0], right['coef'])

    wrong = cc.swd_cells(x, cells, y, theta, 2, empty_takes_next=True)
    assert all(v == 0 for v in right['loss_cl'][1])
    least = min(float(v) for l, v in enumerate(wrong['loss_cl'][1]) if l != L // 2)
    bound = (max(sizes) + m + 4) * 2.0 ** -52
    moved['empty cell takes the next start: loss_cl of the cell, in bounds'] = \
        least / (bound * max(float(v) for row in right['loss_cl'] for v in row))
    for what, by in moved.items():
        print(what, 'moves by', by)
    assert least >= 0.1015
    assert min(moved.values()) >= 4.0e6


# ---- 3. the second companion library ------------------------------------------------------------------------------------

def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    return sorted(set(re.findall(r'^\s*(?:int|long|size_t|double|const char \*|const char\*)\s*\*?\s*([a-z_0-9]+)\s*\(', text,
                                 flags=re.M)))


def _exported(library):
    out = subprocess.check_output(['nm', '-D', '--defined-only', os.path.join(ROOT, 'tc_gan_amd', 'ext', library)]).decode()
    return sorted(line.split()[-1].split('@')[0] for line in out.splitlines() if line.strip())


def test_second_companion_exports_its_header_and_nothing_else():
    """header == clib.EXT2_DECLARED_SYMBOLS == nm -D, with no list of names here: the next entry point is added to the header and
    to clib and this test passes as it stands."""
    from tc_gan_amd import clib
    names = _declared('ssnode_mi355x_ext2.h')
    assert sorted(clib.EXT2_DECLARED_SYMBOLS) == names == _exported('libssnode_ext2.so')
    assert len(set(clib.EXT2_DECLARED_SYMBOLS)) == len(clib.EXT2_DECLARED_SYMBOLS) >= 3
    assert all(n.startswith('ssnx2_') for n in names)
    assert not set(names) & (set(clib.DECLARED_SYMBOLS) | set(clib.EXT_DECLARED_SYMBOLS))
    assert not set(names) & (set(_exported('libssnode.so')) | set(_exported('libssnode_ext.so')))
    for name in names:                                            # every declared function has its ctypes signature
        assert getattr(clib.libssnode_ext2, name).argtypes is not None, name
    assert clib.libssnode_ext2.ssnx2_abi_version() == 1
    assert len(clib.libssnode_ext2.ssnx2_swd_match_cells_f32.argtypes) == 12
    header = open(os.path.join(ROOT, 'include', 'ssnode_mi355x_ext2.h')).read()
    opening = header.split('*/')[0]
    assert header.lstrip().startswith('/*') and 'GROW' in opening and 'no literal list of names' in opening
    assert int(re.search(r'#define SSNX2_SWD_MAX_TRUTH (\d+)', header).group(1)) == clib.SWD_MAX_TRUTH
    assert int(re.search(r'#define SSNX2_SWD_MAX_CELLS (\d+)', header).group(1)) == clib.SWD_MAX_CELLS == 256
    assert 'libssnode_ext2.map' in open(os.path.join(ROOT, '.gitignore')).read()
    assert clib.ext2_last_error.__module__ == clib.check_ext2.__module__ == 'tc_gan_amd.clib'


def _starts(*values):
    return (ctypes.c_int * len(values))(*values)


#: (B, cell_start, C, m, L, power) with null device pointers -> what ssnx2_last_error says behind the entry point's name
REFUSALS = [
    ((-1, (0, 0), 1, 8, 3, 2), 'a negative size'),
    ((8, (0, 8), -1, 8, 3, 2), 'a negative size'),
    ((8, (0, 8), 1, -8, 3, 2), 'a negative size'),
    ((8, (0, 8), 1, 8, -3, 2), 'a negative size'),
    ((8, (0, 8), 257, 8, 3, 2), 'more than 256 cells (their starts travel in the kernel arguments)'),
    ((8, (0, 8), 1, 16385, 3, 2), 'more than 16384 truth rows per cell (their values are sorted in 64 KiB of LDS)'),
    ((8, (0, 8), 1, 8, 4097, 2), 'more than 4096 directions'),
    ((8, (0, 8), 1, 8, 3, 0), 'a power other than 1 or 2'),
    ((8, (0, 8), 1, 8, 3, 3), 'a power other than 1 or 2'),
    ((0, (0, 0), 0, 0, 0, -1), 'a power other than 1 or 2'),
    ((8, None, 1, 8, 3, 2), 'invalid argument (null cell_start)'),
    ((8, (1, 8), 1, 8, 3, 2), 'cell_start does not start at 0'),
    ((8, (0, 5, 3, 8), 3, 8, 3, 2), 'cell_start decreases'),
    ((8, (0, 5, 7), 2, 8, 3, 2), 'cell_start does not end at B'),
    ((8, (0, 5, 9), 2, 8, 3, 2), 'cell_start does not end at B'),
    ((5000, (0, 4097, 5000), 2, 8, 3, 2), 'a cell of more than 4096 generated rows (their keys are sorted in 32 KiB of LDS)'),
    ((8, (0, 8), 1, 0, 3, 2), 'no truth rows (m == 0) to match the generated rows with'),
    ((8, (0, 3, 8), 2, 9, 3, 2), 'invalid argument (null pointer)'),
    ((5000, (0, 4096, 5000), 2, 8, 3, 1), 'invalid argument (null pointer)'),        # (B itself is not limited by the sort)
    ((1, (0, 1), 1, 1, 1, 1), 'invalid argument (null pointer)'),
]


@pytest.mark.parametrize('args, message', REFUSALS)
def test_the_match_refuses_from_the_arguments_alone(args, message):
    """Host checks in front of any HIP call: no device needed.  The message is the second companion library's own."""
    from tc_gan_amd import clib
    B, start, C, m, L, power = args
    before, before_ext = clib.last_error(), clib.ext_last_error()
    rc = clib.libssnode_ext2.ssnx2_swd_match_cells_f32(None, B, None, None if start is None else _starts(*start), C, None, m, L,
                                                       power, None, None, None)
    assert rc == clib.SSN_ERR_BASE + 1                                # hipErrorInvalidValue
    assert clib.ext2_last_error() == 'ssnx2_swd_match_cells_f32: ' + message
    assert clib.last_error() == before and clib.ext_last_error() == before_ext      # (the other libraries' strings are not touched)
    with pytest.raises(clib.SSNLibraryError, match=re.escape(message)):
        clib.check_ext2(rc, 'ssnx2_swd_match_cells_f32')


def test_empty_problems_succeed_and_write_nothing():
    from tc_gan_amd import clib
    for power in (1, 2):
        for B, start, C, m, L in ((0, (0, 0, 0), 2, 5, 3), (5, (0, 5), 1, 7, 0), (0, None, 0, 0, 0), (5, None, 0, 3, 3),
                                  (0, None, 3, 0, 3), (5, None, 2, 0, 0)):
            rc = clib.libssnode_ext2.ssnx2_swd_match_cells_f32(None, B, None, None if start is None else _starts(*start), C, None,
                                                               m, L, power, None, None, None)
            assert rc == 0, (B, start, C, m, L)
    clib.check_ext2(0, 'nothing')


def _makefile_flags(stem):
    """What csrc/Makefile compiles `stem`.hip with: its CXXFLAGS (with ARCH expanded) and FLAGS_<stem> where it sets one."""
    makefile = open(os.path.join(CSRC, 'Makefile')).read()

    def value(name):
        found = re.search(r'^%s[ \t]*[?:]?=[ \t]*(.*)$' % re.escape(name), makefile, re.M)
        return found.group(1).strip() if found else ''
    flags = (value('CXXFLAGS') + ' ' + value('FLAGS_' + stem) + ' ' + value('EXTRA')).replace('$(ARCH)', value('ARCH'))
    assert '$(' not in flags, flags
    return flags.split()


def test_cell_kernel_is_wave64_without_spills_or_scratch(tmp_path):
    """Metadata only, with the Makefile's flags.  Static LDS as designed: the four doubles of the ordered block sum and the flag
    of a non-finite segment, 40 bytes, beside the dynamic 8 P(max n_c) + 4 P(m) <= 96 KiB the launch asks for."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_swd_cells.s'
    flags = _makefile_flags('ssn_swd_cells')
    assert '-O3' in flags and '--offload-arch=gfx950' in flags and '-fPIC' in flags
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_swd_cells.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    found = re.findall(r'\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)'
                       r'.*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+).*?\.wavefront_size:\s+(\d+)', text, re.S)
    assert len(found) == 1 and 'swd_match_cells_kernel' in found[0][1], found
    assert [int(v) for k, v in enumerate(found[0]) if k != 1] == [40, 0, 0, 0, 64], found
    source = open(os.path.join(CSRC, 'ssn_swd_cells.hip')).read() + open(os.path.join(CSRC, 'ssn_swd_cells_dev.h')).read()
    assert 'asm' not in source and 'atomicAdd' not in source


def test_the_makefile_builds_the_second_companion_from_objects_of_its_own():
    makefile = open(os.path.join(CSRC, 'Makefile')).read()
    mine = ('ssn_ext2_capi.hip', 'ssn_swd_cells.hip')
    first_srcs = re.search(r'^SRCS\s+:=(.*)$', makefile, re.M).group(1)
    ext_srcs = re.search(r'^EXT_SRCS\s+:=(.*)$', makefile, re.M).group(1)
    ext2_srcs = re.search(r'^EXT2_SRCS\s+:=(.*)$', makefile, re.M).group(1).split()
    assert sorted(ext2_srcs) == sorted(mine)
    for name in mine:                                             # linked into neither of the other two libraries
        assert name not in first_srcs and name not in ext_srcs
    assert re.search(r'^all:.*\$\(EXT2_OUT\)', makefile, re.M)
    assert re.search(r'^EXT2_OUT\s+:=.*libssnode_ext2\.so', makefile, re.M)
    assert re.search(r'^libssnode_ext2\.map: \$\(EXT2_HDR\) gen_export_map\.py', makefile, re.M)
    assert '--version-script=$(EXT2_LINKMAP)' in makefile
    clean = re.search(r'^clean:\n\t(.*)$', makefile, re.M).group(1)
    assert '$(EXT2_OBJS)' in clean and '$(EXT2_OUT)' in clean and 'libssnode_ext2.map' in clean
    # the second companion's headers are its own: no object of the other libraries depends on them
    hdrs = re.search(r'^HDRS\s+:=\s*\$\(filter-out ([^,]*),', makefile, re.M).group(1)
    assert hdrs.split()[0] == '$(EXT_HDRS)' and '$(EXT2_HDRS)' in hdrs.split()
    ext2_hdrs = re.search(r'^EXT2_HDRS\s+:=(.*)$', makefile, re.M).group(1).split()
    assert {'ssn_ext2_host.h', 'ssn_swd_cells_dev.h', '../../include/ssnode_mi355x_ext2.h'} <= set(ext2_hdrs)
    assert {'ssn_ext_host.h', 'ssn_swd_sizes_dev.h'} <= set(re.search(r'^EXT_HDRS\s+:=(.*)$', makefile, re.M).group(1).split())
    for name in os.listdir(CSRC):
        if name.endswith(('.hip', '.h')) and name not in mine + ('ssn_swd_cells_dev.h',):
            text = open(os.path.join(CSRC, name)).read()
            assert 'ssn_ext2_host.h' not in text and 'ssn_swd_cells_dev.h' not in text and 'mi355x_ext2.h' not in text, name
            assert name == 'ssn_ext2_host.h' or 'launch_swd_match_cells' not in text, name
    for name in mine + ('ssn_swd_cells_dev.h', 'ssn_ext2_host.h'):          # and the new files keep off the first companion's
        text = open(os.path.join(CSRC, name)).read()
        for word in ('ssn_ext_host.h', 'ssn_swd_sizes_dev.h', 'mi355x_ext.h', 'launch_swd_match_sizes'):
            assert word not in text, (name, word)


# ---- 4. the command line ------------------------------------------------------------------------------------------------

CSWD_KEYS = {'D0', 'D_max', 'D_min', 'J0', 'J_max', 'J_min', 'S0', 'S_max', 'S_min', 'contrasts', 'dataset_provider', 'datastore',
             'datastore_template', 'dynamics_cost', 'gen_kernel', 'include_inhibitory_neurons', 'iterations', 'learning_rate',
             'load_config', 'load_gen_param', 'n_bandwidths', 'norm_probes', 'num_models', 'probes_per_model', 'quiet', 'seqlen',
             'skip_steps', 'ssn_type', 'swd_direction_seed', 'swd_directions', 'swd_power', 'truth_seed', 'truth_size',
             'unroll_scan', 'update_name', 'z_device_seed', 'z_host_draw'}


def test_command_line_of_the_conditional_script():
    from tc_gan_amd.run import bptt_cswd, bptt_swd, bptt_swd_ensemble, options
    with pytest.raises(SystemExit) as err:
        bptt_cswd.make_parser().parse_args(['--help'])
    assert err.value.code == 0
    ns = vars(bptt_cswd.make_parser().parse_args([]))
    assert set(ns) == CSWD_KEYS
    assert ns['datastore_template'] == 'logfiles/BPTT_CSWD_{swd_directions}_{swd_power}'
    assert (ns['num_models'], ns['probes_per_model'], ns['norm_probes']) == (15, 1, [0])
    for refused in (['--swd-truth-batch', '-1'], ['--batchsize', '4'], ['--lam', '1']):
        with pytest.raises(SystemExit) as err:
            bptt_cswd.make_parser().parse_args(refused)
        assert err.value.code == 2
    got = vars(bptt_cswd.make_parser().parse_args(['--num-models', '64', '--probes-per-model', '2', '--norm-probes', '0,0.5',
                                                   '--contrasts', '5,20', '--swd-power', '1']))
    assert (got['num_models'], got['probes_per_model'], got['norm_probes'], got['contrasts']) == (64, 2, [0, 0.5], [5, 20])
    # no row of the table carries the new script's letter: its rows are derived, as those of 's' are
    assert all(set(o['scripts']) <= set('wcm') for o in options.OPTIONS)
    flags = [o['flags'][0] for o in options.options_of('k')]
    assert flags[-3:] == ['--num-models', '--probes-per-model', '--norm-probes'] and len(set(flags)) == len(flags)
    s_flags = [o['flags'][0] for o in options.options_of('s')]
    assert flags[:-3] == [f for f in s_flags if f not in ('--batchsize', '--sample-sites', '--swd-truth-batch')]
    # the namespaces of the unconditional scripts are what they were
    solo = vars(bptt_swd.make_parser().parse_args([]))
    assert set(solo) == (CSWD_KEYS - {'norm_probes', 'num_models', 'probes_per_model'}) | {'batchsize', 'sample_sites'}
    assert solo['datastore_template'] == 'logfiles/BPTT_SWD_{swd_directions}_{swd_power}'
    assert set(vars(bptt_swd_ensemble.make_parser().parse_args(['--members', 'm.json']))) == set(solo) | {'members'}
    assert set(vars(bptt_swd.make_parser().parse_args(['--swd-truth-batch', '8']))) == set(solo) | {'swd_truth_batch'}


def test_main_hands_the_conditions_to_the_run_config(monkeypatch):
    """info.json is written from this config: `norm_probes` is in it, which is what the scorer reads."""
    from tc_gan_amd.run import bptt_cswd
    seen = []
    monkeypatch.setattr(bptt_cswd, 'do_learning', lambda learn, run_config, **kw: seen.append((dict(run_config), kw)))
    bptt_cswd.main(['--norm-probes', '0,0.5', '--num-models', '8'])
    rc, kw = seen[0]
    assert rc['norm_probes'] == [0, 0.5] and rc['num_models'] == 8 and 'batchsize' not in rc and 'sample_sites' not in rc
    assert kw['init_driver'] is bptt_cswd.init_driver and kw['script_file'] == bptt_cswd.__file__


# ---- 5. the host code -------------------------------------------------------------------------------------------------------

def test_cell_ids_and_layout():
    from tc_gan_amd.networks.conditional_sliced_wasserstein import cell_ids, cell_layout, truth_by_cell, weighted_mean_over_cells
    from tc_gan_amd.networks.cwgan import RandomChoiceSampler
    T, P, Cn, D, S = 2, 3, 2, 4, 5
    cond_values = [np.array([0, 1]), np.array([-0.5, 0.0, 0.25]), np.array([5.0, 20.0]), np.arange(D) / 4.0]
    nested = np.random.RandomState(0).rand(S, T, P, Cn, D)
    sampler = RandomChoiceSampler(nested, cond_values, e_ratio=0.8, seed=1)
    batch = sampler.select_minibatch(16, 2)
    ids = cell_ids(batch.conditions, sampler.cond_values)
    assert ids.shape == (32,) and ids.dtype == np.int64 and len(set(ids)) > 3
    by_cell = truth_by_cell(nested)
    assert by_cell.shape == (T * P * Cn, S, D) and by_cell.dtype == np.float32 and by_cell.flags['C_CONTIGUOUS']
    for row, (contrast, probe, cell_type) in enumerate(batch.conditions):
        t, p, k = int(cell_type), list(cond_values[1]).index(probe), list(cond_values[2]).index(contrast)
        assert ids[row] == (t * P + p) * Cn + k
        np.testing.assert_array_equal(by_cell[ids[row]], nested[:, t, p, k].astype('float32'))
    # the sampler's own truth rows of the batch are rows of the cell's block: same table, same indexing
    for row in range(32):
        assert (by_cell[ids[row]] == batch.tuning_curves[row].astype('float32')).all(axis=1).any()
    rows, start = cell_layout(ids, T * P * Cn)
    want_rows, want_start = cc.cell_layout(ids, T * P * Cn)
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(start, want_start)
    assert rows.dtype == start.dtype == np.int32
    for c in range(T * P * Cn):
        seg = rows[start[c]:start[c + 1]]
        assert (ids[seg] == c).all() and (np.diff(seg) > 0).all()
    loss_cl = np.random.RandomState(2).rand(T * P * Cn, 7)
    got, want = weighted_mean_over_cells(loss_cl, start), cc.swd_in_host_order(loss_cl, start)
    assert got[0] == want[0] and (got[1] == want[1]).all()
    with pytest.raises(ValueError, match='cell ids must be in 0 .. 2'):
        cell_layout(np.array([0, 3]), 3)


def test_refusals_by_name(monkeypatch):
    from tc_gan_amd import clib
    from tc_gan_amd.networks.conditional_sliced_wasserstein import (cell_ids, cswd_loss_grad, make_conditional_sliced_wasserstein,
                                                                    truth_by_cell)
    good = [np.array([0]), np.array([0.0, 0.5]), np.array([5.0, 20.0])]
    for k, name in enumerate(('cell_types', 'norm_probes', 'contrasts')):
        values = [v.copy() for v in good]
        values[k] = np.concatenate([values[k], values[k][:1]])
        with pytest.raises(ValueError, match=name + r' = .* has duplicate values'):
            cell_ids(np.zeros((0, 3)), values)
    with pytest.raises(ValueError, match='a value of contrasts that is not in'):
        cell_ids(np.array([[7.0, 0.0, 0]]), good)
    with pytest.raises(ValueError, match=r'the truth has 16385 rows, the match takes 1 \.\. 16384 per cell'):
        truth_by_cell(np.zeros((clib.SWD_MAX_TRUTH + 1, 1, 1, 1, 2), dtype='float32'))
    with pytest.raises(ValueError, match=r'= 260 cells, the match takes 256'):
        truth_by_cell(np.zeros((2, 2, 65, 2, 2), dtype='float32'))
    assert truth_by_cell(np.zeros((clib.SWD_MAX_TRUTH, 1, 1, 1, 2), dtype='float32')).shape == (1, clib.SWD_MAX_TRUTH, 2)
    x, theta = torch.zeros(4, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError, match='contiguous'):
        cswd_loss_grad(x, np.zeros(4, dtype=int), torch.zeros(2, 5, 4), theta, 2)
    with pytest.raises(ValueError, match='truth rows per cell'):
        cswd_loss_grad(x, np.zeros(4, dtype=int), torch.zeros(2, 0, 3), theta, 2)
    with pytest.raises(ValueError, match='3 cell ids for 4 rows'):
        cswd_loss_grad(x, np.zeros(3, dtype=int), torch.zeros(2, 5, 3), theta, 2)
    with pytest.raises(ValueError, match='cell ids must be in 0 .. 1'):
        cswd_loss_grad(x, np.array([0, 1, 2, 0]), torch.zeros(2, 5, 3), theta, 2)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one GPU'):
        make_conditional_sliced_wasserstein({})


def test_generator_step_defaults_are_the_callers_of_before():
    """`GeneratorStepTrainer.generator_step` takes the forward's inputs and the noise as optional parameters; without them it
    makes the call it made: the trainer's grid, `_draw_noise()`."""
    import inspect
    from tc_gan_amd.networks.moment_matching import GeneratorStepTrainer
    sig = inspect.signature(GeneratorStepTrainer.generator_step)
    assert list(sig.parameters) == ['self', 'info', 'loss_grad', 'forward_kwargs', 'noise']
    assert sig.parameters['forward_kwargs'].default is None and sig.parameters['noise'].default is None

    class Stop(Exception):
        pass

    class Gen(object):
        def forward(self, **kw):
            self.seen = kw
            raise Stop

    t = GeneratorStepTrainer()
    t.gen, t.rng, t.rate_penalty_threshold = Gen(), 'rng', 3.0
    t.stimulator_bandwidths, t.stimulator_contrasts = 'bw', 'con'
    t._draw_noise = lambda: dict(model_zs='z')
    with pytest.raises(Stop):
        t.generator_step(None, None)
    assert t.gen.seen == dict(rng='rng', save=True, stimulator_bandwidths='bw', stimulator_contrasts='con',
                              model_rate_penalty_threshold=3.0, model_zs='z')
    with pytest.raises(Stop):
        t.generator_step(None, None, forward_kwargs=dict(stimulator_bandwidths='b2', prober_model_ids='ids'), noise={})
    assert t.gen.seen == dict(rng='rng', save=True, model_rate_penalty_threshold=3.0, stimulator_bandwidths='b2',
                              prober_model_ids='ids')

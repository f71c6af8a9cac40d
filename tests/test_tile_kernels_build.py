"""The kernel set and the resources of every kernel of csrc/ssn_tile.hip and csrc/ssn_gen.hip, cross-compiled for gfx950 as
tests/test_tile_mixed6_build.py does; nothing runs.

  * Same kernel set: the mangled names of ssn_tile.hip's 27 kernels are the ones listed here and no others (profiles/ and the
    other build tests go by these names), and ssn_gen.hip keeps its 38.
  * Resources, from the kernel descriptors' metadata: no spilled VGPR, no scratch, the LDS size listed, and at most the VGPRs
    listed.  The figures are those of the build before the source was split into one function per loop.
    Several sit right at a register step, which csrc/ssn_tile.hip::tile_hard_split's comment names: 128 VGPRs at C = 13 (a
    fourth wave per SIMD), 168 at C = 19 and C = 25 (three).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')

# solve_tile_kernel<T, RA, C, RL, NB, 64 * MAXW, MINW>: (T, RA, C, RL, NB) -> (MAXW, MINW, VGPRs, LDS bytes)
UNIFORM = {
    ('f', 7, 4, 0, 4): (1, 2, 88, 1072), ('f', 7, 4, 0, 2): (1, 2, 64, 536), ('f', 7, 4, 0, 1): (1, 2, 52, 264),
    ('f', 7, 8, 0, 4): (2, 2, 128, 3120), ('f', 7, 8, 0, 2): (2, 2, 98, 1560), ('f', 7, 8, 0, 1): (2, 2, 80, 776),
    ('f', 7, 13, 0, 4): (2, 2, 166, 5168), ('f', 7, 13, 0, 2): (2, 2, 140, 2584), ('f', 7, 13, 0, 1): (2, 2, 128, 1288),
    ('f', 7, 19, 1, 1): (3, 3, 150, 15624),
    ('f', 7, 19, 0, 4): (3, 2, 216, 5168), ('f', 7, 19, 0, 2): (3, 2, 184, 2584), ('f', 7, 19, 0, 1): (3, 2, 168, 1288),
    ('f', 7, 25, 2, 1): (4, 3, 166, 50440),
    ('f', 7, 25, 0, 2): (4, 2, 244, 3608), ('f', 7, 25, 0, 1): (4, 2, 212, 1800),
    ('f', 7, 26, 0, 2): (4, 2, 253, 3608), ('f', 7, 26, 0, 1): (4, 2, 219, 1800),
    ('d', 7, 4, 0, 1): (1, 1, 138, 528), ('d', 7, 8, 0, 1): (2, 1, 199, 1552), ('d', 7, 13, 0, 1): (2, 1, 268, 2576),
    ('d', 4, 19, 0, 1): (5, 2, 234, 2576), ('d', 4, 26, 1, 1): (7, 2, 249, 97808),
}
EXPECTED = {'_ZN3ssn17solve_tile_kernelI%sLi%dELi%dELi%dELi%dELi%dELi%dEEEvNS_9SolveArgsIT_EE' % (t, ra, c, rl, nb, 64 * mw, mnw): (v, l)
            for (t, ra, c, rl, nb), (mw, mnw, v, l) in UNIFORM.items()}
# solve_tile_mixed_kernel<float, C, RL, NW, LRA, 1, 3> and solve_tile_mixed6_kernel<float, 25, 12, 1, 3>
EXPECTED.update({
    '_ZN3ssn23solve_tile_mixed_kernelIfLi19ELi1ELi3ELi4ELi1ELi3EEEvNS_9SolveArgsIT_EE': (150, 14600),
    '_ZN3ssn23solve_tile_mixed_kernelIfLi19ELi1ELi3ELi5ELi1ELi3EEEvNS_9SolveArgsIT_EE': (151, 14600),
    '_ZN3ssn23solve_tile_mixed_kernelIfLi25ELi2ELi4ELi4ELi1ELi3EEEvNS_9SolveArgsIT_EE': (167, 49416),
    '_ZN3ssn24solve_tile_mixed6_kernelIfLi25ELi12ELi1ELi3EEEvNS_9SolveArgsIT_EE': (168, 36616),
})
GEN_KERNELS = {'gen_forward_kernel': 18, 'gen_backward_kernel': 18, 'jds_grad_kernel': 2}


def _descriptors(module, tmp):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp / (module + '.s')
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', module + '.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    got = {}
    for doc in re.split(r'\n  - \.agpr_count:', open(str(out)).read())[1:]:
        name = re.search(r'\.name:\s+(\S+)', doc).group(1)
        got[name] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, doc).group(1))
                     for k in ('vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')}
    return got


@pytest.fixture(scope='module')
def tile(tmp_path_factory):
    return _descriptors('ssn_tile', tmp_path_factory.mktemp('tile_kernels'))


@pytest.fixture(scope='module')
def gen(tmp_path_factory):
    return _descriptors('ssn_gen', tmp_path_factory.mktemp('gen_kernels'))


def test_tile_kernel_set(tile):
    assert len(EXPECTED) == 27
    assert sorted(tile) == sorted(EXPECTED), sorted(set(tile) ^ set(EXPECTED))


def test_tile_kernel_resources(tile):
    bad = []
    for name, (vgprs, lds) in sorted(EXPECTED.items()):
        got = tile[name]
        print(name, got)
        if (got['vgpr_spill_count'] or got['private_segment_fixed_size'] or got['vgpr_count'] > vgprs
                or got['group_segment_fixed_size'] != lds):
            bad.append((name, got, vgprs, lds))
    assert not bad, bad


def test_register_steps(tile):
    """the shapes that tile_hard_split's comment names stay on their side of the step"""
    for key, step in ((('f', 7, 13, 0, 1), 128), (('f', 7, 19, 0, 1), 168), (('f', 7, 19, 1, 1), 168), (('f', 7, 25, 2, 1), 168)):
        mw, mnw = UNIFORM[key][:2]
        name = '_ZN3ssn17solve_tile_kernelI%sLi%dELi%dELi%dELi%dELi%dELi%dEEEvNS_9SolveArgsIT_EE' % (key + (64 * mw, mnw))
        assert tile[name]['vgpr_count'] <= step, (name, tile[name])
    for name in EXPECTED:
        if 'mixed' in name:
            assert tile[name]['vgpr_count'] <= 168, (name, tile[name])


def test_gen_kernel_set(gen):
    count = {k: sum(1 for n in gen if k in n) for k in GEN_KERNELS}
    assert count == GEN_KERNELS and len(gen) == 38, (count, len(gen))
    for name, got in sorted(gen.items()):
        assert got['vgpr_spill_count'] == 0 and got['private_segment_fixed_size'] == 0, (name, got)

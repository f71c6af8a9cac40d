"""The generated code of the fp32 matrix-core kernels (csrc/ssn_mfma.hip): 16 kernels = (forward with and without the trajectory
stores, adjoint sweep, solver) x the ladder sizes 104 / 152 / 200 / 208.  Their launch bounds promise three waves per SIMD of the
512-register file at 152 / 200 (K-split operand layout: 168 VGPRs) and two at 104 / 208 (slab layout: 256), with no scratch; the
LDS sizes are the layout itself (state rows, hand-off block, solver flags).  Compiled for gfx950 with the Makefile's flags, as
tests/test_tile_mixed6_build.py does; read from the kernel descriptors' metadata, not from the instructions.

SGPR spills go to lanes of a VGPR (no memory).  The ceilings are what the kernels had when the matrix-wave role was still
written out per kernel and layout: adjoint 36 (152) and 66 (200), solver 38 (152), none elsewhere.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')
LADDER = (104, 152, 200, 208)
VGPR_MAX = {104: 256, 152: 168, 200: 168, 208: 256}
# kernel -> ladder size -> (LDS bytes, ceiling of the SGPR spill count)
EXPECT = {
    'gen_forward_mfma_kernel': {104: (15104, 0), 152: (35328, 0), 200: (46080, 0), 208: (21760, 0)},
    'gen_backward_mfma_kernel': {104: (11648, 0), 152: (29952, 36), 200: (39424, 66), 208: (14976, 0)},
    'solve_mfma_kernel': {104: (15200, 0), 152: (35424, 38), 200: (46176, 0), 208: (21856, 0)},
}


def _makefile_flags():
    text = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'FLAGS_ssn_mfma ' not in text and 'FLAGS_ssn_mfma:' not in text        # no per-file flags for this file
    return re.search(r'^CXXFLAGS \?= (.*)$', text, re.M).group(1).replace('$(ARCH)', 'gfx950').split()


def test_mfma_kernel_resources(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_mfma.s'
    subprocess.run([hipcc] + _makefile_flags() + ['-S', '--cuda-device-only', 'ssn_mfma.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    docs = [d for d in re.split(r'\n  - \.agpr_count:', open(str(out)).read())[1:] if '.vgpr_count:' in d]
    seen = []
    for d in docs:
        name = re.search(r'\.name:\s+(\S+)', d).group(1)
        m = re.match(r'_ZN3ssn\d+(\w+_kernel)ILi(\d+)E(Lb[01]E)?', name)
        assert m, name
        kernel, mk = m.group(1), int(m.group(2))
        seen.append((kernel, mk, m.group(3)))
        got = {k: int(re.search(r'\.%s:\s+(\d+)' % k, d).group(1)) for k in (
            'vgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')}
        print(kernel, mk, m.group(3), got)
        lds, sgpr_spills = EXPECT[kernel][mk]
        assert got['vgpr_spill_count'] == 0 and got['private_segment_fixed_size'] == 0, (name, got)
        assert got['group_segment_fixed_size'] == lds, (name, got)
        assert got['sgpr_spill_count'] <= sgpr_spills, (name, got)
        assert got['vgpr_count'] <= VGPR_MAX[mk], (name, got)
    want = [('gen_forward_mfma_kernel', mk, s) for mk in LADDER for s in ('Lb1E', 'Lb0E')]
    want += [(k, mk, None) for k in ('gen_backward_mfma_kernel', 'solve_mfma_kernel') for mk in LADDER]
    assert len(seen) == 16 and sorted(seen, key=str) == sorted(want, key=str), seen

"""The generated code of `solve_tile_mixed6_kernel` (csrc/ssn_tile.hip: rows 56/48/48/48 at 2N = 200): three workgroups share a
CU only if the kernel stays within 168 VGPRs and a third of the LDS that three workgroups can have, 54,613 B, and a spill
inside the step loop would cost more than the layout gains.  Compiled for gfx950 as tests/test_distdiff.py does for the scorer;
read from the kernel descriptor's metadata, not from the instructions.

SGPR spills go to lanes of a VGPR (no memory); the parent's mixed kernel has 4 of them in its prologue and this one may have as
many, so the count is only bounded by what fits one VGPR.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')
LDS_FOR_THREE = 163840 // 3       # 54,613 B


def test_threshold_in_the_source_is_the_one_the_gpu_tests_use():
    from test_tile_mixed6_gpu import MIXED6_MIN_M
    text = open(os.path.join(CSRC, 'ssn_tile.hip')).read()
    assert [int(m) for m in re.findall(r'TILE_MIXED6_MIN_M = (\d+);', text)] == [MIXED6_MIN_M]


def test_mixed6_kernel_resources(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_tile.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_tile.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(str(out)).read()
    docs = [d for d in re.split(r'\n  - \.agpr_count:', text) if 'solve_tile_mixed6_kernel' in d and '.vgpr_count:' in d]
    assert len(docs) == 1, len(docs)

    def field(name):
        return int(re.search(r'\.%s:\s+(\d+)' % name, docs[0]).group(1))

    got = {k: field(k) for k in ('vgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                 'group_segment_fixed_size', 'max_flat_workgroup_size')}
    print(got)
    assert got['vgpr_spill_count'] == 0 and got['private_segment_fixed_size'] == 0, got
    assert got['vgpr_count'] <= 168, got
    assert got['group_segment_fixed_size'] <= LDS_FOR_THREE, got
    assert got['sgpr_spill_count'] <= 64 and got['max_flat_workgroup_size'] == 256, got

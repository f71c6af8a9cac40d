"""The generated code of the device MT19937 draw (csrc/ssn_mt19937.hip): 13 kernels = expand, jump, solo, the generation kernel
for float with every combination of its three switches (ODD, BUILDW, TAIL) and for double with ODD alone -- BUILDW and TAIL are
float-only, and the host's kernel choice must not instantiate them for double.  No scratch; the fixed LDS sizes are the layout
itself (solo: the ring of 1248 words + the arrival flag; generation: two block buffers + the carry, + alignment in the W form;
the tap windows of jump and solo and the expanded sequence are dynamic).  The VGPR ceilings are what the kernels had when jump
and solo each carried their own copy of the tap loop.  Compiled for gfx950 with the Makefile's flags, as tests/test_mfma_build.py
does; read from the kernel descriptors' metadata, not from the instructions."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')
# kernel -> (VGPR ceiling, fixed LDS bytes)
FIXED = {'mt_expand_kernel': (50, 0), 'mt_jump_kernel': (86, 0), 'mt_solo_kernel': (89, 5008)}
GEN_PLAIN, GEN_BUILDW = (34, 5256), (58, 5264)
BOOLS = ('Lb0E', 'Lb1E')


def _makefile_flags():
    text = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'FLAGS_ssn_mt19937 ' not in text and 'FLAGS_ssn_mt19937:' not in text        # no per-file flags for this file
    return re.search(r'^CXXFLAGS \?= (.*)$', text, re.M).group(1).replace('$(ARCH)', 'gfx950').split()


def test_mt19937_kernel_resources(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'ssn_mt19937.s'
    subprocess.run([hipcc] + _makefile_flags() + ['-S', '--cuda-device-only', 'ssn_mt19937.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    docs = [d for d in re.split(r'\n  - \.agpr_count:', open(str(out)).read())[1:] if '.vgpr_count:' in d]
    seen = []
    for d in docs:
        name = re.search(r'\.name:\s+(\S+)', d).group(1)
        m = re.match(r'_ZN3ssn2mt\d+(mt_\w+_kernel)(?:I([fd])(Lb[01]E)(Lb[01]E)(Lb[01]E)E)?', name)
        assert m, name
        kernel, form = m.group(1), m.groups()[1:]
        seen.append((kernel,) + form)
        got = {k: int(re.search(r'\.%s:\s+(\d+)' % k, d).group(1)) for k in (
            'vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')}
        print(kernel, form, got)
        if kernel == 'mt_gen_kernel':
            vgprs, lds = GEN_BUILDW if form[2] == 'Lb1E' else GEN_PLAIN
        else:
            assert form == (None,) * 4, name
            vgprs, lds = FIXED[kernel]
        assert got['vgpr_spill_count'] == 0 and got['private_segment_fixed_size'] == 0, (name, got)
        assert got['group_segment_fixed_size'] == lds, (name, got)
        assert got['vgpr_count'] <= vgprs, (name, got)
    want = [(k, None, None, None, None) for k in FIXED]
    want += [('mt_gen_kernel', 'f', odd, buildw, tail) for odd in BOOLS for buildw in BOOLS for tail in BOOLS]
    want += [('mt_gen_kernel', 'd', odd, 'Lb0E', 'Lb0E') for odd in BOOLS]
    assert len(seen) == 13 and sorted(seen, key=str) == sorted(want, key=str), seen

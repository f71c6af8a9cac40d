"""The generated code of `solve_tile_mixed6_kernel` (csrc/ssn_tile.hip) behind the transpose-reduce on DPP bank masks (form D of
DESIGN 3.1, round 9), the verdict byte that is stored only when it changes and the loop without the rate-bound compare.  Cross-compiled for gfx950 as
tests/test_tile_mixed6_build.py does; nothing runs.

  * Resources, from the kernel descriptor's metadata: at most 168 VGPRs, no scratch, no spilled VGPR, LDS for three workgroups
    per CU (54,613 B).
  * The steady-state loops, counted by mnemonic with the rule of DESIGN 3.1's round-7 table: every instruction of every block
    that the compiler marks as part of the loop (both arms of the soft-bound branch included; the loop holds two steps, the
    figures are per step).  The kernel holds each wave kind's loop twice, with and without the test of the rate bound.  Not
    counted: the two blocks of three to five instructions that store a changed verdict byte, which a solve enters twice.
    Vector instructions per step:

        without the rate test (asym_tanh)    7-row wave <= 126    6-row waves <= 111
        with it                              one more, the compare: <= 127, <= 112

    (parent: 130 and 115 in its one loop per wave kind.)
  * The loops without the rate test hold no v_cmp_le_f32 (the compare against hard_stop), the others one per step.
  * Between the last packed FMA and the v_log_f32 of a step stand the reduce's 12 (7 rows) or 11 (6 rows) DPP adds and the two
    selects of its third exchange, and no other select.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tc_gan_amd', 'csrc')
LDS_FOR_THREE = 163840 // 3       # 54,613 B
PK_PER_STEP = {7: 87, 6: 75}      # v_pk_fma_f32 / v_pk_mul_f32 of a wave kind's step: what tells the loops apart
BOUND = {(7, False): 126, (6, False): 111, (7, True): 127, (6, True): 112}


@pytest.fixture(scope='module')
def assembly(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path_factory.mktemp('tile_reduce') / 'ssn_tile.s'
    flags = ['-O3', '-std=c++17', '--offload-arch=gfx950']                       # csrc/Makefile: CXXFLAGS
    subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', 'ssn_tile.hip', '-o', str(out)], cwd=CSRC, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(str(out)).read()


def test_mixed6_kernel_resources(assembly):
    docs = [d for d in re.split(r'\n  - \.agpr_count:', assembly) if 'solve_tile_mixed6_kernel' in d and '.vgpr_count:' in d]
    assert len(docs) == 1, len(docs)
    got = {k: int(re.search(r'\.%s:\s+(\d+)' % k, docs[0]).group(1))
           for k in ('vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')}
    print(got)
    assert got['vgpr_spill_count'] == 0 and got['private_segment_fixed_size'] == 0, got
    assert got['vgpr_count'] <= 168 and got['group_segment_fixed_size'] <= LDS_FOR_THREE, got


def _blocks(body):
    """[label, label of the loop header it belongs to or None, is a loop header, [instruction, ...]] per basic block"""
    out, cur = [], None
    for line in body.split('\n'):
        m = re.match(r'^\.L(BB\d+_\d+):(.*)', line) or re.match(r'^; %bb\.(\d+):(.*)', line)
        if m:
            h = re.search(r'Header=(BB\d+_\d+)', m.group(2))
            cur = [m.group(1), h.group(1) if h else None, 'Loop Header' in m.group(2), []]
            out.append(cur)
            continue
        code = line.split(';')[0].strip()
        if cur is not None and code and not code.startswith('.'):
            cur[3].append(code)
    return out


def _loops(assembly):
    """{(rows of the wave kind, has the rate test): [instruction, ...] of the steady-state loop (two steps)}"""
    m = re.search(r'^(_ZN3ssn24solve_tile_mixed6_kernel\w+):.*?\n(.*?)^\s*s_endpgm', assembly, re.S | re.M)
    assert m, 'kernel not found'
    blocks = _blocks(m.group(2))
    out = {}
    for label, _, is_header, _ in blocks:
        if not is_header:
            continue
        members = [b for b in blocks if b[0] == label or b[1] == label]
        cold = [b for b in members if len(b[3]) <= 6 and any(i.startswith('ds_write_b8') for i in b[3])]
        code = [i for b in members if b not in cold for i in b[3]]
        pk = sum(i.startswith(('v_pk_fma_f32', 'v_pk_mul_f32')) for i in code)
        rows = {2 * v: k for k, v in PK_PER_STEP.items()}.get(pk)
        if rows is None:
            continue                                            # (the prologue's loops)
        assert len(cold) == 2, (label, len(cold))
        hard = any(i.startswith('v_cmp_le_f32') for i in code)
        assert (rows, hard) not in out, (rows, hard)
        out[(rows, hard)] = code
    return out


def test_steady_state_loops(assembly):
    loops = _loops(assembly)
    assert sorted(loops) == sorted(BOUND), sorted(loops)
    for key, code in sorted(loops.items()):
        mnem = collections.Counter(i.split()[0] for i in code)
        vector = sum(n for k, n in mnem.items() if k.startswith('v_'))
        lds = sum(n for k, n in mnem.items() if k.startswith('ds_'))
        print('%d-row wave, rate test %s: all %.1f vector %.1f LDS %.1f per step; DPP adds %d, v_cndmask %d, v_mov %d per two steps'
              % (key[0], key[1], len(code) / 2, vector / 2, lds / 2, mnem['v_add_f32_dpp'],
                 sum(n for k, n in mnem.items() if k.startswith('v_cndmask')), mnem['v_mov_b32_e32']))
        assert vector <= 2 * BOUND[key], (key, vector / 2)
        assert sum(n for k, n in mnem.items() if k.startswith('v_cmp_le_f32')) == (2 if key[1] else 0), key
        assert not any(k.startswith('ds_write_b8') for k in mnem), key


def test_two_selects_between_the_fma_block_and_the_io_function(assembly):
    for key, code in sorted(_loops(assembly).items()):
        mnem = [i.split()[0] for i in code]
        logs = [n for n, k in enumerate(mnem) if k.startswith('v_log_f32')]
        assert len(logs) == 2, (key, len(logs))
        for n in logs:
            # backwards from the v_log_f32 to the last packed FMA, round the loop (the loop's branch stands between them)
            between = []
            for j in range(1, len(mnem)):
                k = mnem[(n - j) % len(mnem)]
                if k.startswith(('v_pk_fma_f32', 'v_pk_mul_f32')):
                    break
                between.append(k)
            assert sum(k.startswith('v_add_f32_dpp') for k in between) == {7: 12, 6: 11}[key[0]], (key, between)
            assert sum(k.startswith('v_cndmask') for k in between) == 2, (key, between)

#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds of one module, kernel by kernel (a refactor's working check).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only ssn_tile.hip -o tree.s      (and the same for the parent)
    tools/isa_compare.py parent.s tree.s

One line per kernel: its resources in both builds, and whether the instruction text is the same (labels and comments
stripped), or else whether at least the histogram of v_* and ds_* mnemonics is.  For solve_tile_mixed6_kernel also the
steady-state loops as tests/test_tile_reduce_build.py extracts them.  Exit status 1 if a kernel is missing or new, uses
more VGPRs, another LDS size, spills, or differs in its v_* / ds_* histogram.
"""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
KEYS = ('vgpr_count', 'sgpr_count', 'group_segment_fixed_size', 'vgpr_spill_count', 'private_segment_fixed_size')


def kernels(text):
    """{mangled name: ({resource: value}, [instruction, ...])}"""
    meta = {}
    for doc in re.split(r'\n  - \.agpr_count:', text)[1:]:
        name = re.search(r'\.name:\s+(\S+)', doc).group(1)
        meta[name] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, doc).group(1)) for k in KEYS}
    out = {}
    for name in meta:
        body = re.search(r'^%s:.*?\n(.*?)^\.Lfunc_end' % re.escape(name), text, re.S | re.M).group(1)
        code = []
        for line in body.split('\n'):
            line = line.split(';')[0].strip()
            if line and not line.startswith('.') and not line.endswith(':'):
                code.append(re.sub(r'\.LBB\d+_\d+', 'L', line))
        out[name] = (meta[name], code)
    return out


def hist(code):
    return collections.Counter(i.split()[0] for i in code if i.startswith(('v_', 'ds_')))


def main(parent_s, tree_s):
    parent_text, tree_text = open(parent_s).read(), open(tree_s).read()
    parent, tree = kernels(parent_text), kernels(tree_text)
    bad = 0
    for name in sorted(set(parent) | set(tree)):
        if name not in parent or name not in tree:
            print('%s: only in the %s' % (name, 'tree' if name in tree else 'parent'))
            bad += 1
            continue
        (pm, pc), (tm, tc) = parent[name], tree[name]
        ok = (tm['vgpr_count'] <= pm['vgpr_count'] and tm['group_segment_fixed_size'] == pm['group_segment_fixed_size']
              and tm['vgpr_spill_count'] == 0 and tm['private_segment_fixed_size'] == 0)
        if pc == tc:
            verdict = 'identical (%d instructions)' % len(pc)
        elif hist(pc) == hist(tc):
            verdict = 'same v_/ds_ histogram (%d -> %d instructions)' % (len(pc), len(tc))
        else:
            diff = {k: (hist(pc)[k], hist(tc)[k]) for k in set(hist(pc)) | set(hist(tc)) if hist(pc)[k] != hist(tc)[k]}
            verdict = 'DIFFERS (%d -> %d instructions) %s' % (len(pc), len(tc), sorted(diff.items()))
            ok = False
        print('%s: VGPRs %d -> %d, SGPRs %d -> %d, LDS %d -> %d: %s%s'
              % (name, pm['vgpr_count'], tm['vgpr_count'], pm['sgpr_count'], tm['sgpr_count'], pm['group_segment_fixed_size'],
                 tm['group_segment_fixed_size'], verdict, '' if ok else '  <-- NOT OK'))
        bad += not ok
    if 'solve_tile_mixed6_kernel' in parent_text:
        from test_tile_reduce_build import _loops
        pl, tl = _loops(parent_text), _loops(tree_text)
        for key in sorted(pl):
            same = hist(pl[key]) == hist(tl[key])
            ok = same and len(tl[key]) <= len(pl[key])
            print('solve_tile_mixed6_kernel loop, %d-row wave, rate test %s: %d -> %d instructions per two steps, v_/ds_ histogram %s%s'
                  % (key[0], key[1], len(pl[key]), len(tl[key]), 'same' if same else 'DIFFERS', '' if ok else '  <-- NOT OK'))
            bad += not ok
    print('%d kernels in the parent, %d in the tree, %d not ok' % (len(parent), len(tree), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))

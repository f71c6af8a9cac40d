"""The GAN loop's host code against records frozen before its state was gathered into objects (tools/gan_loop_records.py,
tests/golden/gan_loop_records.npz): every case runs again through the tool's own functions and every array -- the records'
scalar fields, the critic norms, the final parameters, each updater's step and moments, the RandomState, the collectives
issued, the builder's unconsumed keys -- must come out bit for bit, NaN positions included.  The file was made on the commit
before the refactor; two runs of that commit gave the same bits for every case, so no case is compared with a tolerance.

A later change that alters arithmetic on purpose regenerates the file with the tool (`tools/gan_loop_records.py
tests/golden/gan_loop_records.npz`) and says so."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gan_loop_records as glr  # noqa: E402


@pytest.fixture(scope='module')
def frozen():
    return glr.load(os.path.join(ROOT, 'tests', 'golden', 'gan_loop_records.npz'))


def test_the_file_holds_every_case(frozen):
    assert sorted(frozen) == sorted(glr.CASES)


@pytest.mark.parametrize('case', list(glr.CASES))
def test_case_reproduces_the_frozen_records_bit_for_bit(case, frozen):
    got, want = glr.CASES[case](), frozen[case]
    assert sorted(got) == sorted(want)
    differing = [field for field in sorted(want) if not glr.same_bits(got[field], want[field])]
    assert not differing, '{}: {} differ from the frozen run'.format(case, differing)

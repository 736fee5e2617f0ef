"""k_gemm_fp8_tn and k_gemm_mxfp4_tn on real data, bit for bit: the SHA-256
digests of tests/gemm_digest_cases.py against tests/data/gemm_tiled_digests.json.

The exact tests of the two kernels use integer and one-hot data, which any
order of the fp32 sum satisfies, and hold real data only to a tolerance.  These
digests pin the bits on random e4m3 operands, non-power-of-two row scales and
MXFP4 blocks of many binades, so a change to the shared tile loop
(csrc/hip/gemm_q_tile.hpp) or to either operand policy that moves one output
bit fails here.  The file was recorded on the MI355X from the build of the
commit named in its "recorded_from" field, with `python
tests/gemm_digest_cases.py`; it is never recorded from the change under test.
A later change that reorders the fp32 sum on purpose re-records the file from
its own build and says so."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_digest_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_tiled_digests.json")


@pytest.fixture(scope="module")
def got():
    assert torch.cuda.is_available()
    return DC.digests()


def test_digests_equal_the_recorded_ones(got):
    with open(RECORDED) as f:
        rec = json.load(f)
    assert rec["recorded_from"]
    want = rec["digests"]
    assert sorted(got) == sorted(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, wrong


def test_a_shape_has_one_digest_whatever_the_grid(got):
    """grid = 3: a workgroup walks many tiles through the same LDS buffers and
    registers; the default grid gives every tile its own workgroup."""
    for M, N, K in DC.SHAPES:
        for form in DC.forms(K):
            ds = {got[f"{form}/{M}x{N}x{K}/grid{g}"] for g in DC.GRIDS}
            assert len(ds) == 1, (form, M, N, K)

"""The inputs of the tiled-GEMM digest guard (tests/gemm_digest_cases.py) on the
CPU: the builders are deterministic and free of NaN codes, the scales and MXFP4
blocks are what makes a digest sensitive, and the shapes reach the branches of
the tile loop that they are there for."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_digest_cases as DC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402


def test_builders_are_deterministic():
    for M, N, K in DC.SHAPES:
        for x, y in zip(DC.operands(M, N, K), DC.operands(M, N, K)):
            assert torch.equal(x, y)
        assert torch.equal(DC.mxfp4_source(N, K, 5).view(torch.int16), DC.mxfp4_source(N, K, 5).view(torch.int16))
    assert not torch.equal(DC.e4m3_bytes(64, 128, 1), DC.e4m3_bytes(64, 128, 2))


def test_e4m3_operands_hold_every_code_but_the_two_nans():
    for M, N, K in DC.SHAPES:
        a, _, b, _ = DC.operands(M, N, K)
        for x in (a, b):
            assert x.dtype == torch.uint8 and not bool(((x & 0x7F) == 0x7F).any())
            assert bool(x.view(DC.F8).float().isfinite().all())
    codes = DC.e4m3_bytes(1300, 512, 9).unique()
    assert codes.numel() == 254  # subnormals, both zeros and +-448 included


def test_row_scales_are_no_powers_of_two():
    for M, N, K in DC.SHAPES:
        _, sa, _, sb = DC.operands(M, N, K)
        for s in (sa, sb):
            assert s.dtype == torch.float32 and bool((s >= 0.5).all()) and bool((s < 2).all())
            assert bool(((s.view(torch.int32) & 0x7FFFFF) != 0).all())  # a mantissa: the product rounds


def test_mxfp4_scale_bytes_differ_between_blocks():
    for M, N, K in DC.SHAPES:
        if "mxfp4" not in DC.forms(K):
            continue
        w = llm.Mxfp4Weight(DC.mxfp4_source(N, K, 7 * M + N + K))
        sc = w.scales
        assert sc.unique().numel() >= 8 and not bool((sc == 0xFF).any())
        assert bool((sc[:, 1:] != sc[:, :-1]).any(-1).all())  # in every row
        assert bool(w.dequant().isfinite().all())


def test_shapes_reach_the_tail_group_the_odd_k_count_and_the_ragged_tile():
    tails, odd_k, ragged, forms = set(), [], [], set()
    for M, N, K in DC.SHAPES:
        assert N % 128 == 0 and K % 128 == 0
        tiles_m = (M + 127) // 128
        tails.add(tiles_m % DC.GROUP_M if tiles_m > DC.GROUP_M else 0)
        odd_k.append(K // 128 % 2 == 1)
        ragged.append(M % 128 != 0)
        forms.update(DC.forms(K))
        assert ("fp8_shuf" in DC.forms(K)) == ("mxfp4" in DC.forms(K)) == (K % 256 == 0)
    assert {1, 3} <= tails  # a tail group of one tile row and one of three
    assert any(odd_k) and any(ragged) and not all(ragged)
    assert forms == {"fp8_rm", "fp8_shuf", "mxfp4"}
    assert any(((M + 127) // 128) * (N // 128) > 4 * max(DC.GRIDS) for M, N, _ in DC.SHAPES)  # grid 3 walks many tiles
    assert DC.GRIDS[0] == 0 and len(DC.GRIDS) == 2

"""Shapes of the tiled MXFP4 GEMM tests (tests/test_mxfp4_gemm_cpu.py,
tests/test_gpu_mxfp4_gemm.py): k_gemm_mxfp4_tn, csrc/hip/fp4_gemm_kernels.hip.
The data come from the builders of tests/mxfp4_cases.py unchanged; this file
holds only the shape lists and thin wrappers at the tile's sizes.

k_gemm_mxfp4_tn: 128 x 128 output tile, two LDS buffers of 128 k, the K loop
unrolled over the two steps u = 0, 1 of a block of 256 k; GROUP_M = 8 row tiles
share a column panel; rows >= M are staged clamped to M - 1 and not stored.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_cases as MC  # noqa: E402

# (M, N, K): 1 / 2 / 3 / 5 / 25 blocks of 256 k (prologue only, both buffers, odd parity, a long loop), the M edges
# around a tile, and ten row tiles (the GROUP_M tail group and a ragged last tile)
INT_SHAPES = [(1, 128, 256), (127, 128, 512), (129, 256, 768), (200, 384, 1280), (384, 256, 6400), (1153, 256, 256)]
HOT_NKB = [1, 2, 3, 5]
HOT_M, HOT_N = 128, 256
RAGGED_M = [1, 17, 129, 200]
RAGGED_N = RAGGED_K = 256
REAL_M, REAL_N, REAL_K = 200, 128, [2304, 4352, 14336]
ROW_K = 4352  # the real case of the row-independence test
GATE = 1024  # M = N = K of the gating test
BAD_SHAPES = [(0, 128, 256), (64, 64, 256), (64, 0, 256), (64, 128, 384), (64, 128, 0)]  # (M, N, K) the library refuses
FALLBACK_N = 48  # no multiple of 128: tiled=True runs today's calls


def hot_phases(nkb: int):
    """Phases of HOT_M rows that visit every k of K = 256 nkb once."""
    return range(2 * nkb)


def one_hot_case(nkb: int, phase: int):
    return MC.one_hot_case(nkb, phase, M=HOT_M, N=HOT_N)


def scale_case(nkb: int, phase: int):
    return MC.scale_case(nkb, phase, M=HOT_M, N=HOT_N)


def one_hot_weight(nkb: int):
    return MC.one_hot_weight(nkb, HOT_N)


def scale_weight(nkb: int):
    return MC.scale_weight(nkb, HOT_N)


def real_case(K: int):
    return MC.real_case(REAL_M, REAL_N, K)

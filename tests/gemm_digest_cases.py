"""Real-data guard of the tiled quantised GEMMs, k_gemm_fp8_tn and
k_gemm_mxfp4_tn (csrc/hip/fp8_gemm_kernels.hip, fp4_gemm_kernels.hip, the
shared skeleton csrc/hip/gemm_q_tile.hpp): SHA-256 digests of their bf16 output
on seeded data (tests/test_gpu_gemm_digests.py against
tests/data/gemm_tiled_digests.json, the builders checked on the CPU by
tests/test_gemm_digest_cpu.py).

The exact tests use integer and one-hot data, on which every order of the fp32
sum gives the same bits.  Here the operands are random e4m3 bytes, the row
scales are no powers of two and the MXFP4 blocks span several binades, so the
digest moves with any change of the summation order, of the epilogue's
operations or of a rounding.  Every input is made on the CPU from a seeded
torch.Generator: no GPU kernel stands between the seed and the GEMM.  Only
kernels.gemm_fp8, kernels.gemm_mxfp4, llm.Fp8Weight and llm.Mxfp4Weight are
used, so `python tests/gemm_digest_cases.py` prints the same dict as one JSON
line on any commit that has the two kernels.
"""
import hashlib
import json
import os
import sys

import torch

F8 = torch.float8_e4m3fn

# (M, N, K), each for one place of the shared tile loop:
#   (200, 128, 256)   a ragged last tile, one block of 256 k
#   (129, 256, 384)   an odd count of 128-k steps (fp8 row-major B only), one row in the second tile row
#   (1152, 256, 512)  9 tile rows: the GROUP_M = 8 tail group has gsz = 1
#   (1300, 384, 512)  11 tile rows: a tail group of 3, and ragged
SHAPES = [(200, 128, 256), (129, 256, 384), (1152, 256, 512), (1300, 384, 512)]
# 0: the library's default; 3: one workgroup walks many tiles, so LDS buffers and registers are reused across tiles
GRIDS = [0, 3]
GROUP_M = 8


def forms(K: int):
    """The kernels a shape runs: the shuffled fp8 weight and MXFP4 need K % 256 == 0."""
    return ["fp8_rm"] + (["fp8_shuf", "mxfp4"] if K % 256 == 0 else [])


def e4m3_bytes(rows: int, cols: int, seed: int) -> torch.Tensor:
    """Random e4m3fn codes (uint8) with the two NaN codes 0x7f / 0xff replaced by +-1.0."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (rows, cols), generator=g, dtype=torch.uint8)
    return torch.where((b & 0x7F) == 0x7F, (b & 0x80) | 0x38, b)


def row_scales(rows: int, seed: int) -> torch.Tensor:
    """fp32 in [0.5, 2) with full mantissas: multiplying by one rounds."""
    g = torch.Generator().manual_seed(seed)
    return 0.5 + 1.5 * torch.rand(rows, generator=g, dtype=torch.float32)


def mxfp4_source(N: int, K: int, seed: int) -> torch.Tensor:
    """bf16 [N, K] whose blocks of 32 have magnitudes spread over 13 binades, so
    the E8M0 bytes of neighbouring blocks differ."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(N, K // 32, 32, generator=g, dtype=torch.float32)
    e = torch.randint(-6, 7, (N, K // 32, 1), generator=g).float()
    return (v * torch.exp2(e)).view(N, K).to(torch.bfloat16)


def operands(M: int, N: int, K: int):
    """(a bytes [M, K], sa [M], b bytes [N, K], sb [N]) of a shape, on the CPU."""
    seed = 1000003 * M + 1009 * N + K
    return e4m3_bytes(M, K, seed), row_scales(M, seed + 1), e4m3_bytes(N, K, seed + 2), row_scales(N, seed + 3)


def _sha(y: torch.Tensor) -> str:
    return hashlib.sha256(y.cpu().contiguous().view(torch.int16).numpy().tobytes()).hexdigest()


def digests(device: str = "cuda") -> dict:
    """{"<form>/<M>x<N>x<K>/grid<g>": sha256 of the bf16 output bytes}."""
    from pbs_amd.ops import kernels, llm

    out = {}
    for M, N, K in SHAPES:
        a, sa, b, sb = operands(M, N, K)
        ad, sad = a.view(F8).to(device), sa.to(device)
        for form in forms(K):
            if form == "fp8_rm":
                bd, sbd = b.view(F8).to(device), sb.to(device)
                run = lambda g: kernels.gemm_fp8(ad, sad, bd, sbd, grid=g)  # noqa: E731
            elif form == "fp8_shuf":
                w = llm.Fp8Weight.from_quantised(b.view(F8), sb)  # shuffled on the CPU
                qs, ws = w.qs.to(device), w.s.to(device)
                run = lambda g: kernels.gemm_fp8(ad, sad, qs, ws, b_shuffled=True, grid=g)  # noqa: E731
            else:
                w4 = llm.Mxfp4Weight(mxfp4_source(N, K, 7 * M + N + K))  # quantised and shuffled on the CPU
                w4.qs, w4.ss = w4.qs.to(device), w4.ss.to(device)
                run = lambda g: kernels.gemm_mxfp4(ad, sad, w4, grid=g)  # noqa: E731
            for g in GRIDS:
                out[f"{form}/{M}x{N}x{K}/grid{g}"] = _sha(run(g))
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(digests(), sort_keys=True))

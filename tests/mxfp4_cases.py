"""Shared cases of the MXFP4 linear tests (tests/test_mxfp4_cpu.py,
tests/test_gpu_mxfp4_linear.py), all built on the CPU with fixed seeds.
Kernel: csrc/hip/fp4_kernels.hip; format: pbs_amd.ops.llm.Mxfp4Weight.

k_mxfp4_gemm_skinny: wave w of 8 takes the blocks of 256 k w, w + 8 of each trip
of 16; lane (r = l & 15, g = l >> 4) holds at step u = 0, 1 the 32 codes
k = 256 block + 128 u + 32 g .. + 32 of row r (16 bytes, the even k in the low
nibble) and byte u of its scale word is their E8M0 scale.

* int_case: integer activations in [-8, 8], all 16 e2m1 codes, power-of-two
  block and row scales: every fp32 sum is exact in any order, the expected bf16
  output is one rounding of the exact value.
* one_hot_case: x row m is 1 at a single k_m, all scales 1; the weight columns
  spell k in base 4, so y[m] names the k (block, step, lane group, byte,
  nibble) that the kernel paired with row m.  Over its phases every k is visited.
* scale_case: the same x, every code +1.0, the scale byte of block j of row n
  is 127 + ((j + n) % 31 - 15): y[m, n] is that power of two and names the
  scale byte the kernel applied to the block holding k_m.
* real_case: quantised normal data, the fp64 product of the same codes and
  scales and a derived elementwise bound.
"""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as FC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

BF, F8 = FC.BF, FC.F8
NKB, M_EDGES, M_EDGE_K, CHUNK_M, RESID_M = FC.NKB, FC.M_EDGES, FC.M_EDGE_K, FC.CHUNK_M, FC.RESID_M
LIN_M, LIN_N = 64, 48
REAL_K, REAL_M, REAL_N = [2304, 4352, 14336], [5, 40], 64
E2M1 = torch.tensor(llm.MXFP4_VALUES + tuple(-v for v in llm.MXFP4_VALUES), dtype=torch.float64)  # value of code c
CODE_ONE = 2  # +1.0


def pack(nib: torch.Tensor) -> torch.Tensor:
    """Codes [N, K] (one per element, 0..15) -> bytes [N, K / 2], the even k in the low nibble."""
    n = nib.to(torch.uint8).view(nib.shape[0], -1, 2)
    return (n[..., 0] | (n[..., 1] << 4)).contiguous()


def weight64(nib: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """fp64 [N, K] of value(code) 2^e, e [N, K / 32] integers: the fixtures' own dequantisation."""
    sc = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    return (E2M1[nib.long()].view(nib.shape[0], -1, 32) * sc.unsqueeze(-1)).view(nib.shape)


# ------------------------------------------------------------------ integer case
def int_case(M: int, N: int, K: int, seed: int = 0):
    """(xq e4m3 [M, K], sx fp32 [M], codes uint8 [N, K / 2], scales uint8 [N, K / 32],
    acc fp64 [M, N]): x integers in [-8, 8], codes drawn from all 16, block
    scale 2^((n + block) % 5 - 2), sx = 2^(m % 5 - 2).  Every product is a
    multiple of 2^-3 and |acc| <= 8 * 6 * 4 K = 192 K < 2^24 * 2^-3 for
    K <= 6400, so any fp32 summation order gives acc itself."""
    assert K <= 6400
    g = torch.Generator().manual_seed(9100 + 131 * M + 17 * N + K + seed)
    x = torch.randint(-8, 9, (M, K), generator=g).double()
    nib = torch.randint(0, 16, (N, K), generator=g)
    e = (torch.arange(N)[:, None] + torch.arange(K // 32)[None, :]) % 5 - 2
    sx = torch.pow(torch.tensor(2.0), (torch.arange(M) % 5 - 2).float())
    xq = x.float().to(F8)
    assert torch.equal(xq.double(), x)
    w = weight64(nib, e)
    assert torch.equal(w * 8, (w * 8).round()) and w.abs().max().item() <= 24
    return xq, sx, pack(nib), (e + 127).to(torch.uint8), x @ w.t()


def int_resid(M: int, N: int, seed: int = 0) -> torch.Tensor:
    return FC.int_resid(M, N, seed)


def int_expect(acc, sx, resid=None) -> torch.Tensor:
    """bf16 of the exact acc sx (+ resid): the fp64 value is exact and fits fp32
    (asserted), so this is the kernel's one rounding."""
    v = acc * sx.double()[:, None]
    if resid is not None:
        v = v + resid.double()
    assert torch.equal(v.float().double(), v)
    return v.float().to(BF)


# ------------------------------------------------------------------ one-hot and scale placement
def one_hot_phases(nkb: int) -> int:
    """Phases of 64 rows that visit every k of K = 256 nkb once."""
    return 4 * nkb


def one_hot_k(nkb: int, phase: int, M: int = LIN_M) -> torch.Tensor:
    """k_m of row m in this phase: 67 j mod K for j = 64 phase + m.  67 is prime
    to K = 256 nkb (nkb <= 25), so j -> k is a bijection of [0, K) and one phase
    already spreads over blocks, steps, lane groups, bytes and nibbles."""
    K = 256 * nkb
    assert nkb < 67
    return (67 * (phase * M + torch.arange(M))) % K


DIGITS = 7  # base-4 digits of k: 4^7 = 16384 > 6400 + 5 * 5


def one_hot_nibbles(N: int, K: int) -> torch.Tensor:
    """Codes [N, K] of the one-hot weight.  Columns come in groups of 8: column
    n of group q = n // 8 holds digit n % 8 of k + 5 q in base 4 (values 0, 1,
    2, 3: codes 0, 2, 4, 5); its eighth column holds minus digit 0 (the sign bit).
    Columns 0..6 spell k itself."""
    assert K + 5 * (N // 8) < 4 ** DIGITS
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    i = n % 8
    d = ((k + 5 * (n // 8)) // 4 ** torch.where(i < DIGITS, i, torch.zeros_like(i))) % 4
    code = torch.tensor([0, 2, 4, 5])[d]
    return torch.where(i < DIGITS, code, code | 8)


def one_hot_decode(y7: torch.Tensor) -> torch.Tensor:
    """The k spelled by output columns 0..6 ([.., 7] -> [..])."""
    d = y7.double().round().long()
    return sum(d[..., i] * 4 ** i for i in range(DIGITS))


def one_hot_x(nkb: int, phase: int, M: int = LIN_M):
    K = 256 * nkb
    k = one_hot_k(nkb, phase, M)
    x = torch.zeros(M, K)
    x[torch.arange(M), k] = 1.0
    return x.to(F8), k


@functools.lru_cache(maxsize=None)
def one_hot_weight(nkb: int, N: int = LIN_N):
    """(codes uint8 [N, K / 2], scales uint8 [N, K / 32] all 127, values fp64 [N, K])."""
    K = 256 * nkb
    nib = one_hot_nibbles(N, K)
    e = torch.zeros(N, K // 32, dtype=torch.long)
    return pack(nib), (e + 127).to(torch.uint8), weight64(nib, e)


def one_hot_case(nkb: int, phase: int, M: int = LIN_M, N: int = LIN_N):
    """(xq e4m3 [M, K], k [M], expect bf16 [M, N]) for one_hot_weight(nkb, N); sx is
    1 and expect[m] = W[:, k_m]."""
    xq, k = one_hot_x(nkb, phase, M)
    return xq, k, one_hot_weight(nkb, N)[2][:, k].t().contiguous().to(BF)


@functools.lru_cache(maxsize=None)
def scale_weight(nkb: int, N: int = LIN_N):
    """(codes all +1.0, scales uint8 [N, K / 32], exponents [N, K / 32]): byte of block j
    of row n is 127 + ((j + n) % 31 - 15)."""
    K = 256 * nkb
    e = (torch.arange(K // 32)[None, :] + torch.arange(N)[:, None]) % 31 - 15
    return pack(torch.full((N, K), CODE_ONE)), (e + 127).to(torch.uint8), e


def scale_case(nkb: int, phase: int, M: int = LIN_M, N: int = LIN_N):
    """(xq, k [M], expect bf16 [M, N], exponents int [M, N]) for scale_weight(nkb, N):
    y[m, n] = 2^e of the block k_m // 32 of row n."""
    xq, k = one_hot_x(nkb, phase, M)
    e = scale_weight(nkb, N)[2][:, k // 32].t().contiguous()
    return xq, k, torch.pow(torch.tensor(2.0), e.float()).to(BF), e


# ------------------------------------------------------------------ real data
def real_case(M: int, N: int, K: int):
    """Seeded normal x quantised by quant_rows_fp8_ref, seeded 0.02 N(0, 1)
    weights quantised by mxfp4_quant_ref, ref = the fp64 product of those codes
    and scales (llm.mxfp4_linear_ref), and the elementwise bound

        |y - ref| <= 2^-8 |ref| + (1 + 2^-8) g A,   g = K u / (1 - K u), u = 2^-24,
        A = (|xq| |deq W|^T) sx.

    Every product xq deq(W) has at most 4 + 2 significant bits before its
    power-of-two scale: exact in fp32.  The kernel adds the K products of an
    output in some order (inside the MFMA, over the k loop, across the waves):
    K - 1 fp32 additions, each with relative error <= u of a partial sum that
    is at most sum |product|, then one multiplication by sx: K roundings on the
    path of any product, (1 + u)^K - 1 <= g.  So the fp32 value v before the
    output rounding has |v - ref| <= g A, and the bf16 rounding adds at most
    2^-8 |v| <= 2^-8 (|ref| + g A) (2^-9 for round to nearest; 2^-8 holds for
    any rounding).  Returns (xq, sx, W (CPU Mxfp4Weight), ref, bound)."""
    g = torch.Generator().manual_seed(7100 + 11 * M + K)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF)
    xq, sx = llm.quant_rows_fp8_ref(x)
    W = llm.Mxfp4Weight(w)
    ref = llm.mxfp4_linear_ref(xq, sx, W)
    A = xq.double().abs() @ W.dequant().double().abs().t() * sx.double()[:, None]
    ku = K * 2.0 ** -24
    bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * ku / (1 - ku) * A
    return xq, sx, W, ref, bound

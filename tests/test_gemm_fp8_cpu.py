"""Host side of the gated fp8 GEMM (csrc/hip/fp8_gemm_kernels.hip): the runner
kind number, the fp32 reference, argument validation before the library is
touched, and the shuffled-weight address formula.  Runs without a GPU."""
import pytest
import torch

from pbs_amd.ops import hipabi, llm
from pbs_amd.ops import kernels as K

F8 = torch.float8_e4m3fn


def _ints(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (rows, cols), generator=g)


def test_runner_kind_number():
    assert hipabi.KIND["gemm_fp8"] == 6


def test_gemm_fp8_ref_equals_integer_matmul():
    a, b = _ints(37, 256, 1), _ints(128, 256, 2)
    aq, bq = a.float().to(F8), b.float().to(F8)
    assert torch.equal(aq.float().long(), a) and torch.equal(bq.float().long(), b)  # exact in e4m3
    ref = K.gemm_fp8_ref(aq, torch.ones(37), bq, torch.ones(128))
    assert ref.dtype == torch.float32
    assert torch.equal(ref.long(), a @ b.t())
    # the scales multiply rows, then columns
    sa, sb = torch.arange(1, 38).float(), 2.0 ** (torch.arange(128) % 5 - 2).float()
    ref2 = K.gemm_fp8_ref(aq, sa, bq, sb)
    assert torch.equal(ref2, ((a @ b.t()).float() * sa[:, None]) * sb[None, :])


@pytest.mark.parametrize("M,N,Kd,dtype,shuf", [
    (64, 192, 256, F8, False),           # N % 128
    (64, 128, 192, F8, False),           # K % 128
    (64, 128, 256, torch.bfloat16, False),  # wrong dtype
    (64, 128, 384, F8, True),            # b_shuffled with K % 256
])
def test_gemm_fp8_rejects_bad_arguments_before_the_library(M, N, Kd, dtype, shuf, monkeypatch):
    def no_lib():
        raise AssertionError("gemm_fp8 touched the library before validating")

    monkeypatch.setattr(K, "lib", no_lib)
    aq = torch.zeros(M, Kd).to(dtype)
    bq = torch.zeros(N, Kd).to(F8)
    with pytest.raises(ValueError):
        K.gemm_fp8(aq, torch.ones(M), bq, torch.ones(N), b_shuffled=shuf)


def test_fp8_shuffled_offset_addresses_every_16_byte_piece():
    torch.manual_seed(3)
    N, Kd = 32, 512
    W = llm.Fp8Weight(torch.randn(N, Kd).bfloat16())
    flat, rm = W.qs.view(torch.uint8).reshape(-1), W.q.view(torch.uint8)
    seen = set()
    for n in range(N):
        for k in range(0, Kd, 16):
            off = llm.fp8_shuffled_offset(n, k, Kd)
            assert torch.equal(flat[off:off + 16], rm[n, k:k + 16]), (n, k, off)
            seen.add(off)
    assert seen == set(range(0, N * Kd, 16))  # a bijection onto the 16-byte pieces
    with pytest.raises(ValueError):
        llm.fp8_shuffled_offset(0, 8, Kd)

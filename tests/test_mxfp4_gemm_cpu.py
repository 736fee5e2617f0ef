"""The fixtures of the tiled MXFP4 GEMM tests at their shapes
(tests/mxfp4_gemm_cases.py over tests/mxfp4_cases.py) on the CPU, and the flags
that reach the kernel: LlamaDecoder(w4_tiled=True) and linear_q(tiled4=True)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_cases as MC  # noqa: E402
import mxfp4_gemm_cases as GC  # noqa: E402

from pbs_amd.models.llama import PRESETS, LlamaDecoder  # noqa: E402
from pbs_amd.ops import kernels, llm  # noqa: E402

BF = torch.bfloat16


# ------------------------------------------------------------------ fixtures at the new shapes
@pytest.mark.parametrize("M,N,K", GC.INT_SHAPES)
def test_integer_expectation_is_the_rounded_fp64_product(M, N, K):
    xq, sx, codes, scales, acc = MC.int_case(M, N, K)
    assert N % 128 == 0 and K % 256 == 0
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    ref = llm.mxfp4_linear_ref(xq, sx, W)
    assert torch.equal(ref.float().double(), ref)  # fits fp32: one rounding to bf16
    assert torch.equal(MC.int_expect(acc, sx), ref.float().to(BF))
    # every fp32 partial sum is exact in any order (the case's docstring): multiples of 2^-3 below 2^24 * 2^-3
    assert (xq.double().abs() @ W.dequant().double().abs().t()).max().item() < 2 ** 21


@pytest.mark.parametrize("nkb", GC.HOT_NKB)
def test_one_hot_phases_of_128_rows_visit_every_k_once(nkb):
    K = 256 * nkb
    ks = torch.cat([MC.one_hot_k(nkb, ph, GC.HOT_M) for ph in GC.hot_phases(nkb)])
    assert torch.equal(ks.sort().values, torch.arange(K))
    _, _, w = GC.one_hot_weight(nkb)
    assert w.shape == (GC.HOT_N, K)
    for ph in GC.hot_phases(nkb):
        xq, k, expect = GC.one_hot_case(nkb, ph)
        assert xq.shape == (GC.HOT_M, K) and expect.shape == (GC.HOT_M, GC.HOT_N)
        assert torch.equal(xq.float().sum(-1), torch.ones(GC.HOT_M))
        assert torch.equal(MC.one_hot_decode(expect[:, :7]), k)  # columns 0..6 spell k
        assert torch.equal(expect.double(), xq.double() @ w.t())
        # every group of 8 columns spells k + 5 q: no two k give the same row
        for q in (1, GC.HOT_N // 8 - 1):
            assert torch.equal(MC.one_hot_decode(expect[:, 8 * q:8 * q + 7]), k + 5 * q)


@pytest.mark.parametrize("nkb", GC.HOT_NKB)
def test_scale_case_names_the_byte_of_the_block_of_k(nkb):
    codes, scales, e = GC.scale_weight(nkb)
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    for ph in GC.hot_phases(nkb):
        xq, k, expect, em = GC.scale_case(nkb, ph)
        assert torch.equal(expect.double(), llm.mxfp4_linear_ref(xq, torch.ones(GC.HOT_M), W))
        assert torch.equal(em, e[:, k // 32].t())
    # the 8 blocks of a 256-k block of one row, and the same block of 16 consecutive rows, all differ
    assert all(len(set(e[n, 8 * j:8 * j + 8].tolist())) == 8 for n in (0, 17) for j in range(nkb))
    assert len(set(e[:16, 0].tolist())) == 16


@pytest.mark.parametrize("K", GC.REAL_K)
def test_an_fp32_sum_on_the_cpu_is_inside_the_real_data_bound(K):
    """The bound holds for any order of the K fp32 additions, the CPU's among
    them (measured here: 0.68 / 0.50 / 0.15 of it at K 2304 / 4352 / 14336)."""
    xq, sx, W, ref, bound = GC.real_case(K)
    assert xq.shape == (GC.REAL_M, K) and W.N == GC.REAL_N and W.N % 128 == 0
    y = ((xq.float() @ W.dequant().t()) * sx[:, None]).to(BF)
    worst = ((y.double() - ref).abs() / bound).max().item()
    print(f"K={K}: an fp32 CPU sum is at {worst:.2f} of the bound")
    assert 0 < worst <= 1


# ------------------------------------------------------------------ the flags
def test_decoder_records_w4_tiled_and_refuses_it_without_w4():
    cfg = PRESETS["tiny"]
    d = LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=True, w4_tiled=True)
    assert d.w4 is True and d.w4_tiled is True and not d.prefill_tiled
    assert isinstance(d.model.layers[0]._fp8["qkv"], llm.Mxfp4Weight)
    assert LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=True).w4_tiled is False
    assert LlamaDecoder(cfg, batch=1, context=32, device="cpu").w4_tiled is False
    for w4 in (False, "emulate"):
        with pytest.raises(ValueError, match="w4_tiled=True .*needs w4=True"):
            LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=w4, w4_tiled=True)
    with pytest.raises(ValueError, match="no tiled fp4 GEMM"):
        LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=True, w4_tiled=True, prefill_tiled=True)


def test_linear_q_reaches_the_tiled_fp4_gemm_only_through_tiled4(monkeypatch):
    xq, sx, codes, scales, _ = MC.int_case(4, 128, 256)
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    seen = []
    monkeypatch.setattr(llm, "mxfp4_linear_q", lambda xq, sx, w, resid=None, tiled=False: seen.append((tiled, resid)))
    with pytest.raises(ValueError, match="no tiled fp4 GEMM"):
        llm.linear_q(xq, sx, W, tiled=True)
    with pytest.raises(ValueError, match="no tiled fp4 GEMM"):
        llm.linear_q(xq, sx, W, tiled=True, tiled4=True)
    assert not seen
    llm.linear_q(xq, sx, W)
    llm.linear_q(xq, sx, W, tiled4=True)
    llm.linear_q(xq, sx, W, resid="r", tiled4=True)
    assert seen == [(False, None), (True, None), (True, "r")]


def test_tiled4_is_ignored_for_an_fp8_weight(monkeypatch):
    seen = []
    monkeypatch.setattr(llm, "fp8_linear_q", lambda xq, sx, w, resid=None, tiled=False: seen.append(tiled))
    w8 = llm.Fp8Weight.from_quantised(torch.zeros(16, 256).to(torch.float8_e4m3fn), torch.ones(16))
    llm.linear_q(None, None, w8, tiled4=True)
    llm.linear_q(None, None, w8, tiled=True, tiled4=True)
    assert seen == [False, True]


def test_the_new_keywords_default_to_false():
    import inspect
    from pbs_amd.models.llama import Block, Llama
    for fn in (Block.forward_fp8, Llama.forward_fp8, llm.linear_q):
        assert inspect.signature(fn).parameters["tiled4"].default is False
    for fn in (llm.mxfp4_linear_q, llm.mxfp4_linear):
        assert inspect.signature(fn).parameters["tiled"].default is False
    assert inspect.signature(LlamaDecoder.__init__).parameters["w4_tiled"].default is False


@pytest.mark.parametrize("case,match", [("cpu", "needs CUDA tensors"), ("xq_bf16", "needs e4m3fn rows"),
                                        ("sx_fp64", "needs e4m3fn rows"), ("xq_3d", "needs 2-D rows"),
                                        ("xq_k", "needs N % 128 == 0 and K % 256 == 0"),
                                        ("n_48", "needs N % 128 == 0 and K % 256 == 0"),
                                        ("sx_count", "row scales"), ("ss_cut", "weight \\["), ("qs_int8", "weight \\[")])
def test_gemm_mxfp4_checks_its_arguments_before_the_library(case, match, monkeypatch):
    def no_lib():
        raise AssertionError("the wrapper touched the library before validating")

    monkeypatch.setattr(kernels, "lib", no_lib)
    N = 48 if case == "n_48" else 128
    xq, sx, codes, scales, _ = MC.int_case(4, N, 256)
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    if case == "xq_bf16":
        xq = xq.to(BF)
    elif case == "sx_fp64":
        sx = sx.double()
    elif case == "xq_3d":
        xq = xq.view(2, 2, -1)
    elif case == "xq_k":
        xq = torch.cat([xq, xq], -1)
    elif case == "sx_count":
        sx = sx[:3].contiguous()
    elif case == "ss_cut":
        W.ss = W.ss[:, :4].contiguous()
    elif case == "qs_int8":
        W.qs = W.qs.view(torch.int8)
    with pytest.raises(ValueError, match=match):
        kernels.gemm_mxfp4(xq, sx, W)

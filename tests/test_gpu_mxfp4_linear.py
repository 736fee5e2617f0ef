"""k_mxfp4_gemm_skinny (csrc/hip/fp4_kernels.hip) on the MI355X against exact
data and fp64 references.  The fixtures and what they guarantee:
tests/mxfp4_cases.py, checked on the CPU by tests/test_mxfp4_cpu.py.  Every
reference is computed on the CPU; the device only runs the kernel."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_cases as MC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402
from pbs_amd.ops.kernels import _ptr, _stream, lib  # noqa: E402

pytestmark = pytest.mark.gpu

BF = MC.BF


def _weight(codes, scales):
    return llm.Mxfp4Weight.from_quantised(codes.cuda(), scales.cuda())


def _wrong(y, expect):
    """The (m, n) whose bf16 bits differ, for the message."""
    bad = (y.cpu().view(torch.int16) != expect.view(torch.int16)).nonzero()
    return bad.shape[0], bad[:6].tolist()


# ------------------------------------------------------------------ exact data
@pytest.mark.parametrize("nkb", MC.NKB)
def test_integer_operands_give_the_exact_product(nkb):
    """Every fp32 sum is exact whatever its order: the output is one rounding of
    the true value, for every shape of the K loop."""
    xq, sx, codes, scales, acc = MC.int_case(MC.LIN_M, MC.LIN_N, 256 * nkb)
    expect = MC.int_expect(acc, sx)
    y = llm.mxfp4_linear_q(xq.cuda(), sx.cuda(), _weight(codes, scales))
    assert y.shape == (MC.LIN_M, MC.LIN_N) and y.dtype == BF
    assert torch.equal(y.cpu(), expect), _wrong(y, expect)


@pytest.mark.parametrize("nkb", MC.NKB)
def test_one_hot_rows_select_their_weight_column(nkb):
    """y[m] = W[:, k_m] with all scales 1; columns 0..6 spell in base 4 the k that
    the kernel paired with row m.  Over the phases every k is visited, so the
    lane map of the fp4 operand, the nibble order and the shuffled layout are
    proved element by element, and a block skipped or taken twice is named."""
    codes, scales, _ = MC.one_hot_weight(nkb)
    W, one = _weight(codes, scales), torch.ones(MC.LIN_M, device="cuda")
    for ph in range(MC.one_hot_phases(nkb)):
        xq, k, expect = MC.one_hot_case(nkb, ph)
        y = llm.mxfp4_linear_q(xq.cuda(), one, W).cpu()
        rows = (y != expect).any(-1).nonzero().flatten().tolist()
        assert not rows, (f"phase={ph}: {len(rows)} wrong rows; row, k, k read by the kernel: "
                          f"{[(m, int(k[m]), int(MC.one_hot_decode(y[m, :7]))) for m in rows[:8]]}")


@pytest.mark.parametrize("nkb", MC.NKB)
def test_every_block_gets_its_own_scale_byte(nkb):
    """Every code is +1.0 and the scale byte of block j of row n is
    127 + ((j + n) % 31 - 15): y[m, n] is the power of two of the byte that the
    kernel applied to the block holding k_m (the scale layout, the lane that
    carries a scale, the byte op_sel picks)."""
    codes, scales, _ = MC.scale_weight(nkb)
    W, one = _weight(codes, scales), torch.ones(MC.LIN_M, device="cuda")
    for ph in range(MC.one_hot_phases(nkb)):
        xq, k, expect, e = MC.scale_case(nkb, ph)
        y = llm.mxfp4_linear_q(xq.cuda(), one, W).cpu()
        bad = (y != expect).nonzero()
        assert not bad.numel(), (f"phase={ph}: {bad.shape[0]} wrong; (m, n), k, exponent wanted, log2 y: "
                                 f"{[((m, n), int(k[m]), int(e[m, n]), y[m, n].float().log2().item()) for m, n in bad[:8].tolist()]}")


@pytest.mark.parametrize("M", MC.M_EDGES)
def test_m_edges_are_exact_and_rows_past_m_stay_untouched(M):
    """Both entry points of the library by pointer, with y the first M rows of a
    buffer of 64 rows holding a sentinel: the 16-row tiles past M must not be stored."""
    N, K = MC.LIN_N, MC.M_EDGE_K
    xq, sx, codes, scales, acc = MC.int_case(M, N, K)
    r = MC.int_resid(M, N)
    W, xd, sd, rd = _weight(codes, scales), xq.cuda(), sx.cuda(), r.cuda()
    L = lib()
    for resid, expect in ((None, MC.int_expect(acc, sx)), (rd, MC.int_expect(acc, sx, r))):
        buf = torch.full((64, N), -768.0, dtype=BF, device="cuda")
        if resid is None:
            rc = L.gpbs_hip_mxfp4_linear(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.ss), _ptr(buf), M, N, K, _stream())
        else:
            rc = L.gpbs_hip_mxfp4_linear_res(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.ss), _ptr(buf), _ptr(resid), M, N,
                                             K, _stream())
        assert rc == 0
        got = buf.cpu()
        assert torch.equal(got[:M], expect), (resid is not None, _wrong(got[:M], expect))
        assert torch.equal(got[M:], torch.full((64 - M, N), -768.0, dtype=BF)), "rows >= M were written"


@pytest.mark.parametrize("M", MC.CHUNK_M)
def test_chunk_loop_of_the_wrapper_is_exact(M):
    """mxfp4_linear_q splits M > 64 into launches of 64 rows and a rest."""
    xq, sx, codes, scales, acc = MC.int_case(M, MC.LIN_N, MC.M_EDGE_K)
    expect = MC.int_expect(acc, sx)
    W = _weight(codes, scales)
    y = llm.mxfp4_linear_q(xq.cuda(), sx.cuda(), W)
    assert torch.equal(y.cpu(), expect), _wrong(y, expect)
    y3 = llm.mxfp4_linear_q(xq.cuda().view(M, 1, -1), sx.cuda().view(M, 1), W)
    assert y3.shape == (M, 1, MC.LIN_N) and torch.equal(y3.cpu().view(M, -1), expect)


@pytest.mark.parametrize("M", MC.RESID_M)
def test_fused_residual_is_added_after_the_scaling(M):
    """Integer residual, power-of-two scales: (acc sx + resid) is exact in fp32, so
    the bf16 output is known bit for bit (and differs from (acc + resid) sx
    wherever sx is not 1)."""
    for K in (MC.M_EDGE_K, 256 * 17):
        xq, sx, codes, scales, acc = MC.int_case(M, MC.LIN_N, K)
        r = MC.int_resid(M, MC.LIN_N)
        expect = MC.int_expect(acc, sx, r)
        rd = r.cuda()
        y = llm.mxfp4_linear_q(xq.cuda(), sx.cuda(), _weight(codes, scales), resid=rd)
        assert torch.equal(y.cpu(), expect), (K, _wrong(y, expect))
        assert torch.equal(rd.cpu(), r)  # read, not written


def test_a_row_is_bit_equal_whatever_m_it_is_launched_in():
    """Row 3 alone (as the only row), in M = 17 and in M = 64 (one, two and four M
    tiles) on real data: the same bits."""
    xq, sx, W, _, _ = _real(40, 4352)
    g = torch.Generator().manual_seed(11)
    x64 = xq.view(torch.uint8)[torch.randint(0, 40, (64,), generator=g)].view(MC.F8)
    s64 = sx[torch.randint(0, 40, (64,), generator=g)].contiguous()
    Wd, xd, sd = _weight(W.codes, W.scales), x64.cuda(), s64.cuda()
    y64 = llm.mxfp4_linear_q(xd, sd, Wd)
    y17 = llm.mxfp4_linear_q(xd[:17].contiguous(), sd[:17].contiguous(), Wd)
    y1 = llm.mxfp4_linear_q(xd[3:4].contiguous(), sd[3:4].contiguous(), Wd)
    assert torch.equal(y1[0], y17[3]) and torch.equal(y1[0], y64[3])
    assert torch.equal(y17, y64[:17])


# ------------------------------------------------------------------ real data
@functools.lru_cache(maxsize=None)
def _real(M, K):
    return MC.real_case(M, MC.REAL_N, K)


@pytest.mark.parametrize("M", MC.REAL_M)
@pytest.mark.parametrize("K", MC.REAL_K)
def test_real_data_stays_inside_the_derived_bound(K, M):
    """Against the fp64 product of the same codes and scales, per element:
    |y - ref| <= 2^-8 |ref| + (1 + 2^-8) g (|xq| |deq W|^T) sx, g = K 2^-24 / (1 - K 2^-24)
    (mxfp4_cases.real_case has the derivation)."""
    xq, sx, W, ref, bound = _real(M, K)
    y = llm.mxfp4_linear_q(xq.cuda(), sx.cuda(), _weight(W.codes, W.scales))
    err = (y.cpu().double() - ref).abs()
    print(f"K={K} M={M}: largest fraction of the bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()
    y2 = llm.mxfp4_linear((xq.float() * sx[:, None]).to(BF).cuda(), _weight(W.codes, W.scales))
    assert y2.shape == y.shape and y2.dtype == BF


# ------------------------------------------------------------------ wrapper and library argument checks
def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


@pytest.mark.parametrize("case,match", [("w_cpu", "weight must be a CUDA tensor"), ("xq_cpu", "xq must be a CUDA"),
                                        ("sx_cpu", "sx must be a CUDA tensor"), ("resid_cpu", "resid must be a CUDA"),
                                        ("sx_fp64", "sx must be contiguous fp32"), ("no_rows", "has no rows"),
                                        ("xq_k", "need contiguous e4m3fn"), ("xq_bf16", "need contiguous e4m3fn"),
                                        ("sx_count", "sx must be contiguous fp32"), ("resid_shape", "resid must be"),
                                        ("resid_fp32", "resid must be"), ("scales_cut", "weight \\[")])
def test_mxfp4_linear_q_rejects_cpu_tensors_and_mismatched_shapes(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    xq, sx, codes, scales, _ = MC.int_case(4, MC.LIN_N, 256)
    W = llm.Mxfp4Weight.from_quantised(codes, scales) if case == "w_cpu" else _weight(codes, scales)
    xd, sd, rd = xq.cuda(), sx.cuda(), None
    if case == "xq_cpu":
        xd = xq
    elif case == "sx_cpu":
        sd = sx
    elif case == "resid_cpu":
        rd = MC.int_resid(4, MC.LIN_N)
    elif case == "sx_fp64":
        sd = sd.double()
    elif case == "no_rows":
        xd, sd = xd[:0], sd[:0]
    elif case == "xq_k":
        xd = torch.cat([xd, xd], -1)
    elif case == "xq_bf16":
        xd = xd.to(BF)
    elif case == "sx_count":
        sd = sd[:3].contiguous()
    elif case == "resid_shape":
        rd = MC.int_resid(4, MC.LIN_N + 16).cuda()
    elif case == "resid_fp32":
        rd = MC.int_resid(4, MC.LIN_N).cuda().float()
    elif case == "scales_cut":
        W.ss = W.ss[:, :4].contiguous()
    with pytest.raises(ValueError, match=match):
        llm.mxfp4_linear_q(xd, sd, W, resid=rd)


def test_library_refuses_shapes_it_cannot_launch():
    """-22 before any launch: M = 0, M = 65, N % 16 != 0, K % 256 != 0."""
    xq, sx, codes, scales, _ = MC.int_case(MC.LIN_M, MC.LIN_N, 512)
    W, xd, sd = _weight(codes, scales), xq.cuda(), sx.cuda()
    y = torch.full((80, MC.LIN_N), -768.0, dtype=BF, device="cuda")
    L = lib()
    for M, N, K in ((0, 48, 512), (65, 48, 512), (64, 40, 512), (64, 48, 384), (64, 0, 512), (64, 48, 0)):
        assert L.gpbs_hip_mxfp4_linear(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.ss), _ptr(y), M, N, K, _stream()) == -22
        assert L.gpbs_hip_mxfp4_linear_res(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.ss), _ptr(y), _ptr(y), M, N, K,
                                           _stream()) == -22
    assert bool((y == -768.0).all())
    with pytest.raises(ValueError, match="M <= 64"):
        llm.mxfp4_linear_q(torch.cat([xd, xd]), torch.cat([sd, sd]), W,
                           resid=torch.zeros(128, MC.LIN_N, dtype=BF, device="cuda"))

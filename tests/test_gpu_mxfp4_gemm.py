"""k_gemm_mxfp4_tn (csrc/hip/fp4_gemm_kernels.hip), the tiled MXFP4 GEMM, on
the MI355X against exact data and fp64 references.  The data are those of the
skinny kernel's tests (tests/mxfp4_cases.py) at the shapes of
tests/mxfp4_gemm_cases.py, checked on the CPU by tests/test_mxfp4_gemm_cpu.py.
Every reference is computed on the CPU; the device only runs the kernel."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_cases as MC  # noqa: E402
import mxfp4_gemm_cases as GC  # noqa: E402

from pbs_amd.ops import kernels as K  # noqa: E402
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
@pytest.mark.parametrize("M,N,Kd", GC.INT_SHAPES)
def test_integer_operands_give_the_exact_product(M, N, Kd):
    """Every fp32 sum is exact whatever its order: the output is one rounding of
    the true value for every shape of the K loop and every M edge, through the
    kernel's wrapper, through mxfp4_linear_q(tiled=True), and equal to the
    sliced mxfp4_linear_q."""
    xq, sx, codes, scales, acc = MC.int_case(M, N, Kd)
    expect = MC.int_expect(acc, sx)
    W, xd, sd = _weight(codes, scales), xq.cuda(), sx.cuda()
    y = K.gemm_mxfp4(xd, sd, W)
    assert y.shape == (M, N) and y.dtype == BF
    assert torch.equal(y.cpu(), expect), _wrong(y, expect)
    yt = llm.mxfp4_linear_q(xd, sd, W, tiled=True)
    assert yt.shape == (M, N) and torch.equal(yt.cpu(), expect), _wrong(yt, expect)
    assert torch.equal(yt, llm.mxfp4_linear_q(xd, sd, W))
    if M % 3 == 0:  # leading dimensions are kept
        y3 = llm.mxfp4_linear_q(xd.view(3, M // 3, Kd), sd.view(3, M // 3), W, tiled=True)
        assert y3.shape == (3, M // 3, N) and torch.equal(y3.view(M, N), yt)


@pytest.mark.parametrize("nkb", GC.HOT_NKB)
def test_one_hot_rows_select_their_weight_column(nkb):
    """y[m] = W[:, k_m] with all scales 1; columns 0..6 of every group of 8 spell
    in base 4 the k that the kernel paired with row m.  Over the phases every k
    is visited: the chunks of the e4m3 fragment (g and 4 + g, not 2 g and
    2 g + 1), the nibble order and the strip address are proved element by
    element, and a step skipped or taken twice is named."""
    codes, scales, _ = GC.one_hot_weight(nkb)
    W, one = _weight(codes, scales), torch.ones(GC.HOT_M, device="cuda")
    for ph in GC.hot_phases(nkb):
        xq, k, expect = GC.one_hot_case(nkb, ph)
        y = K.gemm_mxfp4(xq.cuda(), one, W).cpu()
        rows = (y != expect).any(-1).nonzero().flatten().tolist()
        assert not rows, (f"phase={ph}: {len(rows)} wrong rows; row, k, k read by the kernel: "
                          f"{[(m, int(k[m]), int(MC.one_hot_decode(y[m, :7]))) for m in rows[:8]]}")


@pytest.mark.parametrize("nkb", GC.HOT_NKB)
def test_every_block_gets_its_own_scale_byte(nkb):
    """Every code is +1.0 and the scale byte of block j of row n is
    127 + ((j + n) % 31 - 15): y[m, n] is the power of two of the byte that the
    kernel applied to the block holding k_m (the scale address, the lane that
    carries a scale, the byte op_sel picks at each of the two steps)."""
    codes, scales, _ = GC.scale_weight(nkb)
    W, one = _weight(codes, scales), torch.ones(GC.HOT_M, device="cuda")
    for ph in GC.hot_phases(nkb):
        xq, k, expect, e = GC.scale_case(nkb, ph)
        y = K.gemm_mxfp4(xq.cuda(), one, W).cpu()
        bad = (y != expect).nonzero()
        assert not bad.numel(), (f"phase={ph}: {bad.shape[0]} wrong; (m, n), k, exponent wanted, log2 y: "
                                 f"{[((m, n), int(k[m]), int(e[m, n]), y[m, n].float().log2().item()) for m, n in bad[:8].tolist()]}")


@pytest.mark.parametrize("M", GC.RAGGED_M)
def test_rows_past_m_stay_untouched(M):
    """The library by pointer, with y the first M rows of a buffer that reaches 8
    rows past the last tile and holds a sentinel."""
    N, Kd = GC.RAGGED_N, GC.RAGGED_K
    xq, sx, codes, scales, acc = MC.int_case(M, N, Kd)
    W, xd, sd = _weight(codes, scales), xq.cuda(), sx.cuda()
    rows = (M + 127) // 128 * 128 + 8
    buf = torch.full((rows, N), -768.0, dtype=BF, device="cuda")
    q = K.work_queue("cuda")
    rc = lib().gpbs_hip_gemm_mxfp4(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.ss), _ptr(buf), M, N, Kd, _ptr(q), None,
                                   K.GATE_NONE, 0, None, None, 0, _stream())
    assert rc == 0
    got, expect = buf.cpu(), MC.int_expect(acc, sx)
    assert torch.equal(got[:M], expect), _wrong(got[:M], expect)
    assert torch.equal(got[M:], torch.full((rows - M, N), -768.0, dtype=BF)), "rows >= M were written"
    out = K.gemm_mxfp4(xd, sd, W, out=buf[:M])
    assert out.data_ptr() == buf.data_ptr()


# ------------------------------------------------------------------ real data
@functools.lru_cache(maxsize=None)
def _real(Kd):
    return GC.real_case(Kd)


def test_a_row_is_bit_equal_whatever_m_it_is_launched_in():
    """Rows 0..128 launched as M = 129 (a full tile and a tile of one row) and
    row 3 launched alone equal the same rows of the M = 200 launch, on real data."""
    xq, sx, W, _, _ = _real(GC.ROW_K)
    Wd, xd, sd = _weight(W.codes, W.scales), xq.cuda(), sx.cuda()
    y200 = K.gemm_mxfp4(xd, sd, Wd)
    y129 = K.gemm_mxfp4(xd[:129].contiguous(), sd[:129].contiguous(), Wd)
    y1 = K.gemm_mxfp4(xd[3:4].contiguous(), sd[3:4].contiguous(), Wd)
    assert torch.equal(y129, y200[:129])
    assert torch.equal(y1[0], y200[3])


@pytest.mark.parametrize("Kd", GC.REAL_K)
def test_real_data_stays_inside_the_derived_bound(Kd):
    """Against the fp64 product of the same codes and scales, per element:
    |y - ref| <= 2^-8 |ref| + (1 + 2^-8) g (|xq| |deq W|^T) sx, g = K 2^-24 / (1 - K 2^-24)
    (mxfp4_cases.real_case has the derivation: K fp32 roundings on exact
    products plus the output rounding, which is this kernel as written)."""
    xq, sx, W, ref, bound = _real(Kd)
    Wd = _weight(W.codes, W.scales)
    y = K.gemm_mxfp4(xq.cuda(), sx.cuda(), Wd)
    err = (y.cpu().double() - ref).abs()
    print(f"K={Kd} M={GC.REAL_M}: largest fraction of the bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()
    y2 = llm.mxfp4_linear((xq.float() * sx[:, None]).to(BF).cuda(), Wd, tiled=True)
    assert y2.shape == y.shape and y2.dtype == BF


# ------------------------------------------------------------------ gating
def test_gating_confines_the_gemm_to_owned_xcds():
    from pbs_amd.runtime.gpu import GpuContext
    ctx = GpuContext(0)
    owners = [5, 5, 7, 7, 7, 7, -1, 5]
    ctx.set_owners(owners)
    n = GC.GATE
    xq, sx, codes, scales, acc = MC.int_case(n, n, n)
    out = K.gemm_mxfp4(xq.cuda(), sx.cuda(), _weight(codes, scales), table=ctx.table, tenant=5, counters=ctx.counters)
    torch.cuda.synchronize()
    expect = MC.int_expect(acc, sx)
    assert torch.equal(out.cpu(), expect), _wrong(out, expect)
    per = ctx.read_counters(5, per_xcd=True)
    for x in range(8):
        if owners[x] == 5:
            continue
        assert per[x] == (0, 0, 0, 0), (x, per[x])
    assert sum(p[0] for p in per) > 0
    ctx.close()


# ------------------------------------------------------------------ wrapper and library argument checks
def test_library_refuses_shapes_it_cannot_launch():
    """-22 before any launch: M = 0, N = 64, N = 0, K = 384, K = 0."""
    xq, sx, codes, scales, _ = MC.int_case(64, 128, 512)
    W, xd, sd = _weight(codes, scales), xq.cuda(), sx.cuda()
    y = torch.full((136, 128), -768.0, dtype=BF, device="cuda")
    q = K.work_queue("cuda")
    for M, N, Kd in GC.BAD_SHAPES:
        assert lib().gpbs_hip_gemm_mxfp4(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.ss), _ptr(y), M, N, Kd, _ptr(q), None,
                                         K.GATE_NONE, 0, None, None, 0, _stream()) == -22, (M, N, Kd)
    torch.cuda.synchronize()
    assert bool((y == -768.0).all())


def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


@pytest.mark.parametrize("case,match", [("w_cpu", "CUDA tensor"), ("xq_cpu", "CUDA tensor"), ("sx_cpu", "CUDA tensor"),
                                        ("xq_bf16", "e4m3fn"), ("sx_fp64", "fp32"), ("xq_k", "e4m3fn|K % 256"),
                                        ("sx_count", "sx must be|row scales"), ("ss_cut", "weight \\["),
                                        ("out_shape", "out must be"), ("out_fp32", "out must be"),
                                        ("out_cpu", "out must be")])
def test_wrappers_reject_bad_arguments_before_the_library(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    monkeypatch.setattr(K, "lib", _no_lib)
    xq, sx, codes, scales, _ = MC.int_case(4, 128, 256)
    W = llm.Mxfp4Weight.from_quantised(codes, scales) if case == "w_cpu" else _weight(codes, scales)
    xd, sd, out = xq.cuda(), sx.cuda(), None
    if case == "xq_cpu":
        xd = xq
    elif case == "sx_cpu":
        sd = sx
    elif case == "xq_bf16":
        xd = xd.to(BF)
    elif case == "sx_fp64":
        sd = sd.double()
    elif case == "xq_k":
        xd = torch.cat([xd, xd], -1)
    elif case == "sx_count":
        sd = sd[:3].contiguous()
    elif case == "ss_cut":
        W.ss = W.ss[:, :4].contiguous()
    elif case == "out_shape":
        out = torch.empty(4, 256, dtype=BF, device="cuda")
    elif case == "out_fp32":
        out = torch.empty(4, 128, dtype=torch.float32, device="cuda")
    elif case == "out_cpu":
        out = torch.empty(4, 128, dtype=BF)
    with pytest.raises(ValueError, match=match):
        K.gemm_mxfp4(xd, sd, W, out)
    if out is None:
        with pytest.raises(ValueError, match=match):
            llm.mxfp4_linear_q(xd, sd, W, tiled=True)


def test_tiled_falls_back_to_the_sliced_calls_with_a_residual_or_a_narrow_n(monkeypatch):
    """tiled=True with a residual, or with N = 48 (no multiple of 128), issues
    today's calls: the sliced result's bits and no gemm_mxfp4 launch."""
    def no_gemm(*a, **k):
        raise AssertionError("the fall-back launched the tiled GEMM")

    M = 64
    xq, sx, codes, scales, _ = MC.int_case(M, 128, 512)
    W, xd, sd, rd = _weight(codes, scales), xq.cuda(), sx.cuda(), MC.int_resid(M, 128).cuda()
    x2, s2, c2, sc2, _ = MC.int_case(200, GC.FALLBACK_N, 512)
    W2, x2d, s2d = _weight(c2, sc2), x2.cuda(), s2.cuda()
    want, want2 = llm.mxfp4_linear_q(xd, sd, W, resid=rd), llm.mxfp4_linear_q(x2d, s2d, W2)
    monkeypatch.setattr(llm, "gemm_mxfp4", no_gemm)
    assert torch.equal(llm.mxfp4_linear_q(xd, sd, W, resid=rd, tiled=True), want)
    y2 = llm.mxfp4_linear_q(x2d, s2d, W2, tiled=True)
    assert y2.shape == (200, GC.FALLBACK_N) and torch.equal(y2, want2)
    with pytest.raises(AssertionError, match="launched the tiled GEMM"):
        llm.mxfp4_linear_q(xd, sd, W, tiled=True)

"""k_fp8_gemm_skinny and the fp8 row quantisers (csrc/hip/fp8_kernels.hip) on the
MI355X against exact data and fp64 references.  The fixtures and what they
guarantee: tests/fp8_cases.py, checked on the CPU by tests/test_fp8_cases_cpu.py.
Every reference is computed on the CPU; the device only runs the kernels."""
import contextlib
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as FC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402
from pbs_amd.ops.kernels import _ptr, _stream, lib  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F8 = FC.BF, FC.F8


def _u8(q):
    return q.contiguous().view(torch.uint8).cpu()


def _by_value(c):
    return torch.where(c == 0x80, torch.zeros_like(c), c)


@contextlib.contextmanager
def _opts(o):
    """Select a launch variant of the skinny linear; the old one comes back."""
    prev = lib().gpbs_hip_fp8_set_opts(o)
    try:
        yield
    finally:
        lib().gpbs_hip_fp8_set_opts(prev)


def _weight(wq, sw):
    return llm.Fp8Weight.from_quantised(wq.cuda(), sw.cuda())


def _wrong(y, expect):
    """The (m, n) whose bf16 bits differ, for the message."""
    bad = (y.cpu().view(torch.int16) != expect.view(torch.int16)).nonzero()
    return bad.shape[0], bad[:6].tolist()


# ------------------------------------------------------------------ skinny linear, exact
@pytest.mark.parametrize("nkb", FC.NKB)
def test_integer_operands_give_the_exact_product(nkb):
    """Every fp32 sum is exact whatever its order: the output is one rounding of
    the true value, for every launch variant and every shape of the K loop."""
    xq, sx, wq, sw, acc = FC.int_linear_case(FC.LIN_M, FC.LIN_N, 256 * nkb)
    expect = FC.int_expect(acc, sx, sw)
    W, xd, sd = _weight(wq, sw), xq.cuda(), sx.cuda()
    for o in FC.OPTS:
        with _opts(o):
            y = llm.fp8_linear_q(xd, sd, W)
        assert y.shape == (FC.LIN_M, FC.LIN_N) and y.dtype == BF
        assert torch.equal(y.cpu(), expect), (o, _wrong(y, expect))


@pytest.mark.parametrize("nkb", FC.NKB)
def test_one_hot_rows_select_their_weight_column(nkb):
    """y[m] = W[:, k_m]; columns 0..3 spell in base 17 the k that the kernel paired
    with row m, so a mismatch of the A permutation and the shuffled B layout, or
    a block that is skipped or taken twice, is named."""
    one = torch.ones(FC.LIN_M, device="cuda")
    sw = torch.ones(FC.LIN_N)
    for ph in range(FC.one_hot_phases(nkb)):
        xq, wq, k, expect = FC.one_hot_case(nkb, ph)
        W, xd = _weight(wq, sw), xq.cuda()
        for o in FC.OPTS:
            with _opts(o):
                y = llm.fp8_linear_q(xd, one, W).cpu()
            rows = (y != expect).any(-1).nonzero().flatten().tolist()
            assert not rows, (f"opts={o} phase={ph}: {len(rows)} wrong rows; row, k, k read by the kernel: "
                              f"{[(m, int(k[m]), int(FC.one_hot_decode(y[m, :4]))) for m in rows[:8]]}")


@pytest.mark.parametrize("o", [0, 2])
@pytest.mark.parametrize("M", FC.M_EDGES)
def test_m_edges_are_exact_and_rows_past_m_stay_untouched(M, o):
    """Both entry points of the library, with y the first M rows of a buffer that
    has 8 rows to spare: the 16-row tiles past M must not be stored."""
    N, K = FC.LIN_N, FC.M_EDGE_K
    xq, sx, wq, sw, acc = FC.int_linear_case(M, N, K)
    r = FC.int_resid(M, N)
    W, xd, sd, rd = _weight(wq, sw), xq.cuda(), sx.cuda(), r.cuda()
    L = lib()
    with _opts(o):
        for resid, expect in ((None, FC.int_expect(acc, sx, sw)), (rd, FC.int_expect(acc, sx, sw, r))):
            buf = torch.full((M + 8, N), -768.0, dtype=BF, device="cuda")
            if resid is None:
                rc = L.gpbs_hip_fp8_linear(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.s), _ptr(buf), M, N, K, _stream())
            else:
                rc = L.gpbs_hip_fp8_linear_res(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.s), _ptr(buf), _ptr(resid), M,
                                               N, K, _stream())
            assert rc == 0
            got = buf.cpu()
            assert torch.equal(got[:M], expect), (resid is not None, _wrong(got[:M], expect))
            assert torch.equal(got[M:], torch.full((8, N), -768.0, dtype=BF)), "rows >= M were written"


@pytest.mark.parametrize("M", FC.CHUNK_M)
def test_chunk_loop_of_the_wrapper_is_exact(M):
    """fp8_linear_q splits M > 64 into launches of 64 rows and a rest."""
    xq, sx, wq, sw, acc = FC.int_linear_case(M, FC.LIN_N, FC.M_EDGE_K)
    expect = FC.int_expect(acc, sx, sw)
    y = llm.fp8_linear_q(xq.cuda(), sx.cuda(), _weight(wq, sw))
    assert torch.equal(y.cpu(), expect), _wrong(y, expect)
    y3 = llm.fp8_linear_q(xq.cuda().view(M, 1, -1), sx.cuda().view(M, 1), _weight(wq, sw))
    assert y3.shape == (M, 1, FC.LIN_N) and torch.equal(y3.cpu().view(M, -1), expect)


@pytest.mark.parametrize("M", FC.RESID_M)
def test_fused_residual_is_added_after_the_scaling(M):
    """Integer residual, power-of-two scales: (acc sx sw + resid) is exact in
    fp32, so the bf16 output is known bit for bit (and differs from
    (acc + resid) sx sw wherever the scale is not 1)."""
    for K in (FC.M_EDGE_K, 256 * 17):
        xq, sx, wq, sw, acc = FC.int_linear_case(M, FC.LIN_N, K)
        r = FC.int_resid(M, FC.LIN_N)
        expect = FC.int_expect(acc, sx, sw, r)
        W, xd, sd, rd = _weight(wq, sw), xq.cuda(), sx.cuda(), r.cuda()
        for o in FC.OPTS:
            with _opts(o):
                y = llm.fp8_linear_q(xd, sd, W, resid=rd)
            assert torch.equal(y.cpu(), expect), (K, o, _wrong(y, expect))
            assert torch.equal(rd.cpu(), r)  # read, not written


# ------------------------------------------------------------------ skinny linear, real data
@functools.lru_cache(maxsize=None)
def _real(M, K):
    return FC.real_linear_case(M, FC.REAL_N, K, llm.quant_rows_fp8_ref)


@pytest.mark.parametrize("M", FC.REAL_M)
@pytest.mark.parametrize("K", FC.REAL_K)
def test_real_data_stays_inside_the_derived_bound(K, M):
    """Against the fp64 product of the same codes and scales, per element:
    |y - ref| <= 2^-8 |ref| + K 2^-24 (|xq| |wq|^T) sx sw (fp8_cases.real_linear_case)."""
    xq, sx, wq, sw, ref, bound = _real(M, K)
    W, xd, sd = _weight(wq, sw), xq.cuda(), sx.cuda()
    for o in FC.OPTS:
        with _opts(o):
            y = llm.fp8_linear_q(xd, sd, W)
        err = (y.cpu().double() - ref).abs()
        print(f"K={K} M={M} opts={o}: largest fraction of the bound {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), (o, (err / bound).max().item())


# ------------------------------------------------------------------ k_quant_rows_fp8
def _quant(x):
    q, s = llm.quant_rows_fp8(x.cuda())
    return _u8(q), s.cpu()


@pytest.mark.parametrize("K", FC.QUANT_K)
def test_quantiser_returns_all_codes_rows_unchanged(K):
    """amax = 448, inv = scale = 1: the convert alone decides, for every finite
    code (subnormals and both zeros included) in every slot of the packed convert."""
    x, codes = FC.all_codes_case(K)
    q, s = _quant(x)
    bad = (q != codes).nonzero()
    assert bad.numel() == 0, [(i, j, hex(codes[i, j]), hex(q[i, j])) for i, j in bad[:8].tolist()]
    assert torch.equal(s, torch.ones(x.shape[0]))


def test_quantiser_rounds_ties_to_even():
    x, expect = FC.tie_case()
    q, s = _quant(x)
    bad = (q != expect).nonzero()
    assert bad.numel() == 0, [(x[i, j].item(), hex(expect[i, j]), hex(q[i, j])) for i, j in bad[:8].tolist()]
    assert torch.equal(s, torch.ones(4))


@pytest.mark.parametrize("K", FC.QUANT_K)
def test_quantiser_finds_the_maximum_wherever_it_sits(K):
    x, codes, pos = FC.placement_case(K)
    q, s = _quant(x)
    assert torch.equal(s, torch.ones(len(pos) + 1)), [(pos[i] if i < len(pos) else None, s[i].item())
                                                      for i in (s != 1).nonzero().flatten().tolist()]
    assert torch.equal(q, codes)
    q1, s1 = _quant(x[:1])  # rows = 1
    assert torch.equal(q1, codes[:1]) and s1.tolist() == [1.0]


@pytest.mark.parametrize("K", FC.RANDOM_K)
def test_quantiser_matches_the_mirrored_reference_bit_for_bit(K):
    """Normal data, 67 rows: codes and scales equal those of quant_rows_fp8_ref
    (the same fp32 operations in the same order), and independently every code
    is within half an e4m3 step plus 2^-20 relative of the fp64 value
    x 448 / amax (two fp32 roundings before the convert)."""
    x = FC.random_rows(67, K, seed=5)
    q, s = _quant(x)
    qr, sr = llm.quant_rows_fp8_ref(x)
    t, s64 = FC.quant64(x)
    err, bound = FC.code_excess(q, t, 2.0 ** -20)
    diff = q != _u8(qr)
    print(f"K={K}: {int(diff.sum())} of {diff.numel()} codes differ from quant_rows_fp8_ref, "
          f"{int((s != sr).sum())} of 67 scales; beyond half a step: {FC.rel_used(q, t, 2.0 ** -20):.3f} "
          f"of the 2^-20 allowance")
    assert torch.equal(s, sr) and torch.equal(s, s64.float())
    assert bool((err <= bound).all())
    assert not diff.any(), [(x[i, j].item(), sr[i].item(), hex(_u8(qr)[i, j]), hex(q[i, j]))
                            for i, j in diff.nonzero()[:8].tolist()]


# ------------------------------------------------------------------ k_rmsnorm_quant_fp8
@pytest.mark.parametrize("K", FC.QUANT_K)
def test_rmsnorm_quantiser_exact_case(K):
    """x = +-1, eps = 0: mean(x^2) is exactly 1 and the row is +-w, all e4m3
    values; the 448 of w visits every edge and every wave's first element."""
    for peak in FC.placement_positions(K):
        x, w, codes = FC.rmsnorm_exact_case(K, peak)
        q, s = llm.rmsnorm_quant_fp8(x.cuda(), w.cuda(), 0.0)
        q, s = _u8(q), s.cpu()
        assert torch.equal(q, codes), (peak, int((q != codes).sum()))
        assert (s - 1).abs().max().item() <= 2 * 2.0 ** -23, (peak, s.tolist())  # 2 ulp of 1: rsqrtf may be 1 off


@pytest.mark.parametrize("K", FC.RANDOM_K)
def test_rmsnorm_quantiser_tracks_fp64(K):
    """x normal, w = 1 + 0.1 normal, 9 rows.  2^-16 relative covers the fp32 sum
    of squares (at most ~140 additions of non-negative terms per thread and in
    the tree: 140 x 2^-24 < 2^-16.8, halved by the square root), rsqrtf to 1 ulp
    and the four roundings of x rs w inv."""
    x, w = FC.rmsnorm_random_case(K)
    q, s = llm.rmsnorm_quant_fp8(x.cuda(), w.cuda(), 1e-5)
    t, s64 = FC.quant64(FC.rmsnorm64(x, w, 1e-5))
    srel = ((s.cpu().double() - s64).abs() / s64).max().item()
    err, bound = FC.code_excess(_u8(q), t, 2.0 ** -16)
    print(f"K={K}: scale error {srel * 2 ** 16:.3f} x 2^-16, codes beyond half a step: "
          f"{FC.rel_used(_u8(q), t, 2.0 ** -16):.3f} of the 2^-16 allowance")
    assert srel <= 2.0 ** -16
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ k_swiglu_quant_fp8
@pytest.mark.parametrize("F", FC.SWIGLU_F)
def test_swiglu_quantiser_exact_case(F):
    """gate in {0, 32}: silu(32) is 32 in fp32, y is a code of `up` or a zero
    (compared by value behind a closed gate, bit for bit behind an open one)."""
    gu, codes, on = FC.swiglu_exact_case(F)
    q, s = llm.swiglu_quant_fp8(gu.cuda())
    q, s = _u8(q), s.cpu()
    expect = torch.where(on, codes, torch.zeros_like(codes))
    assert torch.equal(s, torch.ones(3)), s.tolist()
    assert torch.equal(q[on], codes[on]), int((q[on] != codes[on]).sum())
    assert torch.equal(_by_value(q), _by_value(expect))


@pytest.mark.parametrize("F", FC.SWIGLU_F)
def test_swiglu_quantiser_finds_the_maximum_in_all_16_waves(F):
    gu, codes, pos = FC.swiglu_placement_case(F)
    q, s = llm.swiglu_quant_fp8(gu.cuda())
    q, s = _u8(q), s.cpu()
    assert torch.equal(s, torch.ones(len(pos) + 1)), [(pos[i] if i < len(pos) else None, s[i].item())
                                                      for i in (s != 1).nonzero().flatten().tolist()]
    assert torch.equal(q[:-1], codes[:-1]) and not _by_value(q[-1]).any()
    q1, s1 = llm.swiglu_quant_fp8(gu[:1].cuda())
    assert torch.equal(_u8(q1), codes[:1]) and s1.tolist() == [1.0]


@pytest.mark.parametrize("F", FC.RANDOM_F)
def test_swiglu_quantiser_tracks_fp64(F):
    """Normal data, 5 rows, against fp64 to 2^-18 relative.  The kernel computes
    silu(v) = v / (1 + __expf(-v)); the HIP headers define __expf(x) as the
    hardware exp2 of x log2(e) rounded to fp32.  The rounded constant and
    product put 1.5 x 2^-24 |x| log2(e) into the exponent, which exp2 turns into
    1.5 x 2^-24 |x| relative; the exp2 instruction is good to 1 ulp (2^-23).
    For |gate| <= 8 (asserted) that is <= 14 x 2^-24 in e = exp(-v), no more in
    1 + e, plus one rounding each for the sum, the division and the product
    with `up`: y is within 17 x 2^-24.  amax carries the same error and inv and
    y inv two more roundings: 36 x 2^-24 < 2^-18 on the value a code rounds."""
    gu = FC.swiglu_random_case(F)
    assert gu[:, :F].float().abs().max().item() <= 8
    q, s = llm.swiglu_quant_fp8(gu.cuda())
    t, s64 = FC.quant64(FC.swiglu64(gu))
    srel = ((s.cpu().double() - s64).abs() / s64).max().item()
    err, bound = FC.code_excess(_u8(q), t, 2.0 ** -18)
    print(f"F={F}: scale error {srel * 2 ** 18:.3f} x 2^-18, codes beyond half a step: "
          f"{FC.rel_used(_u8(q), t, 2.0 ** -18):.3f} of the 2^-18 allowance")
    assert srel <= 2.0 ** -18
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ wrapper and library argument checks
def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


@pytest.mark.parametrize("case,match", [("w_cpu", "weight must be a CUDA tensor"), ("xq_cpu", "xq must be a CUDA"),
                                        ("sx_cpu", "sx must be a CUDA tensor"), ("resid_cpu", "resid must be a CUDA"),
                                        ("sx_fp64", "sx must be contiguous fp32"), ("no_rows", "has no rows")])
def test_fp8_linear_q_rejects_tensors_off_the_gpu(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    xq, sx, wq, sw, _ = FC.int_linear_case(4, FC.LIN_N, 256)
    W = llm.Fp8Weight.from_quantised(wq, sw) if case == "w_cpu" else _weight(wq, sw)
    xd, sd, rd = xq.cuda(), sx.cuda(), FC.int_resid(4, FC.LIN_N).cuda() if case == "resid_cpu" else None
    if case == "xq_cpu":
        xd = xq
    elif case == "sx_cpu":
        sd = sx
    elif case == "resid_cpu":
        rd = rd.cpu()
    elif case == "sx_fp64":
        sd = sd.double()
    elif case == "no_rows":
        xd, sd = xd[:0], sd[:0]
    with pytest.raises(ValueError, match=match):
        llm.fp8_linear_q(xd, sd, W, resid=rd)


def test_library_refuses_shapes_it_cannot_launch():
    """-22 before any launch: M = 0, M = 65, N % 16 != 0, K % 256 != 0."""
    xq, sx, wq, sw, _ = FC.int_linear_case(FC.LIN_M, FC.LIN_N, 512)
    W, xd, sd = _weight(wq, sw), xq.cuda(), sx.cuda()
    y = torch.full((80, FC.LIN_N), -768.0, dtype=BF, device="cuda")
    L = lib()
    for M, N, K in ((0, 48, 512), (65, 48, 512), (64, 40, 512), (64, 48, 384), (64, 0, 512), (64, 48, 0)):
        assert L.gpbs_hip_fp8_linear(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.s), _ptr(y), M, N, K, _stream()) == -22
        assert L.gpbs_hip_fp8_linear_res(_ptr(xd), _ptr(sd), _ptr(W.qs), _ptr(W.s), _ptr(y), _ptr(y), M, N, K,
                                         _stream()) == -22
    assert bool((y == -768.0).all())
    with pytest.raises(ValueError, match="M <= 64"):
        llm.fp8_linear_q(torch.cat([xd, xd]), torch.cat([sd, sd]), W,
                         resid=torch.zeros(128, FC.LIN_N, dtype=BF, device="cuda"))

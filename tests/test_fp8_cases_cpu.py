"""fp8 decode linear and row quantisers: the fixtures of tests/fp8_cases.py do
what they claim, against llm.quant_rows_fp8_ref and fp64, and fp8_linear_q
refuses what the library cannot take before it touches the library.
Everything that can be checked without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as FC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

BF, F8 = FC.BF, FC.F8


def _u8(q):
    return q.contiguous().view(torch.uint8)


def _by_value(c):
    return torch.where(c == 0x80, torch.zeros_like(c), c)


def test_every_finite_code_is_exact_in_bf16_and_the_step_table_is_right():
    fc = FC.finite_codes()
    v = FC.values(fc)
    assert fc.numel() == 254 and torch.isfinite(v).all() and v.abs().max().item() == 448
    assert torch.equal(v.to(BF).float(), v)
    assert torch.equal(_u8(v.to(F8)), fc)  # both zeros keep their sign
    pos = FC.values(torch.arange(0x7F, dtype=torch.uint8)).double()
    assert torch.equal(FC.e4m3_step(pos[:-1]), pos[1:] - pos[:-1])
    assert torch.equal(FC.e4m3_step(-pos[:-1]), pos[1:] - pos[:-1])
    assert FC.e4m3_step(torch.tensor([448.0, 2.0 ** -12], dtype=torch.float64)).tolist() == [32.0, 2.0 ** -9]


def test_sizes_sit_below_on_and_one_vector_past_a_pass():
    assert [k // 8 for k in FC.QUANT_K] == [1, 63, 256, 257, 513] and all(k % 8 == 0 for k in FC.QUANT_K)
    assert [f // 8 for f in FC.SWIGLU_F] == [1, 1024, 1025, 1792] and all(f % 8 == 0 for f in FC.SWIGLU_F)
    assert all(k // 8 % 256 for k in FC.RANDOM_K[:2]) and FC.RANDOM_K[2] // 8 == 512


@pytest.mark.parametrize("K", sorted(set(FC.QUANT_K + FC.SWIGLU_F)))
def test_all_codes_rows_quantise_to_themselves(K):
    x, codes = FC.all_codes_case(K)
    assert x.shape == codes.shape == (codes.shape[0], K) and x.dtype == BF
    assert (x.float().abs().amax(-1) == 448).all()
    assert set(codes.flatten().tolist()) == set(FC.finite_codes().tolist())
    if K >= 254:
        assert all(set(r.tolist()) == set(FC.finite_codes().tolist()) for r in codes)
    q, s = llm.quant_rows_fp8_ref(x)
    assert torch.equal(_u8(q), codes) and torch.equal(s, torch.ones_like(s))


def test_tie_rows_round_to_the_even_neighbour():
    x, expect = FC.tie_case()
    v = x.double()
    pos = FC.values(torch.arange(0x7F, dtype=torch.uint8)).double()
    for xi, e in zip(v.flatten().tolist(), expect.flatten().tolist()):
        if abs(xi) == 448:
            assert e == FC.CODE_448
            continue
        below = int((pos <= abs(xi)).sum()) - 1
        assert pos[below] < abs(xi) < pos[below + 1] and abs(xi) - pos[below] == pos[below + 1] - abs(xi)
        assert (e & 0x7F) in (below, below + 1) and e % 2 == 0 and (e >> 7) == (xi < 0)
    assert set(expect.flatten().tolist()) >= {0x00, 0x80, 0x7E, 0xFE, 0x08, 0x88}  # zeros, top, first normal
    assert torch.equal(_u8(x.float().to(F8)), expect)  # torch's cast rounds to nearest even
    q, s = llm.quant_rows_fp8_ref(x)
    assert torch.equal(_u8(q), expect) and torch.equal(s, torch.ones_like(s))
    assert not torch.equal(expect[0], expect[1])  # the ties move between the lanes from row to row


@pytest.mark.parametrize("threads,sizes", [(256, FC.QUANT_K), (1024, FC.SWIGLU_F)])
def test_placement_rows_need_every_wave(threads, sizes):
    for K in sizes:
        x, codes, pos = FC.placement_case(K, threads)
        assert {p for p in (0, 7, 8, 511, 512, 2047, 2048, K - 1) if p < K} <= set(pos)
        owner = (torch.arange(K) // 8) % threads // 64  # wave of each element
        passes = (torch.arange(K) // 8) // threads
        firsts = {(int(owner[p]), int(passes[p])) for p in pos if p % 8 == 0 and (p // 8) % 64 == 0}
        assert firsts == {(int(w), int(p)) for w, p in zip(owner.tolist(), passes.tolist())}
        xf = x.float()
        for i, p in enumerate(pos):
            assert abs(xf[i, p].item()) == 448 and (xf[i].abs() == 448).sum() == 1
            rest = xf[i][owner != owner[p]]
            assert rest.numel() == 0 or rest.abs().max().item() <= 2  # lose that wave: scale <= 2 / 448
        assert not x[-1].any()
        q, s = llm.quant_rows_fp8_ref(x)
        assert torch.equal(_u8(q), codes) and torch.equal(s, torch.ones_like(s))
        q1, s1 = llm.quant_rows_fp8_ref(x[:1])
        assert torch.equal(_u8(q1), codes[:1]) and s1.tolist() == [1.0]


@pytest.mark.parametrize("K", FC.QUANT_K)
def test_rmsnorm_exact_case_has_unit_mean_square(K):
    for peak in FC.placement_positions(K)[:3] + [K - 1]:
        x, w, codes = FC.rmsnorm_exact_case(K, peak)
        xf = x.float()
        assert torch.equal(xf.abs(), torch.ones_like(xf)) and xf.pow(2).mean(-1).tolist() == [1.0] * 3
        assert w.float()[peak].item() == 448 and (w.float().abs() == 448).sum() == 1
        h = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 0.0) * w.float()
        q, s = llm.quant_rows_fp8_ref(h)
        assert torch.equal(_u8(q), codes) and torch.equal(s, torch.ones_like(s))
        t, s64 = FC.quant64(FC.rmsnorm64(x, w, 0.0))
        assert torch.equal(t, FC.values(codes).double()) and s64.tolist() == [1.0] * 3
        # a reciprocal square root one ulp off moves no code: the values are codes, never ties
        for rs in (1 - 2.0 ** -24, 1 + 2.0 ** -23):
            q, s = llm.quant_rows_fp8_ref(xf * torch.tensor(rs, dtype=torch.float32) * w.float())
            assert torch.equal(_u8(q), codes) and (s - 1).abs().max().item() <= 2 * 2.0 ** -23


@pytest.mark.parametrize("F", FC.SWIGLU_F)
def test_swiglu_exact_case_yields_codes_and_zeros(F):
    gu, codes, on = FC.swiglu_exact_case(F)
    a, b = gu[:, :F].float(), gu[:, F:].float()
    assert set(a.flatten().tolist()) <= {0.0, 32.0} and torch.equal(a == 32, on)
    thirty_two = torch.tensor(32.0)
    assert (thirty_two / (1 + torch.exp(-thirty_two))).item() == 32.0  # v / (1 + exp(-v)) in fp32
    assert torch.nn.functional.silu(thirty_two).item() == 32.0 and float(2.0 ** -24) > torch.exp(-thirty_two).item() > 0
    y = a / (1 + torch.exp(-a)) * b
    want = torch.where(on, FC.values(codes), torch.zeros(()))
    assert torch.equal(y, want)  # == compares the zeros by value
    assert (y.abs().amax(-1) == 448).all()
    q, s = llm.quant_rows_fp8_ref(y)
    expect = torch.where(on, codes, torch.zeros_like(codes))
    assert torch.equal(_by_value(_u8(q)), _by_value(expect)) and torch.equal(s, torch.ones_like(s))
    assert torch.equal(_u8(q)[on], codes[on])  # behind an open gate the sign of a zero is fixed too
    assert torch.equal(FC.swiglu64(gu).float(), want)

    gu, codes, pos = FC.swiglu_placement_case(F)
    y = FC.swiglu64(gu).float()
    assert torch.equal(y[:-1], FC.values(codes)[:-1]) and not y[-1].any()
    assert {8 * 64 * w for w in range(16) if 8 * 64 * w < F} <= set(pos)


# ------------------------------------------------------------------ the mirrored reference against fp64
@pytest.mark.parametrize("K", FC.RANDOM_K)
def test_reference_quantiser_is_within_half_a_step_of_fp64(K):
    """quant_rows_fp8_ref rounds x (448 / amax) computed in fp32: two roundings
    of 2^-24 relative before the cast, so every code is within half an e4m3 step
    plus 2^-20 relative of the fp64 value, and differs from the fp64 rounding
    only where fp32 rounding moved a value onto or across a tie."""
    x = FC.random_rows(67, K, seed=5)
    q, s = llm.quant_rows_fp8_ref(x)
    t, s64 = FC.quant64(x)
    assert not q[3].float().any() and s[3].item() == 1.0
    assert torch.equal(s, s64.float())  # amax / 448: one correctly rounded division
    err, bound = FC.code_excess(_u8(q), t, 2.0 ** -20)
    assert bool((err <= bound).all())
    q64 = t.clamp(-448, 448).float().to(F8)  # fp64 -> fp32 is exact or far from a tie at 8 + 24 bits
    diff = _u8(q) != _u8(q64)
    gap = (err - FC.e4m3_step(t.clamp(-448, 448)) / 2).abs()[diff]
    print(f"K={K}: {int(diff.sum())} of {diff.numel()} codes differ from the fp64 rounding, all within "
          f"{gap.max().item() if diff.any() else 0:.3g} of a tie")
    assert diff.float().mean().item() < 5e-3
    assert not diff.any() or bool((gap <= 2.0 ** -20 * t.abs().clamp(max=448)[diff]).all())


# ------------------------------------------------------------------ linear fixtures
def test_integer_operands_survive_the_quantiser_and_from_quantised():
    xq, sx, wq, sw, acc = FC.int_linear_case(FC.LIN_M, FC.LIN_N, 768, scales=False)
    W = llm.Fp8Weight(wq.float().to(BF))
    assert torch.equal(_u8(W.q), _u8(wq)) and torch.equal(W.s, torch.ones(FC.LIN_N))
    q, s = llm.quant_rows_fp8_ref(xq.float().to(BF)[(xq.float().abs() == 8).any(-1)] * 56)  # amax 448: scale 1
    assert torch.equal(s, torch.ones_like(s))
    V = llm.Fp8Weight.from_quantised(wq, sw)
    assert (V.N, V.K) == (FC.LIN_N, 768) and torch.equal(_u8(V.qs), _u8(W.qs)) and torch.equal(_u8(V.q), _u8(wq))
    assert V.s.dtype == torch.float32 and torch.equal(V.s, sw)
    # power-of-two row scales: the quantiser gives the same codes and those scales
    xq, sx, wq, sw, acc = FC.int_linear_case(FC.LIN_M, FC.LIN_N, 768)
    assert set(sw.tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0} == set(sx.tolist())
    W = llm.Fp8Weight((wq.float() * sw[:, None]).to(BF))
    assert torch.equal(_u8(W.q), _u8(wq)) and torch.equal(W.s, sw)
    for bad_q, bad_s in ((wq.float(), sw), (wq[:40], sw[:40]), (wq[:, :300], sw), (wq, sw.double()), (wq, sw[:47])):
        with pytest.raises(ValueError):
            llm.Fp8Weight.from_quantised(bad_q, bad_s)


def test_integer_case_is_exact_in_fp32_at_the_largest_k():
    nkb = max(FC.NKB)
    K = 256 * nkb
    xq, sx, wq, sw, acc = FC.int_linear_case(FC.LIN_M, FC.LIN_N, K)
    assert (wq.float().abs() == 448).sum(-1).tolist() == [1] * FC.LIN_N
    assert acc.dtype == torch.float64 and acc.abs().max().item() <= 64 * K + 3584 < 2 ** 24
    # fp32 sums in several orders, blocks of 32 k as the MFMA takes them included
    xf, wf = xq.float(), wq.float()
    shuffled = torch.randperm(K, generator=torch.Generator().manual_seed(1))
    for order in (torch.arange(K), torch.arange(K - 1, -1, -1), shuffled):
        s = torch.zeros(FC.LIN_M, FC.LIN_N)
        for k0 in range(0, K, 32):
            idx = order[k0:k0 + 32]
            s = s + xf[:, idx] @ wf[:, idx].t()
        assert torch.equal(s.double(), acc)
    r = FC.int_resid(FC.LIN_M, FC.LIN_N)
    assert torch.equal(r.float(), r.float().round()) and r.float().abs().max().item() <= 128
    # the kernel's epilogue in fp32, (s sx) sw then + r, against fp64
    v32 = s * sx[:, None] * sw[None, :]
    v64 = acc * sx.double()[:, None] * sw.double()[None, :]
    assert torch.equal(v32.double(), v64) and torch.equal((v32 + r.float()).double(), v64 + r.double())
    assert torch.equal(FC.int_expect(acc, sx, sw), v32.to(BF))
    assert torch.equal(FC.int_expect(acc, sx, sw, r), (v32 + r.float()).to(BF))
    # a residual added before the scaling, or one dropped block, is another bf16 value somewhere
    assert not torch.equal(((s + r.float()) * sx[:, None] * sw[None, :]).to(BF), FC.int_expect(acc, sx, sw, r))
    less = (xf[:, :-256] @ wf[:, :-256].t()) * sx[:, None] * sw[None, :]
    assert (less.to(BF) != FC.int_expect(acc, sx, sw)).float().mean().item() > 0.9


@pytest.mark.parametrize("nkb", FC.NKB)
def test_one_hot_rows_visit_every_block_and_every_byte(nkb):
    K = 256 * nkb
    seen = set()
    for ph in range(FC.one_hot_phases(nkb)):
        xq, wq, k, expect = FC.one_hot_case(nkb, ph)
        assert (xq.float() != 0).sum(-1).tolist() == [1] * FC.LIN_M and _u8(xq).max().item() == FC.CODE_ONE
        assert int(k.max()) < K and torch.equal(xq.float()[torch.arange(FC.LIN_M), k], torch.ones(FC.LIN_M))
        assert torch.equal(expect.double(), xq.double() @ wq.double().t())
        assert torch.equal(FC.one_hot_decode(expect[:, :4]), k)  # the output names its k
        seen |= {(int(v) // 256, int(v) % 256 // 8, int(v) % 8) for v in k}
        assert {b for b, _, _ in seen} == set(range(nkb)) or ph == 0 and nkb > 16
    assert {(b, s) for b, s, _ in seen} == {(b, s) for b in range(nkb) for s in range(32)}
    assert {(s, e) for _, s, e in seen} == {(s, e) for s in range(32) for e in range(8)}
    w = FC.one_hot_weight(FC.LIN_N, K)
    assert w.abs().max().item() <= 8 and torch.unique(w[:4], dim=1).shape[1] == K  # columns 0..3 tell every k apart


def test_skinny_loop_cases_cover_every_kind_of_trip():
    """kb = w, w + 2 WV, ..; the second block kb + WV only when it exists."""
    for WV in (8, 4):
        kinds = set()
        for nkb in FC.NKB:
            for w in range(WV):
                trips = [(kb, kb + WV < nkb) for kb in range(w, nkb, 2 * WV)]
                kinds.add((len(trips), trips[-1][1] if trips else None))
        # no block, a lone first block, a first pair, a lone block in the second trip, a pair there
        assert {(0, None), (1, False), (1, True), (2, False), (2, True)} <= kinds
    assert FC.M_EDGE_K == 256 * 9 and {16, 17, 32, 33} <= set(FC.M_EDGES)


@pytest.mark.parametrize("K", FC.REAL_K)
def test_real_data_bound_holds_for_fp32_and_sees_a_dropped_block(K):
    xq, sx, wq, sw, ref, bound = FC.real_linear_case(FC.REAL_M[1], FC.REAL_N, K, llm.quant_rows_fp8_ref)
    assert torch.isfinite(ref).all() and bool((bound > 0).all())
    fp32 = (xq.float() @ wq.float().t()) * sx[:, None] * sw[None, :]
    assert bool(((fp32.to(BF).double() - ref).abs() <= bound).all())
    # one dropped 256-byte block is outside it almost everywhere
    less = (xq.float()[:, 256:] @ wq.float()[:, 256:].t()) * sx[:, None] * sw[None, :]
    assert ((less.to(BF).double() - ref).abs() > bound).float().mean().item() > 0.5


# ------------------------------------------------------------------ validation before the library
def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


@pytest.mark.parametrize("case,match", [
    ("ok_but_cpu", "xq must be a CUDA tensor"), ("sx_fp64", "sx must be contiguous fp32"),
    ("sx_strided", "sx must be contiguous fp32"), ("sx_short", "sx must be contiguous fp32 with 4 elements"),
    ("resid_fp32", "resid must be contiguous bf16"), ("resid_strided", "resid must be contiguous bf16"),
    ("resid_short", "resid must be contiguous bf16 with 4 x 48"), ("no_rows", "has no rows"),
    ("xq_bf16", "need contiguous e4m3fn"), ("xq_width", "need contiguous e4m3fn")])
def test_fp8_linear_q_rejects_bad_arguments_before_the_library(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    xq, sx, wq, sw, _ = FC.int_linear_case(4, FC.LIN_N, 256)
    W = llm.Fp8Weight.from_quantised(wq, sw)
    resid = FC.int_resid(4, FC.LIN_N) if case.startswith("resid") else None
    if case == "sx_fp64":
        sx = sx.double()
    elif case == "sx_strided":
        sx = torch.ones(8)[::2]
    elif case == "sx_short":
        sx = sx[:3].contiguous()
    elif case == "resid_fp32":
        resid = resid.float()
    elif case == "resid_strided":
        resid = torch.zeros(4, 2 * FC.LIN_N, dtype=BF)[:, ::2]
        assert resid.numel() == 4 * FC.LIN_N and not resid.is_contiguous()
    elif case == "resid_short":
        resid = resid[:3].contiguous()
    elif case == "no_rows":
        xq, sx = xq[:0], sx[:0]
    elif case == "xq_bf16":
        xq = xq.float().to(BF)
    elif case == "xq_width":
        xq = xq[:, :128].contiguous()
    with pytest.raises(ValueError, match=match):
        llm.fp8_linear_q(xq, sx, W, resid=resid)
    if case in ("sx_fp64", "no_rows"):
        with pytest.raises(ValueError, match=match):
            llm.fp8_linear_q(xq, sx, W, tiled=True)

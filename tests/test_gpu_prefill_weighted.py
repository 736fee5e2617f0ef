"""The twelve prefill-attention kernels (k_prefill_attn, _seq, _paged for
G = 1/2/4/8, csrc/hip/prefill_attn_body.hpp) on the MI355X against data whose
softmax weights are not 0 or 1 (tests/weighted_cases.py), at shapes where
G = 1 runs a second query tile, and page 256 through all four paged kernels.

* census: every weight exactly 1; |out - expect| <= (2^-8 + 2^-20) |expect|,
  zeros exactly zero, nothing non-finite although every stale row is NaN.
* ramp: the rescale factor of the even heads lies strictly between 0 and 1 at
  every full tile; |out - fp64| within weighted_cases.ramp_bound.
* the _seq kernel carries the bits of the uniform kernel run on each sequence
  alone, the _paged kernel those of the _seq kernel on the gathered cache.

Largest fraction of each bound reached on the MI355X (the tests print theirs):
  census  uniform 0.992  _seq 0.992  _paged 0.992  (the plain-torch emulation
          of tests/test_weighted_cases_cpu.py reaches the same 0.992);
  ramp    uniform 0.546  _seq 0.536  _paged 0.536  (the emulation: 0.546, at
          the same case, S = 200 at pos 0 with G = 8).
Only in-range block-table entries are used here.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import paged_cases as PG  # noqa: E402
import prefill_cases as PC  # noqa: E402
import ragged_cases as RC  # noqa: E402
import weighted_cases as WC  # noqa: E402
# the pool checks of the rope-cache kernels at pages 64 / 128, reused as they stand
from test_gpu_paged_attn import _check_pools, _check_rope_prefill, _random_paged, _tables  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu

B, HD, C = WC.B, WC.HD, WC.C
UNIFORM = [(S, pos, H, Hkv) for (S, pos) in WC.ALL for (H, Hkv) in WC.HEADS]
WIDE = [(S, pos, H, Hkv) for (S, pos) in WC.WIDE for (H, Hkv) in WC.HEADS]
KINDS = ("census", "ramp")
SEQ = [(kind, pairs, H, Hkv) for kind in KINDS for pairs in WC.RAGGED for (H, Hkv) in WC.HEADS]
PAGED = [(kind, pairs, H, Hkv, page) for (kind, pairs, H, Hkv) in SEQ for page in WC.PAGES]
DECODE_256 = [(kind, s, H, Hkv) for kind in WC.DECODE_KINDS for s in range(len(WC.DECODE_SETS))
              for (H, Hkv) in DC.HEADS]


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_census(out, expect, what):
    """out (bf16, CPU) against the fp64 expectation: finite, within
    CENSUS_REL |expect| (NaN counts as outside), zeros exactly zero.  Returns the
    largest fraction of the bound reached."""
    out = out.double().reshape(expect.shape)
    assert torch.isfinite(out).all(), f"{what}: {(~torch.isfinite(out)).sum().item()} non-finite outputs"
    bound = WC.CENSUS_REL * expect.abs()
    bad = WC.outside(out, expect, bound).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} outputs outside the census bound, first {bad[:6].tolist()}: got "
                              f"{[out[tuple(i)].item() for i in bad[:4].tolist()]} for "
                              f"{[expect[tuple(i)].item() for i in bad[:4].tolist()]}")
    assert (out[expect == 0] == 0).all(), f"{what}: a dimension no visible key feeds is not 0"
    return WC.fraction(out, expect, bound)


def _check_ramp(out, ref, bound, what):
    """out (bf16, CPU) within the ramp bound of the fp64 reference; returns the
    largest fraction of it reached."""
    out = out.double().reshape(ref.shape)
    frac = WC.fraction(out, ref, bound)
    bad = WC.outside(out, ref, bound).nonzero()  # NaN counts as outside
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} outputs outside the ramp bound ({frac:.3g} of it), first "
                              f"{bad[:6].tolist()}")
    return frac


# ------------------------------------------------------------------ k_prefill_attn
@pytest.mark.parametrize("S,pos,H,Hkv", WIDE)
def test_one_hot_data_on_the_wide_shapes_bit_for_bit(S, pos, H, Hkv):
    """The exact-data fixture where G = 1 has a second query tile (q0 = 256) of
    1, 44 and 128 tokens and the heaviest-first order two tiles to order."""
    q, kc, vc, t, expect = PC.exact_case(S, pos, H, Hkv)
    out = llm.prefill_attn(*_cuda(q, kc, vc), pos).cpu()
    assert out.shape == (B, S, H * HD) and out.dtype == torch.bfloat16
    bad = (_bits(out) != _bits(expect)).view(B, S, H, HD).any(-1).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong (b, s, h) rows, first {bad[:8].tolist()}"


@pytest.mark.parametrize("S,pos,H,Hkv", [c for c in WIDE if c[0] + c[1] + 1 <= C])
def test_first_masked_key_is_not_seen_on_the_wide_shapes(S, pos, H, Hkv):
    """Every target one up, key pos + S coded (so (384, 16), which fills the cache,
    has no such key and is left to the other tests).  A query whose target is
    still visible returns its V row bit for bit; one aimed at key pos + s + 1
    must not return that row, and stays close to the reference."""
    q, kc, vc, t, leaked = PC.exact_case(S, pos, H, Hkv, shift=1)
    hidden = t > (pos + torch.arange(S)).view(1, S, 1)
    assert hidden[:, :, 0].all() and torch.equal(t[:, :, 0], (pos + 1 + torch.arange(S)).expand(B, S))
    out = llm.prefill_attn(*_cuda(q, kc, vc), pos).cpu()
    same = (_bits(out) == _bits(leaked)).view(B, S, H, HD).all(-1)
    assert not (same & hidden).any(), f"(b, s, h) {(same & hidden).nonzero()[:8].tolist()} see their first masked key"
    assert same[~hidden].all(), f"wrong rows with a visible target: {(~same & ~hidden).nonzero()[:8].tolist()}"
    ref = llm.prefill_attn_ref(q, kc, vc, pos)
    err, mag = (out.float() - ref).abs().max().item(), ref.abs().max().item()
    print(f"first-masked-key S={S} pos={pos} H={H} Hkv={Hkv}: err {err:.4g} of {mag:.4g}")
    assert err < 2e-2 * mag


@pytest.mark.parametrize("S,pos,H,Hkv", UNIFORM)
def test_census_counts_every_visible_key_once(S, pos, H, Hkv):
    """q = 0: every weight is 1 and l = pos + s + 1 exactly, through every rescale
    (corr = 1) and every masked tile; one key dropped or doubled moves one
    dimension by at least 25 %."""
    q, kc, vc, expect = WC.census_case(S, pos, H, Hkv)
    out = llm.prefill_attn(*_cuda(q, kc, vc), pos).cpu()
    assert out.shape == (B, S, H * HD) and out.dtype == torch.bfloat16
    frac = _check_census(out, expect, "prefill_attn")
    print(f"FRACTION census uniform S={S} pos={pos} G={H // Hkv}: {frac:.4f}")


@pytest.mark.parametrize("S,pos,H,Hkv", UNIFORM)
def test_ramp_against_fp64(S, pos, H, Hkv):
    """The running max of the even heads rises by 0.5 .. 12 nats per full tile
    (tests/test_weighted_cases_cpu.py), so l *= corr and o *= corr act on finite
    values with 0 < corr < 1.  Equal calls give equal bits."""
    q, kc, vc = WC.ramp_case(S, pos, H, Hkv)
    ref, bound = WC.ramp_ref(S, pos, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    out = llm.prefill_attn(qd, kd, vd, pos)
    frac = _check_ramp(out.cpu(), ref, bound, "prefill_attn")
    print(f"FRACTION ramp uniform S={S} pos={pos} G={H // Hkv}: {frac:.4f}")
    assert _same_bits(out, llm.prefill_attn(qd, kd, vd, pos)), "equal calls, different bits"


# ------------------------------------------------------------------ k_prefill_attn_seq
def _alone(qd, kd, vd, b, n, p):
    """The uniform kernel on sequence b alone: its batch-1 slice with (S = n, pos = p)."""
    return llm.prefill_attn(qd[b:b + 1, :n].contiguous(), kd[b:b + 1], vd[b:b + 1], p)[0]


def _check_against_fp64(kind, out, pairs, H, Hkv, expect, form):
    """The rows of every active sequence against the fp64 expectation of the
    uniform fixture they were taken from; prints the fraction of the bound."""
    if kind == "census":
        frac = _check_census(out, expect, form)
    else:
        frac = 0.0
        for b, pair in enumerate(pairs):
            if pair is not None:
                n, p = pair
                ref, bound = WC.ramp_ref(n, p, H, Hkv)
                frac = max(frac, _check_ramp(out[b, :n], ref[b], bound[b], f"{form}, sequence {b}"))
    print(f"FRACTION {kind} {form} {pairs} G={H // Hkv}: {frac:.4f}")


@pytest.mark.parametrize("kind,pairs,H,Hkv", SEQ)
def test_seq_rows_carry_the_bits_of_the_uniform_kernel(kind, pairs, H, Hkv):
    """Padding query rows and an idle sequence's q and caches are NaN, and so is
    every cache row past a sequence's last: rows < n_b are the bits of
    prefill_attn on that sequence alone, everything else zero bits."""
    q, kc, vc, pos, lens, expect = WC.ragged_case(kind, pairs, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    out = llm.prefill_attn_seq(qd, kd, vd, _i32(pos), _i32(lens))
    assert out.shape == (B, q.shape[1], H * HD) and out.dtype == torch.bfloat16
    for b, n in enumerate(lens):
        assert not _bits(out[b, n:]).any(), f"sequence {b}: rows >= {n} are not zero bits"
        if n:
            assert _same_bits(out[b, :n], _alone(qd, kd, vd, b, n, pos[b])), f"sequence {b} differs from prefill_attn"
    _check_against_fp64(kind, out.cpu(), pairs, H, Hkv, expect, "_seq")


# ------------------------------------------------------------------ k_prefill_attn_paged
def _paged_and_seq(c):
    """prefill_attn_paged on a paged case and prefill_attn_seq on the dense cache
    of Cl rows gathered from its pools."""
    qd, kp, vp, table = _cuda(c["q"], c["kpool"], c["vpool"], c["table"])
    kd = PG.gather_dense(kp, c["ids"], c["rows"], c["Cl"])
    vd = PG.gather_dense(vp, c["ids"], c["rows"], c["Cl"])
    pos_t, len_t = _i32(c["pos"]), _i32(c["lens"])
    return llm.prefill_attn_paged(qd, kp, vp, table, pos_t, len_t), llm.prefill_attn_seq(qd, kd, vd, pos_t, len_t)


def _check_paged_against_seq(out, ref, lens):
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    for b, n in enumerate(lens):
        assert not _bits(out[b, n:]).any() and not _bits(ref[b, n:]).any(), f"sequence {b}: rows >= {n} not zero bits"
        assert _same_bits(out[b, :n], ref[b, :n]), f"sequence {b} differs from prefill_attn_seq"
        assert n == 0 or _bits(out[b, :n]).any()


@pytest.mark.parametrize("kind,pairs,H,Hkv,page", PAGED)
def test_paged_rows_carry_the_bits_of_the_seq_kernel(kind, pairs, H, Hkv, page):
    """Pages of 64, 128 and 256 rows (1, 2 and 4 key tiles per table entry) under
    a shuffled assignment; every pool row that is not a sequence's is NaN."""
    c = WC.paged_case(kind, pairs, H, Hkv, page)
    out, ref = _paged_and_seq(c)
    _check_paged_against_seq(out, ref, c["lens"])
    _check_against_fp64(kind, out.cpu(), pairs, H, Hkv, c["expect"], f"_paged page={page}")


@pytest.mark.parametrize("H,Hkv", PC.HEADS)
@pytest.mark.parametrize("s", range(len(PG.PREFILL_SETS)))
def test_one_hot_ragged_data_through_pages_of_256_bit_for_bit(s, H, Hkv):
    c = PG.prefill_case(s, H, Hkv, 256)
    assert (c["NP"], c["Cl"]) == (2, 512)
    out, ref = _paged_and_seq(c)
    _check_paged_against_seq(out, ref, c["lens"])
    bad = (_bits(out.cpu()) != _bits(c["expect"])).view(B, -1, H, HD).any(-1).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong (b, s, h) rows, first {bad[:8].tolist()}"


# ------------------------------------------------------------------ page 256 in the other three paged kernels
@pytest.mark.parametrize("kind,s,H,Hkv", DECODE_256)
def test_decode_attn_through_pages_of_256(kind, s, H, Hkv):
    """The decode fixtures over Cl = 1280 (NP = 5), every nsplit: an active row has
    the bits of decode_attn_seq on the gathered dense cache and meets its
    fixture's expectation (the V row bit for bit; the census bound; the bound of
    the decode ramp), an idle row (NaN q, a table row of garbage) is zero bits."""
    c = WC.decode_case_256(kind, s, H, Hkv)
    assert (c["NP"], c["Cl"]) == (5, 1280)
    qd, kp, vp, table = _cuda(c["q"], c["kpool"], c["vpool"], c["table"])
    kd = PG.gather_dense(kp, c["ids"], c["rows"], c["Cl"])
    vd = PG.gather_dense(vp, c["ids"], c["rows"], c["Cl"])
    pos_t = _i32(c["positions"])
    for ns in DC.NSPLITS:
        out = llm.decode_attn_paged(qd, kp, vp, table, pos_t, ns)
        ref = llm.decode_attn_seq(qd, kd, vd, pos_t, ns)
        assert out.shape == (DC.B, H * HD) and out.dtype == torch.bfloat16
        host = out.cpu()
        for b, p in enumerate(c["positions"]):
            what = f"{kind}, nsplit={ns}, sequence {b} at pos {p}"
            if not WC.decode_active(p):
                assert not _bits(out[b]).any(), f"{what}: an idle row is not zero bits"
                continue
            assert _same_bits(out[b], ref[b]), f"{what}: differs from decode_attn_seq"
            expect, bound = c["expect"][b], c["bound"][b]
            if kind == "exact":
                bad = (_bits(host[b]) != _bits(expect)).view(H, HD).any(-1).nonzero().flatten().tolist()
                assert not bad, f"{what}: wrong heads {bad}"
            elif kind == "census":
                _check_census(host[b], expect, what)
            else:
                assert not WC.outside(host[b], expect, bound).any(), \
                    f"{what}: {WC.fraction(host[b], expect, bound):.3g} of the decode ramp bound"


@pytest.mark.parametrize("s", range(len(WC.DECODE_SETS)))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_through_pages_of_256(s, H, Hkv):
    """q has the bits of qkv_rope_cache_seq on the gathered dense caches, the page
    rows written are the rows it wrote, every other pool row keeps its bits."""
    positions, Bd, page = WC.DECODE_SETS[s], DC.B, WC.DECODE_PAGE
    NP = PG.n_table(DC.C, page)
    rows = [p + 1 if WC.decode_active(p) else 0 for p in positions]
    kp, vp, table, ids, kd, vd = _random_paged(Bd, Hkv, rows, page, NP, seed=sum(positions) + H + page)
    kp0, vp0 = kp.clone(), vp.clone()
    cos, sin = _tables(H, Hkv, NP * page)
    qkv = torch.randn(Bd, 1, (H + 2 * Hkv) * HD, generator=torch.Generator().manual_seed(s)).bfloat16().cuda()
    pos_t = _i32(positions)
    q = llm.qkv_rope_cache_paged(qkv, cos, sin, pos_t, table, kp, vp, H)
    qs = llm.qkv_rope_cache_seq(qkv, cos, sin, pos_t, kd, vd, H)
    assert q.shape == (Bd, H, HD) and _same_bits(q, qs)
    for b, p in enumerate(positions):
        assert WC.decode_active(p) == bool(_bits(q[b]).any())
    _check_pools(kp, vp, kp0, vp0, ids, kd, vd, page, [[p] if WC.decode_active(p) else [] for p in positions])


@pytest.mark.parametrize("pairs", WC.RAGGED)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_prefill_through_pages_of_256(pairs, H, Hkv):
    """Two pages per sequence at most (Cl = 512): a sequence of the wide shapes
    writes rows on both sides of the page edge at row 256."""
    S = max(RC.prefill_tokens(p) for p in pairs)
    pos = [-1 if p is None else p[1] for p in pairs]
    lens = [RC.prefill_tokens(p) for p in pairs]
    _check_rope_prefill(S, H, Hkv, 256, pos, lens, lens, seed=S + H + 256)

"""Guards of the weighted-softmax fixtures (tests/weighted_cases.py) behind
tests/test_gpu_prefill_weighted.py: everything about them that can be checked
without a GPU, the derived bounds included."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import paged_cases as PG  # noqa: E402
import weighted_cases as WC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

CASES = [(S, pos, H, Hkv) for (S, pos) in WC.ALL for (H, Hkv) in WC.HEADS]
INF = float("inf")


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------ 1. the fp64 reference
@pytest.mark.parametrize("H,Hkv", [(8, 2), (2, 2), (8, 1)])
@pytest.mark.parametrize("S,pos", [(1, 0), (7, 0), (65, 64), (300, 37)])
def test_ref64_equals_prefill_attn_ref_on_fp64_inputs(S, pos, H, Hkv):
    g = torch.Generator().manual_seed(S + pos + H)
    q = torch.randn(WC.B, S, H, WC.HD, dtype=torch.float64, generator=g)
    kc = torch.randn(WC.B, Hkv, WC.C, WC.HD, dtype=torch.float64, generator=g)
    vc = torch.randn(WC.B, Hkv, WC.C, WC.HD, dtype=torch.float64, generator=g)
    kc[:, :, pos + S:], vc[:, :, pos + S:] = WC.NAN, WC.NAN  # not read by either
    ref, A = WC.ref64(q, kc, vc, pos)
    want = llm.prefill_attn_ref(q, kc, vc, pos)
    assert ref.dtype == torch.float64 and ref.shape == want.shape == (WC.B, S, H * WC.HD)
    torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-13)
    # A is the same weighted mean taken of |V|
    torch.testing.assert_close(A, llm.prefill_attn_ref(q, kc, vc.abs(), pos), rtol=1e-12, atol=1e-13)
    assert (A >= ref.abs() - 1e-13).all()


# ------------------------------------------------------------------ 2. the census fixture and its bound
@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_census_fixture_counts_the_visible_keys(S, pos, H, Hkv):
    q, kc, vc, expect = WC.census_case(S, pos, H, Hkv)
    rows = pos + S
    assert not _bits(q).any() and q.dtype == kc.dtype == vc.dtype == torch.bfloat16
    assert torch.isfinite(kc[:, :, :rows].float()).all() and torch.isfinite(vc[:, :, :rows].float()).all()
    assert torch.isnan(kc[:, :, rows:].float()).all() and torch.isnan(vc[:, :, rows:].float()).all()
    assert (vc[:, :, :rows].float().sum(-1) == 256).all()  # one dimension per key
    ref, _ = WC.ref64(q, kc, vc, pos)  # q = 0: uniform weights
    torch.testing.assert_close(ref, expect, rtol=1e-12, atol=1e-12)
    # one key more or less moves its dimension by at least 25 %: no residue is met more than 4 times
    L = (pos + 1 + torch.arange(S)).double().view(1, S, 1)
    count = expect * L / 256
    torch.testing.assert_close(count, count.round(), rtol=0, atol=1e-9)
    assert count.max().item() <= 4 + 1e-9
    torch.testing.assert_close(count.view(WC.B, S, H, WC.HD).sum(-1), L.expand(WC.B, S, H), rtol=0, atol=1e-9)


def test_census_bound_covers_the_fp32_arithmetic_for_every_key_count():
    """The kernels compute bf16(fp32(256 count) * fp32(1 / L)) on exact integers.
    Half a bf16 ulp is at most 2^-8 of the value, the reciprocal and the multiply
    add less than 2^-22: for every L up to 400 (prefill) and up to 1100 (the
    decode fixtures at page 256), also with a reciprocal one ulp off either way,
    the result lies within (2^-8 + 2^-20) |expect| and zeros stay zero."""
    worst = {400: 0.0, DC.C: 0.0}
    d = torch.arange(WC.HD)
    for L in range(1, DC.C + 1):
        count = ((torch.arange(L)[:, None] % WC.HD) == d[None, :]).sum(0).double()
        expect = 256 * count / L
        bound = WC.CENSUS_REL * expect.abs()
        for du in (-1, 0, 1):
            inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(L), dtype=torch.float32)
            inv = (inv.view(torch.int32) + du).view(torch.float32)
            out = ((256 * count).float() * inv).bfloat16().double()
            err = (out - expect).abs()
            assert (err <= bound).all(), (L, du)
            assert (out[expect == 0] == 0).all(), (L, du)
            nz = expect > 0
            frac = (err[nz] / bound[nz]).max().item()
            for top in worst:
                if L <= top:
                    worst[top] = max(worst[top], frac)
    print(f"census: the emulated arithmetic reaches {worst[400]:.4f} of the bound for L <= 400, "
          f"{worst[DC.C]:.4f} for L <= {DC.C}")
    assert 0.9 < worst[400] <= 1.0  # the bound is tight, not generous


# ------------------------------------------------------------------ 3. the ramp fixture
def _tile_max(sc):
    """[.., L] -> [.., ntiles]: the maximum of each 64-key tile."""
    L = sc.shape[-1]
    return torch.stack([sc[..., k0:k0 + WC.KT].max(-1).values for k0 in range(0, L, WC.KT)], -1)


@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_ramp_fixture_keeps_the_rescale_factor_strictly_between_0_and_1(S, pos, H, Hkv):
    """The last token in fp64: the running max of every even head rises from one
    full 64-key tile to the next by at least 0.5 and at most 12 nats, so
    corr = exp(-rise) lies in [6e-6, 0.61]; every odd head has its max in the
    first tile (corr = 1 from then on).

    A partial last tile of n < 64 keys continues the ramp by n / 64 of a tile's
    rise only: with n = 1 (shapes (65, 64) and (257, 64)) no slope that keeps
    the full tiles below 12 nats can lift one key 0.5 nats over the 64 before
    it.  For that tile only the upper limit is asserted."""
    q, kc, vc = WC.ramp_case(S, pos, H, Hkv)
    rows = pos + S
    assert torch.isnan(kc[:, :, rows:].float()).all() and torch.isnan(vc[:, :, rows:].float()).all()
    assert torch.isfinite(kc[:, :, :rows].float()).all() and torch.isfinite(vc[:, :, :rows].float()).all()
    h = torch.arange(H)
    assert torch.equal(q[:, :, :, 0].float(), torch.where(h % 2 == 0, 8.0 + h, -(8.0 + h)).expand(WC.B, S, H))
    ramp = (WC.SLOPE * torch.arange(rows) / rows).to(torch.bfloat16)
    assert torch.equal(kc[:, :, :rows, 0], ramp.expand(WC.B, Hkv, rows))
    sc = WC.scores64(q, kc, pos)[:, :, :, -1].reshape(WC.B, H, rows)  # the last token sees every row
    assert torch.isfinite(sc).all() and sc.abs().max().item() <= 40  # the range the score term of the bound assumes
    tm = _tile_max(sc)
    assert (tm[:, 1::2].argmax(-1) == 0).all(), "an odd head's max is not in the first tile"
    run = tm[:, 0::2].cummax(-1).values
    rise = run[..., 1:] - run[..., :-1]
    full = rows // WC.KT  # full tiles; a partial one follows if rows % 64
    if rise.numel():
        assert rise.max().item() <= 12, f"a running max rises by {rise.max().item():.2f} nats"
    between_full = rise[..., :max(full - 1, 0)]
    if between_full.numel():
        lo, hi = between_full.min().item(), between_full.max().item()
        print(f"ramp S={S} pos={pos} H={H} Hkv={Hkv}: full-tile rises in [{lo:.2f}, {hi:.2f}] nats")
        assert lo >= 0.5, f"a running max rises by only {lo:.2f} nats between two full tiles"


def test_ramp_shapes_cover_more_than_one_rescale():
    """At least one shape with 6 full tiles (5 fractional rescales in a row) and
    the three WIDE shapes among those with several."""
    tiles = {(S, pos): (pos + S) // WC.KT for (S, pos) in WC.ALL}
    assert max(tiles.values()) == 6 and all(tiles[w] >= 5 for w in WC.WIDE)


# ------------------------------------------------------------------ 4. the kernel's arithmetic, emulated
def _emulate(q, kc, vc, pos, rescale=torch.exp2):
    """k_prefill_attn's arithmetic in plain torch fp32: scores scaled into the
    log2 domain in one separate rounding, ascending tiles of 64 keys, the
    rescale by exp2(m - mn), P rounded to bf16 as the PV operand, l summed from
    the rounded P, 1 / l in the epilogue, bf16 output.  [B, S, H * 128] bf16."""
    Bq, S, H, hd = q.shape
    Hkv, L = kc.shape[1], pos + S
    G = H // Hkv
    sl = torch.tensor(hd ** -0.5, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    qg = q.float().view(Bq, S, Hkv, G, hd).permute(0, 2, 3, 1, 4)  # [B, Hkv, G, S, hd]
    sc = (qg @ kc[:, :, :L].float().transpose(-1, -2).unsqueeze(2)) * sl
    seen = torch.arange(L)[None, :] <= pos + torch.arange(S)[:, None]
    sc = sc.masked_fill(~seen, -INF)
    v = vc[:, :, :L].float().unsqueeze(2)
    m = torch.full(sc.shape[:-1], -INF)
    l = torch.zeros(sc.shape[:-1])
    o = torch.zeros(*sc.shape[:-1], hd)
    for k0 in range(0, L, WC.KT):
        blk = sc[..., k0:k0 + WC.KT]
        mn = torch.maximum(m, blk.max(-1).values)  # finite: key 0 is in the first tile
        corr = rescale(m - mn)
        p = torch.exp2(blk - mn.unsqueeze(-1)).bfloat16().float()
        l = l * corr + p.sum(-1)
        o = o * corr.unsqueeze(-1) + p @ v[..., k0:k0 + WC.KT, :]
        m = mn
    out = (o * (1.0 / l).unsqueeze(-1)).bfloat16()
    return out.permute(0, 3, 1, 2, 4).reshape(Bq, S, H * hd)


@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_emulated_kernel_arithmetic_stays_within_the_ramp_bound(S, pos, H, Hkv):
    q, kc, vc = WC.ramp_case(S, pos, H, Hkv)
    ref, bound = WC.ramp_ref(S, pos, H, Hkv)
    out = _emulate(q, kc, vc, pos)
    frac = WC.fraction(out, ref, bound)
    print(f"emulation S={S} pos={pos} H={H} Hkv={Hkv}: {frac:.3f} of the ramp bound")
    assert torch.isfinite(out.float()).all()
    assert not WC.outside(out, ref, bound).any(), f"{frac:.3f} of the bound"


@pytest.mark.parametrize("S,pos,H,Hkv", [(300, 37, 2, 2), (129, 130, 8, 2)])
def test_ramp_bound_catches_a_rescale_in_the_wrong_base(S, pos, H, Hkv):
    """The bound is not so wide that it hides what it is for: the emulation with
    corr = exp(m - mn) on log2-domain values leaves it."""
    q, kc, vc = WC.ramp_case(S, pos, H, Hkv)
    ref, bound = WC.ramp_ref(S, pos, H, Hkv)
    assert WC.outside(_emulate(q, kc, vc, pos, rescale=torch.exp), ref, bound).any()


# ------------------------------------------------------------------ 5. ragged and paged forms
@pytest.mark.parametrize("kind", ["census", "ramp"])
@pytest.mark.parametrize("pairs", WC.RAGGED)
def test_ragged_fixture_follows_the_conventions_of_ragged_cases(kind, pairs):
    H, Hkv = 8, 2
    q, kc, vc, pos, lens, expect = WC.ragged_case(kind, pairs, H, Hkv)
    S = max(0 if p is None else p[0] for p in pairs)
    assert q.shape == (WC.B, S, H, WC.HD) and kc.shape == vc.shape == (WC.B, Hkv, WC.C, WC.HD)
    for b, pair in enumerate(pairs):
        if pair is None:
            assert (pos[b], lens[b]) == (-1, 0)
            assert torch.isnan(q[b].float()).all() and torch.isnan(kc[b].float()).all()
            assert torch.isnan(vc[b].float()).all()
            assert expect is None or not expect[b].any()
            continue
        n, p = pair
        uq, uk, uv, ue = WC._uniform(kind, n, p, H, Hkv)
        assert (pos[b], lens[b]) == (p, n)
        assert torch.equal(_bits(q[b, :n]), _bits(uq[b])) and torch.isnan(q[b, n:].float()).all()
        assert torch.equal(_bits(kc[b]), _bits(uk[b])) and torch.equal(_bits(vc[b]), _bits(uv[b]))
        assert torch.isnan(kc[b, :, p + n:].float()).all() and torch.isnan(vc[b, :, p + n:].float()).all()
        if expect is not None:
            assert torch.equal(expect[b, :n], ue[b]) and not expect[b, n:].any()


def _check_round_trip(c, page, B):
    """Pools -> gather_dense gives back each sequence's first rows[b] rows, NaN
    elsewhere; every pool row that is not one of them is NaN."""
    live = torch.zeros(c["P"], page, dtype=torch.bool)
    for name, pool in (("kc", c["kpool"]), ("vc", c["vpool"])):
        assert pool.shape[0] == c["P"] and pool.shape[2] == page
        dense = PG.gather_dense(pool, c["ids"], c["rows"], c["Cl"])
        assert dense.shape[2] == c["Cl"] == c["NP"] * page
        for b, r in enumerate(c["rows"]):
            assert torch.equal(_bits(dense[b, :, :r]), _bits(c[name][b, :, :r]))
            assert torch.isnan(dense[b, :, r:].float()).all()
            assert len(c["ids"][b]) == -(-r // page)
            for i, pg in enumerate(c["ids"][b]):
                live[pg, :min(page, r - i * page)] = True
        assert torch.isnan(pool.transpose(1, 2)[~live].float()).all()
        assert torch.isfinite(pool.transpose(1, 2)[live].float()).all()
    used = [pg for ids in c["ids"] for pg in ids]
    assert len(set(used)) == len(used) and c["P"] == len(used) + PG.SPARE
    assert c["table"].shape == (B, c["NP"]) and c["table"].dtype == torch.int32
    for b, ids in enumerate(c["ids"]):
        assert c["table"][b, :len(ids)].tolist() == ids
        assert all(int(e) in PG.GARBAGE for e in c["table"][b, len(ids):])  # entries no kernel may read


@pytest.mark.parametrize("page", WC.PAGES)
@pytest.mark.parametrize("kind", ["census", "ramp"])
@pytest.mark.parametrize("pairs", WC.RAGGED)
def test_paged_prefill_fixture_round_trips(pairs, kind, page):
    c = WC.paged_case(kind, pairs, 8, 2, page)
    assert c["Cl"] == {64: 448, 128: 512, 256: 512}[page] and c["NP"] == {64: 7, 128: 4, 256: 2}[page]
    assert c["rows"] == [0 if p is None else p[0] + p[1] for p in pairs]
    _check_round_trip(c, page, WC.B)


@pytest.mark.parametrize("s", range(len(PG.PREFILL_SETS)))
def test_one_hot_paged_fixture_at_page_256(s):
    c = PG.prefill_case(s, 8, 2, 256)
    assert (c["NP"], c["Cl"]) == (2, 512)
    _check_round_trip(c, 256, WC.B)


def test_decode_sets_at_page_256_follow_the_paged_idle_rule():
    assert (WC.DECODE_PAGE, WC.DECODE_CL, PG.n_table(DC.C, WC.DECODE_PAGE)) == (256, 1280, 5)
    assert WC.DECODE_SETS == [[0, 63, 512, 1099], [1099, 64, -1, 511], [1023, 1024, 575, 62], [-1, -1, 1280, 5]]
    for ours, theirs in zip(WC.DECODE_SETS, PG.DECODE_SETS):  # the same slots are idle as at pages 64 / 128
        assert [WC.decode_active(p) for p in ours] == [PG.decode_active(p) for p in theirs]
    # four 64-key steps per page, and steps of 512 keys across page edges: all of it needs more than one page
    assert max(p for s in WC.DECODE_SETS for p in s if WC.decode_active(p)) // 256 == 4


@pytest.mark.parametrize("kind", WC.DECODE_KINDS)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (2, 2)])
@pytest.mark.parametrize("s", range(len(WC.DECODE_SETS)))
def test_decode_fixture_at_page_256_round_trips(s, H, Hkv, kind):
    c = WC.decode_case_256(kind, s, H, Hkv)
    assert (c["NP"], c["Cl"]) == (5, 1280)
    assert c["rows"] == [p + 1 if WC.decode_active(p) else 0 for p in c["positions"]]
    _check_round_trip(c, 256, DC.B)
    for b, p in enumerate(c["positions"]):
        if not WC.decode_active(p):
            assert torch.isnan(c["q"][b].float()).all() and c["expect"][b] is None
            continue
        e, bound = c["expect"][b], c["bound"][b]
        assert e.shape == (H * DC.HD,) and (bound is None) == (kind == "exact")
        if kind == "exact":
            continue
        # the sequence's row of the fixture at its own position: the fp64 reference meets its expectation
        ref = DC.ref64(c["q"], c["kc"], c["vc"], p)[b]
        torch.testing.assert_close(ref, e.double(), rtol=1e-12, atol=1e-12)
        assert (bound >= 0).all() and bound.shape == e.shape

"""k_decode_attn / k_decode_attn_combine on the MI355X against exact data and an
fp64 reference (csrc/hip/decode_kernels.hip), with caches long enough that a
wave runs its online-softmax loop more than once."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu

B, HD, C = DC.B, DC.HD, DC.C
EXACT = [(pos, H, Hkv) for pos in DC.POSITIONS for (H, Hkv) in DC.HEADS]
CENSUS = [(L, H, Hkv) for L in DC.CENSUS_L for (H, Hkv) in DC.HEADS]
RAMP = [(pos, H, Hkv) for pos in DC.RAMP_POSITIONS for (H, Hkv) in DC.HEADS]


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _pos(pos):
    return torch.tensor([pos], dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def _ramp(pos, H, Hkv):
    """One ramp case and its fp64 reference, shared (and left unchanged) by the
    tests that need it."""
    q, kc, vc = DC.ramp_case(pos, H, Hkv, seed=0)
    return q, kc, vc, DC.ref64(q, kc, vc, pos)


def _bound(ref, vmax):
    """The rounding of the result to bf16 (half an ulp of 8 significant bits is at
    most 2^-8 of the value) plus the fp32 worst case: a 128-term dot
    product at |score| <= 40 is off by at most 3e-4, hence that relative error
    in a weight; an L-term fp32 sum adds less than L 2^-24.  That derivation is
    for the ramp fixture.  The one-hot data of the first-masked-key test score
    in the hundreds, but as sums of 16 terms of one magnitude: a score is off by
    a few fp32 ulps of ~1.4e3 (about 1e-4, no more than the ramp's 3e-4), tied
    keys keep weights equal to that, every other weight underflows to 0 (the
    gap is a multiple of ~181), and V holds small integers."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -10 * vmax


def _terms(out, ref, vmax):
    """The observed maximum of the error in units of each term of _bound (the
    first over the elements with ref != 0: small |ref| dominate it)."""
    err = (out - ref).abs()
    nz = ref != 0
    return (err[nz] / ref[nz].abs()).max().item() * 2 ** 8, err.max().item() / vmax * 2 ** 10


@pytest.mark.parametrize("pos,H,Hkv", EXACT)
def test_exact_data_selects_the_target_value_row_bit_for_bit(pos, H, Hkv):
    """Every wave, every loop iteration and every split edge is some head's
    target; the rest of the cache is NaN."""
    q, kc, vc, t, expect = DC.exact_case(pos, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    for ns in DC.NSPLITS:
        out = llm.decode_attn(qd, kd, vd, _pos(pos), ns).cpu()
        assert out.shape == (B, H * HD) and out.dtype == torch.bfloat16
        bad = (out.view(torch.int16) != expect.view(torch.int16)).view(B, H, HD).any(-1).nonzero()
        assert bad.numel() == 0, (f"nsplit={ns}: {bad.shape[0]} wrong (b, h) rows, first {bad[:8].tolist()} with "
                                  f"targets {[int(t[b, h]) for b, h in bad[:8].tolist()]}")


@pytest.mark.parametrize("pos,H,Hkv", [c for c in EXACT if c[0] + 1 < C])
def test_first_masked_key_is_not_seen(pos, H, Hkv):
    """Every target moves up by one and row pos + 1 carries its code: a head whose
    target was the last visible key now aims at the first masked one, and
    L = pos + 2 would return that key's V row."""
    q, kc, vc, t, leaked = DC.exact_case(pos, H, Hkv, shift=1)
    hidden = t == pos + 1
    assert hidden[0, 0] and torch.equal(hidden, DC.targets(pos, H) == pos)
    ref = DC.ref64(q, kc, vc, pos)
    vmax = vc[:, :, :pos + 1].float().abs().max().item()
    qd, kd, vd = _cuda(q, kc, vc)
    for ns in DC.NSPLITS:
        out = llm.decode_attn(qd, kd, vd, _pos(pos), ns).cpu()
        same = (out.view(torch.int16) == leaked.view(torch.int16)).view(B, H, HD).all(-1)
        assert not (same & hidden).any(), f"nsplit={ns}: (b, h) {(same & hidden).nonzero().tolist()} see key {pos + 1}"
        out = out.double()
        rel, absv = _terms(out, ref, vmax)
        print(f"first-masked-key pos={pos} H={H} Hkv={Hkv} nsplit={ns}: {rel:.3g} x 2^-8 |ref|, "
              f"{absv:.3g} x 2^-10 max|V|")
        assert ((out - ref).abs() <= _bound(ref, vmax)).all(), (ns, rel, absv)


@pytest.mark.parametrize("L,H,Hkv", CENSUS)
def test_census_counts_every_key_once(L, H, Hkv):
    """q = 0: every weight is 1 and l = L exactly; V counts the keys of each
    residue mod 128.  The fp32 work is L * 256 * (1 / L) on exact integers, so the
    only error is 1 / L and one multiply in fp32 (2^-23) and the rounding to
    bf16: at most 2^-8 of the power of two below the value, and at these L
    256 count / L is such a power or at least 2^-6 above it."""
    q, kc, vc, expect = DC.census_case(L, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    for ns in DC.NSPLITS:
        out = llm.decode_attn(qd, kd, vd, _pos(L - 1), ns).cpu().double()
        assert torch.isfinite(out).all(), f"nsplit={ns}: {(~torch.isfinite(out)).sum().item()} non-finite outputs"
        err = (out - expect).abs()
        bad = (~(err <= 2.0 ** -8 * expect.abs())).view(B, H, HD).nonzero()  # NaN counts as outside
        assert bad.numel() == 0, (f"nsplit={ns}: {bad.shape[0]} wrong (b, h, d), first {bad[:8].tolist()}: got "
                                  f"{[out.view(B, H, HD)[tuple(i)].item() for i in bad[:4].tolist()]} for "
                                  f"{[expect.view(B, H, HD)[tuple(i)].item() for i in bad[:4].tolist()]}")
        assert (out[expect == 0] == 0).all()


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
def test_single_key_returns_its_value_row(H, Hkv):
    """pos = 0: softmax of one key is 1 and a * (1 / 1) is exact, through the
    combine kernel with 7 empty splits too."""
    g = torch.Generator().manual_seed(H)
    q = torch.randn(B, H, HD, generator=g).bfloat16()
    kc = torch.full((B, Hkv, C, HD), float("nan"), dtype=torch.bfloat16)
    vc = kc.clone()
    kc[:, :, 0] = torch.randn(B, Hkv, HD, generator=g).bfloat16()
    vc[:, :, 0] = torch.randn(B, Hkv, HD, generator=g).bfloat16()
    expect = vc[:, :, 0].repeat_interleave(H // Hkv, dim=1).reshape(B, H * HD)
    qd, kd, vd = _cuda(q, kc, vc)
    for ns in DC.NSPLITS:
        out = llm.decode_attn(qd, kd, vd, _pos(0), ns).cpu()
        assert torch.equal(out.view(torch.int16), expect.view(torch.int16)), f"nsplit={ns}"


@pytest.mark.parametrize("pos,H,Hkv", RAMP)
def test_ramp_against_fp64(pos, H, Hkv):
    """The running max of the even heads rises by a few nats per loop iteration
    (tests/test_decode_attn_cpu.py), so l * corr and o *= corr act on finite
    values with 0 < corr < 1."""
    q, kc, vc, ref = _ramp(pos, H, Hkv)
    vmax = vc[:, :, :pos + 1].float().abs().max().item()
    qd, kd, vd = _cuda(q, kc, vc)
    for ns in DC.NSPLITS:
        out = llm.decode_attn(qd, kd, vd, _pos(pos), ns).cpu().double()
        rel, absv = _terms(out, ref, vmax)
        worst = ((out - ref).abs() / _bound(ref, vmax)).max().item()
        print(f"ramp pos={pos} G={H // Hkv} nsplit={ns}: {rel:.3g} x 2^-8 |ref|, {absv:.3g} x 2^-10 max|V|, "
              f"{worst:.3g} of the bound")
        assert torch.isfinite(out).all(), f"nsplit={ns}: {(~torch.isfinite(out)).sum().item()} non-finite outputs"
        bad = (~((out - ref).abs() <= _bound(ref, vmax))).view(B, H, HD).any(-1).nonzero()  # NaN counts as outside
        assert bad.numel() == 0, f"nsplit={ns}: (b, h) {bad[:8].tolist()} outside the bound ({worst:.3g} of it)"


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
def test_equal_calls_give_equal_bits(H, Hkv):
    q, kc, vc, _ = _ramp(C - 1, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    for ns in DC.NSPLITS:
        a = llm.decode_attn(qd, kd, vd, _pos(C - 1), ns)
        b = llm.decode_attn(qd, kd, vd, _pos(C - 1), ns)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"nsplit={ns}"


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
@pytest.mark.parametrize("pos", [62, 512, 1024])
def test_stale_rows_do_not_reach_the_output(pos, H, Hkv):
    """Rows > pos hold NaN, finite garbage of an earlier request, or +inf: the
    output bits are the same."""
    qd, kd, vd = _cuda(*DC.ramp_case(pos, H, Hkv, seed=1))
    n = C - (pos + 1)
    g = torch.Generator().manual_seed(pos)
    fills = {"nan": None, "randn * 100": (torch.randn(B, Hkv, n, HD, generator=g) * 100).bfloat16().cuda(),
             "+inf": torch.full((B, Hkv, n, HD), float("inf"), dtype=torch.bfloat16, device="cuda")}
    for ns in DC.NSPLITS:
        outs = {}
        for name, fill in fills.items():
            if fill is not None:
                kd[:, :, pos + 1:] = fill
                vd[:, :, pos + 1:] = fill
            else:
                kd[:, :, pos + 1:] = float("nan")
                vd[:, :, pos + 1:] = float("nan")
            outs[name] = llm.decode_attn(qd, kd, vd, _pos(pos), ns)
            assert torch.isfinite(outs[name].float()).all(), f"nsplit={ns}, fill {name}"
        for name in ("randn * 100", "+inf"):
            assert torch.equal(outs[name].view(torch.int16), outs["nan"].view(torch.int16)), f"nsplit={ns}, {name}"


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
def test_device_position_changes_in_place(H, Hkv):
    """As the captured graph does: the same tensors, pos_t refilled between the
    calls.  A short context after a long one leaves nothing behind in the
    workspace of the splits."""
    q, kc, vc = DC.ramp_case(C - 1, H, Hkv, seed=2)
    ref64 = DC.ref64(q, kc, vc, 64)
    vmax = vc[:, :, :65].float().abs().max().item()
    qd, kd, vd = _cuda(q, kc, vc)
    pos_t = _pos(C - 1)
    for ns in DC.NSPLITS:
        outs = []
        for p in (C - 1, 64, C - 1):
            pos_t.fill_(p)
            outs.append(llm.decode_attn(qd, kd, vd, pos_t, ns))
        assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16)), f"nsplit={ns}"
        assert not torch.equal(outs[0], outs[1])
        assert ((outs[1].cpu().double() - ref64).abs() <= _bound(ref64, vmax)).all(), f"nsplit={ns}"

"""Decode attention: the fixtures of tests/decode_cases.py do what they claim,
and the wrappers refuse what the kernels cannot do before they touch the
library.  Everything that can be checked without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

B, HD, C = DC.B, DC.HD, DC.C


def test_geometry_reaches_the_third_iteration_of_a_wave():
    """nsplit = 1: wave w takes keys 64 w + 512 i; C = 1100 gives wave 0 a full
    third step, wave 1 a partial one, and every wave a second one."""
    steps = [[(base, min(64, C - base)) for base in range(64 * w, C, 512)] for w in range(8)]
    assert all(len(s) >= 2 for s in steps)
    assert steps[0][2] == (1024, 64) and steps[1][2] == (1088, 12) and len(steps[2]) == 2
    assert C - 1 in DC.POSITIONS and max(DC.CENSUS_L) == C


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
@pytest.mark.parametrize("pos", DC.POSITIONS)
def test_exact_fixture_selects_one_value_row(pos, H, Hkv):
    """The reference returns V[t] bit for bit; with shift = 1 the fixture codes
    row pos + 1 too, and the expected row is what a mask one too loose returns."""
    q, kc, vc, t, expect = DC.exact_case(pos, H, Hkv)
    assert int(t.max()) <= pos and int(t[0, 0]) == pos and int(t.min()) == 0
    assert torch.isnan(kc[:, :, pos + 1:].float()).all() and torch.isnan(vc[:, :, pos + 1:].float()).all()
    assert torch.isfinite(kc[:, :, :pos + 1].float()).all() and torch.isfinite(vc[:, :, :pos + 1].float()).all()
    out = llm.prefill_attn_ref(q.view(B, 1, H, HD), kc, vc, pos)
    assert torch.equal(out.view(B, H * HD), expect.float())
    if pos + 1 < C:
        q, kc, vc, t1, leaked = DC.exact_case(pos, H, Hkv, shift=1)
        assert torch.equal(t1, t + 1) and int(t1[0, 0]) == pos + 1
        assert torch.isnan(kc[:, :, pos + 2:].float()).all() and torch.isfinite(kc[:, :, :pos + 2].float()).all()
        loose = llm.prefill_attn_ref(q.view(B, 1, H, HD), kc, vc, pos + 1)
        assert torch.equal(loose.view(B, H * HD), leaked.float())
        tight = llm.prefill_attn_ref(q.view(B, 1, H, HD), kc, vc, pos).view(B, H, HD)
        hidden = t1 == pos + 1
        assert not (tight == leaked.float().view(B, H, HD)).all(-1)[hidden].any()
        assert torch.equal(tight[~hidden], leaked.float().view(B, H, HD)[~hidden])


def test_exact_fixture_targets_every_edge():
    """At the last position the 32 (b, h) of H = 8 meet every boundary, so every
    wave step, loop iteration and split edge is some head's target."""
    t = DC.targets(C - 1, 8)
    assert set(t.flatten().tolist()) == {C - 1 if e is None else e for e in DC.BOUNDARY}


@pytest.mark.parametrize("L", [1, 5, 64, 130, 513, 1100])
def test_census_fixture_counts_the_keys(L):
    for H, Hkv in DC.HEADS:
        q, kc, vc, expect = DC.census_case(L, H, Hkv)
        assert not q.any() and torch.isfinite(kc[:, :, :L].float()).all()
        assert torch.isnan(kc[:, :, L:].float()).all() and torch.isnan(vc[:, :, L:].float()).all()
        count = torch.tensor([len(range(d, L, 128)) for d in range(HD)], dtype=torch.float64)
        assert torch.equal(vc[0, 0, :L].double().sum(0), 256 * count) and count.sum() == L and count.max() <= 9
        want = (256 * count / L).repeat(H).expand(B, H * HD)
        ref = DC.ref64(q, kc, vc, L - 1)
        assert ref.dtype == torch.float64
        assert (ref - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        assert (expect - want).abs().max().item() <= 1e-12 * want.abs().max().item()
        assert torch.equal(expect == 0, want == 0)


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
def test_ramp_fixture_moves_the_running_max(H, Hkv):
    """Even heads: the running max that a wave of k_decode_attn carries (nsplit =
    1: wave w sees keys [64 w + 512 i, + 64) at iteration i) rises at every
    iteration by 0.5 .. 30 nats, for every batch, even head, wave and iteration:
    corr = exp(-rise) is neither 1 nor lost to fp32 underflow.  So does the
    maximum over the full 512-key blocks 0 and 1.  Odd heads: block 0 holds the
    maximum.

    The maximum over the partial third block (keys 1024..1099, 76 keys against
    512) is within +-30 nats of block 1 but does not rise for every head: the
    ramp gains 0.8 .. 1.4 nats there, about what the maximum of 76 random
    scores loses against that of 512 (head 0 of batch 0 at (H, Hkv) = (8, 2):
    7.4, 12.3, 12.9; over the four head pairs the last step spans -0.56 .. 2.4).
    The kernel never forms that
    maximum; the per-wave rises above are what its rescale acts on."""
    pos = C - 1
    q, kc, vc = DC.ramp_case(pos, H, Hkv, seed=0)
    sc = DC.scores64(q, kc, pos)  # [B, H, L]
    assert sc.abs().max().item() <= 40  # the premise of the fp32 error bound of the GPU test
    even = sc[:, 0::2]
    lo, hi = float("inf"), float("-inf")
    for w in range(8):
        mx = [even[..., base:base + 64].amax(-1) for base in range(64 * w, pos + 1, 512)]
        assert len(mx) == (3 if w < 2 else 2)
        for a, b in zip(mx[:-1], mx[1:]):
            lo, hi = min(lo, (b - a).min().item()), max(hi, (b - a).max().item())
    mx = torch.stack([sc[..., i:i + 512].amax(-1) for i in range(0, pos + 1, 512)], -1)  # [B, H, 3]
    assert mx.shape[-1] == 3
    rise = mx[:, 0::2, 1:] - mx[:, 0::2, :-1]
    print(f"H={H} Hkv={Hkv}: per-wave rises {lo:.3g} .. {hi:.3g}; head 0 block maxima {mx[0, 0].tolist()}, "
          f"block rises {rise[..., 0].min():.3g} .. {rise[..., 0].max():.3g} then "
          f"{rise[..., 1].min():.3g} .. {rise[..., 1].max():.3g}")
    assert lo > 0.5 and hi < 30
    assert rise[..., 0].min().item() > 0.5 and rise[..., 0].max().item() < 30
    assert rise[..., 1].abs().max().item() < 30
    if H > 1:
        assert (mx[:, 1::2].argmax(-1) == 0).all()


def test_ramp_fixture_hides_rows_past_pos():
    q, kc, vc = DC.ramp_case(512, 8, 2, seed=0)
    for t in (kc, vc):
        assert torch.isfinite(t[:, :, :513].float()).all() and torch.isnan(t[:, :, 513:].float()).all()


# ------------------------------------------------------------------ validation before the library
def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


def _args(H=8, Hkv=2, hd=128, Cn=16):
    bf = torch.bfloat16
    return (torch.zeros(2, H, hd, dtype=bf), torch.zeros(2, Hkv, Cn, hd, dtype=bf),
            torch.zeros(2, Hkv, Cn, hd, dtype=bf), torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("case,match", [
    ("strided_kc", "kc must be contiguous"), ("fp32_kc", "kc must be bf16"), ("vc_shape", "of one shape"),
    ("q_shape", r"q .* must be \[B, H, 128\]"), ("q_4d", r"q .* must be \[B, H, 128\]"), ("hd64", "128"),
    ("g3", "group size"), ("pos_int64", "1-element int32"), ("pos_two", "1-element int32"),
    ("pos_cpu", "pos_t must be a CUDA tensor"), ("nsplit0", "nsplit"), ("nsplit_float", "nsplit")])
def test_decode_attn_rejects_bad_arguments_before_the_library(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    q, kc, vc, pos_t = _args()
    nsplit = None
    if case == "strided_kc":
        kc = torch.zeros(2, 2, 32, 128, dtype=torch.bfloat16)[:, :, ::2]
        assert kc.shape == vc.shape and not kc.is_contiguous()
    elif case == "fp32_kc":
        kc = kc.float()
    elif case == "vc_shape":
        vc = torch.zeros(2, 2, 17, 128, dtype=torch.bfloat16)
    elif case == "q_shape":
        q = torch.zeros(3, 8, 128, dtype=torch.bfloat16)  # batch of another size
    elif case == "q_4d":
        q = q.view(2, 1, 8, 128)
    elif case == "hd64":
        q, kc, vc, pos_t = _args(hd=64)
    elif case == "g3":
        q, kc, vc, pos_t = _args(H=6)
    elif case == "pos_int64":
        pos_t = pos_t.long()
    elif case == "pos_two":
        pos_t = torch.zeros(2, dtype=torch.int32)
    elif case == "pos_cpu":
        pass  # every other argument is as good as it can be without a GPU
    elif case == "nsplit0":
        nsplit = 0
    else:
        nsplit = 2.0
    with pytest.raises(ValueError, match=match):
        llm.decode_attn(q, kc, vc, pos_t, nsplit)


@pytest.mark.parametrize("case", ["pos_cpu", "pos_two", "pos_int64"])
def test_qkv_rope_cache_rejects_a_bad_position_tensor_before_the_library(case, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    _, kc, vc, pos_t = _args()
    qkv = torch.zeros(2, 1, (8 + 4) * 128, dtype=torch.bfloat16)
    cos = torch.zeros(16, 64)
    if case == "pos_two":
        pos_t = torch.zeros(2, dtype=torch.int32)
    elif case == "pos_int64":
        pos_t = pos_t.long()
    with pytest.raises(ValueError, match="pos_t must be a" if case != "pos_cpu" else "pos_t must be a CUDA tensor"):
        llm.qkv_rope_cache(qkv, cos, cos.clone(), pos_t, kc, vc, 8)


def test_qkv_rope_cache_rejects_caches_of_another_rank_or_shape(monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    _, kc, vc, pos_t = _args()
    qkv = torch.zeros(2, 1, (8 + 4) * 128, dtype=torch.bfloat16)
    cos = torch.zeros(16, 64)
    for k, v in ((kc[0], vc[0]), (kc, vc[:, :, :8].contiguous())):
        with pytest.raises(ValueError, match="of one shape"):
            llm.qkv_rope_cache(qkv, cos, cos.clone(), pos_t, k, v, 8)

"""The fp8 KV-cache codec (llm.kv8_quant_ref / kv8_dequant), the plain-torch
reference of the _kv8 attention kernels on the fp8 fixtures of
tests/kv8_cases.py, and LlamaDecoder(paged=True, kv_fp8=True) on its eager
path.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import kv8_cases as K8  # noqa: E402
import paged_cases as PG  # noqa: E402
import prefill_cases as PC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

BF = torch.bfloat16
DECODE = [(s, H, Hkv, page) for s in range(len(PG.DECODE_SETS)) for (H, Hkv) in DC.HEADS for page in PG.PAGES]
PREFILL = [(s, H, Hkv, page) for s in range(len(PG.PREFILL_SETS)) for (H, Hkv) in PC.HEADS for page in PG.PAGES]


# ------------------------------------------------------------------ the codec
def _random_rows(n=4096, seed=0):
    """bf16 rows with magnitudes 2^-30 .. 2^30, then rows with amax 0, 448 and 450."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-30, 31, (n, 1), generator=g).float()
    x = (torch.randn(n, 128, generator=g) * 2.0 ** k).to(BF)
    tail = torch.zeros(3, 128, dtype=BF)
    tail[1, 7], tail[2, 9] = 448.0, -450.0
    return torch.cat([x, tail])


def _frexp_form(x):
    """The codec as the issue states it, with torch.frexp / torch.ldexp."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(min=-100)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    return torch.ldexp(xf, -e.unsqueeze(-1)).to(torch.float8_e4m3fn), torch.ldexp(torch.ones_like(amax), e), e


def _check_codec(x):
    codes, scale = llm.kv8_quant_ref(x)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    c2, s2, e = _frexp_form(x)
    assert torch.equal(scale, s2) and torch.equal(codes.view(torch.uint8), c2.view(torch.uint8))
    amax = x.float().abs().amax(-1)
    nz = amax > 0
    unclamped = nz & (e > -100)
    ratio = amax[unclamped] / scale[unclamped]
    assert (ratio > 224).all() and (ratio <= 448).all(), (ratio.min().item(), ratio.max().item())
    assert (amax[nz] / scale[nz] <= 448).all()  # the clamp only makes codes smaller
    assert torch.isfinite(codes.float()).all()  # nothing saturates to the NaN code
    prod = codes.float() * scale.unsqueeze(-1)  # the fp32 product
    deq = llm.kv8_dequant(codes, scale)
    assert deq.dtype == BF and torch.equal(deq.float(), prod), "dequantisation rounds somewhere"
    err = (prod - x.float()).abs().amax(-1)
    assert (err <= 16 * scale).all()
    assert (err[unclamped] * 14 < amax[unclamped]).all(), (err[unclamped] / amax[unclamped]).max().item()
    return codes, scale, e


def test_codec_properties_on_random_rows():
    x = _random_rows()
    codes, scale, _ = _check_codec(x)
    assert scale[-3:].tolist() == [1.0, 1.0, 2.0]  # amax 0, 448, 450
    assert not codes[-3].view(torch.uint8).any()  # a zero row: scale 1 and zero codes
    assert codes[-2, 7].float().item() == 448.0 and codes[-1, 9].float().item() == -224.0


def test_codec_on_the_edge_rows():
    rows, want_e = K8.edge_rows()
    _, scale, e = _check_codec(rows)
    assert torch.equal(e, want_e), (e.tolist(), want_e.tolist())
    assert torch.equal(scale, torch.ldexp(torch.ones(len(want_e)), want_e))
    assert (want_e == -100).sum() == 2 and (rows[want_e == -100] != 0).any()  # the clamp is met


def test_the_codec_is_not_idempotent_in_the_scale():
    """An amax that rounds down to 224 x scale gets half the scale on a second
    pass: nothing may rely on requantising (the decoder never does)."""
    x = torch.zeros(1, 128, dtype=BF)
    x[0, 0] = 230.0  # scale 1, code 224
    c1, s1 = llm.kv8_quant_ref(x)
    c2, s2 = llm.kv8_quant_ref(llm.kv8_dequant(c1, s1))
    assert (s1.item(), c1[0, 0].float().item(), s2.item(), c2[0, 0].float().item()) == (1.0, 224.0, 0.5, 448.0)


# ------------------------------------------------------------------ the reference on the fixtures
def _live_ok(c):
    live = c["live"][:, None, :].expand(c["kscale"].shape)
    for name in ("k", "v"):
        assert (c[name + "pool8"].view(torch.uint8)[~live] == K8.NAN_CODE).all()
        assert torch.isnan(c[name + "scale"][~live]).all() and torch.isfinite(c[name + "scale"][live]).all()


@pytest.mark.parametrize("s,H,Hkv,page", DECODE)
@pytest.mark.parametrize("shift", [0, 1])
def test_reference_on_the_decode_fixtures_returns_the_dequantised_value_row(s, H, Hkv, page, shift):
    c = K8.decode_case(s, H, Hkv, page, shift)
    _live_ok(c)
    lens = [1 if PG.decode_active(p) else 0 for p in c["positions"]]
    out = llm.attn_paged_kv8_ref(c["q"].unsqueeze(1), c["kpool8"], c["vpool8"], c["kscale"], c["vscale"], c["table"],
                                 c["positions"], lens)[:, 0]
    assert torch.equal(out, llm.attn_paged_ref(c["q"].unsqueeze(1), c["ktwin"], c["vtwin"], c["table"],
                                               c["positions"], lens)[:, 0])
    want = c["expect8"].float()
    for b, p in enumerate(c["positions"]):
        row, w = out[b].view(H, DC.HD), want[b].view(H, DC.HD)
        if shift and PG.decode_active(p) and p + 1 < DC.C:
            hidden = c["t"][b] == p + 1
            same = (row == w).all(-1)
            assert hidden.any() or b, "the fixture aims head 0 of sequence 0 at the first masked key"
            assert not (same & hidden).any() and same[~hidden].all()
        else:
            assert torch.equal(row, w), f"sequence {b} at pos {p}"


@pytest.mark.parametrize("s,H,Hkv,page", PREFILL)
def test_reference_on_the_prefill_fixtures_returns_the_dequantised_value_rows(s, H, Hkv, page):
    c = K8.prefill_case(s, H, Hkv, page)
    _live_ok(c)
    out = llm.attn_paged_kv8_ref(c["q"], c["kpool8"], c["vpool8"], c["kscale"], c["vscale"], c["table"], c["pos"],
                                 c["lens"])
    assert torch.equal(out, c["expect8"].float())
    assert not torch.equal(c["expect8"], c["expect"])


def test_page_256_and_weighted_fixtures_quantise_and_poison():
    c = K8.decode_case_256("exact", 0, 8, 2)
    _live_ok(c)
    assert c["kpool8"].shape[2] == 256 and c["expect8"][0] is not None
    w = K8.weighted_case("ramp", ((65, 64), (129, 130)), 8, 2, 256)
    _live_ok(w)
    live = w["live"][:, None, :, None].expand_as(w["kpool"])
    err = (w["vtwin"].float() - w["vpool"].float())[live].abs().max().item()
    assert 0 < err < w["vpool"].float()[live].abs().max().item() / 14


# ------------------------------------------------------------------ the eager decoder
CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, PAGE, PAGES = 4, 200, 64, 12


def _decoder(state=None, **kw):
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, device="cpu", dtype=torch.float64, fused=False, paged=True,
                     pages=PAGES, page=PAGE, **kw)
    if state is not None:
        d.model.load_state_dict(state)
    return d


def _spy(d, call):
    seen, fwd = [], d._forward_paged

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].clone())
        return r

    d._forward_paged = spy
    try:
        return call(), seen
    finally:
        d._forward_paged = fwd


def test_eager_decoder_rounds_the_cache_through_the_codec():
    plain = _decoder()
    state = plain.model.state_dict()
    whole, chunked = _decoder(state, kv_fp8=True), _decoder(state, kv_fp8=True)
    prompts = torch.randint(0, CFG.vocab, (BATCH, 150), generator=torch.Generator().manual_seed(5))
    (t0, l0), (t1, l1), (t2, l2) = (_spy(d, lambda: d.prefill(prompts, **kw))
                                    for d, kw in ((plain, {}), (whole, {}), (chunked, {"chunk": 64})))
    assert len(l0) == len(l1) == len(l2) == 1
    # chunked and unchunked prefill: every query sees the same rounded rows, in the same arithmetic
    assert torch.equal(l1[0], l2[0]) and torch.equal(t1, t2)
    # the flag does something
    assert not torch.equal(l0[0], l1[0])
    assert (l0[0] - l1[0]).abs().max() < 0.1 * l0[0].abs().max()
    # layer 0 sees the same inputs in both decoders: its pool rows are the plain decoder's through the codec
    for b in range(BATCH):
        for i in (0, 1):
            rows = llm.paged_gather(plain.cache[0][i], plain.pages_of(b), 150)
            got = llm.paged_gather(whole.cache[0][i], whole.pages_of(b), 150)
            assert torch.equal(got, llm.kv8_dequant(*llm.kv8_quant_ref(rows)).to(got.dtype))
            assert not torch.equal(got, rows)
            assert torch.equal(got, llm.paged_gather(chunked.cache[0][i], chunked.pages_of(b), 150))
    # a decode step rounds its new row too
    n0, n1 = plain.decode_step(t0), whole.decode_step(t1)
    assert n0.shape == n1.shape == (BATCH, 1)
    k0 = llm.paged_gather(plain.cache[0][0], plain.pages_of(0), 151)[:, 150]
    k1 = llm.paged_gather(whole.cache[0][0], whole.pages_of(0), 151)[:, 150]
    if torch.equal(t0, t1):  # the same token went in: the same layer-0 row, through the codec
        assert torch.equal(k1, llm.kv8_round(k0))


def test_kv_fp8_needs_a_paged_cache_and_emulation_is_not_captured():
    with pytest.raises(ValueError, match="paged=True"):
        LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, device="cpu", fused=False, kv_fp8=True)
    with pytest.raises(ValueError, match="paged=True"):
        LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, device="cpu", fused=False, ragged=True, kv_fp8="emulate")
    with pytest.raises(ValueError, match="fp8=True"):
        _decoder(kv_fp8="emulate")
    with pytest.raises(ValueError, match="graph"):
        LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, graph=True, paged=True, pages=PAGES, page=PAGE,
                     kv_fp8="emulate")
    with pytest.raises(ValueError, match="kv_fp8"):
        _decoder(kv_fp8="yes")
    assert _decoder().kv_fp8 is False


def test_kv8_wrappers_check_the_four_tensors_before_the_library():
    P, Hkv, page = 3, 2, 64
    k8 = torch.zeros(P, Hkv, page, 128).to(torch.float8_e4m3fn)
    sc = torch.ones(P, Hkv, page)
    table = torch.zeros(2, 4, dtype=torch.int32)
    q, pos = torch.zeros(2, 8, 128, dtype=BF), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        llm.decode_attn_paged_kv8(q, k8.to(BF), k8, sc, sc, table, pos)
    with pytest.raises(ValueError, match="kscale"):
        llm.decode_attn_paged_kv8(q, k8, k8, sc[:, :, :32], sc, table, pos)
    with pytest.raises(ValueError, match="vscale"):
        llm.prefill_attn_paged_kv8(q.unsqueeze(1), k8, k8, sc, sc.double(), table, pos, pos)
    with pytest.raises(ValueError, match="CUDA"):  # every check passed on the host: the device is asked for last
        llm.decode_attn_paged_kv8(q, k8, k8, sc, sc, table, pos)

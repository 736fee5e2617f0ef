"""The MXFP4 weight format, its quantiser and the fixtures of the fp4 linear tests
(pbs_amd.ops.llm, tests/mxfp4_cases.py) on the CPU, and the decoder's w4 flag."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_cases as MC  # noqa: E402

from pbs_amd.models.llama import PRESETS, Block, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

BF = torch.bfloat16


def _nibbles(codes):
    return torch.stack([codes & 0xF, codes >> 4], -1).view(codes.shape[0], -1)


def _all_codes_rows(N=16, K=512, seed=0):
    """Rows of e2m1 values times block scales 2^((n + block) % 9 - 4) with a 4 or a 6 in
    every block: amax names the block's scale, so the quantiser must return the codes."""
    g = torch.Generator().manual_seed(40 + seed)
    nib = torch.randint(0, 16, (N, K), generator=g)
    blk = nib.view(N, K // 32, 32)
    top = torch.randint(6, 8, (N, K // 32), generator=g) | (torch.randint(0, 2, (N, K // 32), generator=g) << 3)
    blk[:, :, 0] = top  # +-4 or +-6
    blk[:, :, 1:17] = torch.arange(16)  # every code in every block
    e = (torch.arange(N)[:, None] + torch.arange(K // 32)[None, :]) % 9 - 4
    w = MC.weight64(nib, e)
    wb = w.to(BF)
    assert torch.equal(wb.double(), w)
    return wb, nib, e


def test_all_16_codes_round_trip_through_the_quantiser():
    w, nib, e = _all_codes_rows()
    codes, scales = llm.mxfp4_quant_ref(w)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    assert torch.equal(scales.long(), e + 127)
    assert torch.equal(_nibbles(codes).long(), nib)


def _block(vals):
    """One block of 32 (zeros after vals, and a +4 anchor at the end: E = 0) in a [16, 256] weight."""
    w = torch.zeros(16, 256, dtype=torch.float64)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float64)
    w[0, 31] = 4.0
    wb = w.to(BF)
    assert torch.equal(wb.double(), w)
    codes, scales = llm.mxfp4_quant_ref(wb)
    return _nibbles(codes)[0, :len(vals)].tolist(), int(scales[0, 0])


def test_ties_go_to_the_even_code():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]  # 0, 1, 1, 2, 2, 4, 4
    got, byte = _block(ties + [-t for t in ties])
    assert byte == 127
    assert got == want + [c | 8 for c in want]
    # a bf16 step off the tie goes to the nearer value
    up = [(torch.tensor(t, dtype=BF).view(torch.int16) + 1).view(BF).item() for t in ties]
    dn = [(torch.tensor(t, dtype=BF).view(torch.int16) - 1).view(BF).item() for t in ties]
    assert _block(up)[0] == [1, 2, 3, 4, 5, 6, 7] and _block(dn)[0] == [0, 1, 2, 3, 4, 5, 6]


def test_values_between_5_and_8_become_6():
    vals = [5.03125, 5.5, 6.0, 6.5, 7.0, 7.5, 7.96875]
    w = torch.zeros(16, 256, dtype=torch.float64)
    w[0, :7] = torch.tensor(vals, dtype=torch.float64)
    w[0, 7:14] = -w[0, :7]
    w[1, :7] = w[0, :7] * 2.0 ** -9  # the same in another binade
    wb = w.to(BF)
    assert torch.equal(wb.double(), w)
    codes, scales = llm.mxfp4_quant_ref(wb)
    assert _nibbles(codes)[0, :14].tolist() == [7] * 7 + [15] * 7 and int(scales[0, 0]) == 127
    assert _nibbles(codes)[1, :7].tolist() == [7] * 7 and int(scales[1, 0]) == 127 - 9


def test_an_all_zero_block_gives_byte_127():
    w = torch.zeros(16, 256, dtype=BF)
    w[0, 32:64] = -0.0
    w[0, 64] = 3.0  # floor(log2 3) - 2 = -1
    codes, scales = llm.mxfp4_quant_ref(w)
    assert scales[0].tolist() == [127, 127, 126] + [127] * 5
    assert not (codes[0, :16] != 0).any() and bool((codes[0, 16:32] == 0x88).all())  # -0 keeps its sign
    assert _nibbles(codes)[0, 64].item() == 7  # 3 * 2 = 6


def test_quantiser_is_bit_equal_on_the_rows_of_a_second_call_and_on_its_own_output():
    """The rows of a call do not depend on the other rows, and (not needed by
    anything, stated in mxfp4_quant_ref) requantising the dequantised weight
    gives the same codes and scales."""
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(32, 512, generator=g) * 0.02).to(BF)
    c, s = llm.mxfp4_quant_ref(w)
    c2, s2 = llm.mxfp4_quant_ref(w[16:])
    assert torch.equal(c2, c[16:]) and torch.equal(s2, s[16:])
    d = llm.Mxfp4Weight.from_quantised(c, s).dequant()
    assert torch.equal(d.to(BF).float(), d)
    c3, s3 = llm.mxfp4_quant_ref(d.to(BF))
    assert torch.equal(c3, c) and torch.equal(s3, s)


def test_pack_shuffle_and_the_row_major_views_are_the_identity():
    g = torch.Generator().manual_seed(4)
    codes = torch.randint(0, 256, (48, 384), generator=g).to(torch.uint8)
    scales = torch.randint(0, 255, (48, 24), generator=g).to(torch.uint8)
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    assert (W.N, W.K) == (48, 768)
    assert torch.equal(W.codes, codes) and torch.equal(W.scales, scales)
    assert W.qs.shape == codes.shape and W.ss.shape == scales.shape and not torch.equal(W.qs, codes)
    assert W.nbytes() == 48 * (768 // 2 + 768 // 32)
    w = (torch.randn(32, 512, generator=g) * 0.02).to(BF)
    c, s = llm.mxfp4_quant_ref(w)
    Wq = llm.Mxfp4Weight(w)
    assert torch.equal(Wq.codes, c) and torch.equal(Wq.scales, s)


def test_shuffled_offsets_agree_with_the_stored_bytes():
    g = torch.Generator().manual_seed(5)
    N, K = 32, 768
    codes = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
    scales = torch.randint(0, 255, (N, K // 32), generator=g).to(torch.uint8)
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    qs, ss = W.qs.flatten(), W.ss.flatten()
    seen = set()
    for n in range(N):
        for k in range(K):
            o = llm.mxfp4_shuffled_offset(n, k - k % 32, K) + (k % 32) // 2
            assert (int(qs[o]) >> (4 * (k % 2))) & 0xF == (int(codes[n, k // 2]) >> (4 * (k % 2))) & 0xF
            so = llm.mxfp4_scale_offset(n, k, K)
            assert int(ss[so]) == int(scales[n, k // 32])
            seen.add((o, so))
    assert len({o for o, _ in seen}) == N * K // 2 and len({s for _, s in seen}) == N * K // 32
    # the kernel's reads: lane l = 16 g + r of (strip, block, step u) reads 16 bytes at ... + 1024 u + 16 l,
    # and the 2-byte scale word at ... + 2 l
    for strip, kb, u, lane in ((0, 0, 0, 0), (1, 2, 1, 37), (1, 1, 0, 63)):
        r, gq = lane & 15, lane >> 4
        n, k = 16 * strip + r, 256 * kb + 128 * u + 32 * gq
        assert llm.mxfp4_shuffled_offset(n, k, K) == (strip * (K // 256) + kb) * 2048 + 1024 * u + 16 * lane
        assert llm.mxfp4_scale_offset(n, k, K) == (strip * (K // 256) + kb) * 128 + 2 * lane + u
    with pytest.raises(ValueError):
        llm.mxfp4_shuffled_offset(0, 16, K)
    with pytest.raises(ValueError):
        llm.mxfp4_scale_offset(0, K, K)


def test_from_quantised_rejects_wrong_data():
    codes, scales = torch.zeros(16, 128, dtype=torch.uint8), torch.full((16, 8), 127, dtype=torch.uint8)
    llm.Mxfp4Weight.from_quantised(codes, scales)
    with pytest.raises(ValueError, match="codes must be uint8"):
        llm.Mxfp4Weight.from_quantised(codes.to(torch.int8), scales)
    with pytest.raises(ValueError, match="scales must be uint8"):
        llm.Mxfp4Weight.from_quantised(codes, scales.float())
    with pytest.raises(ValueError, match="scales must be uint8"):
        llm.Mxfp4Weight.from_quantised(codes, scales[:, :7])
    with pytest.raises(ValueError, match="N % 16 == 0 and K % 256 == 0"):
        llm.Mxfp4Weight.from_quantised(codes[:8], scales[:8])
    with pytest.raises(ValueError, match="N % 16 == 0 and K % 256 == 0"):
        llm.Mxfp4Weight.from_quantised(codes[:, :64], scales[:, :4])
    bad = scales.clone()
    bad[3, 5] = 0xFF
    with pytest.raises(ValueError, match="0xFF"):
        llm.Mxfp4Weight.from_quantised(codes, bad)
    with pytest.raises(ValueError, match="N % 16 == 0 and K % 256 == 0"):
        llm.Mxfp4Weight(torch.zeros(16, 128))


def test_dequant_is_exact():
    g = torch.Generator().manual_seed(6)
    N, K = 16, 512
    nib = torch.randint(0, 16, (N, K), generator=g)
    e = torch.randint(-127, 125, (N, K // 32), generator=g)  # 6 * 2^124 is a finite fp32, 0.5 * 2^-127 a subnormal
    e[0, 0], e[0, 1] = -127, 124
    W = llm.Mxfp4Weight.from_quantised(MC.pack(nib), (e + 127).to(torch.uint8))
    d = W.dequant()
    assert d.dtype == torch.float32 and d.shape == (N, K)
    assert torch.equal(d.double(), MC.weight64(nib, e))
    xq = torch.randint(-8, 9, (3, K), generator=g).float().to(MC.F8)
    sx = torch.tensor([0.5, 1.0, 3.0])
    ref = llm.mxfp4_linear_ref(xq, sx, W)
    assert ref.dtype == torch.float64 and torch.equal(ref, xq.double() @ MC.weight64(nib, e).t() * sx.double()[:, None])


@pytest.mark.parametrize("nkb", [1, 9, 25])
def test_fixtures_are_exact(nkb):
    """What the GPU tests take for granted: the integer case's expected output is
    one rounding of an exact fp32 value, the one-hot phases visit every k once,
    its columns spell k, and the scale case names its byte."""
    K = 256 * nkb
    xq, sx, codes, scales, acc = MC.int_case(MC.LIN_M, MC.LIN_N, K)
    W = llm.Mxfp4Weight.from_quantised(codes, scales)
    assert torch.equal(llm.mxfp4_linear_ref(xq, sx, W), acc * sx.double()[:, None])
    assert set(_nibbles(codes).flatten().tolist()) == set(range(16))
    assert acc.abs().max().item() <= 192 * K and torch.equal(acc * 8, (acc * 8).round())
    MC.int_expect(acc, sx)
    MC.int_expect(acc, sx, MC.int_resid(MC.LIN_M, MC.LIN_N))
    ks = torch.cat([MC.one_hot_k(nkb, p) for p in range(MC.one_hot_phases(nkb))])
    assert sorted(ks.tolist()) == list(range(K))
    xq, k, expect = MC.one_hot_case(nkb, 1)
    assert torch.equal(MC.one_hot_decode(expect[:, :7]), k)
    assert torch.equal(expect[:, 7].double(), -(k % 4).double())
    assert torch.equal(MC.one_hot_decode(expect[:, 8:15]), k + 5)
    oc, os_, ow = MC.one_hot_weight(nkb)
    assert torch.equal(llm.Mxfp4Weight.from_quantised(oc, os_).dequant().double(), ow)
    xq, k, expect, e = MC.scale_case(nkb, 1)
    sc, ss, _ = MC.scale_weight(nkb)
    ref = llm.mxfp4_linear_ref(xq, torch.ones(MC.LIN_M), llm.Mxfp4Weight.from_quantised(sc, ss))
    assert torch.equal(ref, expect.double()) and torch.equal(expect.double().log2().long(), e)
    assert e.min().item() >= -15 and e.max().item() <= 15


def test_real_case_bound_holds_for_an_fp32_sum_on_the_cpu():
    xq, sx, W, ref, bound = MC.real_case(5, MC.REAL_N, 2304)
    y = ((xq.float() @ W.dequant().t()) * sx[:, None]).to(BF)
    assert bool(((y.double() - ref).abs() <= bound).all())
    assert bool((bound > 0).all())


# ------------------------------------------------------------------ the decoder's flag
def test_decoder_refuses_w4_without_fp8_with_tiled_prefill_and_bad_values():
    cfg = PRESETS["tiny"]
    with pytest.raises(ValueError, match="needs fp8=True"):
        LlamaDecoder(cfg, batch=1, context=32, device="cpu", w4=True)
    with pytest.raises(ValueError, match="needs fp8=True"):
        LlamaDecoder(cfg, batch=1, context=32, device="cpu", w4="emulate")
    with pytest.raises(ValueError, match="no tiled fp4 GEMM"):
        LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=True, prefill_tiled=True)
    for bad in (1, "yes", None, "fp4"):
        with pytest.raises(ValueError, match="must be False, True or 'emulate'"):
            LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=bad)


def test_w4_decoders_attach_mxfp4_blocks_and_an_fp8_head_on_the_cpu():
    cfg = PRESETS["tiny"]
    d = LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4=True)
    e = LlamaDecoder(cfg, batch=1, context=32, device="cpu", fp8=True, w4="emulate")
    assert isinstance(d.model._fp8_head, llm.Fp8Weight) and isinstance(e.model._fp8_head, llm.Fp8Weight)
    for ld, le in zip(d.model.layers, e.model.layers):
        assert sorted(ld._fp8) == ["o", "qkv", "w13", "w2"]
        for name, w in ld._fp8.items():
            assert isinstance(w, llm.Mxfp4Weight) and isinstance(le._fp8[name], llm.Fp8Weight)
            assert torch.equal(le._fp8[name].q.float() * le._fp8[name].s[:, None], w.dequant())
    with pytest.raises(ValueError, match="no tiled fp4 GEMM"):
        llm.linear_q(None, None, d.model.layers[0]._fp8["o"], tiled=True)


def test_emulate_raises_on_a_row_spanning_more_than_15_binades():
    blk = Block(PRESETS["tiny"]).to(BF)
    with torch.no_grad():
        for p in blk.parameters():
            p.fill_(0.25)
        blk.wo.weight[3, 32:64] = 0.25 * 2.0 ** -14  # 15 binades: fits
        blk.attach_mxfp4(emulate=True)
        assert isinstance(blk._fp8["o"], llm.Fp8Weight)
        blk.wo.weight[3, 64:96] = 0.25 * 2.0 ** -15  # 16: does not
        with pytest.raises(ValueError, match="row 3 span 16 binades"):
            blk.attach_mxfp4(emulate=True)
        blk.wo.weight[3, 64:96] = 0.0  # a block of zeros has no exponent to keep
        blk.attach_mxfp4(emulate=True)

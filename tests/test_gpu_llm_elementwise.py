"""The elementwise Llama kernels of every decode step on the MI355X
(csrc/hip/llm_kernels.hip: rmsnorm, swiglu, rope, rope_dpos;
csrc/hip/decode_kernels.hip: qkv_rope_cache) against fp64 references computed
from the bf16 inputs, at the sizes where they take another path: rows shorter
than the workgroup, ragged passes, and tensors large enough that the
grid-stride loops stride (more than 2048 blocks x 256 threads = 524 288
sixteen-byte chunks)."""
import pytest
import torch

from pbs_amd.models.llama import LlamaConfig, rope_tables
from pbs_amd.ops import llm

pytestmark = pytest.mark.gpu

GRID_CHUNKS = 2048 * 256  # the grid cap of all four kernels, in 16-byte chunks
EPS = 1e-5


def _within(out: torch.Tensor, ref: torch.Tensor, in_max: float, what: str):
    """|out - ref| <= 2^-8 |ref| + 2^-20 max|input|: the rounding of the result to
    bf16 (8 significant bits: half an ulp is at most 2^-8 of the value, reached
    just above a power of two) plus fp32 cancellation in a cos - b sin.  The
    first term leaves the fp32 arithmetic no room just above a power of two,
    the second a few hundred fp32 ulps, so the largest errors sit close to the
    bound: they are the rounding itself."""
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape, what
    out = out.cpu().double()
    assert torch.isfinite(out).all(), f"{what}: {(~torch.isfinite(out)).sum().item()} non-finite outputs"
    err, bound = (out - ref).abs(), 2.0 ** -8 * ref.abs() + 2.0 ** -20 * in_max
    worst = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3g}, {worst:.3g} of the bound")
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside the bound, first {bad[:4].tolist()}"


def _rope64(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """fp64 rotation of interleaved pairs: x [..., hd], cos / sin broadcastable to [..., hd / 2]."""
    xd = x.double().unflatten(-1, (-1, 2))
    a, b, c, s = xd[..., 0], xd[..., 1], cos.double(), sin.double()
    return torch.stack((a * c - b * s, a * s + b * c), dim=-1).flatten(-2)


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("dim", [8, 512, 2048, 2056, 4096, 4104, 8192])
def test_rmsnorm(dim, rows):
    """dim / 8 chunks against 256 threads: 1 chunk, fewer chunks than threads,
    exactly 256, 257, two full passes, a ragged third one, four passes."""
    g = torch.Generator().manual_seed(dim + rows)
    x = torch.randn(rows, dim, generator=g).bfloat16()
    if rows > 1:
        x[rows // 2] = 0  # the statistics of this row are 0: eps alone keeps rsqrt finite
    w = (1 + 0.1 * torch.randn(dim, generator=g)).bfloat16()
    xd = x.double()
    ref = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + EPS) * w.double()
    out = llm.rmsnorm(x.cuda(), w.cuda(), EPS)
    _within(out, ref, x.float().abs().max().item(), f"rmsnorm {rows} x {dim}")
    if rows > 1:
        assert (out[rows // 2].cpu().float() == 0).all()


@pytest.mark.parametrize("shape", [(8, 14336), (8 * (GRID_CHUNKS + 300),)])
def test_swiglu(shape):
    """The FFN width of Llama-3-8B, and one tensor 300 chunks longer than the
    grid.  Planted gates of +-80 and +-20: silu is the identity or a clean 0
    there, and exp(80) must not turn into a NaN."""
    g = torch.Generator().manual_seed(len(shape))
    a = torch.randn(*shape, generator=g).bfloat16()
    b = torch.randn(*shape, generator=g).bfloat16()
    planted = torch.tensor([80.0, -80.0, 20.0, -20.0]).bfloat16()
    n = a.numel()
    af = a.view(-1)
    for k, at in enumerate((0, 9, n // 2 + 3, 8 * GRID_CHUNKS - 1, n - 1)):  # both halves of a 32-bit pair, both ends
        if at < n:
            af[at] = planted[k % 4]
    af[n - 8:n - 4] = planted
    ad = a.double()
    ref = ad / (1 + torch.exp(-ad)) * b.double()
    out = llm.swiglu(a.cuda(), b.cuda())
    _within(out, ref, max(a.float().abs().max().item(), b.float().abs().max().item()), f"swiglu {shape}")


ROPE = [(2, 3, 32, 8192, 0, 7), (2, 3, 32, 8192, 100, 8189), (2, 1100, 16, 2048, 0, 948)]


@pytest.mark.parametrize("B,S,H,max_seq,pos,other", ROPE)
def test_rope_and_rope_dpos(B, S, H, max_seq, pos, other):
    """(2, 1100, 16) is 563 200 chunks: the grid strides.  rope_dpos at the same
    device position gives the bits of rope; refilled in place, as between the
    replays of a captured graph, it rotates by the new position."""
    assert pos + S <= max_seq and other + S <= max_seq
    cos, sin = rope_tables(LlamaConfig(dim=H * 128, n_heads=H, max_seq=max_seq), "cpu")
    x = torch.randn(B, S, H, 128, generator=torch.Generator().manual_seed(S + pos)).bfloat16()
    in_max = x.float().abs().max().item()
    xd, cd, sd = x.cuda(), cos.cuda(), sin.cuda()

    def ref(p):
        return _rope64(x, cos[p:p + S, None, :], sin[p:p + S, None, :])

    out = llm.rope(xd, cd, sd, pos)
    _within(out, ref(pos), in_max, f"rope {(B, S, H)} pos {pos}")
    pos_t = torch.tensor([pos], dtype=torch.int32, device="cuda")
    assert torch.equal(llm.rope_dpos(xd, cd, sd, pos_t).view(torch.int16), out.view(torch.int16))
    pos_t.fill_(other)
    _within(llm.rope_dpos(xd, cd, sd, pos_t), ref(other), in_max, f"rope_dpos {(B, S, H)} pos {other}")


@pytest.mark.parametrize("B,H,Hkv,C,pos", [(3, 8, 2, 200, 0), (3, 8, 2, 200, 199), (2100, 14, 1, 3, 1)])
def test_qkv_rope_cache(B, H, Hkv, C, pos):
    """(2100, 14, 1, 3) is 537 600 chunks: the grid strides.  q and the new K row
    are rotated, V is copied bit for bit, every other cache row keeps its bits."""
    hd = 128
    g = torch.Generator().manual_seed(B + pos)
    cos, sin = rope_tables(LlamaConfig(dim=H * hd, n_heads=H, max_seq=C), "cpu")
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * hd, generator=g).bfloat16()
    kc0 = torch.randn(B, Hkv, C, hd, generator=g).bfloat16()
    vc0 = torch.randn(B, Hkv, C, hd, generator=g).bfloat16()
    kc, vc = kc0.cuda(), vc0.cuda()
    pos_t = torch.tensor([pos], dtype=torch.int32, device="cuda")
    q = llm.qkv_rope_cache(qkv.cuda(), cos.cuda(), sin.cuda(), pos_t, kc, vc, H)
    in_max = qkv.float().abs().max().item()
    _within(q, _rope64(qkv[:, 0, :H * hd].view(B, H, hd), cos[pos], sin[pos]), in_max, f"q {(B, H, Hkv, C)} pos {pos}")
    _within(kc[:, :, pos], _rope64(qkv[:, 0, H * hd:(H + Hkv) * hd].view(B, Hkv, hd), cos[pos], sin[pos]), in_max,
            f"k row {(B, H, Hkv, C)} pos {pos}")
    kc, vc = kc.cpu(), vc.cpu()
    assert torch.equal(vc[:, :, pos].view(torch.int16), qkv[:, 0, (H + Hkv) * hd:].view(B, Hkv, hd).view(torch.int16))
    others = torch.ones(C, dtype=torch.bool)
    others[pos] = False
    assert others.sum() == C - 1
    for new, old in ((kc, kc0), (vc, vc0)):
        assert torch.equal(new[:, :, others].view(torch.int16), old[:, :, others].view(torch.int16))

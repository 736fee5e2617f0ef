"""The fp8-cache (_kv8) forms of the four paged attention-block kernels on the
MI355X (csrc/hip/decode_kernels.hip, csrc/hip/prefill_kernels.hip,
csrc/hip/kv8_codec.hpp) on the fp8 fixtures of tests/kv8_cases.py.

Dequantisation is exact, so no tolerance appears anywhere: an attention kernel
over the fp8 pools must give, bit for bit, the output of the bf16 _paged kernel
over the dequantised twin pools (and, on the one-hot fixtures, the dequantised V
row), and a write kernel the codes and scales of llm.kv8_quant_ref on the rows
the bf16 write kernel stored.  The out-of-range table entries come last in the
file: they run only after everything else here has passed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import kv8_cases as K8  # noqa: E402
import paged_cases as PG  # noqa: E402
import prefill_cases as PC  # noqa: E402
import weighted_cases as WC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, rope_tables  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu

HD = DC.HD
F8 = torch.float8_e4m3fn
DECODE = [(s, H, Hkv, page) for s in range(len(PG.DECODE_SETS)) for (H, Hkv) in DC.HEADS for page in PG.PAGES]
PREFILL = [(s, H, Hkv, page) for s in range(len(PG.PREFILL_SETS)) for (H, Hkv) in PC.HEADS for page in PG.PAGES] \
    + [(1, H, Hkv, 256) for (H, Hkv) in PC.HEADS]  # page 256 on one set
DECODE_256 = [(kind, s, H, Hkv) for kind in WC.DECODE_KINDS for s in range(len(WC.DECODE_SETS))
              for (H, Hkv) in DC.HEADS if kind != "exact" or s == 0]  # one-hot at 256 on one set, weighted on all
WEIGHTED = [(kind, pairs, H, Hkv, page) for kind in ("census", "ramp") for pairs in WC.RAGGED
            for (H, Hkv) in WC.HEADS for page in WC.PAGES]
FAILED = []  # tests of this file that failed, seen by the out-of-range cases


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _guard(name):
    """Run the body of a test and note a failure for the last cases of the file."""
    def deco(fn):
        def run(*a, **k):
            try:
                return fn(*a, **k)
            except BaseException:
                FAILED.append(name)
                raise
        run.__name__ = fn.__name__
        run.__doc__ = fn.__doc__
        return run
    return deco


def _four(c):
    return _cuda(c["kpool8"], c["vpool8"], c["kscale"], c["vscale"])


# ------------------------------------------------------------------ decode attention
def _check_decode(c, H, active, expect8=None, shift=0):
    """Every nsplit: active rows have the bits of decode_attn_paged on the twin
    pools (and of expect8, where the fixture has one), idle rows are zero bits."""
    positions = c["positions"]
    qd, table, kt, vt = _cuda(c["q"], c["table"], c["ktwin"], c["vtwin"])
    k8, v8, ks, vs = _four(c)
    pos_t = _i32(positions)
    for ns in DC.NSPLITS:
        out = llm.decode_attn_paged_kv8(qd, k8, v8, ks, vs, table, pos_t, ns)
        ref = llm.decode_attn_paged(qd, kt, vt, table, pos_t, ns)
        assert out.shape == (DC.B, H * HD) and out.dtype == torch.bfloat16
        for b, p in enumerate(positions):
            if not active(p):
                assert not _bits(out[b]).any(), f"nsplit={ns}: idle sequence {b} (pos {p}) is not zero bits"
                continue
            assert _same_bits(out[b], ref[b]), f"nsplit={ns}: sequence {b} at pos {p} differs from decode_attn_paged"
            assert _bits(out[b]).any() and not torch.isnan(out[b].float()).any()
            if expect8 is None:
                continue
            row, want = out[b].cpu().view(H, HD), expect8[b].view(H, HD)
            if shift and p + 1 < DC.C:  # heads aimed at the first masked key must not get its V row
                hidden = c["t"][b] == p + 1
                same = (_bits(row) == _bits(want)).all(-1)
                assert hidden[0] or b, "the fixture aims head 0 of sequence 0 at the first masked key"
                assert not (same & hidden).any(), f"nsplit={ns}: sequence {b} sees key {p + 1}"
                assert same[~hidden].all()
            else:
                bad = (_bits(row) != _bits(want)).any(-1).nonzero().flatten().tolist()
                assert not bad, f"nsplit={ns}: sequence {b} at pos {p}: wrong heads {bad}"


@pytest.mark.parametrize("s,H,Hkv,page", DECODE)
def test_decode_over_fp8_pools_has_the_bits_of_the_bf16_kernel_over_the_twin(s, H, Hkv, page):
    @_guard("decode")
    def body():
        c = K8.decode_case(s, H, Hkv, page)
        _check_decode(c, H, PG.decode_active, c["expect8"])
    body()


@pytest.mark.parametrize("s,H,Hkv,page", DECODE)
def test_decode_first_masked_key_is_not_seen_over_fp8_pools(s, H, Hkv, page):
    @_guard("decode shift")
    def body():
        c = K8.decode_case(s, H, Hkv, page, 1)
        _check_decode(c, H, PG.decode_active, c["expect8"], shift=1)
    body()


@pytest.mark.parametrize("kind,s,H,Hkv", DECODE_256)
def test_decode_over_fp8_pages_of_256_and_weighted_softmax(kind, s, H, Hkv):
    """Census and ramp data: softmax weights that are not 0 or 1, which the
    one-hot cases cannot see go wrong."""
    @_guard("decode 256")
    def body():
        c = K8.decode_case_256(kind, s, H, Hkv)
        _check_decode(c, H, WC.decode_active, c.get("expect8"))
    body()


# ------------------------------------------------------------------ prefill attention
def _check_prefill(c, H, expect8=None):
    qd, table, kt, vt = _cuda(c["q"], c["table"], c["ktwin"], c["vtwin"])
    k8, v8, ks, vs = _four(c)
    pos_t, len_t = _i32(c["pos"]), _i32(c["lens"])
    out = llm.prefill_attn_paged_kv8(qd, k8, v8, ks, vs, table, pos_t, len_t)
    ref = llm.prefill_attn_paged(qd, kt, vt, table, pos_t, len_t)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    for b, n in enumerate(c["lens"]):
        assert not _bits(out[b, n:]).any(), f"sequence {b}: rows >= {n} are not zero bits"
        assert _same_bits(out[b, :n], ref[b, :n]), f"sequence {b} differs from prefill_attn_paged"
        assert n == 0 or (_bits(out[b, :n]).any() and not torch.isnan(out[b, :n].float()).any())
    if expect8 is not None:
        bad = (_bits(out.cpu()) != _bits(expect8)).view(out.shape[0], -1, H, HD).any(-1).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} wrong (b, s, h) rows, first {bad[:8].tolist()}"


@pytest.mark.parametrize("s,H,Hkv,page", PREFILL)
def test_prefill_over_fp8_pools_has_the_bits_of_the_bf16_kernel_over_the_twin(s, H, Hkv, page):
    @_guard("prefill")
    def body():
        c = K8.prefill_case(s, H, Hkv, page)
        _check_prefill(c, H, c["expect8"])
    body()


@pytest.mark.parametrize("kind,pairs,H,Hkv,page", WEIGHTED)
def test_prefill_weighted_softmax_over_fp8_pools(kind, pairs, H, Hkv, page):
    @_guard("prefill weighted")
    def body():
        _check_prefill(K8.weighted_case(kind, pairs, H, Hkv, page), H)
    body()


# ------------------------------------------------------------------ the two write kernels
def _tables(H, Hkv, C):
    return _cuda(*rope_tables(LlamaConfig(dim=H * HD, n_heads=H, n_kv_heads=Hkv, max_seq=C), "cpu"))


def _poisoned_bf16(P, Hkv, page):
    return torch.full((P, Hkv, page, HD), float("nan"), dtype=torch.bfloat16, device="cuda")


def _poisoned_kv8(P, Hkv, page):
    code = lambda: torch.full((P, Hkv, page, HD), K8.NAN_CODE, dtype=torch.uint8, device="cuda").view(F8)  # noqa: E731
    scale = lambda: torch.full((P, Hkv, page), float("nan"), device="cuda")  # noqa: E731
    return code(), code(), scale(), scale()


def _qkv(B, S, H, Hkv, seed):
    """Random rows scaled by 2^k, k in -20 .. 20 per (token, head): [B, S, H + 2 Hkv, 128] bf16."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-20, 21, (B, S, H + 2 * Hkv, 1), generator=g).float()
    return (torch.randn(B, S, H + 2 * Hkv, HD, generator=g) * 2.0 ** k).bfloat16()


def _check_written(pools, four, written_mask):
    """Codes (as uint8) and scales (as int32) are kv8_quant_ref of the rows the
    bf16 kernel wrote; every other byte keeps its poison."""
    W = written_mask
    keep = W[:, None, :, None]
    for i, name in enumerate(("k", "v")):
        rows = pools[i].cpu()
        assert torch.isfinite(rows[keep.expand_as(rows)]).all() and torch.isnan(rows[~keep.expand_as(rows)]).all()
        codes, scale = llm.kv8_quant_ref(torch.where(keep, rows, torch.zeros_like(rows)))
        codes, scale = K8.poison(codes, scale, W)
        got_c, got_s = four[i].cpu().view(torch.uint8), four[2 + i].cpu().view(torch.int32)
        bad = (got_c != codes.view(torch.uint8)).any(-1).nonzero()
        assert bad.numel() == 0, f"{name} codes: {bad.shape[0]} wrong (page, head, row), first {bad[:6].tolist()}"
        bad = (got_s != scale.view(torch.int32)).nonzero()
        assert bad.numel() == 0, f"{name} scales: {bad.shape[0]} wrong (page, head, row), first {bad[:6].tolist()}"


def _run_decode_write(positions, active, H, Hkv, page, NP, qkv, seed):
    B = len(positions)
    rows = [p + 1 if active(p) else 0 for p in positions]
    ids, P = PG.assign_pages([-(-r // page) for r in rows], seed)
    table = PG.make_table(ids, NP).cuda()
    kp, vp = _poisoned_bf16(P, Hkv, page), _poisoned_bf16(P, Hkv, page)
    four = _poisoned_kv8(P, Hkv, page)
    cos, sin = _tables(H, Hkv, NP * page)
    x = qkv.reshape(B, 1, -1).cuda()
    pos_t = _i32(positions)
    q = llm.qkv_rope_cache_paged(x, cos, sin, pos_t, table, kp, vp, H)
    q8 = llm.qkv_rope_cache_paged_kv8(x, cos, sin, pos_t, table, *four, H)
    assert q8.shape == (B, H, HD) and _same_bits(q8, q)
    W = torch.zeros(P, page, dtype=torch.bool)
    for b, p in enumerate(positions):
        if active(p):
            W[ids[b][p // page], p % page] = True
    assert W.sum() == sum(map(active, positions))
    _check_written((kp, vp), four, W)


@pytest.mark.parametrize("page", WC.PAGES)
@pytest.mark.parametrize("s", range(len(PG.DECODE_SETS)))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_paged_kv8(s, H, Hkv, page):
    """Set 0 has a sequence at position 0, where RoPE is the identity: its k and v
    rows carry edge rows of the codec (a multiple of 448, of 450, of 224; with
    s + H they walk the list)."""
    @_guard("rope decode")
    def body():
        positions = (WC.DECODE_SETS if page == 256 else PG.DECODE_SETS)[s]
        active = WC.decode_active if page == 256 else PG.decode_active
        qkv = _qkv(DC.B, 1, H, Hkv, seed=s + H + page)
        edge, _ = K8.edge_rows()
        for b, p in enumerate(positions):
            if p == 0:
                for j in range(2 * Hkv):
                    qkv[b, 0, H + j] = edge[(3 * (s + H + page // 64) + j) % len(edge)]
        _run_decode_write(positions, active, H, Hkv, page, PG.n_table(DC.C, page), qkv, seed=sum(positions) + H + page)
    body()


def _run_prefill_write(pos, lens, n_want, S, H, Hkv, page, NP, qkv, seed):
    B = len(pos)
    Cl = NP * page
    assert [llm.seq_tokens(p, ln, S, Cl) for p, ln in zip(pos, lens)] == n_want
    rows = [p + n if n else 0 for p, n in zip(pos, n_want)]
    ids, P = PG.assign_pages([-(-r // page) for r in rows], seed)
    table = PG.make_table(ids, NP).cuda()
    kp, vp = _poisoned_bf16(P, Hkv, page), _poisoned_bf16(P, Hkv, page)
    four = _poisoned_kv8(P, Hkv, page)
    cos, sin = _tables(H, Hkv, Cl)
    x = qkv.reshape(B, S, -1).cuda()
    pos_t, len_t = _i32(pos), _i32(lens)
    q = llm.qkv_rope_cache_prefill_paged(x, cos, sin, pos_t, len_t, table, kp, vp, H)
    q8 = llm.qkv_rope_cache_prefill_paged_kv8(x, cos, sin, pos_t, len_t, table, *four, H)
    assert q8.shape == (B, S, H, HD) and _same_bits(q8, q)
    W = torch.zeros(P, page, dtype=torch.bool)
    for b, (p, n) in enumerate(zip(pos, n_want)):
        for r in range(p, p + n):
            W[ids[b][r // page], r % page] = True
    assert W.sum() == sum(n_want)
    _check_written((kp, vp), four, W)


def _with_edge_rows(qkv, pos, lens, H, Hkv):
    """Every v row of a sequence that starts at position 0 is an edge row (they
    walk the whole list), and so is the k row of its token 0 (no rotation there)."""
    edge, _ = K8.edge_rows()
    for b, (p, n) in enumerate(zip(pos, lens)):
        if p == 0:
            for s in range(min(n, qkv.shape[1])):
                for kvh in range(Hkv):
                    qkv[b, s, H + Hkv + kvh] = edge[(s * Hkv + kvh + b) % len(edge)]
            for kvh in range(Hkv):
                qkv[b, 0, H + kvh] = edge[(7 * b + kvh + H) % len(edge)]
    return qkv


@pytest.mark.parametrize("page", WC.PAGES)
@pytest.mark.parametrize("s", range(len(PG.PREFILL_SETS)))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_prefill_paged_kv8(s, H, Hkv, page):
    @_guard("rope prefill")
    def body():
        pairs = PG.PREFILL_SETS[s]
        S = max(0 if p is None else p[0] for p in pairs)
        pos = [-1 if p is None else p[1] for p in pairs]
        lens = [0 if p is None else p[0] for p in pairs]
        qkv = _with_edge_rows(_qkv(PC.B, S, H, Hkv, seed=S + H + page), pos, lens, H, Hkv)
        _run_prefill_write(pos, lens, lens, S, H, Hkv, page, PG.n_table(PC.C, page), qkv, seed=S + H + page)
    body()


@pytest.mark.parametrize("page", WC.PAGES)
def test_the_kv8_write_kernel_clamps_lengths_to_the_launch_and_to_the_logical_context(page):
    @_guard("clamps")
    def body():
        H, Hkv, S, NP = 8, 2, 64, PG.n_table(PC.C, page)
        Cl = NP * page
        for pos, lens, n in (([Cl - 10, 0], [64, 1000], [10, 64]), ([Cl, 17], [5, -3], [0, 0])):
            qkv = _with_edge_rows(_qkv(PC.B, S, H, Hkv, seed=7 + page), pos, n, H, Hkv)
            _run_prefill_write(pos, lens, n, S, H, Hkv, page, NP, qkv, seed=7 + page)
    body()


def test_every_edge_row_of_the_codec_through_both_write_kernels_at_position_0():
    """As many sequences as edge rows / Hkv, all at position 0 (cos = 1, sin = 0:
    the k row is stored as it came): the kernels' integer exponent rule meets a
    multiple of 448, of 450 and of 224 at every scale of K8.EDGE_K, the zero row
    and the clamp at 2^-100, in k and in v."""
    @_guard("edge rows")
    def body():
        H, Hkv, page = 4, 2, 64
        edge, _ = K8.edge_rows()
        B = len(edge) // Hkv
        assert B * Hkv == len(edge)
        qkv = _qkv(B, 1, H, Hkv, seed=3)
        qkv[:, 0, H:H + Hkv] = edge.view(B, Hkv, HD)
        qkv[:, 0, H + Hkv:] = edge.flip(0).view(B, Hkv, HD)
        _run_decode_write([0] * B, PG.decode_active, H, Hkv, page, 2, qkv, seed=5)
        _run_prefill_write([0] * B, [1] * B, [1] * B, 1, H, Hkv, page, 2, qkv, seed=6)
    body()


def test_dequantisation_at_every_scale_of_the_edge_rows():
    """One key per sequence and q = 0: the only softmax weight is exactly 1, so
    both attention kernels return the dequantised V row of the edge rows, whose
    scales run from 2^-100 to 2^101: the bits of the bf16 kernel over the twin
    pools and the values of llm.kv8_dequant (a -0 comes back as +0 from 0 + -0)."""
    @_guard("edge dequant")
    def body():
        H, Hkv, page = 4, 2, 64
        edge, _ = K8.edge_rows()
        B = len(edge) // Hkv
        codes, scale = llm.kv8_quant_ref(edge.view(B, Hkv, HD))
        v8 = torch.zeros(B, Hkv, page, HD, dtype=torch.uint8)
        v8[:, :, 0] = codes.view(torch.uint8)
        vs = torch.ones(B, Hkv, page)
        vs[:, :, 0] = scale
        k8, ks = torch.zeros_like(v8), torch.ones_like(vs)
        k8, v8, ks, vs = _cuda(k8.view(F8), v8.view(F8), ks, vs)
        kt, vt = llm.kv8_dequant(k8, ks), llm.kv8_dequant(v8, vs)
        table = torch.arange(B, dtype=torch.int32, device="cuda").view(B, 1)
        pos, one = _i32([0] * B), _i32([1] * B)
        want = llm.kv8_dequant(codes, scale).repeat_interleave(H // Hkv, dim=1).reshape(B, H * HD).float().cuda()
        assert torch.isfinite(want).all() and want.abs().max() > 2.0 ** 100 and 0 < want.abs()[want != 0].min() < 2.0 ** -80
        q = torch.zeros(B, H, HD, dtype=torch.bfloat16, device="cuda")
        out = llm.decode_attn_paged_kv8(q, k8, v8, ks, vs, table, pos, 1)
        assert _same_bits(out, llm.decode_attn_paged(q, kt, vt, table, pos, 1)) and torch.equal(out.float(), want)
        qp = q.view(B, 1, H, HD)
        out = llm.prefill_attn_paged_kv8(qp, k8, v8, ks, vs, table, pos, one)
        assert _same_bits(out, llm.prefill_attn_paged(qp, kt, vt, table, pos, one))
        assert torch.equal(out.view(B, H * HD).float(), want)
    body()


# ------------------------------------------------------------------ shared pages, refusals
def _random_kv8(P, Hkv, page, seed):
    """Random fp8 pools (rows scaled by 2^k) and their twins, on the GPU."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        k = torch.randint(-6, 7, (P, Hkv, page, 1), generator=g).float()
        codes, scale = llm.kv8_quant_ref((torch.randn(P, Hkv, page, HD, generator=g) * 2.0 ** k).bfloat16())
        out.append((codes.cuda(), scale.cuda(), llm.kv8_dequant(codes, scale).cuda()))
    (k8, ks, kt), (v8, vs, vt) = out
    return (k8, v8, ks, vs), (kt, vt)


@pytest.mark.parametrize("page", PG.PAGES)
def test_sequences_that_share_their_first_pages_over_fp8_pools(page):
    """Sequences 0 and 1 map the same two first pages, scales included."""
    @_guard("shared")
    def body():
        H, Hkv, B, NP = 8, 2, 2, 5
        four, (kt, vt) = _random_kv8(9, Hkv, page, seed=11 + page)
        table = PG.make_table([[6, 2, 7, 0], [6, 2, 3]], NP).cuda()
        pos = [3 * page + 17, 2 * page + 5]
        g = torch.Generator().manual_seed(page)
        q = torch.randn(B, H, HD, generator=g).bfloat16().cuda()
        for ns in (None, 1, 3):
            assert _same_bits(llm.decode_attn_paged_kv8(q, *four, table, _i32(pos), ns),
                              llm.decode_attn_paged(q, kt, vt, table, _i32(pos), ns))
        S = 40
        qp = torch.randn(B, S, H, HD, generator=g).bfloat16().cuda()
        start, lens = [p + 1 - S for p in pos], [S, S - 9]
        out = llm.prefill_attn_paged_kv8(qp, *four, table, _i32(start), _i32(lens))
        assert _same_bits(out, llm.prefill_attn_paged(qp, kt, vt, table, _i32(start), _i32(lens)))
        assert _bits(out[1]).any()
    body()


def test_library_refuses_what_the_kv8_kernels_cannot_do():
    @_guard("refusals")
    def body():
        from pbs_amd.ops.kernels import _ptr, _stream, lib
        L, B, S, NP, P, page = lib(), 2, 4, 3, 5, 64
        bf = dict(dtype=torch.bfloat16, device="cuda")
        q, out = torch.zeros(B, S, 8, HD, **bf), torch.zeros(B, S, 8 * HD, **bf)
        k8, v8, ks, vs = (t.zero_() for t in _poisoned_kv8(P, 2, page))
        ws = torch.zeros(B * 2 * 2 * 4 * (HD + 2), device="cuda")
        v, f = _i32([0] * B), torch.zeros(NP * page, HD // 2, device="cuda")
        tab = torch.zeros(B, NP, dtype=torch.int32, device="cuda")
        sc, st = 0.1, _stream()
        ok = dict(table=tab, ks=ks, vs=vs, H=8, NP=NP, P=P, page=page, hd=HD)

        def pf(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_prefill_attn_paged_kv8(_ptr(q), _ptr(k8), _ptr(v8), _ptr(a["ks"]), _ptr(a["vs"]),
                                                     _ptr(v), _ptr(v), _ptr(a["table"]), _ptr(out), B, S, a["H"], 2,
                                                     a["NP"], a["P"], a["page"], a["hd"], sc, st)

        def dec(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_decode_attn_paged_kv8(_ptr(q), _ptr(k8), _ptr(v8), _ptr(a["ks"]), _ptr(a["vs"]),
                                                    _ptr(v), _ptr(a["table"]), _ptr(out), _ptr(ws), 2, B, a["H"], 2,
                                                    a["NP"], a["P"], a["page"], a["hd"], sc, st)

        def rope(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_qkv_rope_cache_paged_kv8(_ptr(q), _ptr(f), _ptr(f), _ptr(v), _ptr(a["table"]),
                                                       _ptr(out), _ptr(k8), _ptr(v8), _ptr(a["ks"]), _ptr(a["vs"]),
                                                       B, a["H"], 2, a["NP"], a["P"], a["page"], a["hd"], st)

        def rope_pf(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_qkv_rope_cache_prefill_paged_kv8(_ptr(q), _ptr(f), _ptr(f), _ptr(v), _ptr(v),
                                                               _ptr(a["table"]), _ptr(out), _ptr(k8), _ptr(v8),
                                                               _ptr(a["ks"]), _ptr(a["vs"]), B, 1, a["H"], 2, a["NP"],
                                                               a["P"], a["page"], a["hd"], st)

        bad = [dict(table=None), dict(ks=None), dict(vs=None), dict(page=32), dict(page=96), dict(NP=0), dict(P=0),
               dict(hd=64)]
        for fn in (pf, dec, rope, rope_pf):
            for k in bad:
                assert fn(**k) == -22, (fn.__name__, k)
        for fn in (pf, dec):
            assert fn(H=6) == -22 and fn(H=32) == -22  # group size 3, 16
        for fn in (pf, dec, rope, rope_pf):  # the same calls with nothing wrong are accepted
            assert fn() == 0, fn.__name__
        torch.cuda.synchronize()
    body()


# ------------------------------------------------------------------ out-of-range table entries (last)
GUARD = 1 << 16  # bytes of 0xff on either side of every cache tensor


def _guarded(t: torch.Tensor):
    """A copy of t in the middle of a larger allocation of 0xff bytes (NaN as a
    code, as a scale and as bf16); returns (the copy, the allocation)."""
    n = t.numel() * t.element_size()
    buf = torch.full((GUARD + n + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + n] = t.contiguous().view(-1).view(torch.uint8)
    return buf[GUARD:GUARD + n].view(t.dtype).view(t.shape), buf


def _guards_intact(bufs):
    return all(bool((b[:GUARD] == 0xFF).all()) and bool((b[-GUARD:] == 0xFF).all()) for b in bufs)


def _spoil(table, b, value):
    t = table.clone()
    t[b, 0] = value
    return t


@pytest.mark.parametrize("value", ["P + 3", "-7", "2 ** 30"])
def test_an_out_of_range_entry_spoils_its_own_sequence_alone_over_fp8_pools(value):
    """Sequence 1's first used entry is P + 3, -7, 2^30: its reads come from page
    0 (its rows are those of the same call with the entry set to 0) and its
    writes, codes and scales, are dropped; sequences 0, 2 and 3 keep their bits,
    and so do the 64 KiB of 0xff on either side of each of the four tensors.  Not
    run unless the rest of the file has passed: the clamp is the only thing
    between such an entry and an address outside the tensors."""
    if FAILED:
        pytest.fail(f"not run: earlier tests of this file failed ({sorted(set(FAILED))})")
    H, Hkv, page, B = 8, 2, 64, DC.B
    entry = lambda P: {"P + 3": P + 3, "-7": -7, "2 ** 30": 2 ** 30}[value]  # noqa: E731
    # decode attention, every nsplit
    c = K8.decode_case(0, H, Hkv, page)  # positions 0, 63, 512, 1099: all active
    qd, table = _cuda(c["q"], c["table"])
    four, bufs = zip(*(_guarded(t) for t in _four(c)))
    spoiled, zeroed = _spoil(table, 1, entry(c["P"])), _spoil(table, 1, 0)
    pos_t = _i32(c["positions"])
    for ns in DC.NSPLITS:
        good = llm.decode_attn_paged_kv8(qd, *four, table, pos_t, ns)
        out = llm.decode_attn_paged_kv8(qd, *four, spoiled, pos_t, ns)
        page0 = llm.decode_attn_paged_kv8(qd, *four, zeroed, pos_t, ns)
        for b in (0, 2, 3):
            assert _same_bits(out[b], good[b]), f"decode nsplit={ns}: sequence {b} changed"
        assert _same_bits(out[1], page0[1]), f"decode nsplit={ns}: sequence 1 does not read page 0"
    assert _guards_intact(bufs)
    # prefill attention
    NP = PG.n_table(PC.C, page)
    pos, lens = [64, 5, 130, 0], [65, 63, 129, 7]
    rows = [p + n for p, n in zip(pos, lens)]
    ids, P = PG.assign_pages([-(-r // page) for r in rows], 33)
    table = PG.make_table(ids, NP).cuda()
    plain, _ = _random_kv8(P, Hkv, page, seed=33)
    four, bufs = zip(*(_guarded(t) for t in plain))
    spoiled, zeroed = _spoil(table, 1, entry(P)), _spoil(table, 1, 0)
    S = max(lens)
    g = torch.Generator().manual_seed(21)
    q = torch.randn(B, S, H, HD, generator=g).bfloat16().cuda()
    good = llm.prefill_attn_paged_kv8(q, *four, table, _i32(pos), _i32(lens))
    out = llm.prefill_attn_paged_kv8(q, *four, spoiled, _i32(pos), _i32(lens))
    page0 = llm.prefill_attn_paged_kv8(q, *four, zeroed, _i32(pos), _i32(lens))
    for b in (0, 2, 3):
        assert _same_bits(out[b], good[b]), f"prefill: sequence {b} changed"
    assert _same_bits(out[1], page0[1]) and _guards_intact(bufs)
    # the write kernels: sequence 1 writes into its first page only (5 + 58 rows, position 20)
    cos, sin = _tables(H, Hkv, NP * page)
    qkv = _qkv(B, S, H, Hkv, seed=9).reshape(B, S, -1).cuda()
    own = ids[1][0]
    rest = torch.arange(P, device="cuda") != own

    def as_bytes(ts):
        return [t.view(torch.uint8) if t.dtype == F8 else t.view(torch.int32) for t in ts]

    for launch in ("prefill", "decode"):
        a, abufs = zip(*(_guarded(t) for t in plain))
        s_, sbufs = zip(*(_guarded(t) for t in plain))
        if launch == "prefill":
            lens1 = [65, 58, 129, 7]
            q1 = llm.qkv_rope_cache_prefill_paged_kv8(qkv, cos, sin, _i32(pos), _i32(lens1), table, *a, H)
            q2 = llm.qkv_rope_cache_prefill_paged_kv8(qkv, cos, sin, _i32(pos), _i32(lens1), spoiled, *s_, H)
        else:
            dpos = [64, 20, 130, 0]
            q1 = llm.qkv_rope_cache_paged_kv8(qkv[:, :1].contiguous(), cos, sin, _i32(dpos), table, *a, H)
            q2 = llm.qkv_rope_cache_paged_kv8(qkv[:, :1].contiguous(), cos, sin, _i32(dpos), spoiled, *s_, H)
        assert _same_bits(q1, q2)
        for t1, t2, t0 in zip(as_bytes(a), as_bytes(s_), as_bytes(plain)):
            assert not torch.equal(t1[own], t0[own]), f"{launch}: the unspoiled call wrote nothing"
            assert torch.equal(t2[own], t0[own]), f"{launch}: a write through the entry was not dropped"
            assert torch.equal(t2[rest], t1[rest]) and torch.equal(t2[0], t1[0] if own else t0[0])  # page 0 included
        assert _guards_intact(abufs) and _guards_intact(sbufs), launch
    torch.cuda.synchronize()

"""The paged (_paged) forms of the four attention-block kernels on the MI355X
(csrc/hip/decode_kernels.hip, csrc/hip/prefill_kernels.hip): the ragged
exact-data fixtures scattered into shuffled, poisoned pools
(tests/paged_cases.py), and the _seq kernels on the gathered dense caches as
the reference, bit for bit.  The out-of-range table entries come last in the
file: they run only after everything else here has passed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import paged_cases as PG  # noqa: E402
import prefill_cases as PC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, rope_tables  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu

HD = DC.HD
DECODE = [(s, H, Hkv, page) for s in range(len(PG.DECODE_SETS)) for (H, Hkv) in DC.HEADS for page in PG.PAGES]
PREFILL = [(s, H, Hkv, page) for s in range(len(PG.PREFILL_SETS)) for (H, Hkv) in PC.HEADS for page in PG.PAGES]
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


# ------------------------------------------------------------------ decode
def _check_decode(s, H, Hkv, page, shift):
    c = PG.decode_case(s, H, Hkv, page, shift)
    positions, t, expect = c["positions"], c["t"], c["expect"]
    qd, kp, vp, table = _cuda(c["q"], c["kpool"], c["vpool"], c["table"])
    kd = PG.gather_dense(kp, c["ids"], c["rows"], c["Cl"])
    vd = PG.gather_dense(vp, c["ids"], c["rows"], c["Cl"])
    pos_t = _i32(positions)
    for ns in DC.NSPLITS:
        out = llm.decode_attn_paged(qd, kp, vp, table, pos_t, ns)
        ref = llm.decode_attn_seq(qd, kd, vd, pos_t, ns)
        assert out.shape == (DC.B, H * HD) and out.dtype == torch.bfloat16
        for b, p in enumerate(positions):
            if not PG.decode_active(p):
                assert not _bits(out[b]).any(), f"nsplit={ns}: idle sequence {b} (pos {p}) is not zero bits"
                continue
            assert _same_bits(out[b], ref[b]), f"nsplit={ns}: sequence {b} at pos {p} differs from decode_attn_seq"
            row, want = out[b].cpu().view(H, HD), expect[b].view(H, HD)
            if shift and p + 1 < DC.C:  # heads aimed at the first masked key must not get its V row
                hidden = t[b] == p + 1
                same = (_bits(row) == _bits(want)).all(-1)
                assert hidden[0] or b, "the fixture aims head 0 of sequence 0 at the first masked key"
                assert not (same & hidden).any(), f"nsplit={ns}: sequence {b} sees key {p + 1}"
                assert same[~hidden].all()
            else:
                bad = (_bits(row) != _bits(want)).any(-1).nonzero().flatten().tolist()
                assert not bad, f"nsplit={ns}: sequence {b} at pos {p}: wrong heads {bad}, targets {t[b, bad].tolist()}"


@pytest.mark.parametrize("s,H,Hkv,page", DECODE)
def test_decode_exact_data_through_the_table_bit_for_bit(s, H, Hkv, page):
    """Active rows: the bits of decode_attn_seq on the gathered dense cache of Cl
    rows with the same nsplit, and the fixture's V row; idle rows (NaN q, a table
    row of garbage) zero bits."""
    _guard("decode")(_check_decode)(s, H, Hkv, page, 0)


@pytest.mark.parametrize("s,H,Hkv,page", DECODE)
def test_decode_first_masked_key_is_not_seen_through_the_table(s, H, Hkv, page):
    _guard("decode shift")(_check_decode)(s, H, Hkv, page, 1)


# ------------------------------------------------------------------ prefill
@pytest.mark.parametrize("s,H,Hkv,page", PREFILL)
def test_prefill_exact_data_through_the_table_bit_for_bit(s, H, Hkv, page):
    @_guard("prefill")
    def body():
        c = PG.prefill_case(s, H, Hkv, page)
        qd, kp, vp, table = _cuda(c["q"], c["kpool"], c["vpool"], c["table"])
        kd = PG.gather_dense(kp, c["ids"], c["rows"], c["Cl"])
        vd = PG.gather_dense(vp, c["ids"], c["rows"], c["Cl"])
        pos_t, len_t = _i32(c["pos"]), _i32(c["lens"])
        out = llm.prefill_attn_paged(qd, kp, vp, table, pos_t, len_t)
        ref = llm.prefill_attn_seq(qd, kd, vd, pos_t, len_t)
        assert out.shape == c["expect"].shape and out.dtype == torch.bfloat16
        for b, n in enumerate(c["lens"]):
            assert not _bits(out[b, n:]).any(), f"sequence {b}: rows >= {n} are not zero bits"
            assert _same_bits(out[b, :n], ref[b, :n]), f"sequence {b} differs from prefill_attn_seq"
        assert _same_bits(out.cpu(), c["expect"])
    body()


@pytest.mark.parametrize("s,H,Hkv,page", PREFILL)
def test_prefill_rows_past_each_sequence_in_every_page_do_not_reach_the_output(s, H, Hkv, page):
    """Every pool row that is not one of a sequence's rows 0 .. pos + n - 1 (the
    rest of its last page, every unreferenced page) refilled with NaN, +-inf and
    finite garbage: not a bit changes."""
    @_guard("prefill stale")
    def body():
        c = PG.prefill_case(s, H, Hkv, page)
        qd, kp, vp, table = _cuda(c["q"], c["kpool"], c["vpool"], c["table"])
        pos_t, len_t = _i32(c["pos"]), _i32(c["lens"])
        first = llm.prefill_attn_paged(qd, kp, vp, table, pos_t, len_t)
        live = torch.zeros(c["P"], page, dtype=torch.bool)
        for ids, r in zip(c["ids"], c["rows"]):
            for i, pg in enumerate(ids):
                live[pg, :min(page, r - i * page)] = True
        dead = (~live).cuda()[:, None, :, None].expand_as(kp)
        g = torch.Generator().manual_seed(3)
        for fill in (float("nan"), float("inf"), float("-inf"), None):
            for pool in (kp, vp):
                junk = (torch.randn(pool.shape, generator=g) * 100).bfloat16().cuda() if fill is None \
                    else torch.full_like(pool, fill)
                pool.copy_(torch.where(dead, junk, pool))
            assert _same_bits(first, llm.prefill_attn_paged(qd, kp, vp, table, pos_t, len_t)), f"fill {fill}"
    body()


# ------------------------------------------------------------------ the two rope-cache kernels
def _tables(H, Hkv, C):
    return _cuda(*rope_tables(LlamaConfig(dim=H * HD, n_heads=H, n_kv_heads=Hkv, max_seq=C), "cpu"))


def _random_paged(B, Hkv, rows, page, NP, seed):
    """Random pools with a shuffled assignment of ceil(rows[b] / page) pages per
    sequence, and the dense caches of NP * page rows that hold the same rows."""
    g = torch.Generator().manual_seed(seed)
    ids, P = PG.assign_pages([-(-r // page) for r in rows], seed)
    kp = torch.randn(P, Hkv, page, HD, generator=g).bfloat16().cuda()
    vp = torch.randn(P, Hkv, page, HD, generator=g).bfloat16().cuda()
    full = [len(i) * page for i in ids]  # whole pages, so that every row of a sequence's pages is compared
    kd, vd = PG.gather_dense(kp, ids, full, NP * page), PG.gather_dense(vp, ids, full, NP * page)
    return kp, vp, PG.make_table(ids, NP).cuda(), ids, torch.nan_to_num(kd), torch.nan_to_num(vd)


def _check_pools(kp, vp, kp0, vp0, ids, kd, vd, page, written):
    """The pages of every sequence hold the dense caches' rows (which the _seq
    kernel wrote); every pool row outside written[b] keeps its bits."""
    keep = torch.ones(kp.shape[0], page, dtype=torch.bool)
    for b, i in enumerate(ids):
        for j, pg in enumerate(i):
            assert _same_bits(kp[pg], kd[b, :, j * page:(j + 1) * page]), f"sequence {b}, page {j}: k rows"
            assert _same_bits(vp[pg], vd[b, :, j * page:(j + 1) * page]), f"sequence {b}, page {j}: v rows"
        for r in written[b]:
            keep[i[r // page], r % page] = False
    keep = keep.cuda()
    assert _same_bits(kp.transpose(1, 2)[keep], kp0.transpose(1, 2)[keep])
    assert _same_bits(vp.transpose(1, 2)[keep], vp0.transpose(1, 2)[keep])
    for b, rows in enumerate(written):
        for r in rows:
            assert not _same_bits(kp[ids[b][r // page], :, r % page], kp0[ids[b][r // page], :, r % page])


@pytest.mark.parametrize("page", PG.PAGES)
@pytest.mark.parametrize("s", range(len(PG.DECODE_SETS)))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_paged(s, H, Hkv, page):
    @_guard("rope decode")
    def body():
        positions, B = PG.DECODE_SETS[s], DC.B
        NP = PG.n_table(DC.C, page)
        rows = [p + 1 if PG.decode_active(p) else 0 for p in positions]
        kp, vp, table, ids, kd, vd = _random_paged(B, Hkv, rows, page, NP, seed=sum(positions) + H + page)
        kp0, vp0 = kp.clone(), vp.clone()
        cos, sin = _tables(H, Hkv, NP * page)
        g = torch.Generator().manual_seed(s)
        qkv = torch.randn(B, 1, (H + 2 * Hkv) * HD, generator=g).bfloat16().cuda()
        pos_t = _i32(positions)
        q = llm.qkv_rope_cache_paged(qkv, cos, sin, pos_t, table, kp, vp, H)
        qs = llm.qkv_rope_cache_seq(qkv, cos, sin, pos_t, kd, vd, H)
        assert q.shape == (B, H, HD) and _same_bits(q, qs)
        for b, p in enumerate(positions):
            if not PG.decode_active(p):
                assert not _bits(q[b]).any()
        _check_pools(kp, vp, kp0, vp0, ids, kd, vd, page, [[p] if PG.decode_active(p) else [] for p in positions])
    body()


def _check_rope_prefill(S, H, Hkv, page, pos, lens, n_want, seed):
    B, NP = PC.B, PG.n_table(PC.C, page)
    Cl = NP * page
    rows = [p + n if n else 0 for p, n in zip(pos, n_want)]
    kp, vp, table, ids, kd, vd = _random_paged(B, Hkv, rows, page, NP, seed)
    kp0, vp0 = kp.clone(), vp.clone()
    cos, sin = _tables(H, Hkv, Cl)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * HD, generator=g).bfloat16().cuda()
    pos_t, len_t = _i32(pos), _i32(lens)
    assert [llm.seq_tokens(p, ln, S, Cl) for p, ln in zip(pos, lens)] == n_want
    q = llm.qkv_rope_cache_prefill_paged(qkv, cos, sin, pos_t, len_t, table, kp, vp, H)
    qs = llm.qkv_rope_cache_prefill_seq(qkv, cos, sin, pos_t, len_t, kd, vd, H)
    assert q.shape == (B, S, H, HD) and _same_bits(q, qs)
    for b, n in enumerate(n_want):
        assert not _bits(q[b, n:]).any()
    _check_pools(kp, vp, kp0, vp0, ids, kd, vd, page, [list(range(p, p + n)) for p, n in zip(pos, n_want)])
    return q, kp, vp, table, kd, vd


@pytest.mark.parametrize("page", PG.PAGES)
@pytest.mark.parametrize("s", range(len(PG.PREFILL_SETS)))
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_prefill_paged(s, H, Hkv, page):
    @_guard("rope prefill")
    def body():
        pairs = PG.PREFILL_SETS[s]
        S = max(0 if p is None else p[0] for p in pairs)
        pos = [-1 if p is None else p[1] for p in pairs]
        lens = [0 if p is None else p[0] for p in pairs]
        _check_rope_prefill(S, H, Hkv, page, pos, lens, lens, seed=S + H + page)
    body()


@pytest.mark.parametrize("page", PG.PAGES)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (2, 2)])
def test_the_paged_kernels_clamp_lengths_to_the_launch_and_to_the_logical_context(H, Hkv, page):
    """len > Cl - pos (10 rows left) and len > S: the kernels clamp n_b themselves
    with Cl = NP * page for C, and pos >= Cl or len <= 0 is an idle sequence."""
    @_guard("clamps")
    def body():
        S, Cl = 64, PG.n_table(PC.C, page) * page
        for pos, lens, n in (([Cl - 10, 0], [64, 1000], [10, 64]), ([Cl, 17], [5, -3], [0, 0])):
            q, kp, vp, table, kd, vd = _check_rope_prefill(S, H, Hkv, page, pos, lens, n, seed=7 + page)
            pos_t, len_t = _i32(pos), _i32(lens)
            out = llm.prefill_attn_paged(q, kp, vp, table, pos_t, len_t)
            ref = llm.prefill_attn_seq(q, kd, vd, pos_t, len_t)
            for b in range(PC.B):
                assert not _bits(out[b, n[b]:]).any() and _same_bits(out[b], ref[b])
                assert n[b] == 0 or _bits(out[b, :n[b]]).any()
    body()


# ------------------------------------------------------------------ shared pages, a table refilled in place
@pytest.mark.parametrize("page", PG.PAGES)
def test_sequences_that_share_their_first_pages(page):
    """Sequences 0 and 1 map the same two first pages: both kernels give the bits
    of two dense sequences that each hold a copy of those rows."""
    @_guard("shared")
    def body():
        H, Hkv, B = 8, 2, 2
        NP = 5
        g = torch.Generator().manual_seed(11 + page)
        kp = torch.randn(9, Hkv, page, HD, generator=g).bfloat16().cuda()
        vp = torch.randn(9, Hkv, page, HD, generator=g).bfloat16().cuda()
        ids = [[6, 2, 7, 0], [6, 2, 3]]
        table = PG.make_table(ids, NP).cuda()
        full = [len(i) * page for i in ids]
        kd, vd = PG.gather_dense(kp, ids, full, NP * page), PG.gather_dense(vp, ids, full, NP * page)
        pos = [3 * page + 17, 2 * page + 5]
        q = torch.randn(B, H, HD, generator=g).bfloat16().cuda()
        for ns in (None, 1, 3):
            assert _same_bits(llm.decode_attn_paged(q, kp, vp, table, _i32(pos), ns),
                              llm.decode_attn_seq(q, kd, vd, _i32(pos), ns))
        S = 40
        qp = torch.randn(B, S, H, HD, generator=g).bfloat16().cuda()
        start, lens = [p + 1 - S for p in pos], [S, S - 9]
        out = llm.prefill_attn_paged(qp, kp, vp, table, _i32(start), _i32(lens))
        assert _same_bits(out, llm.prefill_attn_seq(qp, kd, vd, _i32(start), _i32(lens))) and _bits(out[1]).any()
    body()


@pytest.mark.parametrize("page", PG.PAGES)
def test_table_and_positions_refilled_in_place(page):
    """One table tensor and one position tensor refilled long, short, long (what
    the graph-captured step does before a replay): the first and third results
    are equal bits, each the _seq kernel's on the gathered cache."""
    @_guard("refill")
    def body():
        H, Hkv, B, NP = 8, 2, DC.B, PG.n_table(DC.C, page)
        long_, short = [1099, 1023, 1024, 575], [0, 5, -1, 63]
        g = torch.Generator().manual_seed(page)
        q = torch.randn(B, H, HD, generator=g).bfloat16().cuda()
        sets = []
        for vals, seed in ((long_, 1), (short, 2)):
            ids, P = PG.assign_pages([-(-(p + 1) // page) if p >= 0 else 0 for p in vals], seed, spare=0)
            sets.append((vals, ids, PG.make_table(ids, NP)))
        P = max(sum(len(i) for i in ids) for _, ids, _ in sets)
        kp = torch.randn(P, Hkv, page, HD, generator=g).bfloat16().cuda()
        vp = torch.randn(P, Hkv, page, HD, generator=g).bfloat16().cuda()
        table, pos_t = torch.zeros(B, NP, dtype=torch.int32, device="cuda"), _i32(long_)
        for ns in (None, 1, 3):
            outs = []
            for vals, ids, tab in (sets[0], sets[1], sets[0]):
                table.copy_(tab)
                pos_t.copy_(_i32(vals))
                outs.append(llm.decode_attn_paged(q, kp, vp, table, pos_t, ns))
                full = [len(i) * page for i in ids]
                kd, vd = PG.gather_dense(kp, ids, full, NP * page), PG.gather_dense(vp, ids, full, NP * page)
                assert _same_bits(outs[-1], llm.decode_attn_seq(q, kd, vd, pos_t, ns)), (ns, vals)
            assert _same_bits(outs[0], outs[2]) and not _same_bits(outs[0], outs[1])
    body()


# ------------------------------------------------------------------ refusals
def test_library_refuses_what_the_paged_kernels_cannot_do():
    @_guard("refusals")
    def body():
        from pbs_amd.ops.kernels import _ptr, _stream, lib
        L, B, S, NP, P, page = lib(), 2, 4, 3, 5, 64
        bf = dict(dtype=torch.bfloat16, device="cuda")
        q, kp, vp = torch.zeros(B, S, 8, HD, **bf), torch.zeros(P, 2, page, HD, **bf), torch.zeros(P, 2, page, HD, **bf)
        out, ws = torch.zeros(B, S, 8 * HD, **bf), torch.zeros(B * 2 * 2 * 4 * (HD + 2), device="cuda")
        v, f = _i32([0] * B), torch.zeros(NP * page, HD // 2, device="cuda")
        tab = torch.zeros(B, NP, dtype=torch.int32, device="cuda")
        sc, st = 0.1, _stream()
        ok = dict(table=tab, H=8, NP=NP, P=P, page=page, hd=HD)

        def pf(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_prefill_attn_paged(_ptr(q), _ptr(kp), _ptr(vp), _ptr(v), _ptr(v), _ptr(a["table"]),
                                                 _ptr(out), B, S, a["H"], 2, a["NP"], a["P"], a["page"], a["hd"], sc,
                                                 st)

        def dec(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_decode_attn_paged(_ptr(q), _ptr(kp), _ptr(vp), _ptr(v), _ptr(a["table"]), _ptr(out),
                                                _ptr(ws), 2, B, a["H"], 2, a["NP"], a["P"], a["page"], a["hd"], sc, st)

        def rope(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_qkv_rope_cache_paged(_ptr(q), _ptr(f), _ptr(f), _ptr(v), _ptr(a["table"]), _ptr(out),
                                                   _ptr(kp), _ptr(vp), B, a["H"], 2, a["NP"], a["P"], a["page"],
                                                   a["hd"], st)

        def rope_pf(**k):
            a = dict(ok, **k)
            return L.gpbs_hip_qkv_rope_cache_prefill_paged(_ptr(q), _ptr(f), _ptr(f), _ptr(v), _ptr(v),
                                                           _ptr(a["table"]), _ptr(out), _ptr(kp), _ptr(vp), B, 1,
                                                           a["H"], 2, a["NP"], a["P"], a["page"], a["hd"], st)

        bad = [dict(table=None), dict(page=32), dict(page=96), dict(NP=0), dict(P=0), dict(hd=64)]
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
def _spoil(table, b, value):
    t = table.clone()
    t[b, 0] = value
    return t


@pytest.mark.parametrize("value", ["P + 3", "-7"])
def test_an_out_of_range_entry_spoils_its_own_sequence_alone(value):
    """Sequence 1's first used entry is P + 3, then -7: its reads come from page 0
    and its writes are dropped, so sequences 0, 2 and 3 keep their bits in both
    attention kernels, and in both rope-cache kernels every pool row, page 0
    included, keeps its bits.  Not run unless the rest of the file has passed:
    the clamp is the only thing between such an entry and an address outside
    the pools."""
    if FAILED:
        pytest.fail(f"not run: earlier tests of this file failed ({sorted(set(FAILED))})")
    H, Hkv, page, B = 8, 2, 64, DC.B
    # decode attention, every nsplit
    c = PG.decode_case(0, H, Hkv, page)  # positions 0, 63, 512, 1099: all active
    bad_entry = c["P"] + 3 if value == "P + 3" else -7
    qd, kp, vp, table = _cuda(c["q"], c["kpool"], c["vpool"], c["table"])
    # page 0 may be an unreferenced NaN page: whatever sequence 1 then computes is its own affair
    spoiled = _spoil(table, 1, bad_entry)
    pos_t = _i32(c["positions"])
    for ns in DC.NSPLITS:
        good = llm.decode_attn_paged(qd, kp, vp, table, pos_t, ns)
        out = llm.decode_attn_paged(qd, kp, vp, spoiled, pos_t, ns)
        for b in (0, 2, 3):
            assert _same_bits(out[b], good[b]), f"decode nsplit={ns}: sequence {b} changed"
    # prefill attention: a batch of 4 out of two prefill sets' sequences
    NP = PG.n_table(PC.C, page)
    g = torch.Generator().manual_seed(21)
    pos, lens = [64, 5, 130, 0], [65, 63, 129, 7]
    rows = [p + n for p, n in zip(pos, lens)]
    kp, vp, table, ids, kd, vd = _random_paged(B, Hkv, rows, page, NP, seed=33)
    spoiled = _spoil(table, 1, kp.shape[0] + 3 if value == "P + 3" else -7)
    S = max(lens)
    q = torch.randn(B, S, H, HD, generator=g).bfloat16().cuda()
    good = llm.prefill_attn_paged(q, kp, vp, table, _i32(pos), _i32(lens))
    out = llm.prefill_attn_paged(q, kp, vp, spoiled, _i32(pos), _i32(lens))
    for b in (0, 2, 3):
        assert _same_bits(out[b], good[b]), f"prefill: sequence {b} changed"
    # the rope-cache kernels: sequence 1 writes into its first page only (5 + 58 rows, position 20)
    cos, sin = _tables(H, Hkv, NP * page)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * HD, generator=g).bfloat16().cuda()
    lens1 = [65, 58, 129, 7]
    kp1, vp1, kp2, vp2 = kp.clone(), vp.clone(), kp.clone(), vp.clone()
    q1 = llm.qkv_rope_cache_prefill_paged(qkv, cos, sin, _i32(pos), _i32(lens1), table, kp1, vp1, H)
    q2 = llm.qkv_rope_cache_prefill_paged(qkv, cos, sin, _i32(pos), _i32(lens1), spoiled, kp2, vp2, H)
    own = ids[1][0]
    assert _same_bits(q1, q2) and not _same_bits(kp1[own], kp[own])
    assert _same_bits(kp2[own], kp[own]) and _same_bits(vp2[own], vp[own])  # the writes were dropped
    rest = torch.arange(kp.shape[0], device="cuda") != own
    assert _same_bits(kp2[rest], kp1[rest]) and _same_bits(vp2[rest], vp1[rest])  # page 0 included
    assert _same_bits(kp2[0], kp1[0]) and _same_bits(vp2[0], vp1[0])
    dpos = [64, 20, 130, 0]
    kp1, vp1, kp2, vp2 = kp.clone(), vp.clone(), kp.clone(), vp.clone()
    q1 = llm.qkv_rope_cache_paged(qkv[:, :1].contiguous(), cos, sin, _i32(dpos), table, kp1, vp1, H)
    q2 = llm.qkv_rope_cache_paged(qkv[:, :1].contiguous(), cos, sin, _i32(dpos), spoiled, kp2, vp2, H)
    assert _same_bits(q1, q2) and not _same_bits(kp1[own], kp[own])
    assert _same_bits(kp2[own], kp[own]) and _same_bits(vp2[own], vp[own])
    assert _same_bits(kp2[rest], kp1[rest]) and _same_bits(vp2[rest], vp1[rest])
    assert _same_bits(kp2[0], kp1[0]) and _same_bits(vp2[0], vp1[0])
    torch.cuda.synchronize()

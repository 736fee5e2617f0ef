"""Weighted-softmax fixtures of the prefill-attention tests and the page-256
cases (tests/test_weighted_cases_cpu.py, tests/test_gpu_prefill_weighted.py),
all built on the CPU in bf16 and cached: every fixture and fp64 reference is
built once and shared, unchanged, by the uniform, _seq and _paged kernel forms.

The one-hot fixture of prefill_cases makes every softmax weight 0 or 1, so the
online rescale corr = ex2(m - mn) only ever is 0 or 1 there.  Here:

* census_case: q = 0, so every weight is exactly 1 and l = L = pos + s + 1; V
  counts the visible keys per dimension, so one dropped or doubled key moves
  one dimension by at least 25 % (a residue is met at most 4 times in 400 keys).
* ramp_case: random data with a score ramp in dimension 0: the running max of
  the even heads rises by a few nats from one 64-key tile to the next (corr is
  neither 0 nor 1), the odd heads see their max in the first tile.

Cache rows past pos + S - 1 hold NaN: a stale row that leaked with weight
exactly 0 still gives NaN.

WIDE adds the shapes at which k_prefill_attn<1> (256 tokens per workgroup) runs
a second query tile: 1 token, 44 tokens (one full wave and a partial one) and
128 tokens (four full waves) in it; G = 8 gets up to 12 query tiles.
"""
import functools

import torch

import decode_cases as DC
import paged_cases as PG
import prefill_cases as PC
import ragged_cases as RC

B, HD, C, HEADS = PC.B, PC.HD, PC.C, PC.HEADS
BF = torch.bfloat16
NAN = float("nan")

WIDE = [(257, 64), (300, 37), (384, 16)]  # (S, pos), all within C = 400
ALL = PC.SHAPES + WIDE
RAGGED = RC.PREFILL_SETS + [((300, 37), (257, 64)), ((384, 16), None)]
PAGES = (64, 128, 256)
KT = 64  # keys per tile of k_prefill_attn
# The ramp of K dimension 0 climbs SLOPE over the visible keys.  The decode ramp uses 16; on 64-key tiles, with
# 129 .. 400 keys and q[.., 0] from 8 to 14, 16 let the running max of three cases at ~400 keys rise by less than
# 0.5 nats between two full tiles (0.37 at the least), and 19 lifts it past 12 nats at 129 / 138 keys.  18 keeps
# every full-tile rise of every ALL shape within [0.66, 11.61] (tests/test_weighted_cases_cpu.py checks it).
SLOPE = 18.0

# half a bf16 ulp is at most 2^-8 of the value; the fp32 reciprocal and multiply add less than 2^-22 each
CENSUS_REL = 2.0 ** -8 + 2.0 ** -20


# ------------------------------------------------------------------ uniform fixtures
@functools.lru_cache(maxsize=None)
def census_case(S: int, pos: int, H: int, Hkv: int):
    """(q [B, S, H, 128], kc, vc [B, Hkv, C, 128] in bf16, expect [B, S, H * 128] fp64):
    q = 0, K rows 0 .. pos + S - 1 randn, V[b, kvh, j, d] = 256 if
    (j + b + 2 kvh) % 128 == d else 0, every row >= pos + S NaN.
    expect[b, s, h, d] = 256 count / L with L = pos + s + 1 and count the number
    of keys j < L of that residue."""
    rows = pos + S
    assert S >= 1 and pos >= 0 and rows <= C
    g = torch.Generator().manual_seed(5 * S + 3 * pos + H + Hkv)
    q = torch.zeros(B, S, H, HD)
    kc = torch.full((B, Hkv, C, HD), NAN)
    vc = torch.full((B, Hkv, C, HD), NAN)
    kc[:, :, :rows] = torch.randn(B, Hkv, rows, HD, generator=g)
    j, d = torch.arange(rows), torch.arange(HD)
    expect = torch.zeros(B, S, H, HD, dtype=torch.float64)
    G = H // Hkv
    L = (pos + 1 + torch.arange(S)).double().view(S, 1)
    for b in range(B):
        for kvh in range(Hkv):
            hot = ((j[:, None] + b + 2 * kvh) % HD == d[None, :])
            vc[b, kvh, :rows] = hot.float() * 256
            count = hot.double().cumsum(0)[pos:]  # [S, 128]: keys 0 .. pos + s
            expect[b, :, kvh * G:(kvh + 1) * G] = (256 * count / L).unsqueeze(1)
    return q.to(BF), kc.to(BF), vc.to(BF), expect.reshape(B, S, H * HD)


@functools.lru_cache(maxsize=None)
def ramp_case(S: int, pos: int, H: int, Hkv: int, seed: int = 0):
    """(q, kc, vc) in bf16 of random normal data with K[.., j, 0] = SLOPE j / (pos + S)
    and q[b, s, h, 0] = +(8 + h) for even h, -(8 + h) for odd h; rows >= pos + S
    are NaN.  The decode ramp (decode_cases.ramp_case) on 64-key tiles."""
    rows = pos + S
    assert S >= 1 and pos >= 0 and rows <= C
    g = torch.Generator().manual_seed(1000 * seed + 31 * S + 3 * pos + 7 * H + Hkv)
    q = torch.randn(B, S, H, HD, generator=g)
    h = torch.arange(H)
    q[:, :, :, 0] = torch.where(h % 2 == 0, 8.0 + h, -(8.0 + h))
    kc = torch.full((B, Hkv, C, HD), NAN)
    vc = torch.full((B, Hkv, C, HD), NAN)
    kc[:, :, :rows] = torch.randn(B, Hkv, rows, HD, generator=g)
    kc[:, :, :rows, 0] = SLOPE * torch.arange(rows) / rows
    vc[:, :, :rows] = torch.randn(B, Hkv, rows, HD, generator=g)
    return q.to(BF), kc.to(BF), vc.to(BF)


def scores64(q: torch.Tensor, kc: torch.Tensor, pos: int) -> torch.Tensor:
    """fp64 scaled scores in nats, masked keys -inf: [B, Hkv, G, S, pos + S]."""
    Bq, S, H, hd = q.shape
    Hkv, L = kc.shape[1], pos + S
    qg = q.double().view(Bq, S, Hkv, H // Hkv, hd).permute(0, 2, 3, 1, 4)
    sc = qg @ kc[:, :, :L].double().transpose(-1, -2).unsqueeze(2) * hd ** -0.5
    seen = torch.arange(L)[None, :] <= pos + torch.arange(S)[:, None]
    return sc.masked_fill(~seen, float("-inf"))


def ref64(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos: int):
    """fp64 attention of the bf16 inputs with the mask key <= pos + s:
    (ref, A), both [B, S, H * hd]; A = w @ |V|, the weighted mean of |V| behind
    each output element.  Two matmuls per KV head, nothing of size S x L x hd."""
    Bq, S, H, hd = q.shape
    L = pos + S
    w = torch.softmax(scores64(q, kc, pos), -1)  # [B, Hkv, G, S, L]
    v = vc[:, :, :L].double().unsqueeze(2)
    ref, A = w @ v, w @ v.abs()  # [B, Hkv, G, S, hd]
    return tuple(t.permute(0, 3, 1, 2, 4).reshape(Bq, S, H * hd) for t in (ref, A))


def ramp_bound(ref: torch.Tensor, A: torch.Tensor, pos: int, vmax: float) -> torch.Tensor:
    """|out - ref| allowed on the ramp data, per element:
      2^-8 |ref|                   the rounding of the result to bf16;
      2^-8 (A + |ref|)             each P rounded to bf16 (at most 2^-8 relative), on
                                   sum w |v - ref| <= A + |ref| (l is summed from the
                                   same rounded P, so the error is in the deviations);
      2^-11 (A + |ref|)            the fp32 score: a 128-term dot product at
                                   |score| <= 40 is off by at most 3e-4 < 2^-11, hence
                                   that relative error in a weight (the derivation of
                                   tests/test_gpu_decode_attn.py::_bound);
      L 2^-24 max|V|               the fp32 sums over L = pos + s + 1 keys."""
    L = (pos + 1 + torch.arange(ref.shape[1])).double().view(1, -1, 1)
    dev = A + ref.abs()
    return 2.0 ** -8 * ref.abs() + (2.0 ** -8 + 2.0 ** -11) * dev + L * 2.0 ** -24 * vmax


@functools.lru_cache(maxsize=None)
def ramp_ref(S: int, pos: int, H: int, Hkv: int):
    """(ref, bound) of ramp_case(S, pos, H, Hkv), fp64 [B, S, H * 128] each."""
    q, kc, vc = ramp_case(S, pos, H, Hkv)
    ref, A = ref64(q, kc, vc, pos)
    vmax = vc[:, :, :pos + S].float().abs().max().item()
    return ref, ramp_bound(ref, A, pos, vmax)


def outside(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """Elements outside the bound; NaN counts as outside."""
    return ~((out.double() - ref).abs() <= bound)


def fraction(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """The largest |out - ref| / bound over the elements with bound > 0."""
    nz = bound > 0
    if not nz.any():
        return 0.0
    return ((out.double() - ref).abs()[nz] / bound[nz]).max().item()


# ------------------------------------------------------------------ ragged and paged prefill
def _uniform(kind: str, S: int, pos: int, H: int, Hkv: int):
    """(q, kc, vc, expect or None) of one uniform fixture."""
    if kind == "census":
        return census_case(S, pos, H, Hkv)
    assert kind == "ramp"
    return ramp_case(S, pos, H, Hkv) + (None,)


@functools.lru_cache(maxsize=None)
def ragged_case(kind: str, pairs, H: int, Hkv: int):
    """The conventions of ragged_cases.prefill_case on the census / ramp data:
    (q [B, S, H, 128] padded to the longest sequence, kc, vc [B, Hkv, C, 128],
    pos [B], lens [B], expect): sequence b is row b of the uniform fixture of its
    own (S_b, pos_b); padding query rows are NaN; an idle sequence has pos -1,
    len 0, NaN q and caches.  expect (census only, else None) is fp64
    [B, S, H * 128], zero in the rows >= S_b."""
    assert len(pairs) == B
    S = max(RC.prefill_tokens(p) for p in pairs)
    q = torch.full((B, S, H, HD), NAN, dtype=BF)
    kc = torch.full((B, Hkv, C, HD), NAN, dtype=BF)
    vc = torch.full((B, Hkv, C, HD), NAN, dtype=BF)
    expect = torch.zeros(B, S, H * HD, dtype=torch.float64) if kind == "census" else None
    pos, lens = [], []
    for b, pair in enumerate(pairs):
        if pair is None:
            pos.append(-1)
            lens.append(0)
            continue
        n, p = pair
        uq, uk, uv, ue = _uniform(kind, n, p, H, Hkv)
        q[b, :n], kc[b], vc[b] = uq[b], uk[b], uv[b]
        if expect is not None:
            expect[b, :n] = ue[b]
        pos.append(p)
        lens.append(n)
    return q, kc, vc, pos, lens, expect


@functools.lru_cache(maxsize=None)
def paged_case(kind: str, pairs, H: int, Hkv: int, page: int):
    """Paged form of ragged_case (as paged_cases.prefill_case): rows = pos + n of
    each sequence scattered into shuffled, NaN-poisoned pools; Cl = NP * page is
    448 / 512 / 512 for page 64 / 128 / 256."""
    q, kc, vc, pos, lens, expect = ragged_case(kind, pairs, H, Hkv)
    rows = [p + n if n else 0 for p, n in zip(pos, lens)]
    seed = 3000 * RAGGED.index(pairs) + page + (7 if kind == "ramp" else 0)
    kpool, vpool, table, ids = PG.scatter(kc, vc, rows, page, seed=seed)
    return dict(q=q, kpool=kpool, vpool=vpool, table=table, ids=ids, pos=pos, lens=lens, rows=rows, kc=kc, vc=vc,
                expect=expect, P=kpool.shape[0], NP=table.shape[1], Cl=table.shape[1] * page)


# ------------------------------------------------------------------ decode at page 256
DECODE_PAGE = 256
DECODE_CL = PG.n_table(DC.C, DECODE_PAGE) * DECODE_PAGE  # 1280, NP = 5
# RC.DECODE_SETS with the ">= C" idle value moved to the paged rule's ">= Cl"
DECODE_SETS = [[DECODE_CL if p >= DC.C else p for p in s] for s in RC.DECODE_SETS]
DECODE_KINDS = ("exact", "census", "ramp")


def decode_active(pos: int) -> bool:
    return 0 <= pos < DECODE_CL


def decode_bound(ref: torch.Tensor, vmax: float) -> torch.Tensor:
    """The bound of tests/test_gpu_decode_attn.py::_bound on the decode ramp."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -10 * vmax


@functools.lru_cache(maxsize=None)
def _decode_uniform(kind: str, pos: int, H: int, Hkv: int):
    """(q, kc, vc, expect, bound) of one DC fixture at one position: expect is the
    bf16 V row (exact, bound None: bit for bit), 256 count / L in fp64 (census,
    bound CENSUS_REL |expect|: the positions of DECODE_SETS are not those of
    DC.CENSUS_L, for which the decode suite argues a plain 2^-8) or the fp64
    reference (ramp, decode_bound)."""
    if kind == "exact":
        q, kc, vc, _, expect = DC.exact_case(pos, H, Hkv)
        return q, kc, vc, expect, None
    if kind == "census":
        q, kc, vc, expect = DC.census_case(pos + 1, H, Hkv)
        return q, kc, vc, expect, CENSUS_REL * expect.abs()
    assert kind == "ramp"
    q, kc, vc = DC.ramp_case(pos, H, Hkv, seed=0)
    ref = DC.ref64(q, kc, vc, pos)
    return q, kc, vc, ref, decode_bound(ref, vc[:, :, :pos + 1].float().abs().max().item())


@functools.lru_cache(maxsize=None)
def decode_case_256(kind: str, s: int, H: int, Hkv: int):
    """DECODE_SETS[s] over the DC fixtures, scattered into pages of 256 rows:
    sequence b is row b of the DC fixture at its own position; an idle sequence
    has NaN q and caches and a table row of garbage.  expect / bound are lists
    over b (None for idle; bound None for exact)."""
    positions = DECODE_SETS[s]
    q = torch.full((DC.B, H, DC.HD), NAN, dtype=BF)
    kc = torch.full((DC.B, Hkv, DC.C, DC.HD), NAN, dtype=BF)
    vc = torch.full((DC.B, Hkv, DC.C, DC.HD), NAN, dtype=BF)
    expect, bound = [None] * DC.B, [None] * DC.B
    for b, p in enumerate(positions):
        if not decode_active(p):
            continue
        assert p < DC.C  # an active sequence lies within the DC fixtures
        uq, uk, uv, ue, ub = _decode_uniform(kind, p, H, Hkv)
        q[b], kc[b], vc[b], expect[b] = uq[b], uk[b], uv[b], ue[b]
        bound[b] = None if ub is None else ub[b]
    rows = [p + 1 if decode_active(p) else 0 for p in positions]
    seed = 5000 * s + DECODE_PAGE + DECODE_KINDS.index(kind)
    kpool, vpool, table, ids = PG.scatter(kc, vc, rows, DECODE_PAGE, seed=seed)
    return dict(q=q, kpool=kpool, vpool=vpool, table=table, ids=ids, positions=positions, rows=rows, kc=kc, vc=vc,
                expect=expect, bound=bound, P=kpool.shape[0], NP=table.shape[1], Cl=table.shape[1] * DECODE_PAGE)

"""Shared cases and fixtures of the fp8 decode-linear and row-quantiser tests
(tests/test_fp8_cases_cpu.py, tests/test_gpu_fp8_linear.py), all built on the
CPU with fixed seeds.  Kernels: csrc/hip/fp8_kernels.hip.

Quantisers (one workgroup per row; thread t owns the 8 elements 8 (t + NT p),
NT = 256 threads, 1024 for SwiGLU):

* all_codes_case: rows of the 254 finite e4m3fn values (all exact in bf16) with
  +-448 present, so inv == scale == 1 and the expected codes are the input
  codes: no arithmetic, nothing ambiguous.
* tie_case: the midpoints of adjacent codes and a 448 anchor; the expected code
  is the even neighbour.
* placement_case: rows of small codes with one +-448 at an edge index or at the
  first element of a wave; a reduction that loses a wave gives the wrong scale.
* rmsnorm_exact_case: x = +-1, eps = 0, w = e4m3 values with one 448: mean(x^2)
  is exactly 1 and the codes are those of +-w.
* swiglu_exact_case / swiglu_placement_case: gate in {0, 32}, up = code / 32;
  silu(32) is 32 in fp32, so y is a code or a zero.

Skinny linear (k_fp8_gemm_skinny: wave w of WV takes the 256-byte blocks w,
w + WV of each trip of 2 WV; lane (r, g) reads bytes 64 u + 16 g .. + 16 of
its block at step u, the low and high 8 bytes in one MFMA each):

* int_linear_case: integer operands in [-8, 8], one 448 per weight row,
  power-of-two scales: every fp32 sum is exact in any order, the expected bf16
  output is one rounding of the exact value.
* one_hot_case: x row m is 1 at a single k_m, W[n, k] spells k in base 17, so
  y[m, :4] names the k that the kernel paired with row m.
* real_linear_case: quantised normal data, the fp64 product of the same codes
  and a derived elementwise bound.
"""
import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
FP8_MAX = 448.0

QUANT_K = [8, 504, 2048, 2056, 4104]  # below one pass of 256 threads, one pass (2048), one element into the next
SWIGLU_F = [8, 8192, 8200, 14336]  # the same for 1024 threads, and the Llama-3-8B width
RANDOM_K = [504, 2056, 4096]
RANDOM_F = [8200, 14336]
NKB = [1, 2, 3, 4, 5, 7, 8, 9, 13, 15, 16, 17, 25]
LIN_M, LIN_N = 64, 48
M_EDGES = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64]
M_EDGE_K = 2304
CHUNK_M = [65, 128, 130]
RESID_M = [1, 17, 64]
REAL_K = [2304, 4352, 14336]
REAL_M = [5, 40]
REAL_N = 64
OPTS = [0, 1, 2, 3]  # gpbs_hip_fp8_set_opts: bit 0 non-temporal loads, bit 1 four waves
CODE_448, CODE_ONE = 0x7E, 0x38


def finite_codes() -> torch.Tensor:
    """The 254 finite e4m3fn codes (both zeros included), uint8."""
    c = torch.arange(256, dtype=torch.int64)
    return c[(c & 0x7F) != 0x7F].to(torch.uint8)


def values(codes: torch.Tensor) -> torch.Tensor:
    """fp32 values of uint8 e4m3fn codes."""
    return codes.contiguous().view(F8).float()


def _small_codes() -> torch.Tensor:
    fc = finite_codes()
    return fc[(fc & 0x7F) <= 0x40]  # |v| <= 2


def all_codes_case(K: int, seed: int = 0):
    """(x bf16 [rows, K], codes uint8 [rows, K]): every row is a run of seeded
    permutations of the 254 finite codes cut to K; for K < 254 a +-448 is
    inserted at slot row % K and there are enough rows to show every code."""
    g = torch.Generator().manual_seed(1000 + 7 * K + seed)
    fc = finite_codes()
    body = K if K >= 254 else K - 1
    rows = 3 if K >= 254 else -(-254 // body) + 1
    if K >= 254:
        codes = torch.stack([torch.cat([fc[torch.randperm(254, generator=g)] for _ in range(-(-K // 254))])[:K]
                             for _ in range(rows)])
    else:
        stream = torch.cat([fc[torch.randperm(254, generator=g)] for _ in range(-(-rows * body // 254))])
        codes = torch.empty(rows, K, dtype=torch.uint8)
        for r in range(rows):
            p, part = r % K, stream[r * body:(r + 1) * body]
            anchor = torch.tensor([CODE_448 | (0x80 if r % 2 else 0)], dtype=torch.uint8)
            codes[r] = torch.cat([part[:p], anchor, part[p:]])
    return values(codes).to(BF), codes


def tie_case(seed: int = 0):
    """(x bf16 [4, 256], expect uint8 [4, 256]): the 126 midpoints of adjacent
    non-negative codes, their negatives and four 448 anchors, permuted per row.
    Round to nearest even: the midpoint of codes c and c + 1 goes to the even one."""
    g = torch.Generator().manual_seed(77 + seed)
    c = torch.arange(0x7E, dtype=torch.int64)  # 0 .. 0x7d: the lower neighbour
    v = values(torch.arange(0x7F, dtype=torch.uint8)).double()
    mid = (v[:-1] + v[1:]) / 2
    even = torch.where(c % 2 == 0, c, c + 1)
    x = torch.cat([mid, -mid, torch.full((4,), FP8_MAX, dtype=torch.float64)])
    e = torch.cat([even, even | 0x80, torch.full((4,), CODE_448)]).to(torch.uint8)
    perm = torch.stack([torch.randperm(256, generator=g) for _ in range(4)])
    xb = x.to(BF)
    assert torch.equal(xb.double(), x)  # 5 significant bits: exact in bf16
    return xb[perm], e[perm]


def placement_positions(K: int, threads: int = 256):
    """Element indices of the maximum: the edges 0, 7, 8, 511, 512, 2047, 2048,
    K - 1 and the first element of every wave of the workgroup in every pass."""
    pos = {p for p in (0, 7, 8, 511, 512, 2047, 2048, K - 1) if p < K}
    pos |= {8 * (64 * w + base) for base in range(0, K // 8, threads) for w in range(threads // 64)
            if 8 * (64 * w + base) < K}
    return sorted(pos)


def placement_case(K: int, threads: int = 256, seed: int = 0):
    """(x bf16 [P + 1, K], codes uint8, positions): row i holds codes of |v| <= 2
    and one +-448 at positions[i]; the last row is all zero (scale 1, codes 0).
    Every scale is exactly 1 and the expected codes are the input codes."""
    g = torch.Generator().manual_seed(31 * K + threads + seed)
    pos = placement_positions(K, threads)
    sm = _small_codes()
    codes = sm[torch.randint(0, sm.numel(), (len(pos) + 1, K), generator=g)]
    for i, p in enumerate(pos):
        codes[i, p] = CODE_448 | (0x80 if i % 2 else 0)
    codes[-1] = 0
    return values(codes).to(BF), codes, pos


def rmsnorm_exact_case(K: int, peak: int, seed: int = 0):
    """(x bf16 [3, K] of +-1, w bf16 [K], codes uint8 [3, K]): w holds e4m3 values
    of |v| <= 240 and a 448 at `peak`; with eps = 0 the normalised row is +-w."""
    g = torch.Generator().manual_seed(13 * K + peak + seed)
    fc = finite_codes()
    fc = fc[(fc & 0x7F) < 0x78]
    wc = fc[torch.randint(0, fc.numel(), (K,), generator=g)]
    wc[peak] = CODE_448
    neg = torch.randint(0, 2, (3, K), generator=g).to(torch.uint8)
    x = (1.0 - 2.0 * neg.float()).to(BF)
    return x, values(wc).to(BF), wc[None, :] ^ (neg << 7)


def swiglu_exact_case(F: int, seed: int = 0):
    """(gu bf16 [3, 2 F], codes uint8 [3, F], on bool [3, F]): gate = 32 where `on`,
    else 0; up = (e4m3 value) / 32, with a gated 448 / 32 per row.  y is the
    value of `codes` where on, a zero (of either sign) elsewhere."""
    g = torch.Generator().manual_seed(17 * F + seed)
    fc = finite_codes()
    codes = fc[torch.randint(0, 254, (3, F), generator=g)]
    on = torch.randint(0, 2, (3, F), generator=g).bool()
    for r, p in enumerate(torch.randint(0, F, (3,), generator=g).tolist()):
        codes[r, p], on[r, p] = CODE_448 | (0x80 if r % 2 else 0), True
    up = (values(codes) / 32).to(BF)
    assert torch.equal(up.float() * 32, values(codes))
    return torch.cat([on.float().to(BF) * 32, up], -1).contiguous(), codes, on


def swiglu_placement_case(F: int, seed: int = 0):
    """placement_case behind gate = 32 (up = value / 32) for the 1024-thread
    kernel: (gu bf16 [P + 1, 2 F], codes, positions); the last row has gate 0."""
    x, codes, pos = placement_case(F, threads=1024, seed=seed)
    gate = torch.full_like(x, 32.0)
    gate[-1] = 0
    up = (values(codes) / 32).to(BF)
    up[-1] = 1.0  # behind a closed gate: y = 0 whatever up holds
    return torch.cat([gate, up], -1).contiguous(), codes, pos


# ------------------------------------------------------------------ fp64 references of the quantisers
def quant64(h: torch.Tensor):
    """(t, s) in fp64: t = h 448 / amax, the exact value that each code rounds,
    and s = amax / 448 (1 for a zero row)."""
    h = h.double()
    amax = h.abs().amax(-1, keepdim=True)
    one = torch.ones_like(amax)
    t = h * torch.where(amax > 0, FP8_MAX / amax, one)
    return t, torch.where(amax > 0, amax / FP8_MAX, one).squeeze(-1)


def e4m3_step(t: torch.Tensor) -> torch.Tensor:
    """Spacing of the e4m3fn values in the binade of |t| (fp64): 2^(e - 3) for
    2^e <= |t| < 2^(e + 1), 2^-9 below 2^-6 (subnormals), 32 in the top binade."""
    e = torch.frexp(t.abs())[1].long() - 1
    e = torch.where(t == 0, torch.full_like(e, -6), e).clamp(-6, 8)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 3).double())


def code_excess(codes: torch.Tensor, t: torch.Tensor, rel: float):
    """(err, bound) in fp64: |value(code) - t| against half an e4m3 step at t plus
    `rel` relative.  A code that rounds a value within `rel` of t obeys it."""
    t = t.clamp(-FP8_MAX, FP8_MAX)
    return (values(codes).double() - t).abs(), e4m3_step(t) / 2 + rel * t.abs()


def rel_used(codes: torch.Tensor, t: torch.Tensor, rel: float) -> float:
    """The largest part of the relative allowance of code_excess that a code
    needs beyond half a step (0: every code is the nearest one or at a tie)."""
    t = t.clamp(-FP8_MAX, FP8_MAX)
    over = ((values(codes).double() - t).abs() - e4m3_step(t) / 2).clamp(min=0)
    nz = t != 0
    return (over[nz] / (rel * t[nz].abs())).max().item() if nz.any() else 0.0


def rmsnorm64(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xd = x.double()
    return xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def swiglu64(gu: torch.Tensor) -> torch.Tensor:
    F = gu.shape[-1] // 2
    a, b = gu[..., :F].double(), gu[..., F:].double()
    return a / (1 + torch.exp(-a)) * b


def random_rows(rows: int, K: int, seed: int) -> torch.Tensor:
    """Seeded normal bf16 rows (x 3), one of them all zero."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, K, generator=g) * 3).to(BF)
    if rows > 3:
        x[3] = 0
    return x


def rmsnorm_random_case(K: int):
    g = torch.Generator().manual_seed(400 + K)
    return torch.randn(9, K, generator=g).to(BF), (1 + 0.1 * torch.randn(K, generator=g)).to(BF)


def swiglu_random_case(F: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(500 + F)
    return torch.randn(5, 2 * F, generator=g).to(BF)


# ------------------------------------------------------------------ skinny linear
def int_linear_case(M: int, N: int, K: int, seed: int = 0, scales: bool = True):
    """(xq e4m3 [M, K], sx fp32 [M], wq e4m3 [N, K], sw fp32 [N], acc fp64 [M, N]):
    integers in [-8, 8], one +-448 per weight row, scales 2^(i % 5 - 2).
    |acc| <= 64 K + 3584 < 2^24 for K <= 6400, so any fp32 summation order gives
    acc itself."""
    g = torch.Generator().manual_seed(9000 + 131 * M + 17 * N + K + seed)
    x = torch.randint(-8, 9, (M, K), generator=g).double()
    w = torch.randint(-8, 9, (N, K), generator=g).double()
    n = torch.arange(N)
    w[n, (7 * n + 3) % K] = torch.where(n % 2 == 0, FP8_MAX, -FP8_MAX).double()
    two = torch.tensor(2.0)
    sx = torch.pow(two, (torch.arange(M) % 5 - 2).float()) if scales else torch.ones(M)
    sw = torch.pow(two, (n % 5 - 2).float()) if scales else torch.ones(N)
    xq, wq = x.float().to(F8), w.float().to(F8)
    assert torch.equal(xq.double(), x) and torch.equal(wq.double(), w)
    return xq, sx, wq, sw, x @ w.t()


def int_resid(M: int, N: int, seed: int = 0) -> torch.Tensor:
    """Integer residual in [-128, 128], bf16 [M, N]."""
    g = torch.Generator().manual_seed(600 + 3 * M + N + seed)
    return torch.randint(-128, 129, (M, N), generator=g).to(BF)


def int_expect(acc, sx, sw, resid=None) -> torch.Tensor:
    """bf16 of the exact acc sx sw (+ resid): the fp64 value is exact, fits fp32
    (test_fp8_cases_cpu.py asserts both), so this is the kernel's one rounding."""
    v = acc * sx.double()[:, None] * sw.double()[None, :]
    if resid is not None:
        v = v + resid.double()
    assert torch.equal(v.float().double(), v)
    return v.float().to(BF)


def one_hot_phases(nkb: int) -> int:
    """Phases of 64 rows that visit every (block, 8-byte slot) pair and every
    (slot, byte) pair of a block."""
    return max(4, -(-nkb // 2))


def one_hot_k(nkb: int, phase: int, M: int = LIN_M) -> torch.Tensor:
    """k_m of row m in this phase.  j = 64 phase + m counts the (block, slot)
    pairs: slot = 8 u + 2 g + half is the 8-byte unit of the 256-byte block
    (step u, lane group g, low or high MFMA), the block index is skewed by the slot so one phase already spreads
    over the blocks, the byte within the unit advances every 32 rows."""
    j = phase * M + torch.arange(M)
    pair = j % (32 * nkb)
    slot = pair % 32
    kb = (pair // 32 + slot) % nkb
    byte = (slot + j // 32) % 8
    return 256 * kb + 8 * slot + byte


def one_hot_weight(N: int, K: int) -> torch.Tensor:
    """W[n, k] = digit (n % 4) of k + 5 (n // 4) in base 17, minus 8: integers in
    [-8, 8]; columns 0..3 spell k itself (K < 17^4)."""
    assert K + 5 * (N // 4) < 17 ** 4
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return ((k + 5 * (n // 4)) // 17 ** (n % 4)) % 17 - 8


def one_hot_decode(y4: torch.Tensor) -> torch.Tensor:
    """The k spelled by output columns 0..3 ([.., 4] -> [..])."""
    d = (y4.double().round().long() + 8)
    return d[..., 0] + 17 * d[..., 1] + 289 * d[..., 2] + 4913 * d[..., 3]


def one_hot_case(nkb: int, phase: int, M: int = LIN_M, N: int = LIN_N):
    """(xq e4m3 [M, K], wq e4m3 [N, K], k [M], expect bf16 [M, N]), K = 256 nkb;
    both scale vectors are 1 and expect[m] = W[:, k_m]."""
    K = 256 * nkb
    k = one_hot_k(nkb, phase, M)
    x = torch.zeros(M, K)
    x[torch.arange(M), k] = 1.0
    w = one_hot_weight(N, K).float()
    return x.to(F8), w.to(F8), k, w[:, k].t().contiguous().to(BF)


def real_linear_case(M: int, N: int, K: int, quant):
    """Operands quantised by `quant` (quant_rows_fp8_ref) from seeded normal data,
    with the fp64 product of those codes and scales and the derived bound
        |y - ref| <= 2^-8 |ref| + K 2^-24 (|xq| |wq|^T) sx sw:
    the bf16 rounding of the output, and the fp32 accumulation of K products
    (each exact in fp32: 4-bit significands) in any order; the second term also
    covers the two fp32 multiplications by the scales.
    Returns (xq, sx, wq, sw, ref, bound)."""
    g = torch.Generator().manual_seed(7000 + 11 * M + K)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF)
    (xq, sx), (wq, sw) = quant(x), quant(w)
    sc = sx.double()[:, None] * sw.double()[None, :]
    ref = xq.double() @ wq.double().t() * sc
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (xq.double().abs() @ wq.double().abs().t()) * sc
    return xq, sx, wq, sw, ref, bound

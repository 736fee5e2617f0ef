"""Fixtures and fp64 references for the bf16 tenant kernels of
csrc/hip/tenant_kernels.hip (k_gemm_bf16_tn, k_gemm256_bf16_tn, k_stream_copy,
k_reduce_bf16, k_gemv_bf16).  Importable without a GPU: every input comes from
a seeded CPU generator, every reference is computed here in fp64 (or by plain
indexing) and rounded where the kernel rounds, and nothing is taken from the
code under test.  tests/test_tenant_cases_cpu.py checks that the fixtures do
what they claim; tests/test_gpu_tenant_exact.py holds the kernels to them."""
from functools import lru_cache

import torch

BF = torch.bfloat16

# ------------------------------------------------------------------ GEMM ---
# Bits prefilled into C before a launch: a bf16 NaN with a payload.  Every GEMM
# reference here is finite, so a tile the kernel never wrote keeps them.
GEMM_SENTINEL = 0x7FA5

# 256x256 kernel (M, N % 256 == 0): 1, 2, 3, 4 K-tiles on one tile (prologue
# only, both LDS buffers, buffer parity), then 4 tiles, 8 tiles (the smallest
# count at which the 2-D per-XCD blocks engage) and 12 tiles (where they fall
# back to row-major).
G256_KTILES = [(256, 256, 64), (256, 256, 128), (256, 256, 192), (256, 256, 256)]
G256_MULTI = [(512, 512, 192), (1024, 512, 128), (1024, 768, 64)]
G256_SHAPES = G256_KTILES + G256_MULTI
G256_GRIDS = (0, 1, 3)      # 0: the default (one tile per workgroup here); 1 and 3: several tiles per workgroup
G256_OPTS = (8, 9, 0, 1)    # 2-D blocks, 2-D blocks on the XCD-range queue, row-major, row-major XCD-range
# 128x128 kernel: 1 tile at 1 and 2 K-tiles, 3 tiles, and nine row panels
# (GROUP_M = 8: groups of 8 and 1) at one and three column panels.
G128_SHAPES = [(128, 128, 64), (128, 128, 128), (128, 384, 192), (1152, 128, 64), (1152, 384, 128)]
G128_GRIDS = (0, 1, 5)
GEMM_SHAPES = G256_SHAPES + G128_SHAPES
REAL_SHAPES = [(256, 256, 4096), (384, 128, 1024)]


def is_g256(M, N):
    return M % 256 == 0 and N % 256 == 0


def gemm_tile(M, N):
    return 256 if is_g256(M, N) else 128


def gemm_units(M, N):
    t = gemm_tile(M, N)
    return (M // t) * (N // t)


def gemm_ref64(A, B):
    """C = A @ B^T in fp64 from the bf16 operands."""
    return A.double() @ B.double().t()


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


@lru_cache(maxsize=None)
def int_case(M, N, K):
    """Integer operands in [-8, 8]: |sum| <= 64 K < 2^24, so an fp32 accumulator
    holds the exact integer whatever the order, and the only rounding is the
    epilogue's, to bf16: the output is ref64.to(bf16) bit for bit."""
    g = _gen(1, M, N, K)
    A = torch.randint(-8, 9, (M, K), generator=g).to(BF)
    B = torch.randint(-8, 9, (N, K), generator=g).to(BF)
    ref = gemm_ref64(A, B)
    return A, B, ref, ref.to(BF).view(torch.int16)


def kselect_f(rows, K):
    """k = f(row).  Within every aligned 128-row block -- an A or B half of the
    256x256 kernel, a tile of the 128x128 kernel -- f hits all 64 positions of
    a K-tile (8 sixteen-byte chunks x 8 elements: both kernels' XOR swizzles)
    and every K-tile; it differs from block to block, so no two tiles of the
    selected output are equal."""
    r = torch.arange(rows)
    nk = K // 64
    pos = (5 * r + 3 + 9 * (r // 128)) % 64               # a bijection on 64 consecutive rows, shifted per block
    kt = ((r % 128) * nk // 128 + r // 128) % nk          # every K-tile within 128 rows, rotated per block
    return kt * 64 + pos


def coded(rows, K):
    """Integers in [-125, 125] (exact in bf16) from (row, k), not symmetric in
    the two."""
    r = torch.arange(rows)[:, None]
    k = torch.arange(K)[None, :]
    return ((7 * r + 13 * k + (r * k) % 11) % 251 - 125).to(BF)


def _onehot(rows, K):
    f = kselect_f(rows, K)
    X = torch.zeros(rows, K)
    X[torch.arange(rows), f] = 1
    return X.to(BF), f


@lru_cache(maxsize=None)
def kselect_case(M, N, K, direction):
    """'a': A has one 1 per row at k = f(m), so C[m, n] = B[n, f(m)].
    'b': the mirror, C[m, n] = A[m, f(n)].  The reference is the indexing
    itself, in fp64; each output is one product and exact."""
    if direction == "a":
        A, f = _onehot(M, K)
        B = coded(N, K)
        ref = B.double()[:, f].t().contiguous()
    else:
        B, f = _onehot(N, K)
        A = coded(M, K)
        ref = A.double()[:, f].contiguous()
    return A, B, ref, ref.to(BF).view(torch.int16)


@lru_cache(maxsize=None)
def real_case(M, N, K):
    """randn bf16 operands, the fp64 product and the per-element error bound
    2^-8 |ref| + K 2^-23 (|A| @ |B|^T): see gemm_bound."""
    g = _gen(2, M, N, K)
    A = torch.randn(M, K, generator=g).to(BF)
    B = torch.randn(N, K, generator=g).to(BF)
    ref = gemm_ref64(A, B)
    return A, B, ref, gemm_bound(A, B, ref)


def gemm_bound(A, B, ref):
    """Products of two bf16 values are exact in fp32 (16 significant bits), so
    the only errors are (1) the K - 1 fp32 additions of a dot product, each at
    most one unit in the last place of a partial sum -- 2^-23 relative, which
    also covers an MFMA adder that truncates instead of rounding -- and no
    partial sum exceeds sum |a||b|: (K - 1) 2^-23 (|A| @ |B|^T) in any order;
    and (2) rounding the fp32 result to bf16, half a unit of its 8-bit
    significand: at most 2^-8 of the value.  That value is the computed one,
    not the reference; the difference is 2^-8 of term (1), and the K-th
    multiple of 2^-23 in K 2^-23 pays for it."""
    K = A.shape[1]
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (A.double().abs() @ B.double().abs().t())


def tiles_of(ref, t=128):
    """The t x t tiles of a reference, as byte strings, in row-major tile order."""
    M, N = ref.shape
    return [ref[i:i + t, j:j + t].contiguous().numpy().tobytes() for i in range(0, M, t) for j in range(0, N, t)]


# ------------------------------------------------- stream copy and reduce ---
# Both walk chunks of 16-byte vectors; a workgroup of NT threads keeps U
# vectors per thread in flight, so one pass of its inner loop covers NT * U
# vectors and every vector of a pass sits behind its own idx < end guard.
MEM_LEAD = 16            # bytes: buffers are views 16 bytes into their allocations (alignment 16, not 256)
MEM_GRIDS = (0, 1, 3)    # default (256 workgroups), one, and three with more chunks than workgroups
STREAM_OPTS = (0, 1, 2, 3)
REDUCE_OPTS = tuple(range(32))
COPY_SENTINEL = 0xA5     # guard byte of the copy destination
REDUCE_SENTINEL = 0x5A5A  # guard bits of the reduce output: a finite bf16 (1.5e16) no sum here reaches


def stream_geom(opts):
    """(threads, vectors in flight per thread) of gpbs_hip_set_stream_opts(opts)."""
    return 256, (8 if opts & 2 else 16)


def reduce_geom(opts):
    """(threads, vector pairs in flight per thread) of gpbs_hip_set_reduce_opts(opts)."""
    return (512 if opts & 16 else 256), (6, 8, 4, 12)[opts & 3]


def mem_chunks(nt, u):
    """Chunk sizes in vectors: one vector, 4096 bytes, one pass exactly, one pass + one vector."""
    return [1, 256, nt * u, nt * u + 1]


def mem_sizes(nt, u, chunk):
    """Buffer sizes in vectors: 1; one below, at and above the workgroup (256
    threads, and NT where that is 512); one pass; one pass + 1; three chunks +
    17 (a partial last chunk, and more chunks than three workgroups)."""
    s = [1, 255, 256, 257, nt - 1, nt, nt + 1, nt * u, nt * u + 1, 3 * chunk + 17]
    return sorted(set(s))


def _round_up(x, m):
    return (x + m - 1) // m * m


# One guard size for every launch: at least the largest chunk of any variant
# (one pass + one vector), a multiple of 256 bytes so a guarded view keeps the
# 16-byte offset of its buffer.
STREAM_GUARD = _round_up((256 * 16 + 1) * 16, 256)
REDUCE_GUARD = _round_up((512 * 12 + 1) * 16, 256)
STREAM_MAX_VEC = 3 * (256 * 16 + 1) + 17
REDUCE_MAX_VEC = 3 * (512 * 12 + 1) + 17


@lru_cache(maxsize=None)
def stream_payload():
    """Random bytes, one vector more than the largest copy (so that a copy that
    runs one vector long has something other than the guard to bring along)."""
    g = _gen(3)
    return torch.randint(0, 256, ((STREAM_MAX_VEC + 1) * 16,), generator=g, dtype=torch.int32).to(torch.uint8)


def copy_image(src, nbytes, guard=STREAM_GUARD):
    """What the destination allocation must hold after copying src[:nbytes]
    into the view that starts MEM_LEAD + guard bytes in: sentinel bytes,
    the payload, sentinel bytes."""
    img = torch.full((MEM_LEAD + guard + nbytes + guard,), COPY_SENTINEL, dtype=torch.uint8)
    img[MEM_LEAD + guard:MEM_LEAD + guard + nbytes] = src[:nbytes]
    return img


def _bits(*v):
    return torch.tensor([x - 0x10000 if x >= 0x8000 else x for x in v], dtype=torch.int16)


# (a bits, b bits, bits of a + b; None = any NaN).  bf16: 1 sign, 8 exponent, 7
# fraction bits.  0x4380 = 256, 0x4381 = 258, 0x4382 = 260, 0x3F80 = 1,
# 0x7F7F = the largest finite value, 0x0080 = the smallest normal one,
# 0x0001-0x007F the subnormals (multiples of 2^-133).
REDUCE_PLANTED = [
    (0x0000, 0x0000, 0x0000),   # +0 + +0 = +0
    (0x8000, 0x8000, 0x8000),   # -0 + -0 = -0
    (0x0000, 0x8000, 0x0000),   # +0 + -0 = +0 (round to nearest)
    (0x7F80, 0x7F80, 0x7F80),   # inf + inf
    (0xFF80, 0xFF80, 0xFF80),   # -inf + -inf
    (0x7F80, 0xC380, 0x7F80),   # inf + -256
    (0x7F80, 0xFF80, None),     # inf + -inf = NaN
    (0xFF80, 0x7F80, None),
    (0x7F7F, 0x7F7F, 0x7F80),   # largest finite twice: 2^129 (1 - 2^-8) is past fp32, inf before the bf16 rounding
    (0xFF7F, 0xFF7F, 0xFF80),
    (0x4380, 0x3F80, 0x4380),   # 256 + 1 = 257: a tie between 256 and 258, to the even 256
    (0x4381, 0x3F80, 0x4382),   # 258 + 1 = 259: a tie between 258 and 260, to the even 260
    (0xC380, 0xBF80, 0xC380),   # and their negatives
    (0xC381, 0xBF80, 0xC382),
    (0x0001, 0x0001, 0x0002),   # smallest subnormal twice
    (0x0040, 0x0040, 0x0080),   # two subnormals make the smallest normal
    (0x0080, 0x8001, 0x007F),   # smallest normal - smallest subnormal: a subnormal result
    (0x0003, 0x8001, 0x0002),   # subnormal - subnormal
    (0x8055, 0x802A, 0x807F),   # negative subnormals, the largest subnormal result
]
REDUCE_SUBNORMAL_ROWS = range(14, 19)


def _planted_run():
    """The planted pairs twice over, the second copy an odd distance after the
    first: every pair sits once in the low and once in the high half of a
    32-bit word."""
    a = [p[0] for p in REDUCE_PLANTED]
    b = [p[1] for p in REDUCE_PLANTED]
    pad = [0x3F80] if len(a) % 2 == 0 else []
    return _bits(*(a + pad + a)), _bits(*(b + pad + b))


def reduce_planted_at(n):
    """[(element index, planted row)] for a buffer of n elements: the run from
    element 0 on (cut off where the buffer ends) and, where two runs fit, again
    ending on the last element."""
    L = len(REDUCE_PLANTED)
    gap = 1 if L % 2 == 0 else 0
    run = [(i, i) for i in range(L)] + [(L + gap + i, i) for i in range(L)]
    R = 2 * L + gap
    at = [(i, r) for i, r in run if i < n]
    if n >= 2 * R:
        at += [(n - R + i, r) for i, r in run]
    return at


@lru_cache(maxsize=None)
def _reduce_base():
    g = _gen(4)
    n = REDUCE_MAX_VEC * 8
    scale = torch.exp2(torch.randint(-12, 13, (2, n), generator=g).float())
    x = (torch.randn(2, n, generator=g) * scale).to(BF)
    return x[0].contiguous(), x[1].contiguous()


@lru_cache(maxsize=None)
def reduce_case(n8):
    """a, b (bf16 [8 n8]) with the planted pairs at both ends, the expected
    output bits and the mask of outputs that must be NaN (any payload).
    Reference: the fp64 sum (exact, or far from any fp32 tie when the
    exponents lie more than 45 apart), rounded once to fp32 and then to bf16,
    which is what the kernel does."""
    n = 8 * n8
    a0, b0 = _reduce_base()
    a, b = a0[:n].clone(), b0[:n].clone()
    pa, pb = _planted_run()
    R = pa.numel()
    head = min(R, n)
    a.view(torch.int16)[:head] = pa[:head]
    b.view(torch.int16)[:head] = pb[:head]
    if n >= 2 * R:
        a.view(torch.int16)[n - R:] = pa
        b.view(torch.int16)[n - R:] = pb
    ref = (a.double() + b.double()).float().to(BF)
    return a, b, ref.view(torch.int16).clone(), ref.isnan()


def reduce_image(n8, guard=REDUCE_GUARD):
    """(expected bits, must-be-NaN mask) of the whole output allocation: the
    result in a view MEM_LEAD + guard bytes in, sentinel bits around it."""
    _, _, bits, nan = reduce_case(n8)
    lead, n = (MEM_LEAD + guard) // 2, bits.numel()
    img = torch.full((lead + n + guard // 2,), REDUCE_SENTINEL, dtype=torch.int16)
    img[lead:lead + n] = bits
    mask = torch.zeros(img.numel(), dtype=torch.bool)
    mask[lead:lead + n] = nan
    return img, mask


# ------------------------------------------------------------------ GEMV ---
# A wave walks K in 512-column chunks, two at a time (GV_U = 2) and a tail loop
# for the odd one: K = 512 is the tail loop alone, 1536 one unrolled step and
# the tail, 2048 unrolled steps only.  A unit is 16 rows; R = 4097 is 257
# units, one more than the 256-workgroup cap.
GEMV_K = (512, 1536, 2048)
GEMV_R = (1, 15, 16, 17, 1000, 4097)
GEMV_GRID1_R = 100
GEMV_ONEHOT_R = 17
GEMV_GUARD = 17                 # floats on either side of y: its alignment is 4 bytes
GEMV_SENTINEL = 0x7FC00A5A      # an fp32 NaN with a payload


@lru_cache(maxsize=None)
def gemv_int_case(R, K):
    """Integer W and x in [-8, 8]: |sum| <= 64 K < 2^24, the fp32 output is the
    exact integer and equality is bitwise."""
    g = _gen(5, R, K)
    W = torch.randint(-8, 9, (R, K), generator=g).to(BF)
    x = torch.randint(-8, 9, (K,), generator=g).to(BF)
    return W, x, (W.double() @ x.double()).float().view(torch.int32)


def gemv_onehot_ks(K):
    """Every column of the first and of the last 512-column chunk: all 8
    elements of all 64 lanes' 16-byte slots."""
    return sorted(set(range(512)) | set(range(K - 512, K)))


@lru_cache(maxsize=None)
def gemv_onehot_case(K, R=GEMV_ONEHOT_R):
    """W coded from (row, k); x = e_k gives y = W[:, k].  Returns W, the list of
    k and the expected columns [len(ks), R] as fp32 bits."""
    W = coded(R, K)
    ks = gemv_onehot_ks(K)
    return W, ks, W.double()[:, ks].t().contiguous().float().view(torch.int32)


@lru_cache(maxsize=None)
def gemv_real_case(R, K):
    """randn data, the fp64 product and the bound K 2^-23 (|W| @ |x|) per row:
    exact bf16 products, fewer than K fp32 additions in an unknown order, each
    within 2^-23 of a partial sum that never exceeds sum |w||x|."""
    g = _gen(6, R, K)
    W = torch.randn(R, K, generator=g).to(BF)
    x = torch.randn(K, generator=g).to(BF)
    return W, x, W.double() @ x.double(), K * 2.0 ** -23 * (W.double().abs() @ x.double().abs())


def gemv_image(bits, guard=GEMV_GUARD):
    """The whole y allocation as int32: sentinels, the result, sentinels."""
    img = torch.full((guard + bits.numel() + guard,), GEMV_SENTINEL, dtype=torch.int32)
    img[guard:guard + bits.numel()] = bits
    return img

"""Paged cases of the block-table attention tests (tests/test_paged_cpu.py,
tests/test_gpu_paged_attn.py), built from the ragged exact-data fixtures
(ragged_cases.decode_case / prefill_case): each sequence's dense cache is
scattered into a pool under a shuffled page assignment, non-monotonic and
interleaved between the sequences.

Everything the kernels must not read is poisoned: every unreferenced pool page
and every page row past a sequence's last row is NaN, and the table entries
past a sequence's last used page (the whole row of an idle sequence) are
garbage, -1 and 2**30 in turn.

Logical contexts: Cl = NP * page = 1152 for the decode fixtures (C 1100) with
either page size, 448 (page 64) / 512 (page 128) for the prefill fixtures
(C 400).
"""
import torch

import decode_cases as DC
import prefill_cases as PC
import ragged_cases as RC

BF = torch.bfloat16
PAGES = (64, 128)
SPARE = 3  # unreferenced (all-NaN) pages in every pool
GARBAGE = (-1, 2 ** 30)
DECODE_CL = 1152

# RC.DECODE_SETS with the ">= C" idle value moved to the paged rule's ">= Cl"
DECODE_SETS = [[DECODE_CL if p >= DC.C else p for p in s] for s in RC.DECODE_SETS]
PREFILL_SETS = RC.PREFILL_SETS


def n_table(C: int, page: int) -> int:
    return -(-C // page)


def decode_active(pos: int) -> bool:
    return 0 <= pos < DECODE_CL


def assign_pages(npages, seed: int, spare: int = SPARE):
    """A shuffled page assignment: ids[b] = the pool pages of sequence b in logical
    order, dealt round-robin over the sequences from a random permutation of
    range(P), P = sum(npages) + spare.  Returns (ids, P)."""
    P = sum(npages) + spare
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed)).tolist()
    ids = [[] for _ in npages]
    for i in range(max(npages, default=0)):
        for b, n in enumerate(npages):
            if i < n:
                ids[b].append(perm.pop())
    return ids, P


def make_table(ids, NP: int) -> torch.Tensor:
    """int32 [B, NP]: the used entries, then garbage."""
    rows = [list(r) + [GARBAGE[(b + i) % 2] for i in range(NP - len(r))] for b, r in enumerate(ids)]
    return torch.tensor(rows, dtype=torch.int32)


def scatter(kc: torch.Tensor, vc: torch.Tensor, rows, page: int, seed: int = 0, ids=None, P=None):
    """Dense caches [B, Hkv, C, 128] -> (kpool, vpool [P, Hkv, page, 128], table
    int32 [B, NP], ids): the first rows[b] rows of sequence b go to its pages,
    everything else in the pools is NaN."""
    B, Hkv, C, hd = kc.shape
    if ids is None:
        ids, P = assign_pages([-(-r // page) for r in rows], seed)
    kpool = torch.full((P, Hkv, page, hd), float("nan"), dtype=kc.dtype)
    vpool = torch.full((P, Hkv, page, hd), float("nan"), dtype=vc.dtype)
    for b, r in enumerate(rows):
        for i, pg in enumerate(ids[b]):
            n = min(page, r - i * page)
            kpool[pg, :, :n] = kc[b, :, i * page:i * page + n]
            vpool[pg, :, :n] = vc[b, :, i * page:i * page + n]
    return kpool, vpool, make_table(ids, n_table(C, page)), ids


def gather_dense(pool: torch.Tensor, ids, rows, Cl: int) -> torch.Tensor:
    """The dense [B, Hkv, Cl, 128] cache the _seq kernels take: sequence b's first
    rows[b] rows read back through its pages with plain indexing, NaN elsewhere."""
    P, Hkv, page, hd = pool.shape
    out = torch.full((len(ids), Hkv, Cl, hd), float("nan"), dtype=pool.dtype, device=pool.device)
    for b, r in enumerate(rows):
        for i in range(-(-r // page)):
            n = min(page, r - i * page)
            out[b, :, i * page:i * page + n] = pool[ids[b][i], :, :n]
    return out


def decode_case(s: int, H: int, Hkv: int, page: int, shift: int = 0):
    """Paged form of RC.decode_case(RC.DECODE_SETS[s], ...): a dict with q, the
    pools, table, ids, positions (paged rule), rows (pos + 1 per active sequence,
    one more where the shifted fixture codes row pos + 1), the dense caches and
    t / expect of the ragged fixture."""
    positions = DECODE_SETS[s]
    q, kc, vc, t, expect = RC.decode_case(RC.DECODE_SETS[s], H, Hkv, shift)
    rows = [min(p + 1 + shift, DC.C) if decode_active(p) else 0 for p in positions]
    kpool, vpool, table, ids = scatter(kc, vc, rows, page, seed=1000 * s + page + shift)
    return dict(q=q, kpool=kpool, vpool=vpool, table=table, ids=ids, positions=positions, rows=rows, kc=kc, vc=vc,
                t=t, expect=expect, P=kpool.shape[0], NP=table.shape[1], Cl=table.shape[1] * page)


def prefill_case(s: int, H: int, Hkv: int, page: int, shift: int = 0):
    """Paged form of RC.prefill_case(RC.PREFILL_SETS[s], ...); rows = pos + n."""
    q, kc, vc, pos, lens, expect = RC.prefill_case(PREFILL_SETS[s], H, Hkv, shift)
    rows = [p + n if n else 0 for p, n in zip(pos, lens)]
    kpool, vpool, table, ids = scatter(kc, vc, rows, page, seed=2000 * s + page + shift)
    return dict(q=q, kpool=kpool, vpool=vpool, table=table, ids=ids, pos=pos, lens=lens, rows=rows, kc=kc, vc=vc,
                expect=expect, P=kpool.shape[0], NP=table.shape[1], Cl=table.shape[1] * page)

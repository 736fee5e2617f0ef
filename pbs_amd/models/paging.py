"""Host-side page accounting of the paged KV cache (LlamaDecoder(paged=True)).

A pool of ``pages`` fixed-size pages, a free list and a reference count per
page.  The counts exist for prefix sharing: a page mapped into two slots'
block tables is returned to the free list when the second of them lets go.
Nothing here touches a device: the pool hands out page ids, the decoder
writes them into its block table.
"""
from __future__ import annotations

from collections import Counter
from typing import Iterable, List


class PoolExhausted(RuntimeError):
    """A request for more pages than are free; nothing was allocated."""


class PagePool:
    def __init__(self, pages: int):
        if not isinstance(pages, int) or isinstance(pages, bool) or pages < 1:
            raise ValueError(f"PagePool: pages must be a positive int, got {pages!r}")
        self.pages = pages
        self.ref = [0] * pages
        self._free = list(range(pages - 1, -1, -1))  # popped from the end: lowest id first

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def alloc(self, n: int) -> List[int]:
        """n fresh pages (refcount 1 each), or PoolExhausted with the pool unchanged."""
        if n < 0:
            raise ValueError(f"PagePool: cannot allocate {n} pages")
        if n > len(self._free):
            raise PoolExhausted(f"PagePool: {n} pages wanted, {len(self._free)} of {self.pages} free")
        ids = [self._free.pop() for _ in range(n)]
        for i in ids:
            self.ref[i] = 1
        return ids

    def _held(self, ids: Iterable[int], what: str) -> Counter:
        want = Counter(int(i) for i in ids)
        for i, k in want.items():
            if not 0 <= i < self.pages or self.ref[i] < k:
                raise ValueError(f"PagePool: {what} of page {i} x{k}, which has "
                                 f"{self.ref[i] if 0 <= i < self.pages else 'no'} reference(s)")
        return want

    def share(self, ids: Iterable[int]) -> List[int]:
        """One more reference to each of these allocated pages."""
        ids = [int(i) for i in ids]
        self._held(set(ids), "share")
        for i in ids:
            self.ref[i] += 1
        return ids

    def free(self, ids: Iterable[int]):
        """Drop one reference per listed page; a page with none left is free
        again.  A page that is not allocated (a double free) is refused, and
        then no count has changed."""
        for i, k in sorted(self._held(ids, "free").items()):
            self.ref[i] -= k
            if self.ref[i] == 0:
                self._free.append(i)

    def snapshot(self):
        return list(self.ref), list(self._free)

    def restore(self, snap):
        self.ref, self._free = list(snap[0]), list(snap[1])

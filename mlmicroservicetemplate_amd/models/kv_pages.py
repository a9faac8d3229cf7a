"""Paged KV cache bookkeeping (SURVEY.md §2.E.1 K13 "paged write", §5.7 paged allocator).

The fused decode-attention kernel walks a sequence's keys in splits of ``page_rows`` (64) rows,
so one page is exactly one split: a block reads ONE page-table entry and then the same contiguous
rows it read from a per-sequence cache.  The caches become page pools ``[pages, page_rows, Hkv,
D]`` per layer, shared by every sequence, and a sequence holds only the pages its prompt +
generation budget needs instead of a ``max_seq`` slab -- on 288 GB of HBM the pool is sized by
the tokens actually in flight, not by ``max_batch x max_seq``.

Page 0 is a scratch page that every unassigned table entry points at: idle decode slots (the
fixed-shape decode graph runs all ``max_batch`` rows) write their dummy token there, never into
a live sequence's page.

Shared pages (prefix caching, models/prefix_cache.py): every page carries a reference count.  A page
that only ``assign`` ever handed out has one owner and behaves as before.  ``adopt(slot, pages)`` puts
already-filled pages at the front of a slot's list and counts the slot as one more holder; ``release``
drops one reference per page, and a page nobody holds returns to the free list -- unless the prefix
index (``PageTable.index``) still maps a token run to it: then it is *reclaimable*, counted as
available by ``free_pages`` / ``can_fit`` and evicted by ``assign`` only when the free list runs short.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch


class OutOfPages(RuntimeError):
    pass


class PageTable:
    """Host page allocator + the ``[max_batch, pages_per_seq]`` int32 table the kernels read.

    ``assign(slot, rows)`` gives a slot pages for ``rows`` cache rows (growing its list),
    ``release(slot)`` returns them; ``device_table()`` copies the host table into a static device
    buffer (the captured decode graphs read that same buffer, so it is refreshed in place)."""

    def __init__(self, num_pages: int, page_rows: int, max_batch: int, pages_per_seq: int, device="cpu"):
        if num_pages < 2:
            raise ValueError("need at least one scratch page and one data page")
        self.num_pages, self.page_rows = int(num_pages), int(page_rows)
        self.max_batch, self.pages_per_seq = int(max_batch), int(pages_per_seq)
        self.device = torch.device(device)
        self._free: List[int] = list(range(self.num_pages - 1, 0, -1))  # page 0 = scratch
        self._owned: Dict[int, List[int]] = {}
        self._ref: List[int] = [0] * self.num_pages  # holders (slots) of each page
        self.index = None  # models/prefix_cache.PrefixCache when prefix caching is on
        self._reclaimable = 0  # pages with no holder that the index still maps
        pin = self.device.type == "cuda"
        self.host = torch.zeros(self.max_batch, self.pages_per_seq, dtype=torch.int32, pin_memory=pin)
        self.dev = torch.zeros(self.max_batch, self.pages_per_seq, dtype=torch.int32, device=self.device)
        self._dirty = False

    # ------------------------------------------------------------------ accounting
    @property
    def free_pages(self) -> int:
        return len(self._free) + self._reclaimable

    def refcount(self, page: int) -> int:
        return self._ref[page]

    def pages_for(self, rows: int) -> int:
        return -(-int(rows) // self.page_rows)

    def can_fit(self, rows: int, slot: Optional[int] = None) -> bool:
        have = len(self._owned.get(slot, ())) if slot is not None else 0
        return self.pages_for(rows) - have <= self.free_pages

    def pages_of(self, slot: int) -> List[int]:
        return list(self._owned.get(slot, ()))

    # ------------------------------------------------------------------ assignment
    def assign(self, slot: int, rows: int) -> None:
        """Make ``slot`` cover cache rows ``[0, rows)``; raises :class:`OutOfPages` (changing
        nothing) when the pool cannot."""
        if not 0 <= slot < self.max_batch:
            raise ValueError(f"slot {slot} outside [0, {self.max_batch})")
        need = self.pages_for(rows)
        if need > self.pages_per_seq:
            raise ValueError(f"{rows} rows exceed the {self.pages_per_seq * self.page_rows}-row sequence limit")
        owned = self._owned.setdefault(slot, [])
        extra = need - len(owned)
        if extra <= 0:
            return
        if extra > self.free_pages:
            raise OutOfPages(f"slot {slot} needs {extra} more pages, {self.free_pages} free")
        if extra > len(self._free):  # evict exactly the shortfall: least recently used reclaimable pages
            for page in self.index.evict(extra - len(self._free)):
                self._reclaimable -= 1
                self._free.append(page)
        for _ in range(extra):
            page = self._free.pop()
            self._ref[page] = 1
            self.host[slot, len(owned)] = page
            owned.append(page)
        self._dirty = True

    def adopt(self, slot: int, pages: List[int]) -> None:
        """Put the already-filled shared ``pages`` at the front of ``slot``'s (empty) list: the slot
        becomes one more holder of each and must never write their rows."""
        if not 0 <= slot < self.max_batch:
            raise ValueError(f"slot {slot} outside [0, {self.max_batch})")
        if self._owned.get(slot):
            raise ValueError(f"slot {slot} already holds pages: shared pages go first")
        if len(pages) > self.pages_per_seq:
            raise ValueError(f"{len(pages)} pages exceed the {self.pages_per_seq}-page sequence limit")
        for page in pages:
            if not 0 < page < self.num_pages or (self._ref[page] == 0 and not self._indexed(page)):
                raise ValueError(f"page {page} is not a filled page")
        owned = self._owned.setdefault(slot, [])
        for page in pages:
            if self._ref[page] == 0:
                self._reclaimable -= 1
            self._ref[page] += 1
            self.host[slot, len(owned)] = page
            owned.append(page)
        if pages:
            self._dirty = True

    def _indexed(self, page: int) -> bool:
        return self.index is not None and self.index.holds(page)

    def release(self, slot: int) -> None:
        pages = self._owned.pop(slot, [])
        if pages:
            for page in reversed(pages):
                self._ref[page] -= 1
                if self._ref[page] == 0:
                    if self._indexed(page):
                        self._reclaimable += 1
                    else:
                        self._free.append(page)
            self.host[slot].zero_()
            self._dirty = True

    def unindexed(self, pages: List[int]) -> None:
        """The index dropped its entries for ``pages`` without evicting them (``PrefixCache.clear``):
        those nobody holds return to the free list."""
        for page in pages:
            if self._ref[page] == 0:
                self._reclaimable -= 1
                self._free.append(page)

    def reset(self) -> None:
        for slot in list(self._owned):
            self.release(slot)

    def device_table(self) -> torch.Tensor:
        if self._dirty:
            self.dev.copy_(self.host, non_blocking=self.device.type == "cuda")
            self._dirty = False
        return self.dev

    # ------------------------------------------------------------------ row addressing
    def rows(self, slots: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """Flat pool row of (slot, position) pairs (broadcasting) from the DEVICE table."""
        table = self.device_table()
        p = positions.long()
        page = table[slots.long(), torch.div(p, self.page_rows, rounding_mode="floor")]
        return page.long() * self.page_rows + p % self.page_rows

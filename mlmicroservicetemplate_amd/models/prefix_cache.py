"""Prefix caching for the paged KV cache: an index from "these 64 tokens after that prefix" to the page
that already holds their K / V rows, so a request repeating an earlier prompt's beginning adopts those
pages (``PageTable.adopt``) and prefills only its suffix (``LlamaTP.step(past=hit rows)``).

Host only, pure Python.  The index is a trie over full pages of *prompt* tokens: a page's key is
(its parent entry, the tuple of its ``page_rows`` token ids).  The token tuple is stored and compared
exactly -- a hash only picks the dict bucket, it never produces a hit on its own.

Invariant -- shared pages are never written.  A sequence with a hit of ``P`` rows (a multiple of the
page size) writes rows ``>= P`` only, and those lie in pages ``assign`` gave it alone: the rows of its
prompt suffix, its decode rows, a verify step's rejected-draft rows, and the chunked-prefill dummy
decode row at ``pos = rows done`` (``rows done >= P``).  Idle slots keep writing to scratch page 0.
``match`` therefore never returns the page that holds a prompt's last token: at least one prompt token
is always computed (its logits are needed), so ``P <= len - 1``.

Eviction takes reclaimable pages only (no holder, ``PageTable``), least recently used first by the
engine's iteration counter -- never by wall-clock time, so TP ranks that see the same admissions and
retirements keep identical indexes without exchanging anything.  Among equal stamps the deeper page
goes first, then the lower page id; every operation that stamps an entry stamps its ancestors with the
same value, so a parent never goes before its child.

Invariant -- every holder of an entry's page holds the pages of all its ancestors.  Adoption takes a
whole chain, and ``insert`` hangs a sequence's page only under an entry whose page that sequence holds:
when two prompts with a common beginning both miss (a burst admitted before the first has prefilled),
the first indexes the common pages and the second, whose copies of them stay private, stops indexing at
the first entry that maps to a page it does not hold.  So an entry nobody holds has no held descendant:
every page ``PageTable`` counts as reclaimable can in fact be evicted, and admission never over-commits.

The cached rows are functions of the model's weights: anything that replaces the weights of a model in
service must call :meth:`PrefixCache.clear`.
"""
from __future__ import annotations

import heapq
from typing import Dict, List, Optional, Sequence

from .kv_pages import PageTable


def _key_hash(tokens: tuple) -> int:
    return hash(tokens)


class _Key:
    """The token run of one page as a dict key: hashed through :func:`_key_hash`, equal only when the
    tuples are."""
    __slots__ = ("tokens",)

    def __init__(self, tokens: Sequence[int]):
        self.tokens = tuple(int(t) for t in tokens)

    def __hash__(self) -> int:
        return _key_hash(self.tokens)

    def __eq__(self, other) -> bool:
        return isinstance(other, _Key) and self.tokens == other.tokens


class _Node:
    __slots__ = ("page", "key", "parent", "children", "stamp", "depth")

    def __init__(self, page: int, key: Optional[_Key], parent: Optional["_Node"], stamp: int):
        self.page, self.key, self.parent = page, key, parent
        self.children: Dict[_Key, "_Node"] = {}
        self.stamp = stamp
        self.depth = 0 if parent is None else parent.depth + 1


class PrefixCache:
    def __init__(self, pages: PageTable):
        if pages.index is not None:
            raise ValueError("the page table already has a prefix index")
        self.pages = pages
        self.rows = pages.page_rows
        self._root = _Node(0, None, None, 0)
        self._by_page: Dict[int, _Node] = {}
        self.evictions = 0
        pages.index = self

    def __len__(self) -> int:
        return len(self._by_page)

    def holds(self, page: int) -> bool:
        return page in self._by_page

    def _walk(self, ids: Sequence[int], limit: int) -> List[_Node]:
        node, chain = self._root, []
        for i in range(limit):
            node = node.children.get(_Key(ids[i * self.rows: (i + 1) * self.rows]))
            if node is None:
                break
            chain.append(node)
        return chain

    def match(self, ids: Sequence[int], stamp: Optional[int] = None) -> List[int]:
        """Pages of the longest cached chain of ``ids``' full pages, at most ``(len(ids) - 1) // rows`` of
        them.  ``stamp`` (the engine's iteration counter, when the caller adopts the pages): marks the
        whole chain as used now."""
        chain = self._walk(ids, (len(ids) - 1) // self.rows)
        if stamp is not None:
            for n in chain:
                n.stamp = max(n.stamp, stamp)
        return [n.page for n in chain]

    def insert(self, ids: Sequence[int], pages: Sequence[int], stamp: int) -> int:
        """Index the full pages of the prompt ``ids`` whose rows are completely in ``pages`` (the
        sequence's page list, shared pages first).  A run that is already indexed keeps its entry (and
        its page); indexing stops at the first entry that maps to a page other than the sequence's own
        (module docstring: nothing hangs under a page its holder does not hold).  The chain walked is
        stamped.  Returns the number of new entries."""
        node, new = self._root, 0
        for i in range(min(len(ids) // self.rows, len(pages))):
            key = _Key(ids[i * self.rows: (i + 1) * self.rows])
            page = int(pages[i])
            child = node.children.get(key)
            if child is None:
                if page in self._by_page:  # a page is the value of one entry only
                    break
                child = node.children[key] = _Node(page, key, node, stamp)
                self._by_page[page] = child
                new += 1
            elif child.page != page:  # another sequence's copy of this run: ours stays private
                break
            child.stamp = max(child.stamp, stamp)
            node = child
        return new

    def evict(self, count: int) -> List[int]:
        """Drop the ``count`` first reclaimable entries by (stamp, deeper first, page id) and return their
        pages (``PageTable.assign`` puts them on its free list).  An entry's descendants are reclaimable
        when it is and sort before it, so each entry is a leaf when its turn comes."""
        cand = heapq.nsmallest(count, (n for n in self._by_page.values() if self.pages.refcount(n.page) == 0),
                               key=lambda n: (n.stamp, -n.depth, n.page))
        if len(cand) < count or any(self.pages.refcount(c.page) for n in cand for c in n.children.values()):
            raise RuntimeError(f"prefix index: {count} reclaimable pages asked for, {len(cand)} evictable")
        for n in cand:
            del n.parent.children[n.key]
            del self._by_page[n.page]
        self.evictions += len(cand)
        return [n.page for n in cand]

    def clear(self) -> None:
        """Drop every entry; pages nobody holds return to the free list (pages in use stay with their
        sequences, now private).  The engine's failure / reset path calls this, and so must anything
        that replaces the model's weights."""
        pages = sorted(self._by_page, reverse=True)
        self._root.children.clear()
        self._by_page.clear()
        self.pages.unindexed(pages)

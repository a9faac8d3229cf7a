"""Speculative decoding: drafts and exact-match acceptance (pure Python, no model in here).

A sequence that has emitted ``e`` tokens, the last one ``x`` at position ``p``, proposes up to K draft
tokens ``d1 .. dK'`` and feeds ``[x, d1 .. dK']`` to one forward of K' + 1 positions
(``LlamaTP.verify_step``).  Row ``t`` of that forward has seen ``x, d1 .. dt`` -- if those drafts are what
the sequence would have produced anyway, row ``t``'s candidates are exactly the ones plain decoding
would get at generated-token index ``e + t``, so ``y[t] = pick_token(row t, gp, step=e + t)`` is the
token plain decoding emits there (same rule, same counter-based draw).  The sequence therefore emits
``y[0]``, then ``y[t]`` while ``d[t] == y[t-1]``: by construction the output is what non-speculative
decoding produces from the same candidates.  Cache rows of rejected drafts are stale but unreachable
(the sequence's length governs what attention reads) and the next step overwrites them.

``K' = min(K, max_new_tokens - e - 1)``: nothing is ever written past the rows plain decoding uses, so
the KV page accounting is unchanged.

Drafts come from a ``drafter(tokens, n_draft) -> List[int]`` hook; the default is prompt lookup
(:func:`prompt_lookup_draft`): no draft model, nothing to load.  Draft models, tree verification and
rejection sampling are out of scope.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional, Sequence

Drafter = Callable[[Sequence[int], int], List[int]]


def prompt_lookup_draft(tokens: Sequence[int], n_draft: int, max_ngram: int = 3, min_ngram: int = 1) -> List[int]:
    """Up to ``n_draft`` tokens that followed the most recent earlier occurrence of the sequence's last
    n-gram, the longest n in ``[min_ngram, max_ngram]`` that has one (with at least one token after
    it).  A shorter continuation is padded to ``n_draft`` with its last element, no match at all with
    the sequence's last token -- a padded draft is merely a guess, accepted only if it is right."""
    n_draft = int(n_draft)
    if n_draft <= 0:
        return []
    toks = list(tokens)
    L = len(toks)
    if L == 0:
        return [0] * n_draft
    found: List[int] = []
    for n in range(min(int(max_ngram), L - 1), max(1, int(min_ngram)) - 1, -1):
        tail = toks[L - n:]
        for i in range(L - n - 1, -1, -1):  # the most recent earlier occurrence: i + n <= L - 1
            if toks[i: i + n] == tail:
                found = toks[i + n: i + n + n_draft]
                break
        if found:
            break
    pad = found[-1] if found else toks[-1]
    return found + [pad] * (n_draft - len(found))


def make_prompt_lookup(max_ngram: int = 3, min_ngram: int = 1) -> Drafter:
    """The default drafter with its n-gram range fixed (MODEL_CONFIG ``speculate_ngram``)."""

    def draft(tokens: Sequence[int], n_draft: int) -> List[int]:
        return prompt_lookup_draft(tokens, n_draft, max_ngram=max_ngram, min_ngram=min_ngram)

    return draft


def spec_feed(tokens: Sequence[int], K: int, remaining: int, drafter: Optional[Drafter] = None) -> List[int]:
    """The verify step's input of one sequence: its last token and ``K' = min(K, remaining - 1)`` drafts
    (``remaining`` = tokens the sequence may still emit, >= 1).  A drafter that returns too few tokens is
    padded with its last one, too many are cut."""
    n = max(0, min(int(K), int(remaining) - 1))
    last = int(tokens[-1])
    if n == 0:
        return [last]
    d = [int(t) for t in (drafter or prompt_lookup_draft)(tokens, n)][:n]
    d += [d[-1] if d else last] * (n - len(d))
    return [last] + d


def accept(feed: Sequence[int], pick: Callable[[int], int], eos: Iterable[int] = ()) -> List[int]:
    """The tokens a verify step emits for one sequence.  ``feed = [x, d1 .. dK']``, ``pick(t)`` the token
    row ``t``'s candidates give (called for the rows that are reached only): ``y[0]``, then ``y[t]``
    while ``d[t] == y[t-1]``; stops after the first token in ``eos``."""
    eos = set(eos)
    out: List[int] = []
    for t in range(len(feed)):
        y = int(pick(t))
        out.append(y)
        if y in eos or t + 1 >= len(feed) or int(feed[t + 1]) != y:
            break
    return out

"""Speculative decoding on the client: draft K tokens, verify them in one step, keep what matches.

The last stage samples server-side with a seed derived from (session, position), so the token at
a position is a function of the logits, the history and the position alone.  A verify step
carries the last accepted token and K drafted ones; the last stage draws every row as a
one-token step would (``ops.sample_verify``) and returns the draws up to and including the first
that differs from its draft.  Exact-match acceptance therefore reproduces the plain loop's output
token for token, for greedy and for stochastic sampling; a wrong draft costs nothing but the rows.

``Drafter`` is the protocol, ``NgramDrafter`` (prompt lookup) the built-in one, and
``speculative_generate`` the accept loop, written against two callables so that the CLI client and
the tests drive the same code.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, List, Optional, Protocol, Sequence


class Drafter(Protocol):
    def propose(self, prompt_ids: Sequence[int], generated: Sequence[int], k: int) -> List[int]:
        """Up to ``k`` guesses of the tokens that follow prompt + generated ([] = no guess)."""


class NgramDrafter:
    """Prompt lookup: find the longest suffix of prompt + generated, up to ``max_ngram`` tokens, that
    occurred earlier in it, and propose the tokens that followed its most recent earlier occurrence."""

    def __init__(self, max_ngram: int = 3):
        self.max_ngram = int(max_ngram)

    def propose(self, prompt_ids: Sequence[int], generated: Sequence[int], k: int) -> List[int]:
        seq = list(prompt_ids) + list(generated)
        n_seq = len(seq)
        if k <= 0:
            return []
        for n in range(min(self.max_ngram, n_seq - 1), 0, -1):
            tail = seq[n_seq - n:]
            for i in range(n_seq - n - 1, -1, -1):  # the most recent earlier occurrence first
                if seq[i:i + n] == tail:
                    return seq[i + n:i + n + k]
        return []


DRAFTERS = {"ngram": NgramDrafter}


@dataclasses.dataclass
class SpecStats:
    steps: int = 0       # decode + verify steps sent
    verify_steps: int = 0
    drafted: int = 0     # drafted tokens sent
    accepted: int = 0    # drafted tokens the last stage confirmed
    tokens: int = 0      # tokens received from those steps

    def summary(self) -> str:
        rate = self.accepted / self.drafted if self.drafted else 0.0
        per = self.tokens / self.steps if self.steps else 0.0
        return (f"speculative: {self.steps} steps ({self.verify_steps} verify), drafted {self.drafted}, accepted "
                f"{self.accepted} ({100 * rate:.0f}%), {per:.2f} tokens/step")


def speculative_generate(first_token: int, prompt_ids: Sequence[int], max_new_tokens: int, k: int, drafter: Drafter,
                         decode_step: Callable[[int, int, List[int]], int],
                         verify_step: Callable[[List[int], int, List[int]], List[int]],
                         eos: Optional[int] = None, max_length: Optional[int] = None,
                         on_step: Optional[Callable[[int], None]] = None, log=None):
    """The decode loop of the CLI client with blocks of up to ``k`` drafted tokens per step.

    ``decode_step(token, cur_len, generated) -> token`` runs a plain one-token step;
    ``verify_step([token, d_1..d_K], cur_len, generated) -> [t_0..t_n]`` a verify step, where
    ``cur_len`` counts the session's tokens including all rows of the step.  Every returned token
    goes through the plain loop's stop rules (EOS, five consecutive repeats, ``max_new_tokens``),
    one by one, so the output equals the plain loop's.  Returns (generated, SpecStats)."""
    prompt_ids = list(prompt_ids)
    next_id = int(first_token)
    generated = [next_id]
    cur_len = len(prompt_ids) + 1
    repeat, last = 0, None
    stats = SpecStats()
    left = max_new_tokens - 1  # tokens the plain loop would still ask for
    done = False
    while left > 0 and not done:
        if eos is not None and next_id == eos:
            if log:
                log.info("EOS token generated, stopping generation")
            break
        kk = min(int(k), left - 1)
        if max_length is not None:
            kk = min(kk, int(max_length) - cur_len)
        drafts = [int(t) for t in drafter.propose(prompt_ids, generated, kk)][:max(kk, 0)] if kk > 0 else []
        if on_step:
            on_step(stats.steps)
        if drafts:
            toks = [int(t) for t in verify_step([next_id] + drafts, cur_len + len(drafts), generated)]
            stats.verify_steps += 1
            stats.drafted += len(drafts)
            stats.accepted += len(toks) - 1
        else:
            toks = [int(decode_step(next_id, cur_len, generated))]
        stats.steps += 1
        stats.tokens += len(toks)
        for t in toks:
            next_id = t
            left -= 1
            if eos is not None and next_id == eos:
                if log:
                    log.info("EOS token generated, stopping generation")
                done = True
                break
            if next_id == last:
                repeat += 1
                if repeat >= 5:
                    if log:
                        log.warning(f"Consecutive repetition detected (token {next_id}), stopping generation")
                    done = True
                    break
            else:
                repeat, last = 0, next_id
            generated.append(next_id)
            cur_len += 1
            if left <= 0:
                break
    return generated, stats

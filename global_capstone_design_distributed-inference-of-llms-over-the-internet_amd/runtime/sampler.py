"""Batched server-side sampling (the last stage samples; only token ids leave it).

Reference: ``StageConnectionHandler._sample_token`` samples one row per request in
Python (reference src/rpc_handler.py:327-403) with defaults temperature 0.8 / top_p 0.9 /
top_k 0 in the handler (:71-73) and repetition penalty 1.5 (:164); the CLI sends
temperature 1.0 / top_p 0.92 / top_k 50 (src/main.py:806-809).  Here all rows of a step are
sampled by one HIP kernel launch with per-row parameters (``ops.sample``).
"""
from __future__ import annotations

import dataclasses
import hashlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops

RECENT = 50  # reference: generated_tokens[-50:] (src/rpc_handler.py:348; src/rpc_transport.py:797)


@dataclasses.dataclass
class SamplingParams:
    temperature: float = 0.8
    top_p: float = 0.9
    top_k: int = 0
    repetition_penalty: float = 1.5

    @classmethod
    def from_metadata(cls, md: dict) -> "SamplingParams":
        return cls(float(md.get("temperature", 0.8)), float(md.get("top_p", 0.9)), int(md.get("top_k", 0)),
                   float(md.get("repetition_penalty", 1.5)))


def session_seed(session_id: str, step: int, base_seed: int = 0) -> int:
    h = hashlib.blake2b(f"{base_seed}:{session_id}:{step}".encode(), digest_size=8).digest()
    return int.from_bytes(h, "little") & 0x7FFFFFFFFFFFFFFF


class BatchSampler:
    def __init__(self, device, max_rows: int = 256):
        self.device = torch.device(device)
        self.max_rows = max_rows
        pin = self.device.type == "cuda"
        self._f = torch.empty(3, max_rows, dtype=torch.float32, pin_memory=pin)
        self._i = torch.empty(2 + RECENT, max_rows, dtype=torch.int32, pin_memory=pin)
        self._s = torch.empty(max_rows, dtype=torch.int64, pin_memory=pin)
        self._ws: Optional[torch.Tensor] = None
        self._vws: Optional[torch.Tensor] = None  # workspace of ``verify``
        self._vi: Optional[torch.Tensor] = None   # pinned int32 staging of ``verify``

    def __call__(self, logits: torch.Tensor, params: Sequence[SamplingParams], histories: Sequence[Sequence[int]],
                 seeds: Sequence[int]) -> torch.Tensor:
        R, V = logits.shape
        assert R == len(params) == len(histories) == len(seeds)
        if R == 0:
            return torch.empty(0, dtype=torch.long, device=logits.device)
        if all(p.temperature <= 0 for p in params):
            return ops.argmax(logits)
        if R > self.max_rows:
            return torch.cat([self(logits[i:i + self.max_rows], params[i:i + self.max_rows],
                                   histories[i:i + self.max_rows], seeds[i:i + self.max_rows])
                              for i in range(0, R, self.max_rows)])
        f = self._f[:, :R].numpy()
        ii = self._i[:, :R].numpy()
        f[0] = [p.temperature for p in params]
        f[1] = [p.top_p for p in params]
        f[2] = [p.repetition_penalty for p in params]
        ii[0] = [p.top_k for p in params]
        rec = np.zeros((R, RECENT), dtype=np.int32)
        lens = np.zeros(R, dtype=np.int32)
        for r, h in enumerate(histories):
            h = list(h)[-RECENT:]
            lens[r] = len(h)
            if h:
                rec[r, : len(h)] = h
        ii[1] = lens
        self._s[:R].numpy()[:] = [int(s) & 0x7FFFFFFFFFFFFFFF for s in seeds]
        dev = logits.device
        fd = self._f[:, :R].to(dev, non_blocking=True)
        idv = self._i[:2, :R].to(dev, non_blocking=True)
        recent = torch.from_numpy(rec).to(dev, non_blocking=False)
        seeds_d = self._s[:R].to(dev, non_blocking=True)
        if dev.type == "cuda":
            if self._ws is None or self._ws.numel() < R * V:
                self._ws = torch.empty(self.max_rows * V, dtype=torch.float32, device=dev)
            ws = self._ws
        else:
            ws = None
        out = ops.sample(logits, fd[0].contiguous(), fd[1].contiguous(), idv[0].contiguous(), fd[2].contiguous(),
                         recent, idv[1].contiguous(), seeds_d, workspace=ws)
        if dev.type == "cuda":
            torch.cuda.current_stream().synchronize()  # pinned staging is reused by the next call
        return out

    def verify(self, logits: torch.Tensor, drafts: Sequence[Sequence[int]], params: Sequence[SamplingParams],
               histories: Sequence[Sequence[int]], seeds: Sequence[Sequence[int]]) -> List[List[int]]:
        """Speculative verify of one step (``ops.sample_verify``).  Session s owns the next
        ``len(drafts[s]) + 1`` rows of ``logits``: the row of its last accepted token, then one per
        drafted token; ``seeds[s]`` has one seed per row.  Returns, per session, the tokens it keeps:
        the draws that equal their draft, and the first one that does not (or the bonus token after
        the last draft).  A session without drafts gets what ``__call__`` gives it."""
        S = len(drafts)
        assert S == len(params) == len(histories) == len(seeds)
        nrow = [len(d) + 1 for d in drafts]
        R, V = logits.shape
        assert R == sum(nrow) and all(len(sd) == n for sd, n in zip(seeds, nrow))
        if S == 0:
            return []
        if S > self.max_rows or R > self.max_rows:
            raise ValueError(f"verify step of {S} sessions / {R} rows exceeds the sampler's {self.max_rows} rows")
        dev = logits.device
        # staged like ``__call__``: pinned buffers, one copy each for the floats, the int32s and the seeds.
        # int32 layout: row_start [S + 1] | draft [R] | top_k [S] | recent_len [S] | recent [S, RECENT]
        if self._vi is None:
            pin = self.device.type == "cuda"
            n = self.max_rows
            self._vi = torch.empty((n + 1) + n + 2 * n + n * RECENT, dtype=torch.int32, pin_memory=pin)
        o_draft, o_k, o_len, o_rec = S + 1, S + 1 + R, 2 * S + 1 + R, 3 * S + 1 + R
        n_int = o_rec + S * RECENT
        ii = self._vi[:n_int].numpy()
        ii[0] = 0
        ii[1:S + 1] = np.cumsum(nrow)
        row_start = ii[:S + 1]
        ii[o_draft:o_k] = -1
        for s, d in enumerate(drafts):
            if len(d):
                ii[o_draft + row_start[s]:o_draft + row_start[s] + len(d)] = d
        ii[o_k:o_len] = [p.top_k for p in params]
        rec = ii[o_rec:n_int].reshape(S, RECENT)
        rec[:] = 0
        for s, h in enumerate(histories):
            h = list(h)[-RECENT:]
            ii[o_len + s] = len(h)
            if h:
                rec[s, :len(h)] = h
        f = self._f[:, :S].numpy()
        f[0] = [p.temperature for p in params]
        f[1] = [p.top_p for p in params]
        f[2] = [p.repetition_penalty for p in params]
        self._s[:R].numpy()[:] = [int(v) & 0x7FFFFFFFFFFFFFFF for row in seeds for v in row]
        fd = self._f[:, :S].to(dev, non_blocking=True)
        idv = self._vi[:n_int].to(dev, non_blocking=True)
        seeds_d = self._s[:R].to(dev, non_blocking=True)
        ws = None
        if dev.type == "cuda":
            need = ops.sample_verify_workspace(R, V, RECENT)
            if self._vws is None or self._vws.numel() < need:
                self._vws = torch.empty(need, dtype=torch.float32, device=dev)
            ws = self._vws
        toks, cnt = ops.sample_verify(
            logits, idv[:o_draft], idv[o_draft:o_k], fd[0].contiguous(), fd[1].contiguous(), idv[o_k:o_len],
            fd[2].contiguous(), idv[o_rec:].view(S, RECENT), idv[o_len:o_rec], seeds_d, workspace=ws,
            all_greedy=all(p.temperature <= 0 for p in params))
        row_start = [int(v) for v in row_start]  # (the pinned staging is reused by the next call)
        toks, cnt = toks.tolist(), cnt.tolist()
        return [toks[row_start[s]:row_start[s] + int(cnt[s])] for s in range(S)]

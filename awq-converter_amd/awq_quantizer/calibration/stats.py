"""Running activation statistics of one linear input (include/awq_hip.h awq_act_stats_accum).

The C contract wants whole 256-token blocks from every call on an accumulator but the last, so
that the canonical summation order continues across calls.  StatsAccumulator takes chunks of any
row count: whole blocks go to the kernel straight from the caller's (possibly row-strided) view,
a remainder of fewer than 256 rows is copied into a carry buffer and leads the next call.  The
result is the bits of awq_act_stats on the concatenated rows, whatever the chunking.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _hip

BLOCK = _hip.ACT_ROW_BLOCK


class StatsAccumulator:
    def __init__(self, K: int, device):
        self.K = int(K)
        self.device = torch.device(device)
        _hip.require_device(self.device)
        self.acc_abs = torch.zeros(self.K, dtype=torch.float64, device=self.device)
        self.acc_sq = torch.zeros(self.K, dtype=torch.float64, device=self.device)
        self.tokens = 0                       # rows already in the sums: a multiple of 256 until finish()
        self._carry: Optional[torch.Tensor] = None
        self._n_carry = 0
        self._done = False

    # the fused producers (awq_rmsnorm_stats / awq_swiglu_stats) add to the sums themselves
    def fusable(self) -> bool:
        """True while a kernel may add rows directly: no rows are waiting in the carry buffer."""
        return self._n_carry == 0 and self.tokens % BLOCK == 0 and not self._done

    def added(self, rows: int) -> None:
        """Bookkeeping after a fused producer added `rows` rows at tokens_before = self.tokens."""
        self.tokens += int(rows)

    def _accum(self, x: torch.Tensor) -> None:
        _hip.act_stats_accum(x, self.tokens, self.acc_abs, self.acc_sq)
        self.tokens += x.shape[0]

    def add(self, x: torch.Tensor) -> None:
        if self._done:
            raise RuntimeError("StatsAccumulator.add after finish()")
        if x.dim() != 2 or x.shape[1] != self.K:
            raise ValueError(f"StatsAccumulator({self.K}).add takes [rows, {self.K}], got {tuple(x.shape)}")
        if self.tokens % BLOCK:
            raise RuntimeError("a fused producer added a partial block: it was this accumulator's last call")
        if x.shape[0] == 0:
            return
        if self._carry is None:
            self._carry = torch.empty((BLOCK, self.K), dtype=x.dtype, device=self.device)
        elif x.dtype != self._carry.dtype:
            raise ValueError(f"StatsAccumulator: chunks of {self._carry.dtype} and {x.dtype}")
        if self._n_carry:
            take = min(BLOCK - self._n_carry, x.shape[0])
            self._carry[self._n_carry:self._n_carry + take].copy_(x[:take])
            self._n_carry += take
            x = x[take:]
            if self._n_carry < BLOCK:
                return
            self._accum(self._carry)
            self._n_carry = 0
        whole = x.shape[0] // BLOCK * BLOCK
        if whole:
            self._accum(x[:whole])
        rest = x.shape[0] - whole
        if rest:
            self._carry[:rest].copy_(x[whole:])
            self._n_carry = rest

    def finish(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(x_mean, x_sq) fp32 [K] on the device."""
        if not self._done:
            if self._n_carry:
                self._accum(self._carry[:self._n_carry])
                self._n_carry = 0
            self._done = True
        if self.tokens == 0:
            raise ValueError("StatsAccumulator.finish: no rows were added")
        return _hip.column_mean(self.acc_abs, self.tokens), _hip.column_mean(self.acc_sq, self.tokens)

"""Device-side dedup, row expansion and gradient pre-sum of the sharded embedding
exchange's SENDER (``csrc/kernels/sparse_exchange.hip``).

``ShardedEmbedding(exchange="device")`` (``parallel/embedding.py``) replaces the
host ``torch.unique`` plan, ``index_select`` and the fp32 ``index_add_`` pre-sum
of a world > 1 lookup with these.  The functions need no process group:

* :func:`build_plan` — launches only: owner-major keys, radix sort, segment heads,
  a device-wide prefix sum, compaction (distinct local rows, inverse map, run
  bounds, per-owner counts, an out-of-range flag);
* :func:`expand_rows` — ``back[inv]``, bit-exact;
* :func:`presum_rows` — one bf16 row per distinct id, summed in fp32 in a fixed
  order (bitwise reproducible, unlike ``index_add_``'s atomics).

:meth:`ExchangePlan.split_sizes` is the one host wait of a lookup: ``2 world + 2``
integers copied to pinned memory, waited for on that copy's event.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ..ops import _lib

_P, _L, _I = _lib.P, _lib.L, _lib.I
_lib.register("kfa_xchg_ws_bytes", [_L], restype=_L)
_lib.register("kfa_xchg_part_floats", [_L, _I], restype=_L)
_lib.register("kfa_xchg_plan", [_P, _L, _I, _I, _L, _L, _P, _L, _P, _P, _P, _P, _P])
_lib.register("kfa_xchg_expand", [_P, _L, _P, _L, _I, _P, _P])
_lib.register("kfa_xchg_presum", [_P, _L, _I, _L, _P, _L, _P, _P, _P, _L, _P, _P])

MAX_N = 2 ** 31 - 1      # entries of one lookup (32-bit positions)
MAX_KEYS = 2 ** 32       # owners * rows_per_owner (32-bit keys)
MAX_DIM = 248            # the pre-sum's LDS tile: 64 rows of dim + 4 floats


def supported(n: int, dim: int, owners: int, rows_per_owner: int) -> bool:
    """The size limits of the kernels: 16-B row vectors, 32-bit keys and positions."""
    return n <= MAX_N and dim % 8 == 0 and 0 < dim <= MAX_DIM and owners * rows_per_owner <= MAX_KEYS


class ExchangePlan:
    """What one lookup's sender needs, all on the device: ``rows`` (int64, local row on
    its owner of each distinct id, owner-major), ``inv`` (int32 [n], index into ``rows``
    per lookup), ``seg_start`` (int32, bounds of each distinct id's run in the sorted
    order), ``meta`` (int32 ``[counts | peer counts | U | error flag]``) and the sort's
    workspace (sorted keys and positions, read again by the pre-sum).  ``rows`` /
    ``seg_start`` are sized for n distinct ids; :attr:`U` (known after
    :meth:`split_sizes` or a :meth:`finish`) says how many are valid."""

    def __init__(self, n: int, world: int, owners: int, rows_per_owner: int, num_rows: int, device):
        self.n, self.world, self.owners, self.rows_per_owner, self.num_rows = n, world, owners, rows_per_owner, num_rows
        self.device = device
        self.rows_buf = torch.empty(n, dtype=torch.int64, device=device)
        self.inv = torch.empty(n, dtype=torch.int32, device=device)
        self.seg_start = torch.empty(n + 1 if n else 0, dtype=torch.int32, device=device)
        self.meta = torch.zeros(2 * world + 2, dtype=torch.int32, device=device) if n == 0 else \
            torch.empty(2 * world + 2, dtype=torch.int32, device=device)
        self.ws: Optional[torch.Tensor] = None
        self._host: Optional[torch.Tensor] = None
        self._U: Optional[int] = 0 if n == 0 else None

    # ------------------------------------------------------------------ host view
    def _fetch(self) -> torch.Tensor:
        """``meta`` on the host: one small copy to pinned memory, waited for on its own event."""
        if self._host is None:
            host = torch.empty(self.meta.numel(), dtype=torch.int32, pin_memory=True)
            host.copy_(self.meta, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            ev.synchronize()
            self._host = host
            self._U = int(host[2 * self.world])
        return self._host

    def _check(self, host: torch.Tensor) -> None:
        if int(host[2 * self.world + 1]):
            raise IndexError(f"ShardedEmbedding: lookup ids outside the valid range [0, {self.num_rows})")

    def finish(self) -> "ExchangePlan":
        """Read U and the error flag without a peer exchange (single-process use)."""
        self._check(self._fetch())
        return self

    @property
    def U(self) -> int:
        if self._U is None:
            self._fetch()
        return self._U

    @property
    def rows(self) -> torch.Tensor:
        return self.rows_buf[:self.U]

    @property
    def counts(self) -> torch.Tensor:
        return self.meta[:self.world]

    def split_sizes(self, comm=None, pg=None) -> Tuple[List[int], List[int]]:
        """(send counts, receive counts) of the id all-to-all: this rank's per-owner counts
        go to the peers in one small all-to-all of device tensors on the table's
        communicator, then ``[send | recv | U | flag]`` comes to the host in one copy.
        Raises ``IndexError`` when an id was outside ``[0, num_rows)``."""
        W = self.world
        if self._host is None and W > 1 and (comm is not None or pg is not None or _dist_world() == W):
            from .embedding import _a2a
            _a2a(self.meta[W:2 * W], self.meta[:W], [1] * W, [1] * W, pg, comm)
        host = self._fetch()
        self._check(host)
        vals = host.tolist()
        return vals[:W], vals[W:2 * W]


def _dist_world() -> int:
    """Ranks of the default process group (0 without one: a single process planning for a
    layout of several ranks has no peers to tell)."""
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 0


def build_plan(ids: torch.Tensor, world: int, owners: int, rows_per_owner: int, num_rows: int) -> ExchangePlan:
    """Plan the exchange of a lookup of ``ids`` (contiguous int64, on the GPU) on a table of
    ``num_rows`` rows interleaved over ``owners`` of ``world`` ranks.  Launches only."""
    ids = ids.reshape(-1)
    n = ids.numel()
    if not (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()):
        raise ValueError("build_plan: ids must be a contiguous int64 tensor on the GPU")
    if n > MAX_N or owners * rows_per_owner > MAX_KEYS or not (1 <= owners <= world) or \
            num_rows > owners * rows_per_owner:
        raise ValueError(f"build_plan: {n} ids, {owners} owners x {rows_per_owner} rows of {world} ranks: "
                         f"outside the kernels' limits")
    plan = ExchangePlan(n, world, owners, rows_per_owner, num_rows, ids.device)
    if n == 0:
        return plan
    plan.ws = torch.empty(_lib.lib().kfa_xchg_ws_bytes(n), dtype=torch.uint8, device=ids.device)
    _lib.call("kfa_xchg_plan", _lib.ptr(ids), n, world, owners, rows_per_owner, num_rows, _lib.ptr(plan.ws),
              plan.ws.numel(), _lib.ptr(plan.rows_buf), _lib.ptr(plan.inv), _lib.ptr(plan.seg_start),
              _lib.ptr(plan.meta), _lib.stream())
    return plan


def expand_rows(back: torch.Tensor, plan: ExchangePlan) -> torch.Tensor:
    """``back[plan.inv]``: the distinct rows the owners returned, one per lookup (bf16)."""
    D = back.shape[1]
    if not (back.is_cuda and back.dtype == torch.bfloat16 and back.is_contiguous() and back.dim() == 2
            and D % 8 == 0 and back.data_ptr() % 16 == 0):
        raise ValueError(f"expand_rows: expected contiguous bf16 [U, 8k] rows, got {back.dtype} {tuple(back.shape)}")
    if plan.n and back.shape[0] < plan.U:
        raise ValueError(f"expand_rows: {back.shape[0]} rows for {plan.U} distinct ids")
    out = torch.empty(plan.n, D, dtype=back.dtype, device=back.device)
    if plan.n:
        _lib.call("kfa_xchg_expand", _lib.ptr(back), back.shape[0], _lib.ptr(plan.inv), plan.n, D, _lib.ptr(out),
                  _lib.stream())
    return out


def presum_rows(dout: torch.Tensor, plan: ExchangePlan) -> torch.Tensor:
    """bf16 ``[U, D]``: the fp32 sum of ``dout``'s rows per distinct id, rounded once."""
    D = dout.shape[1]
    if not (dout.is_cuda and dout.dtype == torch.bfloat16 and dout.is_contiguous() and dout.dim() == 2
            and dout.shape[0] == plan.n and D % 8 == 0 and D <= MAX_DIM and dout.data_ptr() % 16 == 0):
        raise ValueError(f"presum_rows: expected contiguous bf16 [{plan.n}, 8k <= {MAX_DIM}], got {dout.dtype} "
                         f"{tuple(dout.shape)}")
    U = plan.U
    out = torch.empty(U, D, dtype=torch.bfloat16, device=dout.device)
    if plan.n:
        nf = _lib.lib().kfa_xchg_part_floats(plan.n, D)
        part = _lib.workspace(nf * 4, dout.device, "xchg_presum_part").view(torch.float32)
        _lib.call("kfa_xchg_presum", _lib.ptr(dout), plan.n, D, U, _lib.ptr(plan.ws), plan.ws.numel(),
                  _lib.ptr(plan.inv), _lib.ptr(plan.seg_start), _lib.ptr(part), nf, _lib.ptr(out), _lib.stream())
    return out

"""Fused SGD(+momentum, weight decay, nesterov), Adam/AdamW, LAMB and LARS over flat
parameter groups, and global-norm gradient clipping for the latter three —
``csrc/kernels/optim.hip``.

One kernel launch per optimizer space per step (LAMB and LARS: two passes and one
small launch for their per-tensor trust ratios; clipping: one more read of the
gradient, which LARS shares with its norms pass, every norm and coefficient kept on
the device); the gradient average over data-parallel ranks (``1/world``) and any
loss scale are folded into ``grad_scale`` so no separate scaling pass runs.  A
space is a whole flat group
or the compact parameter-server / ZeRO shard a rank owns (``parallel/ps.py``):
the optimizer state is allocated at the space's size, so an owner holds state
only for what it owns.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ..parallel.flat import FlatGroup

P, L, I, F = _lib.P, _lib.L, _lib.I, _lib.F
_lib.register("kfa_sgd_step", [P, P, P, I, P, L, F, F, F, F, I, F, I, P])
_lib.register("kfa_adam_step", [P, P, P, I, P, P, L, F, F, F, F, F, F, F, F, P, P])
_lib.register("kfa_adam_bc", [P, P, F, F, I, P])
_lib.register("kfa_f32_to_bf16", [P, P, L, P])
_lib.register("kfa_adam_step_clip", [P, P, P, I, P, P, L, F, F, F, F, F, F, P, P, P])
_lib.register("kfa_chunk_sumsq", [P, I, P, I, P, P])
_lib.register("kfa_clip_finish", [P, I, F, F, P, P])
_lib.register("kfa_lamb_stage1", [P, P, I, P, P, P, I, P, F, F, F, F, F, P, P, P])
_lib.register("kfa_lamb_ratio", [P, P, I, P, P])
_lib.register("kfa_lamb_stage2", [P, P, P, P, P, I, P, F, F, F, P, P])
_lib.register("kfa_lars_norms", [P, P, I, P, I, P, P, P])
_lib.register("kfa_lars_ratio", [P, P, P, I, P, F, P, F, F, F, P])
_lib.register("kfa_lars_apply", [P, P, P, I, P, P, I, P, F, F, F, I, F, P, P])

# elements per chunk of the fixed-order segmented reductions (LAMB norms, the clip norm):
# one block reduces one chunk, 8 vectors of 8 elements per lane (kfa_chunk_sumsq: <= 65536)
CHUNK = 16384


class OptSpace:
    """One contiguous region a fused optimizer updates in ONE launch: fp32
    weights ``w`` (updated in place), an optional low-precision compute copy
    ``wb`` rewritten from ``w`` in the same kernel, and the gradient ``grad``
    (bf16 or fp32).  A whole flat group (data-parallel all-reduce) or one
    rank's compact shard of it (parameter-server / ZeRO owner, ``parallel/ps.py``).

    ``segments``: the ``(start, numel)`` of every tensor in the region, for the
    per-tensor norms of LAMB; ``None`` for the compact shards, whose cuts do not
    follow tensor boundaries."""

    __slots__ = ("name", "w", "wb", "_grad", "segments")

    def __init__(self, name: str, w: torch.Tensor, wb: Optional[torch.Tensor], grad,
                 segments: Optional[Sequence[Tuple[int, int]]] = None):
        self.name = name
        self.w = w
        self.wb = wb
        self._grad = grad
        self.segments = [(int(a), int(n)) for a, n in segments] if segments is not None else None

    @classmethod
    def of_group(cls, g: FlatGroup) -> "OptSpace":
        return cls(g.name, g.fp32, g.data if g.master is not None else None, lambda: g.opt_grad,
                   segments=[(o, p.numel()) for o, p in zip(g.offsets, g.params)])

    @property
    def grad(self) -> torch.Tensor:
        return self._grad() if callable(self._grad) else self._grad

    @property
    def numel(self) -> int:
        return self.w.numel()

    @property
    def device(self) -> torch.device:
        return self.w.device


def _as_spaces(items) -> List[OptSpace]:
    return [x if isinstance(x, OptSpace) else OptSpace.of_group(x) for x in items]


class _ChunkTable:
    """The chunks of one space's tensors for the segmented reductions: ``chunks``
    holds a row ``(tensor id, start, length)`` per chunk, a chunk never crossing a
    tensor boundary, and ``tens`` a row ``(first chunk, chunk count)`` per tensor;
    both int64, built once and kept on the space's device.  A space without
    ``segments`` is one tensor.  The kernels load whole 8-element vectors, so
    every segment must start on a multiple of 8 and leave the padding up to the
    next multiple of 8 inside the buffer and outside every other segment."""

    def __init__(self, s: OptSpace):
        segs = s.segments if s.segments is not None else [(0, s.numel)]
        rows, tens, end = [], [], 0
        for t, (a, n) in enumerate(segs):
            if a % 8 or n < 0 or a < end or -(-(a + n) // 8) * 8 > s.numel:
                raise ValueError(f"optimizer space {s.name!r}: segment {t} = ({a}, {n}) is not an 8-aligned, "
                                 f"ordered, padded cut of its {s.numel} elements")
            end = a + n
            first = len(rows)
            rows += [(t, a + o, min(CHUNK, n - o)) for o in range(0, n, CHUNK)]
            tens.append((first, len(rows) - first))
        self.nchunks, self.ntens = len(rows), len(tens)
        self.chunks = torch.tensor(rows, dtype=torch.int64, device=s.device).reshape(-1, 3)
        self.tens = torch.tensor(tens, dtype=torch.int64, device=s.device).reshape(-1, 2)


# The trainers' rules, once: WHOLE_GRAD take per-tensor norms and max_grad_norm a global one, so every
# rank must hold the whole gradient (all-reduce layout); CLIPS are the optimizers that take max_grad_norm.
WHOLE_GRAD = ("lamb", "lars")
CLIPS = ("adam", "adamw", "lamb", "lars")


def needs_whole_grad(optimizer: str, max_grad_norm: Optional[float]) -> bool:
    return optimizer in WHOLE_GRAD or max_grad_norm is not None


def _garg(g: torch.Tensor) -> Tuple[int, int]:
    """A gradient as the kernels take it: (device address, is_bf16)."""
    return g.data_ptr(), int(g.dtype == torch.bfloat16)


class _FusedBase:
    """The spaces, their one device (``_gpu``: the kernels run, else the CPU arithmetic), the chunk
    tables and the clip scalar.  ``g2_partials``: the subclass reads ``_gpart`` itself, clipping or not."""

    def __init__(self, spaces: Sequence, lr: float, weight_decay: float,
                 decay_groups: Optional[Sequence[str]] = None, max_grad_norm: Optional[float] = None,
                 g2_partials: bool = False):
        self.spaces: List[OptSpace] = _as_spaces(spaces)
        self.device = self.spaces[0].device if self.spaces else torch.device("cpu")
        self._gpu = self.device.type == "cuda"
        self.lr = lr
        self.weight_decay = weight_decay
        self.decay_groups = set(decay_groups) if decay_groups is not None else {"weights"}
        self.step_count = 0
        self._tabs: Optional[List[_ChunkTable]] = None
        # LAMB / LARS: per space, the per-chunk partial sums and the per-tensor trust ratios
        self._part: List[Optional[torch.Tensor]] = []
        self._ratio: List[Optional[torch.Tensor]] = []
        # global-norm clipping: (pre-clip norm, coefficient) stay on the device; the step
        # kernels read the coefficient there, so no step waits for the host
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._clip: Optional[torch.Tensor] = None
        if self.max_grad_norm is not None:
            if not self.max_grad_norm > 0:
                raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm!r}")
            self._clip = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.device)
        self._dcoef = self._clip.data_ptr() + 4 if self._clip is not None else None  # the coefficient's address
        # GPU: one g^2 partial per chunk, every space's in one buffer, each space's chunks contiguous
        self._gpart: Optional[torch.Tensor] = None
        self._gaddr: List[int] = []  # per space, the device address of its partials in _gpart
        if self._gpu and (self._clip is not None or g2_partials):
            counts = [t.nchunks for t in self._tables()]
            self._gpart = torch.zeros(sum(counts), dtype=torch.float32, device=self.device)
            self._gaddr = [self._gpart.data_ptr() + 4 * sum(counts[:si]) for si in range(len(counts))]

    def _wd(self, s: OptSpace) -> float:
        return self.weight_decay if s.name in self.decay_groups or not s.name else 0.0

    def _tables(self) -> List[_ChunkTable]:
        if self._tabs is None:
            self._tabs = [_ChunkTable(s) for s in self.spaces]
        return self._tabs

    def scratch_bytes(self) -> int:
        """Bytes of the norm reductions' tables and partial sums: per chunk and per
        tensor, never per element (0 without LAMB, LARS or clipping)."""
        bufs = [self._clip, self._gpart, *self._part, *self._ratio]
        for t in self._tabs or []:
            bufs += [t.chunks, t.tens]
        return sum(b.numel() * b.element_size() for b in bufs if b is not None)

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """The gradient's global L2 norm before clipping, as of the last step: a 0-d
        tensor on the optimizer's device (``None`` without ``max_grad_norm``).  For
        logging: reading it waits for the device, so the caller decides when."""
        return self._clip[0] if self._clip is not None else None

    def _g2_partials(self, si: int, stream: int) -> None:
        """GPU: leave the per-chunk sums of g^2 of space ``si`` at ``_gaddr[si]``."""
        t = self._tabs[si]
        _lib.call("kfa_chunk_sumsq", *_garg(self.spaces[si].grad), _lib.ptr(t.chunks), t.nchunks, self._gaddr[si],
                  stream)

    @torch.no_grad()
    def _clip_scalar(self, grad_scale: float, stream: Optional[int] = None) -> None:
        """norm = grad_scale * |g| over every space and coef = min(1, max / (norm + 1e-6))
        (``torch.nn.utils.clip_grad_norm_``) into ``_clip``, in a fixed summation order."""
        if self._gpu:
            stream = _lib.stream() if stream is None else stream
            for si in range(len(self.spaces)):
                self._g2_partials(si, stream)
            _lib.call("kfa_clip_finish", _lib.ptr(self._gpart), self._gpart.numel(), grad_scale, self.max_grad_norm,
                      _lib.ptr(self._clip), stream)
            return
        total = torch.zeros((), dtype=torch.float32)
        for s in self.spaces:
            g = s.grad
            for a, n in (s.segments if s.segments is not None else [(0, s.numel)]):
                total += g[a:a + n].float().pow(2).sum()
        norm = total.sqrt() * grad_scale
        self._clip[0] = norm
        self._clip[1] = (self.max_grad_norm / (norm + 1e-6)).clamp(max=1.0)

    def _cpu_grad(self, g: torch.Tensor, grad_scale: float) -> torch.Tensor:
        """The CPU paths' gradient slice in fp32: scaled, and clipped by the coefficient of ``_clip``."""
        d = g.float() * grad_scale
        return d * self._clip[1] if self._clip is not None else d

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        """The whole step of an elementwise optimizer (SGD, Adam): every space as one range."""
        self.begin_step()
        if self._clip is not None:
            self._clip_scalar(grad_scale)
        for si, s in enumerate(self.spaces):
            self.update(si, 0, s.numel, grad_scale, lr)


class FusedSGD(_FusedBase):
    def __init__(self, groups, lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
                 decay_groups=None, max_grad_norm=None):
        if max_grad_norm is not None:
            raise ValueError("FusedSGD: global-norm gradient clipping (max_grad_norm) is not built for SGD; "
                             "use FusedAdam or FusedLAMB")
        super().__init__(groups, lr, weight_decay, decay_groups)
        self.momentum = momentum
        self.dampening = dampening
        self.nesterov = nesterov
        self.mom = [torch.zeros(s.numel, dtype=torch.float32, device=s.device) if momentum else None
                    for s in self.spaces]
        self._first = 1  # set per step by begin_step

    def begin_step(self) -> None:
        """Open one optimizer step whose updates are issued per range (``update``)."""
        self._first = int(self.step_count == 0)
        self.step_count += 1

    @torch.no_grad()
    def update(self, si: int, a: int, b: int, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        """Elements [a, b) of space ``si`` in the step opened by ``begin_step`` (the
        update is elementwise, so any cut of a space into ranges gives the whole-space result)."""
        if b <= a:
            return
        lr = self.lr if lr is None else lr
        s, mom = self.spaces[si], self.mom[si]
        w, wb, gr = s.w[a:b], (s.wb[a:b] if s.wb is not None else None), s.grad[a:b]
        mom = mom[a:b] if mom is not None else None
        if not self._gpu:
            d = gr.float() * grad_scale + self._wd(s) * w
            if mom is not None:
                if self._first:
                    mom.copy_(d)
                else:
                    mom.mul_(self.momentum).add_(d, alpha=1 - self.dampening)
                d = d + self.momentum * mom if self.nesterov else mom
            w.add_(d, alpha=-lr)
            if wb is not None:
                wb.copy_(w)
            return
        _lib.call("kfa_sgd_step", _lib.ptr(w), _lib.ptr(wb), *_garg(gr), _lib.ptr(mom), b - a, lr, self.momentum,
                  self.dampening, self._wd(s), int(self.nesterov), grad_scale, self._first, _lib.stream())

class _AdamMoments(_FusedBase):
    """The state Adam and LAMB share: the moments ``m`` / ``v`` (the names
    ``trainer/checkpoint.py`` saves) and the device step count / bias corrections."""

    def __init__(self, groups, lr, betas, eps, weight_decay, decay_groups, max_grad_norm):
        super().__init__(groups, lr, weight_decay, decay_groups, max_grad_norm)
        self.b1, self.b2 = betas
        self.eps = eps
        self.m = [torch.zeros(s.numel, dtype=torch.float32, device=s.device) for s in self.spaces]
        self.v = [torch.zeros(s.numel, dtype=torch.float32, device=s.device) for s in self.spaces]
        # GPU: the step count t and (1 - b1^t, 1 - b2^t) live on the device, advanced
        # by kfa_adam_bc inside the step, so the step replays from a HIP graph
        self._t = torch.zeros(1, dtype=torch.int32, device=self.device) if self._gpu else None
        self._bc = torch.ones(2, dtype=torch.float32, device=self.device) if self._gpu else None

    def begin_step(self) -> None:
        """Open one optimizer step whose updates are issued per range (``update``):
        the step count and the bias corrections advance once, here."""
        if self._gpu:
            # eager steps (and resumes) re-seed the device count inside the same launch; a
            # captured step advances it on the device (graph replay)
            seed = -1 if torch.cuda.is_current_stream_capturing() else self.step_count
            _lib.call("kfa_adam_bc", _lib.ptr(self._t), _lib.ptr(self._bc), self.b1, self.b2, seed, _lib.stream())
        self.step_count += 1


class FusedAdam(_AdamMoments):
    """``max_grad_norm``: clip the gradient to that global L2 norm first, as
    ``torch.nn.utils.clip_grad_norm_`` does.  ``step`` computes the coefficient on
    the device and the update kernel reads it there; the ranged ``update`` applies
    the coefficient of the last ``step``, so a clipped optimizer is stepped whole."""

    def __init__(self, groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay_groups=None,
                 max_grad_norm=None):
        super().__init__(groups, lr, betas, eps, weight_decay, decay_groups, max_grad_norm)

    @torch.no_grad()
    def update(self, si: int, a: int, b: int, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        """Elements [a, b) of space ``si`` in the step opened by ``begin_step`` (elementwise:
        any cut of a space into ranges gives the whole-space result bit for bit)."""
        if b <= a:
            return
        lr = self.lr if lr is None else lr
        t = self.step_count
        bc1 = 1.0 - self.b1 ** t
        bc2 = 1.0 - self.b2 ** t
        s = self.spaces[si]
        w, wb, gr = s.w[a:b], (s.wb[a:b] if s.wb is not None else None), s.grad[a:b]
        m, v = self.m[si][a:b], self.v[si][a:b]
        wd = self._wd(s)
        if not self._gpu:
            d = self._cpu_grad(gr, grad_scale)
            m.mul_(self.b1).add_(d, alpha=1 - self.b1)
            v.mul_(self.b2).addcmul_(d, d, value=1 - self.b2)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(self.eps)
            w.mul_(1 - lr * wd).addcdiv_(m, denom, value=-lr / bc1)
            if wb is not None:
                wb.copy_(w)
            return
        if self._clip is not None:
            _lib.call("kfa_adam_step_clip", _lib.ptr(w), _lib.ptr(wb), *_garg(gr), _lib.ptr(m), _lib.ptr(v), b - a, lr,
                      self.b1, self.b2, self.eps, wd, grad_scale, _lib.ptr(self._bc), self._dcoef, _lib.stream())
            return
        _lib.call("kfa_adam_step", _lib.ptr(w), _lib.ptr(wb), *_garg(gr), _lib.ptr(m), _lib.ptr(v), b - a, lr,
                  self.b1, self.b2, self.eps, wd, bc1, bc2, grad_scale, _lib.ptr(self._bc), _lib.stream())

class _TrustRatios:
    """What LAMB and LARS share, mixed in ahead of their state class: per adapting space
    (``adapt_groups``) ``_ratio`` holds an entry per tensor and, on the GPU, ``_part`` ``PARTS`` partial
    sums per chunk; both are ``None`` for a space that does not adapt.  The ratios are norms of whole
    tensors, so a space without ``segments`` is refused."""

    PARTS = 1

    def __init__(self, spaces, *args, adapt_groups=None, **kw):
        name = type(self).__name__
        for s in _as_spaces(spaces):
            if s.segments is None:
                raise ValueError(f"{name}: optimizer space {s.name!r} has no per-tensor segments "
                                 f"(a sharded layout); {name[len('Fused'):]} needs whole tensors for its trust ratios")
        super().__init__(spaces, *args, **kw)
        self.adapt_groups = set(adapt_groups) if adapt_groups is not None else set(self.decay_groups)
        self._ratio = [torch.ones(len(s.segments), dtype=torch.float32, device=s.device) if self._adapts(s) else None
                       for s in self.spaces]
        if self._gpu:
            self._part = [torch.zeros(self.PARTS * t.nchunks, dtype=torch.float32, device=s.device)
                          if self._adapts(s) else None for s, t in zip(self.spaces, self._tables())]

    def _adapts(self, s: OptSpace) -> bool:
        return s.name in self.adapt_groups or not s.name

    @property
    def trust_ratios(self) -> List[Optional[torch.Tensor]]:
        """Per space, the trust ratios of the last step: one tensor on the space's
        device with an entry per tensor, or ``None`` for a space that does not adapt.
        For logging: the step writes them, nothing may write them from outside."""
        return list(self._ratio)


class FusedLAMB(_TrustRatios, _AdamMoments):
    """LAMB (You et al., 2020): Adam's moments, and per tensor ``t`` of a space

        u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * w
        w -= lr * r_t * u,   r_t = |w_t| / |u_t|  (1 when either norm is 0)

    with the trust ratio ``r_t`` on the spaces named in ``adapt_groups`` (default:
    the decay groups, i.e. ``"weights"``) and 1 elsewhere.  Two passes over a
    space and no per-element state beyond ``m`` and ``v``: stage 1 updates the
    moments and leaves per-chunk partial sums of ``w^2`` and ``u^2``, one small
    launch turns them into the ratios, stage 2 recomputes ``u`` and applies it.
    Every sum runs in a fixed order, so a step is bit-repeatable.  The step is
    not elementwise: there is no ranged ``update``, and every space needs its
    tensors' ``segments`` (the compact parameter-server shards have none)."""

    PARTS = 2  # the kernels' layout: part[2c], part[2c + 1] = the sums of w^2, u^2 of chunk c

    def __init__(self, spaces, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, decay_groups=None,
                 adapt_groups=None, max_grad_norm=None):
        super().__init__(spaces, lr, betas, eps, weight_decay, decay_groups, max_grad_norm, adapt_groups=adapt_groups)

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        self.begin_step()
        lr = self.lr if lr is None else lr
        if self._clip is not None:
            self._clip_scalar(grad_scale)
        if not self._gpu:
            for si in range(len(self.spaces)):
                self._cpu_step(si, grad_scale, lr)
            return
        stream, bc, dcoef = _lib.stream(), _lib.ptr(self._bc), self._dcoef
        for si, (s, t) in enumerate(zip(self.spaces, self._tables())):
            w, m, v, chunks = _lib.ptr(s.w), _lib.ptr(self.m[si]), _lib.ptr(self.v[si]), _lib.ptr(t.chunks)
            part, ratio, wd = _lib.ptr(self._part[si]), _lib.ptr(self._ratio[si]), self._wd(s)
            _lib.call("kfa_lamb_stage1", w, *_garg(s.grad), m, v, chunks, t.nchunks, part, self.b1, self.b2, self.eps,
                      wd, grad_scale, bc, dcoef, stream)
            if ratio is not None:
                _lib.call("kfa_lamb_ratio", part, _lib.ptr(t.tens), t.ntens, ratio, stream)
            _lib.call("kfa_lamb_stage2", w, _lib.ptr(s.wb), m, v, chunks, t.nchunks, ratio, lr, self.eps, wd, bc,
                      stream)

    def _cpu_step(self, si: int, grad_scale: float, lr: float) -> None:
        s = self.spaces[si]
        bc1 = 1.0 - self.b1 ** self.step_count
        bc2 = 1.0 - self.b2 ** self.step_count
        wd, ratio = self._wd(s), self._ratio[si]
        gr = s.grad
        for k, (a, n) in enumerate(s.segments):
            w, m, v = s.w[a:a + n], self.m[si][a:a + n], self.v[si][a:a + n]
            d = self._cpu_grad(gr[a:a + n], grad_scale)
            m.mul_(self.b1).add_(d, alpha=1 - self.b1)
            v.mul_(self.b2).addcmul_(d, d, value=1 - self.b2)
            u = (m / bc1) / ((v / bc2).sqrt() + self.eps) + wd * w
            r = 1.0
            if ratio is not None:
                wn, un = float(w.norm()), float(u.norm())
                if wn > 0 and un > 0:
                    r = wn / un
                ratio[k] = r
            w.add_(u, alpha=-lr * r)
        if s.wb is not None:
            s.wb.copy_(s.w)


class FusedLARS(_TrustRatios, _FusedBase):
    """LARS (You, Gitman, Ginsburg, 2017): momentum SGD whose update of tensor ``t`` of
    a space is scaled by a layer-wise rate.  With g~ = g * grad_scale * clip

        lambda_t = trust * |w_t| / (|g~_t| + wd * |w_t| + eps)   (1 when either norm is 0)
        d   = lambda_t * (g~ + wd * w)
        mom = momentum * mom + d
        w  -= lr * (d + momentum * mom  if nesterov else  mom)

    with ``lambda_t`` on the spaces named in ``adapt_groups`` (default: the decay
    groups, i.e. ``"weights"``) and exactly 1 elsewhere; ``wd`` follows
    ``decay_groups``.  ``lr`` multiplies what the momentum buffer gives, which is
    ``FusedSGD``'s and ``torch.optim.SGD``'s convention; the paper folds ``lr`` into
    the buffer, so the two differ whenever ``lr`` changes between steps.  ``mom``
    starts at 0 and there is no dampening, so no step is special.

    An adapting space takes one pass for its norms (g and w read once, per-chunk sums
    of w^2 and g^2), one small launch for the rates and the update pass; the other
    spaces take the update pass alone.  With ``max_grad_norm`` the g^2 partials are
    also the global norm's (the spaces that do not adapt add theirs with one read of
    their gradient), so a clipped step reads no gradient twice for a norm.  Every sum
    runs in a fixed order and every scalar stays on the device: a step is
    bit-repeatable and replays from a HIP graph.  The step is not elementwise: there
    is no ranged ``update``, and every space needs its tensors' ``segments``.

    ``FusedLARS(adapt_groups=())`` is momentum SGD with global-norm clipping, which
    ``FusedSGD`` does not take: without ``max_grad_norm``, and with the norm under
    it, the step is ``FusedSGD(dampening=0)``'s bit for bit."""

    def __init__(self, spaces, lr=0.1, momentum=0.9, weight_decay=5e-5, trust=0.001, eps=1e-8, nesterov=False,
                 decay_groups=None, adapt_groups=None, max_grad_norm=None):
        super().__init__(spaces, lr, weight_decay, decay_groups, max_grad_norm, g2_partials=True,
                         adapt_groups=adapt_groups)
        self.momentum = momentum
        self.trust = trust
        self.eps = eps
        self.nesterov = nesterov
        self.mom = [torch.zeros(s.numel, dtype=torch.float32, device=s.device) for s in self.spaces]

    def _g2_partials(self, si: int, stream: int) -> None:
        """An adapting space's norms pass: its w^2 partials into ``_part``, and its g^2 partials
        where the clip norm takes them."""
        if self._ratio[si] is None:
            return _FusedBase._g2_partials(self, si, stream)
        s, t = self.spaces[si], self._tabs[si]
        _lib.call("kfa_lars_norms", _lib.ptr(s.w), *_garg(s.grad), _lib.ptr(t.chunks), t.nchunks,
                  _lib.ptr(self._part[si]), self._gaddr[si], stream)

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        self.step_count += 1
        lr = self.lr if lr is None else lr
        stream, dcoef = _lib.stream() if self._gpu else None, self._dcoef
        if self._clip is not None:  # GPU: every space's g^2 partials, the adapting ones' from their norms pass
            self._clip_scalar(grad_scale, stream)
        if not self._gpu:
            for si in range(len(self.spaces)):
                self._cpu_step(si, grad_scale, lr)
            return
        if self._clip is None:
            for si, ratio in enumerate(self._ratio):
                if ratio is not None:
                    self._g2_partials(si, stream)
        for si, (s, t) in enumerate(zip(self.spaces, self._tabs)):
            ratio, wd = _lib.ptr(self._ratio[si]), self._wd(s)
            if ratio is not None:
                _lib.call("kfa_lars_ratio", _lib.ptr(self._part[si]), self._gaddr[si], _lib.ptr(t.tens), t.ntens, ratio,
                          grad_scale, dcoef, self.trust, wd, self.eps, stream)
            _lib.call("kfa_lars_apply", _lib.ptr(s.w), _lib.ptr(s.wb), *_garg(s.grad), _lib.ptr(self.mom[si]),
                      _lib.ptr(t.chunks), t.nchunks, ratio, lr, self.momentum, wd, int(self.nesterov), grad_scale,
                      dcoef, stream)

    def _cpu_step(self, si: int, grad_scale: float, lr: float) -> None:
        s = self.spaces[si]
        wd, ratio = self._wd(s), self._ratio[si]
        gr = s.grad
        for k, (a, n) in enumerate(s.segments):
            w, mom = s.w[a:a + n], self.mom[si][a:a + n]
            d = self._cpu_grad(gr[a:a + n], grad_scale)
            lam = 1.0
            if ratio is not None:
                wn, gn = float(w.double().norm()), float(d.double().norm())  # fp32 sums drift at 1e6 elements
                if wn > 0 and gn > 0:
                    lam = self.trust * wn / (gn + wd * wn + self.eps)
                ratio[k] = lam
            d = d.add(w, alpha=wd)
            if ratio is not None:
                d = d * lam
            mom.mul_(self.momentum).add_(d)
            w.add_(d + self.momentum * mom if self.nesterov else mom, alpha=-lr)
        if s.wb is not None:
            s.wb.copy_(s.w)

"""Input batch builder (HIP, ``csrc/kernels/image_batch.hip``): gather, crop / pad,
flip, bilinear resize, normalise, cast and channels-last layout of a uint8 image
store in one launch.

``params`` is an int32 ``[B, 6]`` table, one row ``(index, y0, x0, h, w, flip)`` per
sample.  A box of the output size is copied (it may overhang the image: taps
outside are zero pixels, i.e. pad-and-crop); any other box is resampled
bilinearly (``align_corners=False``, no antialias) and must lie inside the image.
``image_batch_reference`` is the same arithmetic in torch on the CPU: the CPU
path of ``image_batch`` and what the tests compare the kernel with.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import _lib

_lib.register("kfa_image_batch", [_lib.P] * 6 + [_lib.L] + [_lib.I] * 5 + [_lib.F] * 6 + [_lib.I, _lib.P])

IMAGENET_MEAN = (123.675, 116.28, 103.53)
IMAGENET_STD = (58.395, 57.12, 57.375)

ERR_ARGS, ERR_ROW, ERR_BOX = -1, -2, -3  # the entry's refusals (see kfa_image_batch)


def _norm_consts(mean: Sequence[float], std: Sequence[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``mean`` and ``1 / std`` exactly as both the kernel and the reference use them."""
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f"mean and std take 3 values each, got {len(mean)} and {len(std)}")
    if not all(float(s) > 0 for s in std):
        raise ValueError(f"std must be positive, got {list(std)}")
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32)
    s = torch.tensor([float(v) for v in std], dtype=torch.float32)
    return m, s.reciprocal()


def _check_inputs(src, labels, params, out_hw, dtype) -> Tuple[int, int]:
    if not (isinstance(src, torch.Tensor) and src.dtype == torch.uint8):
        raise ValueError(f"src must be a uint8 tensor, got {getattr(src, 'dtype', type(src))}")
    if src.dim() != 4 or src.shape[3] != 3 or src.shape[0] < 1 or src.shape[1] < 1 or src.shape[2] < 1:
        raise ValueError(f"src must be [N, Hs, Ws, 3] (NHWC, RGB), got {tuple(src.shape)}")
    if not src.is_contiguous():
        raise ValueError("src must be C-contiguous")
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != src.shape[0]:
        raise ValueError(f"labels must be int64 [{src.shape[0]}], got {labels.dtype} {tuple(labels.shape)}")
    if not labels.is_contiguous() or labels.device != src.device:
        raise ValueError("labels must be contiguous and on the device of src")
    if params.dtype != torch.int32 or params.dim() != 2 or params.shape[1] != 6 or params.shape[0] < 1:
        raise ValueError(f"params must be int32 [B, 6] with B >= 1, got {params.dtype} {tuple(params.shape)}")
    if not params.is_contiguous():
        raise ValueError("params must be contiguous")
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"dtype must be torch.bfloat16 or torch.float32, got {dtype}")
    Ho, Wo = (int(v) for v in out_hw)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"out_hw must be positive, got {tuple(out_hw)}")
    return Ho, Wo


def check_boxes(params: torch.Tensor, N: int, Hs: int, Ws: int, Ho: int, Wo: int) -> None:
    """What the entry checks, as ``ValueError``s that name the row."""
    p = params.cpu().long()
    idx, y0, x0, h, w = (p[:, k] for k in range(5))
    bad = ((idx < 0) | (idx >= N) | (h < 1) | (w < 1) | (y0.abs() > 1 << 24) | (x0.abs() > 1 << 24)).nonzero()
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"params row {b} {p[b].tolist()}: index outside [0, {N}), empty box or origin out of range")
    direct = (h == Ho) & (w == Wo)
    out = (~direct & ((y0 < 0) | (x0 < 0) | (y0 + h > Hs) | (x0 + w > Ws))).nonzero()
    if out.numel():
        b = int(out[0])
        raise ValueError(f"params row {b} {p[b].tolist()}: a resample box must lie inside the {Hs}x{Ws} image "
                         f"(only a {Ho}x{Wo} box may overhang it)")


def _taps(n_out: int, n: torch.Tensor, flip: torch.Tensor = None):
    """Bilinear taps of every output position for per-sample source sizes ``n`` [B]:
    ``(t0, t1, l)`` as [B, n_out]; integer coordinates, one fp32 rounding of l, as the kernel."""
    o = torch.arange(n_out, dtype=torch.int64).unsqueeze(0).expand(n.shape[0], n_out)
    if flip is not None:
        o = torch.where(flip.unsqueeze(1), n_out - 1 - o, o)
    # s = (o + 0.5) n / n_out - 0.5 = num / den exactly; clamped to [0, n - 1]
    num = ((2 * o + 1) * n.unsqueeze(1) - n_out).clamp_min(0)
    den = 2 * n_out
    t0 = torch.div(num, den, rounding_mode="floor")
    l = (num - t0 * den).to(torch.float32) / torch.tensor(float(den), dtype=torch.float32)
    last = (n - 1).unsqueeze(1)
    l = torch.where(t0 >= last, torch.zeros_like(l), l)
    t0 = torch.minimum(t0, last)
    return t0, torch.minimum(t0 + 1, last), l


def _resample_reference(src, params, Ho: int, Wo: int) -> torch.Tensor:
    """Resample arithmetic for every row of ``params`` -> fp32 [B, Ho, Wo, 3], not normalised."""
    p = params.long()
    idx, y0, x0, h, w, flip = (p[:, k] for k in range(6))
    ya, yb, ly = _taps(Ho, h)
    xa, xb, lx = _taps(Wo, w, flip != 0)
    Hs, Ws = src.shape[1], src.shape[2]
    ya, yb = ((t + y0.unsqueeze(1)).clamp(0, Hs - 1) for t in (ya, yb))
    xa, xb = ((t + x0.unsqueeze(1)).clamp(0, Ws - 1) for t in (xa, xb))
    n = idx.view(-1, 1, 1)

    def px(yy, xx):
        return src[n, yy.unsqueeze(2), xx.unsqueeze(1)].to(torch.float32)  # [B, Ho, Wo, 3]

    lx4, ly4 = lx.view(-1, 1, Wo, 1), ly.view(-1, Ho, 1, 1)
    wx0, wy0 = 1.0 - lx4, 1.0 - ly4
    top = wx0 * px(ya, xa) + lx4 * px(ya, xb)
    bot = wx0 * px(yb, xa) + lx4 * px(yb, xb)
    return wy0 * top + ly4 * bot


def _direct_reference(src, params, Ho: int, Wo: int) -> torch.Tensor:
    """Copy arithmetic (zero pixels outside the image) -> fp32 [B, Ho, Wo, 3], not normalised."""
    p = params.long()
    idx, y0, x0, flip = p[:, 0], p[:, 1], p[:, 2], p[:, 5] != 0
    Hs, Ws = src.shape[1], src.shape[2]
    j = torch.arange(Wo).unsqueeze(0).expand(p.shape[0], Wo)
    j = torch.where(flip.unsqueeze(1), Wo - 1 - j, j)
    yy = y0.unsqueeze(1) + torch.arange(Ho).unsqueeze(0)  # [B, Ho]
    xx = x0.unsqueeze(1) + j                                # [B, Wo]
    inside = ((yy >= 0) & (yy < Hs)).unsqueeze(2) & ((xx >= 0) & (xx < Ws)).unsqueeze(1)
    v = src[idx.view(-1, 1, 1), yy.clamp(0, Hs - 1).unsqueeze(2), xx.clamp(0, Ws - 1).unsqueeze(1)]
    return (v * inside.unsqueeze(3)).to(torch.float32)


def image_batch_reference(src: torch.Tensor, labels: torch.Tensor, params: torch.Tensor, mean: Sequence[float],
                          std: Sequence[float], out_hw, dtype: torch.dtype = torch.float32,
                          resample_all: bool = False):
    """The kernel's arithmetic in torch on the CPU -> ``(x [B, 3, Ho, Wo] channels-last, y [B])``.
    ``resample_all`` runs boxes of the output size through the resample arithmetic too."""
    src, labels, params = src.cpu(), labels.cpu(), params.cpu()
    Ho, Wo = _check_inputs(src, labels, params, out_hw, dtype)
    check_boxes(params, src.shape[0], src.shape[1], src.shape[2], -1 if resample_all else Ho,
                -1 if resample_all else Wo)
    m, inv = _norm_consts(mean, std)
    direct = (params[:, 3] == Ho) & (params[:, 4] == Wo) & (not resample_all)
    raw = torch.empty((params.shape[0], Ho, Wo, 3), dtype=torch.float32)
    if direct.any():
        raw[direct] = _direct_reference(src, params[direct], Ho, Wo)
    if (~direct).any():
        raw[~direct] = _resample_reference(src, params[~direct], Ho, Wo)
    x = ((raw - m) * inv).to(dtype)  # NHWC memory
    return x.permute(0, 3, 1, 2), labels[params[:, 0].long()]


def launch(src, labels, params_dev, params_host, x, y, mean, inv, Ho: int, Wo: int) -> int:
    """The raw entry: its status, unchecked (``image_batch`` raises on a non-zero one)."""
    return _lib.lib().kfa_image_batch(
        _lib.ptr(src), _lib.ptr(labels), _lib.ptr(params_dev), _lib.ptr(params_host), _lib.ptr(x), _lib.ptr(y),
        src.shape[0], params_host.shape[0], src.shape[1], src.shape[2], Ho, Wo,
        float(mean[0]), float(mean[1]), float(mean[2]), float(inv[0]), float(inv[1]), float(inv[2]),
        int(x.dtype == torch.float32), _lib.stream())


def image_batch(src: torch.Tensor, labels: torch.Tensor, params: torch.Tensor, mean: Sequence[float],
                std: Sequence[float], out_hw, dtype: torch.dtype = torch.bfloat16, validate: bool = True):
    """``(x, y)``: x ``[B, 3, Ho, Wo]`` in channels-last memory, ``y[b] = labels[params[b, 0]]``.

    ``src`` / ``labels`` on a GPU run the HIP kernel on the current stream; on the
    CPU the reference runs.  ``params`` may live on either side: a host table
    (pinned for an asynchronous upload) is copied to the device, a device table
    is read back, because the entry checks the host copy before it launches.
    ``validate=False`` leaves the box check to the entry (``RuntimeError`` with
    its status)."""
    Ho, Wo = _check_inputs(src, labels, params, out_hw, dtype)
    m, inv = _norm_consts(mean, std)
    if not src.is_cuda:
        return image_batch_reference(src, labels, params, mean, std, (Ho, Wo), dtype)
    host = params.cpu() if params.is_cuda else params
    if validate:
        check_boxes(host, src.shape[0], src.shape[1], src.shape[2], Ho, Wo)
    dev = params if params.is_cuda else params.to(src.device, non_blocking=True)
    if dev.device != src.device:
        raise ValueError("params must be on the host or on the device of src")
    B = host.shape[0]
    x = torch.empty((B, 3, Ho, Wo), dtype=dtype, device=src.device, memory_format=torch.channels_last)
    y = torch.empty((B,), dtype=torch.int64, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(launch(src, labels, dev, host, x, y, m.tolist(), inv.tolist(), Ho, Wo), "kfa_image_batch")
    return x, y

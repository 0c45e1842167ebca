"""References, error bounds and input generators for the transformer-kernel tests
(csrc/kernels/transformer.hip).  Not a test module; needs no GPU.

Every operation is written ONCE as a formula over a dtype:

* ``dtype=torch.float64``: the reference, evaluated from exactly the bits the kernel
  receives (bf16 / fp32 inputs cast up, nothing rounded on the way);
* ``dtype=torch.float32``: the *emulation* - the kernel's formula in the kernel's
  operation order in plain torch, rounded to bf16 where the kernel rounds
  (``*_emul``).  ``test_transformer_bounds_cpu.py`` asserts that the emulation sits
  at <= 0.75 of every bound below, which pins the bounds independently of the
  kernels they judge.

Bounds (u = 2^-24, K = 64): a bf16 output computed in fp32 and rounded once obeys
``|out - ref| <= 2^-7 |ref| + K u A``: one bf16 ulp (twice round-to-nearest) plus K
fp32 roundings (<= 64 serial adds per lane + 6 shuffle levels) of ``A``, the sum of the
absolute values of the terms the formula combines.  Column sums of non-grid data use
the probabilistic ``max(4, 2 sqrt(rows)) u sum|term|``; pure column sums are tested
exactly on grid data (multiples of 1/8 in [-4, 4]: every partial sum fits fp32).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
K = 64
BF = 2.0 ** -7          # one bf16 ulp, relative
SM_FLOOR = 2.0 ** -120  # softmax: below this a flushed denormal is not an error
GELU_FWD = 4e-7         # |gelu_kernel(z) - gelu(z)| <= GELU_FWD |z|  (A&S 7.1.26 + fp32 + v_rcp / v_exp)
GELU_GRAD = 8e-7        # |gelu'_kernel(z) - gelu'(z)| <= GELU_GRAD (1 + |z|)
TANH_FWD = 8 * U        # tanhf + the rounding of z = x + b (|z| (1 - tanh^2) u <= 0.45 u)
TANH_GRAD = 24 * U      # 1 - t^2: 2 |t| TANH_FWD + two roundings + the rounding of z (<= 0.6 u)
ACTS = ("gelu", "tanh", "relu", None)


def f32(v):
    """A Python float as the value it has after crossing the C ABI as ``float``."""
    return float(np.float32(v))


def bf16_exact(t):
    """Round through bf16 (the kernel's pack8) and come back in t's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


# ----------------------------------------------------------------------------- dropout
def drop_thresh(p):
    if p <= 0:
        return 0
    return min(int(float(np.float32(p)) * 4294967296.0), 4294967295)


def drop_scale(p):
    """dscale as the launcher computes it: fp32 1 / (1 - p)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def keep_mask(key, rows, N, p):
    """bool [rows, N]: keep(i) = drop_hash(key, i) >= thresh, i the linear element index.
    ``key`` is what the kernel is launched with (``hash_key(seed)`` for the wrappers)."""
    from test_attention_gpu import _drop_hash
    idx = np.arange(rows * N, dtype=np.uint64)
    return torch.from_numpy((_drop_hash(key, idx) >= np.uint32(drop_thresh(p))).reshape(rows, N))


def _drop(t, keep, dscale):
    if keep is None:
        return t
    return torch.where(keep, t * dscale, torch.zeros_like(t))


# ----------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def grid(shape, seed):
    """Multiples of 1/8 in [-4, 4] (bf16-exact; sums of <= 8200 of them are fp32-exact)."""
    return (torch.randint(-32, 33, shape, generator=_gen(seed)).float() / 8).to(torch.bfloat16)


def ln_inputs(kind, rows, H, seed=0):
    """(x, res, bias, gamma, beta) on the CPU; x / res bf16, the rest fp32.
    normal: N(3, 2^2) rows (large mean: the variance cancels);
    near:   1 + k 2^-7, k in {-1, 0, 1} (eps = 1e-5 moves rstd by ~10 %);
    const:  constant rows of bf16-exact values (variance exactly 0)."""
    g = _gen(seed * 7919 + rows * 31 + H)
    gamma = torch.rand(H, generator=g) + 0.5
    beta = torch.randn(H, generator=g)
    if kind == "normal":
        x = (3 + 2 * torch.randn(rows, H, generator=g)).to(torch.bfloat16)
        res = torch.randn(rows, H, generator=g).to(torch.bfloat16)
        bias = torch.randn(H, generator=g)
    elif kind == "near":
        x = (1 + torch.randint(-1, 2, (rows, H), generator=g).float() * 2.0 ** -7).to(torch.bfloat16)
        res = (0.5 + torch.randint(-1, 2, (rows, H), generator=g).float() * 2.0 ** -7).to(torch.bfloat16)
        bias = torch.full((H,), 0.25)
    elif kind == "const":
        x = (torch.randint(-12, 13, (rows, 1), generator=g).float() / 4).expand(rows, H).contiguous().to(torch.bfloat16)
        res = (torch.randint(-8, 9, (rows, 1), generator=g).float() / 2).expand(rows, H).contiguous().to(torch.bfloat16)
        bias = torch.full((H,), -1.5)
    else:
        raise ValueError(kind)
    return x, res, bias, gamma, beta


def ln_bwd_inputs(rows, H, seed=0):
    """(dy, dy2, xs, gamma) on the CPU: xs ~ N(3, 2^2) bf16, dy / dy2 ~ N(0, 1) bf16."""
    g = _gen(seed * 104729 + rows * 17 + H)
    xs = (3 + 2 * torch.randn(rows, H, generator=g)).to(torch.bfloat16)
    dy = torch.randn(rows, H, generator=g).to(torch.bfloat16)
    dy2 = torch.randn(rows, H, generator=g).to(torch.bfloat16)
    gamma = torch.rand(H, generator=g) + 0.5
    return dy, dy2, xs, gamma


def ln_bwd_grid_inputs(rows, H, seed=0):
    """Inputs on which ln_bwd is exact in fp32 in any order (H % 8 == 0, rows <= 8200).
    Columns come in pairs (2i, 2i + 1) sharing xs and a power-of-two gamma and carrying
    dy = +t / -t, with mean = 0 and rstd = 1: then sum(g) = sum(g xhat) = 0 exactly per
    row, dx == dy gamma, and every partial sum of dgamma (multiples of 1/64, < 2^23 of
    them), dbeta and dbias is an fp32 integer multiple of its grid."""
    g = _gen(seed * 15485863 + rows * 13 + H)
    half = lambda t: t.repeat_interleave(2, dim=-1)  # noqa: E731
    xs = half(torch.randint(-32, 33, (rows, H // 2), generator=g).float() / 8).to(torch.bfloat16)
    t = torch.randint(-32, 33, (rows, H // 2), generator=g).float() / 8
    dy = torch.stack((t, -t), -1).reshape(rows, H).to(torch.bfloat16)
    gamma = half(2.0 ** torch.randint(-1, 2, (H // 2,), generator=g).float())
    return dy, xs, gamma, torch.zeros(rows), torch.ones(rows)


def act_inputs(rows, N, seed=0):
    """(x, b, dy) on the CPU.  x + b covers [-8, 8]: the first 8 columns of every row
    hold a ramp (period 1024 rows at 1/64 steps); the rest is N(0, 1.5^2)."""
    g = _gen(seed * 32452843 + rows * 11 + N)
    x = 1.5 * torch.randn(rows, N, generator=g)
    b = 0.5 * torch.randn(N, generator=g)
    ramp = ((torch.arange(rows * 8) * 37) % 1025).float().view(rows, 8) / 64 - 8
    x[:, :8] = ramp
    b[:8] = 0
    dy = torch.randn(rows, N, generator=g)
    # dropout zero-pattern checks need |dy| and |x| bounded away from 0
    dy = torch.where(dy.abs() < 0.05, torch.full_like(dy, 0.25), dy)
    return x.to(torch.bfloat16), b, dy.to(torch.bfloat16)


def softmax_inputs(B, heads, S, rows_q=None, seed=0):
    """(scores [B*heads*rows_q, S] bf16, key_bias [B, S] fp32, dp like scores).  ~20 % of
    the keys masked at -10000; the LAST batch entry fully masked."""
    g = _gen(seed * 49979687 + B * 7 + heads * 3 + S)
    rq = S if rows_q is None else rows_q
    sc = (3 * torch.randn(B * heads * rq, S, generator=g)).to(torch.bfloat16)
    kb = (torch.rand(B, S, generator=g) < 0.2).float() * -10000.0
    kb[B - 1] = -10000.0
    dp = torch.randn(B * heads * rq, S, generator=g)
    dp = torch.where(dp.abs() < 0.05, torch.full_like(dp, 0.25), dp)
    return sc, kb, dp.to(torch.bfloat16)


# ----------------------------------------------------------------------------- LayerNorm
def ln_fwd_formula(x, res, bias, gamma, beta, eps, keep=None, dscale=1.0, dtype=torch.float64):
    """v = res + drop(x + bias); returns (y, v, mean, rstd) unrounded in ``dtype``."""
    H = x.shape[-1]
    v = x.to(dtype)
    if bias is not None:
        v = v + bias.to(dtype)
    v = _drop(v, keep, dscale)
    if res is not None:
        v = v + res.to(dtype)
    mean = v.sum(-1, keepdim=True) / H
    d = v - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / H + f32(eps))
    y = (v - mean) * rstd * gamma.to(dtype) + beta.to(dtype)
    return y, v, mean.squeeze(-1), rstd.squeeze(-1)


def ln_fwd_emul(x, res, bias, gamma, beta, eps, keep=None, dscale=1.0):
    y, v, mean, rstd = ln_fwd_formula(x, res, bias, gamma, beta, eps, keep, dscale, torch.float32)
    return y.to(torch.bfloat16), v.to(torch.bfloat16), mean, rstd


def ln_fwd_bounds(v, mean, rstd, gamma, beta):
    """(y_abs, mean_bound, rstd_bound) from the fp64 reference's v / mean / rstd: the
    caller adds BF |y_ref| to y_abs."""
    va = v.abs()
    mva = va.mean(-1, keepdim=True)
    r = rstd.unsqueeze(-1)
    A = r * gamma.abs().to(v.dtype) * (va + mva) + beta.abs().to(v.dtype)
    return K * U * A, K * U * mva.squeeze(-1), K * U * rstd * (1 + mean.abs() * rstd)


def ln_bwd_formula(dy, dy2, xs, mean, rstd, gamma, keep=None, dscale=1.0, dtype=torch.float64):
    """(dx, dbranch, dgamma, dbeta, dbias) unrounded in ``dtype``; dbias sums dbranch."""
    H = dy.shape[-1]
    d = dy.to(dtype)
    if dy2 is not None:
        d = d + dy2.to(dtype)
    m, r = mean.to(dtype).unsqueeze(-1), rstd.to(dtype).unsqueeze(-1)
    xh = (xs.to(dtype) - m) * r
    g = d * gamma.to(dtype)
    c1 = (g * xh).sum(-1, keepdim=True) / H
    c2 = g.sum(-1, keepdim=True) / H
    dx = r * (g - c2 - xh * c1)
    dbr = _drop(dx, keep, dscale)
    return dx, dbr, (d * xh).sum(0), d.sum(0), dbr.sum(0)


def ln_bwd_emul(dy, dy2, xs, mean, rstd, gamma, keep=None, dscale=1.0):
    dx, dbr, dg, db, dbias = ln_bwd_formula(dy, dy2, xs, mean, rstd, gamma, keep, dscale, torch.float32)
    return dx.to(torch.bfloat16), dbr.to(torch.bfloat16), dg, db, dbias


def colsum_factor(rows):
    return max(4.0, 2.0 * math.sqrt(rows)) * U


def ln_bwd_bounds(dy, dy2, xs, mean, rstd, gamma, dx_ref, dscale=1.0):
    """(dx_abs, dgamma_bound, dbeta_bound, dbias_bound) in fp64.  dbranch's absolute part
    is dscale * dx_abs.  dbias sums the fp32 dbranch before it is rounded: every term
    carries its own dx_abs (worst case, summed) plus the accumulation's share of
    sum |dbranch| (with dropout dx_ref over-counts the dropped terms: still a bound)."""
    t = torch.float64
    rows = dy.shape[0]
    d = dy.to(t) if dy2 is None else dy.to(t) + dy2.to(t)
    m, r = mean.to(t).unsqueeze(-1), rstd.to(t).unsqueeze(-1)
    g = (d * gamma.to(t)).abs()
    xa = (xs.to(t).abs() + m.abs()) * r
    A = r * (g + g.mean(-1, keepdim=True) + xa * (g * xa).mean(-1, keepdim=True))
    cf = colsum_factor(rows)
    dx_abs = K * U * A
    return (dx_abs, cf * (d.abs() * xa).sum(0), cf * d.abs().sum(0),
            dscale * (dx_abs.sum(0) + cf * dx_ref.abs().sum(0)))


# ----------------------------------------------------------------------------- activations
def _erf_as(x):
    """The kernel's erf (Abramowitz & Stegun 7.1.26, common.h erf_as) and exp(-x^2), fp32."""
    a = x.abs()
    t = 1.0 / (0.3275911 * a + 1.0)
    e = torch.exp(-a * a)
    poly = t * (t * (t * (t * (t * 1.061405429 - 1.453152027) + 1.421413741) - 0.284496736) + 0.254829592)
    return torch.copysign(1.0 - poly * e, x), e


def act_formula(z, act, dtype=torch.float64):
    if act == "gelu":
        if dtype == torch.float64:
            return 0.5 * z * torch.special.erfc(-z * math.sqrt(0.5))  # no cancellation in the negative tail
        return 0.5 * z * (1.0 + _erf_as(z * 0.70710678118654752)[0])
    if act == "tanh":
        return torch.tanh(z)
    if act == "relu":
        return torch.clamp_min(z, 0)
    return z


def act_grad_formula(z, act, dtype=torch.float64):
    if act == "gelu":
        if dtype == torch.float64:
            return 0.5 * torch.special.erfc(-z * math.sqrt(0.5)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
        erf, e = _erf_as(z * 0.70710678118654752)
        return z * 0.39894228040143268 * e + 0.5 * (1.0 + erf)
    if act == "tanh":
        t = torch.tanh(z)
        return 1.0 - t * t
    if act == "relu":
        return (z > 0).to(z.dtype)
    return torch.ones_like(z)


def bias_act_fwd_formula(x, b, act, keep=None, dscale=1.0, dtype=torch.float64):
    """drop(act(x + b)); returns (y, z)."""
    z = x.to(dtype) if b is None else x.to(dtype) + b.to(dtype)
    return _drop(act_formula(z, act, dtype), keep, dscale), z


def bias_act_fwd_emul(x, b, act, keep=None, dscale=1.0):
    return bias_act_fwd_formula(x, b, act, keep, dscale, torch.float32)[0].to(torch.bfloat16)


def act_fwd_abs(z, act):
    """fp32 error of act(z) before the bf16 rounding (z: the fp64 x + b)."""
    if act == "gelu":
        return GELU_FWD * z.abs()
    if act == "tanh":
        return torch.full_like(z, TANH_FWD)
    return 2 * U * z.abs()  # relu / none: the one rounding of x + b


def act_grad_abs(z, act):
    if act == "gelu":
        return GELU_GRAD * (1 + z.abs())
    if act == "tanh":
        return torch.full_like(z, TANH_GRAD)
    return torch.zeros_like(z)  # relu / none: exact


def bias_act_bwd_formula(dy, x, b, act, gscale=None, keep=None, dscale=1.0, dtype=torch.float64):
    """dx = drop(dy gscale) act'(x + b); returns (dx, dbias, d, z) with d = drop(dy gscale)."""
    d = dy.to(dtype)
    if gscale is not None:
        d = d * gscale
    d = _drop(d, keep, dscale)
    if act is None:
        return d, d.sum(0), d, None
    z = x.to(dtype) if b is None else x.to(dtype) + b.to(dtype)
    dx = d * act_grad_formula(z, act, dtype)
    return dx, dx.sum(0), d, z


def bias_act_bwd_emul(dy, x, b, act, gscale=None, keep=None, dscale=1.0):
    dx, db, _, _ = bias_act_bwd_formula(dy, x, b, act, gscale, keep, dscale, torch.float32)
    return dx.to(torch.bfloat16), db


def bias_act_bwd_bounds(dx_ref, d, z, act):
    """(dx_abs, dbias_bound): act' error carried through dy act' (+ 2u for the scale and
    the product), and for the column sum those systematic errors summed plus the
    accumulation's share of sum |dx|."""
    rows = dx_ref.shape[0]
    dx_abs = 2 * U * dx_ref.abs()
    if z is not None:
        dx_abs = dx_abs + d.abs() * act_grad_abs(z, act)
    return dx_abs, dx_abs.sum(0) + colsum_factor(rows) * dx_ref.abs().sum(0)


# ----------------------------------------------------------------------------- softmax
def softmax_fwd_formula(sc, kb, heads, keep=None, dscale=1.0, dtype=torch.float64):
    """(P, pdrop).  sc [rows, S] (rows = B heads rows_q), kb [B, S] or None.  The bias is
    added in fp32 as the kernel does it; the softmax itself runs in ``dtype``."""
    rows, S = sc.shape
    f = sc.float()
    if kb is not None:
        B = kb.shape[0]
        f = (f.view(B, -1, S) + kb.view(B, 1, S)).view(rows, S)
    f = f.to(dtype)
    e = torch.exp(f - f.max(-1, keepdim=True).values)
    P = e / e.sum(-1, keepdim=True)
    return P, _drop(P, keep, dscale)


def softmax_fwd_emul(sc, kb, heads, keep=None, dscale=1.0):
    P, pd = softmax_fwd_formula(sc, kb, heads, keep, dscale, torch.float32)
    return P.to(torch.bfloat16), pd.to(torch.bfloat16)


def softmax_bwd_formula(p, dp, keep=None, dscale=1.0, dtype=torch.float64):
    """dS = P (dP - sum(P dP)), dP = drop(dp); returns (dS, abs bound without the ulp term)."""
    P = p.to(dtype)
    dP = _drop(dp.to(dtype), keep, dscale)
    s = (P * dP).sum(-1, keepdim=True)
    A = P * (dP.abs() + (P * dP.abs()).sum(-1, keepdim=True))
    return P * (dP - s), K * U * A


def softmax_bwd_emul(p, dp, keep=None, dscale=1.0):
    return softmax_bwd_formula(p, dp, keep, dscale, torch.float32)[0].to(torch.bfloat16)


# ----------------------------------------------------------------------------- QKV layout
def qkv_split_formula(qkv, bias, B, S, heads, d, qscale, dtype=torch.float64):
    """q, k, v [B, heads, S, d] of qkv [B S, 3 heads d] (+ bias), q scaled."""
    x = qkv.to(dtype)
    if bias is not None:
        x = x + bias.to(dtype)
    q, k, v = x.view(B, S, 3, heads, d).permute(2, 0, 3, 1, 4)
    return (q * qscale).contiguous(), k.contiguous(), v.contiguous()


def qkv_merge_formula(dq, dk, dv, B, S, heads, d, qscale, dtype=torch.float64):
    """dqkv [B S, 3 heads d] (dq scaled) and its column sums."""
    parts = [t.to(dtype).view(B, heads, S, d) for t in (dq, dk, dv)]
    parts[0] = parts[0] * qscale
    out = torch.stack(parts, 0).permute(1, 3, 0, 2, 4).reshape(B * S, 3 * heads * d)
    return out, out.sum(0)


# ----------------------------------------------------------------------------- checks
def worst_ratio(out, ref, bound):
    """max |out - ref| / bound (0 / 0 counts as 0; anything over a zero bound as inf)."""
    err = (out.to(torch.float64) - ref.to(torch.float64)).abs()
    bound = bound.to(torch.float64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    return ratio.max().item() if ratio.numel() else 0.0

"""fp64 references and helpers the LAMB / LARS tests share (tests/test_lamb_*.py,
tests/test_lars_*.py).  Not a test module; needs no GPU.  Each test file keeps its own shapes,
seeds, hyper-parameters and its own way of drawing inputs."""
import socket

import torch


def dev():
    return torch.device("cuda")


def ref_clip(grads, gscale, max_norm):
    """(pre-clip norm, coefficient) of torch.nn.utils.clip_grad_norm_ in fp64; coefficient 1 without max_norm."""
    norm = gscale * torch.sqrt(sum(g.double().pow(2).sum() for g in grads))
    if max_norm is None:
        return norm, 1.0
    return norm, min(1.0, float(max_norm / (norm + 1e-6)))


def ref_lamb_step(w, m, v, g, t, *, lr, b1, b2, eps, wd, adapt, gs):
    """One LAMB step of one tensor in fp64, in place; gs = gscale * clip."""
    g = g.double() * gs
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd * w
    wn, un = float(w.norm()), float(u.norm())
    r = wn / un if (adapt and wn > 0 and un > 0) else 1.0
    w.sub_(lr * r * u)


def ref_lars_step(w, mom, g, *, lr, momentum, wd, trust, eps, nesterov, adapt, gs, lam_scale=1.0):
    """One LARS step of one tensor in fp64, in place; gs = gscale * clip.  Returns the rate
    (``lam_scale``: a deliberately wrong rate, for the sharpness check)."""
    g = g.double() * gs
    wn, gn = float(w.norm()), float(g.norm())
    lam = trust * wn / (gn + wd * wn + eps) if (adapt and wn > 0 and gn > 0) else 1.0
    if adapt:
        lam *= lam_scale
    d = lam * (g + wd * w)
    mom.mul_(momentum).add_(d)
    w.sub_(lr * (d + momentum * mom if nesterov else mom))
    return lam


def flat_pair(pw, pb, pad_to=64):
    """The two flat groups of the tests: "weights" and 1-D "norms_biases", each with a group tail."""
    from kubeflow_controller_amd.parallel.flat import FlatGroup
    return FlatGroup(pw, pad_to=pad_to, name="weights"), FlatGroup(pb, pad_to=pad_to, name="norms_biases")


def cpu_groups(shapes_w, shapes_b, pad_to=64):
    torch.manual_seed(7)
    pw = [torch.nn.Parameter(torch.randn(*s)) for s in shapes_w]
    pb = [torch.nn.Parameter(torch.randn(*s)) for s in shapes_b]
    return flat_pair(pw, pb, pad_to)


def set_grads(groups, grads):
    for g, gs in zip(groups, grads):
        g.zero_grad()
        for p, x in zip(g.params, gs):
            p.grad.copy_(x)


def pad_mask(g):
    mask = torch.ones(g.numel, dtype=torch.bool, device=g.device)
    for o, p in zip(g.offsets, g.params):
        mask[o:o + p.numel()] = False
    return mask


def check_against(groups, bufs, refs, atol=1e-4, rtol=1e-4):
    """``bufs[j][gi]``, the flat fp32 buffers of the optimizer (the weights first, then its state),
    per tensor against the flat fp64 ``refs[j][gi][k]``; the bf16 copy where there is one against
    the weights' reference; and the padding of every buffer, which must hold exact zeros."""
    for gi, g in enumerate(groups):
        for k, (o, p) in enumerate(zip(g.offsets, g.params)):
            n = p.numel()
            for buf, ref in zip(bufs, refs):
                got = buf[gi][o:o + n]
                assert torch.isfinite(got).all()
                torch.testing.assert_close(got.double(), ref[gi][k], atol=atol, rtol=rtol)
            if g.master is not None:
                torch.testing.assert_close(p.detach().flatten().double(), refs[0][gi][k], atol=2e-2, rtol=1e-2)
        pad = pad_mask(g)
        assert pad.any()
        for buf in (*(b[gi] for b in bufs), g.data.float()):
            assert torch.count_nonzero(buf[pad]) == 0, "padding must stay exactly 0"


# ---- the CPU files' data-parallel and engine runs: one small model, one batch ---------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(12, 32), torch.nn.ReLU(), torch.nn.Linear(32, 5))


def data():
    g = torch.Generator().manual_seed(1)
    return torch.randn(16, 12, generator=g), torch.randint(0, 5, (16,), generator=g)


def train(model, opt, sync, x, y, steps):
    """``steps`` clipped steps on one batch; the pre-clip norm of each."""
    import torch.nn.functional as F
    norms = []
    for _ in range(steps):
        for g in sync.groups:
            g.zero_grad()
        F.cross_entropy(model(x), y).backward()
        opt.step(grad_scale=sync.finish())
        norms.append(float(opt.last_grad_norm))
    return norms

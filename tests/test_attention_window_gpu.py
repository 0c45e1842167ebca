"""Sliding-window causal attention at head dim 128 (attention_d128.hip, the windowed instances)."""
import math

import numpy as np
import pytest
import torch

from test_attention_gpu import _close, _t16
from test_attention_varlen_gpu import PAD, _keep_masks
from test_gpt_cpu import lm_batch

pytestmark = pytest.mark.gpu

D = torch.device("cuda")
HD = 128


def _band(n, window):
    """[n, n] bool: key <= query and query - key < window."""
    return torch.ones(n, n, device=D).tril().bool() & ~torch.ones(n, n, device=D).tril(-window).bool()


def _run(qkv, bqkv, seqs, dout, heads, kv_heads, p, seed, window):
    from kubeflow_controller_amd.ops import transformer as T
    out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, heads, p, seed, causal=True, kv_heads=kv_heads, window=window)
    db = torch.zeros_like(bqkv)
    dqkv = T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, db, heads, p, seed, causal=True, kv_heads=kv_heads,
                             window=window)
    return out, lse, dqkv, db


@pytest.mark.parametrize("heads,kv_heads", [(2, 2), (2, 1)])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("lens", [[1, 63, 65], [129, 300], [257, 1, 384]], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("window", [1, 17, 64, 100, 200])
def test_window_fwd_bwd(window, lens, p, heads, kv_heads):
    """Tolerances of test_gqa_fwd_bwd (2e-2 ctx and lse, 3e-2 dqkv and dbqkv): they hold, none was widened."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    W, own = (heads + 2 * kv_heads) * HD, sum(lens)
    T_ = own + PAD
    qkv = torch.randn(T_, W, device=D).to(torch.bfloat16)
    dout = torch.randn(T_, heads * HD, device=D).to(torch.bfloat16)
    qkv[own:] = float("nan")    # unowned rows: never read into anything
    dout[own:] = float("nan")
    bqkv = torch.randn(W, device=D) * 0.1
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    out, lse, dqkv, db = _run(qkv, bqkv, seqs, dout, heads, kv_heads, p, 987654321, window)
    xr = qkv.float().nan_to_num(0.0).requires_grad_()
    br = bqkv.clone().requires_grad_()
    keep = [k * _band(n, window) for k, n in zip(_keep_masks(987654321, lens, T_, seqs.max_seqlen, p), lens)] if p else None
    ref = T.attention_varlen_reference(xr, br, seqs, heads, keep, 1.0 / (1.0 - _t16(p) / 65536.0), causal=True,
                                       kv_heads=kv_heads, window=window)
    ref.backward(dout.float().nan_to_num(0.0))
    for name, t in (("out", out[:own]), ("lse", lse[:, :own]), ("dqkv", dqkv[:own]), ("dbqkv", db)):
        assert torch.isfinite(t.float()).all(), name
    _close(out[:own], ref[:own], 2e-2, "ctx")
    _close(dqkv[:own], xr.grad[:own], 3e-2, "dqkv")
    _close(db, br.grad, 3e-2, "dbqkv")
    assert not out[own:].any() and not dqkv[own:].any(), "unowned rows must be written as zeros"
    x = xr.detach() + bqkv
    for i, n in enumerate(lens):
        s0 = int(seqs.cu_host[i])
        q = x[s0:s0 + n, :heads * HD].view(n, heads, HD).transpose(0, 1)
        k = x[s0:s0 + n, heads * HD:(heads + kv_heads) * HD].view(n, kv_heads, HD).transpose(0, 1)
        sc = (q @ k.repeat_interleave(heads // kv_heads, 0).transpose(1, 2)) / math.sqrt(HD)
        _close(lse[:, s0:s0 + n], torch.logsumexp(sc.masked_fill(~_band(n, window), -math.inf), -1), 2e-2, "lse")


@pytest.mark.parametrize("window", [129, 8192])
@pytest.mark.parametrize("heads,kv_heads", [(2, 2), (2, 1)])
def test_window_covers_sequence_is_causal(heads, kv_heads, window):
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    lens, T_ = [129, 1, 70], 200 + PAD
    qkv = torch.randn(T_, (heads + 2 * kv_heads) * HD, device=D).to(torch.bfloat16)
    bqkv = torch.randn(qkv.shape[1], device=D) * 0.1
    dout = torch.randn(T_, heads * HD, device=D).to(torch.bfloat16)
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    for p in (0.0, 0.1):
        got, want = (_run(qkv, bqkv, seqs, dout, heads, kv_heads, p, 5, w) for w in (window, None))
        assert all(torch.equal(g, w) for g, w in zip((got[0], got[1][:, :200], got[2]), (want[0], want[1][:, :200], want[2])))


def test_window_ignores_keys_before_it():
    """Queries 199.. at W = 100 see keys 100.. only: rows 0..99 change nothing of theirs, to the bit."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    heads, n = 2, 300
    qkv = torch.randn(n, 3 * heads * HD, device=D).to(torch.bfloat16)
    bqkv = torch.randn(qkv.shape[1], device=D) * 0.1
    dout = torch.randn(n, heads * HD, device=D).to(torch.bfloat16)
    seqs = T.PackedSeqs([0, n], n, device=D)
    a = _run(qkv, bqkv, seqs, dout, heads, None, 0.0, 0, 100)
    qkv2 = qkv.clone()
    qkv2[:100] = (torch.randn(100, qkv.shape[1], device=D) * 2).to(torch.bfloat16)
    b = _run(qkv2, bqkv, seqs, dout, heads, None, 0.0, 0, 100)
    assert torch.equal(a[0][199:], b[0][199:]) and torch.equal(a[1][:, 199:], b[1][:, 199:])
    assert torch.equal(a[2][199:, :heads * HD], b[2][199:, :heads * HD])


def test_gpt_window_matches_reference():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    cfg = GptConfig(vocab_size=1000, hidden=256, layers=2, heads=2, window=48, intermediate=512, max_position=256)
    torch.manual_seed(0)
    m = GptLM(cfg).eval()
    ref = m.forward_reference(*lm_batch(cfg, [5, 130, 64], 256, "cpu"))
    ref.backward()
    gref = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    mg = m.to(D)
    for p in mg.parameters():
        if p.dim() == 2:
            p.data = p.data.to(torch.bfloat16)
    out = mg(*lm_batch(cfg, [5, 130, 64], 256, D))
    assert abs(out.item() - ref.item()) < 3e-2 * ref.item(), (out.item(), ref.item())
    out.backward()
    for n, p in mg.named_parameters():
        _close(p.grad.cpu(), gref[n], 8e-2, n)

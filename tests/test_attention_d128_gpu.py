"""Packed and causal attention at head dim 128 (csrc/kernels/attention_d128.hip) against the
fp32 reference from the same bf16 bits; lengths cross the 16-key tile, the 32-key slice, the
64-row streamed block and the 128-row owner block on both sides."""
import math

import numpy as np
import pytest
import torch

from test_attention_gpu import _close, _t16
from test_attention_varlen_gpu import HEADS, PAD, _keep_masks
from test_gpt_cpu import lm_batch

pytestmark = pytest.mark.gpu

D = torch.device("cuda")
HD = 128


@pytest.mark.parametrize("lens", [[1], [15, 16, 17], [31, 33], [127, 128, 129], [257, 1, 384]],
                         ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [False, True])
def test_d128_fwd_bwd(causal, p, lens):
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    H, own = HEADS * HD, sum(lens)
    T_ = own + PAD
    qkv = torch.randn(T_, 3 * H, device=D).to(torch.bfloat16)
    dout = torch.randn(T_, H, device=D).to(torch.bfloat16)
    qkv[own:] = float("nan")    # unowned rows: never read into anything
    dout[own:] = float("nan")
    bqkv = torch.randn(3 * H, device=D) * 0.1
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    seed = 987654321
    out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, HEADS, p, seed, causal=causal)
    db = torch.zeros(3 * H, device=D)
    dqkv = T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, db, HEADS, p, seed, causal=causal)

    xr = qkv.float().nan_to_num(0.0).requires_grad_()
    br = bqkv.clone().requires_grad_()
    keep = _keep_masks(seed, lens, T_, seqs.max_seqlen, p) if p > 0 else None
    if keep and causal:
        keep = [torch.tril(k) for k in keep]
    ref = T.attention_varlen_reference(xr, br, seqs, HEADS, keep, 1.0 / (1.0 - _t16(p) / 65536.0), causal=causal)
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
        q, k, _ = x[s0:s0 + n].view(n, 3, HEADS, HD).permute(1, 2, 0, 3)
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(HD)
        if causal:
            sc = sc.masked_fill(~torch.ones(n, n, device=D).tril().bool(), -math.inf)
        _close(lse[:, s0:s0 + n], torch.logsumexp(sc, -1), 2e-2, "lse")


@pytest.mark.parametrize("t", [1, 128, 129, 299])
def test_d128_causal_no_look_ahead(t):
    """Queries before the cut never see rows at or past it: same shape, same work split, so
    the same operations in the same order — bit-identical."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(1)
    n, H = 300, HEADS * HD
    qkv = torch.randn(n, 3 * H, device=D).to(torch.bfloat16)
    seqs = T.PackedSeqs([0, n], n, device=D)
    out0, lse0 = T.attn_varlen_fwd(qkv, None, seqs, HEADS, causal=True)
    qkv[t:] = torch.randn(n - t, 3 * H, device=D).to(torch.bfloat16)
    out1, lse1 = T.attn_varlen_fwd(qkv, None, seqs, HEADS, causal=True)
    assert torch.equal(out0[:t], out1[:t]) and torch.equal(lse0[:, :t], lse1[:, :t])
    assert not torch.equal(out0[t:], out1[t:])


def test_gpt_d128_matches_reference():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    cfg = GptConfig(vocab_size=1000, hidden=256, layers=2, heads=2, intermediate=512, max_position=256)
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

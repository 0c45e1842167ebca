"""Grouped-query attention at head dim 128 (csrc/kernels/attention_d128.hip, the GQA instances) against the fp32
reference from the same bf16 bits, and against the multi-head kernels on the K/V-expanded batch."""
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


@pytest.mark.parametrize("lens", [[1], [15, 16, 17], [63, 65], [127, 128, 129], [257, 1, 384]],
                         ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_fwd_bwd(causal, p, lens):
    """Multi-query attention (2 query heads, 1 KV head) against the fp32 reference."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    heads, W, own = 2, 4 * HD, sum(lens)
    T_ = own + PAD
    qkv = torch.randn(T_, W, device=D).to(torch.bfloat16)
    dout = torch.randn(T_, heads * HD, device=D).to(torch.bfloat16)
    qkv[own:] = float("nan")    # unowned rows: never read into anything
    dout[own:] = float("nan")
    bqkv = torch.randn(W, device=D) * 0.1
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, heads, p, 987654321, causal=causal, kv_heads=1)
    db = torch.zeros(W, device=D)
    dqkv = T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, db, heads, p, 987654321, causal=causal, kv_heads=1)
    xr = qkv.float().nan_to_num(0.0).requires_grad_()
    br = bqkv.clone().requires_grad_()
    keep = _keep_masks(987654321, lens, T_, seqs.max_seqlen, p) if p > 0 else None
    if keep and causal:
        keep = [torch.tril(k) for k in keep]
    ref = T.attention_varlen_reference(xr, br, seqs, heads, keep, 1.0 / (1.0 - _t16(p) / 65536.0), causal=causal,
                                       kv_heads=1)
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
        q, k = x[s0:s0 + n, :heads * HD].view(n, heads, HD).transpose(0, 1), x[s0:s0 + n, heads * HD:3 * HD]
        sc = (q @ k.t()) / math.sqrt(HD)
        if causal:
            sc = sc.masked_fill(~torch.ones(n, n, device=D).tril().bool(), -math.inf)
        _close(lse[:, s0:s0 + n], torch.logsumexp(sc, -1), 2e-2, "lse")


@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (6, 2)])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_matches_expanded_mha(causal, p, heads, kv_heads):
    """The multi-head kernels on the K/V-expanded batch: per query head the same operations in the
    same order and the same hash, so out, lse and dQ are bit-identical; dK / dV / their bias
    gradients are the sums over each group (MHA rounds each of the g terms to bf16, GQA once)."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    lens, g, H = [129, 1, 70], heads // kv_heads, heads * HD
    own = sum(lens)
    T_ = own + PAD
    qkv = torch.randn(T_, (heads + 2 * kv_heads) * HD, device=D).to(torch.bfloat16)
    bqkv = torch.randn((heads + 2 * kv_heads) * HD, device=D) * 0.1
    dout = torch.randn(T_, H, device=D).to(torch.bfloat16)
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    # the multi-head batch: KV head c's K / V columns and biases copied to query heads c·g .. c·g + g-1
    qkv_m = torch.cat([qkv[:, :H], qkv[:, H:].view(T_, 2, kv_heads, HD).repeat_interleave(g, 2).view(T_, 2 * H)],
                      1).contiguous()
    bqkv_m = torch.cat([bqkv[:H], bqkv[H:].view(2, kv_heads, HD).repeat_interleave(g, 1).view(2 * H)])
    out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, heads, p, 5, causal=causal, kv_heads=kv_heads)
    db = torch.zeros_like(bqkv)
    dqkv = T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, db, heads, p, 5, causal=causal, kv_heads=kv_heads)
    out_m, lse_m = T.attn_varlen_fwd(qkv_m, bqkv_m, seqs, heads, p, 5, causal=causal)
    db_m = torch.zeros_like(bqkv_m)
    dqkv_m = T.attn_varlen_bwd(qkv_m, bqkv_m, seqs, out_m, lse_m, dout, db_m, heads, p, 5, causal=causal)
    assert torch.equal(out, out_m) and torch.equal(lse[:, :own], lse_m[:, :own])
    assert torch.equal(dqkv[:, :H], dqkv_m[:, :H])
    _close(dqkv[:, H:], dqkv_m[:, H:].float().reshape(T_, 2, kv_heads, g, HD).sum(3).view(T_, -1), 2e-2, "dk dv")
    _close(db[:H], db_m[:H], 3e-2, "dbq")
    _close(db[H:], db_m[H:].view(2, kv_heads, g, HD).sum(2).view(-1), 3e-2, "dbk dbv")


def test_gpt_gqa_matches_reference():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    cfg = GptConfig(vocab_size=1000, hidden=256, layers=2, heads=2, kv_heads=1, intermediate=512, max_position=256)
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

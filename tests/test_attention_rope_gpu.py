"""Rotary position embeddings: rope_qk_kernel (rope.hip) against fp64, and GptLM with ``rotary``."""
import numpy as np
import pytest
import torch

from test_attention_gpu import _close
from test_attention_varlen_gpu import PAD
from test_gpt_cpu import lm_batch

pytestmark = pytest.mark.gpu

D = torch.device("cuda")


def _batch(d, heads, kv_heads, lens):
    """qkv [own + PAD, W] bf16 with a finite sentinel on the V columns and the unowned rows, bqkv, seqs, nrot."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    kvh = kv_heads or heads
    W, nrot, own = (heads + 2 * kvh) * d, heads + kvh, sum(lens)
    x = torch.randn(own + PAD, W, device=D).to(torch.bfloat16)
    x[own:] = 7.0
    x[:, nrot * d:] = -3.0
    return x, torch.randn(W, device=D) * 0.1, T.PackedSeqs(np.cumsum([0] + lens), own + PAD, device=D), nrot


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("lens", [[1, 63, 65], [129, 300]], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("d,heads,kv_heads", [(64, 2, None), (128, 2, None), (128, 2, 1)])
def test_rope_kernel(d, heads, kv_heads, lens, inverse):
    """Per element |got - ref| <= 2^-8 |ref| (bf16's half ulp) + 1e-5 (|x_j| + |x_{j+d/2}|) (the fp32
    evaluation, ~2e-7 of the operands, with a wide margin) against fp64 from the same bf16 input,
    fp32 bias and fp32 table."""
    from kubeflow_controller_amd.ops import transformer as T
    x, bqkv, seqs, nrot = _batch(d, heads, kv_heads, lens)
    own, rot = sum(lens), T.RotaryTable(d, 512, device=D)
    x0 = x.clone()
    got_bias = T.rope_qk_(x, bqkv, seqs, heads, rot, kv_heads, inverse=inverse)
    xin = x0.double() if inverse else x0.double() + bqkv.double()
    ref = T.rope_reference(xin, seqs, nrot, rot, inverse=inverse)[:own, :nrot * d]
    mag = xin[:own, :nrot * d].abs().view(own, nrot, 2, d // 2)
    mag = (mag[:, :, :1] + mag[:, :, 1:]).expand(-1, -1, 2, -1).reshape(own, nrot * d)
    err = (x[:own, :nrot * d].double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * mag
    print(f"max err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), f"max err / bound {(err / bound).max().item()}"
    assert torch.equal(x[own:].view(torch.int16), x0[own:].view(torch.int16)), "unowned rows were written"
    assert torch.equal(x[:, nrot * d:].view(torch.int16), x0[:, nrot * d:].view(torch.int16)), "V columns were written"
    if inverse:
        assert got_bias is None
    else:
        assert not got_bias[:nrot * d].any() and torch.equal(got_bias[nrot * d:], bqkv[nrot * d:])


@pytest.mark.parametrize("d,heads,kv_heads", [(64, 2, None), (128, 2, 1)])
def test_rope_position_zero_is_exact(d, heads, kv_heads):
    """The first row of every sequence has cos = 1, sin = 0: its rotated columns are the rounded
    qkv + bqkv, to the bit (a position taken from the global row rotates rows 1 and 64 here)."""
    from kubeflow_controller_amd.ops import transformer as T
    x, bqkv, seqs, nrot = _batch(d, heads, kv_heads, [1, 63, 65])
    first = seqs.cu_host[:-1].long().to(D)
    want = (x[first].float() + bqkv).to(torch.bfloat16)[:, :nrot * d]
    T.rope_qk_(x, bqkv, seqs, heads, T.RotaryTable(d, 512, device=D), kv_heads)
    assert torch.equal(x[first][:, :nrot * d].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("hidden,heads,kv_heads,window", [(128, 2, None, None), (256, 2, 1, 48)])
def test_gpt_rope_matches_reference(hidden, heads, kv_heads, window):
    """The bounds of test_gpt_window_matches_reference (3e-2 loss, 8e-2 gradients), not widened."""
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    cfg = GptConfig(vocab_size=1000, hidden=hidden, layers=2, heads=heads, kv_heads=kv_heads, window=window,
                    intermediate=512, max_position=256, rotary=True)
    torch.manual_seed(0)
    m = GptLM(cfg).eval()
    assert "pos_emb" not in dict(m.named_parameters())
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

"""Grouped-query attention without a GPU: the reference's layout, the argument checks, the GPT model's shapes."""
import pytest
import torch

from test_gpt_cpu import lm_batch


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads,kv_heads,d", [(2, 1, 128), (6, 2, 64)])
def test_gqa_reference_matches_expanded_mha(heads, kv_heads, d, causal):
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    g, H, rows = heads // kv_heads, heads * d, 40
    qkv = torch.randn(rows, (heads + 2 * kv_heads) * d)
    b = torch.randn((heads + 2 * kv_heads) * d) * 0.1
    seqs = T.PackedSeqs([0, 17, 18, 37], rows)
    mha = torch.cat([qkv[:, :H], qkv[:, H:].view(rows, 2, kv_heads, d).repeat_interleave(g, 2).view(rows, 2 * H)], 1)
    b_mha = torch.cat([b[:H], b[H:].view(2, kv_heads, d).repeat_interleave(g, 1).view(2 * H)])
    got = T.attention_varlen_reference(qkv, b, seqs, heads, causal=causal, kv_heads=kv_heads)
    assert torch.allclose(got, T.attention_varlen_reference(mha, b_mha, seqs, heads, causal=causal), atol=1e-6)


@pytest.mark.parametrize("heads,kv_heads,width,bias,match", [
    (4, 3, 10 * 128, None, "kv_heads must divide heads"),
    (4, 2, 8 * 64, None, "grouped-query attention needs head dim 128"),
    (4, 2, 8 * 128, 12 * 128, r"bqkv must be a contiguous fp32 \[\(heads \+ 2·kv_heads\)·128\]"),
])
def test_gqa_argument_errors(heads, kv_heads, width, bias, match):
    from kubeflow_controller_amd.ops import transformer as T
    qkv = torch.zeros(8, width, dtype=torch.bfloat16)
    bqkv = None if bias is None else torch.zeros(bias)
    with pytest.raises(ValueError, match=match):
        T.attn_varlen_fwd(qkv, bqkv, T.PackedSeqs([0, 8], 8), heads, kv_heads=kv_heads)


@pytest.mark.parametrize("fn", ["EncoderLayerFn", "encoder_layer_reference"])
def test_gqa_layer_needs_packed_batch(fn):
    from kubeflow_controller_amd.ops import transformer as T
    f = T.EncoderLayerFn.apply if fn == "EncoderLayerFn" else T.encoder_layer_reference
    with pytest.raises(ValueError, match="grouped-query attention needs a packed batch"):
        f(torch.zeros(8, 256), None, (1, 8, 2, 0.0, 0.0, 0, 1e-5, None, None, None, False, 1), *[torch.zeros(1)] * 12)


def test_gpt_gqa_model():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM, flops_per_step
    kw = dict(vocab_size=1000, hidden=256, layers=2, heads=2, intermediate=512, max_position=256)
    cfg = GptConfig(kv_heads=1, **kw)
    torch.manual_seed(0)
    m = GptLM(cfg)
    assert tuple(m.layers[0].wqkv.shape) == ((2 + 2) * 128, 256) and tuple(m.layers[0].bqkv.shape) == (4 * 128,)
    lens = [5, 130, 64]
    loss = m(*lm_batch(cfg, lens, 256, "cpu"))
    loss.backward()
    assert torch.isfinite(loss) and all(p.grad is not None for p in m.parameters())
    qkv_term = 3.0 * cfg.layers * 2 * sum(lens) * (6 - 4) * 128 * cfg.hidden
    assert flops_per_step(GptConfig(**kw), lens) - flops_per_step(cfg, lens) == qkv_term
    with pytest.raises(ValueError, match="kv_heads must divide heads"):
        GptLM(GptConfig(vocab_size=1000, hidden=384, layers=1, heads=3, kv_heads=2, intermediate=512))
    with pytest.raises(ValueError, match="head dim 128"):
        GptLM(GptConfig(vocab_size=1000, hidden=128, layers=1, heads=2, kv_heads=1, intermediate=512))

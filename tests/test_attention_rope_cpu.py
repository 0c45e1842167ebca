"""Rotary position embeddings without a GPU: the reference rotation, the argument checks, the GPT config."""
import pytest
import torch


@pytest.mark.parametrize("d", [64, 128])
def test_rope_reference_matches_complex_rotation(d):
    """(x_j + i x_{j+d/2}) · e^{i pos θ_j}, θ_j = base^(-2j/d), in fp64; the inverse is its conjugate."""
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    cu, nrot, base = [0, 1, 6, 46], 3, 500.0
    x = torch.randn(48, 4 * d, dtype=torch.float64)
    seqs, rot = T.PackedSeqs(cu, 48), T.RotaryTable(d, 64, base)
    pos = torch.cat([torch.arange(b - a) for a, b in zip(cu, cu[1:])]).double()
    theta = base ** (-torch.arange(0, d, 2, dtype=torch.float64) / d)
    for inverse in (False, True):
        z = torch.complex(*x[:46, :nrot * d].reshape(46, nrot, 2, d // 2).unbind(2))
        z = z * torch.polar(torch.ones(46, 1, d // 2, dtype=torch.float64), (pos[:, None] * theta)[:, None] * (-1 if inverse else 1))
        want = x.clone()
        want[:46, :nrot * d] = torch.stack((z.real, z.imag), 2).reshape(46, nrot * d)
        # the table is rounded to fp32 once: 2^-24 relative on cos and sin
        assert torch.allclose(T.rope_reference(x, seqs, nrot, rot, inverse=inverse), want, rtol=0, atol=1e-6)


def test_reference_without_rotary_is_unchanged_and_with_it_ignores_placement():
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    heads, d = 2, 64
    qkv, b = torch.randn(48, 3 * heads * d), torch.randn(3 * heads * d) * 0.1
    seqs, rot = T.PackedSeqs([0, 1, 6, 46], 48), T.RotaryTable(d, 64)
    plain = T.attention_varlen_reference(qkv, b, seqs, heads, causal=True)
    assert torch.equal(T.attention_varlen_reference(qkv, b, seqs, heads, causal=True, rotary=None), plain)
    got = T.attention_varlen_reference(qkv, b, seqs, heads, causal=True, rotary=rot)
    assert not torch.allclose(got[6:46], plain[6:46], atol=1e-3)
    alone = T.attention_varlen_reference(qkv[6:46], b, T.PackedSeqs([0, 40], 40), heads, causal=True, rotary=rot)
    assert torch.allclose(got[6:46], alone, rtol=0, atol=1e-6)


@pytest.mark.parametrize("call,match", [
    (lambda T: T.RotaryTable(96, 16), "head dim must be 64 or 128"),
    (lambda T: T.RotaryTable(64, 0), "max_position must be >= 1"),
    (lambda T: T.rope_qk_(torch.zeros(8, 6 * 64, dtype=torch.bfloat16), None, T.PackedSeqs([0, 8], 8), 2,
                          T.RotaryTable(128, 16)), "built for head dim 128, the heads have 64"),
    (lambda T: T.rope_qk_(torch.zeros(8, 6 * 64, dtype=torch.bfloat16), None, T.PackedSeqs([0, 8], 8), 2,
                          T.RotaryTable(64, 4)), "max_seqlen 8 exceeds the rotary table's 4 positions"),
    (lambda T: T.rope_qk_(torch.zeros(8, 6 * 64), None, T.PackedSeqs([0, 8], 8), 2, T.RotaryTable(64, 16)),
     "contiguous bf16"),
    (lambda T: T.rope_qk_(torch.zeros(8, 5 * 128, dtype=torch.bfloat16), None, T.PackedSeqs([0, 8], 8), 3,
                          T.RotaryTable(128, 16), kv_heads=2), "kv_heads must divide heads"),
    (lambda T: T.rope_qk_(torch.zeros(8, 6 * 64, dtype=torch.bfloat16), None, T.PackedSeqs([0, 8], 8), 2,
                          T.RotaryTable(64, 16)), "must be on the same GPU"),
    (lambda T: T.EncoderLayerFn.forward(type("Ctx", (), {})(), torch.zeros(8, 128), None,
                                        (1, 8, 2, 0.0, 0.0, 0, 1e-5, None, None, None, False, None, None,
                                         T.RotaryTable(64, 16)), *[None] * 12),
     "rotary position embeddings need a packed batch"),
    (lambda T: T.encoder_layer_reference(torch.zeros(8, 128), None, (1, 8, 2, 0.0, 0.0, 0, 1e-5, None, None, None,
                                                                    False, None, None, T.RotaryTable(64, 16)),
                                         *[None] * 12), "rotary position embeddings need a packed batch"),
])
def test_rope_argument_errors(call, match):
    from kubeflow_controller_amd.ops import transformer as T
    with pytest.raises(ValueError, match=match):
        call(T)


def test_gpt_rope_config():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    c, g = GptConfig.xl_rope(), GptConfig.xl_gqa()
    assert c.rotary and c.rotary_base == 10000.0 and not g.rotary
    assert (c.hidden, c.layers, c.heads, c.kv_heads, c.intermediate, c.max_position, c.window) == \
        (g.hidden, g.layers, g.heads, g.kv_heads, g.intermediate, g.max_position, g.window)
    kw = dict(vocab_size=1000, layers=1, heads=2, intermediate=256, max_position=32)
    m = GptLM(GptConfig(hidden=128, rotary=True, **kw))
    assert "pos_emb" not in dict(m.named_parameters()) and m.rotary_table("cpu").head_dim == 64
    assert "pos_emb" in dict(GptLM(GptConfig(hidden=128, **kw)).named_parameters())
    with pytest.raises(ValueError, match="rotary position embeddings need head dim 64 or 128"):
        GptLM(GptConfig(hidden=64, rotary=True, **kw))

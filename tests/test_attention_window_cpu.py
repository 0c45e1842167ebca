"""Sliding-window attention without a GPU: the reference's band, the argument checks, the GPT model's FLOP count."""
import pytest
import torch


@pytest.mark.parametrize("window", [1, 3, 64])
def test_window_reference_matches_per_query_loop(window):
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    lens, cu, heads, d = [1, 5, 40], [0, 1, 6, 46], 2, 16
    qkv = torch.randn(48, 3 * heads * d)
    got = T.attention_varlen_reference(qkv, None, T.PackedSeqs(cu, 48), heads, causal=True, window=window)
    want = torch.zeros(48, heads * d)
    for b, n in enumerate(lens):
        q, k, v = qkv[cu[b]:cu[b + 1]].view(n, 3, heads, d).unbind(1)
        for h in range(heads):
            for i in range(n):
                lo = max(0, i - window + 1)   # query i sees keys lo..i
                pr = torch.softmax(k[lo:i + 1, h] @ q[i, h] / d ** 0.5, 0)
                want[cu[b] + i, h * d:(h + 1) * d] = pr @ v[lo:i + 1, h]
    assert torch.allclose(got, want, atol=1e-5)


@pytest.mark.parametrize("width,causal,window,match", [
    (6 * 128, False, 4, "a sliding window needs causal=True"),
    (6 * 128, True, 0, "window must be >= 1"),
    (6 * 64, True, 4, "sliding-window attention needs head dim 128"),
])
def test_window_argument_errors(width, causal, window, match):
    from kubeflow_controller_amd.ops import transformer as T
    qkv = torch.zeros(8, width, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=match):
        T.attn_varlen_fwd(qkv, None, T.PackedSeqs([0, 8], 8), 2, causal=causal, window=window)


def test_gpt_window_config():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM, flops_per_step
    kw = dict(vocab_size=1000, hidden=256, layers=2, heads=2, intermediate=512, max_position=256)
    GptLM(GptConfig(window=48, **kw))
    with pytest.raises(ValueError, match="window must be >= 1"):
        GptLM(GptConfig(window=0, **kw))
    with pytest.raises(ValueError, match="sliding-window attention needs head dim 128"):
        GptLM(GptConfig(window=48, **dict(kw, hidden=128)))
    lens, W = [5, 130, 64], 48
    pairs = sum(min(i + 1, W) for n in lens for i in range(n))
    full = sum(n * (n + 1) // 2 for n in lens)
    saved = flops_per_step(GptConfig(**kw), lens) - flops_per_step(GptConfig(window=W, **kw), lens)
    assert saved == 3.0 * 2 * (2 * 2 * (full - pairs) * 256)
    assert GptConfig.xl_swa().window == 1024 and GptConfig.xl_swa().max_position == 8192

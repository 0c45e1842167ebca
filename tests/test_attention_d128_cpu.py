"""Head dim 128 pieces that need no GPU: the wrappers still refuse every other head dim
before a launch, and the d = 128 GPT shapes run through the fp32 reference."""
import pytest
import torch

from test_gpt_cpu import lm_batch


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [32, 256])
def test_d128_wrapper_refuses_other_dims(d, causal, monkeypatch):
    from kubeflow_controller_amd.ops import _lib
    from kubeflow_controller_amd.ops import transformer as T
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("launched"))
    seqs = T.PackedSeqs([0, 4, 9], 16, 8)
    qkv = torch.zeros(16, 3 * 2 * d, dtype=torch.bfloat16)
    out, lse = torch.zeros(16, 2 * d, dtype=torch.bfloat16), torch.zeros(2, 16)
    with pytest.raises(ValueError, match="64 or 128"):
        T.attn_varlen_fwd(qkv, None, seqs, 2, causal=causal)
    with pytest.raises(ValueError, match="64 or 128"):
        T.attn_varlen_bwd(qkv, None, seqs, out, lse, out, None, 2, causal=causal)


def test_gpt_d128_configs():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    xl = GptConfig.xl()
    assert xl.hidden // xl.heads == 128 and xl.hidden % xl.heads == 0
    cfg = GptConfig(vocab_size=100, hidden=256, layers=1, heads=2, intermediate=256, max_position=32)
    torch.manual_seed(0)
    loss = GptLM(cfg).eval().forward_reference(*lm_batch(cfg, [5, 20], 32, "cpu"))
    assert torch.isfinite(loss)

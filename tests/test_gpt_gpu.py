"""GptLM on the GPU path (causal packed attention kernels, fixed-row-budget loss) against its
fp32 forward_reference; tolerances are those of test_bert_packed_gpu.py."""
import pytest
import torch

from test_attention_gpu import _close
from test_gpt_cpu import lm_batch

pytestmark = pytest.mark.gpu

D = torch.device("cuda")


def test_gpt_matches_reference():
    from kubeflow_controller_amd.models.gpt import GptConfig, GptLM
    cfg = GptConfig.tiny()
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

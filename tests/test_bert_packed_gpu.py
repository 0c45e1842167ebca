"""BERT on a packed batch (models/bert.py: pack_batch + forward_packed, the varlen attention
kernels) against the CPU fp32 reference on the PADDED batch with its attention mask."""
import pytest
import torch

from test_bert_packed_cpu import padded_batch
from test_attention_gpu import _close

pytestmark = pytest.mark.gpu

D = torch.device("cuda")


def test_packed_matches_padded_reference():
    from kubeflow_controller_amd.models.bert import BertConfig, BertForPreTraining, pack_batch
    cfg = BertConfig.tiny()
    cfg.hidden_dropout = cfg.attn_dropout = 0.0
    torch.manual_seed(0)
    m = BertForPreTraining(cfg)
    batch = padded_batch(cfg, [128, 37, 90], 128)
    ref = m.forward_reference(*batch)
    ref.backward()
    gref = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    mg = m.to(D)
    for p in mg.parameters():
        if p.dim() == 2:
            p.data = p.data.to(torch.bfloat16)
    out = mg.forward_packed(*pack_batch(*batch, rows=256, device=D))
    assert abs(out.item() - ref.item()) < 3e-2 * ref.item(), (out.item(), ref.item())
    out.backward()
    for n, p in mg.named_parameters():
        _close(p.grad.cpu(), gref[n], 8e-2, n)

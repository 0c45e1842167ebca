"""GPT LM pieces that need no GPU: the causal reference, the next-token labels over the row
budget, and a gpt_tiny replica step on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F


def lm_batch(cfg, lens, rows, device):
    """The positional args of GptLM.forward for sequences of ``lens`` tokens in ``rows`` rows."""
    from kubeflow_controller_amd.models.gpt import next_token_labels
    from kubeflow_controller_amd.ops.transformer import PackedSeqs
    g = torch.Generator().manual_seed(3)
    own = sum(lens)
    ids = torch.zeros(rows, dtype=torch.int64)
    ids[:own] = torch.randint(0, cfg.vocab_size, (own,), generator=g)
    pos = torch.zeros(rows, dtype=torch.int64)
    pos[:own] = torch.cat([torch.arange(n) for n in lens])
    seqs = PackedSeqs(np.cumsum([0] + lens), rows, device=device)
    return ids.to(device), pos.to(device), seqs, next_token_labels(ids, seqs).to(device)


def test_causal_reference_matches_sdpa():
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    lens, heads, d = [5, 1, 33], 2, 64
    qkv = torch.randn(sum(lens) + 3, 3 * heads * d)
    seqs = T.PackedSeqs(np.cumsum([0] + lens), qkv.shape[0])
    out = T.attention_varlen_reference(qkv, None, seqs, heads, causal=True)
    s0 = 0
    for n in lens:
        q, k, v = qkv[s0:s0 + n].view(n, 3, heads, d).permute(1, 2, 0, 3)
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=True).permute(1, 0, 2).reshape(n, heads * d)
        assert (out[s0:s0 + n] - ref).abs().max() < 1e-5
        s0 += n
    assert not out[s0:].any()


def test_next_token_labels():
    from kubeflow_controller_amd.models.gpt import GptConfig
    lens, rows = [5, 1, 7], 16
    ids, _, seqs, labels = lm_batch(GptConfig.tiny(), lens, rows, "cpu")
    last = (seqs.cu_host[1:] - 1).tolist()
    ignored = sorted(last + list(range(sum(lens), rows)))
    assert (labels < 0).nonzero().flatten().tolist() == ignored and (labels[ignored] == -1).all()
    keep = [t for t in range(rows) if t not in ignored]
    assert torch.equal(labels[keep], ids[[t + 1 for t in keep]])


def test_gpt_tiny_replica_step_cpu():
    from kubeflow_controller_amd.trainer import replica
    args = replica.build_parser().parse_args(["--model", "gpt_tiny", "--batch_size", "2", "--seq_len", "48"])
    dev = torch.device("cpu")
    model, _, loss_fn = replica.build(args, dev)
    batch = replica.synthetic_batch(args, model, dev, 0)
    assert batch[0].numel() == 96 and batch[2].max_seqlen == 48
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    first = loss_fn(model, *batch)
    first.backward()
    opt.step()
    assert torch.isfinite(first) and loss_fn(model, *batch) < first

"""Packed BERT batches without a GPU: pack_batch's re-indexing (forward_packed on the CPU
equals forward_reference on the padded batch) and synthetic_packed_mlm_batch's contract."""
import pytest
import torch


def padded_batch(cfg, lens, S, seed=0):
    """A padded [B, S] pre-training batch whose sequence b has lens[b] live tokens (a prefix)
    and cfg.max_predictions masked positions inside them: the arguments of forward()."""
    g = torch.Generator().manual_seed(seed)
    B, n = len(lens), cfg.max_predictions
    L = torch.tensor(lens)
    mask = (torch.arange(S)[None, :] < L[:, None]).long()
    ids = torch.randint(0, cfg.vocab_size, (B, S), generator=g) * mask
    tt = (torch.arange(S)[None, :] >= (L // 2)[:, None]).long() * mask
    pos = torch.stack([torch.randperm(l, generator=g)[:n].sort().values + b * S for b, l in enumerate(lens)])
    labels = torch.randint(0, cfg.vocab_size, (B * n,), generator=g)
    return ids, tt, mask, pos.reshape(-1), labels, torch.randint(0, 2, (B,), generator=g)


@pytest.mark.parametrize("rows", [None, 256])
def test_forward_packed_cpu_matches_padded(rows):
    from kubeflow_controller_amd.models.bert import BertConfig, BertForPreTraining, bert_loss, pack_batch
    cfg = BertConfig.tiny()
    torch.manual_seed(0)
    m = BertForPreTraining(cfg).eval()
    batch = padded_batch(cfg, [128, 37, 90], 128)
    packed = pack_batch(*batch, rows=rows)
    assert packed[0].numel() == (rows or 255) and packed[3].cu_host.tolist() == [0, 128, 165, 255]
    with torch.no_grad():
        ref, out = m.forward_reference(*batch), bert_loss(m, *packed)
    assert torch.allclose(out, ref, rtol=1e-5), (out.item(), ref.item())
    bad = list(batch)
    bad[3] = batch[3].clone()
    bad[3][-1] = 2 * 128 + 100    # sequence 2 has 90 live tokens
    with pytest.raises(ValueError):
        pack_batch(*bad)


def test_synthetic_packed_batch_contract():
    from kubeflow_controller_amd.models.bert import BertConfig, synthetic_packed_mlm_batch
    cfg = BertConfig.tiny()
    rows, S, lo = 1000, 128, 5
    ids, tt, pos_ids, seqs, mlm, labels, nsp = synthetic_packed_mlm_batch(cfg, rows, S, lo, torch.Generator().manual_seed(3))
    cu = seqs.cu_host.long()
    lens = cu[1:] - cu[:-1]
    assert ids.numel() == tt.numel() == pos_ids.numel() == rows == seqs.rows
    assert int(lens.min()) >= lo and int(lens.max()) <= S and int(cu[-1]) <= rows < int(cu[-1]) + S
    assert nsp.numel() == seqs.B and labels.numel() == mlm.numel() == int(lens.clamp(max=cfg.max_predictions).sum())
    owner = torch.bucketize(mlm, cu[1:], right=True)     # the sequence each masked row falls in
    assert torch.equal(owner, torch.repeat_interleave(torch.arange(seqs.B), lens.clamp(max=cfg.max_predictions)))
    assert torch.equal(pos_ids[mlm], mlm - cu[owner]) and mlm.unique().numel() == mlm.numel()

"""Packed variable-length attention (csrc/kernels/attention.hip: attn_varlen_*) against the
plain fp32 reference ops.transformer.attention_varlen_reference, computed from the same bf16
bits the kernels receive.  The dropout case rebuilds the keep mask on the host from the
kernels' hash indexing: row = h·T + token row, key index within its sequence, S = max_seqlen."""
import math

import numpy as np
import pytest
import torch

from test_attention_gpu import _close, _drop_hash, _t16

D = torch.device("cuda")
HEADS, HD = 2, 64
PAD = 5   # unowned rows behind the last sequence


def _keep_masks(seed, lens, T_, max_seqlen, p):
    """Per sequence a [heads, len, len] keep mask: the pair (q, k) / (q, k + 16), k with bit 4
    clear, shares the hash of index (h·T + row)·max_seqlen + k; low half decides k, high half k + 16."""
    from kubeflow_controller_amd.ops.transformer import hash_key
    masks, s0 = [], 0
    for n in lens:
        key = np.arange(n, dtype=np.uint64)
        rows = (np.arange(HEADS, dtype=np.uint64)[:, None] * np.uint64(T_) + np.uint64(s0) + key[None, :]).reshape(-1)
        h = _drop_hash(hash_key(seed), rows[:, None] * np.uint64(max_seqlen) + (key & ~np.uint64(16))[None, :])
        half = np.where((key & np.uint64(16)) != 0, h >> np.uint32(16), h & np.uint32(0xFFFF))
        masks.append(torch.from_numpy((half >= _t16(p)).reshape(HEADS, n, n).astype(np.float32)).to(D))
        s0 += n
    return masks


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [[1], [15, 16, 17], [31, 33], [127, 128, 129], [17, 257, 1, 128, 40], [128, 128]],
                         ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_varlen_fwd_bwd(p, lens):
    from kubeflow_controller_amd.ops import transformer as T
    torch.manual_seed(0)
    H, own = HEADS * HD, sum(lens)
    T_ = own + PAD
    qkv = torch.randn(T_, 3 * H, device=D).to(torch.bfloat16)
    dout = torch.randn(T_, H, device=D).to(torch.bfloat16)
    qkv[own:] = float("nan")    # unowned rows: never read into anything
    dout[own:] = float("nan")
    bqkv = torch.randn(3 * H, device=D) * 0.1
    seqs = T.PackedSeqs(np.cumsum([0] + lens), T_, device=D)
    seed = 987654321
    out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, HEADS, p, seed)
    db = torch.zeros(3 * H, device=D)
    dqkv = T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, db, HEADS, p, seed)

    xr = qkv.float().nan_to_num(0.0).requires_grad_()
    br = bqkv.clone().requires_grad_()
    keep = _keep_masks(seed, lens, T_, seqs.max_seqlen, p) if p > 0 else None
    ref = T.attention_varlen_reference(xr, br, seqs, HEADS, keep, 1.0 / (1.0 - _t16(p) / 65536.0))
    ref.backward(dout.float().nan_to_num(0.0))
    for name, t in (("out", out[:own]), ("lse", lse[:, :own]), ("dqkv", dqkv[:own]), ("dbqkv", db)):
        assert torch.isfinite(t.float()).all(), name
    _close(out[:own], ref[:own], 2e-2, "ctx")
    _close(dqkv[:own], xr.grad[:own], 3e-2, "dqkv")
    _close(db, br.grad, 3e-2, "dbqkv")
    assert not out[own:].any() and not dqkv[own:].any(), "unowned rows must be written as zeros"
    x = xr.detach() + bqkv
    for i, n in enumerate(lens):     # lse as test_fused_attention_lse_matches, per sequence
        s0 = int(seqs.cu_host[i])
        q, k, _ = x[s0:s0 + n].view(n, 3, HEADS, HD).permute(1, 2, 0, 3)
        _close(lse[:, s0:s0 + n], torch.logsumexp((q @ k.transpose(-1, -2)) / math.sqrt(HD), -1), 2e-2, "lse")


@pytest.mark.parametrize("cu,rows,max_seqlen", [
    ([1, 5, 9], 16, 8),      # cu[0] != 0
    ([0, 4, 4, 9], 16, 8),   # a zero-length sequence
    ([0, 6, 3], 16, 8),      # decreasing
    ([0, 8, 16], 12, 8),     # cu[B] > rows
    ([0, 4, 13], 16, 8),     # a length over max_seqlen
    ([0, 4, 9], 16, 8193),   # max_seqlen over 8192
])
def test_varlen_wrapper_refuses(cu, rows, max_seqlen, monkeypatch):
    """Bad tables never reach a launch: PackedSeqs refuses them, and the wrappers refuse a table
    that went bad after construction and a head dim other than 64."""
    from kubeflow_controller_amd.ops import _lib
    from kubeflow_controller_amd.ops import transformer as T
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("launched"))
    with pytest.raises(ValueError):
        T.PackedSeqs(cu, rows, max_seqlen)
    seqs = T.PackedSeqs([0, 4, 9], 16, 8)
    qkv = torch.zeros(16, 3 * 2 * 64, dtype=torch.bfloat16)
    out, lse = torch.zeros(16, 128, dtype=torch.bfloat16), torch.zeros(2, 16)
    with pytest.raises(ValueError):   # d = 32
        T.attn_varlen_fwd(qkv, None, seqs, 4)
    with pytest.raises(ValueError):
        T.attn_varlen_bwd(qkv, None, seqs, out, lse, out, None, 4)
    seqs.cu_host.copy_(torch.tensor(cu, dtype=torch.int32)[:3])
    seqs.rows, seqs.max_seqlen = rows, max_seqlen
    with pytest.raises(ValueError):
        T.attn_varlen_fwd(qkv[:rows], None, seqs, 2)
    with pytest.raises(ValueError):
        T.attn_varlen_bwd(qkv[:rows], None, seqs, out[:rows], lse[:, :rows], out[:rows], None, 2)

"""GPT decoder-only language model (the GPT-1 arrangement: post-LN blocks).

A post-LN decoder block is the project's encoder layer with causal attention, so the
model reuses :class:`~kubeflow_controller_amd.models.bert.BertLayer` parameters and
every fused kernel of :class:`~kubeflow_controller_amd.ops.transformer.EncoderLayerFn`;
attention runs on the causal packed kernels (``csrc/kernels/attention.hip``:
attn_causal_*), which compute only the visible half of the score matrix.

Batches are always packed (:class:`~kubeflow_controller_amd.ops.transformer.PackedSeqs`):
documents of any length back to back in a fixed budget of token rows; a padded batch
of S tokens is the table ``[0, S, 2S, …]``.  The loss is next-token cross-entropy over
the WHOLE row budget: the label of a row is the next token of its sequence, -1 (ignored
by the loss kernel) for a sequence's last token and for the unowned rows.  The decoder
GEMM's M is therefore the row budget, whatever the batch holds, and its route never
changes; the tied decoder keeps a bias (zero-initialised) as BERT's does, because the
loss kernel produces its gradient anyway.

Positions: a learned table added to the token embedding, or with ``GptConfig.rotary`` rotary
position embeddings — no table, every layer rotates Q and K of its QKV projection by the
token's index in its document (``csrc/kernels/rope.hip``), so a score depends on the distance
between query and key only.

Vocabulary is padded to a multiple of 64 (50257 → 50304); padded ids never occur as
inputs or labels.

CPU path: the same parameters through plain PyTorch fp32 ops (no dropout).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import transformer as T
from .bert import BertLayer


@dataclass
class GptConfig:
    vocab_size: int = 50257
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    intermediate: int = 3072
    max_position: int = 1024
    hidden_dropout: float = 0.1
    attn_dropout: float = 0.1
    ln_eps: float = 1e-5
    init_range: float = 0.02
    kv_heads: Optional[int] = None  # grouped-query attention: K / V heads (divides heads; head dim 128 only)
    window: Optional[int] = None    # sliding-window attention: a token sees its last `window` tokens (head dim 128 only)
    rotary: bool = False            # rotary position embeddings on Q and K instead of the learned position table
    rotary_base: float = 10000.0

    @classmethod
    def small(cls) -> "GptConfig":
        return cls()

    @classmethod
    def xl(cls) -> "GptConfig":
        """GPT-3 XL shape: 24 layers of 2048 with 16 heads of 128 (the d = 128 causal kernels);
        1.32 B parameters (24 x 50.4 M of layers + 103 M of tied token and 4 M of position
        embeddings)."""
        return cls(hidden=2048, layers=24, heads=16, intermediate=8192, max_position=2048)

    @classmethod
    def xl_gqa(cls) -> "GptConfig":
        """The ``xl`` shape with grouped-query attention: 16 query heads share 4 K / V heads of 128
        (the QKV projection is [3072, 2048] instead of [6144, 2048])."""
        return cls(hidden=2048, layers=24, heads=16, kv_heads=4, intermediate=8192, max_position=2048)

    @classmethod
    def xl_swa(cls) -> "GptConfig":
        """The ``xl_gqa`` shape for long documents: 8192 positions, each token attending to its
        last 1024 (sliding-window attention: attention cost is linear in the length)."""
        return cls(hidden=2048, layers=24, heads=16, kv_heads=4, intermediate=8192, max_position=8192, window=1024)

    @classmethod
    def xl_rope(cls) -> "GptConfig":
        """The ``xl_gqa`` shape with rotary position embeddings: no learned position table, Q and K
        rotated by in-sequence position before attention (``csrc/kernels/rope.hip``)."""
        return cls(hidden=2048, layers=24, heads=16, kv_heads=4, intermediate=8192, max_position=2048, rotary=True)

    @classmethod
    def tiny(cls) -> "GptConfig":
        return cls(vocab_size=1000, hidden=128, layers=2, heads=2, intermediate=512, max_position=256)

    @property
    def padded_vocab(self) -> int:
        return (self.vocab_size + 63) // 64 * 64


def next_token_labels(input_ids, seqs: T.PackedSeqs):
    """int64 [rows] on the host: row t's label is the token of row t + 1 of the same
    sequence; -1 for every sequence's last token (rows ``cu[1:] - 1``) and the unowned rows."""
    ids = input_ids.reshape(-1).cpu()
    labels = torch.full_like(ids, -1)
    n = seqs.tokens
    labels[:n - 1] = ids[1:n]
    labels[seqs.cu_host[1:].long() - 1] = -1
    return labels


class GptLM(nn.Module):
    def __init__(self, cfg: GptConfig, seed: int = 0):
        super().__init__()
        self.cfg = cfg
        H, V = cfg.hidden, cfg.padded_vocab
        if cfg.kv_heads is not None:
            if cfg.kv_heads < 1 or cfg.heads % cfg.kv_heads:
                raise ValueError(f"GptLM: kv_heads must divide heads (heads={cfg.heads}, kv_heads={cfg.kv_heads})")
            if H != cfg.heads * 128:
                raise ValueError(f"GptLM: grouped-query attention needs head dim 128, got {H / cfg.heads:g} "
                                 f"(hidden={H}, heads={cfg.heads})")
        if cfg.window is not None:
            if cfg.window < 1:
                raise ValueError(f"GptLM: window must be >= 1, got {cfg.window}")
            if H != cfg.heads * 128:
                raise ValueError(f"GptLM: sliding-window attention needs head dim 128, got {H / cfg.heads:g} "
                                 f"(hidden={H}, heads={cfg.heads})")
        if cfg.rotary and (H % cfg.heads or H // cfg.heads not in (64, 128)):
            raise ValueError(f"GptLM: rotary position embeddings need head dim 64 or 128, got {H / cfg.heads:g} "
                             f"(hidden={H}, heads={cfg.heads})")
        self.word_emb = nn.Parameter(torch.empty(V, H))
        nn.init.normal_(self.word_emb, 0.0, cfg.init_range)
        if not cfg.rotary:  # learned positions; with rotary the position enters as a rotation of Q and K
            self.pos_emb = nn.Parameter(torch.empty(cfg.max_position, H))
            nn.init.normal_(self.pos_emb, 0.0, cfg.init_range)
        self._rotary = {}  # device -> RotaryTable, created at the first batch on that device
        self.layers = nn.ModuleList(BertLayer(cfg) for _ in range(cfg.layers))
        self.dec_b = nn.Parameter(torch.zeros(V))
        # the word embedding is written by two direct-gradient kernels per step (lookup
        # and tied decoder), as BertForPreTraining's
        self.word_emb._kfa_uses = 2
        self._kfa_param_uses = {"word_emb": 2}
        self.seed = seed
        self._step = 0

    @property
    def graph_capturable(self) -> bool:
        """The packed batch carries a host sequence table that is checked before every launch."""
        return False

    def rotary_table(self, device) -> Optional[T.RotaryTable]:
        """The model's one :class:`~kubeflow_controller_amd.ops.transformer.RotaryTable` on
        ``device`` (None without ``cfg.rotary``)."""
        cfg = self.cfg
        if not cfg.rotary:
            return None
        key = str(device)
        if key not in self._rotary:
            self._rotary[key] = T.RotaryTable(cfg.hidden // cfg.heads, cfg.max_position, cfg.rotary_base, device)
        return self._rotary[key]

    def forward(self, input_ids, position_ids, seqs, labels):
        """Mean next-token cross-entropy over the rows that have a target.  ``input_ids``,
        ``position_ids``, ``labels`` (:func:`next_token_labels`): flat [rows]; ``seqs``: the table.
        With ``cfg.rotary``, ``position_ids`` is ignored: a row's position is its index in its sequence."""
        cfg = self.cfg
        if seqs.max_seqlen > cfg.max_position:
            raise ValueError(f"GptLM: max_seqlen {seqs.max_seqlen} exceeds max_position {cfg.max_position}")
        rows = input_ids.numel()
        seqs.validate(rows)
        if not input_ids.is_cuda:
            return self.forward_reference(input_ids, position_ids, seqs, labels)
        ph = cfg.hidden_dropout if self.training else 0.0
        pa = cfg.attn_dropout if self.training else 0.0
        step_seed = T.mix_seed(self.seed, self._step)
        if self.training:
            self._step += 1
        rotary = self.rotary_table(input_ids.device)
        if rotary is None:
            h = T.embedding_sum([self.word_emb, self.pos_emb], [input_ids.reshape(-1), position_ids.reshape(-1)])
        else:
            h = T.embedding_sum([self.word_emb], [input_ids.reshape(-1)])
        if ph > 0:
            h = T.dense_dropout(h, ph, T.mix_seed(step_seed, 999))
        join_in = None
        for i, layer in enumerate(self.layers):
            join_out = T.ResidualJoin() if (self.training and i + 1 < len(self.layers)) else None
            lcfg = (seqs.B, seqs.max_seqlen, cfg.heads, ph, pa, T.s64(T.mix_seed(step_seed, i)), cfg.ln_eps, join_in,
                    join_out, seqs, True, cfg.kv_heads, cfg.window) + ((rotary,) if rotary is not None else ())
            h = T.EncoderLayerFn.apply(h, None, lcfg, *layer.params())
            join_in = join_out
        # decoder_xent means over all rows (ignored rows add 0): rescale to the rows with a
        # target, a host integer (every sequence has len - 1 of them)
        targets = seqs.tokens - seqs.B
        if targets <= 0:
            raise ValueError("GptLM: no row has a target (every sequence is a single token)")
        return T.decoder_xent(h, self.word_emb, self.dec_b, labels.reshape(-1)) * (rows / targets)

    def forward_reference(self, input_ids, position_ids, seqs, labels):
        """Plain PyTorch fp32, no dropout (CPU replicas + numerics reference)."""
        cfg = self.cfg
        f = lambda t: t.float()  # noqa: E731
        rotary = self.rotary_table(input_ids.device)
        h = f(self.word_emb)[input_ids.reshape(-1)]
        if rotary is None:
            h = h + f(self.pos_emb)[position_ids.reshape(-1)]
        lcfg = (seqs.B, seqs.max_seqlen, cfg.heads, 0.0, 0.0, 0, cfg.ln_eps, None, None, seqs, True, cfg.kv_heads,
                cfg.window) + ((rotary,) if rotary is not None else ())
        for layer in self.layers:
            h = T.encoder_layer_reference(h, None, lcfg, *layer.params())
        logits = h @ f(self.word_emb).t() + f(self.dec_b)
        return F.cross_entropy(logits, labels.reshape(-1), ignore_index=-1)


def gpt_loss(model, *batch):
    return model(*batch)


def synthetic_lm_batch(cfg: GptConfig, rows: int, seq_len: int, min_len: int, generator=None, device="cpu"):
    """Random documents in the style of ``synthetic_packed_mlm_batch``: lengths uniform in
    [min_len, seq_len], added while they fit in ``rows`` token rows (the remainder stays
    unowned).  Returns the positional args of :meth:`GptLM.forward`."""
    g = generator
    if not 2 <= min_len <= seq_len <= rows:
        raise ValueError(f"synthetic_lm_batch: need 2 <= min_len <= seq_len <= rows, got {min_len}, {seq_len}, {rows}")
    lens = []
    while True:
        n = int(torch.randint(min_len, seq_len + 1, (1,), generator=g))
        if sum(lens) + n > rows:
            break
        lens.append(n)
    cu = torch.tensor([0] + lens).cumsum(0)
    ids = torch.zeros(rows, dtype=torch.int64)
    ids[:cu[-1]] = torch.randint(0, cfg.vocab_size, (int(cu[-1]),), generator=g)
    pos_ids = torch.zeros(rows, dtype=torch.int64)
    for i, n in enumerate(lens):
        pos_ids[int(cu[i]):int(cu[i]) + n] = torch.arange(n)
    seqs = T.PackedSeqs(cu, rows, seq_len, device)
    to = lambda t: t.to(device)  # noqa: E731
    return to(ids), to(pos_ids), seqs, to(next_token_labels(ids, seqs))


def flops_per_step(cfg: GptConfig, lens) -> float:
    """Model FLOPs (fwd+bwd = 3x fwd) of one step on sequences of ``lens`` tokens; attention
    counts the visible half of each score matrix (with ``window`` the visible band,
    ``Σ_i min(i + 1, window)`` pairs per sequence); with ``kv_heads`` the QKV projection is
    ``(heads + 2·kv_heads)·d`` wide."""
    Tk = float(sum(lens))
    H, I, L = cfg.hidden, cfg.intermediate, cfg.layers
    W = cfg.window
    # pairs of a sequence of n tokens: rows 0..m-1 see i + 1 keys, the other n - m rows see W, m = min(n, W)
    pairs = [n * (n + 1) / 2 if W is None else min(n, W) * (min(n, W) + 1) / 2 + (n - min(n, W)) * W for n in lens]
    attn = sum(2 * 2 * pr * H for pr in pairs)
    Wqkv = 3 * H if cfg.kv_heads is None else H + 2 * cfg.kv_heads * (H // cfg.heads)
    per_layer = 2 * Tk * (Wqkv * H + H * H + 2 * H * I) + attn
    return 3.0 * (L * per_layer + 2 * Tk * H * cfg.padded_vocab)

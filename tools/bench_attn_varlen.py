"""Packed (varlen) vs padded attention and BERT-base training step, sides alternated in one run.

    python tools/bench_attn_varlen.py [--rounds 5] [--no-step]

attention  one BERT-base layer (12 heads, dropout 0.1), 256 sequences with lengths uniform in
           [16, 128]: fwd + bwd of the S = 128 kernels on the padded [256, 128] batch (key bias on
           the pad keys) against the varlen kernels on the same sequences packed into sum(len) rows.
step       one Engine step of BERT-base on synthetic_mlm_batch(256, 128) against
           synthetic_packed_mlm_batch(rows = 256·128, lengths uniform in [16, 128]).
Each round times every side once (events around 20 calls / 5 steps); prints per-side min and
median over the rounds.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kubeflow_controller_amd.ops import transformer as T  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate_rounds(sides, rounds, iters):
    """{side: [ms per call of each round]}: every round times every side once, in turn."""
    for fn in sides.values():  # warm-up: code objects, workspaces, the GEMM tuner's choices
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, iters))
    return t


def alternate(sides, rounds, iters):
    return {k: (min(v), statistics.median(v)) for k, v in alternate_rounds(sides, rounds, iters).items()}


def gqa(rounds, kv_heads):
    """--head-dim 128 --kv-heads K: 16 query heads of 128 (H = 2048, dropout 0.1), grouped-query
    attention with K KV heads against the multi-head d = 128 kernels at the same query heads (the
    same Q columns; K / V head c of the GQA batch is head c·g of the MHA batch), bidirectional and
    causal: 32 sequences of 1024 tokens, and lengths uniform in [128, 1024].  The ratio is taken
    per round (both sides timed back to back) and its spread over the rounds is printed."""
    d = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    h, hd, p, S = 16, 128, 0.1, 1024
    H, grp = h * hd, h // kv_heads
    for name, lens in (("32 x 1024", torch.full((32,), S)), ("32, uniform in [128, 1024]",
                                                            torch.randint(128, S + 1, (32,), generator=g))):
        rows = int(lens.sum())
        seqs = T.PackedSeqs(torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)]), rows, S, d)
        mha = torch.randn(rows, 3, h, hd, device=d).to(torch.bfloat16)
        qkv = {"mha": mha.view(rows, 3 * H),
               "gqa": torch.cat([mha[:, 0].reshape(rows, H), mha[:, 1, ::grp].reshape(rows, -1),
                                 mha[:, 2, ::grp].reshape(rows, -1)], 1).contiguous()}
        kvh = {"mha": None, "gqa": kv_heads}
        dout = torch.randn(rows, H, device=d).to(torch.bfloat16)

        def fwd(k, c):
            return T.attn_varlen_fwd(qkv[k], None, seqs, h, p, 7, causal=c, kv_heads=kvh[k])

        def both(k, c):
            out, lse = fwd(k, c)
            T.attn_varlen_bwd(qkv[k], None, seqs, out, lse, dout, None, h, p, 7, causal=c, kv_heads=kvh[k])

        sides = {}
        for c in (False, True):
            for k in ("mha", "gqa"):  # the default arguments bind this iteration's values
                sides[("causal" if c else "bidir", k, "fwd")] = lambda k=k, c=c: fwd(k, c)
                sides[("causal" if c else "bidir", k, "fwd+bwd")] = lambda k=k, c=c: both(k, c)
        t = alternate_rounds(sides, rounds, 20)
        print(f"attention, {name}: {rows} rows, {h} query heads of {hd}, {kv_heads} KV heads")
        for (c, k, w), v in t.items():
            print(f"  {c:6s} {k} {w:8s} min {min(v) * 1e3:7.1f} us  median {statistics.median(v) * 1e3:7.1f} us", flush=True)
        for c in ("bidir", "causal"):
            for w in ("fwd", "fwd+bwd"):
                r = [a / b for a, b in zip(t[(c, "gqa", w)], t[(c, "mha", w)])]
                print(f"  {c} {w}: gqa / mha = {statistics.median(r):.3f} (median of the per-round ratios; "
                      f"min {min(r):.3f}, max {max(r):.3f})")


def rope(rounds):
    """--rope: the two rotary passes (rope_qk_ forward on qkv with its bias, inverse on dqkv) on 32
    sequences of 1024 tokens at 16 query / 4 KV heads of 128, each against the bytes it moves, and
    causal grouped-query attention fwd + bwd (dropout 0.1) with and without the two passes.  A pass
    reads and writes the (heads + kv_heads)·d rotated bf16 columns of every row once; the cos / sin
    table (one 64-byte read per lane and row) and the bias are counted too."""
    d = torch.device("cuda")
    torch.manual_seed(0)
    h, kvh, hd, p, S, B = 16, 4, 128, 0.1, 1024, 32
    rows, W = B * S, (h + 2 * kvh) * hd
    seqs = T.PackedSeqs(torch.arange(B + 1) * S, rows, S, d)
    rot = T.RotaryTable(hd, S, device=d)
    qkv = torch.randn(rows, W, device=d).to(torch.bfloat16)
    dqkv = torch.randn(rows, W, device=d).to(torch.bfloat16)
    dout = torch.randn(rows, h * hd, device=d).to(torch.bfloat16)
    bqkv = torch.randn(W, device=d) * 0.01

    def attn(with_rope):
        b = T.rope_qk_(qkv, bqkv, seqs, h, rot, kvh) if with_rope else bqkv
        out, lse = T.attn_varlen_fwd(qkv, b, seqs, h, p, 7, causal=True, kv_heads=kvh)
        g = T.attn_varlen_bwd(qkv, b, seqs, out, lse, dout, None, h, p, 7, causal=True, kv_heads=kvh)
        if with_rope:
            T.rope_qk_(g, None, seqs, h, rot, kvh, inverse=True)

    sides = {"rope_qk fwd": lambda: T.rope_qk_(qkv, bqkv, seqs, h, rot, kvh),
             "rope_qk inverse": lambda: T.rope_qk_(dqkv, None, seqs, h, rot, kvh, inverse=True),
             "attention fwd+bwd": lambda: attn(False), "attention fwd+bwd + rope": lambda: attn(True)}
    t = alternate_rounds(sides, rounds, 20)
    data = 2 * rows * (h + kvh) * hd * 2            # the rotated columns, read and written
    table = rows * (hd // 2) * 2 * 4                # every row's cos / sin line
    moved = {"rope_qk fwd": data + table + 2 * W * 4, "rope_qk inverse": data + table}
    print(f"rotary passes, {B} x {S}: {rows} rows, {h} query / {kvh} KV heads of {hd}")
    for k, v in t.items():
        bw = f"  {moved[k] / 1e6:6.1f} MB moved, {moved[k] / min(v) / 1e9:5.2f} TB/s at the min" if k in moved else ""
        print(f"  {k:26s} min {min(v) * 1e3:7.1f} us  median {statistics.median(v) * 1e3:7.1f} us{bw}", flush=True)
    r = [a - b for a, b in zip(t["attention fwd+bwd + rope"], t["attention fwd+bwd"])]
    print(f"  attention with the passes - without: {statistics.median(r) * 1e3:.1f} us (median of the per-round "
          f"differences; min {min(r) * 1e3:.1f}, max {max(r) * 1e3:.1f})")


def window(rounds, windows):
    """--head-dim 128 --causal --window W [W ...]: sliding-window causal attention against full causal
    attention of the same build on the same batch, 16 query heads of 128 (dropout 0.1), multi-head and
    grouped-query with 4 KV heads: 4 sequences of 8192 tokens, 16 of 2048, and 8 with lengths uniform
    in [1024, 8192].  Ratios are taken per round (both sides timed back to back) and printed with their
    spread next to the ratio of visible (query, key) pairs, which is the ideal."""
    d = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    h, hd, p, S = 16, 128, 0.1, 8192
    H = h * hd
    for name, lens in (("4 x 8192", torch.full((4,), 8192)), ("16 x 2048", torch.full((16,), 2048)),
                       ("8, uniform in [1024, 8192]", torch.randint(1024, S + 1, (8,), generator=g))):
        rows = int(lens.sum())
        # max_seqlen is the longest sequence: a window that covers it runs the causal kernels
        seqs = T.PackedSeqs(torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)]), rows, None, d)
        dout = torch.randn(rows, H, device=d).to(torch.bfloat16)
        print(f"attention, {name}: {rows} rows, {h} query heads of {hd}")
        for kvh in (h, 4):
            qkv = torch.randn(rows, (h + 2 * kvh) * hd, device=d).to(torch.bfloat16)

            def fwd(w):
                return T.attn_varlen_fwd(qkv, None, seqs, h, p, 7, causal=True, kv_heads=kvh, window=w)

            def both(w):
                out, lse = fwd(w)
                T.attn_varlen_bwd(qkv, None, seqs, out, lse, dout, None, h, p, 7, causal=True, kv_heads=kvh, window=w)

            sides = {}
            for w in [None] + list(windows):  # the default arguments bind this iteration's values
                sides[(w, "fwd")] = lambda w=w: fwd(w)
                sides[(w, "fwd+bwd")] = lambda w=w: both(w)
            t = alternate_rounds(sides, rounds, 5)
            print(f"  {kvh} KV heads")
            for (w, k), v in t.items():
                print(f"    {'causal' if w is None else 'W = %d' % w:10s} {k:8s} min {min(v):8.3f} ms  "
                      f"median {statistics.median(v):8.3f} ms", flush=True)
            full = float((lens * (lens + 1) / 2).sum())
            for w in windows:
                m = lens.clamp(max=w)
                ideal = float((m * (m + 1) / 2 + (lens - m) * w).sum()) / full
                for k in ("fwd", "fwd+bwd"):
                    r = [a / b for a, b in zip(t[(w, k)], t[(None, k)])]
                    print(f"    W = {w} {k}: window / causal = {statistics.median(r):.3f} (median of the per-round "
                          f"ratios; min {min(r):.3f}, max {max(r):.3f}); visible pairs {ideal:.3f}")


def head_dims(rounds):
    """--head-dim 128: one layer's attention at H = 768, dropout 0.1: 6 heads of 128
    (attention_d128.hip) against 12 heads of 64 on the SAME packed qkv (equal FLOPs), bidirectional
    and causal: 32 sequences of 1024 tokens, and lengths uniform in [128, 1024]."""
    d = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    H, p, S = 768, 0.1, 1024
    for name, lens in (("32 x 1024", torch.full((32,), S)), ("32, uniform in [128, 1024]",
                                                            torch.randint(128, S + 1, (32,), generator=g))):
        rows = int(lens.sum())
        seqs = T.PackedSeqs(torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)]), rows, S, d)
        qkv = torch.randn(rows, 3 * H, device=d).to(torch.bfloat16)
        dout = torch.randn(rows, H, device=d).to(torch.bfloat16)
        bqkv = torch.randn(3 * H, device=d) * 0.1

        def fwd(h, c):
            return T.attn_varlen_fwd(qkv, bqkv, seqs, h, p, 7, causal=c)

        def both(h, c):
            out, lse = fwd(h, c)
            T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, None, h, p, 7, causal=c)

        sides = {}
        for c in (False, True):
            for hd in (64, 128):  # the default arguments bind this iteration's values
                sides[("causal" if c else "bidir", hd, "fwd")] = lambda h=H // hd, c=c: fwd(h, c)
                sides[("causal" if c else "bidir", hd, "fwd+bwd")] = lambda h=H // hd, c=c: both(h, c)
        r = alternate(sides, rounds, 20)
        print(f"attention, {name}: {rows} rows, H = {H}")
        for (c, hd, k), (lo, med) in r.items():
            print(f"  {c:6s} d = {hd:3d} {k:8s} min {lo * 1e3:7.1f} us  median {med * 1e3:7.1f} us", flush=True)
        for c in ("bidir", "causal"):
            for k in ("fwd", "fwd+bwd"):
                print(f"  {c} {k}: d128 / d64 = {r[(c, 128, k)][0] / r[(c, 64, k)][0]:.3f} (min), "
                      f"{r[(c, 128, k)][1] / r[(c, 64, k)][1]:.3f} (median)")


def causal(rounds, hd=64):
    """--causal: one BERT-base-shaped layer (H = 768: 12 heads of 64, or 6 of 128 with --head-dim 128;
    dropout 0.1), the causal kernels against the bidirectional varlen kernels on the SAME packed
    batch: 32 sequences of 1024 tokens, and lengths uniform in [128, 1024]."""
    d = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    h, p, S = 768 // hd, 0.1, 1024
    H = h * hd
    for name, lens in (("32 x 1024", torch.full((32,), S)), ("32, uniform in [128, 1024]",
                                                            torch.randint(128, S + 1, (32,), generator=g))):
        rows = int(lens.sum())
        seqs = T.PackedSeqs(torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)]), rows, S, d)
        qkv = torch.randn(rows, 3 * H, device=d).to(torch.bfloat16)
        dout = torch.randn(rows, H, device=d).to(torch.bfloat16)
        bqkv = torch.randn(3 * H, device=d) * 0.1

        def both(c):
            out, lse = T.attn_varlen_fwd(qkv, bqkv, seqs, h, p, 7, causal=c)
            T.attn_varlen_bwd(qkv, bqkv, seqs, out, lse, dout, None, h, p, 7, causal=c)

        sides = {"bidirectional fwd": lambda: T.attn_varlen_fwd(qkv, bqkv, seqs, h, p, 7),
                 "causal fwd": lambda: T.attn_varlen_fwd(qkv, bqkv, seqs, h, p, 7, causal=True),
                 "bidirectional fwd+bwd": lambda: both(False), "causal fwd+bwd": lambda: both(True)}
        r = alternate(sides, rounds, 20)
        nb = (lens + 127) // 128
        print(f"attention, {name}: {rows} rows; 128-row blocks streamed causal / bidirectional = "
              f"{float((nb * (nb + 1) / 2).sum() / (nb * nb).sum()):.4f}")
        for k, (lo, med) in r.items():
            print(f"  {k:22s} min {lo * 1e3:7.1f} us  median {med * 1e3:7.1f} us", flush=True)
        for k in ("fwd", "fwd+bwd"):
            print(f"  causal / bidirectional {k}: {r['causal ' + k][0] / r['bidirectional ' + k][0]:.3f} (min over rounds)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--causal", action="store_true", help="causal vs bidirectional varlen kernels at 1024 tokens")
    ap.add_argument("--head-dim", type=int, default=64, choices=[64, 128],
                    help="128: d = 128 (6 heads) against d = 64 (12 heads) at H = 768; with --causal: the head dim of "
                         "that comparison")
    ap.add_argument("--kv-heads", type=int, default=None,
                    help="with --head-dim 128: grouped-query attention with this many KV heads against the multi-head "
                         "kernels, both at 16 query heads")
    ap.add_argument("--window", type=int, nargs="+", default=None,
                    help="with --head-dim 128 --causal: sliding-window attention with these windows against full "
                         "causal attention, multi-head and grouped-query, up to 8192 tokens")
    ap.add_argument("--rope", action="store_true",
                    help="the rotary position-embedding passes (rope_qk_ forward and inverse) at 16 query / 4 KV "
                         "heads of 128, alone and around causal grouped-query attention")
    args = ap.parse_args()
    if args.rope:
        return rope(args.rounds)
    if args.window is not None:
        if args.head_dim != 128 or not args.causal or min(args.window) < 1:
            ap.error("--window needs --head-dim 128 --causal and windows >= 1")
        return window(args.rounds, args.window)
    if args.kv_heads is not None:
        if args.head_dim != 128 or args.kv_heads < 1 or 16 % args.kv_heads:
            ap.error("--kv-heads needs --head-dim 128 and a divisor of the 16 query heads")
        return gqa(args.rounds, args.kv_heads)
    if args.causal:
        return causal(args.rounds, args.head_dim)
    if args.head_dim == 128:
        return head_dims(args.rounds)
    d = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    B, S, h, p = 256, 128, 12, 0.1
    H = h * 64
    lens = torch.randint(16, S + 1, (B,), generator=g)
    live = int(lens.sum())
    cu = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    seqs = T.PackedSeqs(cu, live, S, d)
    keep = (torch.arange(S)[None, :] < lens[:, None])
    kb = ((~keep).float() * -10000.0).to(d).contiguous()
    qkv_pad = torch.randn(B * S, 3 * H, device=d).to(torch.bfloat16)
    qkv_pk = qkv_pad[keep.reshape(-1).to(d)].contiguous()
    bqkv = torch.randn(3 * H, device=d) * 0.1
    do_pad = torch.randn(B * S, H, device=d).to(torch.bfloat16)
    do_pk = do_pad[keep.reshape(-1).to(d)].contiguous()

    def padded():
        out, lse = T.attn_fwd(qkv_pad, bqkv, kb, B, S, h, p, 7)
        T.attn_bwd(qkv_pad, bqkv, kb, out, lse, do_pad, None, B, S, h, p, 7)

    def packed():
        out, lse = T.attn_varlen_fwd(qkv_pk, bqkv, seqs, h, p, 7)
        T.attn_varlen_bwd(qkv_pk, bqkv, seqs, out, lse, do_pk, None, h, p, 7)

    sides = {"padded fwd": lambda: T.attn_fwd(qkv_pad, bqkv, kb, B, S, h, p, 7),
             "packed fwd": lambda: T.attn_varlen_fwd(qkv_pk, bqkv, seqs, h, p, 7),
             "padded fwd+bwd": padded, "packed fwd+bwd": packed}
    r = alternate(sides, args.rounds, 20)
    print(f"attention: {B} sequences, lengths uniform in [16, {S}] (min {int(lens.min())}, max {int(lens.max())}), "
          f"{live} live of {B * S} padded rows (f = {live / (B * S):.3f})")
    for k, (lo, med) in r.items():
        rows = live if k.startswith("packed") else B * S
        print(f"  {k:15s} min {lo * 1e3:7.1f} us  median {med * 1e3:7.1f} us  ({lo * 1e6 / rows:6.2f} ns per row of its batch, "
              f"{lo * 1e6 / live:6.2f} ns per live token)", flush=True)
    if args.no_step:
        return
    from kubeflow_controller_amd.models.bert import (BertConfig, BertForPreTraining, bert_loss, synthetic_mlm_batch,
                                                     synthetic_packed_mlm_batch)
    from kubeflow_controller_amd.trainer.engine import DistInfo, Engine
    cfg = BertConfig.base()
    eng = Engine(BertForPreTraining(cfg), bert_loss, optimizer="adam", lr=1e-4, weight_decay=0.01,
                 dist_info=DistInfo(device=d), channels_last=False)
    pad_b = synthetic_mlm_batch(cfg, B, S, g, d)
    pk_b = synthetic_packed_mlm_batch(cfg, B * S, S, 16, g, d)
    r = alternate({"padded": lambda: eng.train_step(*pad_b), "packed": lambda: eng.train_step(*pk_b)}, args.rounds, 5)
    nseq = {"padded": B, "packed": pk_b[3].B}
    toks = {"padded": B * S, "packed": pk_b[3].tokens}
    print(f"BERT-base step, {B * S} rows: padded {B} x {S} (every row live) vs packed {nseq['packed']} sequences "
          f"({toks['packed']} live tokens, lengths uniform in [16, {S}])")
    for k, (lo, med) in r.items():
        print(f"  {k:7s} min {lo:7.2f} ms  median {med:7.2f} ms  {nseq[k] / lo * 1e3:8.0f} sequences/s  "
              f"{toks[k] / lo * 1e3 / 1e6:6.3f} M live tokens/s", flush=True)


if __name__ == "__main__":
    main()

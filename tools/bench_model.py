#!/usr/bin/env python3
"""Throughput of the non-headline BASELINE.json configs (BERT-base pre-training,
Wide&Deep) on MI355X: same contract as ``bench.py`` (W warmup, K timed full
steps bracketed by barrier + device sync, MAX over ranks, ONE JSON line).

    python tools/bench_model.py --model bert_base --batch 64 --seq 128
    torchrun --nproc-per-node N tools/bench_model.py --model bert_base --ps 2

``--ps P`` runs the parameter-server layout (P shard owners, reduce-scatter
push / owner-side fused Adam / all-gather pull) instead of all-reduce.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubeflow_controller_amd.trainer.engine import Engine, init_distributed, timed_steps  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model", default="bert_base", choices=["bert_base", "bert_large", "bert_tiny", "gpt_small",
                                                             "gpt_xl", "gpt_xl_gqa", "gpt_xl_swa", "gpt_xl_rope", "gpt_tiny", "wide_deep", "wide_deep_tiny"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default 64; gpt: 8, gpt_xl: 4)")
    ap.add_argument("--seq", type=int, default=None, help="sequence length (default 128; gpt_small: 1024, gpt_xl: 2048, the longest "
                    "document of a packed batch of batch * seq token rows)")
    ap.add_argument("--min-seq", type=int, default=128, help="gpt: the shortest document")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--ps", type=int, default=0, help="parameter-server shard owners (0 = all-reduce)")
    ap.add_argument("--bucket-mb", type=float, default=32.0)
    ap.add_argument("--optimizer", default="adam", choices=["adam", "lamb"])
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip the gradient to this global L2 norm (all-reduce layout only)")
    args = ap.parse_args(argv)
    gpt = args.model.startswith("gpt")
    # gpt_small: 8 x 1024 = 8192 rows keeps the bf16 logits and their gradient (rows x 50304 each) at 0.8 GB apiece
    # gpt_xl: the same 8192-row budget as 4 x 2048 (its max_position), so the logits cost what gpt_small's do
    # gpt_xl_swa: the same budget as 1 x 8192 (its max_position)
    xl_rows = 1 if args.model == "gpt_xl_swa" else 4
    args.batch = args.batch if args.batch is not None else ((xl_rows if args.model.startswith("gpt_xl") else 8) if gpt else 64)
    args.seq = args.seq if args.seq is not None else {"gpt_small": 1024, "gpt_xl": 2048, "gpt_xl_gqa": 2048, "gpt_xl_rope": 2048, "gpt_xl_swa": 8192}.get(args.model, 128)
    info = init_distributed()
    if info.device.type != "cuda":
        raise SystemExit("bench_model.py needs an MI355X")
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(1234 + info.rank)
    if args.model.startswith("bert"):
        from kubeflow_controller_amd.models.bert import (BertConfig, BertForPreTraining, bert_loss, flops_per_step,
                                                         synthetic_mlm_batch)
        cfg = {"bert_base": BertConfig.base, "bert_large": BertConfig.large, "bert_tiny": BertConfig.tiny}[args.model]()
        model = BertForPreTraining(cfg)
        batch = synthetic_mlm_batch(cfg, args.batch, args.seq, g, info.device)
        loss_fn, unit, flops = bert_loss, "sequences/sec", flops_per_step(cfg, args.batch, args.seq)
        metric = f"{args.model} pre-training sequences/sec (seq {args.seq}, whole node)"
    elif gpt:
        from kubeflow_controller_amd.models.gpt import GptConfig, GptLM, flops_per_step, gpt_loss, synthetic_lm_batch
        cfg = {"gpt_small": GptConfig.small, "gpt_xl": GptConfig.xl, "gpt_xl_gqa": GptConfig.xl_gqa,
               "gpt_xl_swa": GptConfig.xl_swa, "gpt_xl_rope": GptConfig.xl_rope, "gpt_tiny": GptConfig.tiny}[args.model]()
        model = GptLM(cfg)
        batch = synthetic_lm_batch(cfg, args.batch * args.seq, args.seq, min(args.min_seq, args.seq), g, info.device)
        cu = batch[2].cu_host
        loss_fn, unit, flops = gpt_loss, "sequences/sec", flops_per_step(cfg, (cu[1:] - cu[:-1]).tolist())
        metric = (f"{args.model} LM training sequences/sec ({batch[2].B} packed documents of {args.min_seq}..{args.seq} "
                  f"tokens, {batch[2].tokens} live of {args.batch * args.seq} rows, whole node)")
        args.batch = batch[2].B  # sequences per step
    else:
        from kubeflow_controller_amd.models.wide_deep import (WideDeep, WideDeepConfig, prepare_batch, synthetic_batch,
                                                              wide_deep_loss)
        cfg = WideDeepConfig() if args.model == "wide_deep" else WideDeepConfig.tiny()
        model = WideDeep(cfg, device=info.device)
        batch = prepare_batch(model, *synthetic_batch(cfg, args.batch, g, "cpu"), info.device)
        loss_fn, unit, flops = wide_deep_loss, "examples/sec", None
        metric = f"{args.model} training examples/sec (whole node)"
    engine = Engine(model, loss_fn, optimizer=args.optimizer, lr=args.lr, weight_decay=0.01, bucket_mb=args.bucket_mb,
                    dist_info=info, channels_last=False, ps=args.ps, max_grad_norm=args.max_grad_norm)
    from kubeflow_controller_amd.ops import routes as _routes
    r = timed_steps(engine, batch, args.steps, args.warmup)
    ms = r["elapsed"] / args.steps * 1e3
    value = args.batch * info.world * args.steps / r["elapsed"]
    if info.rank == 0:
        out = {"metric": metric, "value": round(value, 2), "unit": unit, "n_gpus": info.world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "bf16", "data": "synthetic (random ids / features, random-init weights)",
               "config": {"model": args.model, "global_batch": args.batch * info.world,
                          "seq_len": args.seq if args.model.startswith(("bert", "gpt")) else None,
                          "parallelism": (f"{info.world}w+{args.ps}ps" if args.ps else f"dp{info.world}"),
                          "optimizer": args.optimizer, "max_grad_norm": args.max_grad_norm,
                          "routes": _routes.summary(), "loss": r["loss"]}}
        if flops:
            out["tflops_per_gpu"] = round(flops / (ms / 1e3) / 1e12, 1)
        print(json.dumps(out), flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Optimizer-step time on a model's flat groups: FusedAdam against FusedLAMB, each
with and without global-norm clipping, in ONE process, the variants alternating
round by round (device events around each whole ``step()``; median, min and max
over the rounds).  Bytes are what the algorithm needs, from the shapes:

    Adam     read g, w, m, v; write m, v, w, wb
    LAMB     stage 1: read g, w, m, v; write m, v.  stage 2: read w, m, v; write w, wb
    clip     + one read of g

    python tools/bench_optim_step.py --model bert_base --rounds 30
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def step_bytes(groups, kind: str, clip: bool) -> int:
    n = 0
    for g in groups:
        ge = g.opt_grad.element_size()
        wb = g.data.element_size() if g.master is not None else 0
        per = ge + 12 + 12 + wb  # Adam
        if kind == "lamb":
            per = (ge + 12 + 8) + (12 + 4 + wb)
        if clip:
            per += ge
        n += per * g.numel
    return n


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="bert_base", choices=["bert_base", "bert_large", "bert_tiny"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_step.py needs an MI355X")
    from kubeflow_controller_amd.models.bert import BertConfig, BertForPreTraining
    from kubeflow_controller_amd.ops.optim import FusedAdam, FusedLAMB
    from kubeflow_controller_amd.parallel.flat import split_params
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = {"bert_base": BertConfig.base, "bert_large": BertConfig.large, "bert_tiny": BertConfig.tiny}[args.model]()
    variants = {}
    for name, cls, clip in (("adam", FusedAdam, None), ("adam_clip", FusedAdam, 1.0), ("lamb", FusedLAMB, None),
                            ("lamb_clip", FusedLAMB, 1.0)):
        torch.manual_seed(0)
        groups = split_params(BertForPreTraining(cfg).to(dev), torch.bfloat16)
        for g in groups:  # the gradient of a training step is not needed: any finite values move the same bytes
            g.grad.copy_(torch.randn(g.numel, device=dev) * 1e-3)
            for a, b in zip([o + p.numel() for o, p in zip(g.offsets, g.params)], g.offsets[1:] + [g.numel]):
                g.grad[a:b] = 0
        opt = cls(groups, lr=1e-4, weight_decay=0.01, max_grad_norm=clip)
        variants[name] = (groups, opt, step_bytes(groups, "lamb" if cls is FusedLAMB else "adam", clip is not None))
    for _, opt, _ in variants.values():
        for _ in range(args.warmup):
            opt.step()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (_, opt, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                opt.step()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.inner)
    out = {"model": args.model, "elements": sum(g.numel for g in variants["adam"][0]), "rounds": args.rounds,
           "inner": args.inner, "variants": {}}
    for k, ts in times.items():
        med = statistics.median(ts)
        out["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                              "bytes": variants[k][2], "tb_per_s": round(variants[k][2] / (med * 1e-3) / 1e12, 3)}
    a = out["variants"]["adam"]
    out["lamb_over_adam"] = round(out["variants"]["lamb"]["ms_median"] / a["ms_median"], 4)
    out["adam_spread"] = round((a["ms_max"] - a["ms_min"]) / a["ms_median"], 4)
    out["bytes_ratio"] = round(out["variants"]["lamb"]["bytes"] / a["bytes"], 4)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

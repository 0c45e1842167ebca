#!/usr/bin/env python3
"""Optimizer-step time on a model's flat groups: FusedAdam against FusedLAMB (the BERT
models) or FusedSGD against FusedLARS (``--model resnet50``), each with and without
global-norm clipping, in ONE process, the variants alternating round by round (device
events around each whole ``step()``; median, min and max over the rounds).  Bytes are
what the algorithm needs, from the shapes:

    Adam     read g, w, m, v; write m, v, w, wb
    LAMB     stage 1: read g, w, m, v; write m, v.  stage 2: read w, m, v; write w, wb
    SGD      read g, w, mom; write mom, w, wb
    LARS     SGD's pass, and on the adapting groups a norms pass before it: read g, w
    clip     + one read of g (LARS: only on the groups that do not adapt; the
             adapting groups' norms pass already leaves the g^2 partials)

FusedSGD takes no clipping, so ``sgd_clip`` is ``FusedLARS(adapt_groups=())``: the
same update kernel as ``lars`` with every rate 1, and the g^2 pass over every group.

    python tools/bench_optim_step.py --model bert_base --rounds 30
    python tools/bench_optim_step.py --model resnet50 --rounds 30
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
        if kind in ("sgd", "lars"):
            per = ge + 8 + 8 + wb
        norms = kind == "lars" and g.name == "weights"  # the norms pass of an adapting group: g and w once more
        if norms:
            per += ge + 4
        if clip and not norms:
            per += ge
        n += per * g.numel
    return n


def _model(name: str):
    if name == "resnet50":
        from kubeflow_controller_amd.models.resnet import resnet50
        return resnet50()
    from kubeflow_controller_amd.models.bert import BertConfig, BertForPreTraining
    return BertForPreTraining({"bert_base": BertConfig.base, "bert_large": BertConfig.large,
                               "bert_tiny": BertConfig.tiny}[name]())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="bert_base", choices=["bert_base", "bert_large", "bert_tiny", "resnet50"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_step.py needs an MI355X")
    from kubeflow_controller_amd.ops.optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD
    from kubeflow_controller_amd.parallel.flat import split_params
    dev = torch.device("cuda")
    torch.manual_seed(0)
    if args.model == "resnet50":  # (name, bytes kind, constructor, clip)
        hp = dict(lr=0.1, momentum=0.9, weight_decay=5e-5)
        table = (("sgd", "sgd", lambda g, c: FusedSGD(g, **hp), None),
                 ("sgd_clip", "sgd", lambda g, c: FusedLARS(g, adapt_groups=(), max_grad_norm=c, **hp), 1.0),
                 ("lars", "lars", lambda g, c: FusedLARS(g, max_grad_norm=c, **hp), None),
                 ("lars_clip", "lars", lambda g, c: FusedLARS(g, max_grad_norm=c, **hp), 1.0))
    else:
        hp = dict(lr=1e-4, weight_decay=0.01)
        table = (("adam", "adam", lambda g, c: FusedAdam(g, max_grad_norm=c, **hp), None),
                 ("adam_clip", "adam", lambda g, c: FusedAdam(g, max_grad_norm=c, **hp), 1.0),
                 ("lamb", "lamb", lambda g, c: FusedLAMB(g, max_grad_norm=c, **hp), None),
                 ("lamb_clip", "lamb", lambda g, c: FusedLAMB(g, max_grad_norm=c, **hp), 1.0))
    base, other = table[0][0], table[2][0]
    variants = {}
    for name, kind, make, clip in table:
        torch.manual_seed(0)
        groups = split_params(_model(args.model).to(dev), torch.bfloat16)
        for g in groups:  # the gradient of a training step is not needed: any finite values move the same bytes
            g.grad.copy_(torch.randn(g.numel, device=dev) * 1e-3)
            for a, b in zip([o + p.numel() for o, p in zip(g.offsets, g.params)], g.offsets[1:] + [g.numel]):
                g.grad[a:b] = 0
        variants[name] = (groups, make(groups, clip), step_bytes(groups, kind, clip is not None))
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
    out = {"model": args.model, "elements": sum(g.numel for g in variants[base][0]), "rounds": args.rounds,
           "inner": args.inner, "variants": {}}
    for k, ts in times.items():
        med = statistics.median(ts)
        out["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                              "bytes": variants[k][2], "tb_per_s": round(variants[k][2] / (med * 1e-3) / 1e12, 3)}
    a = out["variants"][base]
    out[f"{other}_over_{base}"] = round(out["variants"][other]["ms_median"] / a["ms_median"], 4)
    out[f"{base}_spread"] = round((a["ms_max"] - a["ms_min"]) / a["ms_median"], 4)
    out["bytes_ratio"] = round(out["variants"][other]["bytes"] / a["bytes"], 4)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

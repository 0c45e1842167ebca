"""A BatchNorm's backward apply + the producing conv's dgrad + wgrad + reduce (``sep``) against the
one-pass ``kfa_<kind>_fused`` (``fused``) on the shapes of a ResNet-50 step (bs 256) each one-pass
backward (``ops.conv.TAIL_BWDS``) covers, as direct launches on scratch operands
(``TailBwd.candidates``: the input BN's backward statistics fused into both forms, fp32 flat
gradient, accumulating).

    python tools/bench_conv_bwd.py                     # both kinds: median of 3 x 30 launches per form
    python tools/bench_conv_bwd.py --kind conv2_bwd    # one kind (conv3_bwd | conv2_bwd)
    python tools/bench_conv_bwd.py --pmc               # 3 launches of each form: run under rocprofv3

A shape the entry does not cover is reported with ``sep`` alone."""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from kubeflow_controller_amd.ops import conv, routes  # noqa: E402


def _conv3_moved(Nb, HW, Ci, Co):
    T = Nb * HW * HW * Co * 2  # bytes of one [K, Co] bf16 tensor
    return {"sep": 5 * T + 3 * T // 4, "fused": 2 * T + 3 * T // 4}


def _conv2_moved(Nb, HW, Ci, Co):
    t = Nb * HW * HW * Ci * 2  # bytes of one [M, C] bf16 tensor
    halo = 1 + 2 * (HW + 1) / 256  # a 256-pixel tile stages 256 + 2 (W + 1) rows
    return {"sep": int((3 + halo + 2 + 2) * t), "fused": int((2 * halo + 3) * t)}


# kind -> ([(name, H = W, Ci, Co)], bytes each form moves, suffix of the printed shape); a record of
# ops.conv.TAIL_BWDS without a row here is not benchmarked
KINDS = {
    "conv3_bwd": ([("stage1", 56, 64, 256), ("stage2", 28, 128, 512)], _conv3_moved, ""),  # identity-block tails
    "conv2_bwd": ([("stage1", 56, 64, 64)], _conv2_moved, ", 3x3"),                        # stride-1 3x3, 64 -> 64
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=list(KINDS), help="default: every kind")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pmc", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda")
    records = {rec.name: rec for rec in conv.TAIL_BWDS}
    for kind, (shapes, bytes_moved, suffix) in KINDS.items():
        if a.kind not in (None, kind):
            continue
        rec = records[kind]
        for name, HW, Ci, Co in shapes:
            cands, clean = rec.candidates(a.batch, HW, HW, Ci, Co, d)
            if not rec.shape_ok((a.batch, Ci, HW, HW), (Co, Ci, rec.taps, rec.taps), 1, rec.pad):
                cands = cands[:1]
            moved = bytes_moved(a.batch, HW, Ci, Co)
            cells = []
            for form, fn in cands:
                if a.pmc:
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    continue
                ms = routes.time_ms(fn)
                cells.append(f"{form} {ms * 1e3:.1f} us ({moved[form] / ms / 1e9:.2f} TB/s of {moved[form] / 1e9:.2f} GB)")
            clean()
            if cells:
                print(f"{name} (Nb {a.batch}, {HW}x{HW}, {Ci} -> {Co}{suffix}): " + "; ".join(cells), flush=True)


if __name__ == "__main__":
    main()

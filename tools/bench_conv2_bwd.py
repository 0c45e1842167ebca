"""bn2 backward apply + conv2 dgrad + wgrad + reduce (``sep``) against the one-pass
``kfa_conv2_bwd_fused`` (``fused``) on the stage-1 conv2 shape of a ResNet-50 step (bs 256: 3x3,
stride 1, 64 -> 64 channels at 56 x 56), as direct launches on scratch operands
(``ops.conv.conv2_bwd_candidates``: bn1's backward statistics fused into both forms, fp32 flat
gradient, accumulating).

    python tools/bench_conv2_bwd.py                # median of 3 x 30 launches per form
    python tools/bench_conv2_bwd.py --pmc          # 3 launches of each form: run under rocprofv3

A shape the entry does not cover is reported with ``sep`` alone."""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from kubeflow_controller_amd.ops import conv, routes  # noqa: E402

# (name, H = W, C)
SHAPES = [("stage1", 56, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pmc", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda")
    for name, HW, C in SHAPES:
        cands, clean = conv.conv2_bwd_candidates(a.batch, HW, HW, C, d)
        if not conv.conv2_bwd_shape_ok((a.batch, C, HW, HW), (C, C, 3, 3), 1, 1):
            cands = cands[:1]
        t = a.batch * HW * HW * C * 2  # bytes of one [M, C] bf16 tensor
        halo = 1 + 2 * (HW + 1) / 256  # a 256-pixel tile stages 256 + 2 (W + 1) rows
        moved = {"sep": int((3 + halo + 2 + 2) * t), "fused": int((2 * halo + 3) * t)}
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
            print(f"{name} (Nb {a.batch}, {HW}x{HW}, {C} -> {C}, 3x3): " + "; ".join(cells), flush=True)


if __name__ == "__main__":
    main()

"""bn3 backward apply + conv3 dgrad + wgrad + reduce (``sep``) against the one-pass
``kfa_conv3_bwd_fused`` (``fused``) on the identity-block tail shapes of a ResNet-50 step
(bs 256), as direct launches on scratch operands (``ops.conv.conv3_bwd_candidates``: bn2's
backward statistics fused into both forms, fp32 flat gradient, accumulating).

    python tools/bench_conv3_bwd.py                # median of 3 x 30 launches per form
    python tools/bench_conv3_bwd.py --pmc          # 3 launches of each form: run under rocprofv3

Both shapes have a fused form (``conv3_bwd_fused_kernel<64>`` / ``<128>``); a shape the entry
does not cover would be reported with ``sep`` alone."""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from kubeflow_controller_amd.ops import conv, routes  # noqa: E402

# (name, H = W, Ci): Co = 4 Ci
SHAPES = [("stage1", 56, 64), ("stage2", 28, 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pmc", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda")
    for name, HW, Ci in SHAPES:
        Co = 4 * Ci
        cands, clean = conv.conv3_bwd_candidates(a.batch, HW, HW, Ci, Co, d)
        if not conv.conv3_bwd_shape_ok((a.batch, Ci, HW, HW), (Co, Ci, 1, 1), 1, 0):
            cands = cands[:1]
        T = a.batch * HW * HW * Co * 2  # bytes of one [K, Co] bf16 tensor
        moved = {"sep": 5 * T + 3 * T // 4, "fused": 2 * T + 3 * T // 4}
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
            print(f"{name} (Nb {a.batch}, {HW}x{HW}, {Ci} -> {Co}): " + "; ".join(cells), flush=True)


if __name__ == "__main__":
    main()

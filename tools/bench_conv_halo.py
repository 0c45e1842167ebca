"""The four narrow stride-1 3x3 launches of a ResNet-50 step (bs 256; stages 1 and 2,
forward and dgrad) on each tile variant of ``kfa_conv_igemm``, as direct launches with
the fused statistics the model uses.

    python tools/bench_conv_halo.py                 # time every variant (median of 3 x 30 launches)
    python tools/bench_conv_halo.py --pmc           # 3 launches of today's best variant and of the halo
                                                    # kernel per shape: run under rocprofv3 --pmc

Under ``--pmc`` each (shape, variant) pair is its own kernel instantiation or grid, so the
counter CSV separates them by kernel name + grid (``tools/pmc_table.py``)."""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from kubeflow_controller_amd.ops import _lib, conv, routes  # noqa: E402

VARIANTS = {"igemm128": 0, "igemm128x64": 1, "igemm256x64": 3, "pp": 4, "pp512": 6, "halo": 7}
# (name, H = W, C, dgrad, today's routed variant)
SHAPES = [("fwd56", 56, 64, False, "igemm256x64"), ("dgrad56", 56, 64, True, "igemm256x64"),
          ("fwd28", 28, 128, False, "igemm128"), ("dgrad28", 28, 128, True, "pp512")]


def launcher(Nb, HW, C, dgrad):
    d = torch.device("cuda")
    torch.manual_seed(0)
    T = torch.randn(Nb, HW, HW, C, device=d).to(torch.bfloat16)
    Bw = (torch.randn(C, 3, 3, C, device=d) / (9 * C) ** 0.5).to(torch.bfloat16)
    D = torch.empty(Nb, HW, HW, C, device=d, dtype=torch.bfloat16)
    stats = torch.zeros(_lib.lib().kfa_bn_slot_floats(C), dtype=torch.float32, device=d)
    bn = (None, None, None, 0, None, None)
    keep = [T, Bw, D, stats]
    if dgrad:  # backward statistics of the BatchNorm + ReLU the dgrad feeds, mask from x / ss
        x = torch.randn(Nb, HW, HW, C, device=d).to(torch.bfloat16)
        mean = torch.zeros(C, device=d)
        ss = torch.cat([torch.ones(C, device=d), torch.zeros(C, device=d)])
        keep += [x, mean, ss]
        bn = (_lib.ptr(x), None, _lib.ptr(mean), 1, _lib.ptr(ss), None)
    ra = -1 if dgrad else 1

    def run(variant):
        _lib.call("kfa_conv_igemm", _lib.ptr(T), _lib.ptr(Bw), _lib.ptr(D), None, Nb, HW, HW, C, HW, HW, 3, 3, 1, ra,
                  -ra, -ra, C, HW, HW, 1, 0, 0, C, variant, _lib.ptr(stats), *bn, None, _lib.stream())
    run.keep = keep
    run.out = D
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pmc", action="store_true")
    a = ap.parse_args()
    for name, HW, C, dgrad, today in SHAPES:
        run = launcher(a.batch, HW, C, dgrad)
        if a.pmc:
            for v in (today, "halo"):
                for _ in range(3):
                    run(VARIANTS[v])
            torch.cuda.synchronize()
            continue
        run(VARIANTS[today])
        ref = run.out.clone()
        flop = 2.0 * a.batch * HW * HW * C * 9 * C
        cells = []
        for v, num in VARIANTS.items():
            if num in (1, 3) and C != 64:
                continue
            ms = routes.time_ms(lambda: run(num))
            run(num)
            same = torch.equal(run.out, ref)
            cells.append(f"{v} {ms * 1e3:.1f} us ({flop / ms / 1e9:.0f} TF/s{'' if same else ', OUTPUT DIFFERS'})")
        print(f"{name} (Nb {a.batch}, {HW}x{HW}, C {C}; routed today: {today}): " + "; ".join(cells), flush=True)


if __name__ == "__main__":
    main()

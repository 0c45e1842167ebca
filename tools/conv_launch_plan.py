#!/usr/bin/env python3
"""Host launch plans of ``conv_igemm.hip`` in two source trees, compared on the CPU.

    python tools/conv_launch_plan.py OLD NEW

``tools/conv_launch_plan.cpp`` is built once per tree around that tree's
``csrc/kernels/conv_igemm.hip`` (host-only, nothing is launched, CU count = the 256
fallback) and prints, per launch, the kernel instantiation, grid, block size, LDS bytes and
the return code.  The sweep: every conv geometry of the committed routing table plus the
K = 0 sibling classes of its single-tap strided dgrad classes, under variants 0-4, 6, 7 and
the epilogue flag combinations (addend, statistics, BN backward with each mask source, masked addend);
``kfa_conv_igemm_bnpro`` over the table's ``bnpro|`` shapes; with ``KFA_CONV_OVERSUB`` unset
and 0.  Exit status 0 when the two outputs are identical — the check to run after a
change to the host side of the launch path (GPU tests cannot see a moved grid: the kernels
are persistent).
"""
import ast
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kubeflow_controller_amd.ops import conv  # noqa: E402

GEO = conv._IGEMM_GEOMETRY
# E stats bn_x bn_y bn_mean bn_relu bn_ss bn_mb add_mb
BN = [(0, 1, 1, 1, 1, 1, 0, 0, 0), (0, 1, 1, 0, 1, 1, 1, 0, 0), (0, 1, 1, 0, 1, 1, 0, 1, 0),
      (0, 1, 1, 0, 1, 0, 0, 0, 0)]
FLAGS = [(0,) * 9, (0, 1) + (0,) * 7, (1,) + (0,) * 8, (1,) + (0,) * 7 + (1,)] + BN + \
    [(1,) + f[1:] for f in BN] + [(1,) + f[1:8] + (1,) for f in BN]


def sweep():
    with open(os.path.join(ROOT, "kubeflow_controller_amd", "ops", "routes_gfx950.json")) as f:
        keys = sorted(json.load(f)["routes"])
    geos = []
    for k in keys:
        if k.startswith(("conv_fwd|", "conv_dgrad|")):
            g = dict(zip(GEO, (int(v) for v in k.split("|")[1].split(",")[:19])))
            geos.append(tuple(g.values()))
            if k.startswith("conv_dgrad|") and g["os"] > 1 and g["R"] * g["S"] == 1:  # its K = 0 sibling classes
                classes = conv.dgrad_geometries((g["Nb"], g["C"], g["H"], g["W"]), (g["C"], g["N"], 1, 1),
                                                (g["Nb"], g["N"], g["OH"], g["OW"]), g["os"], 0)
                geos += [tuple(getattr(c, n) for n in GEO) for c, _ in classes if c.K == 0]
    lines = [f"igemm {v} {' '.join(map(str, f + g))}" for g in dict.fromkeys(geos) for v in (0, 1, 2, 3, 4, 6, 7)
             for f in FLAGS]
    for k in keys:
        if k.startswith("bnpro|"):
            (Nb, C, H, W), (Co, _, R, S), stride, pad, _ = ast.literal_eval(k.split("|")[1])
            P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
            lines += [f"bnpro {v} {st} {y} {Nb} {H} {W} {C} {P} {Q} {R} {S} {stride} {pad} {Co}"
                      for v in range(4) for st in (0, 1) for y in (0, 1)]
    return "\n".join(lines) + "\n"


def plan(tree, text, tmp, tag):
    exe = os.path.join(tmp, "plan_" + tag)
    kdir = os.path.join(os.path.abspath(tree), "csrc", "kernels")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", "--cuda-host-only", "-w",
                    f"-I{kdir}", f'-DKFA_CONV_IGEMM_HIP="{kdir}/conv_igemm.hip"', "-x", "hip",
                    os.path.join(ROOT, "tools", "conv_launch_plan.cpp"), "-o", exe], check=True)
    out = ""
    for oversub in (None, "0"):
        env = {k: v for k, v in os.environ.items() if k != "KFA_CONV_OVERSUB"}
        if oversub is not None:
            env["KFA_CONV_OVERSUB"] = oversub
        out += f"# KFA_CONV_OVERSUB={oversub}\n" + subprocess.run([exe], input=text, capture_output=True, text=True,
                                                                 env=env, check=True).stdout
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = sys.argv[1:3]
    text = sweep()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = plan(old, text, tmp, "old"), plan(new, text, tmp, "new")
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(b)
    la, lb = a.splitlines(), b.splitlines()
    diff = [(x, y) for x, y in zip(la, lb) if x != y]
    print(f"{len(la)} / {len(lb)} lines, {len(diff) + abs(len(la) - len(lb))} differ")
    for x, y in diff[:10]:
        print("-", x, "\n+", y)
    return 1 if diff or len(la) != len(lb) else 0


if __name__ == "__main__":
    sys.exit(main())

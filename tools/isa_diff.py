#!/usr/bin/env python3
"""Per-kernel device-code comparison of two source trees (CPU only).

    python tools/isa_diff.py OLD NEW [name.hip ...] [--md summary.md]

OLD and NEW are repository trees (their ``csrc/kernels/*.hip`` are compiled with
the flags of ``_build.py`` plus ``--cuda-device-only -S``) or directories that
already hold ``<name>.s`` files.  Every kernel is reported ``same`` or
``differs`` (with a unified diff) next to its register, spill, LDS and scratch
figures; the exit status is non-zero if any kernel differs or the set of kernel
names changed.  Text comparison only: the check to run after a change that is
meant to leave device code alone (docs/development.md).
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DEFAULT = ["gemm.hip", "gemm_ppp.hip", "gemm_skinny.hip", "conv_igemm.hip", "wgrad.hip"]
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
META = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size", "private_segment_fixed_size"]
DROP = re.compile(r"^\s*\.(file|ident)\b|__hip_cuid_|^\s*;.*\.(hip|h|cpp|hpp)\b")
# local labels carry the function's index in the file (.LBB22_3, .Lfunc_end22): the order the
# host code instantiates the kernels in, not device code
LABEL = re.compile(r"(?<![\w.])(\.LBB|BB|\.Lfunc_begin|\.Lfunc_end)\d+")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return "hipcc"


def assembly(tree, name, tmp):
    """Path of the .s for ``name``: found in ``tree`` or compiled from its sources."""
    stem = os.path.splitext(name)[0]
    ready = os.path.join(tree, stem + ".s")
    if os.path.exists(ready):
        return ready
    kdir = os.path.join(tree, "csrc", "kernels")
    out = os.path.join(tmp, stem + ".s")
    cmd = [hipcc(), "-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-munsafe-fp-atomics",
           "-Wno-unused-result", f"-I{kdir}", "--cuda-device-only", "-S", os.path.join(kdir, name), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"compile failed: {' '.join(cmd)}\n{r.stderr}")
    return out


def kernels(path):
    """{symbol: (text lines, metadata dict)} of one assembly file."""
    with open(path) as f:
        text = f.read()
    body, _, meta = text.partition(".amdgpu_metadata")
    chunks, name = {}, None
    for line in body.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if re.match(r"\s*\.section\s+\.text", line):  # the next function's preamble
            name = None
        if m:
            name = m.group(1)
            chunks[name] = []
        if name and not DROP.search(line):
            chunks[name].append(LABEL.sub(r"\1", line.rstrip()))
    info = {}
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        keys = dict(re.findall(r"^(?:    )?\.(\w+):\s+(.*)$", entry, flags=re.M))
        info[keys.get("name", "?")] = {k: keys.get(k, "-") for k in META}
    return {k: (v, info.get(k, {})) for k, v in chunks.items() if k in info}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*", default=DEFAULT)
    ap.add_argument("--md", help="also write the summary table to this file")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()

    rows, bad = [], 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new, \
            ThreadPoolExecutor(a.jobs) as pool:
        jobs = [(f, pool.submit(assembly, a.old, f, t_old), pool.submit(assembly, a.new, f, t_new)) for f in a.files]
        for f, fo, fn in jobs:
            old, new = kernels(fo.result()), kernels(fn.result())
            for k in sorted(set(old) | set(new)):
                if k not in old or k not in new:
                    rows.append((f, k, "only in " + ("old" if k in old else "new"), {}, {}))
                    bad += 1
                    continue
                same = old[k][0] == new[k][0]
                rows.append((f, k, "same" if same else "differs", old[k][1], new[k][1]))
                if not same:
                    bad += 1
                    sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(
                        old[k][0], new[k][0], f"old/{f}:{k}", f"new/{f}:{k}", lineterm="", n=2))

    out = ["| file | kernel | result | " + " | ".join(META) + " |", "|---" * (3 + len(META)) + "|"]
    for f, k, res, mo, mn in rows:
        cells = [mo.get(m, "-") if mo.get(m) == mn.get(m) else f"{mo.get(m, '-')} -> {mn.get(m, '-')}" for m in META]
        out.append(f"| {f} | `{k}` | {res} | " + " | ".join(cells) + " |")
    per_file = {f: sum(1 for r in rows if r[0] == f) for f in a.files}
    out.append("")
    out.append(f"{len(rows)} kernels ({', '.join(f'{f} {n}' for f, n in per_file.items())}): "
               f"{len(rows) - bad} same, {bad} differing or unmatched.")
    print("\n".join(out))
    if a.md:
        with open(a.md, "w") as f:
            f.write("# Per-kernel device-code comparison (tools/isa_diff.py)\n\n" + "\n".join(out) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

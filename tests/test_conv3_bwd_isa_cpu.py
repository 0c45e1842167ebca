"""ISA checks of the one-pass conv3 backward (CPU: hipcc cross-compiles gfx950).

``conv3_bwd_fused_kernel`` (csrc/kernels/conv3_bwd.hip) keeps the next tile's global loads in
flight under the current tile's MFMAs and epilogue; the epilogue's LDS staging is inline asm under
the kernel's own ``lgkmcnt`` so that hipcc has no reason to drain ``vmcnt(0)`` in front of it.
Checked on the compiled ``.s``: the register / LDS / scratch budgets from the kernel metadata, no
use of a register an inline-asm LDS read is still filling (tools/asm_read_hazards.py), and no
compiler-placed full vector-memory wait between the issue of the next tile's loads and the tile
loop's back edge.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc not available")

# vgpr_spill_count of the Ci = 128 form as built (0 for Ci = 64, which is not negotiable)
SPILL = {64: 0, 128: 13}
LDS_MAX = {64: 81920, 128: 163840}  # two blocks / one block per CU of 160 KB
# loads of the next tile issued ahead, per lane: Ci = 64 the whole tile (8 g + 8 x3 16-B loads and 8 bit
# bytes), Ci = 128 the half of it that fits beside 128 dW registers
PREFETCH_LOADS = {64: 24, 128: 12}


@pytest.fixture(scope="module")
def conv3_s(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "conv3_bwd.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                    f"-I{ROOT}/csrc/kernels", "--cuda-device-only", "-S", f"{ROOT}/csrc/kernels/conv3_bwd.hip",
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def _bodies(text: str):
    out = {}
    for name in re.findall(r"^(_Z[^:\s]+):", text, re.M):
        if "conv3_bwd_fused_kernel" in name:
            i = text.index(name + ":")
            ci = int(re.search(r"conv3_bwd_fused_kernelILi(\d+)E", name).group(1))
            out[ci] = (name, text[i:text.index(".Lfunc_end", i)].split("\n"))
    return out


def _meta(text: str, name: str, key: str) -> int:
    seg = text[text.rindex("- .agpr_count", 0, text.index(".name:           " + name)):]
    return int(re.search(rf"\.{key}:\s+(\d+)", seg).group(1))


def _main_loop(body):
    """(first, last) line of the longest loop, as test_isa_cpu.py finds it."""
    labels = {m.group(1): k for k, l in enumerate(body) if (m := re.match(r"^\.(LBB\d+_\d+):", l))}
    loops = [(labels[m.group(1)], k) for k, l in enumerate(body)
             if (m := re.search(r"s_c?branch\w* \.(LBB\d+_\d+)", l)) and m.group(1) in labels
             and labels[m.group(1)] < k]
    return max(loops, key=lambda x: x[1] - x[0])


def _in_kernel_asm(body, k):
    """Line k stands inside an inline-asm statement of the kernel's own."""
    for j in range(k - 1, -1, -1):
        t = body[j].strip()
        if t.startswith(";;#ASMEND"):
            return False
        if t.startswith(";;#ASMSTART"):
            return True
    return False


def test_both_forms_are_built(conv3_s):
    assert sorted(_bodies(conv3_s)) == [64, 128]


@pytest.mark.parametrize("ci", [64, 128])
def test_register_lds_and_scratch_budgets(conv3_s, ci):
    name, _ = _bodies(conv3_s)[ci]
    meta = {k: _meta(conv3_s, name, k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                                 "group_segment_fixed_size")}
    print(ci, meta)
    assert meta["vgpr_count"] <= 256
    assert meta["vgpr_spill_count"] == SPILL[ci]
    if SPILL[ci] == 0:
        assert meta["private_segment_fixed_size"] == 0
    assert meta["group_segment_fixed_size"] <= LDS_MAX[ci]


@pytest.mark.parametrize("ci", [64, 128])
def test_asm_lds_reads_have_no_hazards(conv3_s, ci):
    import asm_read_hazards
    name, body = _bodies(conv3_s)[ci]
    assert sum("ds_read" in l and _in_kernel_asm(body, k) for k, l in enumerate(body)) >= 20
    assert asm_read_hazards.check(body) == [], name


@pytest.mark.parametrize("ci", [64, 128])
def test_no_compiler_drain_after_the_next_tiles_loads(conv3_s, ci):
    """From the first global load of the next tile (the first run of register loads in the tile
    loop as long as the prefetch) to the back edge, every ``s_waitcnt vmcnt(0)`` is the kernel's own."""
    name, body = _bodies(conv3_s)[ci]
    first, last = _main_loop(body)
    # runs of buffer loads into registers (LDS-DMAs carry the `lds` modifier and hold no register)
    runs, cur = [], []
    for k in range(first, last):
        t = body[k].strip()
        if re.match(r"buffer_load_\w+\s+v", t) and not t.endswith(" lds"):
            cur.append(k)
        elif cur and re.match(r"(v_mfma|s_barrier|ds_|buffer_store|s_cbranch|s_branch)", t):
            runs.append(cur)
            cur = []
    if cur:
        runs.append(cur)
    ahead = [r for r in runs if len(r) >= PREFETCH_LOADS[ci]]
    assert ahead, (name, [len(r) for r in runs])
    issue = ahead[0]
    drains = [k for k in range(issue[0], last + 1) if re.match(r"\s+s_waitcnt vmcnt\(0\)", body[k])
              and not _in_kernel_asm(body, k)]
    assert drains == [], (name, [(k, body[k].strip()) for k in drains])

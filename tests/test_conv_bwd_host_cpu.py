"""The host path of the one-pass conv backward kernels (``kfa_conv3_bwd_fused`` /
``kfa_conv2_bwd_fused``), on the CPU: the argument vector each fused launch and each ``sep``
candidate hands to the library (checked position by position against the C prototype parsed from
the source), the route keys against the committed table, ``conv2d``'s arming order and gates, the
link a BatchNorm accepts, and the entries' host plans.  ``_lib.call`` is stubbed; the library is
loaded only for ``part_floats`` with ``max_blocks > 0`` and for refusals, which ask the device
nothing."""
import json
import os

import pytest
import torch

from kubeflow_controller_amd.ops import _lib, batchnorm, conv as convmod, routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
STREAM = 77

# ---- the names under test --------------------------------------------------------------------
KINDS = ("conv3_bwd", "conv2_bwd")  # the order conv2d tries them in
SHAPE = {"conv3_bwd": (2, 4, 4, 64, 256, 1, 0), "conv2_bwd": (2, 6, 5, 64, 64, 3, 1)}  # Nb H W Ci Co R pad
MASK_SLOT = {"conv3_bwd": "mb", "conv2_bwd": "ss"}  # the link field behind the entry's third pointer


REC = {rec.name: rec for rec in convmod.TAIL_BWDS}


def test_the_records_are_the_two_kinds_in_order():  # (added after the refactor: the parent has no records)
    assert tuple(REC) == KINDS and convmod.TAIL_BWDS == (convmod.CONV3_BWD, convmod.CONV2_BWD)
    assert {k: (r.mask, r.residual) for k, r in REC.items()} == {"conv3_bwd": ("bits", True), "conv2_bwd": ("ss", False)}


def _fused(kind):
    return REC[kind].fused


def _candidates(kind, Nb, H, W, Ci, Co, dev):
    return REC[kind].candidates(Nb, H, W, Ci, Co, dev)


def _route(kind, xs, ws, dev):
    return REC[kind].route(xs, ws, dev)


def _stub_routes(monkeypatch, asked, value=True):
    for kind in KINDS:
        monkeypatch.setattr(REC[kind], "route", lambda *a, _k=kind: asked.append(_k) or value)


def _set_enabled(monkeypatch, kind, on):
    monkeypatch.setattr(REC[kind], "enabled", on)


def _new_link(kind):
    return convmod.TailBwdLink(REC[kind])


def _tag(y, kind, link):
    y._kfa_tail_link = link


def _armed_kind(y):
    link = getattr(y, "_kfa_tail_link", None)
    return None if link is None else link.rec.name


def _mask_ok(link, ss, mb):
    return link.rec.mask_ok(ss, mb)


def _part_floats(kind, Nb, H, W, Ci, Co, max_blocks):
    return getattr(_lib.lib(), f"kfa_{kind}_part_floats")(Nb, H, W, Co, Ci, max_blocks)


# ---- helpers ---------------------------------------------------------------------------------
def _prototype(kind):
    """[(name, is_pointer)] of ``kfa_<kind>_fused``'s parameters, from the source."""
    with open(os.path.join(ROOT, "csrc", "kernels", f"{kind}.hip")) as f:
        params = f.read().split(f"KFA_API int kfa_{kind}_fused(", 1)[1].split(")", 1)[0]
    out = []
    for p in params.split(","):
        ctype, name = p.strip().rsplit(None, 1)
        assert ctype == "int" or ctype.endswith("*") or ctype == "hipStream_t", p
        out.append((name, ctype != "int"))
    return out


@pytest.fixture
def calls(monkeypatch):
    made = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: made.append((name, a)))
    monkeypatch.setattr(_lib, "stream", lambda: STREAM)
    return made


def _operands(kind, dtype_grad):
    Nb, H, W, Ci, Co, R, pad = SHAPE[kind]
    bf = dict(dtype=torch.bfloat16)
    t = dict(g=torch.randn(Nb, Co, H, W, **bf).contiguous(memory_format=CL),
             x=torch.randn(Nb, Co, H, W, **bf).contiguous(memory_format=CL),
             coef=torch.randn(3 * Co), y=torch.randn(Nb, Ci, H, W, **bf).contiguous(memory_format=CL),
             w=torch.randn(Co, Ci, R, R, **bf).contiguous(memory_format=CL),
             grad=torch.zeros(Co, Ci, R, R, dtype=dtype_grad).contiguous(memory_format=CL))
    t["mask"] = (torch.zeros(Nb * H * W * Co // 8, dtype=torch.uint8) if MASK_SLOT[kind] == "mb"
                 else torch.zeros(2 * Co))
    return t


def _bn_link(Ci, Nb, H, W):
    bn = batchnorm.BnBwdLink()
    bn.x = torch.randn(Nb, Ci, H, W, dtype=torch.bfloat16).contiguous(memory_format=CL)
    bn.mean, bn.ss, bn.mb, bn.relu = torch.zeros(Ci), torch.ones(2 * Ci), None, True
    return bn


# this test's operand names -> the entry's first eight parameters (conv3's / conv2's spelling)
_OPERANDS = ["g", "x", "mask", "coef", "y", "wt", "dx", "grad"]
_SPELLED = {"conv3_bwd": ["g", "x3", "mb", "coef", "y2", "wt", "dx2", "grad"],
            "conv2_bwd": ["g2", "x2", "ss2", "coef", "y1", "wt", "dx1", "grad"]}


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype_grad", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_launch_arguments_follow_the_prototype(kind, with_bn, dtype_grad, accumulate, calls, monkeypatch):
    Nb, H, W, Ci, Co, R, pad = SHAPE[kind]
    proto = _prototype(kind)
    assert len(proto) == 28
    assert _lib._SIGS[f"kfa_{kind}_fused"] == [_lib.P if p else _lib.I for _, p in proto]
    assert [n for n, _ in proto[8:11]] == ["grad_f32", "accumulate", "part"]
    assert [n for n, _ in proto[:8]] == _SPELLED[kind] and _SPELLED[kind][2].startswith(MASK_SLOT[kind])
    assert [n for n, _ in proto[16:]] == ["R", "S", "stride", "pad", "stats", "bn_x", "bn_mean", "bn_relu", "bn_ss",
                                          "bn_mb", "max_blocks", "s"]
    t = _operands(kind, dtype_grad)
    bn = _bn_link(Ci, Nb, H, W) if with_bn else None
    made_wt = []
    real_tw = convmod._transposed_weight
    monkeypatch.setattr(convmod, "_transposed_weight", lambda *a: made_wt.append(real_tw(*a)) or made_wt[-1])
    dx = _fused(kind)(t["g"], t["x"], t["mask"], t["coef"], t["y"], t["w"], t["grad"], accumulate, bn, 3)
    assert dx.shape == t["y"].shape and dx.dtype == torch.bfloat16 and dx.is_contiguous(memory_format=CL)
    assert [n for n, _ in calls] == ["kfa_weight_transpose", f"kfa_{kind}_fused"]
    tw = calls[0][1]
    assert tw[:2] == (t["w"].data_ptr(), made_wt[0].data_ptr()) and tw[2:] == (Co, R, R, Ci, 0, 1, R, 0, 1, R, STREAM)
    assert tuple(made_wt[0].shape) == (Ci, R, R, Co)
    args = calls[1][1]
    assert len(args) == len(proto)
    nfl = _part_floats(kind, Nb, H, W, Ci, Co, 3)
    assert nfl > 0
    part = _lib.workspace(nfl * 4, "cpu", f"{kind}_part{STREAM}")
    slots = batchnorm.bn_slot_workspace(Ci, "cpu")
    want = dict(t, wt=made_wt[0], dx=dx)
    want = [want[n].data_ptr() for n in _OPERANDS]
    want += [int(dtype_grad == torch.float32), int(accumulate), part.data_ptr(), Nb, H, W, Ci, Co, R, R, 1, pad]
    if with_bn:
        want += [slots.data_ptr(), bn.x.data_ptr(), bn.mean.data_ptr(), 1, bn.ss.data_ptr(), None]
    else:
        want += [None, None, None, 0, None, None]
    want += [3, STREAM]
    for i, ((name, is_ptr), got, exp) in enumerate(zip(proto, args, want)):
        assert got == exp, (i, name)
        assert isinstance(got, int) if not is_ptr else (got is None or isinstance(got, int)), (i, name)
    if with_bn:
        assert bn.prestats is True
    # stride / pad reach the entry as given (it refuses what it does not cover)
    del calls[:]
    _fused(kind)(t["g"], t["x"], t["mask"], t["coef"], t["y"], t["w"], t["grad"], accumulate, None, 3, stride=2, pad=5)
    assert calls[-1][1][18:20] == (2, 5) and calls[-1][1][26] == 3


@pytest.mark.parametrize("kind", KINDS)
def test_sep_candidates_hand_the_same_operands_to_the_separate_kernels(kind, calls, monkeypatch):
    Nb, H, W, Ci, Co, R, pad = SHAPE[kind]
    dg, wg = [], []
    monkeypatch.setattr(convmod, "conv_dgrad", lambda *a: dg.append(a))
    monkeypatch.setattr(convmod, "wgrad_into", lambda *a: wg.append(a))
    cands, clean = _candidates(kind, Nb, H, W, Ci, Co, "cpu")
    assert [n for n, _ in cands] == ["sep", "fused"]
    cands[0][1]()
    assert [n for n, _ in calls] == ["kfa_bn_bwd_apply_only"] and len(dg) == 1 and len(wg) == 1
    a = calls[0][1]
    dx, w, y_shape, stride, dpad, addend, bn = dg[0]
    assert a[2] is None and a[4] == dx.data_ptr() and a[5:8] == (Nb * H * W, Co, 1) and a[10] == STREAM
    # the mask source: bits for conv3's BN (slot 9), [scale | shift] for conv2's (slot 8); the other is None
    assert (a[8] is None, a[9] is None) == ((True, False) if MASK_SLOT[kind] == "mb" else (False, True))
    assert tuple(dx.shape) == (Nb, Co, H, W) and tuple(w.shape) == (Co, Ci, R, R) and tuple(y_shape) == (Nb, Ci, H, W)
    assert (stride, dpad, addend) == (1, pad, None) and bn.relu is True and tuple(bn.x.shape) == (Nb, Ci, H, W)
    y, dx2, acc = wg[0][:3]
    assert dx2 is dx and tuple(y.shape) == (Nb, Ci, H, W) and acc.dtype == torch.float32
    assert tuple(acc.shape) == (Co, Ci, R, R) and wg[0][3:] == (Nb, H, W, Ci, H, W, Co, R, R, 1, pad, True)
    # the fused candidate: the same g / x / coef / y / weight, fp32 accumulate, bn's statistics
    del calls[:]
    cands[1][1]()
    f = calls[-1][1]
    assert calls[-1][0] == f"kfa_{kind}_fused" and f[0] == a[0] and f[1] == a[1] and f[3] == a[3]
    assert f[2] == (a[9] if MASK_SLOT[kind] == "mb" else a[8]) and f[4] == y.data_ptr() and f[7] == acc.data_ptr()
    assert f[8:10] == (1, 1) and f[21] == bn.x.data_ptr() and f[23] == 1 and f[26] == 0 and bn.prestats is True
    clean()
    assert bn.prestats is False and not batchnorm.bn_slot_workspace(Ci, "cpu").any()


def test_route_keys_reproduce_the_committed_table(monkeypatch):
    with open(os.path.join(ROOT, "kubeflow_controller_amd", "ops", "routes_gfx950.json")) as f:
        doc = json.load(f)
    keys = sorted(k for k in doc["routes"] if k.startswith(("conv3_bwd|", "conv2_bwd|")))
    assert keys == ["conv2_bwd|256,56,56,64", "conv3_bwd|256,28,28,128,512", "conv3_bwd|256,56,56,64,256"]
    seen = []

    def decide(kind, key, device, candidates, **kw):
        assert [n for n, _ in candidates] == ["sep", "fused"]
        seen.append(routes.key_str(kind, key))
        return 1

    monkeypatch.setattr(routes, "decide", decide)
    for key in keys:
        kind, ints = key.split("|")
        v = [int(i) for i in ints.split(",")]
        Nb, H, W, Ci = v[:4]
        Co = v[4] if len(v) > 4 else Ci
        R = SHAPE[kind][5]
        assert _route(kind, (Nb, Ci, H, W), (Co, Ci, R, R), "cpu") is True  # (no candidate ran: no scratch made)
    assert seen == keys


def _conv(kind, device="cpu", **kw):
    Nb, H, W, Ci, Co, R, pad = SHAPE[kind]
    x = torch.randn(Nb, Ci, H, W, requires_grad=True, device=device)
    w = torch.randn(Co, Ci, R, R, requires_grad=True, device=device)
    return convmod.conv2d(x, w, 1, pad, **kw)


def test_arming_order_and_gates(calls, monkeypatch):
    asked = []
    _stub_routes(monkeypatch, asked)
    for kind in KINDS:
        _set_enabled(monkeypatch, kind, True)
    # CPU tensors: nothing is asked, nothing armed, no library call
    for kind in KINDS:
        assert _armed_kind(_conv(kind, tail_link=True)) is None
    assert asked == [] and calls == []
    # the gate itself, with the device test out of the way: a stand-in conv whose input claims to be on the GPU
    monkeypatch.setattr(convmod, "igemm_ok", lambda x, w: True)
    monkeypatch.setattr(convmod, "stem_ok", lambda *a: False)
    monkeypatch.setattr(convmod, "_use_vendor_fwd", lambda *a: False)
    monkeypatch.setattr(convmod._ConvFn, "apply", staticmethod(lambda x, w, *a: torch.empty(1)))

    class OnGpu(torch.Tensor):
        is_cuda = True

    def run(kind, tail_link=True, join=None, grad=True):
        Nb, H, W, Ci, Co, R, pad = SHAPE[kind]
        x = torch.randn(Nb, Ci, H, W).as_subclass(OnGpu)
        with torch.set_grad_enabled(grad):
            return _armed_kind(convmod.conv2d(x, torch.randn(Co, Ci, R, R), 1, pad, join=join, tail_link=tail_link))

    for kind in KINDS:
        del asked[:]
        assert run(kind) == kind and asked == [kind]          # only the covering kind's route is asked
        assert run(kind, tail_link=False) is None             # the model did not ask
        assert run(kind, grad=False) is None                  # eval
        assert run(kind, join=convmod.GradJoin()) is None     # a join deposits into this conv's dgrad
        assert asked == [kind]
        _set_enabled(monkeypatch, kind, False)                # the switch off: not even the route is asked
        assert run(kind) is None and asked == [kind]
        _set_enabled(monkeypatch, kind, True)
    # the route says sep: no link
    del asked[:]
    _stub_routes(monkeypatch, asked, False)
    assert run("conv3_bwd") is None and run("conv2_bwd") is None and asked == list(KINDS)
    assert calls == []


@pytest.mark.parametrize("kind,residual", [("conv3_bwd", False), ("conv2_bwd", True)])
@pytest.mark.parametrize("mask", ["ss", "mb"])
def test_a_batchnorm_takes_only_the_link_of_its_form(kind, residual, mask, calls, monkeypatch):
    """conv3's link needs a BN with a residual, conv2's one without: the other combination leaves
    the link armed (the conv's backward then runs the separate path), whatever mask the BN keeps."""
    monkeypatch.setattr(batchnorm, "MASK_FROM_X", True)
    seen = []

    class Fn:
        @staticmethod
        def apply(x, weight, bias, rm, rv, res, training, momentum, eps, relu, prestats, link, res_join, lz, tail):
            seen.append(tail)
            return torch.empty(1)

    monkeypatch.setattr(batchnorm, "_BNActFn", Fn)
    x = torch.randn(2, 8, 3, 3, dtype=torch.bfloat16)
    link = _new_link(kind)
    _tag(x, kind, link)
    C = 8
    p = [torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)]
    batchnorm.bn_act(x, *p, residual=torch.zeros_like(x) if residual else None, training=True)
    assert seen == [None] and link.state == "armed"
    ss, mb = (torch.zeros(2 * C), None) if mask == "ss" else (None, torch.zeros(18, dtype=torch.uint8))
    # the matching form hands the link over; whether it is then taken is the mask rule's business
    batchnorm.bn_act(x, *p, residual=None if residual else torch.zeros_like(x), training=True)
    assert seen[1] is link
    assert _mask_ok(link, ss, mb) == (MASK_SLOT[kind] == mask)
    # eval never takes it
    batchnorm.bn_act(x, *p, residual=None if residual else torch.zeros_like(x), training=False)
    assert seen[2] is None and link.state == "armed"


# ---- conv3's host plan (the table tests/test_conv2_bwd_cpu.py has for conv2) --------------------
def test_conv3_part_floats_counts_the_blocks_with_tiles():
    part = lambda Nb, H, W, Ci, Co, mb: _part_floats("conv3_bwd", Nb, H, W, Ci, Co, mb)  # noqa: E731
    s64, s128 = 256 * 64, 512 * 128
    assert part(2, 4, 4, 64, 256, 3) == s64                 # 32 pixels: one 64-pixel tile
    assert part(2, 8, 8, 64, 256, 8) == 2 * s64             # two exact tiles, fewer than the cap
    assert part(5, 12, 10, 64, 256, 1) == s64               # ten tiles in one block
    assert part(1, 56, 56, 64, 256, 2) == 2 * s64           # 49 tiles over two blocks
    assert part(256, 56, 56, 64, 256, 1000) == 1000 * s64   # max_blocks > 0: no two-per-CU cap (12544 tiles)
    assert part(256, 28, 28, 128, 512, 700) == 700 * s128   # ... nor the one-per-CU cap of Ci = 128
    assert part(2, 4, 4, 128, 512, 3) == s128
    # not covered: no workspace
    assert part(2, 4, 4, 256, 1024, 3) == 0
    assert part(2, 4, 4, 64, 64, 3) == 0
    assert part(2, 4, 4, 256, 64, 3) == 0                   # Ci and Co the other way round
    assert part(0, 4, 4, 64, 256, 3) == 0                   # no pixels: no blocks


@pytest.mark.parametrize("geom,code", [
    ((2, 4, 4, 64, 256, 3, 3, 1, 1), -1),      # a 3x3
    ((2, 4, 4, 64, 256, 1, 1, 2, 0), -1),      # stride 2
    ((2, 4, 4, 64, 256, 1, 1, 1, 1), -1),      # padded
    ((2, 4, 4, 256, 1024, 1, 1, 1, 0), -1),    # Ci = 256
    ((2, 4, 4, 64, 128, 1, 1, 1, 0), -1),      # Co != 4 Ci
    ((2, 4, 4, 64, 256, 1, 1, 1, 0), -1),      # covered, but no operands: still no launch
    ((1 << 12, 64, 64, 64, 256, 1, 1, 1, 0), -1),  # missing operands are checked before the offset limit
    ((0, 4, 4, 64, 256, 1, 1, 1, 0), -1),      # ... and before the empty range
])
def test_conv3_entry_refuses_before_any_launch(geom, code):
    fn = _lib.lib().kfa_conv3_bwd_fused
    Nb, H, W, Ci, Co, R, S, stride, pad = geom
    assert fn(None, None, None, None, None, None, None, None, 1, 0, None, Nb, H, W, Ci, Co, R, S, stride, pad,
              None, None, None, 0, None, None, 1, None) == code


def test_conv3_entry_codes_behind_the_operand_check():
    """With (never dereferenced) operands: the -3 refusal, the empty range's 0 and the -2 limit, in
    that order -- none launches anything."""
    fn = _lib.lib().kfa_conv3_bwd_fused
    buf = torch.zeros(64)
    p = buf.data_ptr()

    def call(Nb, H, W, bn_x=None, relu=0, ss=None, mb=None):
        return fn(p, p, p, p, p, p, p, p, 1, 0, p, Nb, H, W, 64, 256, 1, 1, 1, 0, None, bn_x, None, relu, ss, mb, 1, None)

    assert call(2, 4, 4, bn_x=p, relu=1) == -3            # a ReLU mask without a source
    assert call(0, 4, 4, bn_x=p, relu=1) == -3            # ... checked before the empty range
    assert call(0, 4, 4) == 0                             # no pixels: nothing to do
    assert call(0, 4, 4, bn_x=p, relu=1, ss=p) == 0
    assert call(1 << 12, 64, 64) == -2                    # 2^24 pixels
    assert call(1 << 10, 64, 64) == -2                    # 2^22 pixels x 256 channels x 2 B = 2^31

"""The launch record of the fused optimizers (``ops/optim.py`` -> ``csrc/kernels/optim.hip``): every
``_lib.call`` of one ``step(grad_scale=0.5)``, in order, with each pointer resolved to (buffer, byte
offset) against the optimizer's own buffers and each argument checked position by position against
the C prototype parsed from the source.  The expected records are literals, written against the
code before its host paths were merged; only the block under "the private names under test" may
follow a refactor.  The calls are forwarded, so the kernels do run."""
import os
import re

import pytest
import torch

from kubeflow_controller_amd.ops import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (5,): under one vector; (63, 33): numel % 8 == 7; (300, 300): six chunks, the last one ragged
SHAPES_W = [(5,), (63, 33), (300, 300)]
SHAPES_B = [(11,), (768,)]
NW, NB = 92096, 832  # elements of the two groups: tensors padded to 8, the group to 64
CW, CB = 8, 2        # chunks (16384 elements at most, none across a tensor boundary)
TW, TB = 3, 2        # tensors
S = "current"        # the stream argument: torch's current stream

# ---- the private names under test: the only block that may follow a refactor --------------------
BC = "kfa_adam_bc"  # the entry that advances Adam's device step count and bias corrections


def _tables(opt):
    return opt._tabs or []


def _buffers(opt):
    """This test's buffer names -> the optimizer's tensors (``None`` / missing ones dropped)."""
    out = {"gpart": opt._gpart, "clip": opt._clip, "bc": getattr(opt, "_bc", None), "t": getattr(opt, "_t", None)}
    per_space = {"m": getattr(opt, "m", []), "v": getattr(opt, "v", []), "mom": getattr(opt, "mom", []),
                 "part": opt._part, "ratio": opt._ratio,
                 "chunks": [t.chunks for t in _tables(opt)], "tens": [t.tens for t in _tables(opt)]}
    for i, s in enumerate(opt.spaces):
        out.update({f"w{i}": s.w, f"wb{i}": s.wb, f"grad{i}": s.grad})
        for name, bufs in per_space.items():
            if i < len(bufs):
                out[f"{name}{i}"] = bufs[i]
    return {k: v for k, v in out.items() if v is not None}


# ---- the record ---------------------------------------------------------------------------------
# prototype parameter name -> the buffer a pointer handed to it must lie in (without the space index)
_ROLE = {"w": ("w",), "wb": ("wb",), "g": ("grad",), "m": ("m",), "v": ("v",), "mom": ("mom",), "chunks": ("chunks",),
         "tens": ("tens",), "part": ("part", "gpart"), "wpart": ("part",), "gpart": ("gpart",), "ratio": ("ratio",),
         "dbc": ("bc",), "bc": ("bc",), "t": ("t",), "dcoef": ("clip",), "out": ("clip",)}


def _prototypes():
    """entry -> [(parameter name, 'P' | 'I' | 'L' | 'F' | 'S')] from the source; S is the stream."""
    with open(os.path.join(ROOT, "csrc", "kernels", "optim.hip")) as f:
        src = f.read()
    protos = {}
    for name, params in re.findall(r"KFA_API int (kfa_\w+)\(([^)]*)\)", src):
        out = []
        for p in params.split(","):
            ctype, pname = p.strip().rsplit(None, 1)
            kind = "P" if ctype.endswith("*") else {"int": "I", "long": "L", "float": "F", "hipStream_t": "S"}[ctype]
            out.append((pname, kind))
        protos[name] = out
    return protos


PROTOS = _prototypes()


def _resolve(p, bufs):
    for name, t in bufs.items():
        base = t.data_ptr()
        if base <= p < base + max(1, t.numel() * t.element_size()):
            return name, p - base
    raise AssertionError(f"pointer {p:#x} lies in none of {sorted(bufs)}")


def _named(made, opt):
    """The raw record with pointers as (buffer, byte offset) and the stream as "current"; every
    argument checked against its prototype position on the way."""
    bufs = _buffers(opt)
    stream = torch.cuda.current_stream().cuda_stream
    ctypes_of = {"P": _lib.P, "I": _lib.I, "L": _lib.L, "F": _lib.F, "S": _lib.P}
    out = []
    for name, args in made:
        proto = PROTOS[name]
        assert len(args) == len(proto), name
        assert _lib._SIGS[name] == [ctypes_of[k] for _, k in proto], name
        row = []
        for i, ((pname, kind), a) in enumerate(zip(proto, args)):
            where = (name, i, pname)
            if kind == "S":
                assert i == len(proto) - 1, where
                a = S if a == stream else a
            elif kind == "P":
                assert a is None or (isinstance(a, int) and not isinstance(a, bool)), where
                if a is not None:
                    a = _resolve(a, bufs)
                    assert a[0].rstrip("0123456789") in _ROLE[pname], where + (a,)
            elif kind == "F":
                assert isinstance(a, float), where
            else:
                assert isinstance(a, int) and not isinstance(a, bool), where
            row.append(a)
        out.append((name, tuple(row)))
    return out


@pytest.fixture
def made(monkeypatch):
    calls = []
    real = _lib.call

    def call(name, *args):
        calls.append((name, args))
        real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    return calls


def _groups():
    """Two flat groups with a group tail (pad_to=64): bf16 "weights" with an fp32 master, a bf16
    compute copy and bf16 gradients, and fp32 1-D "norms_biases"; random weights and gradients."""
    from kubeflow_controller_amd.parallel.flat import FlatGroup
    gen = torch.Generator().manual_seed(7)
    pw = [torch.nn.Parameter(torch.randn(*s, generator=gen).cuda().bfloat16()) for s in SHAPES_W]
    pb = [torch.nn.Parameter(torch.randn(*s, generator=gen).cuda()) for s in SHAPES_B]
    groups = FlatGroup(pw, pad_to=64, name="weights"), FlatGroup(pb, pad_to=64, name="norms_biases")
    for g in groups:
        for p in g.params:
            p.grad.copy_(torch.randn(p.shape, generator=gen))
    assert [g.numel for g in groups] == [NW, NB]
    assert groups[0].master is not None and groups[0].grad.dtype == torch.bfloat16
    assert groups[1].master is None and groups[1].grad.dtype == torch.float32
    return groups


def _p(name, off=0):
    return (name, off)


# ---- the expected records ----------------------------------------------------------------------
SGD_HP = dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.01)
ADAM_HP = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
LAMB_HP = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
LARS_HP = dict(lr=0.1, momentum=0.9, weight_decay=0.01, trust=0.1, eps=1e-8)
BC1, BC2 = 1.0 - 0.9 ** 1, 1.0 - 0.999 ** 1  # the host's bias corrections of step 1

BEGIN = (BC, (_p("t"), _p("bc"), 0.9, 0.999, 0, S))  # seed: the host's count before the step
CLIP_NORMS = [("kfa_chunk_sumsq", (_p("grad0"), 1, _p("chunks0"), CW, _p("gpart"), S)),
              ("kfa_chunk_sumsq", (_p("grad1"), 0, _p("chunks1"), CB, _p("gpart", 4 * CW), S))]
CLIP_FINISH = ("kfa_clip_finish", (_p("gpart"), CW + CB, 0.5, 1.0, _p("clip"), S))


def _sgd(nesterov):
    return [("kfa_sgd_step", (_p("w0"), _p("wb0"), _p("grad0"), 1, _p("mom0"), NW, 0.1, 0.9, 0.0, 0.01, nesterov,
                              0.5, 1, S)),
            ("kfa_sgd_step", (_p("w1"), None, _p("grad1"), 0, _p("mom1"), NB, 0.1, 0.9, 0.0, 0.0, nesterov,
                              0.5, 1, S))]


ADAM = [BEGIN,
        ("kfa_adam_step", (_p("w0"), _p("wb0"), _p("grad0"), 1, _p("m0"), _p("v0"), NW, 0.01, 0.9, 0.999, 1e-8, 0.1,
                           BC1, BC2, 0.5, _p("bc"), S)),
        ("kfa_adam_step", (_p("w1"), None, _p("grad1"), 0, _p("m1"), _p("v1"), NB, 0.01, 0.9, 0.999, 1e-8, 0.0,
                           BC1, BC2, 0.5, _p("bc"), S))]
ADAM_CLIP = [BEGIN, *CLIP_NORMS, CLIP_FINISH,
             ("kfa_adam_step_clip", (_p("w0"), _p("wb0"), _p("grad0"), 1, _p("m0"), _p("v0"), NW, 0.01, 0.9, 0.999,
                                     1e-8, 0.1, 0.5, _p("bc"), _p("clip", 4), S)),
             ("kfa_adam_step_clip", (_p("w1"), None, _p("grad1"), 0, _p("m1"), _p("v1"), NB, 0.01, 0.9, 0.999,
                                     1e-8, 0.0, 0.5, _p("bc"), _p("clip", 4), S))]
# update(0, 64, 4096): fp32 buffers 256 bytes in, bf16 ones 128
ADAM_RANGED = [BEGIN,
               ("kfa_adam_step", (_p("w0", 256), _p("wb0", 128), _p("grad0", 128), 1, _p("m0", 256), _p("v0", 256),
                                  4032, 0.01, 0.9, 0.999, 1e-8, 0.1, BC1, BC2, 0.5, _p("bc"), S))]


def _lamb(clip, adapt):
    dcoef = _p("clip", 4) if clip else None
    part0, ratio0 = (_p("part0"), _p("ratio0")) if adapt else (None, None)
    rec = [BEGIN] + (CLIP_NORMS + [CLIP_FINISH] if clip else [])
    rec.append(("kfa_lamb_stage1", (_p("w0"), _p("grad0"), 1, _p("m0"), _p("v0"), _p("chunks0"), CW, part0, 0.9, 0.999,
                                    1e-6, 0.01, 0.5, _p("bc"), dcoef, S)))
    if adapt:
        rec.append(("kfa_lamb_ratio", (_p("part0"), _p("tens0"), TW, _p("ratio0"), S)))
    rec += [("kfa_lamb_stage2", (_p("w0"), _p("wb0"), _p("m0"), _p("v0"), _p("chunks0"), CW, ratio0, 0.01, 1e-6, 0.01,
                                 _p("bc"), S)),
            ("kfa_lamb_stage1", (_p("w1"), _p("grad1"), 0, _p("m1"), _p("v1"), _p("chunks1"), CB, None, 0.9, 0.999,
                                 1e-6, 0.0, 0.5, _p("bc"), dcoef, S)),
            ("kfa_lamb_stage2", (_p("w1"), None, _p("m1"), _p("v1"), _p("chunks1"), CB, None, 0.01, 1e-6, 0.0,
                                 _p("bc"), S))]
    return rec


def _lars(clip, adapt):
    dcoef = _p("clip", 4) if clip else None
    rec = []
    if adapt:  # the adapting space's norms pass leaves its g^2 partials where the clip takes them
        rec.append(("kfa_lars_norms", (_p("w0"), _p("grad0"), 1, _p("chunks0"), CW, _p("part0"), _p("gpart"), S)))
    elif clip:
        rec.append(CLIP_NORMS[0])
    if clip:
        rec += [CLIP_NORMS[1], CLIP_FINISH]
    if adapt:
        rec.append(("kfa_lars_ratio", (_p("part0"), _p("gpart"), _p("tens0"), TW, _p("ratio0"), 0.5, dcoef, 0.1, 0.01,
                                       1e-8, S)))
    rec += [("kfa_lars_apply", (_p("w0"), _p("wb0"), _p("grad0"), 1, _p("mom0"), _p("chunks0"), CW,
                                _p("ratio0") if adapt else None, 0.1, 0.9, 0.01, 0, 0.5, dcoef, S)),
            ("kfa_lars_apply", (_p("w1"), None, _p("grad1"), 0, _p("mom1"), _p("chunks1"), CB, None, 0.1, 0.9, 0.0, 0,
                                0.5, dcoef, S))]
    return rec


def _make(kind, **kw):
    from kubeflow_controller_amd.ops import optim
    cls, hp = {"sgd": (optim.FusedSGD, SGD_HP), "adam": (optim.FusedAdam, ADAM_HP),
               "lamb": (optim.FusedLAMB, LAMB_HP), "lars": (optim.FusedLARS, LARS_HP)}[kind]
    return cls(_groups(), **hp, **kw)


CASES = {
    "sgd": ("sgd", {}, _sgd(0)),
    "sgd_nesterov": ("sgd", dict(nesterov=True), _sgd(1)),
    "adam": ("adam", {}, ADAM),
    "adam_clip": ("adam", dict(max_grad_norm=1.0), ADAM_CLIP),
    "lamb": ("lamb", {}, _lamb(False, True)),
    "lamb_clip": ("lamb", dict(max_grad_norm=1.0), _lamb(True, True)),
    "lamb_no_adapt": ("lamb", dict(adapt_groups=()), _lamb(False, False)),
    "lars": ("lars", {}, _lars(False, True)),
    "lars_clip": ("lars", dict(max_grad_norm=1.0), _lars(True, True)),
    "lars_no_adapt": ("lars", dict(adapt_groups=()), _lars(False, False)),
    "lars_no_adapt_clip": ("lars", dict(adapt_groups=(), max_grad_norm=1.0), _lars(True, False)),
}


def _compare(got, want):
    assert [n for n, _ in got] == [n for n, _ in want]
    for k, ((name, a), (_, b)) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, name)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x == y and type(x) is type(y), (k, name, i, PROTOS[name][i][0], x, y)


@pytest.mark.parametrize("case", list(CASES))
def test_one_step_launch_record(case, made):
    kind, kw, want = CASES[case]
    opt = _make(kind, **kw)
    assert [(t.nchunks, t.ntens) for t in _tables(opt)] in ([], [(CW, TW), (CB, TB)])
    del made[:]
    opt.step(grad_scale=0.5)
    torch.cuda.synchronize()
    _compare(_named(made, opt), want)
    assert opt.step_count == 1


def test_adam_ranged_update_launch_record(made):
    opt = _make("adam")
    del made[:]
    opt.begin_step()
    opt.update(0, 64, 4096, grad_scale=0.5)
    opt.update(1, 8, 8)  # an empty range: no launch
    torch.cuda.synchronize()
    _compare(_named(made, opt), ADAM_RANGED)


def test_the_cases_reach_every_entry_of_the_source():  # (added after the refactor: the parent kept dead entries)
    seen = {n for _, _, want in CASES.values() for n, _ in want}
    assert seen | {"kfa_f32_to_bf16"} == set(PROTOS)  # the plain bf16 copy is no optimizer step
    for name, proto in PROTOS.items():
        assert len(_lib._SIGS[name]) == len(proto), name

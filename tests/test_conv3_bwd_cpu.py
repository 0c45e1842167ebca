"""``ops.conv.TailBwdLink`` (of ``CONV3_BWD``): the hand-off's state machine, on the CPU with the kernel library
stubbed out (no GPU call): placeholder identity, the materialise fallback on a foreign ``dy`` or
when a gradient is not wanted, and no arming in eval mode or on the CPU."""
import types

import pytest
import torch

from kubeflow_controller_amd.ops import _lib, conv as convmod


@pytest.fixture
def calls(monkeypatch):
    made = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: made.append(name))
    monkeypatch.setattr(_lib, "stream", lambda: 0)
    return made


def _deferred():
    link = convmod.TailBwdLink(convmod.CONV3_BWD)
    assert link.state == "armed" and link.take() and not link.take()  # picked up once
    g, x3 = torch.randn(2, 8, 3, 3), torch.randn(2, 8, 3, 3)
    ph = torch.empty_like(x3)
    link.defer(g, x3, torch.zeros(18, dtype=torch.uint8), torch.zeros(24), ph)
    assert link.state == "deferred"
    return link, ph


def test_defer_needs_a_taken_link():
    link = convmod.TailBwdLink(convmod.CONV3_BWD)
    with pytest.raises(RuntimeError):
        link.defer(None, None, None, None, None)


def test_placeholder_identity():
    link, ph = _deferred()
    assert link.is_placeholder(ph)
    assert link.is_placeholder(ph.view_as(ph))      # the same memory through another wrapper
    assert not link.is_placeholder(ph.clone())      # a foreign tensor of the same shape
    assert not link.is_placeholder(ph[:1])
    assert not link.is_placeholder(None)


def test_materialize_runs_the_apply_pass_once(calls):
    link, ph = _deferred()
    link.materialize()
    assert calls == ["kfa_bn_bwd_apply_only"] and link.state == "done"
    assert link.g is None and link.placeholder is None  # nothing kept alive
    link.materialize()  # no second pass
    assert calls == ["kfa_bn_bwd_apply_only"]
    assert not link.is_placeholder(ph)


def _ctx(link, x, w, need=(True, True)):
    return types.SimpleNamespace(saved_tensors=(x, w), tail=link, needs_input_grad=need + (False,) * 7, join=None,
                                 bn_link=None, stride=1, pad=0, wparam=None)


def test_backward_takes_the_fused_entry_only_for_the_placeholder(calls, monkeypatch):
    x, w = torch.randn(2, 4, 3, 3), torch.randn(8, 4, 1, 1)
    monkeypatch.setattr(convmod, "wgrad_ok", lambda *a: True)
    monkeypatch.setattr(convmod, "TUNE", False)  # (with the tuner on, only a decision already made counts)
    monkeypatch.setattr(convmod.CONV3_BWD, "enabled", True)
    fused = []
    monkeypatch.setattr(convmod._ConvFn, "_backward_fused", staticmethod(lambda ctx, tail, x, w: fused.append(tail) or "fused"))
    link, ph = _deferred()
    assert convmod._ConvFn.backward(_ctx(link, x, w), ph) == "fused"
    assert fused == [link] and calls == []

    # a foreign dy: dx3 is materialised first, then the ordinary path (no gradient wanted here)
    link, ph = _deferred()
    out = convmod._ConvFn.backward(_ctx(link, x, w, (False, False)), ph.clone())
    assert calls == ["kfa_bn_bwd_apply_only"] and link.state == "done" and out[0] is None and out[1] is None

    # the placeholder, but the weight gradient is not wanted: the fallback again
    del calls[:]
    link, ph = _deferred()
    monkeypatch.setattr(convmod, "conv_dgrad", lambda *a, **k: "dx")
    out = convmod._ConvFn.backward(_ctx(link, x, torch.randn(64, 8, 1, 1), (True, False)), ph)
    assert calls == ["kfa_bn_bwd_apply_only"] and out[0] == "dx" and len(fused) == 1

    # the switch turned off between forward and backward: the fallback too
    del calls[:]
    monkeypatch.setattr(convmod.CONV3_BWD, "enabled", False)
    link, ph = _deferred()
    convmod._ConvFn.backward(_ctx(link, x, w, (False, False)), ph)
    assert calls == ["kfa_bn_bwd_apply_only"] and len(fused) == 1


def test_no_arming_on_cpu_or_in_eval(calls, monkeypatch):
    monkeypatch.setattr(convmod.CONV3_BWD, "route", lambda *a, **k: True)
    x = torch.randn(1, 64, 4, 4, requires_grad=True)
    w = torch.randn(256, 64, 1, 1, requires_grad=True)
    y = convmod.conv2d(x, w, tail_link=True)
    assert getattr(y, "_kfa_tail_link", None) is None and calls == []
    # a CPU bottleneck in training runs plain PyTorch end to end
    from kubeflow_controller_amd.models.resnet import Bottleneck
    blk = Bottleneck(256, 64, 1)
    xb = torch.randn(2, 256, 4, 4, requires_grad=True)
    blk(xb).sum().backward()
    assert xb.grad is not None and calls == []
    # eval: the model does not ask for the link, and conv2d does not arm without autograd
    asked = []
    real = convmod.conv2d
    monkeypatch.setattr(convmod, "conv2d", lambda *a, **k: asked.append(a[-1] if len(a) > 6 else k.get("tail_link")) or real(*a, **k))
    blk.eval()
    with torch.no_grad():
        blk(xb)
    assert not any(asked)
    assert convmod.conv3_bwd_shape_ok((2, 64, 4, 4), (256, 64, 1, 1), 1, 0)
    assert not convmod.conv3_bwd_shape_ok((2, 64, 4, 4), (256, 64, 1, 1), 2, 0)
    assert not convmod.conv3_bwd_shape_ok((2, 64, 4, 4), (256, 64, 3, 3), 1, 1)
    assert not convmod.conv3_bwd_shape_ok((2, 64, 4, 4), (128, 64, 1, 1), 1, 0)

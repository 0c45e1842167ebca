"""``kfa_conv2_bwd_fused``'s host plan without a GPU: the partial-workspace size, the refusal codes
(returned before anything is launched), and the ``TailBwdLink`` hand-off's mask rule and
materialise fallback with the kernel library stubbed out."""
import pytest
import torch

from kubeflow_controller_amd.ops import _lib, conv as convmod


def _part(Nb, H, W, C, Co, max_blocks):
    return _lib.lib().kfa_conv2_bwd_part_floats(Nb, H, W, C, Co, max_blocks)


def test_part_floats_counts_the_blocks_with_tiles():
    slab = 9 * 64 * 64
    assert _part(2, 6, 5, 64, 64, 1) == slab              # 60 pixels: one tile
    assert _part(2, 16, 16, 64, 64, 8) == 2 * slab        # two exact tiles, fewer than the cap
    assert _part(5, 12, 10, 64, 64, 1) == slab            # three tiles in one block
    assert _part(1, 56, 56, 64, 64, 2) == 2 * slab        # 12.25 tiles over two blocks
    assert _part(256, 56, 56, 64, 64, 256) == 256 * slab
    # not covered: no workspace
    assert _part(2, 6, 5, 128, 128, 1) == 0
    assert _part(2, 6, 5, 64, 256, 1) == 0
    assert _part(1, 2, 63, 64, 64, 1) == 0                # 256 + 2 * 64 + 1 rows > 384
    assert _part(1, 2, 62, 64, 64, 1) == slab             # 383 rows + the zero row fit
    assert _part(1 << 12, 64, 64, 64, 64, 1) == 0         # 2^24 pixels


@pytest.mark.parametrize("geom,code", [
    ((2, 6, 5, 64, 64, 1, 1, 1, 0), -1),      # a 1x1
    ((2, 6, 5, 64, 64, 3, 3, 2, 1), -1),      # stride 2
    ((2, 6, 5, 64, 64, 3, 3, 1, 0), -1),      # not 'same' padding
    ((2, 6, 5, 128, 128, 3, 3, 1, 1), -1),    # C = 128
    ((2, 6, 5, 64, 256, 3, 3, 1, 1), -1),     # Co != 64
    ((1 << 12, 64, 64, 64, 64, 3, 3, 1, 1), -2),  # offsets past 32 bits
    ((1, 2, 63, 64, 64, 3, 3, 1, 1), -4),     # a W whose halo does not fit
    ((2, 6, 5, 64, 64, 3, 3, 1, 1), -1),      # covered, but no operands: still no launch
])
def test_entry_refuses_before_any_launch(geom, code):
    fn = _lib.lib().kfa_conv2_bwd_fused
    Nb, H, W, C, Co, R, S, stride, pad = geom
    assert fn(None, None, None, None, None, None, None, None, 1, 0, None, Nb, H, W, C, Co, R, S, stride, pad,
              None, None, None, 0, None, None, 1, None) == code


def test_shape_rule_matches_the_entry():
    ok = convmod.conv2_bwd_shape_ok
    assert ok((256, 64, 56, 56), (64, 64, 3, 3), 1, 1)
    assert ok((1, 64, 2, 62), (64, 64, 3, 3), 1, 1) and not ok((1, 64, 2, 63), (64, 64, 3, 3), 1, 1)
    assert not ok((2, 64, 6, 5), (64, 64, 3, 3), 2, 1)
    assert not ok((2, 64, 6, 5), (64, 64, 1, 1), 1, 0)
    assert not ok((2, 128, 6, 5), (128, 128, 3, 3), 1, 1)
    assert not ok((1 << 12, 64, 64, 64), (64, 64, 3, 3), 1, 1)


def test_link_takes_scale_shift_masks_only_and_materializes_with_them(monkeypatch):
    made = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: made.append((name, a)))
    monkeypatch.setattr(_lib, "stream", lambda: 0)
    ss, mb = torch.zeros(16), torch.zeros(18, dtype=torch.uint8)
    assert convmod.CONV2_BWD.mask_ok(ss, None)
    assert not convmod.CONV2_BWD.mask_ok(None, mb) and not convmod.CONV2_BWD.mask_ok(None, None)
    assert convmod.CONV3_BWD.mask_ok(None, mb) and not convmod.CONV3_BWD.mask_ok(ss, None)
    link = convmod.TailBwdLink(convmod.CONV2_BWD)
    assert link.take()
    g, x2 = torch.randn(2, 8, 3, 3), torch.randn(2, 8, 3, 3)
    ph = torch.empty_like(x2)
    link.defer(g, x2, None, torch.zeros(24), ph, True, ss)
    assert link.is_placeholder(ph) and link.ss is ss
    link.materialize()
    assert [n for n, _ in made] == ["kfa_bn_bwd_apply_only"] and link.state == "done" and link.ss is None
    args = made[0][1]
    assert args[8] == ss.data_ptr() and args[9] is None  # the mask source handed to the apply pass: ss, no bits

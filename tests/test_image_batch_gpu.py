"""The input batch kernel (``kfa_image_batch``) against ``image_batch_reference`` on the
CPU: direct mode bit for bit, resample mode against a float64 reference within one
bf16 ulp, no element exempt."""
import pytest
import torch
import torch.nn.functional as F

from kubeflow_controller_amd.ops import image as I

pytestmark = pytest.mark.gpu
MEAN, STD = I.IMAGENET_MEAN, I.IMAGENET_STD
HS, WS = 37, 41
SIZES = [(32, 32), (30, 20)]  # vector path (Wo % 8 == 0) and the scalar path


def _dev():
    return torch.device("cuda")


def _store(n=4, hs=HS, ws=WS, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, hs, ws, 3), dtype=torch.uint8, generator=g), torch.arange(n) * 7 + 3


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 6)


def _run(src, labels, params, out_hw, dtype=torch.bfloat16):
    x, y = I.image_batch(src.to(_dev()), labels.to(_dev()), params, MEAN, STD, out_hw, dtype)
    assert x.shape == (params.shape[0], 3, *out_hw) and x.is_contiguous(memory_format=torch.channels_last)
    return x.cpu(), y.cpu()


def _bits(t):
    return t.contiguous(memory_format=torch.channels_last).view(torch.int16 if t.dtype == torch.bfloat16
                                                                 else torch.int32)


def _direct_rows(ho, wo):
    """Boxes at each corner, flipped and not, a pad-and-crop box at (-4, -4) and one
    overhanging the bottom-right corner by 4; three samples per launch."""
    rows = []
    for y0, x0 in [(0, 0), (0, WS - wo), (HS - ho, 0), (HS - ho, WS - wo), (-4, -4), (HS - ho + 4, WS - wo + 4)]:
        for flip in (0, 1):
            rows.append([len(rows) % 4, y0, x0, ho, wo, flip])
    return [rows[a:a + 3] for a in range(0, len(rows), 3)]


def _resample_rows():
    boxes = [(0, 0, HS, WS), (11, 17, 9, 7), (5, 6, 1, 1), (8, 0, 1, WS), (HS - 12, WS - 10, 12, 10)]
    rows = []
    for y0, x0, h, w in boxes:
        for flip in (0, 1):
            rows.append([len(rows) % 4, y0, x0, h, w, flip])
    return rows


def _f64_reference(src, params, out_hw):
    """F.interpolate in float64 on the box, flipped afterwards, then normalised -> [B, 3, Ho, Wo]."""
    mean = torch.tensor(MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    inv = torch.tensor(STD, dtype=torch.float32).reciprocal().double().view(1, 3, 1, 1)
    out = []
    for idx, y0, x0, h, w, flip in params.tolist():
        box = src[idx, y0:y0 + h, x0:x0 + w].permute(2, 0, 1).unsqueeze(0).double()
        z = F.interpolate(box, size=out_hw, mode="bilinear", align_corners=False)
        out.append(z.flip(3) if flip else z)
    return (torch.cat(out) - mean) * inv


@pytest.mark.parametrize("out_hw", SIZES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_direct_mode_is_bit_exact(out_hw, dtype):
    src, labels = _store()
    for rows in _direct_rows(*out_hw):
        p = _table(rows)
        x, y = _run(src, labels, p, out_hw, dtype)
        rx, ry = I.image_batch_reference(src, labels, p, MEAN, STD, out_hw, dtype)
        assert torch.equal(_bits(x), _bits(rx)), rows
        assert torch.equal(y, ry)


@pytest.mark.parametrize("out_hw", SIZES)
def test_overhang_never_reads_a_neighbouring_image(out_hw):
    """The source is the inside of a store whose first and last images are all 255:
    what lies outside the first / last real image must come out as the zero pixel."""
    ho, wo = out_hw
    big = torch.full((4, HS, WS, 3), 255, dtype=torch.uint8)
    big[1:3] = _store(2, seed=1)[0]
    dev = big.to(_dev())
    src, labels = dev[1:-1], torch.tensor([5, 9], device=_dev())
    assert src.is_contiguous() and src.data_ptr() != dev.data_ptr()
    rows = [[0, -4, -4, ho, wo, 0], [0, -4, -4, ho, wo, 1], [1, HS - ho + 4, WS - wo + 4, ho, wo, 0],
            [1, HS - ho + 4, WS - wo + 4, ho, wo, 1], [0, -3, WS - wo + 5, ho, wo, 0], [1, HS - ho + 3, -5, ho, wo, 1]]
    p = _table(rows)
    x, _ = I.image_batch(src, labels, p, MEAN, STD, out_hw, torch.bfloat16)
    x = x.cpu()
    rx, _ = I.image_batch_reference(big[1:-1].contiguous(), labels.cpu(), p, MEAN, STD, out_hw, torch.bfloat16)
    assert torch.equal(_bits(x), _bits(rx))
    pad = ((torch.zeros(3) - torch.tensor(MEAN)) * torch.tensor(STD).reciprocal()).to(torch.bfloat16)
    for b, (_, y0, x0, _, _, flip) in enumerate(rows):
        yy = torch.arange(ho) + y0
        xx = torch.arange(wo) + x0
        outside = ((yy < 0) | (yy >= HS)).view(-1, 1) | ((xx < 0) | (xx >= WS)).view(1, -1)
        if flip:
            outside = outside.flip(1)
        assert outside.any()
        got = x[b].permute(1, 2, 0)[outside]
        assert torch.equal(got.view(torch.int16), pad.expand_as(got).contiguous().view(torch.int16)), rows[b]


def test_extreme_rows_and_a_one_pixel_wide_source():
    src = torch.zeros((3, 9, 24, 3), dtype=torch.uint8)
    src[1] = 255
    src[2, ::2] = 255
    labels = torch.arange(3)
    p = _table([[0, 0, 0, 8, 16, 0], [1, 1, 8, 8, 16, 1], [2, -2, 4, 8, 16, 0], [2, 0, 0, 9, 24, 1], [1, 0, 0, 3, 5, 0]])
    for dtype in (torch.bfloat16, torch.float32):
        x, _ = _run(src, labels, p, (8, 16), dtype)
        rx, _ = I.image_batch_reference(src, labels, p, MEAN, STD, (8, 16), dtype)
        assert torch.equal(_bits(x[:3]), _bits(rx[:3]))
        assert torch.allclose(x[3:].float(), rx[3:].float(), rtol=2 ** -7, atol=1e-5)
    thin, tl = _store(2, hs=13, ws=1, seed=2)
    for out_hw in [(8, 8), (6, 3)]:
        ho, wo = out_hw
        q = _table([[0, 0, 0, ho, wo, 0], [1, 2, -3, ho, wo, 1], [1, 5, 1 - wo, ho, wo, 0], [0, 0, 0, 13, 1, 0],
                    [1, 3, 0, 4, 1, 1]])
        x, _ = _run(thin, tl, q, out_hw)
        rx, _ = I.image_batch_reference(thin, tl, q, MEAN, STD, out_hw, torch.bfloat16)
        assert torch.equal(_bits(x[:3]), _bits(rx[:3]))
        assert torch.allclose(x[3:].float(), rx[3:].float(), rtol=2 ** -7, atol=1e-5)


@pytest.mark.parametrize("out_hw", SIZES)
def test_resample_mode_within_one_bf16_ulp_of_float64(out_hw):
    src, labels = _store()
    p = _table(_resample_rows())
    x, y = _run(src, labels, p, out_hw)
    ref = _f64_reference(src, p, out_hw)
    err = (x.double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-5
    print(f"resample bf16 {out_hw}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(y, labels[p[:, 0].long()])


@pytest.mark.parametrize("out_hw", SIZES)
def test_resample_mode_fp32_output(out_hw):
    src, labels = _store()
    p = _table(_resample_rows())
    x, _ = _run(src, labels, p, out_hw, torch.float32)
    ref = _f64_reference(src, p, out_hw)
    err = (x.double() - ref).abs()
    print(f"resample fp32 {out_hw}: max abs err = {float(err.max()):.3g}")
    assert bool((err <= 1e-5).all()), float(err.max())


@pytest.mark.parametrize("out_hw", SIZES)
def test_identity_box_in_resample_arithmetic_equals_direct_mode(out_hw):
    """A box of the output size has sy = i exactly and zero weights on the second
    taps: the resample formula gives the direct-mode bits."""
    ho, wo = out_hw
    src, labels = _store()
    p = _table([[0, 0, 0, ho, wo, 0], [2, HS - ho, WS - wo, ho, wo, 1], [3, 2, 3, ho, wo, 1]])
    x, _ = _run(src, labels, p, out_hw)
    rx, _ = I.image_batch_reference(src, labels, p, MEAN, STD, out_hw, torch.bfloat16, resample_all=True)
    assert torch.equal(_bits(x), _bits(rx))


def test_labels_follow_repeated_and_unordered_indices():
    src, labels = _store(6)
    idx = [5, 0, 5, 3, 3, 1, 4, 0]
    p = _table([[i, 0, 0, 32, 32, 0] for i in idx])
    x, y = _run(src, labels, p, (32, 32))
    assert torch.equal(y, labels[torch.tensor(idx)])
    assert torch.equal(_bits(x[0:1]), _bits(x[2:3])) and not torch.equal(_bits(x[0:1]), _bits(x[1:2]))


def test_offsets_beyond_2_to_31_bytes():
    n = (1 << 31) // (64 * 64 * 3) + 2
    assert n * 64 * 64 * 3 > 1 << 31
    store = torch.empty((n, 64, 64, 3), dtype=torch.uint8, device=_dev())
    last, _ = _store(1, hs=64, ws=64, seed=3)
    store[-1] = last[0].to(_dev())
    labels = torch.zeros(n, dtype=torch.int64, device=_dev())
    labels[-1] = 77
    p = _table([[n - 1, 0, 0, 64, 64, 0]])
    x, y = I.image_batch(store, labels, p, MEAN, STD, (64, 64), torch.bfloat16)
    rx, _ = I.image_batch_reference(last, torch.tensor([77]), _table([[0, 0, 0, 64, 64, 0]]), MEAN, STD, (64, 64),
                                    torch.bfloat16)
    assert torch.equal(_bits(x.cpu()), _bits(rx)) and int(y[0]) == 77


def test_full_workload_shape_both_modes():
    src, labels = _store(4, hs=256, ws=256, seed=4)
    direct = _table([[0, 0, 0, 224, 224, 0], [1, 32, 32, 224, 224, 1], [2, 7, 19, 224, 224, 0], [3, 16, 16, 224, 224, 1]])
    x, y = _run(src, labels, direct, (224, 224))
    rx, ry = I.image_batch_reference(src, labels, direct, MEAN, STD, (224, 224), torch.bfloat16)
    assert torch.equal(_bits(x), _bits(rx)) and torch.equal(y, ry)
    res = _table([[3, 0, 0, 256, 256, 0], [2, 40, 10, 171, 228, 1], [1, 100, 90, 80, 61, 0], [0, 3, 5, 250, 190, 1]])
    x, y = _run(src, labels, res, (224, 224))
    ref = _f64_reference(src, res, (224, 224))
    err = (x.double() - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-5
    print(f"256 -> 224 resample: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(y, labels[res[:, 0].long()])


def test_bad_input_is_refused():
    src, labels = _store()
    d = _dev()
    s, l = src.to(d), labels.to(d)
    outside = _table([[0, 30, 0, 9, 7, 0]])  # a resample box past the bottom edge
    with pytest.raises(ValueError):
        I.image_batch(s, l, outside, MEAN, STD, (32, 32))
    x = torch.empty((1, 3, 32, 32), dtype=torch.bfloat16, device=d, memory_format=torch.channels_last)
    y = torch.empty(1, dtype=torch.int64, device=d)
    m, inv = I._norm_consts(MEAN, STD)
    assert I.launch(s, l, outside.to(d), outside, x, y, m.tolist(), inv.tolist(), 32, 32) == I.ERR_BOX
    with pytest.raises(RuntimeError):
        I.image_batch(s, l, outside, MEAN, STD, (32, 32), validate=False)
    assert I.launch(s, l, _table([[4, 0, 0, 32, 32, 0]]).to(d), _table([[4, 0, 0, 32, 32, 0]]), x, y, m.tolist(),
                    inv.tolist(), 32, 32) == I.ERR_ROW
    ok = _table([[0, 0, 0, 32, 32, 0]])
    with pytest.raises(ValueError):
        I.image_batch(s.float(), l, ok, MEAN, STD, (32, 32))
    with pytest.raises(ValueError):
        I.image_batch(s[:, :, ::2], l, ok, MEAN, STD, (32, 32))
    with pytest.raises(ValueError):
        I.image_batch(s, l.int(), ok, MEAN, STD, (32, 32))
    with pytest.raises(ValueError):
        I.image_batch(s, l, ok.long(), MEAN, STD, (32, 32))
    with pytest.raises(ValueError):
        I.image_batch(s, l, ok, MEAN, STD, (32, 32), torch.float16)
    with pytest.raises(ValueError):
        I.image_batch(s, l, _table([[9, 0, 0, 32, 32, 0]]), MEAN, STD, (32, 32))

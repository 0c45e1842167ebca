"""The conv launch record (``ops.conv.IgemmLaunch``), its geometry builders and its routing
candidates, checked on the CPU against the C prototype and the committed routing table.
The kernel library is never loaded."""
import json
import os

import pytest

from kubeflow_controller_amd.ops import _lib, conv, routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = conv._IGEMM_GEOMETRY


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name, value in dict(PP="auto", PP_MIN_N=256, NARROW=1, NARROW_LONGK=1, BIG=False, BIG_MIN_K=256,
                            BIG_AUTO=True, BIG_AUTO_E=True).items():
        monkeypatch.setattr(conv, name, value)


def _prototype():
    """[(name, is_pointer)] of ``kfa_conv_igemm``'s parameters, from the source."""
    with open(os.path.join(ROOT, "csrc", "kernels", "conv_igemm.hip")) as f:
        params = f.read().split("KFA_API int kfa_conv_igemm(", 1)[1].split(")", 1)[0]
    out = []
    for p in params.split(","):
        kind, name = p.strip().rsplit(None, 1)
        assert kind == "int" or kind.endswith("*") or kind == "hipStream_t", p
        out.append((name, kind != "int"))
    return out


def test_field_order_is_the_c_prototype():
    proto = _prototype()
    assert len(proto) == 33
    assert conv._IGEMM_FIELDS == [n for n, _ in proto]
    assert proto[23][0] == "variant" and proto[24][0] == "stats"
    sig = _lib._SIGS["kfa_conv_igemm"]
    assert sig == [_lib.P if ptr else _lib.I for _, ptr in proto]
    assert GEO == [n for n, _ in proto[4:23]]
    with pytest.raises(TypeError):
        conv.IgemmLaunch(Nb=1)
    with pytest.raises(TypeError):
        _same3x3(64, 28).replace(varient=1)


def _table():
    with open(os.path.join(ROOT, "kubeflow_controller_amd", "ops", "routes_gfx950.json")) as f:
        doc = json.load(f)
    keys = [k for k in doc["routes"] if k.startswith(("conv_fwd|", "conv_dgrad|"))]
    return doc, keys


def _launch_of_key(key):
    kind, ints = key.split("|")
    ints = [int(v) for v in ints.split(",")]
    assert len(ints) == 23
    E, stats, bn_x, add_mb = (1 if f else None for f in ints[19:])
    a = conv.IgemmLaunch(**dict(zip(GEO, ints[:19])), E=E, stats=stats, bn_x=bn_x, add_mb=add_mb)
    return kind, a.replace(variant=conv._variant(a.M, a.N, a.K, E is not None))


def test_keys_and_candidates_match_the_committed_table():
    doc, keys = _table()
    assert len(keys) == 55
    for key in keys:
        kind, a = _launch_of_key(key)
        assert routes.key_str(kind, a.route_key()) == key
        assert a.routed, key
        names = [n for n, _ in a.candidates()]
        assert names[0] == "igemm" and len(set(names)) == len(names), key
        assert set(names) == set(doc["timings_ms"][key]), key
        assert doc["routes"][key] in names, key
        order = ["igemm", "pp", "pp512", "igemm128", "igemm128x64", "igemm256x64", "halo"]
        assert names == [n for n in order if n in names], key


def _resnet50_convs(batch=256):
    """(x_shape, w_shape, stride, pad, has_dgrad) of every conv of ResNet-50 v1.5 at 224 x 224."""
    convs = [((batch, 16, 115, 115), (64, 16, 4, 4), 1, 0, False)]  # the space-to-depth stem
    cin, hw = 64, 56
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            convs.append(((batch, cin, hw, hw), (planes, cin, 1, 1), 1, 0, True))
            convs.append(((batch, planes, hw, hw), (planes, planes, 3, 3), s, 1, True))
            if b == 0:
                convs.append(((batch, cin, hw, hw), (4 * planes, cin, 1, 1), s, 0, True))
            hw //= s
            convs.append(((batch, planes, hw, hw), (4 * planes, planes, 1, 1), 1, 0, True))
            cin = 4 * planes
    return convs


def test_geometry_builders_reproduce_the_table_geometries():
    _, keys = _table()
    table = {tuple(int(v) for v in k.split("|")[1].split(",")[:19]) for k in keys}
    assert len(table) == 54
    built, extra = set(), []
    for x_shape, w_shape, stride, pad, has_dgrad in _resnet50_convs():
        geos = [conv.fwd_geometry(x_shape, w_shape, stride, pad)]
        if has_dgrad:
            assert w_shape[0] % 64 == 0 and w_shape[1] % 8 == 0
            dy_shape = (x_shape[0], w_shape[0], geos[0].P, geos[0].Q)
            classes = conv.dgrad_geometries(dy_shape, w_shape, x_shape, stride, pad)
            assert len(classes) == stride * stride
            for g, (r0, dr, Rs, s0, ds, Ss) in classes:
                assert (dr, ds) == (stride, stride) and (g.R, g.S) == (Rs, Ss)
                assert Rs == len(range(r0, w_shape[2], dr)) and Ss == len(range(s0, w_shape[3], ds))
                geos.append(g)
        for g in geos:
            geo = tuple(getattr(g, n) for n in GEO)
            if g.K > 0:
                built.add(geo)
            else:
                extra.append((g, stride, w_shape))
    assert built == table
    assert len(extra) == 9
    assert all(g.K == 0 and stride == 2 and w_shape[2:] == (1, 1) for g, stride, w_shape in extra)


def _same3x3(C, W, dgrad=False, **kw):
    ra = -1 if dgrad else 1
    a = conv.IgemmLaunch(Nb=4, H=W, W=W, C=C, P=W, Q=W, R=3, S=3, sa=1, ra=ra, oa=-ra, ob=-ra, N=C, OH=W, OW=W,
                         os=1, oph=0, opw=0, ldd=C, **kw)
    return a.replace(variant=conv._variant(a.M, a.N, a.K, a.E is not None))


def _has_halo(a):
    return ("halo", 7) in a.candidates()


@pytest.mark.parametrize("C", [64, 128])
def test_halo_eligibility(C):
    assert _has_halo(_same3x3(C, 28)) and _has_halo(_same3x3(C, 28, dgrad=True))
    assert _has_halo(_same3x3(C, 28, stats=1, bn_x=1, bn_ss=1, bn_relu=1))
    assert not _has_halo(_same3x3(C, 28, E=1))
    assert not _has_halo(_same3x3(C, 28, bn_x=1, bn_y=1, bn_relu=1))
    assert not _has_halo(_same3x3(2 * C if C == 128 else 192, 28))
    base = _same3x3(C, 28)
    for change in (dict(R=1, S=1, oa=0, ob=0), dict(sa=2, P=14, Q=14, OH=14, OW=14), dict(oa=0, ob=0, P=26, Q=26),
                   dict(os=2, OH=56, OW=56), dict(R=5, S=5, oa=-2, ob=-2)):
        assert not _has_halo(base.replace(**change)), change

    # LDS bound: (C/64) * round32(bm + 2 (W + 1) + 32) * 128 + weight ring <= 160 KiB
    def lds(W):
        bm, ring = (256, 3 * 8192) if C == 64 else (128, 2 * 16384)
        return (C // 64) * ((bm + 2 * (W + 1) + 32) // 32 * 32) * 128 + ring
    fits = [W for W in range(8, 1024) if lds(W) <= 160 * 1024]
    wmax = max(fits)
    assert fits == list(range(8, wmax + 1)) and lds(wmax + 1) > 160 * 1024
    for dgrad in (False, True):
        assert _has_halo(_same3x3(C, wmax, dgrad))
        assert not _has_halo(_same3x3(C, wmax + 1, dgrad))

"""GPU: the focal operations (insar_unet_ca_amd/focal.py on csrc/focal.hip) against the numpy restatement of tests/focal_ref.py
(pinned by Python integers in tests/test_focal_host.py). Every comparison is bitwise and covers every pixel of the values and of
the valid plane.

Shapes, with TH x TW the tile of `insar_focal_tile`: 1 x 1, 1 x 37, 37 x 1, 5 x 3 (with R = 15 a window larger than the raster),
(TH + 1) x (TW + 1) (one past a tile edge both ways), (2 TH - 1) x (2 TW + 3) (tile seams and a width that is no multiple of 4),
and three planes with one shared `valid`. Radii 0, 1, 7, 15."""
import functools

import numpy as np
import pytest
import torch

from insar_unet_ca_amd._lib import InsarError
from tests import focal_ref as ref

pytestmark = pytest.mark.gpu
RADII = (0, 1, 7, 15)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _shapes():
    from insar_unet_ca_amd import focal as fc
    tiles = {fc.focal_tile(r) for r in RADII}
    out = [(1, 1), (1, 37), (37, 1), (5, 3)]
    for TH, TW in sorted(tiles):
        out += [(TH + 1, TW + 1), (2 * TH - 1, 2 * TW + 3)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _speckle(shape, holes=True):
    a = ref.speckle(shape, 1000 * shape[-2] + shape[-1], holes)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _valid(H, W):
    v = ref.valid_plane(H, W, 7 * H + W)
    v.setflags(write=False)
    return v


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)        # a copy: the cached arrays are read-only


def _taps(R, kind):
    from insar_unet_ca_amd import focal as fc
    if kind == "box":
        return fc.box_taps(R)
    k = (np.arange(2 * R + 1) * 37 % 11).astype(np.int32)            # not symmetric, with zeros; the sum stays below 4096
    k[0] += 1
    return k


def _same(got, want, what):
    out, ok = got
    w_out, w_ok = want
    assert out.dtype == _t(w_out, "cpu").dtype and ok.dtype == torch.uint8 and tuple(out.shape) == w_out.shape, what
    g_out, g_ok = out.cpu().numpy(), ok.cpu().numpy()
    bad = int((g_out.view(np.uint8).reshape(-1, g_out.itemsize) != w_out.view(np.uint8).reshape(-1, g_out.itemsize)).any(axis=1).sum())
    print(f"{what}: {int(w_ok.sum())} of {w_ok.size} outputs valid, {bad} values and {int((g_ok != w_ok).sum())} valid bytes differ")
    assert np.array_equal(g_ok, w_ok), f"{what}: valid plane"
    assert g_out.tobytes() == w_out.tobytes(), f"{what}: values"


# ---- smoothing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RADII)
def test_smooth_every_shape(dev, R):
    import insar_unet_ca_amd as iu
    for H, W in _shapes():
        r = _speckle((H, W))
        for kind in ("box", "own"):
            k = _taps(R, kind)
            _same(iu.smooth_raster(_t(r, dev), k, return_valid=True), ref.smooth(r, k), f"{H} x {W}, R = {R}, {kind} taps")


def test_smooth_options(dev):
    import insar_unet_ca_amd as iu
    H, W = _shapes()[-1]
    r = _speckle((H, W)).copy()
    r[5, 5:9] = -9999.0
    v = _valid(H, W)
    rt, vt = _t(r, dev), _t(v, dev)
    k = iu.gaussian_taps(1.5)
    for keep in (True, False):
        for cov in (0.0, 0.5, 1.0):
            for valid, nodata, scale in ((None, None, 2 ** 16), (v, None, 2 ** 16), (v, -9999.0, 1000.0)):
                kw = dict(valid=valid, nodata=nodata, scale=scale, min_coverage=cov, keep_invalid=keep)
                got = iu.smooth_raster(rt, k, **dict(kw, valid=None if valid is None else vt), return_valid=True)
                _same(got, ref.smooth(r, k, **kw), f"keep {keep}, coverage {cov}, valid {valid is not None}, nodata {nodata}")
    want = ref.smooth(r, k, valid=v)
    assert (want[1] == 0).any() and (want[1] == 1).any() and np.isnan(want[0]).any()
    # without return_valid the raster alone; out= is written and returned; guard bytes around it stay
    alone = iu.smooth_raster(rt, k, valid=vt)
    assert isinstance(alone, torch.Tensor) and alone.cpu().numpy().tobytes() == want[0].tobytes()
    buf = torch.full((H + 2, W), 7.0, device=dev)
    got = iu.smooth_raster(rt, k, valid=vt, out=buf[1:-1])
    assert got.data_ptr() == buf[1:-1].data_ptr() and got.cpu().numpy().tobytes() == want[0].tobytes()
    assert bool((buf[0] == 7).all()) and bool((buf[-1] == 7).all())
    first = [t.clone() for t in iu.smooth_raster(rt, k, valid=vt, return_valid=True)]
    for _ in range(3):                                                # repeated calls give the same bits
        again = iu.smooth_raster(rt, k, valid=vt, return_valid=True)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, again))
    with pytest.raises(InsarError, match="smooth_raster: out must be"):
        iu.smooth_raster(rt, k, out=rt)
    with pytest.raises(InsarError, match="valid must be a ROCm tensor"):
        iu.smooth_raster(rt, k, valid=torch.from_numpy(np.array(v)))


def test_smooth_all_invalid_and_a_hole_larger_than_the_window(dev):
    import insar_unet_ca_amd as iu
    H, W = _shapes()[-1]
    nothing = np.full((H, W), np.nan, dtype=np.float32)
    for keep in (True, False):
        out, ok = iu.smooth_raster(_t(nothing, dev), iu.box_taps(7), keep_invalid=keep, return_valid=True)
        assert not ok.any() and out.cpu().numpy().tobytes() == np.full((H, W), ref.QNAN).tobytes()
    zeros = np.zeros((H, W), dtype=np.uint8)
    _same(iu.smooth_raster(_t(_speckle((H, W)), dev), iu.box_taps(3), valid=_t(zeros, dev), return_valid=True),
          ref.smooth(_speckle((H, W)), iu.box_taps(3), valid=zeros), "valid plane of zeros")
    r = _speckle((H, W))                                              # its NaN block is 40 x 40: D = 0 in the middle at R = 15
    want = ref.smooth(r, iu.box_taps(15), keep_invalid=False)
    assert (want[1] == 0).any() and (want[1][np.isnan(r)] == 1).any()  # some holes are filled, the middle of the block is not
    _same(iu.smooth_raster(_t(r, dev), iu.box_taps(15), keep_invalid=False, return_valid=True), want, "gap filling at R = 15")


def test_smooth_clamped_values_and_negative_ties(dev):
    import insar_unet_ca_amd as iu
    H, W = _shapes()[-2]
    rng = np.random.default_rng(21)
    big = np.where(rng.random((H, W)) < 0.5, 1e30, -1e30).astype(np.float32)
    big[rng.random((H, W)) < 0.2] = 3.0e4                            # 3e4 * 2^16 < 2^31: not clamped, next to clamped ones
    limit = iu.box_taps(15) * 132
    limit[15] += 4096 - int(limit.sum())                            # the sum at the 4096 limit: |A|, |N| as large as they get
    for k in (limit, iu.box_taps(1)):
        _same(iu.smooth_raster(_t(big, dev), k, return_valid=True), ref.smooth(big, k), f"clamped values, taps sum {int(k.sum())}")
    # small integers under box taps with holes: D takes every value up to 9 and 2 N + D hits exact ties on both sides of zero
    q = rng.integers(-6, 3, (H, W)).astype(np.int32)
    v = (rng.random((H, W)) > 0.4).astype(np.uint8)
    want = ref.smooth(q, iu.box_taps(1), valid=v, keep_invalid=False, fill=-99)
    qp, vp = np.pad(q.astype(np.int64) * (v != 0), 1), np.pad((v != 0).astype(np.int64), 1)
    N = sum(qp[j:j + H, i:i + W] for j in range(3) for i in range(3))
    D = sum(vp[j:j + H, i:i + W] for j in range(3) for i in range(3))
    ties = (D > 0) & ((2 * N + D) % np.maximum(2 * D, 1) == 0)
    assert (ties & (N < 0)).sum() > 20 and (ties & (N > 0)).sum() > 5 and set(range(1, 10)) <= set(np.unique(D).tolist())
    _same(iu.smooth_raster(_t(q, dev), iu.box_taps(1), valid=_t(v, dev), keep_invalid=False, fill=-99, return_valid=True), want,
          "negative ties, int32")
    f = (q.astype(np.float64) / 65536.0).astype(np.float32)
    _same(iu.smooth_raster(_t(f, dev), iu.box_taps(1), valid=_t(v, dev), keep_invalid=False, return_valid=True),
          ref.smooth(f, iu.box_taps(1), valid=v, keep_invalid=False), "negative ties, float32")
    pair = np.array([[-1, -2, 5, -3, 0]], dtype=np.int32)
    out = iu.smooth_raster(_t(pair, dev), [1, 1, 0]).cpu().numpy()
    assert out.tolist() == [[-1, -1, 2, 1, -1]]                      # -1.5 -> -1, 1.5 -> 2, 1 -> 1, -1.5 -> -1: ties towards +infinity


def test_smooth_integer_rasters_and_planes(dev):
    import insar_unet_ca_amd as iu
    H, W = _shapes()[-1]
    rng = np.random.default_rng(33)
    v = _valid(H, W)
    u8 = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    i32 = rng.integers(-(1 << 31), 1 << 31, (3, H, W)).astype(np.int32)
    i32[0, :4] = -(1 << 31)
    for r, nodata, fill in ((u8, 17, 255), (i32, int(i32[1, 9, 9]), -(1 << 31)), (u8[0], None, 0), (i32[2], None, 12345)):
        for k in (iu.gaussian_taps(2.0), _taps(15, "own")):
            kw = dict(nodata=nodata, min_coverage=0.25, fill=fill)
            _same(iu.smooth_raster(_t(r, dev), k, valid=_t(v, dev), return_valid=True, **kw), ref.smooth(r, k, valid=v, **kw),
                  f"{r.dtype} {r.shape}, fill {fill}, taps sum {int(np.sum(k))}")
    # float32 planes: odd H * W puts planes 1 and 2 off the 16-byte grid; the valid plane is shared
    f = np.stack([_speckle((H, W)), _speckle((H, W), False), -_speckle((H, W))])
    _same(iu.smooth_raster(_t(f, dev), iu.box_taps(7), valid=_t(v, dev), return_valid=True), ref.smooth(f, iu.box_taps(7), valid=v), "three planes")
    one = iu.smooth_raster(_t(f[1], dev), iu.box_taps(7), valid=_t(v, dev))
    assert torch.equal(iu.smooth_raster(_t(f, dev), iu.box_taps(7), valid=_t(v, dev))[1].view(torch.int32), one.view(torch.int32))


# ---- rank filters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,radius", [("min", 1), ("min", 15), ("max", 1), ("max", 15), ("median", 1), ("median", 2), ("median", 3)])
def test_rank_every_shape(dev, op, radius):
    import insar_unet_ca_amd as iu
    for H, W in _shapes():
        r = _speckle((H, W)).copy()
        r[0, 0] = -0.0
        if W > 2:
            r[0, 1], r[0, 2] = 0.0, -0.0
        for keep in (True, False):
            _same(iu.rank_filter(_t(r, dev), op, radius, keep_invalid=keep, return_valid=True), ref.rank(r, op, radius, keep_invalid=keep),
                  f"{op} r = {radius}, {H} x {W}, keep {keep}")


def test_rank_signed_zeros_single_pixels_and_min_count(dev):
    import insar_unet_ca_amd as iu
    H, W = _shapes()[-2]
    rng = np.random.default_rng(44)
    z = np.where(rng.random((H, W)) < 0.5, 0.0, -0.0).astype(np.float32)        # only the sign bit tells the values apart
    lonely = np.full((H, W), np.nan, dtype=np.float32)                          # valid pixels so far apart that a window sees one
    lonely[3::8, 5::8] = rng.standard_normal(lonely[3::8, 5::8].shape).astype(np.float32)
    v = _valid(H, W)
    for op, radius in (("min", 2), ("max", 2), ("median", 1), ("median", 3), ("min", 15)):
        _same(iu.rank_filter(_t(z, dev), op, radius, return_valid=True), ref.rank(z, op, radius), f"signed zeros, {op} {radius}")
        if radius <= 3:
            got = iu.rank_filter(_t(lonely, dev), op, radius, keep_invalid=False, return_valid=True)
            _same(got, ref.rank(lonely, op, radius, keep_invalid=False), f"one valid pixel per window, {op} {radius}")
            assert int(got[1].sum()) > int(np.isfinite(lonely).sum())
        for mc in (2, (2 * radius + 1) ** 2 // 2, (2 * radius + 1) ** 2):
            kw = dict(valid=v, nodata=None, min_count=mc, keep_invalid=False)
            _same(iu.rank_filter(_t(_speckle((H, W)), dev), op, radius, **dict(kw, valid=_t(v, dev)), return_valid=True),
                  ref.rank(_speckle((H, W)), op, radius, **kw), f"{op} {radius}, min_count {mc}")
    u8 = rng.integers(0, 256, (2, H, W)).astype(np.uint8)
    i32 = rng.integers(-(1 << 31), 1 << 31, (2, H, W)).astype(np.int32)
    i32[0, :3, :3], i32[1, 5:9, 5:9] = (1 << 31) - 1, -(1 << 31)
    for r, nodata, fill in ((u8, 200, 9), (i32, -(1 << 31), 77)):
        for op, radius in (("min", 7), ("max", 7), ("median", 2)):
            kw = dict(nodata=nodata, fill=fill, min_count=3)
            _same(iu.rank_filter(_t(r, dev), op, radius, valid=_t(v, dev), return_valid=True, **kw), ref.rank(r, op, radius, valid=v, **kw),
                  f"{r.dtype} {op} {radius}")
    buf = torch.zeros(H + 1, W, dtype=torch.int32, device=dev)
    got = iu.rank_filter(_t(i32[0], dev), "median", 1, out=buf[:-1])
    assert got.data_ptr() == buf.data_ptr() and np.array_equal(got.cpu().numpy(), ref.rank(i32[0], "median", 1)[0]) and not buf[-1].any()


# ---- slope -----------------------------------------------------------------------------------------------------------------------------
def test_gradient(dev):
    import insar_unet_ca_amd as iu
    for H, W in _shapes():
        r = _speckle((H, W)).copy()
        r[H // 2, W // 2] = 1e-41                                     # a denormal takes part as it is
        v = _valid(H, W)
        for keep in (True, False):
            for kw in (dict(), dict(spacing=(30.0, 0.1)), dict(valid=v, nodata=float(r[0, 0]) if np.isfinite(r[0, 0]) else 2.0, spacing=(3.0, 7.0))):
                gkw = dict(kw, valid=_t(kw.get("valid"), dev))
                _same(iu.gradient_raster(_t(r, dev), keep_invalid=keep, return_valid=True, **gkw), ref.gradient(r, keep_invalid=keep, **kw),
                      f"gradient {H} x {W}, keep {keep}, {sorted(kw)}")
    H, W = _shapes()[-1]
    # the three stencil cases on both axes, borders and isolated pixels, by construction
    r = np.fromfunction(lambda y, x: (y * y + 3 * x * x).astype(np.float32), (H, W), dtype=np.float32)
    r[10, 10] = r[20, 5:7] = r[30:32, 40] = np.nan
    r[40:43, 20:23] = np.nan
    r[41, 21] = 5.0                                                   # isolated: no component
    want = ref.gradient(r, spacing=(2.0, 0.5))
    assert want[0][1, 10, 9] == np.float32((r[10, 9] - r[10, 8]) * 2.0) and want[0][1, 10, 11] == np.float32((r[10, 12] - r[10, 11]) * 2.0)
    assert want[0][0, 9, 10] == np.float32((r[9, 10] - r[8, 10]) * 0.5) and want[0][1, 0, 0] == np.float32((r[0, 1] - r[0, 0]) * 2.0)
    assert np.isnan(want[0][:, 41, 21]).all() and want[1][41, 21] == 0 and want[0][1, 5, 5] == np.float32((r[5, 6] - r[5, 4]) * 1.0)
    _same(iu.gradient_raster(_t(r, dev), spacing=(2.0, 0.5), return_valid=True), want, "stencils")
    f = np.stack([_speckle((H, W)), r, _speckle((H, W), False)])
    _same(iu.gradient_raster(_t(f, dev), valid=_t(_valid(H, W), dev), return_valid=True), ref.gradient(f, valid=_valid(H, W)), "three planes")
    buf = torch.zeros(3, 2, H, W, device=dev)
    got = iu.gradient_raster(_t(f, dev), out=buf)
    assert got.data_ptr() == buf.data_ptr() and got.cpu().numpy().tobytes() == ref.gradient(f)[0].tobytes()


# ---- launches ----------------------------------------------------------------------------------------------------------------------------
def test_launch_count(dev):
    """One launch per call, counted the way tests/test_hysteresis_gpu.py counts: every entry point on the tape is one launch, and
    nothing else (no copy, no read-back, no torch op) runs between the allocation of the outputs and the return."""
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    H, W = _shapes()[-1]
    r, v = _t(_speckle((3, H, W)), dev), _t(_valid(H, W), dev)
    calls = ((lambda: iu.smooth_raster(r, iu.gaussian_taps(1.5), valid=v, return_valid=True), "insar_focal_smooth"),
             (lambda: iu.smooth_raster(r[0], iu.box_taps(15), nodata=1.0), "insar_focal_smooth"),
             (lambda: iu.rank_filter(r, "min", 15, valid=v), "insar_focal_rank"), (lambda: iu.rank_filter(r, "median", 3), "insar_focal_rank"),
             (lambda: iu.gradient_raster(r, valid=v, return_valid=True), "insar_focal_gradient"))
    for fn, name in calls:
        tape = []
        _lib._TAPE = tape
        try:
            fn()
        finally:
            _lib._TAPE = None
        assert [n for _, _, n in tape] == [name]
    # nothing in a call synchronises or copies: it can sit in a captured graph, and the replay gives the same bits
    k = iu.gaussian_taps(1.5)
    out = torch.empty_like(r)
    want = [t.clone() for t in iu.smooth_raster(r, k, valid=v, return_valid=True)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # as insar_unet_ca_amd/graph.py captures a step
        got = iu.smooth_raster(r, k, valid=v, return_valid=True, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])


# ---- the scene pipeline --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predictor(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((64, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():                                         # split the class map about evenly (tests/test_outlines_gpu.py)
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    return pred, scene


def _equal(x, y):
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_equal(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return x.tobytes() == y.tobytes()
    return x == y


def test_detect_smooths_the_contoured_raster(dev, predictor):
    import insar_unet_ca_amd as iu
    pred, scene = predictor
    det = pred.detect(scene, return_prob=True, min_area=2, contours=dict(levels=[0.5], smooth=1.5))
    raw = iu.contour_lines(det["prob"][1], [0.5])
    smooth, ok = iu.smooth_raster(det["prob"][1], iu.gaussian_taps(1.5), return_valid=True)
    by_hand = iu.contour_lines(smooth, [0.5], valid=ok)
    assert _equal(det["contours"], by_hand)
    w_smooth, w_ok = ref.smooth(det["prob"][1].cpu().numpy(), iu.gaussian_taps(1.5))
    assert smooth.cpu().numpy().tobytes() == w_smooth.tobytes() and np.array_equal(ok.cpu().numpy(), w_ok)
    print(f"detect: 0.5 line {raw['n_vertices']} crossings in {raw['n_lines']} lines, smoothed {by_hand['n_vertices']} in {by_hand['n_lines']}")
    assert by_hand["n_vertices"] != raw["n_vertices"] or by_hand["n_lines"] != raw["n_lines"]
    # the valid plane of a masked predict goes through the smoothing, and the smoothing's valid plane to the lines
    valid = np.ones((64, 96), dtype=np.uint8)
    valid[20:30, 40:60] = 0
    masked = pred.detect(scene, min_area=2, valid=valid, contours=dict(levels=[0.0], raster=scene, smooth=2, scale=1024.0))
    s, m = iu.smooth_raster(_t(scene, dev), iu.gaussian_taps(2.0), valid=masked["valid"], return_valid=True)
    assert not m[20:30, 40:60].any() and bool(m[:20].all())
    assert _equal(masked["contours"], iu.contour_lines(s, [0.0], valid=m, scale=1024.0))
    with pytest.raises(InsarError, match="contours: smooth=6: a Gaussian sigma in pixels, 0 < sigma <= 5"):
        pred.detect(None, contours=dict(levels=[0.5], smooth=6))      # refused before predict looks at the scene


def test_detect_without_smooth_is_unchanged(dev, predictor):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    pred, scene = predictor
    kw = dict(return_prob=True, min_area=2)
    tape = []
    _lib._TAPE = tape
    try:
        a = pred.detect(scene, contours=dict(levels=[0.4, 0.6]), **kw)
    finally:
        _lib._TAPE = None
    assert not [n for _, _, n in tape if n.startswith("insar_focal")]
    b = pred.detect(scene, contours=dict(levels=[0.4, 0.6], smooth=None), **kw)
    plain = pred.detect(scene, **kw)
    assert a.keys() == b.keys() == set(plain) | {"contours"} and _equal(a, b)
    assert all(_equal(plain[k], a[k]) for k in plain)
    assert _equal(a["contours"], iu.contour_lines(plain["prob"][1], [0.4, 0.6]))

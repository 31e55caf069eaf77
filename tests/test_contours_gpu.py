"""GPU: contour lines (insar_unet_ca_amd/contours.py on csrc/contour.hip) against the sequential oracle of
tests/contours_ref.py (pinned by its own invariants in tests/test_contours_host.py).

Every comparison is bitwise: the line table, the vertex array and the counts, once through `contour_lines` and once through the
five phase calls with every buffer inside a guard pattern. The maps are small: a numbering block is 1024 pixels / crossings and
a wave 64 positions, so 64 x 1030 (65 pixel blocks, ~1e4 crossings) crosses every block boundary there is."""
import ctypes

import numpy as np
import pytest
import torch

from tests.contours_ref import LINE_FIELDS, bordered, contours_oracle, quantise, smooth_map

pytestmark = pytest.mark.gpu
PAD = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _compare(out, ref, what):
    for k in ("n_lines", "n_vertices"):
        assert out[k] == ref[k], f"{what}: {k} {out[k]}, oracle {ref[k]}"
    assert out["level_counts"].tolist() == ref["level_counts"].tolist(), what
    assert out["levels_q"].tolist() == ref["levels_q"].tolist() and out["scale"] == ref["scale"], what
    v = out["vertices"].cpu().numpy()
    assert v.dtype == np.int32 and v.shape == (ref["n_vertices"], 2)
    for f in LINE_FIELDS:
        got, want = out["lines"][f], ref["lines"][f]
        assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {f} {got.dtype} {got.shape}"
        assert got.tobytes() == want.tobytes(), f"{what}: {f} differs at lines {np.flatnonzero(got != want)[:8]}"
    assert v.tobytes() == ref["vertices"].tobytes(), f"{what}: vertices differ from row {np.flatnonzero((v != ref['vertices']).any(1))[:8]}"


def _guarded(nbytes, dev, fill=0xA5):
    g = torch.full((PAD + nbytes + PAD,), fill, dtype=torch.uint8, device=dev)
    return g, g[PAD:PAD + nbytes]


def _intact(g, nbytes, fill=0xA5):
    h = g.cpu().numpy()
    return bool((h[:PAD] == fill).all() and (h[PAD + nbytes:] == fill).all())


def _phases(dev, raster, levels_q, *, scale=65536.0, valid=None, nodata=None, max_lines=4096, max_vertices=1 << 16):
    """The five phase calls with scratch, table and vertices inside guards; the result in the shape of contour_lines (E, the raw
    header and the guards' state included)."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import contours as ct
    from insar_unet_ca_amd._lib import call, ptr
    H, W = raster.shape
    L = len(levels_q)
    sb, tb = ct.scratch_bytes(H, W, L, max_lines, max_vertices)
    gs, scratch = _guarded(sb, dev)
    gt, table = _guarded(tb, dev)
    lv = (ctypes.c_int32 * L)(*[int(v) for v in levels_q])
    s = _lib.stream_ptr()
    call("insar_contour_edges", ptr(raster), ct._ELEM[raster.dtype], H, W, float(scale), int(nodata is not None),
         0.0 if nodata is None else float(nodata), ptr(valid), lv, L, max_vertices, ptr(scratch), ptr(table), s)
    torch.cuda.synchronize()
    hdr = table[:192].cpu().numpy().view(np.int32)
    E = int(hdr[ct.HDR_CROSSINGS])
    res = {"E": E, "level_counts": hdr[ct.HDR_LEVELS:ct.HDR_LEVELS + L].astype(np.int64)}
    if 0 < E <= max_vertices:
        gv, verts = _guarded(8 * E, dev)
        call("insar_contour_lead", H, W, L, E, max_vertices, ptr(scratch), s)
        call("insar_contour_rank", H, W, L, E, max_vertices, ptr(scratch), s)
        call("insar_contour_lines", H, W, L, E, max_lines, max_vertices, ptr(scratch), ptr(table), s)
        call("insar_contour_write", H, W, L, E, max_lines, max_vertices, ptr(scratch), ptr(table), ptr(verts), s)
        torch.cuda.synchronize()
        raw = table.cpu().numpy()
        res["n_lines_true"] = int(raw[:192].view(np.int32)[ct.HDR_LINES])
        n = min(res["n_lines_true"], max_lines)
        res.update(lines=ct.lines_from_table(raw, n), vertices=verts.view(torch.int32).reshape(-1, 2), n_lines=n, n_vertices=E)
        res["guards"] = _intact(gs, sb) and _intact(gt, tb) and _intact(gv, 8 * E)
    else:
        res["guards"] = _intact(gs, sb) and _intact(gt, tb)
    return res


_ORACLE = {}


def _check(dev, name, m, levels, **kw):
    """`contour_lines` and the guarded phase calls, bitwise against the oracle; returns (oracle, result)."""
    import insar_unet_ca_amd as iu
    m = np.ascontiguousarray(m)
    if name not in _ORACLE:
        _ORACLE[name] = contours_oracle(m, levels, **kw)
    ref = _ORACLE[name]
    t = torch.from_numpy(m).to(dev)
    dkw = dict(kw)
    if "valid" in dkw:
        dkw["valid"] = torch.from_numpy(np.ascontiguousarray(dkw["valid"])).to(dev)
    out = iu.contour_lines(t, levels, max_lines=4096, max_vertices=1 << 16, **dkw)
    _compare(out, ref, name)
    ph = _phases(dev, t, ref["levels_q"], scale=kw.get("scale", 65536.0), valid=dkw.get("valid"), nodata=kw.get("nodata"))
    assert ph["guards"], f"{name}: a guard was written"
    assert ph["E"] == ref["n_vertices"] and ph["level_counts"].tolist() == ref["level_counts"].tolist(), name
    if ph["E"]:
        assert ph["n_lines_true"] == ref["n_lines"] and torch.equal(ph["vertices"], out["vertices"]), name
        assert all(ph["lines"][f].tobytes() == ref["lines"][f].tobytes() for f in LINE_FIELDS), name
    assert (t.cpu().numpy().tobytes() == m.tobytes())                         # the input is not written
    print(f"{name}: {ref['n_vertices']} crossings, {ref['n_lines']} lines ({int((~ref['lines']['closed']).sum())} open), "
          f"longest {int(ref['lines']['count'].max(initial=0))}")
    return ref, out


# ---- hand-made maps -------------------------------------------------------------------------------------------------------------
def _two_by_two(mask, cut=False):
    hi, lo = 10, (-2 if cut else 0)
    v = [hi if mask >> b & 1 else lo for b in range(4)]
    return np.array([[v[0], v[1]], [v[3], v[2]]], dtype=np.int32)


def test_the_cell_masks(dev):
    for mask in range(16):
        for cut in ((False, True) if mask in (5, 10) else (False,)):
            ref, _ = _check(dev, f"2x2 mask {mask} cut {cut}", _two_by_two(mask, cut), [5])
            assert ref["n_lines"] == (2 if mask in (5, 10) else 0 if mask in (0, 15) else 1)


def spiral_ridge(n=64):
    """float32 n x n: a one-pixel ridge (1.0 on 0.0) spiralling inwards with two pixels between its turns."""
    m = np.zeros((n, n), dtype=np.float32)
    y, x, d = 1, 1, 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[y, x] = 1
    turns = 0
    while turns < 2:
        dy, dx = step[d]
        ny, nx = y + dy, x + dx
        ay, ax = y + 3 * dy, x + 3 * dx
        ok = 1 <= ny < n - 1 and 1 <= nx < n - 1 and m[ny, nx] == 0 and not (0 <= ay < n and 0 <= ax < n and m[ay, ax])
        if ok:
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def corner_cuts(H=40, W=70):
    """float32: single cells of valid nodes between NaN rows and columns, one corner of each above: open lines of 2 vertices."""
    m = np.zeros((H, W), dtype=np.float32)
    y, x = np.mgrid[:H, :W]
    m[(y % 3 == 2) | (x % 3 == 2)] = np.nan
    for by in range(H // 3):
        for bx in range(W // 3):
            k = (by + bx) % 4
            m[3 * by + (k >> 1), 3 * bx + (k & 1)] = 9
    return m


def _nested(H, W):
    y, x = np.mgrid[:H, :W]
    return (100.0 - 3.0 * np.hypot(y - H / 2 + 0.3, x - W / 2 - 0.4)).astype(np.float32)


def _holes(H, W, seed):
    rng = np.random.default_rng(seed)
    v = np.ones((H, W), dtype=np.uint8)
    for _ in range(6):
        y, x = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 6))
        v[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 7))] = 0
    v[0, 0] = v[-1, -1] = 0
    return v


def _cases():
    rng = np.random.default_rng(21)
    peak = np.zeros((3, 3), dtype=np.int32)
    peak[1, 1] = 10
    sm33, sm64 = smooth_map(33, 67, 1), smooth_map(64, 1030, 2, bumps=300, smax=10.0)
    nan33 = sm33.copy()
    nan33[_holes(33, 67, 3) == 0] = np.nan
    nan33[10, 20] = np.inf
    nd = sm33.copy()
    nd[_holes(33, 67, 4) == 0] = -9999.0
    clip = sm33 * np.float32(1e6)
    u8 = rng.integers(0, 256, size=(37, 53)).astype(np.uint8)
    i32 = rng.integers(-1000, 1000, size=(29, 66)).astype(np.int32)
    i32[5, 5], i32[6, 6] = -(1 << 31), (1 << 31) - 1
    eq = rng.integers(0, 4, size=(31, 45)).astype(np.int32)                       # a quarter of the nodes equal each level
    return {
        "1x64": (rng.integers(0, 10, size=(1, 64)).astype(np.int32), [3, 6], {}),
        "64x1": (rng.integers(0, 10, size=(64, 1)).astype(np.int32), [3, 6], {}),
        "peak": (peak, [5], {}), "pit": (10 - peak, [5], {}),
        "flat at the level": (np.full((7, 9), 5, dtype=np.int32), [5], {}),
        "smooth 33x67": (sm33, [0.0], {}),
        "smooth 33x67, 2 levels": (sm33, [-10.0, 10.0], {}),
        "smooth 64x1030, 3 levels": (sm64, [-25.0, 0.0, 25.0], dict(scale=1024.0)),
        "nested, 16 levels": (_nested(41, 59), [10.0 + 5 * k for k in range(16)], dict(scale=256.0)),
        "uint8 speckle": (u8, [64, 128, 200], {}),
        "uint8 nodata": (u8, [100], dict(nodata=7)),
        "int32 speckle": (i32, [-500, 0, 1, 999], {}),
        "int32 nodata": (i32, [0], dict(nodata=-(1 << 31))),
        "spiral ridge": (spiral_ridge(), [0.5], {}),
        "corner cuts": (corner_cuts(), [5], {}),
        "NaN blocks": (nan33, [-10.0, 0.0, 10.0], {}),
        "valid plane": (sm33, [-10.0, 0.0, 10.0], dict(valid=_holes(33, 67, 5))),
        "nodata": (nd, [0.0], dict(nodata=-9999.0)),
        "clipped": (clip, [-3e4, 0.0, 3e4], {}),
        "equal to a level": (eq, [1, 2, 3], {}),
    }


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_against_the_oracle(dev, name):
    m, levels, kw = CASES[name]
    ref, _ = _check(dev, name, m, levels, **kw)
    if name in ("1x64", "64x1", "flat at the level"):
        assert ref["n_vertices"] == 0
    if name == "spiral ridge":
        assert ref["n_lines"] == 1 and ref["lines"]["closed"][0] and 2048 < ref["n_vertices"] < 8192       # a dozen rounds
    if name == "corner cuts":
        assert ref["n_lines"] == 13 * 23 and (ref["lines"]["count"] == 2).all() and not ref["lines"]["closed"].any()
    if name == "smooth 64x1030, 3 levels":
        assert ref["n_vertices"] > 3 * 1024 and (ref["level_counts"] > 0).all()
    if name == "nested, 16 levels":
        assert ref["n_lines"] >= 16 and ref["lines"]["closed"].sum() >= 5 and len(set(ref["lines"]["level"].tolist())) == 16
    if name in ("NaN blocks", "valid plane", "nodata"):
        assert (~ref["lines"]["closed"]).sum() >= 2
    if name == "clipped":
        assert np.abs(quantise(m)[0]).max() == (1 << 31) - 1


def _isolated_pixels(H, W):
    """A uint8 raster that is 2 where y and x are both odd and 0 elsewhere, and its contours at level 1 in closed form: one
    closed line per such pixel through the midpoints of its four lattice edges, from the edge above it clockwise (the pixel on
    the right), led by that edge's id 2 * (pixel - W) + 1."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[1:H - 1:2, 1:W - 1:2] = 2
    y, x = (a.ravel().astype(np.int32) for a in np.mgrid[1:H - 1:2, 1:W - 1:2])
    n = y.size
    four = np.full(n, 4, dtype=np.int32)
    Y, X = 256 * y + 128, 256 * x + 128
    lines = {"line": np.arange(n, dtype=np.int32), "level": np.zeros(n, dtype=np.int32), "closed": np.ones(n, dtype=np.bool_),
             "start": 4 * np.arange(n, dtype=np.int32), "count": four, "leader": 2 * ((y - 1) * W + x) + 1,
             "area2": np.full(n, 2 * 128 * 256, dtype=np.int64), "y0": Y - 128, "x0": X - 128, "y1": Y + 129, "x1": X + 129}
    vertices = np.stack([np.stack([Y - 128, X], 1), np.stack([Y, X + 128], 1), np.stack([Y + 128, X], 1), np.stack([Y, X - 128], 1)], 1)
    return m, {"n_lines": n, "n_vertices": 4 * n, "level_counts": np.array([4 * n]), "levels_q": np.array([1]), "scale": 1.0,
               "lines": lines, "vertices": np.ascontiguousarray(vertices.reshape(-1, 2), dtype=np.int32)}


def test_isolated_pixels_fill_more_than_one_scan_pass(dev):
    """The two array scans take 1024 blocks per pass. 1058 x 1026 pixels are 1061 blocks of 1024 pixels at the one level, and the
    270 336 isolated pixels give 1 081 344 crossings in 1056 blocks of 1024: both scans run a second pass and hand their carry to
    the header (the crossings, the level's count, the lines). The capacities are exact."""
    import insar_unet_ca_amd as iu
    m, ref = _isolated_pixels(1058, 1026)
    assert m.size > 1024 * 1024 and ref["n_vertices"] > 1024 * 1024
    out = iu.contour_lines(torch.from_numpy(m).to(dev), [1], max_lines=ref["n_lines"], max_vertices=ref["n_vertices"])
    _compare(out, ref, "isolated pixels")


@pytest.mark.parametrize("W,E", [(33, 1024), (35, 1088)])
def test_rings_end_on_the_numbering_block_boundary(dev, W, E):
    """A float raster that is 1 at every odd (y, x) of 33 x W and 0 elsewhere, at level 0.5: closed lines of four crossings.
    33 x 33 gives E = 1024, exactly one numbering block of the count / number kernels, and the last leader's line ends on its
    last slot; 33 x 35 gives 1088 and runs into a second block."""
    m = np.zeros((33, W), dtype=np.float32)
    m[1::2, 1::2] = 1.0
    ref, _ = _check(dev, f"odd pixels 33x{W}", m, [0.5])
    assert ref["n_vertices"] == E and ref["n_lines"] == E // 4 and ref["lines"]["closed"].all() and (ref["lines"]["count"] == 4).all()


def test_vector_and_scalar_paths_agree(dev):
    """33 x 67 is off the 4-pixel vector width; 32 x 68 is on it, and a view one element into a buffer is misaligned."""
    import insar_unet_ca_amd as iu
    m = smooth_map(32, 68, 6)
    ref, out = _check(dev, "smooth 32x68", m, [-5.0, 5.0])
    buf = torch.zeros(32 * 68 + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(m).to(dev).reshape(-1)
    _compare(iu.contour_lines(buf[1:].view(32, 68), [-5.0, 5.0]), ref, "misaligned raster")


# ---- round trip through the rasteriser ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smooth", "speckle"])
def test_round_trip_through_rasterise(dev, name):
    import insar_unet_ca_amd as iu
    if name == "smooth":
        m, levels, kw = bordered(smooth_map(45, 83, 8), -1000.0), [-20.0, 0.0, 7.5], dict(scale=4096.0)
    else:
        m, levels, kw = bordered(np.random.default_rng(9).integers(0, 100, size=(38, 61)).astype(np.int32), -1), [25, 50, 75], {}
    H, W = m.shape
    c = iu.contour_lines(torch.from_numpy(m).to(dev), levels, **kw)
    assert c["lines"]["closed"].all()
    q, _ = quantise(m, kw.get("scale", 1.0))
    for i, q_l in enumerate(c["levels_q"]):
        polys = iu.contour_polygons(c, i)
        r = iu.rasterise_polygons(iu.pack_polygons(polys), H, W, device=dev)
        assert int(r["overlap_pixels"]) == 0, (name, i)
        assert (r["labels"].cpu().numpy() == (q >= q_l).astype(np.uint8)).all(), (name, i)


# ---- capacities, scratch, launches ----------------------------------------------------------------------------------------------------
def test_capacities_and_guards(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd._lib import InsarError
    m, levels, kw = CASES["NaN blocks"]
    ref = contours_oracle(m, levels, **kw)
    E, R = ref["n_vertices"], ref["n_lines"]
    t = torch.from_numpy(m).to(dev)
    _compare(iu.contour_lines(t, levels, max_vertices=E, max_lines=R), ref, "capacities exactly as needed")
    with pytest.raises(InsarError, match=rf"contour_lines: {E} vertices exceed max_vertices={E - 1}"):
        iu.contour_lines(t, levels, max_vertices=E - 1, max_lines=R)
    with pytest.raises(InsarError, match=rf"contour_lines: {R} lines exceed max_lines={R - 1}"):
        iu.contour_lines(t, levels, max_vertices=E, max_lines=R - 1)
    # one crossing slot too few: E is reported and nothing is written past the scratch or the header
    ph = _phases(dev, t, ref["levels_q"], max_vertices=E - 1, max_lines=R)
    assert ph["E"] == E and ph["guards"] and "lines" not in ph
    # one record too few: the true count in the header, the first R - 1 records and every vertex as the oracle's
    ph = _phases(dev, t, ref["levels_q"], max_vertices=E, max_lines=R - 1)
    assert ph["guards"] and ph["n_lines_true"] == R and ph["n_lines"] == R - 1
    assert all(ph["lines"][f].tobytes() == ref["lines"][f][:R - 1].tobytes() for f in LINE_FIELDS)
    assert ph["vertices"].cpu().numpy().tobytes() == ref["vertices"].tobytes()


def test_reused_scratch_needs_no_clearing(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd._lib import InsarError
    a, b = smooth_map(33, 67, 1), smooth_map(33, 67, 11)
    b[3:9, 40:50] = np.nan
    levels = [-10.0, 10.0]
    caps = dict(max_lines=512, max_vertices=1 << 14)
    sc = iu.ContourScratch(33, 67, dev, 2, **caps)
    sc.scratch.fill_(0xFF)
    sc.table.fill_(0xFF)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    fresh = [iu.contour_lines(t, levels, **caps) for t in (ta, tb)]
    for t, want in ((ta, fresh[0]), (tb, fresh[1]), (ta, fresh[0])):
        got = iu.contour_lines(t, levels, scratch=sc, **caps)
        assert torch.equal(got["vertices"], want["vertices"]) and got["n_lines"] == want["n_lines"]
        assert all(got["lines"][f].tobytes() == want["lines"][f].tobytes() for f in LINE_FIELDS)
    _compare(fresh[1], contours_oracle(b, levels), "second map")
    with pytest.raises(InsarError, match="scratch of"):
        iu.contour_lines(ta, [0.0], scratch=sc, **caps)


def test_launch_count(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import contours as ct
    for name in ("flat at the level", "peak", "smooth 33x67", "spiral ridge"):
        m, levels, kw = CASES[name]
        tape = []
        _lib._TAPE = tape
        try:
            out = iu.contour_lines(torch.from_numpy(m).to(dev), levels, **kw)
        finally:
            _lib._TAPE = None
        E = out["n_vertices"]
        R = max(E - 1, 0).bit_length()
        per_call = {"insar_contour_scratch_bytes": 0, "insar_contour_edges": 5, "insar_contour_lead": R, "insar_contour_rank": 1 + R,
                    "insar_contour_lines": 3, "insar_contour_write": 2}
        names = [n for _, _, n in tape]
        assert set(names) <= set(per_call), names
        assert sum(per_call[n] for n in names) == ct.launches(E) == (11 + 2 * R if E else 5), (name, E, names)


# ---- the scene pipeline ------------------------------------------------------------------------------------------------------------
def _equal(x, y):
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_equal(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return x.tobytes() == y.tobytes()
    return x == y


def test_detect_with_contours(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd._lib import InsarError
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((64, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():                                         # split the class map about evenly (tests/test_outlines_gpu.py)
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    plain = pred.detect(scene, return_prob=True, min_area=2)
    det = pred.detect(scene, return_prob=True, min_area=2, contours=dict(levels=[0.5]))
    assert "contours" not in plain and set(det) == set(plain) | {"contours"}
    assert all(_equal(plain[k], det[k]) for k in plain)
    direct = iu.contour_lines(det["prob"][1], [0.5])
    assert _equal(det["contours"], direct) and direct["n_lines"] > 2
    _compare(direct, contours_oracle(det["prob"][1].cpu().numpy(), [0.5]), "detect")
    # without return_prob the probabilities are computed for the lines and not returned; another plane, two levels
    quiet = pred.detect(scene, min_area=2, contours=dict(levels=[0.4, 0.6], plane=0, scale=1024.0))
    assert "prob" not in quiet and _equal(quiet["contours"], iu.contour_lines(det["prob"][0], [0.4, 0.6], scale=1024.0))
    # a raster on the scene grid, and the valid plane of a masked predict
    valid = np.ones((64, 96), dtype=np.uint8)
    valid[20:30, 40:60] = 0
    masked = pred.detect(scene, min_area=2, valid=valid, contours=dict(levels=[0.0], raster=scene))
    want = iu.contour_lines(torch.from_numpy(scene).to(dev), [0.0], valid=masked["valid"])
    assert _equal(masked["contours"], want) and (~want["lines"]["closed"]).any()
    with pytest.raises(InsarError, match="contours: a dict of contour_lines keywords with 'levels'"):
        pred.detect(scene, contours=[0.5])
    with pytest.raises(InsarError, match="contours: 'valid' is detect's to give"):
        pred.detect(scene, contours=dict(levels=[0.5], valid=valid))
    print(f"detect: {direct['n_lines']} lines, {direct['n_vertices']} vertices")

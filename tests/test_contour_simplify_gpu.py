"""GPU: contour simplification (`simplify_contours` of insar_unet_ca_amd/contours.py on csrc/contour_simplify.hip) against the
sequential oracle of tests/contour_simplify_ref.py (pinned by its own invariants in tests/test_contour_simplify_host.py).

Every comparison is bitwise: the kept vertices, their positions, every field of the line table, the counts, `rounds` and
`converged`, once through `simplify_contours` and once through the three phase calls with every buffer inside a guard pattern.
The kernels work in blocks of 256 positions and waves of 64, so the rasters (a few hundred vertices) cross a block border or
two and the hand-made polylines (5 000 vertices each, laid so that lines straddle block borders) some forty."""
import numpy as np
import pytest
import torch

from tests import contour_simplify_ref as cr
from tests.contours_ref import bordered, quantise

pytestmark = pytest.mark.gpu
PAD = 4096
TOLERANCES = (0, 0.25, 1, 4)
ROUNDS = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _compare(out, ref, what):
    for k in ("n_lines", "n_vertices", "input_n_vertices", "rounds", "converged"):
        assert out[k] == ref[k] and type(out[k]) is type(ref[k]), f"{what}: {k} {out[k]!r}, oracle {ref[k]!r}"
    assert out["vertices"].dtype == torch.int32 and tuple(out["vertices"].shape) == (ref["n_vertices"], 2), what
    assert out["kept"].dtype == torch.int32 and tuple(out["kept"].shape) == (ref["n_vertices"],), what
    k = out["kept"].cpu().numpy()
    assert k.tobytes() == ref["kept"].tobytes(), f"{what}: kept differs from {np.flatnonzero(k != ref['kept'])[:8]}"
    assert out["vertices"].cpu().numpy().tobytes() == ref["vertices"].tobytes(), f"{what}: vertices differ"
    assert set(out["lines"]) == set(cr.LINE_FIELDS), what
    for f in cr.LINE_FIELDS:
        got, want = out["lines"][f], ref["lines"][f]
        assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {f} {got.dtype} {got.shape}"
        assert got.tobytes() == want.tobytes(), f"{what}: {f} differs at lines {np.flatnonzero(got != want)[:8]}"
    for k in ("level_counts", "levels_q", "scale"):
        assert np.array_equal(out[k], ref[k]), f"{what}: {k}"


def _guarded(nbytes, dev, fill=0xA5):
    g = torch.full((PAD + nbytes + PAD,), fill, dtype=torch.uint8, device=dev)
    return g, g[PAD:PAD + nbytes]


def _intact(g, nbytes, fill=0xA5):
    h = g.cpu().numpy()
    return bool((h[:PAD] == fill).all() and (h[PAD + nbytes:] == fill).all())


def _phases(dev, c, tolerance, max_rounds, vm=None, lm=None):
    """setup, every round in one call and finish with scratch, both tables and both outputs inside guards; the result in the
    shape of simplify_contours, and whether every guard is intact."""
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import contours as ct
    from insar_unet_ca_amd._lib import call, ptr
    v, ln = c["vertices"], c["lines"]
    V, R = int(v.shape[0]), len(ln["start"])
    vm, lm = vm or V, lm or R
    sb, tb = ct.contour_simplify_scratch_bytes(vm, lm)
    used = ct.LINE_DTYPE.itemsize * (1 + R)
    gs, scratch = _guarded(sb, dev)
    gi, tin = _guarded(used, dev)
    gt, table = _guarded(used, dev)
    gv, out_v = _guarded(8 * V, dev)
    gk, out_k = _guarded(4 * V, dev)
    host = np.zeros(1 + R, dtype=ct.LINE_DTYPE)
    for f in ("level", "closed", "start", "count", "leader"):
        host[f][1:] = ln[f]
    tin.copy_(torch.from_numpy(host.view(np.uint8)))
    s = _lib.stream_ptr()
    call("insar_contour_simplify_setup", ptr(v), V, ptr(tin), R, vm, lm, ptr(scratch), s)
    call("insar_contour_simplify_rounds", ptr(v), V, ptr(tin), R, ct.eps_q(tolerance) ** 2, 0, max_rounds + 1, max_rounds, vm, lm,
         ptr(scratch), s)
    call("insar_contour_simplify_finish", ptr(v), V, ptr(tin), R, max_rounds, vm, lm, ptr(scratch), ptr(table), ptr(out_v), ptr(out_k), s)
    torch.cuda.synchronize()
    raw = table.cpu().numpy().view(ct.LINE_DTYPE)
    head, rec = raw[0], raw[1:]
    kept = int(head["count"])
    assert int(head["level"]) == R and int(head["closed"]) == V
    lines = {"line": np.arange(R, dtype=np.int32)}
    for f in ct.LINE_FIELDS[1:]:
        lines[f] = rec[f].astype(np.bool_) if f == "closed" else rec[f].copy()
    lines["input_area2"] = np.asarray(ln["area2"]).astype(np.int64)
    lines["collapsed"] = rec["_pad"] != 0
    res = {"vertices": out_v.view(torch.int32).reshape(-1, 2)[:kept].clone(), "kept": out_k.view(torch.int32)[:kept].clone(),
           "lines": lines, "n_lines": R, "n_vertices": kept, "input_n_vertices": V, "rounds": int(head["leader"]),
           "converged": bool(head["start"]), "level_counts": c["level_counts"], "levels_q": c["levels_q"], "scale": c["scale"]}
    # nothing behind the kept vertices is written either
    tail_v, tail_k = out_v[8 * kept:].cpu().numpy(), out_k[4 * kept:].cpu().numpy()
    ok = (_intact(gs, sb) and _intact(gi, used) and _intact(gt, used) and _intact(gv, 8 * V) and _intact(gk, 4 * V)
          and bool((tail_v == 0xA5).all() and (tail_k == 0xA5).all()))
    return res, ok


def _on_device(c, dev):
    return dict(c, vertices=torch.from_numpy(np.ascontiguousarray(c["vertices"])).to(dev))


def _check(dev, c, ref_in, tolerance, max_rounds, what, ref=None):
    """`simplify_contours` and the guarded phase calls of the device dict c, bitwise against the oracle of its host twin."""
    import insar_unet_ca_amd as iu
    ref = ref or cr.simplify_contours_oracle(ref_in, tolerance, max_rounds)
    before = c["vertices"].clone()
    out = iu.simplify_contours(c, tolerance=tolerance, max_rounds=max_rounds)
    _compare(out, ref, what)
    ph, ok = _phases(dev, c, tolerance, max_rounds)
    assert ok, f"{what}: a guard was written"
    _compare(ph, ref, what + " (phases)")
    assert torch.equal(c["vertices"], before)                                      # the input is not written
    return ref, out


# ---- 1. rasters ---------------------------------------------------------------------------------------------------------------------
RASTERS = cr.raster_cases()


@pytest.mark.parametrize("name", list(RASTERS))
def test_rasters_against_the_oracle(dev, name):
    import insar_unet_ca_amd as iu
    m, levels = RASTERS[name]
    c = iu.contour_lines(torch.from_numpy(m).to(dev), levels, max_lines=4096, max_vertices=1 << 16)
    host = dict(c, vertices=c["vertices"].cpu().numpy())
    closed = c["lines"]["closed"]
    assert c["n_vertices"] > 128 and (~closed).any()
    if "NaN" in name:
        assert closed.any() and (~closed).sum() >= 4                               # open lines and rings mix
    for tol in TOLERANCES:
        ref, out = _check(dev, c, host, tol, ROUNDS, f"{name} tolerance {tol}")
        assert ref["converged"]
        print(f"{name} tol {tol}: {ref['input_n_vertices']} -> {ref['n_vertices']} vertices, {ref['rounds']} rounds, "
              f"{int(ref['lines']['collapsed'].sum())} of {int(closed.sum())} rings collapsed")


# ---- 2. hand-made polylines ------------------------------------------------------------------------------------------------------------
def _long_lines():
    """Open lines and rings of 5 000 vertices behind a short line of 77, so that no line starts on a block border; 300
    two-vertex open lines in a row; a ring of exactly 3 vertices."""
    parts = [(cr.zigzag(77, 3), False), (cr.zigzag(5003, 1), False), (cr.wobbly_ring(4999, 2), True)]
    parts += [([(50 + 7 * k, 100 * k), (60 + 5 * k, 100 * k + 90)], False) for k in range(300)]
    parts += [([(0, 0), (0, 5000), (3000, 100)], True), (cr.wobbly_ring(1501, 4, radius=90000), True), (cr.zigzag(640, 5), False)]
    return cr.make_contours(parts)


def test_hand_made_polylines(dev):
    host = _long_lines()
    start = host["lines"]["start"]
    assert host["n_vertices"] > 40 * 256 and (start[1:] % 256 != 0).all() and (host["lines"]["count"] == 2).sum() == 300
    c = _on_device(host, dev)
    for tol in TOLERANCES:
        ref, _ = _check(dev, c, host, tol, ROUNDS, f"hand-made tolerance {tol}")
        assert ref["converged"] and (ref["lines"]["count"][3:303] == 2).all() and ref["lines"]["count"][303] == 3
        print(f"hand-made tol {tol}: {ref['input_n_vertices']} -> {ref['n_vertices']} vertices, {ref['rounds']} rounds")


@pytest.mark.parametrize("tol", cr.SCAN_PASS_TOLERANCES)
def test_a_ring_longer_than_one_scan_pass(dev, tol):
    """69 677 positions, more than the 65 536 that one pass of the carry and prefix scans takes: a ring of 69 000 vertices
    lies across that boundary, with kept vertices on both sides and its wrap over it, between two open lines. At 0.25 pixel
    more than a tenth of the vertices survive, at 16 pixels fewer than a hundredth (tests/test_contour_simplify_host.py
    asserts both of the oracle)."""
    host = cr.scan_pass_lines()
    start, count = host["lines"]["start"], host["lines"]["count"]
    assert host["n_vertices"] > 65536 + 4096 and start[1] < 65536 - 4096 and start[1] + count[1] > 65536
    ref = cr.scan_pass_oracle(tol)
    assert ref["converged"] and min(cr.scan_pass_ring_kept(ref)) >= 2
    _check(dev, _on_device(host, dev), host, tol, ROUNDS, f"scan pass tolerance {tol}", ref=ref)
    print(f"scan pass tol {tol}: {ref['input_n_vertices']} -> {ref['n_vertices']} vertices, {ref['rounds']} rounds")


def test_ties_duplicates_and_rings_of_one_point(dev):
    """What `contour_lines` never produces and the function is total on: equal distances on either side of a chord, repeated
    coordinates (the smallest position wins), a ring of one point (one seed, collapsed), a line that returns to its head."""
    parts = [([(1000, 0), (1100, 500), (900, 1000), (1000, 1500)], False), ([(1000, 0), (900, 500), (1100, 1000), (1000, 1500)], False),
             ([(0, 0), (300, 100), (300, 100), (0, 200)], False), ([(5, 5)] * 4, True),
             ([(0, 0), (400, 300), (500, 300), (0, 0)], False), ([(0, 0), (0, 900), (0, 0), (0, 900), (700, 0), (700, 0)], True)]
    host = cr.make_contours(parts)
    c = _on_device(host, dev)
    for tol in (0, 50 / 256, 583 / 256, 584 / 256):
        ref, _ = _check(dev, c, host, tol, 8, f"ties tolerance {tol}")
    assert ref["lines"]["collapsed"].tolist() == [False, False, False, True, False, False]


# ---- 3. wide arithmetic ----------------------------------------------------------------------------------------------------------------
def test_wide_arithmetic(dev):
    parts = cr.wide_lines()
    host = cr.make_contours(parts)
    assert int(host["vertices"].max()) == 1 << 30 and int(host["vertices"].min()) == 0
    line = parts[0][0]
    (ay, ax), (by, bx) = line[0], line[-1]
    dy, dx = by - ay, bx - ax
    eps2 = cr.eps_of(1) ** 2
    assert (1 << 49) <= dy * dy + dx * dx and eps2 * (dy * dy + dx * dx) >= 1 << 64
    assert max((dx * (y - ay) - dy * (x - ax)) ** 2 for y, x in line[1:-1]) >= 1 << 64
    c = _on_device(host, dev)
    for tol in (0.5, 1, 2):
        ref, _ = _check(dev, c, host, tol, ROUNDS, f"wide tolerance {tol}")
        narrow = cr.simplify_contours_oracle(host, tol, ROUNDS, mul=cr.wrapped64)
        assert narrow["kept"].tolist() != ref["kept"].tolist()                     # a kernel that wraps cannot pass
        assert ref["lines"]["area2"][1] > 1 << 60 and not ref["lines"]["collapsed"].any()


# ---- 4. truncation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rounds", [1, 2, 8, 9, 17])
def test_truncation_on_the_shedding_arc(dev, max_rounds):
    """Fewer rounds than the arc needs: the oracle's result cut at that depth, not converged. 8 is one batch of rounds between
    two looks at the counter, 9 and 17 put the probe into a batch of its own."""
    arc = cr.shedding_arc()
    host = cr.make_contours([(arc, False)])
    c = _on_device(host, dev)
    ref, out = _check(dev, c, host, 0.25, max_rounds, f"arc max_rounds {max_rounds}")
    assert not out["converged"] and out["rounds"] == max_rounds and out["n_vertices"] == 2 + max_rounds
    if max_rounds == 17:
        full, _ = _check(dev, c, host, 0.25, 64, "arc in full")
        assert full["converged"] and full["rounds"] == len(arc) - 2


# ---- 5. scratch -----------------------------------------------------------------------------------------------------------------------
def test_reused_scratch_and_capacities(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import InsarError, ptr
    big, arc = _long_lines(), cr.make_contours([(cr.shedding_arc(), False)])
    m, levels = RASTERS["33x130 NaN hole, 3 levels"]
    mid = iu.contour_lines(torch.from_numpy(m).to(dev), levels)
    mid_host = dict(mid, vertices=mid["vertices"].cpu().numpy())
    sc = iu.ContourSimplifyScratch(big["n_vertices"] + 100, 512, dev)
    assert sc.key() == (big["n_vertices"] + 100, 512) and sc.device == dev
    sc.scratch.fill_(0xFF)
    sc.table.fill_(0xFF)
    for _ in range(2):                                                             # a larger input first, nothing cleared between
        for host, c, tol, mr in ((big, _on_device(big, dev), 1, 64), (mid_host, mid, 0.25, 64), (arc, _on_device(arc, dev), 0.25, 9),
                                 (mid_host, mid, 4, 64)):
            out = iu.simplify_contours(c, tolerance=tol, max_rounds=mr, scratch=sc)
            _compare(out, cr.simplify_contours_oracle(host, tol, mr), f"scratch reuse, {host['n_vertices']} vertices")
    V, R = big["n_vertices"], big["n_lines"]
    c = _on_device(big, dev)
    for vm, lm in ((V - 1, R), (V, R - 1)):
        with pytest.raises(InsarError, match=f"scratch for {vm} vertices in {lm} lines on {dev}: the input has {V} vertices in {R} lines"):
            iu.simplify_contours(c, tolerance=1, scratch=iu.ContourSimplifyScratch(vm, lm, dev))
    # the entry points refuse the same before a launch, and nothing is written
    sb, _ = iu.contours.contour_simplify_scratch_bytes(V - 1, R)
    g, scratch = _guarded(sb, dev)
    with pytest.raises(InsarError, match=f"n_vertices {V} outside 1..max_vertices = {V - 1}"):
        _lib.call("insar_contour_simplify_setup", ptr(c["vertices"]), V, ptr(scratch), R, V - 1, R, ptr(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((g.cpu().numpy() == 0xA5).all())
    # capacities exactly as needed and larger than needed give the same
    ref = cr.simplify_contours_oracle(big, 1, 64)
    ph, ok = _phases(dev, c, 1, 64, vm=V + 77, lm=R + 5)
    assert ok
    _compare(ph, ref, "larger capacities")


def test_launch_count(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import contours as ct
    arc = _on_device(cr.make_contours([(cr.shedding_arc(), False)]), dev)
    for max_rounds, issued in ((4, 5), (8, 9), (20, 21), (64, 40)):               # 38 rounds keep, the 39th finds nothing: 5 batches
        tape = []
        _lib._TAPE = tape
        try:
            iu.simplify_contours(arc, tolerance=0.25, max_rounds=max_rounds)
        finally:
            _lib._TAPE = None
        rounds = sum(a[6] for _, a, n in tape if n == "insar_contour_simplify_rounds")
        assert rounds == issued and [n for _, _, n in tape].count("insar_contour_simplify_setup") == 1
        assert ct.contour_simplify_launches(rounds) == 12 + 5 * rounds


# ---- 6. round trip through the rasteriser -------------------------------------------------------------------------------------------------
def test_round_trip_through_the_rasteriser_at_tolerance_zero(dev):
    """Plateaus (blocks of 4 x 4 pixels at a few heights, bordered low): the crossings of a straight plateau edge are collinear,
    so tolerance 0 drops vertices and must not move the line by a bit."""
    import insar_unet_ca_amd as iu
    rng = np.random.default_rng(17)
    m = bordered(np.kron(rng.integers(0, 4, size=(11, 15)), np.ones((4, 4), dtype=np.int64)).astype(np.int32) * 10, -1)
    H, W = m.shape
    levels = [5, 15, 25]
    c = iu.contour_lines(torch.from_numpy(m).to(dev), levels)
    assert c["lines"]["closed"].all()
    s = iu.simplify_contours(c, tolerance=0)
    _compare(s, cr.simplify_contours_oracle(dict(c, vertices=c["vertices"].cpu().numpy()), 0, 64), "plateaus")
    assert s["n_vertices"] < c["n_vertices"] and s["converged"] and not s["lines"]["collapsed"].any()
    assert s["lines"]["area2"].tobytes() == c["lines"]["area2"].tobytes()
    q, _ = quantise(m)
    for i, q_l in enumerate(c["levels_q"]):
        r = iu.rasterise_polygons(iu.pack_polygons(iu.contour_polygons(s, i)), H, W, device=dev)
        assert int(r["overlap_pixels"]) == 0, i
        assert (r["labels"].cpu().numpy() == (q >= q_l).astype(np.uint8)).all(), i
    print(f"plateaus: {c['n_vertices']} -> {s['n_vertices']} vertices")


# ---- 7. the scene pipeline -------------------------------------------------------------------------------------------------------------
def _equal(x, y):
    if isinstance(x, torch.Tensor):
        return torch.equal(x, y)
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_equal(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return x.tobytes() == y.tobytes()
    return x == y


def test_detect_with_simplified_contours(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd._lib import InsarError
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((64, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():                                         # split the class map about evenly (tests/test_outlines_gpu.py)
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    plain = pred.detect(scene, return_prob=True, min_area=2, contours=dict(levels=[0.5]))
    det = pred.detect(scene, return_prob=True, min_area=2, contours=dict(levels=[0.5], simplify=0.5))
    assert set(det) == set(plain) and all(_equal(plain[k], det[k]) for k in plain if k != "contours")
    assert _equal(plain["contours"], iu.contour_lines(det["prob"][1], [0.5])) and "collapsed" not in plain["contours"]["lines"]
    hand = iu.simplify_contours(plain["contours"], tolerance=0.5)
    assert _equal(det["contours"], hand) and hand["n_vertices"] < plain["contours"]["n_vertices"]
    _compare(hand, cr.simplify_contours_oracle(dict(plain["contours"], vertices=plain["contours"]["vertices"].cpu().numpy()), 0.5, 64),
             "detect")
    smooth = pred.detect(scene, min_area=2, contours=dict(levels=[0.5], smooth=1.5, simplify=0.5))
    unthinned = pred.detect(scene, min_area=2, contours=dict(levels=[0.5], smooth=1.5))
    assert _equal(smooth["contours"], iu.simplify_contours(unthinned["contours"], tolerance=0.5))
    assert len(iu.contours_to_geojson(smooth["contours"])["features"]) >= 1
    with pytest.raises(InsarError, match="contours: simplify=-1"):
        pred.detect(scene, contours=dict(levels=[0.5], simplify=-1))
    print(f"detect: {plain['contours']['n_vertices']} -> {hand['n_vertices']} vertices in {hand['n_lines']} lines")

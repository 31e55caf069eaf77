"""GPU: centre lines (insar_unet_ca_amd/skeletons.py on csrc/skeleton.hip) against the numpy oracle of tests/skeleton_ref.py
(pinned by its own invariants in tests/test_skeleton_host.py).

Every device result is an integer and compared bitwise: the kinds map, iterations, converged and every field of the records.
The float table is compared with the oracle's formulas on the same integers at rtol 1e-12 (both sides are float64 numpy on
equal integers). A launch holds 8 iterations and a tile is 96 rows x 384 pixels with 64-pixel words, so the maps cross word
edges (70, 131, 200), the tiles' row edge (130 rows) and column edge (420 columns), and the 70 x 70 square needs five launches."""
import numpy as np
import pytest
import torch

from tests import skeleton_ref as ref

pytestmark = pytest.mark.gpu
INT_FIELDS = ref.STAT_FIELDS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_ORACLE = {}


def _oracle(name, labels, max_iterations, widths=True):
    key = (name, max_iterations, widths)
    if key not in _ORACLE:
        _ORACLE[key] = ref.skeleton_oracle(labels, max_iterations, widths)
    return _ORACLE[key]


def _compare(out, want, what, widths=True):
    sk = out["skeleton"]
    assert sk.dtype == torch.uint8 and tuple(sk.shape) == want["skeleton"].shape
    got = sk.cpu().numpy()
    print(f"{what}: iterations {out['iterations']} (oracle {want['iterations']}), converged {out['converged']}, "
          f"{int((got > 0).sum())} skeleton pixels (oracle {int((want['skeleton'] > 0).sum())})")
    assert torch.equal(sk.cpu(), torch.from_numpy(want["skeleton"])), f"{what}: skeleton differs at {np.argwhere(got != want['skeleton'])[:8].tolist()}"
    assert out["iterations"] == want["iterations"] and out["converged"] == want["converged"], what
    st, ws = out["stats"], want["stats"]
    assert np.array_equal(st["label"], ws["label"]), what
    for f in INT_FIELDS:
        assert st[f].dtype == ws[f].dtype, (what, f, st[f].dtype)
        assert np.array_equal(st[f], ws[f]), f"{what}: {f} differs at labels {1 + np.flatnonzero(st[f] != ws[f])[:8]}"
    tab = ref.table_oracle(ws, widths)
    for f, v in tab.items():
        np.testing.assert_allclose(out["table"][f], v, rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{what}: {f}")
    assert np.array_equal(out["table"]["n_end"], ws["n_end"]) and np.array_equal(out["table"]["n_junction"], ws["n_junction"])


def _check(dev, name, labels, max_iterations=32, widths=True, **kw):
    import insar_unet_ca_amd as iu
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    t = torch.from_numpy(labels).to(dev)
    out = iu.thin_regions(t, max_iterations=max_iterations, widths=widths, **kw)
    _compare(out, _oracle(name, labels, max_iterations, widths), f"{name} max_iterations {max_iterations}", widths)
    assert (t.cpu().numpy() == labels).all()                                  # the input is not written
    return out


def abutting():
    m = np.zeros((20, 30), dtype=np.int32)
    m[3:17, 3:14] = 1
    m[3:17, 14:27] = 2                                                       # a shared straight border
    return m


def corner_touch():
    m = np.zeros((24, 24), dtype=np.int32)
    m[2:12, 2:12] = 1
    m[12:22, 12:22] = 2                                                      # diagonal neighbours of another label only
    return m


def wide_bar():
    m = np.zeros((21, 800), dtype=np.int32)                                  # three tiles of 384 pixels side by side
    m[6:15, 3:797] = 1
    return m


OTHER = {"abutting": abutting(), "corner touch": corner_touch(), "zeros": np.zeros((17, 70), dtype=np.int32),
         "one region": np.ones((40, 70), dtype=np.int32), "wide bar": wide_bar(),
         "negative background": np.where(abutting() == 0, -3, abutting()).astype(np.int32)}


@pytest.mark.parametrize("name", list(ref.HAND))
def test_hand_cases(dev, name):
    out = _check(dev, name, ref.HAND[name], max_iterations=40)
    assert out["iterations"] == ref.HAND_ITERATIONS[name] and out["converged"]


@pytest.mark.parametrize("name", list(OTHER))
def test_other_hand_made_maps(dev, name):
    _check(dev, name, OTHER[name])


BLOBS = {"1x1": (1, 1), "1x70": (1, 70), "70x1": (70, 1), "67x131": (67, 131), "130x200": (130, 200), "40x420": (40, 420)}


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", list(BLOBS))
def test_blobs_across_tile_edges(dev, case, connectivity):
    H, W = BLOBS[case]
    fg = ref.blobs(H + 2, W + 2, 7)[1:-1, 1:-1] if min(H, W) > 2 else np.ones((H, W), dtype=bool)   # regions reach the image border
    if min(H, W) == 1 and max(H, W) > 1:
        fg = ref.speckle(H, W, 9, 0.7)
    _check(dev, f"{case} conn {connectivity}", ref.label_scipy(fg, connectivity))


@pytest.mark.parametrize("max_iterations", [1, 2, 3, 9])
def test_bounds_cut_short(dev, max_iterations):
    """9 = one more than a launch holds: the second launch runs exactly one iteration."""
    from insar_unet_ca_amd import skeletons as sk
    assert sk.ITERATIONS_PER_LAUNCH == 8
    out = _check(dev, "square 70x70", ref.HAND["square 70x70"], max_iterations=max_iterations)
    assert out["iterations"] == max_iterations and not out["converged"]


def test_label_above_max_regions_and_guard(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import skeletons as sk
    from insar_unet_ca_amd._lib import InsarError, call, ptr
    labels = ref.label_scipy(ref.blobs(67, 131, 7), 8)
    n = int(labels.max())
    assert n > 4
    t = torch.from_numpy(labels).to(dev)
    _compare(iu.thin_regions(t, max_regions=n), _oracle("67x131 guard", labels, 32), "capacity exactly as needed")
    with pytest.raises(InsarError, match=rf"label {n} exceeds max_regions={n - 1}"):
        iu.thin_regions(t, max_regions=n - 1)
    # the phase calls with scratch and table inside a guard pattern, one record too few
    pad, mi, cap = 4096, 32, n - 1
    sb, tb = sk.scratch_bytes(67, 131, mi, cap)

    def guarded(nbytes):
        g = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
        return g, g[pad:pad + nbytes]

    gs, scratch = guarded(sb)
    gt, table = guarded(tb)
    gk, skel = guarded(67 * 131)
    s = _lib.stream_ptr()
    call("insar_skeleton_planes", ptr(t), 67, 131, mi, cap, ptr(scratch), ptr(table), s)
    for step in range(sk.launches(67, 131, mi, False) - 2):
        call("insar_skeleton_step", 67, 131, mi, step, ptr(scratch), s)
    call("insar_skeleton_stats", ptr(t), None, 67, 131, mi, cap, ptr(scratch), ptr(table), ptr(skel), s)
    torch.cuda.synchronize()
    for g, nbytes in ((gs, sb), (gt, tb), (gk, 67 * 131)):
        h = g.cpu().numpy()
        assert (h[:pad] == 0xA5).all() and (h[pad + nbytes:] == 0xA5).all()
    want = _oracle("67x131 guard", labels, 32)
    rec = table.cpu().numpy().view(sk.STAT_DTYPE)
    assert (int(rec["n_junction"][0]), int(rec["n_orth"][0])) == (n, 1)       # the largest label and the overflow flag
    assert int(rec["n"][0]) == want["iterations"] and int(rec["n_end"][0]) == 1
    for f in ("n", "n_end", "n_junction", "n_orth", "n_diag", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy"):
        assert np.array_equal(rec[f][1:], want["stats"][f][:cap]), f
    assert np.array_equal(skel.cpu().numpy().reshape(67, 131), want["skeleton"])   # label n is thinned and classified all the same


def test_determinism_on_a_reused_scratch(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import skeletons as sk
    labels = ref.label_scipy(ref.blobs(130, 200, 7), 4)
    t = torch.from_numpy(labels).to(dev)
    sc = sk.SkeletonScratch(130, 200, dev, 32, 512)
    raw = []
    for fill in (0xFF, 0x5A):
        sc.scratch.fill_(fill)
        sc.table.fill_(fill)
        sc.distance_scratch().scratch.fill_(fill)
        out = iu.thin_regions(t, max_regions=512, scratch=sc)
        n = int(labels.max())
        raw.append((sc.host.numpy()[:80 * (1 + n)].tobytes(), out["skeleton"].cpu().numpy().tobytes()))
        _compare(out, _oracle("130x200 conn 4 det", labels, 32), "reused scratch")
    assert raw[0] == raw[1]


def test_widths_off_and_launch_count(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd import skeletons as sk
    labels = ref.label_scipy(ref.blobs(67, 131, 7), 8)
    t = torch.from_numpy(labels).to(dev)
    per_call = {"insar_dist_transform": 2, "insar_skeleton_planes": 1, "insar_skeleton_step": 1, "insar_skeleton_stats": 1}
    for widths, mi in ((False, 32), (True, 32), (False, 9), (True, 1)):
        tape = []
        _lib._TAPE = tape
        try:
            out = iu.thin_regions(t, max_iterations=mi, widths=widths)
        finally:
            _lib._TAPE = None
        made = sum(per_call.get(name, 0) for _, _, name in tape)              # the host-only size queries launch nothing
        assert made == sk.launches(67, 131, mi, widths) == 2 + -(-mi // 8) + 2 * widths, (widths, mi, [n for _, _, n in tape])
        _compare(out, _oracle("67x131 conn 8 w", labels, mi, widths), f"widths {widths} max_iterations {mi}", widths)
        if not widths:
            assert not out["stats"]["sum_d2"].any() and not out["stats"]["max_d2"].any() and not out["stats"]["n_far"].any()
            assert np.isnan(out["table"]["mean_width"]).all()


def test_detect_with_skeletons(dev):
    import insar_unet_ca_amd as iu
    torch.manual_seed(3)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(4).standard_normal((64, 96)).astype(np.float32)
    pred = iu.ScenePredictor(net, tile=32, overlap=8, batch=4, num_classes=2)
    # an untrained net puts every pixel in one class: move the output bias by the median log-odds, so that the class map
    # splits about evenly and falls into many regions
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():
        net.outc.bias[1] += torch.log(p[0] / p[1]).median()
    new = ("length", "mean_width", "max_width", "orientation", "n_end", "n_junction")
    for connectivity in (8, 4):
        kw = dict(connectivity=connectivity, min_area=2)
        plain = pred.detect(scene, **kw)
        det = pred.detect(scene, skeletons=True, max_iterations=16, **kw)
        assert set(plain) == {"mask", "conf", "labels", "regions", "count", "mask_clean"}
        assert set(det) == set(plain) | {"skeleton", "skeleton_converged"}
        assert set(det["regions"]) == set(plain["regions"]) | set(new)
        for k in ("mask", "conf", "labels", "mask_clean"):
            assert torch.equal(plain[k], det[k]), k
        for k, v in plain["regions"].items():
            assert v.tobytes() == det["regions"][k].tobytes(), k
        direct = iu.thin_regions(det["labels"], max_iterations=16)
        assert torch.equal(det["skeleton"], direct["skeleton"]) and det["skeleton_converged"] == direct["converged"]
        rows = det["regions"]["id"].astype(np.int64) - 1
        for f in new:
            assert len(det["regions"][f]) == det["count"]
            assert np.array_equal(det["regions"][f], direct["table"][f][rows], equal_nan=True), f
        _compare(direct, ref.skeleton_oracle(det["labels"].cpu().numpy(), 16), f"detect conn {connectivity}")
    one = iu.detect_scene(net, scene, skeletons=True, max_iterations=16, tile=32, overlap=8, batch=4, num_classes=2, connectivity=4,
                          min_area=2)
    assert torch.equal(one["skeleton"], det["skeleton"])
    print(f"detect: {det['count']} regions, {int((det['skeleton'] > 0).sum())} skeleton pixels")
    assert det["count"] > 4

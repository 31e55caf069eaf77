"""GPU: the overlap table of two label maps (insar_unet_ca_amd/score.py on csrc/overlap.hip) and everything built on it,
against the oracles of tests/score_ref.py (pinned in tests/test_score_host.py).

Every integer is compared exactly (ids, counts, areas, matches, tp / fp / fn, the confusion matrix); IoU and the scores to rtol
1e-12 (the same integers divided in float64 on both sides). The scene is 200 x 264 unless a case says otherwise: 52 800 pixels
= 13 200 quads of four = 51.6 work-groups of 256 threads and 206.25 waves, ragged against every unit the count kernel has."""
import numpy as np
import pytest
import torch

from tests.regions_ref import regions_oracle
from tests.score_ref import assert_match_equal, dense_from_labels, match_oracle, overlaps_oracle

pytestmark = pytest.mark.gpu
H0, W0 = 200, 264


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def striped_random(H, W, fill, seed):
    """Random foreground at `fill`, three classes in adjacent 37-pixel stripes: class borders cut the blobs."""
    rng = np.random.default_rng(seed)
    cls = (1 + (np.arange(W) // 37) % 3).astype(np.uint8)
    return (rng.random((H, W)) < fill).astype(np.uint8) * cls[None, :]


def blobs(H, W, seed, share=0.35):
    """8 x 8 blocks, `share` of them foreground, three classes in 37-pixel stripes: compact regions of 64+ pixels."""
    rng = np.random.default_rng(seed)
    coarse = (rng.random(((H + 7) // 8, (W + 7) // 8)) < share).astype(np.uint8)
    cls = (1 + (np.arange(W) // 37) % 3).astype(np.uint8)
    return np.kron(coarse, np.ones((8, 8), dtype=np.uint8))[:H, :W] * cls[None, :]


def void_map(H, W, seed, share=0.1):
    """uint8: 255 on `share` of the pixels, other values (0..3, and 254) elsewhere: only 255 may drop a pixel."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 4, size=(H, W)).astype(np.uint8)
    v[rng.random((H, W)) < 0.02] = 254
    v[rng.random((H, W)) < share] = 255
    return v


def _label(dev, mask, **kw):
    import insar_unet_ca_amd as iu
    return iu.label_regions(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(dev), **kw)


def _check_table(dev, pred_labels, gt_labels, void=None, what="", **kw):
    """region_overlaps on device label maps against the oracle on their host copies; the inputs must not be written."""
    import insar_unet_ca_amd as iu
    p_host, g_host = pred_labels.cpu().numpy(), gt_labels.cpu().numpy()
    v_dev = None if void is None else torch.from_numpy(void).to(dev)
    got = iu.region_overlaps(pred_labels, gt_labels, void=v_dev, **kw)
    want = overlaps_oracle(p_host, g_host, void, 255)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    for name, a, b in zip(("pred", "gt", "count"), got, want):
        assert a.shape == b.shape, f"{what}: {len(a)} keys, oracle {len(b)}"
        assert (a == b).all(), f"{what}: {name}: {(a != b).sum()} of {len(a)} differ"
    live = np.ones(p_host.shape, dtype=bool) if void is None else void != 255
    assert int(got[2].sum()) == int((live & ((p_host != 0) | (g_host != 0))).sum())
    assert (pred_labels.cpu().numpy() == p_host).all() and (gt_labels.cpu().numpy() == g_host).all()
    if void is not None:
        assert (v_dev.cpu().numpy() == void).all()
    print(f"{what}: {len(got[0])} keys, largest count {int(got[2].max(initial=0))}")
    return got


# ---- random blobs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_void", [False, True])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("fill, gt_kind", [(0.3, "shifted"), (0.6, "reseeded")])
def test_random_blobs(dev, fill, gt_kind, connectivity, with_void):
    m = striped_random(H0, W0, fill, seed=int(fill * 10))
    g = np.roll(m, (2, 3), axis=(0, 1)) if gt_kind == "shifted" else striped_random(H0, W0, fill, seed=100 + int(fill * 10))
    pred, gt = _label(dev, m, connectivity=connectivity), _label(dev, g, connectivity=connectivity)
    void = void_map(H0, W0, seed=5) if with_void else None
    got = _check_table(dev, pred["labels"], gt["labels"], void, what=f"random {fill}/{gt_kind}/{connectivity}/void={with_void}")
    assert len(got[0]) > 200
    # every area after voiding follows from the table
    live = np.ones((H0, W0), dtype=bool) if void is None else void != 255
    area_p = np.bincount(got[0], weights=got[2], minlength=pred["count"] + 1).astype(np.int64)
    area_g = np.bincount(got[1], weights=got[2], minlength=gt["count"] + 1).astype(np.int64)
    assert (area_p[1:] == np.bincount(pred["labels"].cpu().numpy()[live], minlength=pred["count"] + 1)[1:]).all()
    assert (area_g[1:] == np.bincount(gt["labels"].cpu().numpy()[live], minlength=gt["count"] + 1)[1:]).all()


# ---- run aggregation ------------------------------------------------------------------------------------------------------
def test_one_region_against_one_region(dev):
    """Every lane of every wave carries the same key: a single record (1, 1) with the whole scene in it."""
    ones = torch.ones(H0, W0, dtype=torch.int32, device=dev)
    got = _check_table(dev, ones, ones.clone(), what="1 x 1")
    assert [v.tolist() for v in got] == [[1], [1], [52800]]
    void = np.zeros((H0, W0), dtype=np.uint8)
    void[:, 100:137] = 255
    got = _check_table(dev, ones, ones.clone(), void, what="1 x 1, void stripe")
    assert [v.tolist() for v in got] == [[1], [1], [52800 - 200 * 37]]
    void[:] = 255
    got = _check_table(dev, ones, ones.clone(), void, what="1 x 1, all void")
    assert [len(v) for v in got] == [0, 0, 0]
    zeros = torch.zeros(H0, W0, dtype=torch.int32, device=dev)
    assert [len(v) for v in _check_table(dev, zeros, zeros.clone(), what="0 x 0")] == [0, 0, 0]
    got = _check_table(dev, ones, zeros, what="1 x 0")
    assert [v.tolist() for v in got] == [[1], [0], [52800]]


def test_checkerboard_against_column_stripes(dev):
    """A 4-connected checkerboard is 26 400 one-pixel regions: every lane is a run of its own. gt: eight 37-pixel stripes."""
    yy, xx = np.indices((H0, W0))
    pred = _label(dev, ((yy + xx) % 2 == 0).astype(np.uint8), connectivity=4, max_regions=32768)
    gt = _label(dev, np.broadcast_to((1 + (np.arange(W0) // 37) % 3).astype(np.uint8), (H0, W0)), connectivity=4)
    assert pred["count"] == 26400 and gt["count"] == 8
    got = _check_table(dev, pred["labels"], gt["labels"], what="checkerboard", max_pairs=32768)
    assert len(got[0]) == 26400 + 8 and (got[2][got[0] > 0] == 1).all()
    assert int(got[2][got[0] == 0].sum()) == 26400


# ---- unaligned ------------------------------------------------------------------------------------------------------------
def test_scene_off_the_vector_width(dev):
    """199 x 263: H * W % 4 == 1, the guarded scalar path and a last quad that is three quarters empty."""
    m = striped_random(199, 263, 0.55, seed=263)
    pred, gt = _label(dev, m, connectivity=8), _label(dev, np.roll(m, (1, 2), axis=(0, 1)), connectivity=8)
    _check_table(dev, pred["labels"], gt["labels"], void_map(199, 263, seed=6), what="199x263")
    _check_table(dev, pred["labels"], gt["labels"], what="199x263, no void")


@pytest.mark.parametrize("with_void", [False, True])
def test_small_scene_off_the_vector_width(dev, with_void):
    """33 x 65 = 2 145 pixels, H * W % 4 == 1: 537 quads, every one through the guarded scalar loads of the count kernel, the
    last with one pixel in it; 2.1 work-groups, 8.4 waves."""
    H, W = 33, 65
    m = striped_random(H, W, 0.55, seed=65)
    pred, gt = _label(dev, m, connectivity=8), _label(dev, np.roll(m, (1, 2), axis=(0, 1)), connectivity=8)
    got = _check_table(dev, pred["labels"], gt["labels"], void_map(H, W, seed=11) if with_void else None,
                       what=f"33x65, void={with_void}")
    assert len(got[0]) > 20


def test_views_off_a_16_byte_boundary(dev):
    import insar_unet_ca_amd as iu
    m = striped_random(H0, W0, 0.55, seed=71)
    pred, gt = _label(dev, m, connectivity=8), _label(dev, np.roll(m, (1, 2), axis=(0, 1)), connectivity=8)
    void = torch.from_numpy(void_map(H0, W0, seed=7)).to(dev)
    base = iu.region_overlaps(pred["labels"], gt["labels"], void=void)

    def shifted(t, by):
        buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[by:by + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == by * t.element_size()
        return v

    for dp, dg, dv in ((1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 0, 1), (3, 2, 2)):
        got = iu.region_overlaps(shifted(pred["labels"], dp), shifted(gt["labels"], dg), void=shifted(void, dv))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base)), (dp, dg, dv)
    _check_table(dev, shifted(pred["labels"], 1), shifted(gt["labels"], 3), void.cpu().numpy(), what="offset views")


# ---- probing ----------------------------------------------------------------------------------------------------------------
def test_a_nearly_full_table_stays_exact_and_a_full_one_raises(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd._lib import InsarError
    m = np.zeros((H0, W0), dtype=np.uint8)
    for r in range(5):
        for c in range(5):
            m[10 + 38 * r:30 + 38 * r, 12 + 50 * c:40 + 50 * c] = 1
    pred, gt = _label(dev, m), _label(dev, np.roll(m, (3, 5), axis=(0, 1)))
    n = len(overlaps_oracle(pred["labels"].cpu().numpy(), gt["labels"].cpu().numpy())[0])
    assert n == 75                                                   # 25 pairs, 25 rows (p, 0), 25 columns (0, g)
    for max_pairs in (n, n + 2, 128):                                # capacity 256: load factor 0.29; n itself is allowed
        _check_table(dev, pred["labels"], gt["labels"], what=f"max_pairs={max_pairs}", max_pairs=max_pairs)
    with pytest.raises(InsarError, match=rf"{n} overlapping pairs exceed max_pairs={n - 1}"):
        iu.region_overlaps(pred["labels"], gt["labels"], max_pairs=n - 1)
    # 16 slots for 75 keys: the probe loop gives up after 16 steps, flags the overflow and returns
    with pytest.raises(InsarError, match="max_pairs=8"):
        iu.region_overlaps(pred["labels"], gt["labels"], max_pairs=8)
    with pytest.raises(InsarError, match="max_pairs=1"):
        iu.region_overlaps(pred["labels"], gt["labels"], max_pairs=1)
    _check_table(dev, pred["labels"], gt["labels"], what="after the overflow")          # nothing is left behind


def test_output_stays_inside_its_buffer(dev):
    """max_pairs below the key count through the phase calls: the header carries the true count, the bytes either side of the
    output and of the table stay untouched."""
    from insar_unet_ca_amd import score
    m = striped_random(H0, W0, 0.5, seed=21)
    pred, gt = _label(dev, m, connectivity=4), _label(dev, np.roll(m, (2, 3), axis=(0, 1)), connectivity=4)
    want = overlaps_oracle(pred["labels"].cpu().numpy(), gt["labels"].cpu().numpy())
    n = len(want[0])
    cap_pairs = 2048
    assert n > 2 * cap_pairs                                          # more keys than records, but fewer than the 4096 slots...
    tb, ob = score.scratch_bytes(cap_pairs)
    pad = 4096
    gt_buf, go_buf = (torch.full((pad + b + pad,), 0xA5, dtype=torch.uint8, device=dev) for b in (tb, ob))
    table, out = gt_buf[pad:pad + tb], go_buf[pad:pad + ob]
    score._launch(pred["labels"], gt["labels"], None, 255, cap_pairs, table, out)
    torch.cuda.synchronize()
    for buf, b in ((gt_buf, tb), (go_buf, ob)):
        g = buf.cpu().numpy()
        assert (g[:pad] == 0xA5).all() and (g[pad + b:] == 0xA5).all()
    raw = go_buf.cpu().numpy()[pad:pad + ob]
    n_keys, overflow = raw[:16].view("<i8")
    assert n_keys == 4096 and overflow == 1                           # ...so the table fills up: every slot taken, the rest dropped
    rec = raw[16:].view(score.OVERLAP_DTYPE)
    keys = set(zip(want[0].tolist(), want[1].tolist()))
    assert len(rec) == cap_pairs and all((int(r["pred"]), int(r["gt"])) in keys for r in rec)
    assert len({(int(r["pred"]), int(r["gt"])) for r in rec}) == cap_pairs


# ---- reproducibility ------------------------------------------------------------------------------------------------------
def test_twenty_calls_are_byte_identical(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import score
    m = striped_random(H0, W0, 0.6, seed=51)
    pred, gt = _label(dev, m, connectivity=8), _label(dev, striped_random(H0, W0, 0.6, seed=52), connectivity=8)
    void = torch.from_numpy(void_map(H0, W0, seed=8)).to(dev)
    before = [t.clone() for t in (pred["labels"], gt["labels"], void)]
    sc = score.OverlapScratch(dev)
    sc.table.fill_(0xFF), sc.out.fill_(0xFF)                          # nothing relies on cleared buffers
    first = iu.region_overlaps(pred["labels"], gt["labels"], void=void, scratch=sc)
    for k in range(19):
        again = iu.region_overlaps(pred["labels"], gt["labels"], void=void, scratch=sc if k % 2 else None)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), k
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = iu.region_overlaps(pred["labels"], gt["labels"], void=void, scratch=sc)
    side.synchronize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, other))
    for t, b in zip((pred["labels"], gt["labels"], void), before):
        assert torch.equal(t, b)
    want = overlaps_oracle(before[0].cpu().numpy(), before[1].cpu().numpy(), before[2].cpu().numpy(), 255)
    assert all((a == b).all() for a, b in zip(first, want))


# ---- matching on device inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iou_threshold", [0.5, 0.3])
@pytest.mark.parametrize("with_void", [False, True])
def test_match_regions_equals_the_oracle(dev, with_void, iou_threshold):
    import insar_unet_ca_amd as iu
    m = blobs(H0, W0, seed=81)
    g = np.roll(m, (1, 2), axis=(0, 1))
    g[:, 150:] = np.roll(blobs(H0, W0, seed=82), (0, 0))[:, 150:]     # the right part: unrelated truth
    conf = np.random.default_rng(83).random((H0, W0)).astype(np.float32)
    pred = iu.label_regions(torch.from_numpy(m).to(dev), torch.from_numpy(conf).to(dev), connectivity=8, min_area=4)
    gt = _label(dev, g, connectivity=8)
    void = void_map(H0, W0, seed=9) if with_void else None
    got = iu.match_regions(pred, gt, void=None if void is None else torch.from_numpy(void).to(dev), iou_threshold=iou_threshold,
                           num_classes=4)
    N = dense_from_labels(pred["labels"].cpu().numpy(), gt["labels"].cpu().numpy(), pred["count"], gt["count"], void, 255)
    n_valid = H0 * W0 if void is None else int((void != 255).sum())
    ref = match_oracle(N, pred["regions"]["cls"], gt["regions"]["cls"], iou_threshold=iou_threshold, num_classes=4,
                       pred_conf=pred["regions"]["mean_conf"], n_valid=n_valid)
    assert_match_equal(got, ref, f"void={with_void} thr={iou_threshold}")
    o = got["overall"]
    print(f"void={with_void} thr={iou_threshold}: {pred['count']} preds, {gt['count']} gts, tp {o['tp']} fp {o['fp']} fn {o['fn']} "
          f"pq {o['pq']:.4f} ap {got['ap_mean']:.4f}")
    assert o["tp"] > 10 and o["fp"] > 0 and o["fn"] > 0
    assert got["confusion"].sum() == n_valid
    # the confusion matrix is the one of the two cleaned class maps
    pm, gm = pred["mask"].cpu().numpy(), gt["mask"].cpu().numpy()
    live = np.ones((H0, W0), dtype=bool) if void is None else void != 255
    want = np.zeros((4, 4), dtype=np.int64)
    np.add.at(want, (gm[live], pm[live]), 1)
    assert np.array_equal(got["confusion"], want)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_evaluate_is_detect_plus_the_oracle_score(dev):
    import insar_unet_ca_amd as iu
    T, o, H, W = 64, 8, 128, 192
    torch.manual_seed(5)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True).to(dev).eval()
    scene = np.random.default_rng(91).standard_normal((H, W)).astype(np.float32)
    gt_mask = blobs(H, W, seed=92)
    gt_mask[gt_mask > 1] = 1
    gt_mask[:6], gt_mask[-6:], gt_mask[:, :6], gt_mask[:, -6:] = 255, 255, 255, 255
    pred = iu.ScenePredictor(net, tile=T, overlap=o, batch=4, num_classes=2)
    before = pred.predict(scene)
    # an untrained net's winning probabilities lie in a narrow band: threshold at their median, so that the confidence
    # filter cuts the class map into many regions
    kw = dict(connectivity=8, min_area=3, min_conf=float(before["conf"].median()))
    det = pred.detect(scene, **kw)
    ev = pred.evaluate(scene, gt_mask, iou_threshold=0.3, gt_min_area=2, **kw)
    for k in ("mask", "conf", "labels", "mask_clean"):
        assert torch.equal(det[k], ev[k]) and ev[k].dtype == det[k].dtype, k
    assert torch.equal(before["mask"], ev["mask"]) and torch.equal(before["conf"], ev["conf"])
    assert ev["count"] == det["count"] and all(ev["regions"][k].tobytes() == v.tobytes() for k, v in det["regions"].items())
    gt_cls = np.where(gt_mask == 255, 0, gt_mask).astype(np.uint8)
    truth = regions_oracle(gt_cls, connectivity=8, min_area=2)
    assert ev["gt_count"] == truth["count"] and (ev["gt_labels"].cpu().numpy() == truth["labels"]).all()
    N = dense_from_labels(ev["labels"].cpu().numpy(), truth["labels"], ev["count"], truth["count"], gt_mask, 255)
    ref = match_oracle(N, ev["regions"]["cls"], truth["regions"]["cls"], iou_threshold=0.3, num_classes=2,
                       pred_conf=ev["regions"]["mean_conf"], n_valid=int((gt_mask != 255).sum()))
    assert_match_equal(ev["score"], ref, "evaluate")
    s = ev["score"]["overall"]
    print(f"evaluate: {ev['count']} preds, {ev['gt_count']} gts, tp {s['tp']} fp {s['fp']} fn {s['fn']}")
    assert ev["count"] > 1 and ev["gt_count"] > 1
    # the tensor form of gt_mask and the one-shot function give the same; scratch objects are cached per scene size
    ev2 = pred.evaluate(scene, torch.from_numpy(gt_mask), iou_threshold=0.3, gt_min_area=2, **kw)
    one = iu.evaluate_scene(net, scene, gt_mask, tile=T, overlap=o, batch=4, num_classes=2, iou_threshold=0.3, gt_min_area=2, **kw)
    for other in (ev2, one):
        assert_match_equal(other["score"], ref, "evaluate again")
        assert torch.equal(other["labels"], ev["labels"]) and torch.equal(other["gt_labels"], ev["gt_labels"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other["score"]["overlaps"], ev["score"]["overlaps"]))
    assert len(pred._cached(iu.regions.RegionScratch)) == 1 and len(pred._cached(iu.score.OverlapScratch)) == 1
    acc = iu.DetectionScore(2, 0.3)
    acc.update(ev["score"])
    acc.update(ev2["score"])
    assert acc.compute()["overall"]["tp"] == 2 * s["tp"]
    pred.release()
    assert not pred._cached(iu.regions.RegionScratch) and not pred._cached(iu.score.OverlapScratch)

"""CPU-only: the host side of whole-scene inference (insar_unet_ca_amd/infer.py): the tiling rule, the blend window, the
float64 restatement of the stitch that tests/test_scene_gpu.py uses as its oracle (pinned here against a brute-force
per-pixel loop), and the argument checks of the three scene entry points, which run before anything touches a device."""
import numpy as np
import pytest

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd._lib import InsarError
from insar_unet_ca_amd.infer import plan_tiles, window_1d


# ---- the oracle of the GPU tests: a float64 restatement of blend + finalize ------------------------------------------
def stitch_oracle(logits, origins, H, W, T, o):
    """logits [N, K, T, T] (any float dtype) -> prob float64 [K, H, W], wsum float64 [H, W]."""
    lg = np.asarray(logits, dtype=np.float64)
    K = lg.shape[1]
    i = np.arange(T)
    r = np.minimum(np.minimum(i + 1, T - i), o + 1) / (o + 1.0)
    w2 = r[:, None] * r[None, :]
    acc = np.zeros((K, H, W))
    wsum = np.zeros((H, W))
    for t, (y, x) in enumerate(np.asarray(origins)):
        e = np.exp(lg[t] - lg[t].max(axis=0, keepdims=True))
        acc[:, y:y + T, x:x + T] += w2 * (e / e.sum(axis=0, keepdims=True))
        wsum[y:y + T, x:x + T] += w2
    return acc / wsum, wsum


# ---- plan_tiles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args, rows, cols", [
    ((512, 512, 256, 0), [0, 256], [0, 256]),
    ((600, 700, 256, 32), [0, 224, 344], [0, 224, 444]),
    ((714, 600, 256, 32), [0, 224, 448, 458], [0, 224, 344]),
    ((768, 768, 256, 128), [0, 128, 256, 384, 512], [0, 128, 256, 384, 512]),
    ((256, 256, 256, 32), [0], [0]),
])
def test_plan_tiles_hand_worked(args, rows, cols):
    H, W, T, o = args
    t = plan_tiles(*args)
    assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 2
    assert t.shape[0] == len(rows) * len(cols)
    # the row-major product of the two axes, exactly
    assert t.tolist() == [[y, x] for y in rows for x in cols]
    assert len(set(map(tuple, t.tolist()))) == t.shape[0]
    # every tile inside, every pixel covered
    assert (t >= 0).all() and (t[:, 0] + T <= H).all() and (t[:, 1] + T <= W).all()
    cover = np.zeros((H, W), dtype=np.int32)
    for y, x in t:
        cover[y:y + T, x:x + T] += 1
    assert cover.min() >= 1


def test_plan_tiles_counts():
    assert len(plan_tiles(512, 512, 256, 0)) == 4 and len(plan_tiles(600, 700, 256, 32)) == 9
    assert len(plan_tiles(714, 600, 256, 32)) == 12 and len(plan_tiles(768, 768, 256, 128)) == 25
    assert len(plan_tiles(256, 256, 256, 32)) == 1


def test_nine_deep_pixels_exist():
    """The edge tile lies over two regular ones: H = 714, T = 256, o = 128 reaches 3 x 3 covering tiles."""
    t = plan_tiles(714, 600, 256, 128)
    cover = np.zeros((714, 600), dtype=np.int32)
    for y, x in t:
        cover[y:y + 256, x:x + 256] += 1
    assert cover.max() == 9


@pytest.mark.parametrize("args", [
    (600, 700, 256, 129),      # overlap > tile // 2
    (600, 700, 256, -1),
    (255, 700, 256, 32),       # scene smaller than the tile
    (600, 200, 256, 32),
    (600, 700, 250, 32),       # tile not a multiple of 16
    (600, 700, 0, 0),
])
def test_plan_tiles_refusals(args):
    with pytest.raises(InsarError):
        plan_tiles(*args)


# ---- window_1d -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, o", [(256, 32), (256, 128), (256, 0), (64, 5), (16, 8), (256, 1)])
def test_window_1d(T, o):
    r = window_1d(T, o)
    assert r.dtype == np.float32 and r.shape == (T,)
    assert (r > 0).all() and r.max() <= 1.0
    if o < T // 2:
        assert r[T // 2] == 1.0                  # a flat top unless the two ramps meet (o = T / 2)
    if o == 0:
        assert (r == 1.0).all()
    # two tiles at the regular stride T - o sum to one across their overlap
    j = np.arange(o)
    s = r[T - o + j] + r[j]
    assert np.abs(s - np.float32(1.0)).max(initial=0.0) <= np.finfo(np.float32).eps
    # the closed form
    i = np.arange(T)
    np.testing.assert_allclose(r, np.minimum(np.minimum(i + 1, T - i), o + 1) / (o + 1.0), rtol=1e-7)
    assert (r == r[::-1]).all()


def test_window_refusals():
    with pytest.raises(InsarError):
        window_1d(256, 129)
    with pytest.raises(InsarError):
        window_1d(256, -1)


# ---- the oracle against a brute-force per-pixel loop ---------------------------------------------------------------
@pytest.mark.parametrize("H, W, T, o, K", [(40, 48, 16, 4, 3), (43, 33, 16, 8, 2), (32, 48, 16, 0, 2)])
def test_oracle_matches_brute_force(H, W, T, o, K):
    origins = plan_tiles(H, W, T, o)
    rng = np.random.default_rng(17)
    lg = rng.standard_normal((len(origins), K, T, T)).astype(np.float32)
    prob, wsum = stitch_oracle(lg, origins, H, W, T, o)

    def r(i):
        return min(i + 1, T - i, o + 1) / (o + 1.0)

    brute = np.zeros((K, H, W))
    bw = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            num = np.zeros(K)
            for t, (y0, x0) in enumerate(origins):
                if y0 <= y < y0 + T and x0 <= x < x0 + T:
                    v = lg[t, :, y - y0, x - x0].astype(np.float64)
                    e = np.exp(v - v.max())
                    w = r(y - y0) * r(x - x0)
                    num += w * e / e.sum()
                    bw[y, x] += w
            brute[:, y, x] = num / bw[y, x]
    assert (bw > 0).all()
    np.testing.assert_allclose(wsum, bw, rtol=1e-13)
    np.testing.assert_allclose(prob, brute, rtol=0, atol=1e-13)
    np.testing.assert_allclose(prob.sum(axis=0), 1.0, rtol=0, atol=1e-13)
    if o == 0:
        assert (wsum[:T, :T] == 1.0).all()


# ---- argument checks of the entry points, without a GPU -------------------------------------------------------------
FAKE = 4096       # a non-null, 16-byte aligned "pointer": the checks below fail before anything dereferences it


def test_scene_symbols_exported():
    for name in ("insar_scene_gather", "insar_scene_blend", "insar_scene_finalize"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)


def test_scene_gather_validates_without_a_gpu():
    call = _lib.call
    with pytest.raises(InsarError, match="null"):
        call("insar_scene_gather", None, _lib.SCENE_U8, 600, 700, FAKE, 9, 256, FAKE, None)
    with pytest.raises(InsarError, match="null"):
        call("insar_scene_gather", FAKE, _lib.SCENE_U8, 600, 700, None, 9, 256, FAKE, None)
    with pytest.raises(InsarError, match="null"):
        call("insar_scene_gather", FAKE, _lib.SCENE_U8, 600, 700, FAKE, 9, 256, None, None)
    with pytest.raises(InsarError, match="dtype"):
        call("insar_scene_gather", FAKE, 7, 600, 700, FAKE, 9, 256, FAKE, None)
    with pytest.raises(InsarError, match="multiple of 16"):
        call("insar_scene_gather", FAKE, _lib.SCENE_U8, 600, 700, FAKE, 9, 250, FAKE, None)
    with pytest.raises(InsarError, match="smaller than the tile"):
        call("insar_scene_gather", FAKE, _lib.SCENE_U8, 200, 700, FAKE, 9, 256, FAKE, None)
    with pytest.raises(InsarError, match="no tiles"):
        call("insar_scene_gather", FAKE, _lib.SCENE_U8, 600, 700, FAKE, 0, 256, FAKE, None)


def test_scene_blend_validates_without_a_gpu():
    call = _lib.call
    ok = dict(logits=FAKE, origins=FAKE, n=9, K=2, T=256, o=32, acc=FAKE, wsum=FAKE, H=600, W=700, box=(0, 600, 0, 700))

    def blend(**kw):
        a = dict(ok, **kw)
        call("insar_scene_blend", a["logits"], a["origins"], a["n"], a["K"], a["T"], a["o"], a["acc"], a["wsum"], a["H"], a["W"],
             *a["box"], None)

    for name in ("logits", "origins", "acc", "wsum"):
        with pytest.raises(InsarError, match="null"):
            blend(**{name: None})
    for K in (0, 1, 9, 1024):
        with pytest.raises(InsarError, match="num_classes"):
            blend(K=K)
    with pytest.raises(InsarError, match="overlap"):
        blend(o=129)
    with pytest.raises(InsarError, match="overlap"):
        blend(o=-1)
    with pytest.raises(InsarError, match="multiple of 16"):
        blend(T=100, o=0)
    with pytest.raises(InsarError, match="smaller than the tile"):
        blend(H=255)
    with pytest.raises(InsarError, match="no tiles"):
        blend(n=0)
    for box in ((0, 601, 0, 700), (0, 600, -1, 700), (300, 300, 0, 700), (0, 600, 0, 701)):
        with pytest.raises(InsarError, match="box"):
            blend(box=box)
    with pytest.raises(InsarError, match=r"\(-1001\)"):                 # INSAR_E_SHAPE, not a launch failure
        blend(K=9)
    with pytest.raises(InsarError, match=r"\(-1005\)"):                 # INSAR_E_ARG
        blend(acc=None)


def test_scene_finalize_validates_without_a_gpu():
    call = _lib.call
    for args in ((None, FAKE, 2, 600, 700, FAKE, FAKE, FAKE), (FAKE, None, 2, 600, 700, FAKE, FAKE, FAKE),
                 (FAKE, FAKE, 2, 600, 700, FAKE, None, FAKE), (FAKE, FAKE, 2, 600, 700, FAKE, FAKE, None)):
        with pytest.raises(InsarError, match="null"):
            call("insar_scene_finalize", *args, None)
    for K in (1, 9):
        with pytest.raises(InsarError, match="num_classes"):
            call("insar_scene_finalize", FAKE, FAKE, K, 600, 700, None, FAKE, FAKE, None)
    with pytest.raises(InsarError, match="empty scene"):
        call("insar_scene_finalize", FAKE, FAKE, 2, 0, 700, None, FAKE, FAKE, None)


# ---- host-side refusals of the Python API (before any launch; no device needed to refuse) -------------------------
def test_predictor_constructor_refusals():
    import torch

    from insar_unet_ca_amd.infer import ScenePredictor
    net = torch.nn.Conv2d(1, 2, 1)
    with pytest.raises(InsarError):
        ScenePredictor(net, tile=256, overlap=129)
    with pytest.raises(InsarError):
        ScenePredictor(net, tile=250, overlap=0)
    with pytest.raises(InsarError):
        ScenePredictor(net, num_classes=9)
    with pytest.raises(InsarError):
        ScenePredictor(net, batch=0)
    # no CPU fallback: a host model is refused, not run in eager PyTorch
    with pytest.raises(InsarError):
        ScenePredictor(net, tile=16, overlap=0).predict(np.zeros((32, 32), dtype=np.uint8))

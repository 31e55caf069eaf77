"""Host: scenes with no-data (insar_unet_ca_amd/infer.py): the tile selection against the restatement of
tests/scene_valid_ref.py, the covering property that the default `min_valid=1` gives, and every refusal of the new arguments,
raised by name before anything is copied to a device (the predictor here wraps a CPU module: had a check let its argument
through, the refusal would be the device's)."""
import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib
from insar_unet_ca_amd._lib import InsarError
from tests import scene_valid_ref as ref

TILE, OVERLAP = 32, 8


# ---- select_tiles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_valid", [1, 5, TILE * TILE])
def test_select_tiles_against_the_restatement(min_valid):
    rng = np.random.default_rng(min_valid)
    counts = rng.integers(0, TILE * TILE + 1, size=40).astype(np.int32)
    counts[[3, 9]] = min_valid                     # ties at exactly min_valid are kept
    counts[[4, 10]] = min_valid - 1                # one short is not
    counts[[0, 17]] = TILE * TILE
    got = iu.select_tiles(counts, min_valid)
    assert np.array_equal(got, ref.select_tiles(counts, min_valid))
    assert np.issubdtype(got.dtype, np.integer) and got.ndim == 1 and (np.diff(got) > 0).all()
    assert 3 in got and 9 in got and 4 not in got and 10 not in got and 0 in got


def test_select_tiles_on_an_empty_census_and_by_default():
    zero = np.zeros(7, dtype=np.int32)
    for mv in (1, TILE * TILE):
        assert iu.select_tiles(zero, mv).size == 0
    assert np.array_equal(iu.select_tiles(np.array([0, 1, 0, 2], dtype=np.int32)), [1, 3])
    assert np.array_equal(iu.select_tiles(np.full(5, TILE * TILE, dtype=np.int32), TILE * TILE), np.arange(5))


@pytest.mark.parametrize("bad", [0, -1, True, 1.0, "1", None])
def test_select_tiles_refuses_a_min_valid_that_is_no_positive_integer(bad):
    with pytest.raises(InsarError, match="select_tiles: min_valid="):
        iu.select_tiles(np.zeros(3, dtype=np.int32), bad)
    with pytest.raises(InsarError, match="select_tiles: counts"):
        iu.select_tiles(np.zeros((3, 2), dtype=np.int32), 1)
    with pytest.raises(InsarError, match="select_tiles: counts"):
        iu.select_tiles(np.zeros(3, dtype=np.float32), 1)


# ---- the covering property -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, H, W, density", [(0, 96, 136, 0.002), (1, 81, 101, 0.0005), (2, 64, 128, 0.01), (3, 96, 136, 0.0)])
def test_every_tile_that_holds_a_valid_pixel_is_run_at_min_valid_1(seed, H, W, density):
    """With min_valid = 1 a valid pixel keeps exactly the covering tiles it has in a full predict."""
    rng = np.random.default_rng(seed)
    valid_px = rng.random((H, W)) < density
    origins = iu.plan_tiles(H, W, TILE, OVERLAP)
    counts = ref.census(valid_px, origins, TILE)
    kept = set(iu.select_tiles(counts, 1).tolist())
    for i, (y, x) in enumerate(origins):
        assert (i in kept) == bool(valid_px[y:y + TILE, x:x + TILE].any())
    for y, x in zip(*np.nonzero(valid_px)):
        covering = {i for i, (y0, x0) in enumerate(origins) if y0 <= y < y0 + TILE and x0 <= x < x0 + TILE}
        assert covering and covering <= kept
    assert ref.covered(origins[sorted(kept)], TILE, H, W)[valid_px].all()


# ---- the restatement itself ------------------------------------------------------------------------------------------------
def test_validity_rule_of_the_restatement():
    f = np.array([[1.0, np.nan, np.inf, -np.inf, -2.5, 0.0]], dtype=np.float32)
    assert ref.valid_pixels(f).tolist() == [[True, False, False, False, True, True]]
    assert ref.valid_pixels(f, nodata=-2.5).tolist() == [[True, False, False, False, False, True]]
    assert ref.valid_pixels(f, nodata=float("nan")).tolist() == [[True, False, False, False, True, True]]
    assert ref.valid_pixels(f, valid=np.array([[0, 1, 1, 1, 2, 255]], dtype=np.uint8)).tolist() == [[False, False, False, False, True, True]]
    u = np.array([[0, 7, 255]], dtype=np.uint8)
    assert ref.valid_pixels(u).all() and ref.valid_pixels(u, nodata=7).tolist() == [[True, False, True]]
    g = ref.gather_ref(np.full((16, 16), np.nan, dtype=np.float32), np.array([[0, 0]]), 16, fill=0.25, norm=(1.0, 2.0))
    assert (g == np.float32(0.25)).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pred():
    return iu.ScenePredictor(torch.nn.Linear(1, 1), tile=TILE, overlap=OVERLAP, batch=2, num_classes=2)


U8 = np.zeros((64, 80), dtype=np.uint8)
F32 = np.zeros((64, 80), dtype=np.float32)
OK_VALID = np.ones((64, 80), dtype=np.uint8)

REFUSALS = [
    ("valid", U8, dict(valid=OK_VALID.astype(np.float32))),
    ("valid", U8, dict(valid=OK_VALID.astype(bool))),
    ("valid", U8, dict(valid=OK_VALID[:, :79])),
    ("valid", F32, dict(valid=torch.ones(64, 80, dtype=torch.int32))),
    ("valid", F32, dict(valid=torch.ones(80, 64, dtype=torch.uint8))),
    ("valid", F32, dict(valid=[[1]])),
    ("nodata", U8, dict(nodata=256)),
    ("nodata", U8, dict(nodata=-1)),
    ("nodata", U8, dict(nodata=1.5)),
    ("nodata", U8, dict(nodata=float("nan"))),
    ("nodata", U8, dict(nodata=True)),
    ("nodata", F32, dict(nodata="nan")),
    ("min_valid", U8, dict(nodata=0, min_valid=0)),
    ("min_valid", U8, dict(nodata=0, min_valid=TILE * TILE + 1)),
    ("min_valid", U8, dict(min_valid=True)),
    ("min_valid", F32, dict(nodata=0.0, min_valid=2.0)),
    ("fill", U8, dict(nodata=0, fill=float("nan"))),
    ("fill", F32, dict(nodata=0.0, fill=float("inf"))),
    ("fill", F32, dict(fill="0")),
    ("norm", U8, dict(norm=(0.0, 1.0))),
    ("scale", F32, dict(norm=(0.0, 0.0))),
    ("scale", F32, dict(norm=(0.0, float("inf")))),
    ("scale", F32, dict(norm=(0.0, float("nan")))),
    ("offset", F32, dict(norm=(float("nan"), 1.0))),
    ("norm", F32, dict(norm=1.0)),
    ("norm", F32, dict(norm=(0.0, 1.0, 2.0))),
    ("norm", F32, dict(norm=("a", 1.0))),
]


@pytest.mark.parametrize("name, scene, kw", REFUSALS, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(REFUSALS)])
def test_refusals_name_the_argument_before_anything_is_copied(pred, name, scene, kw):
    for run in (pred.predict, pred.detect, lambda s, **k: pred.evaluate(s, np.zeros(s.shape, dtype=np.uint8), **k)):
        with pytest.raises(InsarError, match=rf"predict: .*\b{name}\b"):
            run(scene, **kw)
    stack_kw = {k: v for k, v in kw.items() if k != "valid"}
    if stack_kw:
        with pytest.raises(InsarError, match=rf"predict: .*\b{name}\b"):
            pred.detect_stack([scene, scene], **stack_kw)


@pytest.mark.parametrize("scene, kw", [(U8, dict(valid=OK_VALID, nodata=255, min_valid=TILE * TILE, fill=-0.5)),
                                       (U8, dict(nodata=3.0)), (F32, dict(nodata=float("nan"), norm=(3.0, -0.5))),
                                       (F32, dict(valid=torch.ones(64, 80, dtype=torch.uint8), nodata=np.float32(-9999), norm=[0, 2]))])
def test_arguments_that_pass_reach_the_device_refusal(pred, scene, kw):
    with pytest.raises(InsarError, match="ROCm device"):
        pred.predict(scene, **kw)
    with pytest.raises(InsarError, match="ROCm device"):
        iu.predict_scene(torch.nn.Linear(1, 1), scene, tile=TILE, overlap=OVERLAP, **kw)


def test_the_device_helpers_refuse_host_tensors_and_bad_arguments():
    sc, o = torch.zeros(64, 80), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(InsarError, match="tile_census: scene and origins must be ROCm tensors"):
        iu.tile_census(sc, o, TILE, nodata=0.0)
    with pytest.raises(InsarError, match="gather_tiles: scene and origins must be ROCm tensors"):
        iu.gather_tiles(sc, o, TILE, nodata=0.0)


def test_abi_is_additive():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 8
    for name, nargs in (("insar_scene_census", 12), ("insar_scene_gather_valid", 16), ("insar_scene_finalize_valid", 15)):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and len(_lib._SIGNATURES[name]) == nargs
    assert len(_lib._SIGNATURES["insar_scene_gather"]) == 9 and len(_lib._SIGNATURES["insar_scene_finalize"]) == 9
    for name in ("tile_census", "select_tiles", "gather_tiles"):
        assert name in iu.__all__ and callable(getattr(iu, name))


def test_entry_points_validate_before_they_touch_a_device():
    call = _lib.call
    with pytest.raises(InsarError, match="insar_scene_census: null pointer"):
        call("insar_scene_census", None, 0, 64, 80, None, 0, 0.0, None, 1, TILE, None, None)
    with pytest.raises(InsarError, match="nodata 300 of a uint8 scene"):
        call("insar_scene_census", 16, 0, 64, 80, None, 1, 300.0, 16, 1, TILE, 16, None)
    with pytest.raises(InsarError, match="smaller than the tile"):
        call("insar_scene_census", 16, 1, 16, 80, None, 0, 0.0, 16, 1, TILE, 16, None)
    with pytest.raises(InsarError, match="fill is not finite"):
        call("insar_scene_gather_valid", 16, 1, 64, 80, None, 0, 0.0, float("inf"), 0, 0.0, 1.0, 16, 1, TILE, 16, None)
    with pytest.raises(InsarError, match="norm is for float32 scenes"):
        call("insar_scene_gather_valid", 16, 0, 64, 80, None, 0, 0.0, 0.0, 1, 0.0, 1.0, 16, 1, TILE, 16, None)
    with pytest.raises(InsarError, match="finite non-zero scale"):
        call("insar_scene_gather_valid", 16, 1, 64, 80, None, 0, 0.0, 0.0, 1, 0.0, 0.0, 16, 1, TILE, 16, None)
    with pytest.raises(InsarError, match="insar_scene_finalize_valid: null pointer"):
        call("insar_scene_finalize_valid", 16, 16, 2, 64, 80, 16, 0, None, 0, 0.0, None, 16, 16, None, None)
    with pytest.raises(InsarError, match="num_classes 9"):
        call("insar_scene_finalize_valid", 16, 16, 9, 64, 80, 16, 0, None, 0, 0.0, None, 16, 16, 16, None)

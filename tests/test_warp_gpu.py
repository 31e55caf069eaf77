"""GPU: csrc/warp.hip (insar_warp_raster / _gather / _draw, insar_multilook), insar_unet_ca_amd/warp.py and SceneCrops(warp=)
against the numpy restatement in tests/warp_ref.py. Every comparison is bitwise, float32 through its int32 view."""
import math

import numpy as np
import pytest
import torch

from tests import warp_ref as ref

pytestmark = pytest.mark.gpu
IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
SOURCES = [(37, 53), (64, 96)]
OUTPUTS = [(41, 29), (128, 128)]              # 29 and 53 are no multiples of 4: the guarded stores run
NP = {"u8": np.uint8, "f32": np.float32, "i32": np.int32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _same(t: torch.Tensor, want: np.ndarray) -> bool:
    got = t.detach().cpu().numpy()
    if want.dtype == np.float32:
        return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def source(shape, kind, C, seed=0):
    """[H, W] (C = 1) or [C, H, W]; float32 sources carry NaN holes: single pixels and one block."""
    rng = np.random.default_rng(1000 * shape[0] + 10 * C + seed)
    full = (shape if C == 1 else (C,) + shape)
    if kind == "f32":
        a = (rng.standard_normal(full) * 50.0).astype(np.float32)
        a[rng.random(full) < 0.03] = np.nan
        a[..., 5:9, 11:14] = np.nan
        return a
    if kind == "u8":
        return rng.integers(0, 256, size=full).astype(np.uint8)
    return rng.integers(-2 ** 31, 2 ** 31, size=full).astype(np.int32)


def matrices(H, W, h, w):
    """The issue's seven: identity, a sub-pixel shift, 0.5 x and 3 x zoom, 30 degrees about the centres, a shear, mostly outside."""
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    cx, cy, ox, oy = (W - 1) / 2, (H - 1) / 2, (w - 1) / 2, (h - 1) / 2
    return {"identity": IDENTITY,
            "shift": [[1.0, 0.0, 0.37], [0.0, 1.0, -0.61]],
            "zoom0.5": [[0.5, 0.0, -0.25], [0.0, 0.5, -0.25]],
            "zoom3": [[3.0, 0.0, 1.0], [0.0, 3.0, 1.0]],
            "rot30": [[c, -s, cx - c * ox + s * oy], [s, c, cy - s * ox - c * oy]],
            "shear": [[1.0, 0.4, -3.0], [0.15, 1.0, 2.0]],
            "outside": [[1.0, 0.0, W - 5.3], [0.0, 1.0, H - 4.2]]}


FILLS = {"u8": 7, "i32": -5, "f32": None}          # None: the float32 default, NaN


# ---- warp_raster ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_shape", OUTPUTS)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", ["u8", "f32", "i32"])
@pytest.mark.parametrize("shape", SOURCES)
def test_warp_raster_equals_the_reference(dev, shape, kind, C, out_shape):
    import insar_unet_ca_amd as iu
    src = source(shape, kind, C)
    d_src = torch.from_numpy(src).to(dev)
    h, w = out_shape
    fill = FILLS[kind]
    ref_fill = np.float32(np.nan) if fill is None else fill
    for name, m in matrices(*shape, h, w).items():
        q = ref.quantise(m)
        for mode in (("nearest",) if kind == "i32" else ("nearest", "bilinear")):
            want, want_valid = ref.warp(src, q, h, w, mode, ref_fill)
            got, valid = iu.warp_raster(d_src, m, out_shape, mode=mode, fill=fill, return_valid=True)
            assert _same(valid, want_valid), (name, mode, "valid")
            assert _same(got, want), (name, mode)
            if name == "outside":
                assert 0 < want_valid.mean() < 0.25
            if name == "identity" and h <= shape[0] and w <= shape[1]:
                crop = np.ascontiguousarray(src[..., :h, :w])
                if kind == "f32" and mode == "bilinear":          # a NaN tap gives NaN at weight 0 too: the holes grow up and left
                    keep = ~np.isnan(want)
                    assert keep.mean() > 0.5 and np.array_equal(want[keep], crop[keep]) and np.isnan(want[np.isnan(crop)]).all()
                else:
                    assert _same(got, crop)
    assert _same(iu.warp_raster(d_src, IDENTITY, out_shape, mode="nearest", fill=fill),
                 ref.warp(src, ref.quantise(IDENTITY), h, w, "nearest", ref_fill)[0])


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_warp_raster_table_of_matrices_out_and_misaligned_outputs(dev, kind):
    """n warps in one launch from a device table; `out=`; a destination that is not aligned to the wide store."""
    import insar_unet_ca_amd as iu
    shape, (h, w) = (37, 53), (24, 32)
    src = source(shape, kind, 3)
    d_src = torch.from_numpy(src).to(dev)
    ms = matrices(*shape, h, w)
    qs = np.stack([ref.quantise(ms[k]) for k in ("rot30", "shear", "shift", "outside", "zoom3")])
    table = torch.from_numpy(qs).to(dev)
    fill = 3 if kind == "u8" else -1.5
    want = [ref.warp(src, q, h, w, "bilinear", fill) for q in qs]
    got, valid = iu.warp_raster(d_src, table, (h, w), fill=fill, return_valid=True)
    assert got.shape == (5, 3, h, w) and _same(got, np.stack([o for o, _ in want])) and _same(valid, np.stack([v for _, v in want]))
    flat = torch.full((3 * h * w + 8,), 99, dtype=d_src.dtype, device=dev)
    out = flat[1:1 + 3 * h * w].view(3, h, w)                       # one element off every wide store's alignment
    assert iu.warp_raster(d_src, ms["rot30"], (h, w), fill=fill, out=out) is out
    assert _same(out, want[0][0]) and flat[0].item() == 99 and (flat[1 + 3 * h * w:] == 99).all().item()
    got2 = iu.warp_raster(d_src[0], table[1:2], (h, w), fill=fill)
    assert got2.shape == (1, h, w) and _same(got2, want[1][0][None, 0])


def test_warp_raster_refusals(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import InsarError
    f = torch.zeros(8, 8, device=dev)
    bad = [dict(mode="cubic"), dict(out_shape=(0, 8)), dict(out_shape=(8, 40000)), dict(out_shape=8), dict(fill="x"),
           dict(matrix=[[1, 0, 2.0 ** 21], [0, 1, 0]]), dict(matrix=[[1, 0, math.nan], [0, 1, 0]]), dict(matrix=[[1, 0, 0]]),
           dict(out=torch.zeros(8, 9, device=dev)), dict(out=torch.zeros(8, 8, device=dev, dtype=torch.uint8)), dict(out=f),
           dict(matrix=torch.zeros(2, 5, dtype=torch.int64, device=dev)), dict(matrix=torch.zeros(1, 6, dtype=torch.int64))]
    for kw in bad:
        args = dict(matrix=IDENTITY, out_shape=(8, 8))
        args.update(kw)
        with pytest.raises(InsarError):
            iu.warp_raster(f, args.pop("matrix"), args.pop("out_shape"), **args)
    with pytest.raises(InsarError, match="int32"):
        iu.warp_raster(torch.zeros(8, 8, dtype=torch.int32, device=dev), IDENTITY, (8, 8))
    with pytest.raises(InsarError, match="channels"):
        iu.warp_raster(torch.zeros(5, 8, 8, device=dev), IDENTITY, (8, 8))
    with pytest.raises(InsarError, match="dtype"):
        iu.warp_raster(torch.zeros(8, 8, dtype=torch.float64, device=dev), IDENTITY, (8, 8))
    with pytest.raises(InsarError, match="contiguous"):
        iu.warp_raster(torch.zeros(8, 16, device=dev)[:, ::2], IDENTITY, (8, 8))
    for fill in (256, -1, 1.5):
        with pytest.raises(InsarError, match="fill"):
            iu.warp_raster(torch.zeros(8, 8, dtype=torch.uint8, device=dev), IDENTITY, (8, 8), fill=fill)
    for kw in (dict(fy=0), dict(fy=17), dict(fy=2, fx=9), dict(fy=2, min_valid=5), dict(fy=2, min_valid=0), dict(fy=2.0)):
        with pytest.raises(InsarError):
            iu.multilook(f, **kw)
    with pytest.raises(InsarError, match="dtype"):
        iu.multilook(torch.zeros(8, 8, dtype=torch.int32, device=dev), 2)


# ---- multilook -----------------------------------------------------------------------------------------------------------------
# 50 x 83 is the issue's shape (element-wise loads: 83 % 4 != 0); 48 x 96 takes the wide loads at fx = 1, 2, 4, 8 and the
# element-wise ones at fx = 3, 16; 20 x 100 at fx = 2 ends its rows with a quad that is not whole
LOOKS = [((50, 83), f) for f in ((1, 1), (2, 2), (3, 5), (16, 16))] + \
        [((48, 96), f) for f in ((1, 1), (2, 2), (4, 4), (3, 8), (5, 3), (16, 16))] + [((20, 100), (2, 2)), ((20, 100), (1, 4))]


@pytest.mark.parametrize("kind, C", [("u8", 1), ("f32", 1), ("f32", 3), ("u8", 2)])
@pytest.mark.parametrize("shape, factors", LOOKS)
def test_multilook_equals_the_reference(dev, shape, factors, kind, C):
    import insar_unet_ca_amd as iu
    fy, fx = factors
    src = source(shape, kind, C, seed=fy)
    d_src = torch.from_numpy(src).to(dev)
    for min_valid in (1, fy * fx):
        want, want_count = ref.multilook(src, fy, fx, min_valid)
        got, count = iu.multilook(d_src, fy, fx, min_valid=min_valid, return_count=True)
        assert _same(count, want_count) and _same(got, want), (min_valid,)
    if kind == "f32":
        assert np.isnan(want).any() and not np.isnan(ref.multilook(src, fy, fx, 1)[0]).all()
    assert _same(iu.multilook(d_src, fy, fx), ref.multilook(src, fy, fx)[0])
    if fy == fx:
        assert _same(iu.multilook(d_src, fy), ref.multilook(src, fy, fx)[0])


# ---- draw_warps and gather_warped ----------------------------------------------------------------------------------------------
def scene_and_labels(kind, seed=5, shape=(128, 128)):
    rng = np.random.default_rng(seed)
    scene = rng.integers(0, 256, size=shape).astype(np.uint8) if kind == "u8" else (rng.standard_normal(shape) * 3).astype(np.float32)
    labels = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=shape, p=[0.6, 0.2, 0.1, 0.1])
    labels[40:70, 30:90] = 1
    return scene, labels


@pytest.mark.parametrize("n", [1, 5, 64])
def test_draw_warps_equals_the_reference(dev, n):
    import insar_unet_ca_amd as iu
    rng = np.random.default_rng(n)
    origins = (rng.integers(0, 12, size=(n, 2)) * 8).astype(np.int32)
    d_origins = torch.from_numpy(origins).to(dev)
    table = ref.angle_table()
    for key, T, spec in ((0x1234567890ABCDEF, 32, iu.WarpSpec(zoom=(0.75, 1.5), max_angle_deg=30)),
                         (7, 16, iu.WarpSpec(zoom=(1.0, 1.0), max_angle_deg=180)), (2 ** 64 - 1, 64, iu.WarpSpec(zoom=(0.5, 16.0))),
                         (99, 32, iu.WarpSpec())):
        got = iu.draw_warps(key, d_origins, T, spec)
        assert _same(got, ref.draw(key, origins, T, spec.amax, spec.zoom_lo, spec.zoom_hi, table)), (key, T)
    ident = iu.draw_warps(99, d_origins, 32, iu.WarpSpec()).cpu().numpy()
    assert ident.tolist() == [[1 << 32, 0, int(x) << 32, 0, 1 << 32, int(y) << 32] for y, x in origins]


@pytest.mark.parametrize("mask_dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("T", [16, 32])
def test_identity_warps_reproduce_gather_crops(dev, T, kind, mask_dtype):
    import insar_unet_ca_amd as iu
    scene, labels = scene_and_labels(kind)
    d_scene, d_labels = torch.from_numpy(scene).to(dev), torch.from_numpy(labels).to(dev)
    rng = np.random.default_rng(T)
    origins = rng.integers(0, 128 - T + 1, size=(6, 2)).astype(np.int32)
    origins[0], origins[1] = (0, 0), (128 - T, 128 - T)
    d_origins = torch.from_numpy(origins).to(dev)
    mats = iu.draw_warps(3, d_origins, T, iu.WarpSpec(zoom=(1.0, 1.0), max_angle_deg=0.0))
    want_img, want_mask = iu.gather_crops(d_scene, d_labels, d_origins, T, mask_dtype)
    got_img, got_mask = iu.gather_warped(d_scene, d_labels, mats, T, mask_dtype)
    assert got_img.shape == (6, 1, T, T) and got_mask.dtype == mask_dtype
    assert torch.equal(got_img.view(torch.int32), want_img.view(torch.int32)) and torch.equal(got_mask, want_mask)
    only_img, none = iu.gather_warped(d_scene, None, mats, T)
    none2, only_mask = iu.gather_warped(None, d_labels, mats, T, mask_dtype)
    assert none is None and none2 is None and torch.equal(only_img.view(torch.int32), want_img.view(torch.int32))
    assert torch.equal(only_mask, want_mask)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("T", [16, 32])
def test_gather_warped_equals_the_reference(dev, T, kind):
    import insar_unet_ca_amd as iu
    scene, labels = scene_and_labels(kind, seed=9, shape=(96, 128))
    d_scene, d_labels = torch.from_numpy(scene).to(dev), torch.from_numpy(labels).to(dev)
    origins = np.array([[0, 0], [96 - T, 128 - T], [32, 48], [8, 96], [64, 0]], dtype=np.int32)      # the corner tiles leave the scene
    spec = iu.WarpSpec(zoom=(0.6, 1.8), max_angle_deg=180)
    mats = iu.draw_warps(41, torch.from_numpy(origins).to(dev), T, spec)
    qs = ref.draw(41, origins, T, spec.amax, spec.zoom_lo, spec.zoom_hi, ref.angle_table())
    assert _same(mats, qs)
    want_img, want_mask = ref.gather(scene, labels, qs, T, fill=-2.0)
    assert (want_mask == 255).any() and (want_img == np.float32(-2.0)).any()
    for mask_dtype in (torch.uint8, torch.int64):
        img, mask = iu.gather_warped(d_scene, d_labels, mats, T, mask_dtype, fill=-2.0)
        assert _same(img, want_img) and _same(mask, want_mask.astype(np.int64 if mask_dtype == torch.int64 else np.uint8))
    # the image and mask of gather_warped are the two modes of warp_raster on one table
    if kind == "f32":
        assert _same(iu.warp_raster(d_scene, mats, (T, T), fill=-2.0), want_img[:, 0])
    assert _same(iu.warp_raster(d_labels, mats, (T, T), mode="nearest", fill=255), want_mask)


# ---- SceneCrops(warp=) ---------------------------------------------------------------------------------------------------------
def _crops(dev, warp="absent", **kw):
    import insar_unet_ca_amd as iu
    scene, labels = scene_and_labels("u8", seed=21)
    args = dict(tile=32, batch=4, steps_per_epoch=3, num_classes=3, cell=8, seed=11, rank=1, device=dev)
    args.update(kw)
    if warp != "absent":
        args["warp"] = warp
    return iu.SceneCrops(scene, labels, **args)


def _batches(crops, n):
    out = []
    for _ in range(n):
        img, mask = crops.next_batch()
        out.append((img.clone(), mask.clone(), crops.last_origins.clone(), None if crops.last_matrices is None else crops.last_matrices.clone()))
    return out


def _equal_batches(a, b):
    return len(a) == len(b) and all(torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1], y[1])
                                    and torch.equal(x[2], y[2]) and (x[3] is None) == (y[3] is None)
                                    and (x[3] is None or torch.equal(x[3], y[3])) for x, y in zip(a, b))


def test_scene_crops_with_a_warp(dev):
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd import InsarError
    spec = iu.WarpSpec(zoom=(0.8, 1.25), max_angle_deg=20)
    one, two = _crops(dev, spec), _crops(dev, iu.WarpSpec(zoom=(0.8, 1.25), max_angle_deg=20))
    a = _batches(one, 4)
    assert _equal_batches(a, _batches(two, 4))                                # one seed, one stream
    assert not torch.equal(a[0][3], a[1][3]) and a[0][3].shape == (4, 6) and a[0][3].dtype == torch.int64
    # every batch is the reference's, from the origins and the key of its step
    scene, labels = scene_and_labels("u8", seed=21)
    for step, (img, mask, origins, mats) in enumerate(a):
        qs = ref.draw(one.key(step), origins.cpu().numpy(), 32, spec.amax, spec.zoom_lo, spec.zoom_hi, ref.angle_table())
        want_img, want_mask = ref.gather(scene, labels, qs, 32)
        assert _same(mats, qs) and _same(img, want_img) and _same(mask, want_mask.astype(np.int64))
    # resume: a fresh object that loads the state after two batches continues with the third and fourth
    three = _crops(dev, spec)
    _batches(three, 2)
    state = three.state_dict()
    assert state["config"]["warp"] == spec.config() and state["step"] == 2
    four = _crops(dev, spec)
    four.load_state_dict(state)
    assert _equal_batches(_batches(four, 2), a[2:])
    # warp=None is the object built without the argument: same batches, same config, no matrices
    plain, none = _crops(dev), _crops(dev, None)
    assert "warp" not in plain._config() and plain._config() == none._config()
    b = _batches(plain, 3)
    assert _equal_batches(b, _batches(none, 3)) and b[0][3] is None
    assert torch.equal(b[0][2], a[0][2])                                      # the origins do not depend on the warp
    # a state saved without a warp does not load into an object with one, nor the other way round, nor another spec's
    with pytest.raises(InsarError, match="config"):
        _crops(dev, spec).load_state_dict(plain.state_dict())
    with pytest.raises(InsarError, match="config"):
        plain.load_state_dict(one.state_dict())
    with pytest.raises(InsarError, match="config"):
        _crops(dev, iu.WarpSpec(zoom=(0.8, 1.25), max_angle_deg=21)).load_state_dict(one.state_dict())
    # with an Augment the warped batch goes through it as the plain one does
    aug = _crops(dev, spec, augment=iu.Augment(seed=2, rank=1))
    img, mask = aug.next_batch()
    assert img.shape == (4, 1, 32, 32) and mask.shape == (4, 32, 32) and mask.dtype == torch.int64


# ---- composition ---------------------------------------------------------------------------------------------------------------
def test_labels_to_a_finer_grid_and_back(dev):
    """Nearest to a grid of half the spacing and back reproduces the map; so does multilook's grid for a mask predicted there."""
    import insar_unet_ca_amd as iu
    _, labels = scene_and_labels("u8", seed=33, shape=(64, 96))
    d = torch.from_numpy(labels).to(dev)
    coarse, fine = [[2.0, 0.0, 100.0], [0.0, -2.0, 900.0]], [[1.0, 0.0, 100.0], [0.0, -1.0, 900.0]]
    up = iu.warp_raster(d, iu.grid_matrix(coarse, fine), (128, 192), mode="nearest", fill=255)
    assert _same(up, np.repeat(np.repeat(labels, 2, axis=0), 2, axis=1))
    back, valid = iu.warp_raster(up, iu.grid_matrix(fine, coarse), (64, 96), mode="nearest", fill=255, return_valid=True)
    assert _same(back, labels) and valid.all().item()
    wide = iu.warp_raster(d.to(torch.int32), iu.grid_matrix(coarse, fine), (128, 192), mode="nearest")
    assert _same(wide, np.repeat(np.repeat(labels.astype(np.int32), 2, axis=0), 2, axis=1))

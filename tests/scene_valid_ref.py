"""A numpy restatement of the no-data semantics of whole-scene inference ("Scenes with no-data" in DESIGN.md; the prototypes of
insar_scene_census / _gather_valid / _finalize_valid in include/insar_hip.h), written from the rule and not from the kernels.

A pixel is valid iff its byte of `valid` is non-zero (None: every one), its value is not `nodata` (None: no such value; an exact
compare) and, in a float32 scene, it is finite."""
import numpy as np


def valid_pixels(scene: np.ndarray, valid=None, nodata=None) -> np.ndarray:
    """bool [H, W]."""
    ok = np.ones(scene.shape, dtype=bool) if valid is None else np.asarray(valid) != 0
    if scene.dtype == np.float32:
        ok = ok & np.isfinite(scene)
        if nodata is not None:
            ok = ok & ~(scene == np.float32(nodata))             # a NaN no-data value equals nothing
    else:
        assert scene.dtype == np.uint8
        if nodata is not None:
            ok = ok & (scene != int(nodata))
    return ok


def _inside(y0, x0, tile, H, W) -> bool:
    return y0 >= 0 and x0 >= 0 and y0 + tile <= H and x0 + tile <= W


def census(valid_px: np.ndarray, origins, tile: int) -> np.ndarray:
    """int32 [N]: the valid pixels of every tile; a tile that is not inside the scene counts 0."""
    H, W = valid_px.shape
    return np.array([int(valid_px[y:y + tile, x:x + tile].sum()) if _inside(y, x, tile, H, W) else 0 for y, x in np.asarray(origins)],
                    dtype=np.int32)


def select_tiles(counts, min_valid: int = 1) -> np.ndarray:
    return np.array([i for i, c in enumerate(counts) if c >= min_valid], dtype=np.int64)


def covered(origins, tile: int, H: int, W: int) -> np.ndarray:
    """bool [H, W]: the pixels under at least one of the tiles."""
    c = np.zeros((H, W), dtype=bool)
    for y, x in np.asarray(origins).reshape(-1, 2):
        c[y:y + tile, x:x + tile] = True
    return c


def normalise_u8(v: np.ndarray) -> np.ndarray:
    """The reference's ToTensor + Normalize(0.5, 0.5) in float32, in its order."""
    x = v.astype(np.float32) / np.float32(255.0)
    return (x - np.float32(0.5)) / np.float32(0.5)


def gather_ref(scene: np.ndarray, origins, tile: int, valid=None, nodata=None, fill: float = 0.0, norm=None) -> np.ndarray:
    """float32 [n, 1, tile, tile]: the network input. Invalid pixels are `fill`; no arithmetic touches their values."""
    ok = valid_pixels(scene, valid, nodata)
    if scene.dtype == np.uint8:
        x = normalise_u8(scene)
    else:
        x = np.where(ok, scene, np.float32(0.0)).astype(np.float32)
        if norm is not None:
            x = (x - np.float32(norm[0])).astype(np.float32) * np.float32(norm[1])
    x = np.where(ok, x, np.float32(fill)).astype(np.float32)
    H, W = scene.shape
    out = np.zeros((len(origins), 1, tile, tile), dtype=np.float32)
    for i, (y, x0) in enumerate(np.asarray(origins)):
        if _inside(y, x0, tile, H, W):
            out[i, 0] = x[y:y + tile, x0:x0 + tile]
    return out


def mask_outputs(out: dict, valid_px: np.ndarray, covered_px: np.ndarray) -> dict:
    """The outputs of a finalize ("mask", "conf" and, where present, "prob", numpy) with everything forced to 0 where the pixel
    is invalid or uncovered, plus "valid" uint8 [H, W] = valid and covered."""
    keep = valid_px & covered_px
    res = {"mask": np.where(keep, out["mask"], 0).astype(np.uint8), "conf": np.where(keep, out["conf"], np.float32(0)).astype(np.float32),
           "valid": keep.astype(np.uint8)}
    if "prob" in out:
        res["prob"] = np.where(keep[None], out["prob"], np.float32(0)).astype(np.float32)
    return res

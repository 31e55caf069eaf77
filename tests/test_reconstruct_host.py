"""CPU-only: the two restatements of tests/reconstruct_ref.py, the sequential priority flood (a) and the tile-Jacobi rounds (b),
agree with each other and with answers known from elsewhere (scipy's binary propagation, a cone with a pit, the order dual), the
key maps round-trip, and the host side of insar_unet_ca_amd/reconstruct.py refuses what it can refuse without a device."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

from insar_unet_ca_amd import _lib
from insar_unet_ca_amd import reconstruct as rc
from insar_unet_ca_amd._lib import InsarError
from tests import reconstruct_ref as ref

DTYPES = (np.float32, np.uint8, np.int32)


def _both(mode, raster, T=5, **kw):
    """The outputs of (a), after holding (b) at tile edge T to them."""
    a = ref.run(mode, raster, solver="flood", **kw)
    b = ref.run(mode, raster, solver=("jacobi", T), **kw)
    for n in ("out", "residue", "extrema", "valid"):
        assert a[n].tobytes() == b[n].tobytes() and a[n].dtype == b[n].dtype and a[n].shape == b[n].shape, n
    assert b["converged"] and b["rounds"] >= 1
    return a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("connectivity", (4, 8))
def test_flood_equals_tile_jacobi_on_random_inputs(dtype, connectivity):
    shape = (3, 13, 17)
    mask, marker = ref.random_raster(shape, dtype, 1), ref.random_raster(shape, dtype, 2)
    valid = ref.cut_plane(13, 17, 3)
    nodata = -9999 if dtype == np.float32 else None
    for flip in (False, True):
        _both(ref.PLAIN, mask, marker=marker, flip=flip, connectivity=connectivity, valid=valid, nodata=nodata, fill=7)
        _both(ref.FILL, mask, flip=flip, connectivity=connectivity, valid=valid, nodata=nodata)
        _both(ref.HDOME, mask, flip=flip, connectivity=connectivity, h=1 if dtype != np.float32 else 0.75, valid=valid, nodata=nodata)
        _both(ref.EXTREMA, mask, flip=flip, connectivity=connectivity, valid=valid, nodata=nodata)


@pytest.mark.parametrize("T", (3, 4, 16))
def test_round_counts_of_structured_inputs(T):
    marker, mask = ref.serpentine(10, 11)
    a, b = _both(ref.PLAIN, mask, marker=marker, T=T, connectivity=8)
    assert (a["out"] == mask).all()                                  # the corridor fills, the background rises to its own level
    if T < 10:
        assert b["rounds"] > 1
    else:
        assert b["rounds"] == 2                                      # one tile: solved in the first round, confirmed in the second
    same = ref.run(ref.PLAIN, mask, marker=mask, solver=("jacobi", T))
    assert same["rounds"] == 1 and (same["out"] == mask).all()       # a marker equal to the mask: nothing to do
    cut = ref.run(ref.PLAIN, mask, marker=marker, solver=("jacobi", 3), max_rounds=1)
    assert not cut["converged"] and cut["rounds"] == 1
    assert (cut["out"] >= np.minimum(marker, mask)).all() and (cut["out"] <= a["out"]).all() and (cut["out"] != a["out"]).any()


@pytest.mark.parametrize("connectivity", (4, 8))
def test_binary_inputs_equal_scipy_binary_propagation(connectivity):
    rng = np.random.default_rng(5)
    mask = (rng.random((23, 29)) < 0.6)
    seed = (rng.random((23, 29)) < 0.02) & mask
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    want = ndimage.binary_propagation(seed, structure=structure, mask=mask)
    for dtype in DTYPES:
        a, _ = _both(ref.PLAIN, mask.astype(dtype), marker=seed.astype(dtype), connectivity=connectivity)
        assert (a["out"] == want.astype(dtype)).all(), dtype


@pytest.mark.parametrize("connectivity", (4, 8))
def test_erosion_is_the_negated_dilation_of_negated_inputs(connectivity):
    rng = np.random.default_rng(6)
    mask = rng.integers(-50, 50, size=(12, 15)).astype(np.int32)
    marker = (mask + rng.integers(0, 30, size=mask.shape)).astype(np.int32)
    ero, _ = _both(ref.PLAIN, mask, marker=marker, flip=True, connectivity=connectivity)
    dil, _ = _both(ref.PLAIN, -mask, marker=-marker, flip=False, connectivity=connectivity)
    assert (ero["out"] == -dil["out"]).all() and (ero["out"] >= mask).all() and (ero["out"] <= marker).all()


def _cone_with_pit():
    y, x = np.mgrid[0:21, 0:21]
    cone = (np.maximum(abs(y - 10), abs(x - 10))).astype(np.float32)  # a square funnel: 0 at the centre, 10 at the edge
    z = np.float32(10) - cone                                        # ... turned into a hill
    z[8:13, 8:13] = np.float32(3.5)                                  # a flat-bottomed pit in its top; the rim around it stands at 7
    z[10, 10] = np.float32(1.25)
    return z


def test_fill_sinks_of_a_cone_with_a_pit_gives_the_spill_level():
    z = _cone_with_pit()
    a, _ = _both(ref.FILL, z, flip=True)
    want = z.copy()
    want[8:13, 8:13] = np.float32(7)
    assert a["out"].tobytes() == want.tobytes()
    assert a["residue"].max() == np.float32(5.75) and (a["residue"] > 0).sum() == 25
    # a ramp of 1/8 per column moves the spill level with the pit: the rim now spills at its lowest pixel, column 7, three
    # columns from the centre, and the depth there changes by those 3/8 alone, whatever the ramp's offset (exact: dyadic values)
    for offset in (0.0, 100.0):
        ramp = z + (np.mgrid[0:21, 0:21][1] * np.float32(0.125) + np.float32(offset)).astype(np.float32)
        b, _ = _both(ref.FILL, ramp, flip=True)
        assert (b["residue"] > 0).sum() == 25 and b["residue"][10, 10] == np.float32(5.75) - np.float32(0.375)
    # the inverted raster has a dome there; fill_sinks(invert=True) levels it
    c, _ = _both(ref.FILL, -z, flip=False)
    assert c["out"].tobytes() == (-want).tobytes() and c["residue"].tobytes() == a["residue"].tobytes()


def test_idempotence_and_monotonicity_in_the_marker():
    for dtype in DTYPES:
        mask, marker = ref.random_raster((14, 18), dtype, 11), ref.random_raster((14, 18), dtype, 12)
        if dtype == np.float32:
            mask, marker = np.nan_to_num(mask, nan=0.5, posinf=3.0, neginf=-3.0), np.nan_to_num(marker, nan=0.25)
        r1 = ref.reconstruct(marker, mask)["out"]
        assert ref.reconstruct(r1, mask)["out"].tobytes() == r1.tobytes()
        higher = from_k(np.maximum(ref.keys(marker), ref.keys(ref.random_raster((14, 18), dtype, 13))), dtype)
        if dtype == np.float32:
            higher = np.nan_to_num(higher, nan=0.25)
        r2 = ref.reconstruct(higher, mask)["out"]
        assert (ref.keys(r2) >= ref.keys(r1)).all()


def from_k(k, dtype):
    return ref.from_keys(k, dtype)


def test_h_dome_residue_grows_with_h_and_extrema_mark_plateaus():
    z = _cone_with_pit()
    prev = None
    for h in (0.5, 1.0, 2.5, 20.0):
        d = ref.h_dome(z, h)["residue"]
        assert d.min() >= 0 and d.max() <= np.float32(h)
        assert prev is None or (d >= prev).all()
        prev = d
    # the rim at 7 is the one regional maximum (a ring plateau), the pit's centre the one interior minimum
    mx = ref.regional_extrema(z, "max")["extrema"]
    assert mx.sum() == (z == 7).sum() - 0 and (mx == (z == 7)).all()
    mn = ref.regional_extrema(z, "min")["extrema"]
    assert mn[10, 10] == 1 and mn[8:13, 8:13].sum() == 1 and (mn == ((z == 0) | (z == np.float32(1.25)))).all()
    # the key - 1 marker saturates: a plateau at the lowest value of an integer type has nothing to stand above
    assert ref.regional_extrema(np.zeros((3, 3), np.uint8), "max")["extrema"].sum() == 0
    assert ref.regional_extrema(np.ones((3, 3), np.uint8), "max")["extrema"].sum() == 9
    lo, hi = np.full((3, 3), -(1 << 31), np.int32), np.full((3, 3), (1 << 31) - 1, np.int32)
    assert ref.regional_extrema(lo, "max")["extrema"].sum() == 0 and ref.regional_extrema(hi, "min")["extrema"].sum() == 0
    assert ref.regional_extrema(lo, "min")["extrema"].sum() == 9 and ref.regional_extrema(hi, "max")["extrema"].sum() == 9
    # uint8 255 is a minimum like any other: the complement is taken on the 32-bit key, so its key is 0xffffff00, not 0
    assert ref.regional_extrema(np.full((3, 3), 255, np.uint8), "min")["extrema"].sum() == 9


def test_the_random_int32_rasters_reach_both_ends_of_the_range():
    for seed in (100, 103, 105, 106):
        a = ref.random_raster((13, 17), np.int32, seed)
        assert (a == -(1 << 31)).any() and (a == (1 << 31) - 1).any() and (a == 500_000_000).any()


def test_key_maps_round_trip_and_keep_the_order():
    f = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], dtype=np.float32)
    i = np.array([-(1 << 31), -7, -1, 0, 1, (1 << 31) - 1], dtype=np.int32)
    u = np.array([0, 1, 127, 128, 255], dtype=np.uint8)
    for a in (f, i, u):
        for to_k, back in ((ref.keys, ref.from_keys), (rc.raster_keys, rc.raster_from_keys)):
            k = to_k(a)
            assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()
            assert back(k, a.dtype).tobytes() == a.tobytes()
        assert (ref.keys(a) == rc.raster_keys(a)).all()
    assert ref.keys(f)[4] - ref.keys(f)[3] == 1                       # -0.0 directly below 0.0
    nan = np.array([np.nan], dtype=np.float32)
    assert ref.from_keys(ref.keys(nan), np.float32).tobytes() == nan.tobytes()
    with pytest.raises(InsarError, match="raster_keys"):
        rc.raster_keys(np.zeros(3, np.float64))


def test_queries_and_the_c_side_refusals():
    T = rc.reconstruct_tile()
    assert T == 64
    one, three = rc.scratch_bytes(T + 5, T + 3), rc.scratch_bytes(T + 5, T + 3, 3)
    assert one % 16 == 0 and three > one >= 3 * 4 * (T + 5) * (T + 3) + 8 * (rc.MAX_ROUNDS + 1)
    with pytest.raises(InsarError, match="insar_reconstruct_bytes"):
        rc.scratch_bytes(0, 5)
    with pytest.raises(InsarError, match="2\\^31"):
        rc.scratch_bytes(1 << 16, 1 << 15)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf) % 16)
    F32 = _lib.ZONAL_F32
    with pytest.raises(InsarError, match="connectivity 6"):
        _lib.call("insar_reconstruct_prepare", None, p, F32, 1, 4, 4, _lib.RECONSTRUCT_FILL, 1, 6, 0.0, 1, 0, 0.0, None, p, None)
    with pytest.raises(InsarError, match="marker"):
        _lib.call("insar_reconstruct_prepare", None, p, F32, 1, 4, 4, _lib.RECONSTRUCT_PLAIN, 0, 8, 0.0, 1, 0, 0.0, None, p, None)
    with pytest.raises(InsarError, match="positive and finite"):
        _lib.call("insar_reconstruct_prepare", None, p, F32, 1, 4, 4, _lib.RECONSTRUCT_HDOME, 0, 8, 0.0, 1, 0, 0.0, None, p, None)
    with pytest.raises(InsarError, match="max_rounds 0"):
        _lib.call("insar_reconstruct_prepare", None, p, F32, 1, 4, 4, _lib.RECONSTRUCT_FILL, 1, 8, 0.0, 0, 0, 0.0, None, p, None)
    with pytest.raises(InsarError, match="rounds"):
        _lib.call("insar_reconstruct_rounds", 1, 4, 4, 8, 65530, 8, p, None)
    with pytest.raises(InsarError, match="no output"):
        _lib.call("insar_reconstruct_finish", None, p, F32, 1, 4, 4, _lib.RECONSTRUCT_FILL, 1, 0, 0.0, None, 1, 0, p, None, None, None, None, None)
    with pytest.raises(InsarError, match="the mask or the marker itself"):
        _lib.call("insar_reconstruct_finish", None, p, F32, 1, 4, 4, _lib.RECONSTRUCT_FILL, 1, 0, 0.0, None, 1, 0, p, p, None, None, None, None)


def test_argument_refusals_that_need_no_device():
    z = torch.zeros(6, 7)
    cases = [
        (lambda: rc.reconstruct_raster(z, z, method="closing"), "reconstruct_raster: method"),
        (lambda: rc.reconstruct_raster(z.to(torch.int32), z), "reconstruct_raster: marker"),
        (lambda: rc.reconstruct_raster(torch.zeros(6, 8), z), "reconstruct_raster: marker"),
        (lambda: rc.reconstruct_raster(np.zeros((6, 7)), z), "reconstruct_raster: marker"),
        (lambda: rc.reconstruct_raster(z, z.double()), "reconstruct_raster: mask"),
        (lambda: rc.reconstruct_raster(z, z, connectivity=6), "reconstruct_raster: connectivity"),
        (lambda: rc.reconstruct_raster(z, z, fill=3), "reconstruct_raster: fill"),
        (lambda: rc.reconstruct_raster(z, z, max_rounds=0), "reconstruct_raster: max_rounds"),
        (lambda: rc.reconstruct_raster(z, z, max_rounds=1 << 16), "reconstruct_raster: max_rounds"),
        (lambda: rc.reconstruct_raster(z, z, return_info=1), "reconstruct_raster: return_info"),
        (lambda: rc.reconstruct_raster(z, z, nodata=float("nan")), "reconstruct_raster: nodata"),
        (lambda: rc.reconstruct_raster(z, z, valid=torch.ones(6, 7)), "reconstruct_raster: valid"),
        (lambda: rc.reconstruct_raster(z, z, out=torch.zeros(6, 7, dtype=torch.int32)), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(z, z, out=z), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(z, z, scratch=object()), "reconstruct_raster: scratch"),
        (lambda: rc.reconstruct_raster(z, z), "reconstruct_raster: mask must be a ROCm tensor"),
        (lambda: rc.fill_sinks(z, invert=1), "fill_sinks: invert"),
        (lambda: rc.fill_sinks(z.to(torch.uint8), fill=256), "fill_sinks: fill"),
        (lambda: rc.fill_sinks(z.to(torch.uint8), nodata=1.5), "fill_sinks: nodata"),
        (lambda: rc.fill_sinks(z[:, ::2]), "fill_sinks: raster"),
        (lambda: rc.fill_sinks(z), "fill_sinks: raster must be a ROCm tensor"),
        (lambda: rc.h_dome(z, 0.0), "h_dome: h"),
        (lambda: rc.h_dome(z, float("inf")), "h_dome: h"),
        (lambda: rc.h_dome(z, 1e-60), "h_dome: h"),
        (lambda: rc.h_dome(z.to(torch.int32), 0.5), "h_dome: h"),
        (lambda: rc.h_dome(z, True), "h_dome: h"),
        (lambda: rc.h_dome(z.to(torch.uint8), 3, out=torch.zeros(6, 7, dtype=torch.uint8)), "h_dome: out"),
        (lambda: rc.regional_extrema(z, "saddle"), "regional_extrema: kind"),
        (lambda: rc.regional_extrema(z, out=torch.zeros(6, 7)), "regional_extrema: out"),
        (lambda: rc.regional_extrema(torch.zeros(2, 2, 6, 7)), "regional_extrema: raster"),
    ]
    for fn, text in cases:
        with pytest.raises(InsarError) as e:
            fn()
        assert text in str(e.value), (text, str(e.value))


def test_exports_and_abi():
    import insar_unet_ca_amd as iu
    for name in ("ReconstructScratch", "reconstruct_raster", "fill_sinks", "h_dome", "regional_extrema", "reconstruct_tile"):
        assert name in iu.__all__ and getattr(iu, name) is getattr(rc, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8          # additive: the ABI version stays

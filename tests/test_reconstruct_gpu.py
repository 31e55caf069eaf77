"""GPU: grey-scale reconstruction (insar_unet_ca_amd/reconstruct.py on csrc/reconstruct.hip) against the restatements of
tests/reconstruct_ref.py (held to each other and to known answers in tests/test_reconstruct_host.py). Every comparison is bitwise
and covers every pixel of every output; the number of rounds has to be that of the tile-Jacobi restatement at the tile edge T the
library reports.

Shapes: 1 x 1, 1 x 37, 5 x 7, T x T, (T + 1) x (T - 1), (2T + 2) x (3T + 1) and three planes of (T + 5) x (T + 3) with one shared
`valid`."""
import functools

import numpy as np
import pytest
import torch

from insar_unet_ca_amd._lib import InsarError
from tests import reconstruct_ref as ref

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.uint8, np.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _T():
    from insar_unet_ca_amd import reconstruct as rc
    return rc.reconstruct_tile()


def _shapes():
    T = _T()
    return ((1, 1), (1, 37), (5, 7), (T, T), (T + 1, T - 1), (2 * T + 2, 3 * T + 1), (3, T + 5, T + 3))


@functools.lru_cache(maxsize=None)
def _inputs(i, dtype):
    shape = _shapes()[i]
    mask, marker = ref.random_raster(shape, dtype, 100 + i), ref.random_raster(shape, dtype, 200 + i)
    valid = ref.cut_plane(shape[-2], shape[-1], 300 + i)
    for a in (mask, marker, valid):
        a.setflags(write=False)
    return mask, marker, valid


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)        # a copy: the cached arrays are read-only


def _same(got, want, what):
    assert isinstance(got, torch.Tensor) and got.is_cuda, what
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes(), \
        f"{what}: {np.count_nonzero(g.view(np.uint8) != want.view(np.uint8))} bytes differ"


def _info(info, want, what):
    assert info["rounds"] == want["rounds"] and info["converged"] == want["converged"], (what, info, want["rounds"], want["converged"])
    assert info["active_tile_rounds"] == want["active_tile_rounds"], (what, info, want["active_tile_rounds"])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("i", range(7))
def test_every_entry_is_bitwise_the_restatement(dev, i, dtype):
    from insar_unet_ca_amd import reconstruct as rc
    mask, marker, valid = _inputs(i, dtype)
    nodata = -9999.0 if dtype == np.float32 else (31 if dtype == np.uint8 else 500_000_000)
    jac = ("jacobi", _T())
    g, f, v = _t(mask, dev), _t(marker, dev), _t(valid, dev)
    what = f"{mask.shape} {np.dtype(dtype).name}"
    for method, conn, use_valid in (("dilation", 8, True), ("erosion", 4, True), ("dilation", 4, False), ("erosion", 8, False)):
        kw = dict(connectivity=conn, valid=valid if use_valid else None, nodata=nodata if use_valid else None)
        fill = 0 if dtype == np.float32 else 7
        want = ref.reconstruct(marker, mask, method, fill=fill, solver=jac, **kw)
        out, ok, info = rc.reconstruct_raster(f, g, method=method, connectivity=conn, valid=v if use_valid else None,
                                              nodata=kw["nodata"], fill=fill, return_valid=True, return_info=True)
        _same(out, want["out"], f"reconstruct {method} {conn} {what}")
        _same(ok, want["valid"], f"reconstruct valid {what}")
        _info(info, want, f"reconstruct {method} {conn} {what}")
    if i >= 3:                                                       # the sequential flood itself, where there are tiles to get wrong
        flood = ref.reconstruct(marker, mask, "dilation", connectivity=8, valid=valid, nodata=nodata)
        _same(rc.reconstruct_raster(f, g, valid=v, nodata=nodata), flood["out"], f"flood {what}")
    for invert in (False, True):
        want = ref.fill_sinks(mask, invert, connectivity=8, valid=valid, nodata=nodata, solver=jac)
        filled, depth, ok, info = rc.fill_sinks(g, invert=invert, valid=v, nodata=nodata, return_depth=True, return_valid=True,
                                                return_info=True)
        _same(filled, want["out"], f"fill_sinks {invert} {what}")
        _same(depth, want["residue"], f"fill_sinks depth {invert} {what}")
        _same(ok, want["valid"], f"fill_sinks valid {what}")
        _info(info, want, f"fill_sinks {invert} {what}")
        h = 0.75 if dtype == np.float32 else (40 if dtype == np.uint8 else 900_000_000)
        want = ref.h_dome(mask, h, invert, connectivity=4, valid=valid, solver=jac)
        res, info = rc.h_dome(g, h, invert=invert, connectivity=4, valid=v, return_info=True)
        _same(res, want["residue"], f"h_dome {invert} {what}")
        _info(info, want, f"h_dome {invert} {what}")
        kind = "min" if invert else "max"
        want = ref.regional_extrema(mask, kind, connectivity=8, nodata=nodata, solver=jac)
        ext, info = rc.regional_extrema(g, kind, nodata=nodata, return_info=True)
        _same(ext, want["extrema"], f"regional_extrema {kind} {what}")
        _info(info, want, f"regional_extrema {kind} {what}")


@functools.lru_cache(maxsize=None)
def _serpentine():
    T = _T()
    marker, mask = ref.serpentine(2 * T + 2, 2 * T + 2)
    return marker, mask, ref.reconstruct(marker, mask, solver=("jacobi", T))


def test_a_serpentine_corridor_needs_many_rounds(dev):
    from insar_unet_ca_amd import reconstruct as rc
    marker, mask, want = _serpentine()
    assert (want["out"] == mask).all() and want["rounds"] > 1
    out, info = rc.reconstruct_raster(_t(marker, dev), _t(mask, dev), return_info=True)
    _same(out, want["out"], "serpentine")
    _info(info, want, "serpentine")
    assert info["rounds"] > 1 and info["converged"]


def test_a_cut_off_propagation_says_so(dev):
    from insar_unet_ca_amd import reconstruct as rc
    marker, mask, full = _serpentine()
    want = ref.reconstruct(marker, mask, solver=("jacobi", _T()), max_rounds=1)
    out, info = rc.reconstruct_raster(_t(marker, dev), _t(mask, dev), max_rounds=1, return_info=True)
    assert info["converged"] is False and info["rounds"] == 1
    _same(out, want["out"], "serpentine, one round")
    o = out.cpu().numpy()
    assert (o >= np.minimum(marker, mask)).all() and (o <= full["out"]).all() and (o != full["out"]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_marker_equal_to_the_mask_returns_it_in_one_round(dev, dtype):
    from insar_unet_ca_amd import reconstruct as rc
    mask = np.nan_to_num(ref.random_raster(_shapes()[4], dtype, 17), nan=1.0, posinf=2.0, neginf=-2.0)
    g = _t(mask, dev)
    for method in ("dilation", "erosion"):
        out, info = rc.reconstruct_raster(g.clone(), g, method=method, return_info=True)
        _same(out, mask, method)
        assert info["rounds"] == 1 and info["converged"]


def test_plateaus_straddling_a_tile_corner(dev):
    from insar_unet_ca_amd import reconstruct as rc
    T = _T()
    z = np.full((T + 6, T + 6), 5, dtype=np.uint8)
    z[T - 2:T + 2, T - 2:T + 2] = 9                                  # a plateau over the corner where four tiles meet
    z[T + 2, T + 2] = 10                                             # touches it diagonally: a higher neighbour at connectivity 8 only
    z[3:5, T - 1:T + 1] = 2                                          # a low plateau over a tile edge
    z[T - 1:T + 1, 3] = 7                                            # a high one over the other
    for conn in (4, 8):
        for kind in ("max", "min"):
            want = ref.regional_extrema(z, kind, connectivity=conn, solver=("jacobi", T))
            got, info = rc.regional_extrema(_t(z, dev), kind, connectivity=conn, return_info=True)
            _same(got, want["extrema"], f"{kind} {conn}")
            _info(info, want, f"{kind} {conn}")
        mx = rc.regional_extrema(_t(z, dev), "max", connectivity=conn).cpu().numpy()
        assert mx[T + 2, T + 2] == 1 and (mx[T - 1:T + 1, 3] == 1).all()
        assert (mx[T - 2:T + 2, T - 2:T + 2] == (1 if conn == 4 else 0)).all()
        assert mx.sum() == 1 + 2 + (16 if conn == 4 else 0)
    mn = rc.regional_extrema(_t(z, dev), "min").cpu().numpy()
    assert (mn == (z == 2)).all()                                    # the background at 5 has lower neighbours


def test_int32_rasters_at_both_ends_of_the_range(dev):
    """INT32_MIN has the key 0 of a barrier under dilation, INT32_MAX under erosion; the key - 1 marker saturates there, and a
    depth of 2^32 - 1 saturates at 2^31 - 1."""
    from insar_unet_ca_amd import reconstruct as rc
    T = _T()
    lo, hi = -(1 << 31), (1 << 31) - 1
    z = np.zeros((T + 4, T + 4), dtype=np.int32)
    z[T - 3:T + 3, T - 3:T + 3] = hi                                 # a wall of INT32_MAX over the corner where four tiles meet ...
    z[T - 1:T + 1, T - 1:T + 1] = lo                                 # ... round a pit of INT32_MIN
    z[2:4, T - 1:T + 1] = lo                                         # a low plateau and a high one over tile edges
    z[T - 1:T + 1, 2:4] = hi
    g = _t(z, dev)
    jac = ("jacobi", T)
    for invert in (False, True):
        want = ref.fill_sinks(z, invert, solver=jac)
        filled, depth, info = rc.fill_sinks(g, invert=invert, return_depth=True, return_info=True)
        _same(filled, want["out"], f"fill_sinks {invert}")
        _same(depth, want["residue"], f"depth {invert}")
        _info(info, want, f"fill_sinks {invert}")
        for h in (1, hi):
            want = ref.h_dome(z, h, invert, solver=jac)
            _same(rc.h_dome(g, h, invert=invert), want["residue"], f"h_dome {h} {invert}")
        for conn in (4, 8):
            kind = "min" if invert else "max"
            want = ref.regional_extrema(z, kind, connectivity=conn, solver=jac)
            _same(rc.regional_extrema(g, kind, connectivity=conn), want["extrema"], f"{kind} {conn}")
        for method in ("dilation", "erosion"):
            marker = np.where(z == (hi if invert else lo), z, 0).astype(np.int32)
            want = ref.reconstruct(marker, z, method, solver=jac)
            _same(rc.reconstruct_raster(_t(marker, dev), g, method=method), want["out"], f"{method} {invert}")
    d = rc.fill_sinks(g, return_depth=True)[1].cpu().numpy()
    assert (d[T - 1:T + 1, T - 1:T + 1] == hi).all()                 # INT32_MAX - INT32_MIN = 2^32 - 1 saturates
    assert (d[2:4, T - 1:T + 1] == hi).all() and (d > 0).sum() == 8  # 0 - INT32_MIN = 2^31 does too
    assert (rc.regional_extrema(g, "max").cpu().numpy() == (z == hi)).all()
    assert (rc.regional_extrema(g, "min").cpu().numpy() == (z == lo)).all()
    # a whole raster at the end of the order has the key 0 and nothing to stand above: the documented limit
    flat_lo, flat_hi = torch.full((3, T + 1), lo, dtype=torch.int32, device=dev), torch.full((3, T + 1), hi, dtype=torch.int32, device=dev)
    assert int(rc.regional_extrema(flat_lo, "max").sum()) == 0 and int(rc.regional_extrema(flat_hi, "min").sum()) == 0
    assert int(rc.regional_extrema(flat_lo, "min").sum()) == 3 * (T + 1) and int(rc.regional_extrema(flat_hi, "max").sum()) == 3 * (T + 1)
    _same(rc.fill_sinks(flat_lo), flat_lo.cpu().numpy(), "flat INT32_MIN")
    _same(rc.fill_sinks(flat_hi), flat_hi.cpu().numpy(), "flat INT32_MAX")


def test_fill_sinks_finds_the_closed_pits_and_their_depths(dev):
    import insar_unet_ca_amd as iu
    T = _T()
    H, W = T + 8, T + 6
    yy, xx = np.mgrid[0:H, 0:W]
    z = (10 * yy + 3 * xx).astype(np.int32)                          # a tilted plane: everything drains to the top-left
    z[20:23, 20:23] -= 500                                           # A: a closed pit; it spills over its lowest rim pixel (19, 19)
    z[21, 21] -= 200
    z[0:2, 30:33] -= 500                                             # B: cut by the raster's edge: it drains there, nothing fills
    z[T - 2:T + 1, T - 3:T] -= 500                                   # C: its centre is invalid, so its pixels are outlets: unfilled
    z[50, 10] -= 50                                                  # D: a closed one-pixel pit
    valid = np.ones((H, W), dtype=np.uint8)
    valid[T - 1, T - 2] = 0
    want = ref.fill_sinks(z, valid=valid, solver=("jacobi", T))
    filled, depth, info = iu.fill_sinks(_t(z, dev), valid=_t(valid, dev), return_depth=True, return_info=True)
    _same(filled, want["out"], "filled")
    _same(depth, want["residue"], "depth")
    _info(info, want, "pits")
    d = depth.cpu().numpy()
    expect = np.zeros((H, W), dtype=np.int32)
    expect[20:23, 20:23] = (10 * 19 + 3 * 19) - z[20:23, 20:23]      # the spill level minus the pit
    expect[50, 10] = (10 * 49 + 3 * 9) - z[50, 10]
    assert (d == expect).all() and d[21, 21] == 674 and d[50, 10] == 37
    det = iu.label_regions((depth > 0).to(torch.uint8))
    assert det["count"] == 2 and det["regions"]["area"].tolist() == [9, 1]
    st = iu.region_stats(det["labels"], depth, count=det["count"])
    assert st["max"].tolist() == [674.0, 37.0] and st["min"].tolist() == [487.0 - 13.0 * 2, 37.0]
    assert st["argmax"].tolist() == [[21, 21], [50, 10]]


def test_h_dome_at_both_signs_grows_with_h(dev):
    from insar_unet_ca_amd import reconstruct as rc
    mask = np.nan_to_num(ref.random_raster((_T() + 5, _T() + 3), np.float32, 23), nan=0.5, posinf=4.0, neginf=-4.0)
    g = _t(mask, dev)
    for invert in (False, True):
        prev = None
        for h in (0.25, 0.5, 1.75, 100.0):
            want = ref.h_dome(mask, h, invert, solver=("jacobi", _T()))
            res = rc.h_dome(g, h, invert=invert)
            _same(res, want["residue"], f"h={h} invert={invert}")
            r = res.cpu().numpy()
            assert r.min() >= 0 and r.max() <= np.float32(h) and (prev is None or (r >= prev).all())
            prev = r


def test_scratch_reuse_and_repeated_calls_change_nothing(dev):
    from insar_unet_ca_amd import reconstruct as rc
    mask, marker, valid = _inputs(6, np.float32)
    g, f, v = _t(mask, dev), _t(marker, dev), _t(valid, dev)
    scratch = rc.ReconstructScratch(mask.shape[1], mask.shape[2], 3, dev)
    first = rc.reconstruct_raster(f, g, valid=v, return_info=True)
    out = torch.empty_like(g)
    for _ in range(2):
        again = rc.reconstruct_raster(f, g, valid=v, return_info=True, scratch=scratch, out=out)
        assert again[0] is out and again[1] == first[1]
        _same(out, first[0].cpu().numpy(), "scratch / out")
    filled = rc.fill_sinks(g, valid=v, scratch=scratch)              # another entry on the same scratch, then the first again
    _same(rc.fill_sinks(g, valid=v), filled.cpu().numpy(), "fill_sinks scratch")
    _same(rc.reconstruct_raster(f, g, valid=v, scratch=scratch), first[0].cpu().numpy(), "after another entry")


def test_refusals_on_the_device(dev):
    from insar_unet_ca_amd import reconstruct as rc
    g = torch.zeros(9, 11, device=dev)
    f = torch.zeros(9, 11, device=dev)
    big = torch.zeros(2, 9, 11, device=dev)
    cases = [
        (lambda: rc.reconstruct_raster(f, g, out=g), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(f, g, out=f), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(f, big[0], out=big[0]), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(f, g, out=torch.zeros(9, 11)), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(f, g, out=torch.zeros(9, 12, device=dev)), "reconstruct_raster: out"),
        (lambda: rc.reconstruct_raster(f.cpu(), g), "reconstruct_raster: marker must be a ROCm tensor"),
        (lambda: rc.reconstruct_raster(f, g, valid=torch.ones(9, 11, dtype=torch.uint8)), "reconstruct_raster: valid must be a ROCm tensor"),
        (lambda: rc.fill_sinks(g, scratch=rc.ReconstructScratch(9, 12, 1, dev)), "fill_sinks: scratch of 9 x 12, planes=1"),
        (lambda: rc.fill_sinks(big, scratch=rc.ReconstructScratch(9, 11, 1, dev)), "fill_sinks: scratch of 9 x 11, planes=1"),
        (lambda: rc.h_dome(g, 0.5, scratch=torch.zeros(4, device=dev)), "h_dome: scratch must be a ReconstructScratch"),
        (lambda: rc.regional_extrema(g, out=g.to(torch.uint8)[:, :10]), "regional_extrema: out"),
    ]
    for fn, text in cases:
        with pytest.raises(InsarError) as e:
            fn()
        assert text in str(e.value), (text, str(e.value))

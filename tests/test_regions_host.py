"""CPU-only: the host side of the regions stage (insar_unet_ca_amd/regions.py on csrc/regions.hip): the scipy oracle of
tests/regions_ref.py pinned against a brute-force flood fill, the scratch-size query, the argument checks of every new
entry point (they run before anything touches a device), the exports and the refusal of host tensors."""
import ctypes

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib, regions
from insar_unet_ca_amd._lib import InsarError
from tests.regions_ref import quantise_conf, regions_oracle

FAKE = 4096       # a non-null, 16-byte aligned "pointer": the checks below fail before anything dereferences it
ENTRY_POINTS = ("insar_regions_scratch_bytes", "insar_regions_tiles", "insar_regions_merge", "insar_regions_flatten",
                "insar_regions_number", "insar_regions_relabel")


# ---- the oracle against a brute-force flood fill -------------------------------------------------------------------------
def flood_fill(m, connectivity, min_area):
    """Components in ascending order of their first row-major pixel: scanning in that order, every unlabelled foreground
    pixel met is the root of a new component. -> (labels, [(root, cls, pixels)])."""
    H, W = m.shape
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    seen = np.zeros((H, W), dtype=bool)
    comps = []
    for y in range(H):
        for x in range(W):
            if m[y, x] == 0 or seen[y, x]:
                continue
            stack, pix = [(y, x)], []
            seen[y, x] = True
            while stack:
                cy, cx = stack.pop()
                pix.append((cy, cx))
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and not seen[ny, nx] and m[ny, nx] == m[y, x]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            if len(pix) >= min_area:
                comps.append((y * W + x, int(m[y, x]), pix))
    labels = np.zeros((H, W), dtype=np.int32)
    for k, (_, _, pix) in enumerate(comps):
        for py, px in pix:
            labels[py, px] = k + 1
    return labels, comps


@pytest.mark.parametrize("connectivity", [4, 8])
def test_oracle_matches_flood_fill(connectivity):
    rng = np.random.default_rng(100 + connectivity)
    for case in range(100):                                     # 100 masks per connectivity, two classes, <= 40 x 40
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        fill = rng.choice([0.2, 0.45, 0.6, 0.85])
        m = (rng.random((H, W)) < fill).astype(np.uint8) * rng.integers(1, 3, size=(H, W)).astype(np.uint8)
        min_area = int(rng.choice([1, 1, 2, 5]))
        conf = rng.random((H, W)).astype(np.float32) if case % 3 == 0 else None
        min_conf = 0.3 if conf is not None else 0.0
        got = regions_oracle(m, conf, connectivity=connectivity, min_area=min_area, min_conf=min_conf)
        fg = m if conf is None else np.where(conf >= np.float32(min_conf), m, 0).astype(np.uint8)
        labels, comps = flood_fill(fg, connectivity, min_area)
        assert got["count"] == len(comps)
        assert (got["labels"] == labels).all()
        assert (got["mask"] == np.where(labels > 0, fg, 0)).all()
        r = got["regions"]
        q = quantise_conf(conf) if conf is not None else None
        for k, (root, cls, pix) in enumerate(comps):
            ys, xs = np.array([p[0] for p in pix]), np.array([p[1] for p in pix])
            assert (r["id"][k], r["root"][k], r["cls"][k], r["area"][k]) == (k + 1, root, cls, len(pix))
            assert (r["y0"][k], r["x0"][k], r["y1"][k], r["x1"][k]) == (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
            assert r["cy"][k] == ys.sum() / len(pix) and r["cx"][k] == xs.sum() / len(pix)
            if q is not None:
                assert r["sum_conf"][k] == q[ys, xs].sum()
                assert abs(r["mean_conf"][k] - conf[ys, xs].astype(np.float64).mean()) <= 1e-9


def test_quantise_conf():
    c = np.array([-1.0, 0.0, 2.0 ** -10, 0.125, 0.5, 1.0, 3.0], dtype=np.float32)
    assert quantise_conf(c).tolist() == [0, 0, 1 << 20, 1 << 27, 1 << 29, 1 << 30, 1 << 30]


# ---- the library: exports, the scratch query, argument checks without a GPU -------------------------------------------
def test_regions_symbols_exported():
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    for name in ("label_regions", "detect_scene"):
        assert name in iu.__all__ and callable(getattr(iu, name))
    assert callable(iu.ScenePredictor.detect)
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8          # additive: the ABI version stays


def test_region_record_layout(tmp_path):
    """regions.REGION_DTYPE is the C compiler's InsarRegion."""
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "insar_hip.h")
    fields = [n for n in regions.REGION_DTYPE.names]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("%zu\\n", sizeof(InsarRegion));']
    lines += [f'printf("%zu\\n", offsetof(InsarRegion, {f}));' for f in fields]
    lines.append("return 0;}")
    (tmp_path / "r.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "r"), str(tmp_path / "r.c")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "r")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == regions.REGION_DTYPE.itemsize == 64
    assert out[1:] == [regions.REGION_DTYPE.fields[f][1] for f in fields]


def test_scratch_bytes_query():
    def q(H, W, R):
        return regions.scratch_bytes(H, W, R)

    # two int32 planes (each rounded up to 16 bytes) + one int32 per block of 1024 pixels (rounded up to 16 bytes)
    assert q(4096, 4096, 65536) == (2 * 4 * 4096 * 4096 + 4 * 16384, 64 * 65537)
    assert q(200, 264, 10) == (2 * 4 * 52800 + 208, 64 * 11)            # 52 blocks
    assert q(1, 1, 1) == (2 * 16 + 16, 128)
    assert q(1, 300, 1)[0] == 2 * 1200 + 16
    s, t = q(46340, 46340, 1)                                          # the largest square below 2^31 pixels
    assert s >= 8 * 46340 * 46340 and s % 16 == 0
    for args in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (65536, 32768, 1)):           # the last: exactly 2^31 pixels
        with pytest.raises(InsarError, match=r"\(-1001\)"):
            q(*args)
    with pytest.raises(InsarError, match="max_regions"):
        q(5, 5, 0)
    a = ctypes.c_int64(0)
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_regions_scratch_bytes", 5, 5, 1, None, ctypes.byref(a))
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_regions_scratch_bytes", 5, 5, 1, ctypes.byref(a), None)


def _shape_cases(fn):
    for H, W in ((0, 264), (200, 0), (-3, 264), (65536, 32768), (46341, 46341)):
        with pytest.raises(InsarError, match=r"\(-1001\)"):
            fn(H=H, W=W)


def test_regions_tiles_validates_without_a_gpu():
    ok = dict(mask=FAKE, conf=FAKE, min_conf=0.5, H=200, W=264, conn=8, scratch=FAKE)

    def tiles(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_regions_tiles", a["mask"], a["conf"], a["min_conf"], a["H"], a["W"], a["conn"], a["scratch"], None)

    for name in ("mask", "scratch"):
        with pytest.raises(InsarError, match="null"):
            tiles(**{name: None})
    _shape_cases(tiles)
    for conn in (0, 1, 6, 9, -8):
        with pytest.raises(InsarError, match="connectivity"):
            tiles(conn=conn)
    with pytest.raises(InsarError, match="aligned"):
        tiles(scratch=FAKE + 8)
    with pytest.raises(InsarError, match="aligned"):
        tiles(conf=FAKE + 2)
    with pytest.raises(InsarError, match=r"\(-1005\)"):                 # INSAR_E_ARG, not a launch failure
        tiles(mask=None)


def test_regions_merge_and_flatten_validate_without_a_gpu():
    ok = dict(mask=FAKE, H=200, W=264, conn=4, scratch=FAKE)

    def merge(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_regions_merge", a["mask"], a["H"], a["W"], a["conn"], a["scratch"], None)

    def flatten(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_regions_flatten", a["H"], a["W"], a["scratch"], None)

    for name in ("mask", "scratch"):
        with pytest.raises(InsarError, match="null"):
            merge(**{name: None})
    with pytest.raises(InsarError, match="null"):
        flatten(scratch=None)
    for fn in (merge, flatten):
        _shape_cases(fn)
        with pytest.raises(InsarError, match="aligned"):
            fn(scratch=FAKE + 4)
    for conn in (0, 5, 16):
        with pytest.raises(InsarError, match="connectivity"):
            merge(conn=conn)


def test_regions_number_and_relabel_validate_without_a_gpu():
    ok = dict(mask=FAKE, conf=None, H=200, W=264, min_area=1, R=100, scratch=FAKE, table=FAKE, labels=FAKE, out=FAKE)

    def number(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_regions_number", a["mask"], a["H"], a["W"], a["min_area"], a["R"], a["scratch"], a["table"], None)

    def relabel(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_regions_relabel", a["mask"], a["conf"], a["H"], a["W"], a["R"], a["scratch"], a["table"], a["labels"],
                  a["out"], None)

    for name in ("mask", "scratch", "table"):
        for fn in (number, relabel):
            with pytest.raises(InsarError, match="null"):
                fn(**{name: None})
    for name in ("labels", "out"):
        with pytest.raises(InsarError, match="null"):
            relabel(**{name: None})
    for fn in (number, relabel):
        _shape_cases(fn)
        for R in (0, -1):
            with pytest.raises(InsarError, match="max_regions"):
                fn(R=R)
        with pytest.raises(InsarError, match="aligned"):
            fn(scratch=FAKE + 8)
        with pytest.raises(InsarError, match="aligned"):
            fn(table=FAKE + 8)
    with pytest.raises(InsarError, match="min_area"):
        number(min_area=0)
    with pytest.raises(InsarError, match="aligned"):
        relabel(labels=FAKE + 2)


# ---- the Python interface refuses before any launch -----------------------------------------------------------------------
def test_label_regions_refuses_host_tensors_and_bad_arguments():
    m = torch.zeros(8, 8, dtype=torch.uint8)
    with pytest.raises(InsarError, match="no CPU fallback"):
        iu.label_regions(m)
    with pytest.raises(InsarError, match="torch tensor"):
        iu.label_regions(np.zeros((8, 8), dtype=np.uint8))


def test_argument_checks_of_label_regions():
    """The checks that follow the device check, on a stand-in that claims to live on a device (nothing is launched: every
    case is refused first)."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    def dev(t):
        return t.as_subclass(OnDevice)

    good = dev(torch.zeros(8, 8, dtype=torch.uint8))
    for bad in (dev(torch.zeros(8, 8, dtype=torch.int32)), dev(torch.zeros(2, 8, 8, dtype=torch.uint8)),
                dev(torch.zeros(8, 16, dtype=torch.uint8)[:, ::2])):
        with pytest.raises(InsarError, match="contiguous 2-D uint8"):
            iu.label_regions(bad)
    with pytest.raises(InsarError, match="no CPU fallback"):
        iu.label_regions(good, torch.zeros(8, 8))
    for kw, pat in ((dict(connectivity=6), "connectivity"), (dict(min_area=0), "min_area"), (dict(min_area=2.5), "min_area"),
                    (dict(max_regions=0), "max_regions"), (dict(min_conf=float("nan")), "min_conf")):
        with pytest.raises(InsarError, match=pat):
            iu.label_regions(good, **kw)

"""Host: the helpers the scene tools share (insar_unet_ca_amd/_scene.py): the two integer rules, the tensor checks, the
scratch base class, and the refusals of the tools that used to let a TypeError or ValueError escape. No device is touched."""
import math

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _scene
from insar_unet_ca_amd._lib import InsarError

# value, passes the strict rule, passes the rule that takes integral floats (both within 1..5)
INT_CASES = [(3, True, True), (np.int64(3), True, True), (3.0, False, True), (np.float32(3.0), False, True), (1.5, False, False),
             (True, False, False), (math.nan, False, False), (math.inf, False, False), ("3", False, False), (None, False, False),
             (0, False, False), (6, False, False), (0.0, False, False), (6.0, False, False)]


@pytest.mark.parametrize("v, strict, lenient", INT_CASES, ids=[repr(c[0]) for c in INT_CASES])
def test_check_int_under_both_rules(v, strict, lenient):
    for integral_floats, ok in ((False, strict), (True, lenient)):
        if ok:
            got = _scene.check_int("tool", "n", v, 1, 5, integral_floats=integral_floats)
            assert got == 3 and type(got) is int
        else:
            with pytest.raises(InsarError, match=r"tool: n=.*: an integer in 1\.\.5"):
                _scene.check_int("tool", "n", v, 1, 5, integral_floats=integral_floats)


def test_check_int_without_an_upper_bound_or_a_tool():
    assert _scene.check_int(None, "n", 1 << 80, 1, integral_floats=True) == 1 << 80
    with pytest.raises(InsarError, match=r"^n=0: an integer >= 1$"):
        _scene.check_int(None, "n", 0, 1, integral_floats=False)
    with pytest.raises(InsarError, match="n=0: a positive integer"):
        _scene.check_int("tool", "n", 0, 1, integral_floats=False, expect="a positive integer")
    assert _scene.is_int(3) and _scene.is_int(3.0, integral_floats=True) and not _scene.is_int(3.0) and not _scene.is_int(True)


def test_check_map():
    good = torch.zeros(6, 8, dtype=torch.int32)
    _scene.check_map("tool", "m", good, (torch.uint8, torch.int32))
    _scene.check_map("tool", "m", good[None], (torch.int32,), dims=(2, 3), shape=(6, 8))
    _scene.check_map("tool", "m", torch.zeros(6, 8, dtype=torch.int32, device="meta"), (torch.int32,), shape=(6, 8))
    with pytest.raises(InsarError, match="tool: m must be a torch tensor, got ndarray"):
        _scene.check_map("tool", "m", good.numpy(), (torch.int32,))
    for bad in (good.long(), good[None], good.t(), torch.zeros(6, 16, dtype=torch.int32)[:, ::2]):
        with pytest.raises(InsarError, match="m must be a contiguous 2-D int32 tensor, got"):
            _scene.check_map("tool", "m", bad, (torch.int32,))
    with pytest.raises(InsarError, match=r"m \(6, 9\): expected \(6, 8\) for labels"):
        _scene.check_map("tool", "m", torch.zeros(6, 9, dtype=torch.int32), (torch.int32,), shape=(6, 8))
    # one fault at a time, in the order dtype, rank, contiguity
    kw = dict(dims=(2, 3), one_fault=True)
    for bad, what in ((good.float().t(), "uint8 or int32"), (good.t()[None, None], r"2-D \[H, W\] or 3-D \[B, H, W\]"), (good.t(), "contiguous")):
        with pytest.raises(InsarError, match=f"m must be {what}, got"):
            _scene.check_map("tool", "m", bad, (torch.uint8, torch.int32), **kw)


def test_check_on_device():
    cpu, meta = torch.zeros(2, 2), torch.zeros(2, 2, device="meta")
    for bad in (cpu, meta):
        with pytest.raises(InsarError, match=r"tool: m must be a ROCm tensor \(no CPU fallback\)"):
            _scene.check_on_device("tool", "m", bad)
    with pytest.raises(InsarError, match="torch tensor"):
        _scene.check_on_device("tool", "m", cpu.numpy())

    class OnDevice(torch.Tensor):
        is_cuda = True

    here = cpu.as_subclass(OnDevice)
    _scene.check_on_device("tool", "m", here)
    _scene.check_on_device("tool", "m", here, like=cpu)
    with pytest.raises(InsarError, match="m must be a ROCm tensor on meta, not cpu"):
        _scene.check_on_device("tool", "m", here, like=meta)


class Toy(_scene.Scratch):
    """Constant byte counts on the host: nothing is asked of the library or of a device."""
    KEY, SHOW, DEVICE_AT = ("H", "W", "cap"), "{} x {}, cap={}", 2

    def __init__(self, H, W, device, cap=4):
        if cap > 100:
            raise InsarError("cap above 100")
        super().__init__((H, W, cap), device, scratch=32, table=16)


class Other(_scene.Scratch):
    KEY = ("H", "W", "cap")

    def __init__(self, device, H, W, cap):
        super().__init__((H, W, cap), device, table=16)


def test_scratch_base_class():
    sc = Toy(6, 8, "cpu")
    assert sc.key() == (6, 8, 4) and (sc.H, sc.W, sc.cap) == (6, 8, 4) and sc.device == torch.device("cpu")
    assert sc.scratch.numel() == 32 and sc.table.numel() == 16 and sc.scratch.dtype == torch.uint8 and not hasattr(sc, "host")
    Toy.check("tool", sc, (6, 8, 4), torch.device("cpu"))
    Toy.check("tool", sc, (6, 8, 4))
    for wrong in (object(), Other("cpu", 6, 8, 4)):
        with pytest.raises(InsarError, match="tool: scratch must be a Toy, got (object|Other)"):
            Toy.check("tool", wrong, (6, 8, 4), torch.device("cpu"))
    with pytest.raises(InsarError, match=r"tool: scratch of 6 x 8, cap=4 on cpu for 6 x 9, cap=4 on cpu"):
        Toy.check("tool", sc, (6, 9, 4), torch.device("cpu"))
    with pytest.raises(InsarError, match=r"scratch of 6 x 8, cap=4 on cpu for 6 x 8, cap=4 on cuda:0"):
        Toy.check("tool", sc, (6, 8, 4), torch.device("cuda:0"))
    # a stand-in passes only where the size of its table is verified
    Toy.check("tool", Other("cpu", 6, 8, 4), (6, 8, 4), table_bytes=16)
    with pytest.raises(InsarError, match=r"scratch of .* \(32 bytes\)"):
        Toy.check("tool", Other("cpu", 6, 8, 4), (6, 8, 4), table_bytes=32)


def test_scratch_build_and_adopt_table():
    assert Toy.build("cpu", 6, 8, 4).key() == (6, 8, 4) and Other.build("cpu", 6, 8, np.int64(4)).key() == (6, 8, 4)
    for key in ((6, 8, 4.0), (6, 8, True), (6, 8, "x"), (6, 8, None), (6, 8, 101)):      # the last one: the class's own refusal
        assert Toy.build("cpu", *key) is None
    assert _scene.Scratch.adopt_table("Toy", None, 64) == 64
    t = torch.zeros(64, dtype=torch.uint8)
    assert _scene.Scratch.adopt_table("Toy", t, 64) is t
    for bad in (t[:48], t.int(), t.view(8, 8), torch.zeros(128, dtype=torch.uint8)[::2], t.numpy()):
        with pytest.raises(InsarError, match="Toy: table must be a contiguous 16-byte aligned uint8 tensor of 64 bytes"):
            _scene.Scratch.adopt_table("Toy", bad, 64)


def test_query_bytes():
    from insar_unet_ca_amd import regions, score, zonal
    assert _scene.query_bytes("insar_zonal_scratch_bytes", 1, 0, 1, outputs=1) == zonal.scratch_bytes(1, 0, 1) == 128
    assert _scene.query_bytes("insar_overlap_scratch_bytes", 8, outputs=2) == score.scratch_bytes(8) == (16 + 16 * 16, 16 + 16 * 8)
    assert len(regions.scratch_bytes(64, 64, 16)) == 2
    with pytest.raises(InsarError, match="insar_overlap_scratch_bytes"):
        _scene.query_bytes("insar_overlap_scratch_bytes", 0, outputs=2)


@pytest.mark.parametrize("bad", ["x", None, True, [4]])
def test_capacities_that_are_no_numbers_are_refused_by_name(bad):
    """These used to escape as TypeError / ValueError from `int(v) != v` (and True used to pass as 1)."""
    class OnDevice(torch.Tensor):
        is_cuda = True

    mask = torch.zeros(8, 8, dtype=torch.uint8).as_subclass(OnDevice)
    labels = torch.zeros(8, 8, dtype=torch.int32).as_subclass(OnDevice)
    with pytest.raises(InsarError, match="label_regions: max_regions="):
        iu.label_regions(mask, max_regions=bad)
    with pytest.raises(InsarError, match="label_regions: min_area="):
        iu.label_regions(mask, min_area=bad)
    with pytest.raises(InsarError, match="region_overlaps: max_pairs="):
        iu.region_overlaps(labels, labels, max_pairs=bad)
    with pytest.raises(InsarError, match="region_stats: max_regions="):
        iu.region_stats(torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8), max_regions=bad)
    with pytest.raises(InsarError, match="region_stats: bins="):
        iu.region_stats(torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8), bins=bad)


def test_integral_floats_still_pass_where_they_did():
    """3.0 as a capacity was taken by the `int(v) != v` sites and still is: the next refusal is the device's."""
    with pytest.raises(InsarError, match="ROCm"):
        iu.region_stats(torch.zeros(8, 8, dtype=torch.int32), torch.zeros(8, 8), max_regions=16.0, count=3.0, bins=4.0, range=(0, 1))

"""CPU-only: the host side of detection scoring (insar_unet_ca_amd/score.py on csrc/overlap.hip): the additive ABI and its
argument checks (they run before anything touches a device), the overlaps oracle of tests/score_ref.py pinned against a double
loop over region masks, `match_from_overlaps` against the dense `match_oracle` on random tables and on answers worked out by
hand, and `DetectionScore`."""
import ctypes
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

import insar_unet_ca_amd as iu
from insar_unet_ca_amd import _lib, score
from insar_unet_ca_amd._lib import InsarError
from tests.score_ref import assert_match_equal, dense_from_labels, dense_from_table, match_oracle, overlaps_oracle

FAKE = 4096       # a non-null, 16-byte aligned "pointer": the checks below fail before anything dereferences it
ENTRY_POINTS = ("insar_overlap_scratch_bytes", "insar_overlap_clear", "insar_overlap_count", "insar_overlap_compact")


# ---- the library: exports, the scratch query, argument checks without a GPU ---------------------------------------------
def test_overlap_symbols_declared_exported_and_bound():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "insar_hip.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    for name in ("region_overlaps", "match_regions", "DetectionScore", "evaluate_scene"):
        assert name in iu.__all__ and callable(getattr(iu, name))
    assert callable(iu.ScenePredictor.evaluate)
    assert _lib.ABI_VERSION == 8 and _lib.load().insar_version() == 8          # additive: the ABI version stays


def test_overlap_record_layout(tmp_path):
    """score.OVERLAP_DTYPE is the C compiler's InsarOverlap."""
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "insar_hip.h")
    fields = list(score.OVERLAP_DTYPE.names)
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("%zu\\n", sizeof(InsarOverlap));']
    lines += [f'printf("%zu\\n", offsetof(InsarOverlap, {f}));' for f in fields]
    lines.append("return 0;}")
    (tmp_path / "o.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "o"), str(tmp_path / "o.c")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "o")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == score.OVERLAP_DTYPE.itemsize == 16
    assert out[1:] == [score.OVERLAP_DTYPE.fields[f][1] for f in fields]


def test_overlap_scratch_bytes_query():
    for max_pairs in (1, 2, 3, 8, 72, 1000, 65536, 262144, 262145, 1 << 24):
        tb, ob = score.scratch_bytes(max_pairs)
        cap, rem = divmod(tb - 16, 16)                              # a 16-byte header, then 16-byte slots
        assert rem == 0 and cap >= 2 * max_pairs and cap & (cap - 1) == 0
        assert cap < 4 * max_pairs or cap == 2                      # the SMALLEST such power of two
        assert ob == 16 + 16 * max_pairs
    assert score.scratch_bytes(8) == (16 + 16 * 16, 16 + 16 * 8)
    assert score.scratch_bytes() == (16 + 16 * 524288, 16 + 16 * 262144)
    for bad in (0, -1, (1 << 24) + 1):
        with pytest.raises(InsarError, match="max_pairs"):
            score.scratch_bytes(bad)
    a = ctypes.c_int64(0)
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_overlap_scratch_bytes", 8, None, ctypes.byref(a))
    with pytest.raises(InsarError, match="null"):
        _lib.call("insar_overlap_scratch_bytes", 8, ctypes.byref(a), None)


def test_overlap_entry_points_validate_without_a_gpu():
    ok = dict(pred=FAKE, gt=FAKE, void=None, void_value=255, H=200, W=264, table=FAKE, out=FAKE, max_pairs=1024)

    def clear(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_overlap_clear", a["table"], a["out"], a["max_pairs"], None)

    def count(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_overlap_count", a["pred"], a["gt"], a["void"], a["void_value"], a["H"], a["W"], a["table"],
                  a["max_pairs"], None)

    def compact(**kw):
        a = dict(ok, **kw)
        _lib.call("insar_overlap_compact", a["table"], a["max_pairs"], a["out"], None)

    for fn, names in ((clear, ("table", "out")), (count, ("pred", "gt", "table")), (compact, ("table", "out"))):
        for name in names:
            with pytest.raises(InsarError, match="null"):
                fn(**{name: None})
        with pytest.raises(InsarError, match=r"\(-1005\)"):            # INSAR_E_ARG, not a launch failure
            fn(table=None)
        for bad in (0, -5, (1 << 24) + 1):
            with pytest.raises(InsarError, match="max_pairs"):
                fn(max_pairs=bad)
        with pytest.raises(InsarError, match="aligned"):
            fn(table=FAKE + 8)
    for fn in (clear, compact):
        with pytest.raises(InsarError, match="aligned"):
            fn(out=FAKE + 8)
    for H, W in ((0, 264), (200, 0), (-3, 264), (65536, 32768), (46341, 46341)):      # the last two: H * W >= 2^31
        with pytest.raises(InsarError, match=r"\(-1001\)"):
            count(H=H, W=W)
    with pytest.raises(InsarError, match="aligned"):
        count(pred=FAKE + 2)
    for v in (-1, 256):
        with pytest.raises(InsarError, match="void_value"):
            count(void=FAKE, void_value=v)


def test_region_overlaps_refuses_host_tensors_and_bad_arguments():
    z = torch.zeros(8, 8, dtype=torch.int32)
    with pytest.raises(InsarError, match="no CPU fallback"):
        iu.region_overlaps(z, z)
    with pytest.raises(InsarError, match="torch tensor"):
        iu.region_overlaps(np.zeros((8, 8), dtype=np.int32), z)

    class OnDevice(torch.Tensor):
        is_cuda = True

    def dev(t):
        return t.as_subclass(OnDevice)

    good = dev(torch.zeros(8, 8, dtype=torch.int32))
    for bad in (dev(torch.zeros(8, 8, dtype=torch.int64)), dev(torch.zeros(2, 8, 8, dtype=torch.int32)),
                dev(torch.zeros(8, 16, dtype=torch.int32)[:, ::2])):
        with pytest.raises(InsarError, match="contiguous 2-D int32"):
            iu.region_overlaps(good, bad)
    with pytest.raises(InsarError, match=r"expected \(8, 8\)"):
        iu.region_overlaps(good, dev(torch.zeros(8, 12, dtype=torch.int32)))
    with pytest.raises(InsarError, match="no CPU fallback"):
        iu.region_overlaps(good, good, void=torch.zeros(8, 8, dtype=torch.uint8))
    for kw, pat in ((dict(max_pairs=0), "max_pairs"), (dict(max_pairs=2.5), "max_pairs"),
                    (dict(void=dev(torch.zeros(8, 8, dtype=torch.uint8)), void_value=300), "void_value")):
        with pytest.raises(InsarError, match=pat):
            iu.region_overlaps(good, good, **kw)


def test_overflow_and_too_many_keys_name_max_pairs():
    raw = np.zeros(16 + 16 * 4, dtype=np.uint8)
    raw[:16].view("<i8")[:] = (5, 0)                                    # more keys than records
    with pytest.raises(InsarError, match=r"5 overlapping pairs exceed max_pairs=4"):
        score.overlaps_from_raw(raw, 4)
    raw[:16].view("<i8")[:] = (3, 1)                                    # the probe bound ran out
    with pytest.raises(InsarError, match=r"max_pairs=4"):
        score.overlaps_from_raw(raw, 4)
    raw[:16].view("<i8")[:] = (3, 0)
    rec = raw[16:].view(score.OVERLAP_DTYPE)
    rec[:3] = [(2, 1, 7), (0, 1, 9), (1, 0, 4)]
    p, g, n = score.overlaps_from_raw(raw, 4)
    assert p.tolist() == [1, 0, 2] and g.tolist() == [0, 1, 1] and n.tolist() == [4, 9, 7]          # sorted by (gt, pred)
    assert p.dtype == np.int32 and g.dtype == np.int32 and n.dtype == np.int64


# ---- the overlaps oracle against a double loop over region masks ------------------------------------------------------------
def _random_labels(rng, H, W, n, fill):
    """Random label map: `n` ids scattered in blocks of 4 x 7 pixels, `fill` of the blocks foreground."""
    by, bx = (H + 3) // 4, (W + 6) // 7
    ids = rng.integers(1, n + 1, size=(by, bx)) * (rng.random((by, bx)) < fill)
    return np.kron(ids, np.ones((4, 7), dtype=np.int64))[:H, :W].astype(np.int32)


@pytest.mark.parametrize("with_void", [False, True])
def test_overlaps_oracle_matches_a_double_loop(with_void):
    rng = np.random.default_rng(7 + with_void)
    H, W = 40, 56
    pred = _random_labels(rng, H, W, 9, 0.6)
    gt = np.roll(_random_labels(rng, H, W, 7, 0.5), (1, 3), axis=(0, 1))
    void = np.where(rng.random((H, W)) < 0.1, 255, rng.integers(0, 3, size=(H, W))).astype(np.uint8) if with_void else None
    live = np.ones((H, W), dtype=bool) if void is None else void != 255
    want = []
    for g in range(0, 8):
        for p in range(0, 10):
            n = int(((pred == p) & (gt == g) & live).sum())
            if n and (p, g) != (0, 0):
                want.append((p, g, n))
    got = overlaps_oracle(pred, gt, void, 255)
    assert list(zip(*(v.tolist() for v in got))) == want
    assert len(want) > 40


# ---- matching: known answers ---------------------------------------------------------------------------------------------
def _regions(cls, conf=None):
    r = {"id": np.arange(1, len(cls) + 1, dtype=np.int32), "cls": np.asarray(cls, dtype=np.int32)}
    if conf is not None:
        r["mean_conf"] = np.asarray(conf, dtype=np.float64)
    return r


def _match(pred, gt, pcls, gcls, void=None, conf=None, n_valid=True, **kw):
    """match_from_overlaps on the oracle's table of two host label maps, checked against match_oracle on the dense matrix."""
    table = overlaps_oracle(pred, gt, void, 255)
    nv = (pred.size if void is None else int((void != 255).sum())) if n_valid else None
    got = iu.match_from_overlaps(table, _regions(pcls, conf), _regions(gcls), n_valid=nv, **kw)
    ref = match_oracle(dense_from_labels(pred, gt, len(pcls), len(gcls), void, 255), pcls, gcls, pred_conf=conf, n_valid=nv,
                       iou_threshold=kw.get("iou_threshold", 0.5), num_classes=kw.get("num_classes"))
    assert_match_equal(got, ref)
    return got


def _blank(H=20, W=40):
    return np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=np.int32)


def test_offset_squares_have_iou_one_third():
    pred, gt = _blank()
    gt[2:12, 5:15] = 1
    pred[2:12, 10:20] = 1                                              # 10 x 10 squares, 5 columns apart: 50 / 150
    m = _match(pred, gt, [1], [1], iou_threshold=0.5)
    assert m["gt_match"].tolist() == [0] and m["pred_match"].tolist() == [0]
    assert (m["overall"]["tp"], m["overall"]["fp"], m["overall"]["fn"]) == (0, 1, 1) and m["overall"]["pq"] == 0.0
    m = _match(pred, gt, [1], [1], iou_threshold=0.3)
    assert m["gt_match"].tolist() == [1] and m["pred_match"].tolist() == [1]
    assert m["gt_iou"][0] == 50 / 150 and m["pred_iou"][0] == 50 / 150
    assert (m["overall"]["tp"], m["overall"]["fp"], m["overall"]["fn"]) == (1, 0, 0)
    np.testing.assert_allclose(m["overall"]["pq"], 1 / 3, rtol=1e-12)


def test_a_gt_split_in_half_goes_to_the_lower_pred_id():
    pred, gt = _blank()
    gt[0:10, 0:20] = 1
    pred[0:10, 0:10] = 1
    pred[0:10, 10:20] = 2                                              # IoU 100 / 200 each: exactly the threshold
    m = _match(pred, gt, [1, 1], [1], iou_threshold=0.5)
    assert m["gt_match"].tolist() == [1] and m["pred_match"].tolist() == [1, 0]
    assert m["gt_iou"].tolist() == [0.5] and m["pred_iou"].tolist() == [0.5, 0.0]
    assert (m["overall"]["tp"], m["overall"]["fp"], m["overall"]["fn"]) == (1, 1, 0)


def test_a_pred_spanning_two_gts():
    pred, gt = _blank()
    gt[0:10, 0:12] = 1                                                 # 120 pixels
    gt[0:10, 14:22] = 2                                                # 80 pixels
    pred[0:10, 0:22] = 1                                               # 220 pixels over both: IoU 120 / 220 and 80 / 220
    m = _match(pred, gt, [1], [1, 1])
    assert m["gt_match"].tolist() == [1, 0] and m["pred_match"].tolist() == [1]
    assert m["gt_iou"][0] == 120 / 220
    assert (m["overall"]["tp"], m["overall"]["fp"], m["overall"]["fn"]) == (1, 0, 1)
    m = _match(pred, gt, [1], [1, 1], iou_threshold=0.25)              # still one match: each region is used once
    assert m["gt_match"].tolist() == [1, 0] and (m["overall"]["tp"], m["overall"]["fn"]) == (1, 1)


def test_class_mismatch_at_iou_one():
    pred, gt = _blank()
    gt[3:9, 4:30] = 1
    pred[3:9, 4:30] = 1
    m = _match(pred, gt, [2], [1], num_classes=3)
    assert m["gt_match"].tolist() == [0] and m["pred_match"].tolist() == [0]
    assert m["per_class"]["fp"].tolist() == [0, 0, 1] and m["per_class"]["fn"].tolist() == [0, 1, 0]
    want = np.zeros((3, 3), dtype=np.int64)
    want[1, 2] = 156                                                   # row = gt class, column = pred class
    want[0, 0] = 800 - 156
    assert np.array_equal(m["confusion"], want)


def test_a_gt_region_entirely_void_is_neither_tp_nor_fn():
    pred, gt = _blank()
    void = np.zeros_like(gt, dtype=np.uint8)
    gt[0:6, 0:6] = 1                                                   # wholly inside the void block
    gt[10:16, 10:20] = 2
    void[0:8, 0:8] = 255
    pred[0:6, 0:10] = 1                                                # 60 pixels, 48 of them void, none of the rest on a gt
    pred[10:16, 10:20] = 2
    m = _match(pred, gt, [1, 1], [1, 1], void=void)
    assert m["gt_area"].tolist() == [0, 60] and m["pred_area"].tolist() == [12, 60]
    assert m["gt_match"].tolist() == [0, 2] and m["pred_match"].tolist() == [0, 2]
    assert (m["overall"]["tp"], m["overall"]["fp"], m["overall"]["fn"]) == (1, 1, 0)
    pred[0:6, 6:10] = 0                                                # now the pred lies in the void too: no FP either
    m = _match(pred, gt, [1, 1], [1, 1], void=void)
    assert m["pred_area"].tolist() == [0, 60]
    assert (m["overall"]["tp"], m["overall"]["fp"], m["overall"]["fn"]) == (1, 0, 0)
    assert m["overall"]["pq"] == 1.0 and m["confusion"][0, 0] == 800 - 64 - 60


@pytest.mark.parametrize("case", ["no pred", "no gt", "neither"])
def test_empty_sides_score_zero_without_warnings(case):
    pred, gt = _blank()
    pcls, gcls = [], []
    if case != "no pred":
        pred[1:5, 1:5], pcls = 1, [1]
    if case != "no gt":
        gt[8:12, 8:14], gcls = 1, [1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = _match(pred, gt, pcls, gcls, conf=[0.9] * len(pcls))
        s = iu.DetectionScore(2)
        s.update(m)
        total = s.compute()
    assert m["overall"]["tp"] == 0 and m["overall"]["fp"] == len(pcls) and m["overall"]["fn"] == len(gcls)
    for k in ("precision", "recall", "f1", "sq", "rq", "pq"):
        assert m["overall"][k] == 0.0 and total["overall"][k] == 0.0 and (m["per_class"][k] == 0.0).all()
    assert m["ap_mean"] == 0.0 and (m["ap"] == 0.0).all()
    assert m["gt_match"].shape == (len(gcls),) and m["pred_match"].shape == (len(pcls),)


def _three_gts_four_preds():
    """One class. gt 1..3: 10 x 10 squares at columns 0, 20, 40. pred 1 (conf 0.9) = gt 1; pred 2 (0.8) touches nothing;
    pred 3 (0.7) = the top 8 rows of gt 2 (IoU 80 / 100); pred 4 (0.6) = gt 3 moved by 5 columns (IoU 50 / 150)."""
    pred, gt = _blank(20, 80)
    for k, x in enumerate((0, 20, 40)):
        gt[0:10, x:x + 10] = k + 1
    pred[0:10, 0:10] = 1
    pred[0:10, 60:70] = 2
    pred[0:8, 20:30] = 3
    pred[0:10, 45:55] = 4
    return pred, gt, [0.9, 0.8, 0.7, 0.6]


def test_scores_of_three_gts_and_four_preds_by_hand():
    pred, gt, conf = _three_gts_four_preds()
    F = Fraction
    # threshold 0.5: preds 1 and 3 match (IoU 1 and 4/5); pred 2 and pred 4 are false positives, gt 3 is missed
    m = _match(pred, gt, [1] * 4, [1] * 3, conf=conf)
    assert m["gt_match"].tolist() == [1, 3, 0] and m["pred_match"].tolist() == [1, 0, 2, 0]
    want = {"precision": F(2, 4), "recall": F(2, 3), "f1": F(4, 7), "sq": (F(1) + F(4, 5)) / 2, "rq": F(2) / (2 + F(1, 2) * 2 + F(1, 2))}
    want["pq"] = want["sq"] * want["rq"]
    assert want["pq"] == F(18, 35)
    o = m["overall"]
    assert (o["tp"], o["fp"], o["fn"]) == (2, 2, 1)
    for k, v in want.items():
        np.testing.assert_allclose(o[k], float(v), rtol=1e-12, err_msg=k)
        np.testing.assert_allclose(m["per_class"][k][1], float(v), rtol=1e-12, err_msg=k)
    # ranked by confidence: TP, FP, TP, FP -> precision 1, 1/2, 2/3, 1/2 at recall 1/3, 1/3, 2/3, 2/3
    ap = F(1, 3) * 1 + F(1, 3) * F(2, 3)
    assert ap == F(5, 9)
    np.testing.assert_allclose(m["ap"][1], float(ap), rtol=1e-12)
    np.testing.assert_allclose(m["ap_mean"], float(ap), rtol=1e-12)
    # threshold 0.3: pred 4 (IoU 1/3) now finds gt 3: TP, FP, TP, TP -> precision 1, 1/2, 2/3, 3/4 at recall 1/3, 1/3, 2/3, 1
    m = _match(pred, gt, [1] * 4, [1] * 3, conf=conf, iou_threshold=0.3)
    o = m["overall"]
    assert (o["tp"], o["fp"], o["fn"]) == (3, 1, 0)
    sq = (F(1) + F(4, 5) + F(1, 3)) / 3
    rq = F(3) / (3 + F(1, 2))
    for k, v in (("precision", F(3, 4)), ("recall", F(1)), ("f1", F(6, 7)), ("sq", sq), ("rq", rq), ("pq", sq * rq)):
        np.testing.assert_allclose(o[k], float(v), rtol=1e-12, err_msg=k)
    ap = F(1, 3) * 1 + F(1, 3) * F(3, 4) + F(1, 3) * F(3, 4)
    np.testing.assert_allclose(m["ap"][1], float(ap), rtol=1e-12)
    # a confidence order that puts the false positives first lowers ap and nothing else
    m2 = _match(pred, gt, [1] * 4, [1] * 3, conf=[0.1, 0.9, 0.2, 0.8])
    np.testing.assert_allclose(m2["ap"][1], float(F(1, 3) * F(1, 2) + F(1, 3) * F(1, 2)), rtol=1e-12)     # FP, FP, TP, TP
    assert m2["overall"]["tp"] == 2 and m2["gt_match"].tolist() == [1, 3, 0]


def test_ap_ranking_can_differ_from_the_greedy_matching():
    """gt 1 (60 px) holds pred 1 (36 px, IoU 3/5) and 24 px of pred 2, whose other 12 px lie on gt 2 (20 px): IoU(2, 1) = 24 / 72,
    IoU(2, 2) = 12 / 44. The matching pairs 1-1 and 2-2 whatever the confidences; ranked with pred 2 first, pred 2 takes gt 1
    (its best fit) and pred 1 finds it taken."""
    pred, gt = _blank(10, 80)
    gt[0, 0:60] = 1
    gt[2, 0:20] = 2
    pred[0, 0:36] = 1
    pred[0, 36:60] = 2
    pred[2, 0:12] = 2
    for conf, ap in (([0.9, 0.3], 1.0), ([0.3, 0.9], 0.5)):
        m = _match(pred, gt, [1, 1], [1, 1], conf=conf, iou_threshold=0.25)
        assert m["gt_match"].tolist() == [1, 2] and m["overall"]["tp"] == 2
        assert m["gt_iou"].tolist() == [36 / 60, 12 / 44]
        np.testing.assert_allclose(m["ap"][1], ap, rtol=1e-12)


# ---- matching: random pair tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_match_from_overlaps_on_random_tables(seed):
    rng = np.random.default_rng(seed)
    Np, Ng, K = int(rng.integers(1, 30)), int(rng.integers(1, 30)), int(rng.integers(2, 5))
    N = rng.integers(1, 40, size=(Np + 1, Ng + 1)) * (rng.random((Np + 1, Ng + 1)) < 0.08)
    for g in range(1, Ng + 1):                                      # one dominant partner per gt, so that matches exist
        N[int(rng.integers(1, Np + 1)), g] += int(rng.integers(50, 400))
    N[1:, 0] = rng.integers(0, 30, size=Np)
    N[0, 1:] = rng.integers(0, 30, size=Ng)
    N[0, 0] = 0
    if seed % 3 == 0:
        N[int(rng.integers(1, Np + 1)), :] = 0                      # a pred left with area 0
    gcls = rng.integers(1, K, size=Ng)
    pcls = rng.integers(1, K, size=Np)
    for g in range(1, Ng + 1):                                      # mostly agreeing classes
        if rng.random() < 0.8:
            pcls[int(N[1:, g].argmax())] = gcls[g - 1]
    conf = np.round(rng.random(Np), 1)                               # ties in confidence
    p, g = np.nonzero(N)
    shuffle = rng.permutation(len(p))                                # the order of the rows must not matter
    table = (p[shuffle].astype(np.int32), g[shuffle].astype(np.int32), N[p, g][shuffle].astype(np.int64))
    assert np.array_equal(dense_from_table(table, Np, Ng), N)
    for thr in (0.5, 0.25, 0.75):
        got = iu.match_from_overlaps(table, _regions(pcls, conf), _regions(gcls), iou_threshold=thr, num_classes=K,
                                     n_valid=int(N.sum()) + 1000)
        ref = match_oracle(N, pcls, gcls, iou_threshold=thr, num_classes=K, pred_conf=conf, n_valid=int(N.sum()) + 1000)
        assert_match_equal(got, ref, f"seed {seed} thr {thr}")
        assert got["confusion"].sum() == N.sum() + 1000
    assert ref["overall"]["tp"] + ref["overall"]["fn"] > 0


def test_match_from_overlaps_refuses_inconsistent_input():
    t = (np.array([1, 3]), np.array([1, 0]), np.array([5, 2]))
    with pytest.raises(InsarError, match="ids outside"):
        iu.match_from_overlaps(t, _regions([1, 1]), _regions([1]))
    with pytest.raises(InsarError, match="num_classes"):
        iu.match_from_overlaps(t, _regions([1, 1, 4]), _regions([1]), num_classes=3)
    with pytest.raises(InsarError, match="iou_threshold"):
        iu.match_from_overlaps(t, _regions([1, 1, 1]), _regions([1]), iou_threshold=0.0)
    with pytest.raises(InsarError, match="id, cls"):
        iu.match_from_overlaps(t, {"area": []}, _regions([1]))


# ---- DetectionScore ----------------------------------------------------------------------------------------------------------
def test_detection_score_over_two_scenes_equals_the_concatenated_counts():
    pred, gt, conf = _three_gts_four_preds()
    a = _match(pred, gt, [1, 2, 1, 1], [1, 1, 1], conf=conf, num_classes=3)
    pred2, gt2 = _blank()
    gt2[0:10, 0:20] = 1
    gt2[12:18, 0:9] = 2
    pred2[0:10, 0:14] = 1
    pred2[12:18, 0:8] = 2
    b = _match(pred2, gt2, [1, 2], [1, 2], num_classes=3)
    s = iu.DetectionScore(num_classes=3, iou_threshold=0.5)
    s.update(a)
    s.update(b)
    got = s.compute()
    assert got["scenes"] == 2
    tp, fp, fn = (a["per_class"][k] + b["per_class"][k] for k in ("tp", "fp", "fn"))
    assert tp.tolist() == [0, 3, 1] and fp.tolist() == [0, 1, 1] and fn.tolist() == [0, 1, 0]
    iou_sum = np.array([0.0, 1.0 + 0.8 + 0.7, 48 / 54])
    want = score.detection_scores(tp, fp, fn, iou_sum)
    for k in score.SCORE_FIELDS:
        np.testing.assert_allclose(got["per_class"][k], want[k], rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(got["per_class"]["sq"], [0.0, 2.5 / 3, 48 / 54], rtol=1e-12)
    o = got["overall"]
    assert (o["tp"], o["fp"], o["fn"]) == (4, 2, 1)
    np.testing.assert_allclose(o["sq"], (2.5 + 48 / 54) / 4, rtol=1e-12)
    np.testing.assert_allclose(o["rq"], 4 / (4 + 1 + 0.5), rtol=1e-12)
    np.testing.assert_allclose(o["pq"], o["sq"] * o["rq"], rtol=1e-12)
    s.reset()
    assert s.compute()["overall"]["pq"] == 0.0
    with pytest.raises(InsarError, match="num_classes"):
        iu.DetectionScore(2).update(a)
    with pytest.raises(InsarError, match="iou_threshold"):
        iu.DetectionScore(3, 0.75).update(a)

"""Scoring detections against ground truth at the level of sites: the overlap table of two label maps on the device
(csrc/overlap.hip: insar_overlap_clear / _count / _compact), then matching and scores in numpy on that table.

The table holds, for every pair (pred id p, gt id g) != (0, 0) that shares pixels outside the void map, how many pixels they
share; rows (p, 0) and columns (0, g) included, so the areas after voiding are A_p = sum_g n[p, g] and A_g = sum_p n[p, g].
Counts are integers and the table is sorted by (gt, pred) on the host: bitwise reproducible, although the order of the records
in the device buffer is not.

    table = region_overlaps(det["labels"], gt["labels"], void=gt_mask)        # three launches, one read-back
    res = match_from_overlaps(table, det["regions"], gt["regions"])           # numpy only: runs without a GPU
    res = match_regions(det, gt, void=gt_mask)                                # both
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import InsarError, call, ptr
from ._scene import Scratch, check_int, check_map, check_on_device, query_bytes, read_back
from .distance import boundary_iou

DEFAULT_MAX_PAIRS = 262144
MAX_PAIRS_LIMIT = 1 << 24

# the C struct InsarOverlap (include/insar_hip.h); the output buffer is a 16-byte header {n_keys, overflow}, then the records
OVERLAP_DTYPE = np.dtype([("pred", "<i4"), ("gt", "<i4"), ("count", "<i8")])
assert OVERLAP_DTYPE.itemsize == 16
SCORE_FIELDS = ("tp", "fp", "fn", "precision", "recall", "f1", "sq", "rq", "pq")


def scratch_bytes(max_pairs: int = DEFAULT_MAX_PAIRS) -> Tuple[int, int]:
    """(table bytes, output bytes) for room for max_pairs pairs. Host arithmetic only."""
    return query_bytes("insar_overlap_scratch_bytes", max_pairs, outputs=2)


class OverlapScratch(Scratch):
    """The device buffers of one max_pairs: the hash table, the compacted output and the pinned host copy the output is read
    back into. They do not depend on the scene size; nothing in them has to survive between calls."""
    KEY = ("max_pairs",)

    def __init__(self, device: torch.device, max_pairs: int = DEFAULT_MAX_PAIRS):
        tb, ob = scratch_bytes(max_pairs)
        super().__init__((max_pairs,), device, table=tb, out=ob, host=ob)


def _check_args(pred_labels, gt_labels, void, void_value, max_pairs) -> None:
    who = "region_overlaps"
    for name, t in (("pred_labels", pred_labels), ("gt_labels", gt_labels)):
        check_on_device(who, name, t)
        check_map(who, name, t, (torch.int32,))
    H, W = pred_labels.shape
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise InsarError(f"{who}: scene {H} x {W}: need H, W >= 1 and H * W < 2^31")
    check_map(who, "gt_labels", gt_labels, (torch.int32,), shape=(H, W), of="pred_labels")
    check_on_device(who, "gt_labels", gt_labels, like=pred_labels)
    if void is not None:
        check_on_device(who, "void", void, like=pred_labels)
        check_map(who, "void", void, (torch.uint8,), shape=(H, W))
        check_int(who, "void_value", void_value, 0, 255, integral_floats=True)
    check_int(who, "max_pairs", max_pairs, 1, MAX_PAIRS_LIMIT, integral_floats=True)


def _launch(pred_labels: torch.Tensor, gt_labels: torch.Tensor, void: Optional[torch.Tensor], void_value: int, max_pairs: int,
            table: torch.Tensor, out: torch.Tensor) -> None:
    """The three launches on the current stream."""
    H, W = pred_labels.shape
    s = _lib.stream_ptr()
    call("insar_overlap_clear", ptr(table), ptr(out), max_pairs, s)
    call("insar_overlap_count", ptr(pred_labels), ptr(gt_labels), ptr(void), int(void_value), H, W, ptr(table), max_pairs, s)
    call("insar_overlap_compact", ptr(table), max_pairs, ptr(out), s)


def overlaps_from_raw(raw: np.ndarray, max_pairs: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(pred, gt, count), sorted by (gt, pred), fresh arrays, from the raw bytes of an output buffer: raises if the table
    overflowed or holds more keys than max_pairs."""
    n_keys, overflow = (int(v) for v in raw[:16].view("<i8"))
    if overflow or n_keys > max_pairs:
        raise InsarError(f"region_overlaps: {n_keys} overlapping pairs{' and a full table' if overflow else ''} exceed "
                         f"max_pairs={max_pairs}: raise max_pairs, or min_area of the label maps")
    rec = raw[16:16 + 16 * n_keys].view(OVERLAP_DTYPE)
    order = np.lexsort((rec["pred"], rec["gt"]))
    return rec["pred"][order].copy(), rec["gt"][order].copy(), rec["count"][order].copy()


def region_overlaps(pred_labels: torch.Tensor, gt_labels: torch.Tensor, void: Optional[torch.Tensor] = None, void_value: int = 255,
                    max_pairs: int = DEFAULT_MAX_PAIRS, scratch: Optional[OverlapScratch] = None):
    """The overlap table of two device label maps (int32 [H, W], 0 or an id >= 1, as `label_regions` returns them).

        pred, gt, count = region_overlaps(pred_labels, gt_labels, void=gt_mask, void_value=255)
        pred, gt  int32 [n]    count  int64 [n]    sorted by (gt, pred); every (p, g) != (0, 0) that occurs, once

    A pixel is dropped iff `void` (uint8 [H, W]) is given and void == void_value there. Three launches on the current stream
    and ONE device-to-host read-back. More than `max_pairs` distinct pairs (or a table that filled up) raise InsarError.
    `scratch`: an OverlapScratch of this max_pairs to reuse (else allocated)."""
    _check_args(pred_labels, gt_labels, void, void_value, max_pairs)
    max_pairs = int(max_pairs)
    if scratch is None:
        scratch = OverlapScratch(pred_labels.device, max_pairs)
    else:
        OverlapScratch.check("region_overlaps", scratch, (max_pairs,), pred_labels.device)
    with torch.cuda.device(pred_labels.device):
        _launch(pred_labels, gt_labels, void, int(void_value), max_pairs, scratch.table, scratch.out)
        raw = read_back(scratch.host, scratch.out)
    return overlaps_from_raw(raw, max_pairs)


# ---- scores ---------------------------------------------------------------------------------------------------------------
def _ratio(a, b):
    """a / b in float64, 0.0 wherever b == 0 (arrays or scalars), without warnings."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape, dtype=np.float64), where=b != 0)
    return out if out.ndim else float(out)


def detection_scores(tp, fp, fn, iou_sum) -> dict:
    """precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn), sq = iou_sum / tp (the mean IoU of
    the matches), rq = tp / (tp + fp / 2 + fn / 2), pq = sq * rq; 0.0 wherever a denominator is 0. Arrays or scalars."""
    tp_f, fp_f, fn_f = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    sq, rq = _ratio(iou_sum, tp_f), _ratio(tp_f, tp_f + 0.5 * fp_f + 0.5 * fn_f)
    return {"tp": tp, "fp": fp, "fn": fn, "precision": _ratio(tp_f, tp_f + fp_f), "recall": _ratio(tp_f, tp_f + fn_f),
            "f1": _ratio(2 * tp_f, 2 * tp_f + fp_f + fn_f), "sq": sq, "rq": rq, "pq": sq * rq, "iou_sum": iou_sum}


def average_precision(is_tp: np.ndarray, n_gt: int) -> float:
    """All-point-interpolated area under precision / recall of a ranked list of detections (True = a true positive) against
    n_gt ground-truth regions; 0.0 when n_gt == 0."""
    if n_gt == 0:
        return 0.0
    hit = np.asarray(is_tp, dtype=bool)
    tp, fp = np.cumsum(hit), np.cumsum(~hit)
    rec = np.concatenate(([0.0], tp / float(n_gt), [1.0]))
    pre = np.concatenate(([0.0], tp / np.maximum(tp + fp, 1).astype(np.float64), [0.0]))
    pre = np.maximum.accumulate(pre[::-1])[::-1]                  # the envelope: non-increasing in recall
    return float(np.sum((rec[1:] - rec[:-1]) * pre[1:]))


def _region_columns(name: str, regions) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    if not isinstance(regions, dict) or "id" not in regions or "cls" not in regions:
        raise InsarError(f"match_from_overlaps: {name} must be the `regions` table of label_regions (id, cls, ...)")
    ids, cls = np.asarray(regions["id"]), np.asarray(regions["cls"]).astype(np.int64)
    if ids.shape != cls.shape or ids.ndim != 1 or not (ids == np.arange(1, len(ids) + 1)).all():
        raise InsarError(f"match_from_overlaps: {name}: ids must be 1..N in order")
    conf = regions.get("mean_conf")
    return cls, None if conf is None else np.asarray(conf, dtype=np.float64)


def match_from_overlaps(table, pred_regions: dict, gt_regions: dict, *, iou_threshold: float = 0.5,
                        num_classes: Optional[int] = None, n_valid: Optional[int] = None) -> dict:
    """Match predicted to true regions on an overlap table and score the result. Pure numpy.

    table: (pred, gt, count) of `region_overlaps`; pred_regions / gt_regions: the `regions` tables of `label_regions` (only
    `id`, `cls` and, for `ap`, the predictions' `mean_conf` are read). Areas come from the table (after voiding): A_p = the sum
    of row p, A_g = the sum of column g; a region left with area 0 takes no part on either side (neither TP, FP nor FN).
    IoU(p, g) = n / (A_p + A_g - n) in float64. Candidates are the pairs with p, g >= 1, equal class and IoU >= iou_threshold;
    they are taken greedily in the order (IoU descending, gt id ascending, pred id ascending), each region at most once.
    Above 0.5 this is the unique matching: two regions with IoU > 0.5 share more than half of either one, so no region has two
    such partners and no order of visiting can change the result; at exactly 0.5 and below, the order above decides.

    Returns a dict:
      gt_match int32 [Ng] (the matched pred id or 0), gt_iou float64 [Ng], pred_match int32 [Np], pred_iou float64 [Np],
      pred_area, gt_area int64 (after voiding), iou_threshold, num_classes K,
      per_class: tp, fp, fn (int64 [K], indexed by class value; class 0 is background and stays 0), precision, recall, f1,
                 sq, rq, pq, iou_sum (float64 [K]); overall: the same as scalars from the sums over classes,
      confusion int64 [K, K]: pixels by (gt class, pred class) of the two cleaned class maps outside the void map. Its
                 [0, 0] entry is n_valid minus every other entry when `n_valid` (the number of pixels not dropped) is given,
                 else 0: background against background is not in the table;
      with pred_regions["mean_conf"]: ap float64 [K] and ap_mean (the mean over the classes present in gt with area > 0; 0.0
                 if there is none). Preds are ranked by (mean_conf descending, id ascending); each takes the still-free gt of
                 its class with the highest IoU >= iou_threshold (ties: the lower gt id); ap is the all-point-interpolated
                 area under precision / recall."""
    tp_, tg_, tn_ = (np.asarray(v) for v in table)
    if not (tp_.shape == tg_.shape == tn_.shape and tp_.ndim == 1):
        raise InsarError("match_from_overlaps: table must be three 1-D arrays of one length (pred, gt, count)")
    tp_, tg_, tn_ = tp_.astype(np.int64), tg_.astype(np.int64), tn_.astype(np.int64)
    if not np.isfinite(iou_threshold) or not 0.0 < iou_threshold <= 1.0:
        raise InsarError(f"iou_threshold={iou_threshold!r}: a number in (0, 1]")
    pcls, pconf = _region_columns("pred_regions", pred_regions)
    gcls, _ = _region_columns("gt_regions", gt_regions)
    Np, Ng = len(pcls), len(gcls)
    if len(tn_) and (tp_.min() < 0 or tg_.min() < 0 or tp_.max() > Np or tg_.max() > Ng or tn_.min() < 1):
        raise InsarError(f"match_from_overlaps: the table names ids outside 0..{Np} / 0..{Ng}, or a count below 1")
    K = int(max(2, pcls.max(initial=0) + 1, gcls.max(initial=0) + 1)) if num_classes is None else int(num_classes)
    if K < 2 or pcls.max(initial=0) >= K or gcls.max(initial=0) >= K or pcls.min(initial=1) < 1 or gcls.min(initial=1) < 1:
        raise InsarError(f"match_from_overlaps: region classes must lie in 1..{K - 1} (num_classes={K})")

    area_p, area_g = np.zeros(Np + 1, dtype=np.int64), np.zeros(Ng + 1, dtype=np.int64)
    np.add.at(area_p, tp_, tn_)
    np.add.at(area_g, tg_, tn_)
    cls_p, cls_g = np.concatenate(([0], pcls)), np.concatenate(([0], gcls))         # indexed by id; id 0 = background
    confusion = np.zeros((K, K), dtype=np.int64)
    np.add.at(confusion, (cls_g[tg_], cls_p[tp_]), tn_)
    if n_valid is not None:
        if int(n_valid) < int(tn_.sum()):
            raise InsarError(f"match_from_overlaps: n_valid={n_valid} is less than the {int(tn_.sum())} pixels of the table")
        confusion[0, 0] = int(n_valid) - int(tn_.sum())

    fg = (tp_ >= 1) & (tg_ >= 1)
    cp, cg, cn = tp_[fg], tg_[fg], tn_[fg]
    iou = cn.astype(np.float64) / (area_p[cp] + area_g[cg] - cn).astype(np.float64)
    same = cls_p[cp] == cls_g[cg]
    cand = same & (iou >= iou_threshold)
    kp, kg, ki = cp[cand], cg[cand], iou[cand]
    gt_match, pred_match = np.zeros(Ng + 1, dtype=np.int32), np.zeros(Np + 1, dtype=np.int32)
    gt_iou, pred_iou = np.zeros(Ng + 1, dtype=np.float64), np.zeros(Np + 1, dtype=np.float64)
    for j in np.lexsort((kp, kg, -ki)):
        p, g = int(kp[j]), int(kg[j])
        if gt_match[g] or pred_match[p]:
            continue
        gt_match[g], pred_match[p] = p, g
        gt_iou[g] = pred_iou[p] = ki[j]

    live_p, live_g = area_p[1:] > 0, area_g[1:] > 0
    hit_p, hit_g = pred_match[1:] > 0, gt_match[1:] > 0
    tp = np.bincount(gcls[hit_g], minlength=K).astype(np.int64)
    fp = np.bincount(pcls[live_p & ~hit_p], minlength=K).astype(np.int64)
    fn = np.bincount(gcls[live_g & ~hit_g], minlength=K).astype(np.int64)
    iou_sum = np.zeros(K, dtype=np.float64)
    for c in range(1, K):                                        # in ascending gt id: one fixed order of summation
        iou_sum[c] = float(np.sum(gt_iou[1:][hit_g & (gcls == c)]))
    out = {"gt_match": gt_match[1:].copy(), "gt_iou": gt_iou[1:].copy(), "pred_match": pred_match[1:].copy(),
           "pred_iou": pred_iou[1:].copy(), "pred_area": area_p[1:].copy(), "gt_area": area_g[1:].copy(),
           "iou_threshold": float(iou_threshold), "num_classes": K, "confusion": confusion,
           "per_class": detection_scores(tp, fp, fn, iou_sum),
           "overall": detection_scores(int(tp.sum()), int(fp.sum()), int(fn.sum()), float(iou_sum.sum()))}

    if pconf is not None:
        if pconf.shape != (Np,):
            raise InsarError(f"match_from_overlaps: mean_conf of {pconf.shape} for {Np} regions")
        ok = same & (iou >= iou_threshold)
        by_pred: Dict[int, list] = {}
        for p, g, v in zip(cp[ok], cg[ok], iou[ok]):
            by_pred.setdefault(int(p), []).append((-float(v), int(g)))
        taken = np.zeros(Ng + 1, dtype=bool)
        ranked = [int(i) + 1 for i in np.lexsort((np.arange(Np), -pconf)) if live_p[i]]
        is_tp = np.zeros(Np + 1, dtype=bool)
        for p in ranked:
            for _, g in sorted(by_pred.get(p, ())):              # IoU descending, then gt id ascending
                if not taken[g]:
                    taken[g] = is_tp[p] = True
                    break
        ap = np.zeros(K, dtype=np.float64)
        present = []
        for c in range(1, K):
            n_gt = int((live_g & (gcls == c)).sum())
            ap[c] = average_precision([is_tp[p] for p in ranked if pcls[p - 1] == c], n_gt)
            if n_gt:
                present.append(c)
        out["ap"] = ap
        out["ap_mean"] = float(np.mean(ap[present])) if present else 0.0
    return out


def match_regions(pred: dict, gt: dict, *, void: Optional[torch.Tensor] = None, void_value: int = 255, iou_threshold: float = 0.5,
                  max_pairs: int = DEFAULT_MAX_PAIRS, num_classes: Optional[int] = None,
                  scratch: Optional[OverlapScratch] = None) -> dict:
    """`region_overlaps` of pred["labels"] and gt["labels"], then `match_from_overlaps` on it with pred["regions"] and
    gt["regions"]: `pred` and `gt` are the dicts `label_regions` returns (a `ScenePredictor.detect` result serves as `pred`).
    The result carries the sorted table under "overlaps". With a void map, the number of pixels it leaves (for the
    background-background entry of the confusion matrix) is one more small reduction on the device."""
    for name, d in (("pred", pred), ("gt", gt)):
        if not isinstance(d, dict) or "labels" not in d or "regions" not in d:
            raise InsarError(f"match_regions: {name} must be a dict with 'labels' and 'regions', as label_regions returns")
    table = region_overlaps(pred["labels"], gt["labels"], void=void, void_value=void_value, max_pairs=max_pairs, scratch=scratch)
    n_valid = pred["labels"].numel() - (0 if void is None else int((void == int(void_value)).sum()))
    out = match_from_overlaps(table, pred["regions"], gt["regions"], iou_threshold=iou_threshold, num_classes=num_classes,
                              n_valid=n_valid)
    out["overlaps"] = table
    return out


class DetectionScore:
    """Dataset-level detection scores: tp, fp, fn and the IoU sum of the matches per class, added up over scenes.

        score = DetectionScore(num_classes=2, iou_threshold=0.5)
        for scene, gt_mask in scenes:
            score.update(predictor.evaluate(scene, gt_mask)["score"])
        score.compute()["overall"]["pq"]

    Results that carry boundary-band counts (`evaluate(..., boundary_distance=d)`: match_result["boundary"]) have them added up
    too, and `compute()` then reports "boundary" = {"distance", "counts", "iou", "mean_iou", "scenes"} of the sums."""

    def __init__(self, num_classes: int, iou_threshold: float = 0.5):
        self.num_classes = check_int("DetectionScore", "num_classes", num_classes, 2, integral_floats=True)
        self.iou_threshold = float(iou_threshold)
        self.reset()

    def reset(self) -> None:
        K = self.num_classes
        self.tp, self.fp, self.fn = (np.zeros(K, dtype=np.int64) for _ in range(3))
        self.iou_sum = np.zeros(K, dtype=np.float64)
        self.scenes = 0
        self.boundary_counts, self.boundary_distance, self.boundary_scenes = None, None, 0

    def update(self, match_result: dict) -> None:
        if match_result["num_classes"] != self.num_classes or match_result["iou_threshold"] != self.iou_threshold:
            raise InsarError(f"DetectionScore(num_classes={self.num_classes}, iou_threshold={self.iou_threshold}): got a result "
                             f"of num_classes={match_result['num_classes']}, iou_threshold={match_result['iou_threshold']}")
        pc = match_result["per_class"]
        self.tp += pc["tp"]
        self.fp += pc["fp"]
        self.fn += pc["fn"]
        self.iou_sum += pc["iou_sum"]
        self.scenes += 1
        b = match_result.get("boundary")
        if b is not None:
            counts = np.asarray(b["counts"], dtype=np.int64)
            if counts.shape != (self.num_classes, 3) or self.boundary_distance not in (None, b["distance"]):
                raise InsarError(f"DetectionScore(num_classes={self.num_classes}): boundary counts of {counts.shape} at distance "
                                 f"{b['distance']} after counts at distance {self.boundary_distance}")
            self.boundary_counts = counts.copy() if self.boundary_counts is None else self.boundary_counts + counts
            self.boundary_distance = b["distance"]
            self.boundary_scenes += 1

    def compute(self) -> dict:
        """{"per_class": ..., "overall": ..., "scenes": n}: `detection_scores` of the accumulated counts."""
        out = {"per_class": detection_scores(self.tp.copy(), self.fp.copy(), self.fn.copy(), self.iou_sum.copy()),
               "overall": detection_scores(int(self.tp.sum()), int(self.fp.sum()), int(self.fn.sum()), float(self.iou_sum.sum())),
               "scenes": self.scenes}
        if self.boundary_counts is not None:
            out["boundary"] = {"distance": self.boundary_distance, "counts": self.boundary_counts.copy(),
                               "scenes": self.boundary_scenes, **boundary_iou(self.boundary_counts)}
        return out

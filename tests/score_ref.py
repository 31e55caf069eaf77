"""CPU oracles of insar_unet_ca_amd.score (a helper, not a test module), written without reading score.py's method:
`overlaps_oracle` is np.unique on a combined key; `match_oracle` works on the DENSE intersection matrix with explicit loops
(score.py works on the sparse table with sorts). tests/test_score_host.py pins the first against a double loop over region
masks."""
import numpy as np


def overlaps_oracle(pred, gt, void=None, void_value=255):
    """(pred ids, gt ids, counts) sorted by (gt, pred) of two integer label maps: every (p, g) != (0, 0) over the pixels where
    void != void_value."""
    p, g = np.asarray(pred).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    if void is not None:
        keep = np.asarray(void).ravel() != void_value
        p, g = p[keep], g[keep]
    stride = int(p.max(initial=0)) + 1
    key, count = np.unique(g * stride + p, return_counts=True)          # ascending key = ascending (gt, pred)
    keep = key != 0
    key, count = key[keep], count[keep]
    return (key % stride).astype(np.int32), (key // stride).astype(np.int32), count.astype(np.int64)


def dense_from_table(table, Np, Ng):
    """int64 [Np + 1, Ng + 1] intersection matrix of a (pred, gt, count) table; [0, 0] stays 0."""
    N = np.zeros((Np + 1, Ng + 1), dtype=np.int64)
    for p, g, n in zip(*table):
        N[int(p), int(g)] += int(n)
    return N


def dense_from_labels(pred, gt, Np, Ng, void=None, void_value=255):
    return dense_from_table(overlaps_oracle(pred, gt, void, void_value), Np, Ng)


def _div(a, b):
    return float(a) / float(b) if b else 0.0


def scores_oracle(tp, fp, fn, iou_sum):
    sq, rq = _div(iou_sum, tp), _div(tp, tp + 0.5 * fp + 0.5 * fn)
    return {"tp": tp, "fp": fp, "fn": fn, "precision": _div(tp, tp + fp), "recall": _div(tp, tp + fn),
            "f1": _div(2 * tp, 2 * tp + fp + fn), "sq": sq, "rq": rq, "pq": sq * rq}


def ap_oracle(hits, n_gt):
    """All-point interpolation: the sum over the recall steps of (step width) x (the best precision at that recall or beyond)."""
    if n_gt == 0:
        return 0.0
    prec, rec, tp = [], [], 0
    for k, h in enumerate(hits):
        tp += bool(h)
        prec.append(tp / (k + 1))
        rec.append(tp / n_gt)
    ap, last = 0.0, 0.0
    for k in range(len(hits)):
        if rec[k] > last:
            ap += (rec[k] - last) * max(prec[k:])
            last = rec[k]
    return ap


def match_oracle(N, pred_cls, gt_cls, iou_threshold=0.5, num_classes=None, pred_conf=None, n_valid=None):
    """The contract of score.match_from_overlaps on a dense intersection matrix N [Np + 1, Ng + 1] (row / column 0 =
    background; N[0, 0] ignored) and the class of every region."""
    N = np.asarray(N, dtype=np.int64).copy()
    N[0, 0] = 0
    pred_cls, gt_cls = [int(c) for c in pred_cls], [int(c) for c in gt_cls]
    Np, Ng = len(pred_cls), len(gt_cls)
    K = num_classes if num_classes is not None else max([2] + [c + 1 for c in pred_cls + gt_cls])
    area_p, area_g = N.sum(axis=1), N.sum(axis=0)
    union = area_p[:, None] + area_g[None, :] - N
    iou = np.where(N > 0, N / np.maximum(union, 1).astype(np.float64), 0.0)
    iou[0, :] = 0.0
    iou[:, 0] = 0.0
    touching = [(int(p), int(g)) for g, p in zip(*np.nonzero(N.T)) if p and g]          # in (gt, pred) order

    def allowed(p, g):
        return pred_cls[p - 1] == gt_cls[g - 1] and iou[p, g] >= iou_threshold

    cands = [(p, g) for p, g in touching if allowed(p, g)]
    gt_match, pred_match = [0] * (Ng + 1), [0] * (Np + 1)
    while True:                                                      # the best remaining pair, one at a time
        best = None
        for p, g in cands:
            if gt_match[g] or pred_match[p]:
                continue
            if best is None or iou[p, g] > iou[best]:                # strict: the earlier (gt, pred) wins a tie
                best = (p, g)
        if best is None:
            break
        pred_match[best[0]], gt_match[best[1]] = best[1], best[0]

    per_class = {k: [0] * K for k in ("tp", "fp", "fn")}
    iou_sum = [0.0] * K
    for g in range(1, Ng + 1):
        if gt_match[g]:
            per_class["tp"][gt_cls[g - 1]] += 1
            iou_sum[gt_cls[g - 1]] += iou[gt_match[g], g]
        elif area_g[g] > 0:
            per_class["fn"][gt_cls[g - 1]] += 1
    for p in range(1, Np + 1):
        if not pred_match[p] and area_p[p] > 0:
            per_class["fp"][pred_cls[p - 1]] += 1
    rows = [scores_oracle(per_class["tp"][c], per_class["fp"][c], per_class["fn"][c], iou_sum[c]) for c in range(K)]
    confusion = np.zeros((K, K), dtype=np.int64)
    for p, g in zip(*np.nonzero(N)):
        confusion[gt_cls[g - 1] if g else 0, pred_cls[p - 1] if p else 0] += N[p, g]
    if n_valid is not None:
        confusion[0, 0] = n_valid - N.sum()
    out = {"gt_match": np.array(gt_match[1:], dtype=np.int32), "pred_match": np.array(pred_match[1:], dtype=np.int32),
           "gt_iou": np.array([iou[gt_match[g], g] if gt_match[g] else 0.0 for g in range(1, Ng + 1)], dtype=np.float64),
           "pred_iou": np.array([iou[p, pred_match[p]] if pred_match[p] else 0.0 for p in range(1, Np + 1)], dtype=np.float64),
           "pred_area": area_p[1:], "gt_area": area_g[1:], "confusion": confusion,
           "per_class": {k: np.array([r[k] for r in rows]) for k in rows[0]},
           "overall": scores_oracle(sum(per_class["tp"]), sum(per_class["fp"]), sum(per_class["fn"]), sum(iou_sum))}
    if pred_conf is not None:
        order = sorted((p for p in range(1, Np + 1) if area_p[p] > 0), key=lambda p: (-float(pred_conf[p - 1]), p))
        taken, hits, partners = set(), {}, {}
        for p, g in cands:
            partners.setdefault(p, []).append(g)
        for p in order:
            best = 0
            for g in partners.get(p, ()):                           # ascending gt id: the lower id wins a tie
                if g not in taken and (best == 0 or iou[p, g] > iou[p, best]):
                    best = g
            hits[p] = best > 0
            if best:
                taken.add(best)
        ap, present = np.zeros(K, dtype=np.float64), []
        for c in range(1, K):
            n_gt = sum(1 for g in range(1, Ng + 1) if gt_cls[g - 1] == c and area_g[g] > 0)
            ap[c] = ap_oracle([hits[p] for p in order if pred_cls[p - 1] == c], n_gt)
            if n_gt:
                present.append(c)
        out["ap"] = ap
        out["ap_mean"] = float(np.mean(ap[present])) if present else 0.0
    return out


def assert_match_equal(got, ref, what=""):
    """Every integer exactly, IoU and the scores to rtol 1e-12."""
    for k in ("gt_match", "pred_match", "pred_area", "gt_area", "confusion"):
        assert np.array_equal(got[k], ref[k]), f"{what}: {k}: {got[k]} != {ref[k]}"
    for k in ("gt_iou", "pred_iou"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=0, err_msg=f"{what}: {k}")
    for level in ("per_class", "overall"):
        for k in ("tp", "fp", "fn"):
            assert np.array_equal(got[level][k], ref[level][k]), f"{what}: {level} {k}: {got[level][k]} != {ref[level][k]}"
        for k in ("precision", "recall", "f1", "sq", "rq", "pq"):
            np.testing.assert_allclose(got[level][k], ref[level][k], rtol=1e-12, atol=0, err_msg=f"{what}: {level} {k}")
    assert ("ap" in got) == ("ap" in ref), what
    if "ap" in ref:
        np.testing.assert_allclose(got["ap"], ref["ap"], rtol=1e-12, atol=0, err_msg=f"{what}: ap")
        np.testing.assert_allclose(got["ap_mean"], ref["ap_mean"], rtol=1e-12, atol=0, err_msg=f"{what}: ap_mean")

"""Scoring a scene on one GPU, in one process: `region_overlaps` on two pairs of 4096 x 4096 label maps,

  bowls    the label map of the synthetic bowls task (tools/regions_bench.py: 8-connected, min_area 16) against a copy of the
           class map shifted by (5, 9) pixels and labelled the same way
  speckle  random foreground at 50 % fill (4-connected, min_area 64) against its shift by (5, 9)

against three things measured in the same run: the host route a user has today (both label maps .cpu(), then
np.unique(p * (Ng + 1) + g, return_counts=True)), `label_regions` of the same class map, and `ScenePredictor.predict` of the
scene the bowls mask belongs to. Device times are medians over rounds of event pairs around each launch (clear, count,
compact) and around all three; `call_us` is the host clock around the whole region_overlaps call, read-back and sort included;
`match_us` the numpy matching on the table.

    python tools/score_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/scene_score.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import insar_unet_ca_amd as iu  # noqa: E402
from insar_unet_ca_amd import _lib, regions, score  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

LAUNCHES = ("clear", "count", "compact")
SHIFT = (5, 9)


def host_route(pred: torch.Tensor, gt: torch.Tensor, n_gt: int) -> dict:
    """What a user does today: both label maps to the host, one np.unique over the combined key."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    t1 = time.perf_counter()
    key, count = np.unique(p.astype(np.int64).ravel() * (n_gt + 1) + g.ravel(), return_counts=True)
    t2 = time.perf_counter()
    return {"copy_us": (t1 - t0) * 1e6, "unique_us": (t2 - t1) * 1e6, "total_us": (t2 - t0) * 1e6,
            "keys": int(len(key) - (key[0] == 0))}


def measure(name: str, mask: torch.Tensor, connectivity: int, min_area: int, rounds: int, warmup: int) -> dict:
    H, W = mask.shape
    shifted = torch.roll(mask, SHIFT, dims=(0, 1)).contiguous()
    rs = regions.RegionScratch(H, W, mask.device)
    kw = dict(connectivity=connectivity, min_area=min_area, scratch=rs)
    pred, gt = iu.label_regions(mask, **kw), iu.label_regions(shifted, **kw)
    P, G = pred["labels"], gt["labels"]
    M = score.DEFAULT_MAX_PAIRS
    while True:                                      # the smallest power-of-two multiple of the default that holds the table
        sc = score.OverlapScratch(mask.device, M)
        try:
            iu.region_overlaps(P, G, max_pairs=M, scratch=sc)
            break
        except iu.InsarError:
            M *= 2
    s = _lib.stream_ptr()
    steps = {
        "clear": lambda: call("insar_overlap_clear", ptr(sc.table), ptr(sc.out), M, s),
        "count": lambda: call("insar_overlap_count", ptr(P), ptr(G), None, 255, H, W, ptr(sc.table), M, s),
        "compact": lambda: call("insar_overlap_compact", ptr(sc.table), M, ptr(sc.out), s),
    }

    def all_launches():
        for k in LAUNCHES:
            steps[k]()

    for _ in range(warmup):
        table = iu.region_overlaps(P, G, max_pairs=M, scratch=sc)
        iu.label_regions(mask, **kw)
    t = {k: [] for k in LAUNCHES}
    t["device_us"], t["call_us"], t["match_us"], t["label_regions_us"] = [], [], [], []
    for _ in range(rounds):                          # the launches in order: every one runs on the state the one before left
        for k in LAUNCHES:
            t[k].append(timed(steps[k]))
        t["device_us"].append(timed(all_launches))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = iu.region_overlaps(P, G, max_pairs=M, scratch=sc)
        t1 = time.perf_counter()
        res = iu.match_from_overlaps(table, pred["regions"], gt["regions"], n_valid=H * W)
        t2 = time.perf_counter()
        iu.label_regions(mask, **kw)
        t3 = time.perf_counter()
        t["call_us"].append((t1 - t0) * 1e6)
        t["match_us"].append((t2 - t1) * 1e6)
        t["label_regions_us"].append((t3 - t2) * 1e6)
    med = {k: median(v) for k, v in t.items()}
    host = host_route(P, G, gt["count"])
    assert host["keys"] == len(table[0]), (host["keys"], len(table[0]))
    o = res["overall"]
    out = {"case": name, "scene": [H, W], "connectivity": connectivity, "min_area": min_area, "shift": list(SHIFT),
           "pred_regions": pred["count"], "gt_regions": gt["count"], "keys": int(len(table[0])),
           "largest_count": int(table[2].max(initial=0)), "max_pairs": M, "launches_per_call": 3,
           "launch_us": {k: med[k] for k in LAUNCHES}, "device_us": med["device_us"], "call_us": med["call_us"],
           "match_us": med["match_us"], "label_regions_us": med["label_regions_us"],
           "readback_bytes": int(sc.host.numel()), "host_route": host, "host_over_call": host["total_us"] / med["call_us"],
           "call_over_label_regions": med["call_us"] / med["label_regions_us"],
           "score": {"tp": o["tp"], "fp": o["fp"], "fn": o["fn"], "pq": o["pq"]}, "all_rounds": t}
    print(f"{name}: {out['keys']} keys, {med['device_us']:.0f} us on the device, {med['call_us']:.0f} us per call, host route "
          f"{host['total_us']:.0f} us, label_regions {med['label_regions_us']:.0f} us", file=sys.stderr)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    mask = torch.from_numpy(lab).to(dev)
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    cases = [measure("bowls", mask, 8, 16, a.rounds, a.warmup), measure("speckle", speckle, 4, 64, a.rounds, a.warmup)]

    # predict of the scene the bowls mask belongs to, as tools/regions_bench.py measures it
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
    scene = torch.from_numpy(img).to(dev)
    for _ in range(a.warmup):
        pred.predict(scene)
    ms = []
    for _ in range(max(3, a.rounds // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred.predict(scene)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    predict_ms = median(ms)
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "predict_ms": predict_ms,
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16", "cases": cases,
           "call_share_of_predict": {c["case"]: c["call_us"] * 1e-3 / predict_ms for c in cases}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

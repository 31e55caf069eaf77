"""Splitting touching sites on one GPU, in one process: `split_regions` (min_depth 1, distance heights) of three 4096 x 4096
label maps,

  bowls    `label_regions` of the bowls task's class map (tools/regions_bench.py: connectivity 8, min_area 16)
  speckle  `label_regions` of random foreground at 50 % fill, connectivity 4, min_area 64
  discs    overlapping discs of radius 20 on a jittered grid of pitch 30 under one class: chains and sheets of touching sites

next to `label_regions`, `distance_transform` and `ScenePredictor.predict` of the same scene measured in the same run, with the
raw basins, pieces and rounds of every map. If scipy is importable, the host route a user has today is timed as context, not
parity (its markers and flooding order are not this rule): labels.cpu(), distance_transform_edt, maximum-filter markers,
watershed_ift.

`device_us`: events around the launches of one split of a given height map (basins, as many batches of four rounds as the map
needs, finish) with no read-back between them, median over rounds. `height_us`: the same around `distance_transform`.
`call_us`: the host clock around the whole split_regions call (height map, launches, the reads of the control words and of
the table, the host table), median.

    python tools/split_bench.py [--size 4096] [--rounds 5] [--warmup 2] [--out profiles/split.json]
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
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import insar_unet_ca_amd as iu  # noqa: E402
from insar_unet_ca_amd import _lib, split  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from regions_bench import bowls, median, timed  # noqa: E402

MAX_REGIONS = 1 << 22
MAX_PAIRS = 1 << 24
MIN_DEPTH = 1.0


def discs(size: int, pitch: int = 30, r: int = 20, seed: int = 1) -> np.ndarray:
    """uint8 [size, size]: discs on a grid of `pitch`, each kept with probability 1 / 2 and moved by up to 4 pixels."""
    rng = np.random.default_rng(seed)
    m = np.zeros((size, size), dtype=np.uint8)
    yy, xx = np.indices((2 * r + 1, 2 * r + 1)) - r
    stamp = yy * yy + xx * xx <= r * r
    for cy in range(r + 4, size - r - 4, pitch):
        for cx in range(r + 4, size - r - 4, pitch):
            if rng.random() < 0.5:
                continue
            y, x = cy + int(rng.integers(-4, 5)), cx + int(rng.integers(-4, 5))
            m[y - r:y + r + 1, x - r:x + r + 1] |= stamp
    return m


def host_path(labels: torch.Tensor) -> dict:
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab = labels.cpu().numpy()
    t1 = time.perf_counter()
    d = ndimage.distance_transform_edt(lab > 0)
    t2 = time.perf_counter()
    peaks = (ndimage.maximum_filter(d, size=3) == d) & (lab > 0)
    markers, n = ndimage.label(peaks, structure=np.ones((3, 3), dtype=bool))
    t3 = time.perf_counter()
    cost = (255 - np.minimum(d, 255)).astype(np.uint8)
    cost[lab == 0] = 255
    markers = markers.astype(np.int32)
    markers[lab == 0] = -1
    ndimage.watershed_ift(cost, markers)
    t4 = time.perf_counter()
    return {"copy_us": (t1 - t0) * 1e6, "edt_us": (t2 - t1) * 1e6, "markers_us": (t3 - t2) * 1e6, "watershed_ift_us": (t4 - t3) * 1e6,
            "total_us": (t4 - t0) * 1e6, "markers": int(n)}


def measure(name: str, labelled: dict, label_us: float, rounds: int, warmup: int, with_host: bool) -> dict:
    labels, H, W = labelled["labels"], *labelled["labels"].shape
    sc = split.SplitScratch(H, W, labels.device, MAX_REGIONS, MAX_PAIRS, 64)
    kw = dict(mask=labelled["mask"], min_depth=MIN_DEPTH, max_regions=MAX_REGIONS, max_pairs=MAX_PAIRS, scratch=sc)
    for _ in range(max(1, warmup)):
        out = iu.split_regions(labels, **kw)
    batches = max(1, -(-(out["rounds"] + 1) // split.ROUNDS_PER_READ))
    T = int(np.rint(MIN_DEPTH * 16))
    s = _lib.stream_ptr()
    piece_map = torch.empty_like(labels)

    def height():
        return iu.distance_transform(labels, sites="edge", max_distance=None, scratch=sc.distance)["d2"]

    h = height()

    def launches():
        call("insar_split_basins", ptr(labels), ptr(h), H, W, MAX_PAIRS, 64, ptr(sc.scratch), s)
        for b in range(batches):
            call("insar_split_rounds", ptr(h), H, W, 1, T, b * split.ROUNDS_PER_READ, split.ROUNDS_PER_READ, MAX_PAIRS, 64,
                 ptr(sc.scratch), s)
        call("insar_split_finish", ptr(labels), ptr(h), ptr(labelled["mask"]), None, H, W, MAX_REGIONS, MAX_PAIRS, 64,
             ptr(sc.scratch), ptr(sc.table), ptr(piece_map), s)

    dev_us, h_us, call_us = [], [], []
    for _ in range(rounds):
        dev_us.append(timed(launches))
        h_us.append(timed(height))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = iu.split_regions(labels, **kw)
        call_us.append((time.perf_counter() - t0) * 1e6)
    assert torch.equal(piece_map, out["labels"])
    pairs = int(sc.ctrl_host.numpy().view(np.int32)[0])
    res = {"case": name, "map": [H, W], "regions": labelled["count"], "labelled_share": float((labels > 0).float().mean()),
           "raw_basins": out["raw_basins"], "basin_pairs": pairs, "pieces": out["count"], "rounds": out["rounds"],
           "converged": out["converged"], "min_depth": MIN_DEPTH, "launches": 11 + 4 * split.ROUNDS_PER_READ * batches,
           "device_us": median(dev_us), "height_us": median(h_us), "call_us": median(call_us), "label_regions_call_us": label_us,
           "scratch_bytes": int(sc.scratch.numel()), "all_rounds": {"device_us": dev_us, "height_us": h_us, "call_us": call_us}}
    if with_host:
        res["host_path"] = host_path(labels)
    print(f"{name}: {res['regions']} regions, {res['raw_basins']} basins -> {res['pieces']} pieces in {res['rounds']} rounds; "
          f"{res['device_us']:.0f} us on the device + {res['height_us']:.0f} us of distance transform, {res['call_us']:.0f} us per call"
          + (f"; host route {res['host_path']['total_us']:.0f} us" if with_host else ""), file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    maps = {"bowls": (torch.from_numpy(lab).to(dev), dict(connectivity=8, min_area=16)),
            "speckle": (torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev), dict(connectivity=4, min_area=64)),
            "discs": (torch.from_numpy(discs(S)).to(dev), dict(connectivity=8, min_area=16))}
    try:
        import scipy  # noqa: F401
        with_host = True
    except ImportError:
        with_host = False

    cases = []
    for name, (m, kw) in maps.items():
        for _ in range(max(1, a.warmup)):
            out = iu.label_regions(m, None, max_regions=MAX_REGIONS, **kw)
        us = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = iu.label_regions(m, None, max_regions=MAX_REGIONS, **kw)
            us.append((time.perf_counter() - t0) * 1e6)
        cases.append(measure(name, out, median(us), a.rounds, a.warmup, with_host))

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
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "predict_ms": median(ms),
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16",
           "host_path": "scipy: distance_transform_edt, maximum_filter markers, watershed_ift (context, not parity)" if with_host
                        else "not yet measured (scipy is not importable here)", "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

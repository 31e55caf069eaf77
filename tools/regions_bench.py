"""Regions of a scene on one GPU, in one process: `label_regions` on two 4096 x 4096 class maps,

  bowls    the label maps of the synthetic bowls task (data.make_tile_bowl, 256-pixel tiles side by side: its natural
           region density), with a confidence field, connectivity 8, min_area 16
  speckle  the adversarial case: random foreground at 50 % fill, connectivity 4 (a million raw components; min_area 64
           keeps the kept regions below the cap)

against two things measured in the same run: the host path a user has today (mask.cpu() + scipy.ndimage.label +
find_objects) and `ScenePredictor.predict` of the scene the bowls mask belongs to (UNet(use_se=True) bf16, tile 256,
overlap 32, batch 16). Device times are medians over rounds of event pairs around each phase call (tiles, merge, flatten,
number = 3 launches, relabel) and around all five; `call_us` is the host clock around the whole label_regions call,
read-back and host table included.

    python tools/regions_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/scene_regions.json]
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
from insar_unet_ca_amd import _lib, regions  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from insar_unet_ca_amd.data import make_tile_bowl  # noqa: E402

PHASES = ("tiles", "merge", "flatten", "number", "relabel")


def timed(fn) -> float:
    """us between two events on the current stream around fn()."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def bowls(size: int, tile: int = 256):
    """(scene float32 [size, size] in [-1, 1], label map uint8) of the bowls task, tiles side by side."""
    n = (size + tile - 1) // tile
    img = np.zeros((n * tile, n * tile), dtype=np.float32)
    lab = np.zeros((n * tile, n * tile), dtype=np.uint8)
    for r in range(n):
        for c in range(n):
            x, y = make_tile_bowl(9000 + r * n + c, tile, 1)
            img[r * tile:(r + 1) * tile, c * tile:(c + 1) * tile] = x[0]
            lab[r * tile:(r + 1) * tile, c * tile:(c + 1) * tile] = y
    return np.ascontiguousarray(img[:size, :size]), np.ascontiguousarray(lab[:size, :size])


def host_path(mask_dev: torch.Tensor, connectivity: int) -> dict:
    """What a user does today: copy the mask to the host, scipy.ndimage.label, find_objects."""
    from scipy import ndimage
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mask_dev.cpu().numpy()
    t1 = time.perf_counter()
    lab, n = ndimage.label(m != 0, structure=structure)
    t2 = time.perf_counter()
    ndimage.find_objects(lab)
    t3 = time.perf_counter()
    return {"copy_us": (t1 - t0) * 1e6, "label_us": (t2 - t1) * 1e6, "find_objects_us": (t3 - t2) * 1e6,
            "total_us": (t3 - t0) * 1e6, "components": int(n)}


def measure(name: str, mask: torch.Tensor, conf, connectivity: int, min_area: int, rounds: int, warmup: int) -> dict:
    H, W = mask.shape
    R = regions.DEFAULT_MAX_REGIONS
    sc = regions.RegionScratch(H, W, mask.device, R)
    labels = torch.empty(H, W, dtype=torch.int32, device=mask.device)
    clean = torch.empty(H, W, dtype=torch.uint8, device=mask.device)
    s = _lib.stream_ptr()
    steps = {
        "tiles": lambda: call("insar_regions_tiles", ptr(mask), ptr(conf), 0.0, H, W, connectivity, ptr(sc.scratch), s),
        "merge": lambda: call("insar_regions_merge", ptr(mask), H, W, connectivity, ptr(sc.scratch), s),
        "flatten": lambda: call("insar_regions_flatten", H, W, ptr(sc.scratch), s),
        "number": lambda: call("insar_regions_number", ptr(mask), H, W, min_area, R, ptr(sc.scratch), ptr(sc.table), s),
        "relabel": lambda: call("insar_regions_relabel", ptr(mask), ptr(conf), H, W, R, ptr(sc.scratch), ptr(sc.table),
                                ptr(labels), ptr(clean), s),
    }

    def all_phases():
        for p in PHASES:
            steps[p]()

    kw = dict(connectivity=connectivity, min_area=min_area, scratch=sc)
    for _ in range(warmup):
        out = iu.label_regions(mask, conf, **kw)
    t = {p: [] for p in PHASES}
    t["device_us"], t["call_us"] = [], []
    for _ in range(rounds):                          # the phases in order: every one runs on the state the one before left
        for p in PHASES:
            t[p].append(timed(steps[p]))
        t["device_us"].append(timed(all_phases))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = iu.label_regions(mask, conf, **kw)
        t["call_us"].append((time.perf_counter() - t0) * 1e6)
    med = {k: median(v) for k, v in t.items()}
    rec = sc.host.numpy().view(regions.REGION_DTYPE)
    host = host_path(mask, connectivity)
    res = {"case": name, "scene": [H, W], "connectivity": connectivity, "min_area": min_area, "with_conf": conf is not None,
           "foreground_share": float((mask != 0).float().mean()), "regions": out["count"],
           "largest_region": int(out["regions"]["area"].max(initial=0)), "raw_components_host": host["components"],
           "launches_per_call": 7, "phase_us": {p: med[p] for p in PHASES}, "device_us": med["device_us"],
           "call_us": med["call_us"], "table_readback_bytes": int(rec.nbytes), "host_path": host,
           "host_over_call": host["total_us"] / med["call_us"], "all_rounds": t}
    print(f"{name}: {med['device_us']:.0f} us on the device, {med['call_us']:.0f} us per call, host path {host['total_us']:.0f} us",
          file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regions_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    mask = torch.from_numpy(lab).to(dev)
    conf = torch.from_numpy((0.5 + 0.5 * rng.random((S, S))).astype(np.float32)).to(dev)
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    cases = [measure("bowls", mask, conf, 8, 16, a.rounds, a.warmup),
             measure("speckle", speckle, None, 4, 64, a.rounds, a.warmup)]

    # predict of the scene the bowls mask belongs to, as tools/scene_bench.py measures it
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

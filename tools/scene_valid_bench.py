"""Scene inference with no-data on one GPU, in one process: what skipping the empty tiles saves and what the masked path
costs. UNet(use_se=True) bf16 (seeded weights), tile 256, overlap 32, batch 16, a 4096 x 4096 scene whose valid footprint is a
rectangle rotated by 12 degrees that covers about 55 % of the box: once uint8 with the footprint as a validity plane, once
float32 with NaN outside it.

Records (a) tiles run of tiles planned; (b) the census by device events next to its HBM floor N * T^2 * (element size + 1 byte
of the plane where one is given) / 5.5 TB/s (arithmetic, not a measurement); (c) masked `predict` next to plain `predict` of
the same scene, alternated round by round (host clock around the call + device synchronise; the plain predict of the float32
scene runs on the scene with its NaN replaced by 0); (d) masked `predict` of an all-valid scene (nodata = a value that does
not occur) next to plain `predict`, alternated: the cost of census + read-back + masked finalize.

    python tools/scene_valid_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/scene_valid.json]
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

HBM_TBS = 5.5                                     # the achievable figure README.md quotes


def footprint(H: int, W: int, degrees: float = 12.0, cover: float = 0.55) -> np.ndarray:
    """bool [H, W]: a rectangle with the box's aspect, rotated about the centre, scaled to cover `cover` of the box."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.deg2rad(degrees)
    u = (x - W / 2) * np.cos(a) + (y - H / 2) * np.sin(a)
    v = -(x - W / 2) * np.sin(a) + (y - H / 2) * np.cos(a)
    s = np.sqrt(cover)
    return (np.abs(u) < s * W / 2) & (np.abs(v) < s * H / 2)


def timed_us(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def alternate(rounds: int, **legs) -> dict:
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(wall_ms(fn))
    return {k: {"median_ms": median(v), "all_ms": v} for k, v in t.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_valid_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    H = W = a.size
    T, o, B, K = a.tile, a.overlap, a.batch, 2
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=K, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=T, overlap=o, batch=B, num_classes=K)
    rng = np.random.default_rng(0)
    foot = footprint(H, W)
    origins = iu.plan_tiles(H, W, T, o)
    N = len(origins)
    o_dev = torch.from_numpy(origins).to(dev)

    u8 = torch.from_numpy(rng.integers(0, 255, size=(H, W), dtype=np.uint8)).to(dev)           # 255 does not occur
    plane = torch.from_numpy(foot.astype(np.uint8)).to(dev)
    f32_host = rng.standard_normal((H, W)).astype(np.float32)
    f32_filled = torch.from_numpy(np.where(foot, f32_host, np.float32(0))).to(dev)
    f32 = torch.from_numpy(np.where(foot, f32_host, np.float32("nan"))).to(dev)

    cases = {"uint8_plane": (u8, dict(valid=plane), u8, 1 + 1), "float32_nan": (f32, dict(nodata=float("nan")), f32_filled, 4)}
    out = {"scene": [H, W], "model": "UNet(use_se=True) bf16", "tile": T, "overlap": o, "batch": B, "tiles_total": N,
           "footprint": {"rotation_degrees": 12.0, "valid_fraction": float(foot.mean())}, "rounds": a.rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "hbm_TBps_of_the_floor": HBM_TBS, "cases": {}}
    for name, (scene, kw, plain_scene, bytes_per_pixel) in cases.items():
        for _ in range(a.warmup):
            res = pred.predict(scene, **kw)
            pred.predict(plain_scene)
        census_kw = {k: v for k, v in kw.items() if k in ("valid", "nodata")}
        census_us = median([timed_us(lambda: iu.tile_census(scene, o_dev, T, **census_kw)) for _ in range(max(a.rounds, 5))])
        floor_us = N * T * T * bytes_per_pixel / (HBM_TBS * 1e12) * 1e6
        legs = alternate(a.rounds, masked=lambda: pred.predict(scene, **kw), plain=lambda: pred.predict(plain_scene))
        run = res["tiles_run"]
        out["cases"][name] = {"tiles_run": run, "tiles_total": N, "valid_fraction_of_pixels": float(foot.mean()),
                              "census_us": census_us, "census_floor_us": floor_us, "census_bytes_per_pixel": bytes_per_pixel,
                              "masked_predict_ms": legs["masked"]["median_ms"], "plain_predict_ms": legs["plain"]["median_ms"],
                              "masked_over_plain": legs["masked"]["median_ms"] / legs["plain"]["median_ms"],
                              "tiles_run_over_total": run / N, "all_rounds": {k: v["all_ms"] for k, v in legs.items()}}
    # all valid: what the masked path costs when it skips nothing
    for _ in range(a.warmup):
        res = pred.predict(u8, nodata=255)
    assert res["tiles_run"] == N
    legs = alternate(a.rounds, masked=lambda: pred.predict(u8, nodata=255), plain=lambda: pred.predict(u8))
    over = legs["masked"]["median_ms"] - legs["plain"]["median_ms"]
    census_us = median([timed_us(lambda: iu.tile_census(u8, o_dev, T, nodata=255)) for _ in range(max(a.rounds, 5))])
    counts = iu.tile_census(u8, o_dev, T, nodata=255)
    readback_us = median([wall_ms(lambda: counts.cpu().numpy()) * 1e3 for _ in range(max(a.rounds, 5))])
    out["all_valid"] = {"masked_predict_ms": legs["masked"]["median_ms"], "plain_predict_ms": legs["plain"]["median_ms"],
                        "overhead_ms": over, "overhead_fraction_of_plain": over / legs["plain"]["median_ms"],
                        "census_us": census_us, "census_floor_us": N * T * T * 1 / (HBM_TBS * 1e12) * 1e6,
                        "readback_of_the_census_us_host_clock": readback_us,
                        "all_rounds": {k: v["all_ms"] for k, v in legs.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

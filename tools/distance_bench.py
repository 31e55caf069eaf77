"""The distance transform on one GPU, in one process: `distance_transform` on two 4096 x 4096 maps,

  bowls    the class map of the synthetic bowls task (tools/regions_bench.py), sites = "edge": long class borders, most pixels far
           from any
  speckle  random foreground at 50 % fill, sites = "edge": nearly every pixel is a site or next to one

with and without `nearest`, at max_distance 8, 32 and unbounded; `boundary_counts` at distance 3 of the map against its shift by
(5, 9) (what `evaluate(boundary_distance=3)` adds), and `void_band(width=3)` on a 16 x 256 x 256 batch of bowls masks. Each is
compared with the host route a user has today on the same box (.cpu() + scipy.ndimage.distance_transform_edt of the same sites;
without scipy: tests/distance_ref.dist_oracle on a 256 x 256 crop scaled by the pixel ratio, and labelled as such), and with
`ScenePredictor.predict` of the scene the bowls mask belongs to. Device times are medians over rounds of event pairs around
the call (two launches; no read-back), the least and the largest round beside them; `all_sites_map_us` is the
transform of a map of sites only, whose row pass leaves at k = 1: the column pass and the floor of the row pass.

    python tools/distance_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/distance.json]
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
from tools.regions_bench import bowls, median, timed  # noqa: E402

SHIFT = (5, 9)
DISTANCES = (8, 32, None)


def edge_sites(m: np.ndarray) -> np.ndarray:
    s = np.zeros(m.shape, dtype=bool)
    d = m[:, 1:] != m[:, :-1]
    s[:, 1:] |= d
    s[:, :-1] |= d
    d = m[1:] != m[:-1]
    s[1:] |= d
    s[:-1] |= d
    return s


def host_route(mask: torch.Tensor) -> dict:
    """What a user does today: the map to the host, its border pixels in numpy, scipy's exact EDT."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mask.cpu().numpy()
    t1 = time.perf_counter()
    sites = edge_sites(m)
    t2 = time.perf_counter()
    try:
        from scipy import ndimage
    except ImportError:
        from tests.distance_ref import dist_oracle
        c = 256
        t2 = time.perf_counter()
        dist_oracle(sites[:c, :c])
        t3 = time.perf_counter()
        scale = m.size / float(c * c)
        return {"how": f"numpy oracle on a {c} x {c} crop, scaled by {scale:.0f}", "copy_us": (t1 - t0) * 1e6,
                "edt_us": (t3 - t2) * 1e6 * scale, "total_us": (t1 - t0) * 1e6 + (t3 - t2) * 1e6 * scale}
    ndimage.distance_transform_edt(~sites)
    t3 = time.perf_counter()
    return {"how": "scipy.ndimage.distance_transform_edt", "copy_us": (t1 - t0) * 1e6, "sites_us": (t2 - t1) * 1e6,
            "edt_us": (t3 - t2) * 1e6, "total_us": (t3 - t0) * 1e6}


def measure(name: str, mask: torch.Tensor, rounds: int, warmup: int) -> dict:
    H, W = mask.shape
    sc = iu.DistanceScratch(1, H, W, mask.device)
    cases, spread = {}, {}
    for R in DISTANCES:
        for near in (False, True):
            fn = lambda: iu.distance_transform(mask, sites="edge", max_distance=R, return_nearest=near, scratch=sc)
            for _ in range(warmup):
                fn()
            v = [timed(fn) for _ in range(rounds)]
            cases[f"max_distance={R},nearest={near}"] = median(v)
            spread[f"max_distance={R},nearest={near}"] = [min(v), max(v)]
    d2 = iu.distance_transform(mask, sites="edge", max_distance=None, scratch=sc)["d2"]
    reach = d2[d2 != iu.distance.FAR]
    full = lambda: iu.distance_transform(mask, sites=("ne", 255), max_distance=32, scratch=sc)
    for _ in range(warmup):
        full()
    columns_us = median([timed(full) for _ in range(rounds)])
    shifted = torch.roll(mask, SHIFT, dims=(0, 1)).contiguous()
    for _ in range(warmup):
        counts = iu.boundary_counts(mask, shifted, 3, 2, void_value=None, scratch=sc)
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = iu.boundary_counts(mask, shifted, 3, 2, void_value=None, scratch=sc)
        t.append((time.perf_counter() - t0) * 1e6)
    host = host_route(mask)
    out = {"case": name, "map": [H, W], "sites": "edge", "site_share": float((d2 == 0).float().mean()),
           "largest_d2": int(reach.max()) if reach.numel() else None, "launches_per_transform": 2, "transform_us": cases, "spread_us": spread,
           "all_sites_map_us": columns_us, "boundary_counts_call_us": median(t), "boundary_counts_launches": 6,
           "boundary_iou_at_3_vs_shift": iu.boundary_iou(counts)["iou"].tolist(), "host_route": host,
           "host_over_transform_32": host["total_us"] / cases["max_distance=32,nearest=False"]}
    print(f"{name}: " + ", ".join(f"{k} {v:.0f} us" for k, v in cases.items()) + f"; boundary_counts {median(t):.0f} us; host "
          f"route {host['total_us']:.0f} us ({host['how']})", file=sys.stderr)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distance_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    mask = torch.from_numpy(lab).to(dev)
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    cases = [measure("bowls", mask, a.rounds, a.warmup), measure("speckle", speckle, a.rounds, a.warmup)]

    # void_band on a training batch
    n = 256
    batch = torch.from_numpy(np.stack([lab[(i // 4) * n:(i // 4 + 1) * n, (i % 4) * n:(i % 4 + 1) * n] for i in range(16)]).copy()).to(dev)
    band = lambda: iu.void_band(batch, 3)
    for _ in range(a.warmup):
        band()
    void_band_us = median([timed(band) for _ in range(a.rounds)])

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
    out = {"device": torch.cuda.get_device_name(0), "clock_state": "not read; nothing sets it; the spread of the rounds is under spread_us", "rounds": a.rounds, "warmup": a.warmup,
           "predict_ms": predict_ms, "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16", "cases": cases,
           "void_band_16x256x256_width3_us": void_band_us,
           "boundary_counts_share_of_predict": {c["case"]: c["boundary_counts_call_us"] * 1e-3 / predict_ms for c in cases}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

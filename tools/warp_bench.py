"""Resampling on one GPU, in one process: a 4096 x 4096 scene, uint8 and float32, through insar_warp_raster (the identity, and
7 degrees with zoom 1.3 about the centre, both modes) and insar_multilook (4 x 4); a batch of 16 x 256 x 256 warped crops
(insar_warp_draw + insar_warp_gather) next to the axis-aligned gather (insar_crops_gather) at the same origins.

  *_us              median, least and largest over rounds; a round is `reps` back-to-back calls between two events, divided by reps
  floor_us          the bytes the call must move (source once + every output once) at 5.55 TB/s, the HBM rate the other tools
                    quote; a 16 - 64 MB source also fits the last-level cache, so the floor is a yardstick, not a bound
  torch_grid_sample context, not parity: torch.nn.functional.affine_grid + grid_sample on the float32 scene, same warp, same process
                    (float coordinates, another rounding: the results are close, not equal)

    python tools/warp_bench.py [--size 4096] [--rounds 9] [--warmup 3] [--reps 10] [--out profiles/warp.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import insar_unet_ca_amd as iu  # noqa: E402
from tools.regions_bench import median, timed  # noqa: E402

HBM_TBPS = 5.55
TILE, BATCH = 256, 16


def rounds(fn, n: int, warmup: int, reps: int, nbytes: int) -> dict:
    def burst():
        for _ in range(reps):
            fn()

    for _ in range(warmup):
        burst()
    v = [timed(burst) / reps for _ in range(n)]
    floor = nbytes / (HBM_TBPS * 1e6)
    return {"median_us": round(median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "bytes": nbytes,
            "floor_us": round(floor, 2), "times_floor": round(median(v) / floor, 2)}


def about_centre(size: int, degrees: float, zoom: float):
    c, s, m = zoom * math.cos(math.radians(degrees)), zoom * math.sin(math.radians(degrees)), (size - 1) / 2
    return [[c, -s, m - c * m + s * m], [s, c, m - s * m - c * m]]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.size
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(n, n)).astype(np.uint8)).to(dev)
    f32 = torch.from_numpy(rng.standard_normal((n, n)).astype(np.float32)).to(dev)
    labels = torch.from_numpy((rng.random((n, n)) < 0.2).astype(np.uint8)).to(dev)
    ident, turn = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], about_centre(n, 7.0, 1.3)
    res = {"scene": [n, n], "rounds": a.rounds, "reps": a.reps, "hbm_tbps_for_floor": HBM_TBPS, "raster": {}}
    for name, src in (("uint8", u8), ("float32", f32)):
        es = src.element_size()
        out = torch.empty_like(src)
        q_ident = torch.from_numpy(iu.warp.quantise_matrix(ident).reshape(1, 6)).to(dev)
        q_turn = torch.from_numpy(iu.warp.quantise_matrix(turn).reshape(1, 6)).to(dev)
        leg = {}
        for mode in ("nearest", "bilinear"):
            for wname, q in (("identity", q_ident), ("rot7_zoom1.3", q_turn)):
                # a device table: the timed call is the launch alone, without the upload of a host matrix
                leg[f"{wname}_{mode}"] = rounds(lambda: iu.warp_raster(src, q, (n, n), mode=mode, out=out[None]), a.rounds, a.warmup, a.reps,
                                                2 * n * n * es)
        leg["identity_equals_source"] = bool(torch.equal(iu.warp_raster(src, ident, (n, n)), src))
        leg["multilook4"] = rounds(lambda: iu.multilook(src, 4), a.rounds, a.warmup, a.reps, n * n * es + (n // 4) ** 2 * es)
        res["raster"][name] = leg
    x = f32[None, None]
    theta = torch.tensor([[[1.3 * math.cos(math.radians(7.0)), -1.3 * math.sin(math.radians(7.0)), 0.0],
                           [1.3 * math.sin(math.radians(7.0)), 1.3 * math.cos(math.radians(7.0)), 0.0]]], device=dev)

    def torch_warp():
        grid = torch.nn.functional.affine_grid(theta, list(x.shape), align_corners=True)
        return torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)

    res["torch_grid_sample_float32_rot7_zoom1.3"] = rounds(torch_warp, a.rounds, a.warmup, max(1, a.reps // 5), 2 * n * n * 4)
    # compared where all four taps lie inside the source: at the rim the two differ by design (zero padding blends the outermost
    # half pixel, the warp clamps its taps and fills what lies off the extent)
    ours = iu.warp_raster(f32, turn, (n, n), fill=0.0)
    core = torch.zeros(n, n, dtype=torch.uint8, device=dev)
    core[2:-2, 2:-2] = 1
    inner = iu.warp_raster(core, turn, (n, n), mode="nearest") == 1
    diff = (torch_warp()[0, 0] - ours).abs()
    res["torch_grid_sample_max_abs_difference"] = {"interior": float(diff[inner].max()), "anywhere": float(diff.max()),
                                                   "interior_fraction": float(inner.float().mean())}
    origins = torch.from_numpy((rng.integers(0, (n - TILE) // 8 + 1, size=(BATCH, 2)) * 8).astype(np.int32)).to(dev)
    spec = iu.WarpSpec(zoom=(1.0 / 1.3, 1.3), max_angle_deg=7.0)
    mats = iu.draw_warps(5, origins, TILE, spec)
    out_bytes = BATCH * TILE * TILE * (4 + 8)
    res["crops"] = {
        "tile": TILE, "batch": BATCH, "spec": spec.config(),
        "gather_crops": rounds(lambda: iu.gather_crops(u8, labels, origins, TILE), a.rounds, a.warmup, a.reps, out_bytes + BATCH * TILE * TILE * 2),
        "draw_warps": rounds(lambda: iu.draw_warps(5, origins, TILE, spec), a.rounds, a.warmup, a.reps, BATCH * 56),
        "gather_warped": rounds(lambda: iu.gather_warped(u8, labels, mats, TILE), a.rounds, a.warmup, a.reps, out_bytes + BATCH * TILE * TILE * 2),
        "gather_warped_identity": rounds(lambda q=iu.draw_warps(5, origins, TILE, iu.WarpSpec()): iu.gather_warped(u8, labels, q, TILE),
                                         a.rounds, a.warmup, a.reps, out_bytes + BATCH * TILE * TILE * 2)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

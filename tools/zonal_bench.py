"""Per-region statistics of a raster on one GPU, in one process: `region_stats` of a float32 4096 x 4096 raster over three
label maps,

  bowls    `label_regions` of the bowls task's class map (tools/regions_bench.py: connectivity 8, min_area 16)
  speckle  `label_regions` of random foreground at 50 % fill, connectivity 4, min_area 64
  single   one region covering the whole map: every wave of every work-group meets one record

with and without a 64-bin histogram, next to `label_regions` and `ScenePredictor.predict` of the same scene measured in the
same run, and against the host route a user has today: labels.cpu(), raster.cpu(), np.bincount for n, sum and square sum,
scipy.ndimage.minimum_position / maximum_position.

`device_us`: events around `reps` back-to-back clear + accumulate pairs, divided by reps, median over rounds. `call_us`:
the host clock around the whole region_stats call (two launches, the read-back of the table, the host table), median.
`floor_us`: the read traffic the kernel is specified with, 8 bytes per pixel (labels + one float32 channel), at the
5.5 TB/s the repository's streaming kernels report (README): an HBM-only bound. The kernel does not read the raster under
background quads, and 134 MB fit the 256 MB Infinity Cache, so a map that is mostly background, or a rerun on the same
buffers, may come in under it.

    python tools/zonal_bench.py [--size 4096] [--rounds 7] [--reps 20] [--warmup 2] [--out profiles/zonal.json]
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
from insar_unet_ca_amd import _lib, zonal  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from regions_bench import bowls, median, timed  # noqa: E402

STREAM_BYTES_PER_S = 5.5e12          # README: the streaming kernels of this repository, HBM-bound
BINS = 64
RANGE = (-3.0, 3.0)


def host_path(labels: torch.Tensor, raster: torch.Tensor, count: int) -> dict:
    """What a user does today: both maps to the host, bincount for the moments, ndimage for the extremes' positions."""
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab, r = labels.cpu().numpy(), raster.cpu().numpy()
    t1 = time.perf_counter()
    flat, v = lab.ravel(), r.ravel().astype(np.float64)
    n = np.bincount(flat, minlength=count + 1)
    s = np.bincount(flat, weights=v, minlength=count + 1)
    ss = np.bincount(flat, weights=v * v, minlength=count + 1)
    t2 = time.perf_counter()
    idx = np.arange(1, count + 1)
    ndimage.minimum_position(r, lab, idx)
    ndimage.maximum_position(r, lab, idx)
    t3 = time.perf_counter()
    return {"copy_us": (t1 - t0) * 1e6, "bincount_us": (t2 - t1) * 1e6, "positions_us": (t3 - t2) * 1e6,
            "total_us": (t3 - t0) * 1e6, "labelled_pixels": int(n[1:].sum()), "moments_finite": bool(np.isfinite(s).all() and np.isfinite(ss).all())}


def measure(name: str, labels: torch.Tensor, raster: torch.Tensor, count: int, rounds: int, reps: int, warmup: int, with_host: bool) -> dict:
    H, W = labels.shape
    R = zonal.DEFAULT_MAX_REGIONS
    s = _lib.stream_ptr()
    res = {"case": name, "map": [H, W], "regions": count, "labelled_share": float((labels > 0).float().mean()), "launches_per_call": 2,
           "read_bytes_spec": 8 * H * W, "floor_us": 8 * H * W / STREAM_BYTES_PER_S * 1e6}
    for bins in (0, BINS):
        sc = zonal.ZonalScratch(labels.device, R, bins, 1)
        q_lo, q_hi = (zonal.quantise_scalar(RANGE[0], 65536.0), zonal.quantise_scalar(RANGE[1], 65536.0)) if bins else (0, 0)

        def pair():
            call("insar_zonal_clear", ptr(sc.table), R, bins, 1, s)
            call("insar_zonal_accumulate", ptr(labels), ptr(raster), _lib.ZONAL_F32, 1, H, W, 65536.0, 0, 0.0, bins, q_lo, q_hi, R,
                 ptr(sc.table), s)

        def clear_only():
            call("insar_zonal_clear", ptr(sc.table), R, bins, 1, s)

        def many(fn):
            def run():
                for _ in range(reps):
                    fn()
            return run

        kw = dict(count=count, scratch=sc, **(dict(bins=bins, range=RANGE) if bins else {}))
        for _ in range(warmup):
            iu.region_stats(labels, raster, **kw)
        dev_us, clr_us, call_us = [], [], []
        for _ in range(rounds):
            dev_us.append(timed(many(pair)) / reps)
            clr_us.append(timed(many(clear_only)) / reps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            iu.region_stats(labels, raster, **kw)
            call_us.append((time.perf_counter() - t0) * 1e6)
        d, c = median(dev_us), median(clr_us)
        res["hist64" if bins else "plain"] = {"bins": bins, "device_us": d, "clear_us": c, "accumulate_us": d - c, "call_us": median(call_us),
                                              "table_readback_bytes": int(sc.host.numel()), "device_over_floor": d / res["floor_us"],
                                              "accumulate_over_floor": (d - c) / res["floor_us"],
                                              "all_rounds": {"device_us": dev_us, "clear_us": clr_us, "call_us": call_us}}
    if with_host:
        res["host_path"] = host_path(labels, raster, count)
        res["host_over_call"] = res["host_path"]["total_us"] / res["plain"]["call_us"]
    print(f"{name}: {res['plain']['device_us']:.1f} us on the device ({res['plain']['device_over_floor']:.2f} x the floor of "
          f"{res['floor_us']:.1f} us), {res['plain']['call_us']:.0f} us per call; with {BINS} bins {res['hist64']['device_us']:.1f} us"
          + (f"; host route {res['host_path']['total_us']:.0f} us" if with_host else ""), file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("zonal_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    raster = torch.from_numpy(rng.normal(size=(S, S)).astype(np.float32)).to(dev)
    mask = torch.from_numpy(lab).to(dev)
    conf = torch.from_numpy((0.5 + 0.5 * rng.random((S, S))).astype(np.float32)).to(dev)
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)

    def labelled(m, c, **kw):
        for _ in range(a.warmup):
            out = iu.label_regions(m, c, **kw)
        us = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = iu.label_regions(m, c, **kw)
            us.append((time.perf_counter() - t0) * 1e6)
        return out, median(us)

    b, b_us = labelled(mask, conf, connectivity=8, min_area=16)
    sp, sp_us = labelled(speckle, None, connectivity=4, min_area=64)
    cases = [measure("bowls", b["labels"], raster, b["count"], a.rounds, a.reps, a.warmup, True),
             measure("speckle", sp["labels"], raster, sp["count"], a.rounds, a.reps, a.warmup, True),
             measure("single", torch.ones(S, S, dtype=torch.int32, device=dev), raster, 1, a.rounds, a.reps, a.warmup, False)]
    cases[0]["label_regions_call_us"], cases[1]["label_regions_call_us"] = b_us, sp_us

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
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup, "raster": "float32 normal",
           "stream_bytes_per_s_assumed": STREAM_BYTES_PER_S, "predict_ms": median(ms),
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16", "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

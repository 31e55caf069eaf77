"""The focal operations on a 4096 x 4096 float32 raster on one GPU, in one process:

  smooth_gauss_1.5, smooth_box_1, smooth_box_15   `smooth_raster` under gaussian_taps(1.5) (R = 5), box_taps(1), box_taps(15)
  min_3, median_1, median_3                       `rank_filter`
  gradient                                        `gradient_raster`
  smooth_u8_gauss_1.5                             `smooth_raster` of a uint8 raster

Device-event medians over rounds in which the legs are interleaved (one call of each per round). Each leg is quoted next to its
HBM-only floor at the 5.5 TB/s README.md quotes: one read and one write of the raster, 8 B per pixel for the float32 filters,
12 B for the gradient (two output planes), 2 B for uint8. The floors are ARITHMETIC, not measurements. Context, not parity, one
run each: the same smoothing as two torch `conv2d` calls over a value plane and a mask plane (float32, not bitwise reproducible,
no no-data rules beyond the mask), and `.cpu()` plus scipy.ndimage where scipy is installed.

The point of detect's `smooth` hook: `contour_lines` at 0.5 on the probability plane of the bowls scene (the plane of
tools/contours_bench.py), without and with `smooth_raster(gaussian_taps(1.5))` in front: crossings, lines and the time of each.

    python tools/focal_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/focal.json]
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

HBM_BYTES_PER_S = 5.5e12
CAPS = dict(max_lines=1 << 20, max_vertices=1 << 24)


def torch_route(r: torch.Tensor, taps: np.ndarray) -> float:
    """us of the masked smoothing by torch ops: conv2d rows then columns over [value * mask, mask], then the division."""
    k = torch.tensor(taps, dtype=torch.float32, device=r.device)
    R = len(taps) // 2

    def run():
        m = torch.isfinite(r)
        x = torch.stack([torch.where(m, r, torch.zeros_like(r)), m.to(torch.float32)])[:, None]
        x = torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1), padding=(0, R))
        x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1), padding=(R, 0))
        return x[0, 0] / x[1, 0]

    run()
    return timed(run)


def host_route(r: torch.Tensor, sigma: float) -> dict:
    """.cpu() plus scipy's normalised convolution, once."""
    try:
        from scipy import ndimage
    except ImportError:
        return {"available": False}
    t0 = time.perf_counter()
    h = r.cpu().numpy()
    t1 = time.perf_counter()
    m = np.isfinite(h)
    num = ndimage.gaussian_filter(np.where(m, h, 0.0), sigma, mode="constant")
    den = ndimage.gaussian_filter(m.astype(np.float32), sigma, mode="constant")
    with np.errstate(invalid="ignore", divide="ignore"):
        _ = num / den
    t2 = time.perf_counter()
    return {"available": True, "cpu_copy_us": (t1 - t0) * 1e6, "scipy_us": (t2 - t1) * 1e6, "total_us": (t2 - t0) * 1e6, "runs": 1}


def probability_plane(S: int, dev) -> torch.Tensor:
    """Plane 1 of predict on the bowls scene, as tools/contours_bench.py builds it."""
    img, _ = bowls(S)
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
    scene = torch.from_numpy(img).to(dev)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():
        net.outc.bias[1] += torch.log(p[0].clamp_min(1e-30) / p[1].clamp_min(1e-30)).median()
    return pred.predict(scene, return_prob=True)["prob"][1].contiguous()


def contour_case(prob: torch.Tensor, rounds: int, warmup: int) -> dict:
    from insar_unet_ca_amd import contours
    H, W = prob.shape
    sc = contours.ContourScratch(H, W, prob.device, 1, **CAPS)
    taps = iu.gaussian_taps(1.5)

    def raw():
        return iu.contour_lines(prob, [0.5], scratch=sc, **CAPS)

    def smoothed():
        s, ok = iu.smooth_raster(prob, taps, return_valid=True)
        return iu.contour_lines(s, [0.5], valid=ok, scratch=sc, **CAPS)

    res = {}
    for name, fn in (("raw", raw), ("smooth_1.5", smoothed)):
        for _ in range(warmup):
            out = fn()
        us = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            us.append((time.perf_counter() - t0) * 1e6)
        res[name] = {"call_us": median(us), "crossings": int(out["n_vertices"]), "lines": int(out["n_lines"]),
                     "closed": int(out["lines"]["closed"].sum()), "all_rounds": us}
        print(f"contour_lines at 0.5, {name}: {res[name]['crossings']} crossings in {res[name]['lines']} lines, {res[name]['call_us']:.0f} us per call",
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
        raise SystemExit("focal_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    g = torch.Generator(device="cpu").manual_seed(1)
    r = torch.randn(S, S, generator=g).to(dev)
    r[torch.rand(S, S, generator=g).to(dev) < 0.02] = float("nan")          # 2 % no-data, as a speckled raster has
    u8 = (torch.rand(S, S, generator=g) * 256).to(torch.uint8).to(dev)
    out_f, out_u8, out_g = torch.empty_like(r), torch.empty_like(u8), torch.empty(2, S, S, device=dev)
    gauss, box1, box15 = iu.gaussian_taps(1.5), iu.box_taps(1), iu.box_taps(15)
    px = float(S) * S
    legs = {
        "smooth_gauss_1.5": (lambda: iu.smooth_raster(r, gauss, out=out_f), 8.0),
        "smooth_box_1": (lambda: iu.smooth_raster(r, box1, out=out_f), 8.0),
        "smooth_box_15": (lambda: iu.smooth_raster(r, box15, out=out_f), 8.0),
        "min_3": (lambda: iu.rank_filter(r, "min", 3, out=out_f), 8.0),
        "median_1": (lambda: iu.rank_filter(r, "median", 1, out=out_f), 8.0),
        "median_3": (lambda: iu.rank_filter(r, "median", 3, out=out_f), 8.0),
        "gradient": (lambda: iu.gradient_raster(r, out=out_g), 12.0),
        "smooth_u8_gauss_1.5": (lambda: iu.smooth_raster(u8, gauss, out=out_u8), 2.0),
    }
    for _ in range(a.warmup):
        for fn, _b in legs.values():
            fn()
    t = {k: [] for k in legs}
    for _ in range(a.rounds):                                       # interleaved: one call of every leg per round
        for k, (fn, _b) in legs.items():
            t[k].append(timed(fn))
    cases = {}
    for k, (_fn, b) in legs.items():
        floor = b * px / HBM_BYTES_PER_S * 1e6
        cases[k] = {"device_us": median(t[k]), "bytes_per_pixel": b, "hbm_floor_us": floor, "over_floor": median(t[k]) / floor, "all_rounds": t[k]}
        print(f"{k}: {cases[k]['device_us']:.1f} us, floor {floor:.1f} us (arithmetic), x{cases[k]['over_floor']:.1f}", file=sys.stderr)
    out = {"device": torch.cuda.get_device_name(0), "raster": [S, S], "rounds": a.rounds, "warmup": a.warmup, "cases": cases,
           "floor": "arithmetic, not a measurement: bytes per pixel at 5.5 TB/s",
           "contours_at_0.5": contour_case(probability_plane(S, dev), a.rounds, a.warmup), "context": "not yet measured"}

    def write():
        line = json.dumps(out)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    write()                                                         # the context legs come last: what is measured is kept whatever they do
    out["context"] = {"torch_conv2d_gauss_1.5_us": torch_route(r, gauss), "torch_conv2d_box_15_us": torch_route(r, box15),
                      "host_route_gauss_1.5": host_route(r, 1.5),
                      "what": "context, not parity: one run each; float32, no no-data rules, not bitwise"}
    print(write())


if __name__ == "__main__":
    main()

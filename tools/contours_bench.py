"""Contour lines of a 4096 x 4096 raster on one GPU, in one process: `contour_lines` on

  prob      probability plane 1 of `ScenePredictor.predict` on the scene of the synthetic bowls task (UNet(use_se=True) bf16,
            seeded and untrained, its output bias moved to the median log-odds so that the 0.5 line splits the scene), level 0.5
  smooth    a smooth displacement-like float32 field (a sum of long sinusoids, in about +-40 mm), 8 levels 10 mm apart

next to things measured in the same run: `region_outlines` of the labelled arg-max map of the same prediction, `predict` of
the scene, `raster.cpu()` alone (the read-back any host contouring has to start with), and, as CONTEXT and not as parity, the
host route itself: `raster.cpu()` plus contourpy (one run; it orders its lines differently and works in float64). Device times
are medians over rounds of event pairs around each phase call (edges, lead, rank, lines, write) and around all five; `call_us`
is the host clock around the whole contour_lines call, both read-backs and the host table included. `mark_floor_us` is
ARITHMETIC, not a measurement: 4 bytes per pixel at the 5.5 TB/s of HBM the README quotes.

    python tools/contours_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/contours.json]
"""
from __future__ import annotations

import argparse
import ctypes
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
from insar_unet_ca_amd import _lib, contours, outlines  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

PHASES = ("edges", "lead", "rank", "lines", "write")
CAPS = dict(max_lines=1 << 20, max_vertices=1 << 24)
HBM_BYTES_PER_S = 5.5e12


def host_route(raster: torch.Tensor, levels) -> dict:
    """raster.cpu() plus contourpy, once: context for the device numbers, not parity."""
    try:
        import contourpy
    except ImportError:
        return {"available": False}
    t0 = time.perf_counter()
    host = raster.cpu().numpy()
    t1 = time.perf_counter()
    gen = contourpy.contour_generator(z=host)
    n_lines = n_points = 0
    for v in levels:
        ls = gen.lines(float(v))
        n_lines += len(ls)
        n_points += sum(len(a) for a in ls)
    t2 = time.perf_counter()
    return {"available": True, "cpu_copy_us": (t1 - t0) * 1e6, "contourpy_us": (t2 - t1) * 1e6, "total_us": (t2 - t0) * 1e6,
            "lines": n_lines, "points": n_points, "runs": 1}


def measure(name: str, raster: torch.Tensor, levels, scale: float, rounds: int, warmup: int) -> dict:
    H, W = raster.shape
    L = len(levels)
    sc = contours.ContourScratch(H, W, raster.device, L, **CAPS)
    kw = dict(scale=scale, scratch=sc, **CAPS)
    for _ in range(warmup):
        out = iu.contour_lines(raster, levels, **kw)
    E = out["n_vertices"]
    R, cap = sc.max_lines, sc.max_vertices
    verts = torch.empty(max(E, 1), 2, dtype=torch.int32, device=raster.device)
    lv = (ctypes.c_int32 * L)(*out["levels_q"].tolist())
    s, sp, tp = _lib.stream_ptr(), ptr(sc.scratch), ptr(sc.table)
    steps = {
        "edges": lambda: call("insar_contour_edges", ptr(raster), _lib.ZONAL_F32, H, W, float(scale), 0, 0.0, 0, lv, L, cap, sp, tp, s),
        "lead": lambda: call("insar_contour_lead", H, W, L, E, cap, sp, s),
        "rank": lambda: call("insar_contour_rank", H, W, L, E, cap, sp, s),
        "lines": lambda: call("insar_contour_lines", H, W, L, E, R, cap, sp, tp, s),
        "write": lambda: call("insar_contour_write", H, W, L, E, R, cap, sp, tp, ptr(verts), s),
    }

    def all_phases():
        for p in PHASES:
            steps[p]()

    t = {p: [] for p in PHASES}
    for k in ("device_us", "call_us", "raster_cpu_us"):
        t[k] = []
    for _ in range(rounds):                          # the phases in order: every one runs on the state the one before left
        for p in PHASES:
            t[p].append(timed(steps[p]))
        t["device_us"].append(timed(all_phases))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = iu.contour_lines(raster, levels, **kw)
        t["call_us"].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        raster.cpu()
        t["raster_cpu_us"].append((time.perf_counter() - t0) * 1e6)
    med = {k: median(v) for k, v in t.items()}
    ln = out["lines"]
    res = {"case": name, "raster": [H, W], "levels": [float(v) for v in levels], "scale": float(scale), "crossings": E,
           "crossings_per_level": out["level_counts"].tolist(), "lines": out["n_lines"], "closed": int(ln["closed"].sum()),
           "longest_line": int(ln["count"].max(initial=0)), "launches_per_call": contours.launches(E), "readbacks_per_call": 2,
           "phase_us": {p: med[p] for p in PHASES}, "device_us": med["device_us"], "call_us": med["call_us"],
           "raster_cpu_us": med["raster_cpu_us"], "call_over_raster_cpu": med["call_us"] / med["raster_cpu_us"],
           "mark_floor_us": {"value": 4.0 * H * W / HBM_BYTES_PER_S * 1e6, "what": "arithmetic, not a measurement: 4 B per pixel at 5.5 TB/s"},
           "capacities": CAPS, "scratch_bytes": int(sc.scratch.numel()), "host_route": host_route(raster, levels), "all_rounds": t}
    print(f"{name}: {E} crossings, {out['n_lines']} lines: {med['device_us']:.0f} us on the device, {med['call_us']:.0f} us per call; "
          f"raster.cpu() {med['raster_cpu_us']:.0f} us, host route {res['host_route'].get('total_us', float('nan')):.0f} us", file=sys.stderr)
    return res


def smooth_field(S: int, dev) -> torch.Tensor:
    y, x = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float64), torch.arange(S, device=dev, dtype=torch.float64), indexing="ij")
    f = 18.0 * torch.sin(x / 211.0 + 0.3) * torch.cos(y / 173.0) + 14.0 * torch.sin((x + 2 * y) / 389.0) + 9.0 * torch.cos((3 * x - y) / 617.0 + 1.1)
    return f.to(torch.float32).contiguous()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contours_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, _ = bowls(S)
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
    scene = torch.from_numpy(img).to(dev)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():
        net.outc.bias[1] += torch.log(p[0].clamp_min(1e-30) / p[1].clamp_min(1e-30)).median()
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
    res = pred.predict(scene, return_prob=True)
    prob = res["prob"][1].contiguous()

    # region_outlines of the same prediction, for comparison
    reg = iu.label_regions(res["mask"], None, connectivity=8, min_area=16)
    ocaps = dict(max_rings=1 << 20, max_vertices=1 << 24, max_edges=1 << 24)
    osc = outlines.OutlineScratch(S, S, dev, **ocaps)
    us = []
    for i in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ol = iu.region_outlines(reg["labels"], scratch=osc, **ocaps)
        if i >= a.warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    outline = {"call_us": median(us), "edges": ol["edge_count"], "rings": ol["ring_count"], "regions": reg["count"]}
    del osc

    cases = [measure("prob", prob, [0.5], 2.0 ** 16, a.rounds, a.warmup),
             measure("smooth", smooth_field(S, dev), [-35.0 + 10.0 * k for k in range(8)], 2.0 ** 16, a.rounds, a.warmup)]
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "predict_ms": predict_ms,
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16", "region_outlines": outline, "cases": cases,
           "call_share_of_predict": {c["case"]: c["call_us"] * 1e-3 / predict_ms for c in cases}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

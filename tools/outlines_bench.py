"""Outlines of a scene's regions on one GPU, in one process: `region_outlines` on the label maps of the two 4096 x 4096 class
maps of tools/regions_bench.py,

  bowls    the label maps of the synthetic bowls task, connectivity 8, min_area 16
  speckle  random foreground at 50 % fill, connectivity 4, min_area 64

next to three things measured in the same run: `label_regions` of the same class map, `ScenePredictor.predict` of the scene
the bowls mask belongs to (UNet(use_se=True) bf16, tile 256, overlap 32, batch 16), and `labels.cpu()` alone, the read-back
any host contour tracer has to start with. Device times are medians over rounds of event pairs around each phase call
(edges, lead, rank, rings, write) and around all five; `call_us` is the host clock around the whole region_outlines call, both
read-backs and the host table included.

    python tools/outlines_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/outlines.json]
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
from insar_unet_ca_amd import _lib, outlines, regions  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

PHASES = ("edges", "lead", "rank", "rings", "write")
# room for the speckle map, whose kept regions are ragged: four times the default edge and vertex slots, sixteen times the rings
CAPS = dict(max_rings=1 << 20, max_vertices=1 << 24, max_edges=1 << 24)


def measure(name: str, mask: torch.Tensor, connectivity: int, min_area: int, rounds: int, warmup: int) -> dict:
    H, W = mask.shape
    rsc = regions.RegionScratch(H, W, mask.device)
    reg = iu.label_regions(mask, None, connectivity=connectivity, min_area=min_area, scratch=rsc)
    labels = reg["labels"]
    sc = outlines.OutlineScratch(H, W, mask.device, **CAPS)
    kw = dict(connectivity=connectivity, scratch=sc, **CAPS)
    for _ in range(warmup):
        out = iu.region_outlines(labels, **kw)
    E = out["edge_count"]
    R, V, cap = sc.max_rings, sc.max_vertices, sc.max_edges
    verts = torch.empty(min(V, max(E, 1)), 2, dtype=torch.int32, device=mask.device)
    s, sp, tp = _lib.stream_ptr(), ptr(sc.scratch), ptr(sc.table)
    steps = {
        "edges": lambda: call("insar_outline_edges", ptr(labels), H, W, connectivity, cap, sp, tp, s),
        "lead": lambda: call("insar_outline_lead", H, W, E, cap, sp, s),
        "rank": lambda: call("insar_outline_rank", H, W, E, cap, sp, s),
        "rings": lambda: call("insar_outline_rings", ptr(labels), H, W, E, R, cap, sp, tp, s),
        "write": lambda: call("insar_outline_write", H, W, E, 1, R, verts.shape[0], cap, sp, tp, ptr(verts), s),
    }

    def all_phases():
        for p in PHASES:
            steps[p]()

    t = {p: [] for p in PHASES}
    for k in ("device_us", "call_us", "label_regions_us", "labels_cpu_us"):
        t[k] = []
    for _ in range(rounds):                          # the phases in order: every one runs on the state the one before left
        for p in PHASES:
            t[p].append(timed(steps[p]))
        t["device_us"].append(timed(all_phases))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = iu.region_outlines(labels, **kw)
        t["call_us"].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        iu.label_regions(mask, None, connectivity=connectivity, min_area=min_area, scratch=rsc)
        t["label_regions_us"].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        labels.cpu()
        t["labels_cpu_us"].append((time.perf_counter() - t0) * 1e6)
    med = {k: median(v) for k, v in t.items()}
    r = out["rings"]
    res = {"case": name, "scene": [H, W], "connectivity": connectivity, "min_area": min_area, "regions": reg["count"],
           "edges": E, "rings": out["ring_count"], "holes": int(r["hole"].sum()), "vertices": out["vertex_count"],
           "longest_ring": int(r["edges"].max(initial=0)), "launches_per_call": outlines.launches(E), "readbacks_per_call": 2,
           "phase_us": {p: med[p] for p in PHASES}, "device_us": med["device_us"], "call_us": med["call_us"],
           "label_regions_call_us": med["label_regions_us"], "labels_cpu_us": med["labels_cpu_us"],
           "capacities": CAPS, "scratch_bytes": int(sc.scratch.numel()), "call_over_labels_cpu": med["call_us"] / med["labels_cpu_us"], "all_rounds": t}
    print(f"{name}: {E} edges, {out['ring_count']} rings: {med['device_us']:.0f} us on the device, {med['call_us']:.0f} us per "
          f"call; label_regions {med['label_regions_us']:.0f} us, labels.cpu() {med['labels_cpu_us']:.0f} us", file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("outlines_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    mask = torch.from_numpy(lab).to(dev)
    rng.random((S, S))                               # regions_bench draws its confidence field first: the same speckle
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    cases = [measure("bowls", mask, 8, 16, a.rounds, a.warmup), measure("speckle", speckle, 4, 64, a.rounds, a.warmup)]

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

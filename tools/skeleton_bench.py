"""Centre lines of a scene's regions on one GPU, in one process: `thin_regions` on the label maps of the two 4096 x 4096 class
maps of tools/regions_bench.py,

  bowls    the label maps of the synthetic bowls task, connectivity 8, min_area 16
  speckle  random foreground at 50 % fill, connectivity 4, min_area 64

next to two things measured in the same run: `label_regions` of the same class map and `ScenePredictor.predict` of the scene
the bowls mask belongs to (UNet(use_se=True) bf16, tile 256, overlap 32, batch 16). Device times are medians over rounds of
event pairs around each phase (planes, every step launch, stats, the distance transform) and around all of them; `call_us` is
the host clock around the whole thin_regions call, the read-back of the table and the host conversion included.

    python tools/skeleton_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--max-iterations 32] [--out profiles/skeleton.json]
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
from insar_unet_ca_amd import _lib, regions, skeletons  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

MAX_REGIONS = 1 << 20                    # room for the speckle map's kept regions


def measure(name: str, mask: torch.Tensor, connectivity: int, min_area: int, rounds: int, warmup: int, mi: int) -> dict:
    H, W = mask.shape
    rsc = regions.RegionScratch(H, W, mask.device, MAX_REGIONS)
    reg = iu.label_regions(mask, None, connectivity=connectivity, min_area=min_area, max_regions=MAX_REGIONS, scratch=rsc)
    labels = reg["labels"]
    sc = skeletons.SkeletonScratch(H, W, mask.device, mi, MAX_REGIONS)
    kw = dict(max_iterations=mi, max_regions=MAX_REGIONS, scratch=sc)
    for _ in range(warmup):
        out = iu.thin_regions(labels, **kw)
    nsteps = skeletons.launches(H, W, mi, False) - 2
    skel = torch.empty(H, W, dtype=torch.uint8, device=mask.device)
    s, sp, tp = _lib.stream_ptr(), ptr(sc.scratch), ptr(sc.table)
    dist = lambda: iu.distance_transform(labels, sites="edge", max_distance=mi + 2, scratch=sc.distance_scratch())["d2"]
    d2 = dist()
    steps = {"distance": dist,
             "planes": lambda: call("insar_skeleton_planes", ptr(labels), H, W, mi, MAX_REGIONS, sp, tp, s)}
    for k in range(nsteps):
        steps[f"step{k}"] = (lambda k: lambda: call("insar_skeleton_step", H, W, mi, k, sp, s))(k)
    steps["stats"] = lambda: call("insar_skeleton_stats", ptr(labels), ptr(d2), H, W, mi, MAX_REGIONS, sp, tp, ptr(skel), s)
    phases = tuple(steps)

    def all_phases():
        for p in phases:
            steps[p]()

    t = {p: [] for p in phases}
    for k in ("device_us", "call_us", "label_regions_us"):
        t[k] = []
    for _ in range(rounds):                          # the phases in order: every one runs on the state the one before left
        for p in phases:
            t[p].append(timed(steps[p]))
        t["device_us"].append(timed(all_phases))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = iu.thin_regions(labels, **kw)
        t["call_us"].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        iu.label_regions(mask, None, connectivity=connectivity, min_area=min_area, max_regions=MAX_REGIONS, scratch=rsc)
        t["label_regions_us"].append((time.perf_counter() - t0) * 1e6)
    med = {k: median(v) for k, v in t.items()}
    tab = out["table"]
    res = {"case": name, "scene": [H, W], "connectivity": connectivity, "min_area": min_area, "regions": reg["count"],
           "max_iterations": mi, "iterations": out["iterations"], "converged": out["converged"],
           "skeleton_pixels": int(out["stats"]["n"].sum()), "ends": int(tab["n_end"].sum()), "junctions": int(tab["n_junction"].sum()),
           "total_length": float(tab["length"].sum()), "launches_per_call": skeletons.launches(H, W, mi, True), "readbacks_per_call": 1,
           "phase_us": {p: med[p] for p in phases}, "device_us": med["device_us"], "call_us": med["call_us"],
           "label_regions_call_us": med["label_regions_us"], "max_regions": MAX_REGIONS, "scratch_bytes": int(sc.scratch.numel()),
           "all_rounds": t}
    print(f"{name}: {res['skeleton_pixels']} skeleton pixels after {out['iterations']} iterations: {med['device_us']:.0f} us on the "
          f"device, {med['call_us']:.0f} us per call; label_regions {med['label_regions_us']:.0f} us", file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-iterations", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skeleton_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    mask = torch.from_numpy(lab).to(dev)
    rng.random((S, S))                               # regions_bench draws its confidence field first: the same speckle
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    mi = a.max_iterations
    cases = [measure("bowls", mask, 8, 16, a.rounds, a.warmup, mi), measure("speckle", speckle, 4, 64, a.rounds, a.warmup, mi)]

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

"""Outline simplification on one GPU, in one process: `simplify_outlines` at tolerances 0, 1 and 2 on the outlines (every
lattice vertex, corners_only=False) of the two 4096 x 4096 class maps of tools/regions_bench.py,

  bowls    the label maps of the synthetic bowls task, connectivity 8, min_area 16
  speckle  random foreground at 50 % fill, connectivity 4, min_area 64

with the label map (shared borders) and without, next to three things measured in the same run: `region_outlines` of the same
label map, `ScenePredictor.predict` of the scene the bowls mask belongs to (UNet(use_se=True) bf16, tile 256, overlap 32,
batch 16), and the host route: `vertices.cpu()` plus a numpy Douglas-Peucker per ring with the same integer rule (seeds,
threshold, ties by coordinate; without anchors, which a host library does not have either). Device times are medians over
rounds of event pairs around setup, all rounds that the call issued, and finish; `call_us` is the host clock around the whole
`simplify_outlines` call, its counter read-backs and the table read-back included.

    python tools/simplify_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--host-rings 2000] [--out profiles/simplify.json]
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
from insar_unet_ca_amd import _lib, outlines, regions, simplify  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

TOLERANCES = (0.0, 1.0, 2.0)
CAPS = dict(max_rings=1 << 20, max_vertices=1 << 24, max_edges=1 << 24)


def host_ring(c: np.ndarray, q2: int) -> np.ndarray:
    """Kept mask of one ring (int64 [n, 2]) by the rule of include/insar_hip.h without anchors, with an explicit stack."""
    n = len(c)
    key = c[:, 0] * 65536 + c[:, 1]
    s1 = int(np.argmin(key))
    d2 = ((c - c[s1]) ** 2).sum(1)
    far = np.flatnonzero(d2 == d2.max())
    s2 = int(far[np.argmin(key[far])])
    keep = np.zeros(n, dtype=bool)
    keep[[s1, s2]] = True
    rot = np.concatenate([c[s1:], c[:s1 + 1]])                   # starts and ends at seed 1: no segment wraps
    kr = np.zeros(n + 1, dtype=bool)
    b = (s2 - s1) % n
    kr[[0, b, n]] = True
    stack = [(0, b), (b, n)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        d, p = rot[hi] - rot[lo], rot[lo + 1:hi] - rot[lo]
        len2 = int(d @ d)
        num = (d[1] * p[:, 0] - d[0] * p[:, 1]) ** 2 if len2 else (p * p).sum(1)
        m = int(num.max())
        if not 256 * m > q2 * (len2 or 1):
            continue
        cand = np.flatnonzero(num == m)
        k = rot[lo + 1:hi][cand]
        w = lo + 1 + int(cand[np.argmin(k[:, 0] * 65536 + k[:, 1])])
        kr[w] = True
        stack += [(lo, w), (w, hi)]
    keep[(np.flatnonzero(kr[:n]) + s1) % n] = True
    return keep


def host_route(raw: dict, tolerance: float, max_rings: int) -> dict:
    """vertices.cpu() plus the numpy rule over the first `max_rings` rings; the time is scaled to all vertices."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v = raw["vertices"].cpu().numpy().astype(np.int64)
    t_copy = time.perf_counter() - t0
    q2 = simplify.eps2q(tolerance)
    r = raw["rings"]
    n = min(max_rings, len(r["start"]))
    done = kept = 0
    t0 = time.perf_counter()
    for i in range(n):
        s, c = int(r["start"][i]), int(r["count"][i])
        kept += int(host_ring(v[s:s + c], q2).sum())
        done += c
    t_dp = time.perf_counter() - t0
    return {"vertices_cpu_us": t_copy * 1e6, "rings_done": n, "vertices_done": done, "kept_of_done": kept, "dp_us": t_dp * 1e6,
            "dp_us_scaled_to_all": t_dp * 1e6 * len(v) / max(done, 1)}


def measure(name: str, mask: torch.Tensor, connectivity: int, min_area: int, rounds: int, warmup: int, host_rings: int) -> dict:
    H, W = mask.shape
    reg = iu.label_regions(mask, None, connectivity=connectivity, min_area=min_area, scratch=regions.RegionScratch(H, W, mask.device))
    labels = reg["labels"]
    osc = outlines.OutlineScratch(H, W, mask.device, **CAPS)
    okw = dict(connectivity=connectivity, corners_only=False, scratch=osc, **CAPS)
    raw = iu.region_outlines(labels, **okw)
    V, R = raw["vertex_count"], raw["ring_count"]
    ssc = simplify.SimplifyScratch(V, R, H, W, mask.device)
    t_out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iu.region_outlines(labels, **okw)
        t_out.append((time.perf_counter() - t0) * 1e6)
    res = {"case": name, "scene": [H, W], "connectivity": connectivity, "min_area": min_area, "regions": reg["count"], "rings": R,
           "vertices_in": V, "corner_vertices": iu.region_outlines(labels, connectivity=connectivity, scratch=osc, **CAPS)["vertex_count"],
           "region_outlines_call_us": median(t_out), "scratch_bytes": int(ssc.scratch.numel()), "runs": []}
    s, sp, tp, ip = _lib.stream_ptr(), ptr(ssc.scratch), ptr(ssc.table), ptr(ssc.table_in)
    out_v = torch.empty(V, 2, dtype=torch.int32, device=mask.device)
    out_k = torch.empty(V, dtype=torch.int32, device=mask.device)
    for tol in TOLERANCES:
        for lab in (labels, None):
            for _ in range(warmup):
                out = iu.simplify_outlines(raw, lab, tolerance=tol, scratch=ssc)
            issued = min(-(-(out["rounds"] + 1) // simplify.ROUNDS_PER_READ) * simplify.ROUNDS_PER_READ, simplify.DEFAULT_MAX_ROUNDS + 1)
            q2, mr, v = simplify.eps2q(tol), simplify.DEFAULT_MAX_ROUNDS, raw["vertices"]
            steps = {     # table_in still holds this input's rings from the warm-up calls
                "setup": lambda: call("insar_simplify_setup", ptr(v), V, ip, R, ptr(lab), H if lab is not None else 0,
                                      W if lab is not None else 0, V, R, sp, s),
                "rounds": lambda: call("insar_simplify_rounds", ptr(v), V, ip, R, q2, 0, issued, mr, V, R, sp, s),
                "finish": lambda: call("insar_simplify_finish", ptr(v), V, ip, R, mr, V, R, sp, tp, ptr(out_v), ptr(out_k), s),
            }

            def all_steps():
                for f in steps.values():
                    f()

            t = {k: [] for k in ("setup", "rounds", "finish", "device_us", "call_us")}
            for _ in range(rounds):
                for k, f in steps.items():
                    t[k].append(timed(f))
                t["device_us"].append(timed(all_steps))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = iu.simplify_outlines(raw, lab, tolerance=tol, scratch=ssc)
                t["call_us"].append((time.perf_counter() - t0) * 1e6)
            med = {k: median(x) for k, x in t.items()}
            run = {"tolerance": tol, "with_labels": lab is not None, "rounds": out["rounds"], "rounds_issued": issued,
                   "converged": out["converged"], "vertices_out": out["vertex_count"], "collapsed_rings": int(out["rings"]["collapsed"].sum()),
                   "launches": simplify.launches(issued), "phase_us": {k: med[k] for k in steps}, "device_us": med["device_us"],
                   "call_us": med["call_us"], "device_over_region_outlines": med["device_us"] / res["region_outlines_call_us"], "all_rounds": t}
            if lab is None:
                run["host"] = host_route(raw, tol, host_rings)
                run["host_over_device"] = (run["host"]["vertices_cpu_us"] + run["host"]["dp_us_scaled_to_all"]) / med["device_us"]
            res["runs"].append(run)
            print(f"{name} tol {tol} labels {lab is not None}: {V} -> {out['vertex_count']} vertices in {out['rounds']} rounds: "
                  f"{med['device_us']:.0f} us on the device, {med['call_us']:.0f} us per call", file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rings", type=int, default=2000, help="rings the host route simplifies; its time is scaled to all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simplify_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    mask = torch.from_numpy(lab).to(dev)
    rng.random((S, S))                               # regions_bench draws its confidence field first: the same speckle
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    cases = [measure("bowls", mask, 8, 16, a.rounds, a.warmup, a.host_rings),
             measure("speckle", speckle, 4, 64, a.rounds, a.warmup, a.host_rings)]

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
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16", "tolerances": list(TOLERANCES), "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

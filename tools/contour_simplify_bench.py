"""`simplify_contours` on the contour lines of the two 4096 x 4096 cases of tools/contours_bench.py, on one GPU, in one process:

  prob         the 0.5 line of probability plane 1 of `ScenePredictor.predict` on the bowls scene (the model of contours_bench)
  prob_smooth  the same plane behind `smooth_raster(gaussian_taps(1.5))`
  smooth       the smooth displacement-like field at 8 levels

at the tolerances 0, 0.25 and 1 pixel. Device times are medians over rounds of event pairs around each phase (setup, all
rounds the host route would issue, finish) and around all three; `call_us` is the host clock around the whole
`simplify_contours` call, the counter read-backs and the table included. Next to them, measured in the same run:
`contour_lines` of the same raster (host clock around the call), and the host route, as CONTEXT and not as parity: `vertices.cpu()`
plus a numpy Douglas-Peucker with the same rule (float64 cross products, one run, on at most `--host-lines` of the longest lines;
the vertices it covers are recorded). `round_floor_us` is ARITHMETIC, not a measurement: the bytes one round has to move when every
vertex is still undecided, at the 5.5 TB/s of HBM the README quotes.

    python tools/contour_simplify_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/contour_simplify.json]
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
from insar_unet_ca_amd import _lib, contours  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.contours_bench import CAPS, HBM_BYTES_PER_S, smooth_field  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

TOLERANCES = (0.0, 0.25, 1.0)
MAX_ROUNDS = 64
# one round with every vertex undecided: the keep flag read (1), the vertex read (8), its line (4), seg (4) and the deviation (8)
# written in `cross` and read again in `tie`, `pos` and `keep` (3 * 12), the other parity's slots reset (20)
ROUND_BYTES_PER_VERTEX = 1 + 8 + 4 + 12 + 3 * 12 + 20


def host_douglas_peucker(pts: np.ndarray, closed: bool, eps2: float) -> int:
    """Kept vertices of one line by the rule of simplify_contours, iteratively, in float64."""
    n = len(pts)
    if closed:
        s1 = int(np.lexsort((pts[:, 1], pts[:, 0]))[0])
        d2 = ((pts - pts[s1]) ** 2).sum(1)
        s2 = int(np.argmax(d2))
        a, b = sorted((s1, s2))
        pts = np.concatenate([pts[a:], pts[:a + 1]])             # start at a seed; the other one is at b - a
        stack, kept = [(0, b - a), (b - a, n)], 2
    else:
        stack, kept = [(0, n - 1)], 2
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        d, p = pts[b] - pts[a], pts[a + 1:b] - pts[a]
        len2 = float(d @ d)
        dev = np.abs(d[1] * p[:, 0] - d[0] * p[:, 1]) if len2 else (p ** 2).sum(1)
        k = int(np.argmax(dev))
        if (dev[k] * dev[k] > eps2 * len2) if len2 else (dev[k] > eps2):
            kept += 1
            stack += [(a, a + 1 + k), (a + 1 + k, b)]
    return kept


def host_route(c: dict, tolerance: float, max_lines: int) -> dict:
    t0 = time.perf_counter()
    v = c["vertices"].cpu().numpy().astype(np.float64)
    t1 = time.perf_counter()
    ln = c["lines"]
    order = np.argsort(-ln["count"])[:max_lines]
    eps2 = float(contours.eps_q(tolerance)) ** 2
    kept = covered = 0
    for i in order:
        s, n = int(ln["start"][i]), int(ln["count"][i])
        kept += host_douglas_peucker(v[s:s + n], bool(ln["closed"][i]), eps2)
        covered += n
    t2 = time.perf_counter()
    return {"cpu_copy_us": (t1 - t0) * 1e6, "numpy_dp_us": (t2 - t1) * 1e6, "lines": int(len(order)), "vertices": covered,
            "kept": kept, "runs": 1}


def measure(name: str, raster: torch.Tensor, levels, valid, rounds: int, warmup: int, host_lines: int) -> dict:
    H, W = raster.shape
    csc = contours.ContourScratch(H, W, raster.device, len(levels), **CAPS)
    kw = dict(valid=valid, scratch=csc, **CAPS)
    us = []
    for i in range(warmup + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = iu.contour_lines(raster, levels, **kw)
        if i >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    V, R = c["n_vertices"], c["n_lines"]
    res = {"case": name, "raster": [H, W], "levels": [float(v) for v in levels], "vertices": V, "lines": R,
           "closed": int(c["lines"]["closed"].sum()), "longest_line": int(c["lines"]["count"].max(initial=0)),
           "contour_lines_call_us": median(us),
           "round_floor_us": {"value": ROUND_BYTES_PER_VERTEX * V / HBM_BYTES_PER_S * 1e6,
                              "what": f"arithmetic, not a measurement: {ROUND_BYTES_PER_VERTEX} B per vertex at 5.5 TB/s"},
           "tolerances": []}
    sc = contours.ContourSimplifyScratch(V, R, raster.device)
    res["scratch_bytes"] = int(sc.scratch.numel())
    v = c["vertices"]
    out_v, out_k = torch.empty(V, 2, dtype=torch.int32, device=v.device), torch.empty(V, dtype=torch.int32, device=v.device)
    s, sp, tp, ip = _lib.stream_ptr(), ptr(sc.scratch), ptr(sc.table), ptr(sc.table_in)
    for tol in TOLERANCES:
        for _ in range(warmup):
            out = iu.simplify_contours(c, tolerance=tol, max_rounds=MAX_ROUNDS, scratch=sc)
        issued = min(MAX_ROUNDS + 1, -(-(out["rounds"] + 1) // contours.ROUNDS_PER_READ) * contours.ROUNDS_PER_READ)
        eps2 = contours.eps_q(tol) ** 2
        steps = {
            "setup": lambda: call("insar_contour_simplify_setup", ptr(v), V, ip, R, V, R, sp, s),
            "rounds": lambda: call("insar_contour_simplify_rounds", ptr(v), V, ip, R, eps2, 0, issued, MAX_ROUNDS, V, R, sp, s),
            "finish": lambda: call("insar_contour_simplify_finish", ptr(v), V, ip, R, MAX_ROUNDS, V, R, sp, tp, ptr(out_v), ptr(out_k), s),
        }

        def all_phases():
            for p in steps:
                steps[p]()

        t = {p: [] for p in steps}
        t["device_us"], t["call_us"] = [], []
        for _ in range(rounds):                      # the phases in order: every one runs on the state the one before left
            for p in steps:
                t[p].append(timed(steps[p]))
            t["device_us"].append(timed(all_phases))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = iu.simplify_contours(c, tolerance=tol, max_rounds=MAX_ROUNDS, scratch=sc)
            t["call_us"].append((time.perf_counter() - t0) * 1e6)
        med = {k: median(x) for k, x in t.items()}
        row = {"tolerance": tol, "vertices_after": out["n_vertices"], "rounds": out["rounds"], "rounds_issued": issued,
               "converged": out["converged"], "collapsed": int(out["lines"]["collapsed"].sum()),
               "launches": contours.contour_simplify_launches(issued), "phase_us": {p: med[p] for p in steps},
               "device_us": med["device_us"], "call_us": med["call_us"], "host_route": host_route(c, tol, host_lines), "all_rounds": t}
        res["tolerances"].append(row)
        print(f"{name} tol {tol}: {V} -> {out['n_vertices']} vertices in {R} lines, {out['rounds']} rounds: {med['device_us']:.0f} us on "
              f"the device, {med['call_us']:.0f} us per call (contour_lines {res['contour_lines_call_us']:.0f} us)", file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-lines", type=int, default=2000, help="the host route simplifies this many of the longest lines")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contour_simplify_bench: needs a ROCm device (a CPU run gives no time)")
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
    prob = pred.predict(scene, return_prob=True)["prob"][1].contiguous()
    sm, sm_valid = iu.smooth_raster(prob, iu.gaussian_taps(1.5), return_valid=True)
    cases = [measure("prob", prob, [0.5], None, a.rounds, a.warmup, a.host_lines),
             measure("prob_smooth", sm, [0.5], sm_valid, a.rounds, a.warmup, a.host_lines),
             measure("smooth", smooth_field(S, dev), [-35.0 + 10.0 * k for k in range(8)], None, a.rounds, a.warmup, a.host_lines)]
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "max_rounds": MAX_ROUNDS,
           "rounds_per_read": contours.ROUNDS_PER_READ, "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

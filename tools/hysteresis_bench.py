"""Hysteresis thresholds on one GPU, in one process: `hysteresis_regions` of a 4096 x 4096 two-plane probability map built
from the bowls class map of tools/regions_bench.py, its bumps blurred (two 25-pixel box filters) so that their flanks lie
below 0.5, at low 0.2 / high 0.8, connectivity 8, min_area 16: phase by phase and as a whole call, next to `label_regions` of
the arg-max map and `ScenePredictor.predict` of the same scene measured in the same run, interleaved round by round, with the
HBM-only floors of the new pixel passes at 5.5 TB/s. The floors are arithmetic, not measurements: classify reads 4 B per pixel
and class plane and writes 1 + 4 B, seeds reads 4 + 1 + 4 B, apply reads 4 + 1 B and writes 4 + 1 B. If scipy is importable, the
host route a user has today is timed as context, not parity (prob.cpu(), a threshold, scipy.ndimage.label, np.maximum.at for
the per-component peak, a look-up for the kept components).

`classify_us`, `label_us` (the seven labelling launches), `seeds_keep_apply_us` (the clear, seeds, keep and apply launches):
events around those launches alone, median over rounds. `device_us`: events around all 12 launches with no read-back between
them. `call_us`: the host clock around the whole hysteresis_regions call.

    python tools/hysteresis_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/hysteresis.json]
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
from insar_unet_ca_amd import _lib, hysteresis  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from insar_unet_ca_amd.regions import RegionScratch  # noqa: E402
from insar_unet_ca_amd.regions import _launch as label_launch  # noqa: E402
from regions_bench import bowls, median, timed  # noqa: E402

MAX_REGIONS = 65536
HBM_BYTES_PER_US = 5.5e6                                          # 5.5 TB/s
LOW, HIGH, CONN, MIN_AREA = 0.2, 0.8, 8, 16


def blurred_prob(lab: torch.Tensor) -> torch.Tensor:
    """float32 [2, H, W]: p(site) is the class map under two 25-pixel box filters, p(background) the rest."""
    p = lab.float()[None, None]
    for _ in range(2):
        p = torch.nn.functional.avg_pool2d(p, 25, stride=1, padding=12, count_include_pad=True)
    p = p[0, 0].clamp_(0, 1)
    return torch.stack([1 - p, p]).contiguous()


def host_path(prob: torch.Tensor) -> dict:
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p = prob[1].cpu().numpy()
    t1 = time.perf_counter()
    lab, n = ndimage.label(p >= np.float32(LOW), structure=np.ones((3, 3), dtype=bool))
    t2 = time.perf_counter()
    peak = np.full(n + 1, -np.inf, dtype=np.float32)
    np.maximum.at(peak, lab.ravel(), p.ravel())
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = (peak >= np.float32(HIGH)) & (area >= MIN_AREA)
    keep[0] = False
    out = np.where(keep[lab], lab, 0)
    t3 = time.perf_counter()
    return {"copy_us": (t1 - t0) * 1e6, "label_us": (t2 - t1) * 1e6, "peak_and_keep_us": (t3 - t2) * 1e6, "total_us": (t3 - t0) * 1e6,
            "components": int(n), "kept": int(keep.sum()), "labelled_pixels": int((out > 0).sum())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hysteresis_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    prob = blurred_prob(torch.from_numpy(lab).to(dev))
    argmax = (prob[1] > prob[0]).to(torch.uint8)
    conf = prob.max(dim=0).values.contiguous()
    H = W = S

    sc = hysteresis.HysteresisScratch(H, W, dev, MAX_REGIONS)
    kw = dict(connectivity=CONN, min_area=MIN_AREA, max_regions=MAX_REGIONS, scratch=sc)
    rsc = RegionScratch(H, W, dev, MAX_REGIONS)
    rkw = dict(connectivity=CONN, min_area=MIN_AREA, max_regions=MAX_REGIONS, scratch=rsc)
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
    scene = torch.from_numpy(img).to(dev)
    for _ in range(max(1, a.warmup)):
        out = iu.hysteresis_regions(prob, LOW, HIGH, **kw)
        plain = iu.label_regions(argmax, conf, **rkw)
        pred.predict(scene)

    s = _lib.stream_ptr()
    labels, mask, cplane = torch.empty_like(out["labels"]), torch.empty_like(out["mask"]), torch.empty_like(out["conf"])
    thr, planes = sc.thresholds, prob.data_ptr() + 4 * H * W

    def classify():
        call("insar_hyst_classify", planes, 1, H, W, ptr(thr), None, ptr(sc.cand), ptr(cplane), s)

    def label():
        label_launch(sc.cand, cplane, CONN, MIN_AREA, float("-inf"), MAX_REGIONS, sc.regions.scratch, sc.regions.table, labels, mask)

    def tail():
        call("insar_hyst_seeds", ptr(labels), ptr(sc.cand), ptr(cplane), ptr(thr), H, W, MAX_REGIONS, ptr(sc.scratch), s)
        call("insar_hyst_keep", ptr(sc.regions.table), 1, MAX_REGIONS, ptr(sc.scratch), ptr(sc.table), s)
        call("insar_hyst_apply", ptr(sc.cand), H, W, MAX_REGIONS, ptr(sc.scratch), ptr(labels), ptr(mask), s)

    def launches():
        classify()
        label()
        tail()

    t = {k: [] for k in ("classify_us", "label_us", "seeds_keep_apply_us", "device_us", "call_us", "label_regions_call_us", "predict_ms")}
    for _ in range(a.rounds):                                     # interleaved: every figure sees the same minutes of the machine
        t["classify_us"].append(timed(classify))
        t["label_us"].append(timed(label))
        t["seeds_keep_apply_us"].append(timed(tail))
        t["device_us"].append(timed(launches))
        for name, fn, scale in (("call_us", lambda: iu.hysteresis_regions(prob, LOW, HIGH, **kw), 1e6),
                                ("label_regions_call_us", lambda: iu.label_regions(argmax, conf, **rkw), 1e6),
                                ("predict_ms", lambda: pred.predict(scene), 1e3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * scale)
    assert torch.equal(labels, out["labels"]) and torch.equal(mask, out["mask"])
    npix = H * W
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "map": [H, W], "low": LOW, "high": HIGH,
           "connectivity": CONN, "min_area": MIN_AREA, "max_regions": MAX_REGIONS, "launches": hysteresis.LAUNCHES, "read_backs": 1,
           "regions": out["count"], "candidates": out["candidates"], "labelled_pixels": int((out["labels"] > 0).sum()),
           "argmax_regions": plain["count"], "argmax_labelled_pixels": int((plain["labels"] > 0).sum()),
           **{k: median(v) for k, v in t.items()},
           "classify_floor_us": 9 * npix / HBM_BYTES_PER_US, "seeds_floor_us": 9 * npix / HBM_BYTES_PER_US,
           "apply_floor_us": 10 * npix / HBM_BYTES_PER_US, "floors": "arithmetic at 5.5 TB/s, not measurements",
           "table_readback_bytes": int(sc.table.numel()), "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16",
           "all_rounds": t}
    res["classify_over_floor"] = res["classify_us"] / res["classify_floor_us"]
    res["seeds_keep_apply_over_floor"] = res["seeds_keep_apply_us"] / (res["seeds_floor_us"] + res["apply_floor_us"])
    try:
        import scipy  # noqa: F401
        res["host_path"] = host_path(prob)
    except ImportError:
        res["host_path"] = "not yet measured (scipy is not importable here)"
    print(f"hysteresis: {res['regions']} sites of {res['candidates']} candidates ({res['argmax_regions']} arg-max regions); classify "
          f"{res['classify_us']:.0f} us ({res['classify_over_floor']:.1f} x floor), label {res['label_us']:.0f} us, seeds + keep + apply "
          f"{res['seeds_keep_apply_us']:.0f} us ({res['seeds_keep_apply_over_floor']:.1f} x floor), device {res['device_us']:.0f} us, call "
          f"{res['call_us']:.0f} us; label_regions call {res['label_regions_call_us']:.0f} us, predict {res['predict_ms']:.0f} ms",
          file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Polygon rasterisation on one GPU, in one process: `rasterise_polygons` (int32 and uint8) on a 4096 x 4096 scene over the
polygons of the two label maps of tools/regions_bench.py (bowls: connectivity 8, min_area 16; speckle: connectivity 4,
min_area 64), obtained through `label_regions` -> `region_outlines` -> `to_polygons` -> `pack_polygons`, next to
`label_regions` and `ScenePredictor.predict` of the same scene and to a host route plus upload.

`device_us` is the median over rounds of an event pair around the five launches, `call_us` the host clock round the whole
`rasterise_polygons` call with a synchronise (allocation of the map and the scratch included; `call_scratch_us` with a reused
RasterScratch). `pack_us` is the host packer, once. The result is checked against the label map it came from. The host route
burns the same polygons with PIL.ImageDraw.polygon (exterior, then holes with 0) when PIL imports, and uploads the map; its
fill rule is PIL's own scanline rule on vertices rounded to whole pixels, not the top-left rule at 1/256 pixel, so its map is
NOT bitwise ours (`host_route.differs` counts the pixels). Without PIL the upload alone is reported.

    python tools/rasterise_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/rasterise.json]
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
from insar_unet_ca_amd import rasterise as rs  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def host_route(polys, want: np.ndarray, dev) -> dict:
    H, W = want.shape
    res = {"upload_bytes": int(want.nbytes)}
    host = torch.from_numpy(want)
    res["upload_us"] = median([wall(lambda: host.to(dev)) for _ in range(5)])
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        res["rule"] = "none: PIL does not import here, the upload alone is reported"
        return res
    t0 = time.perf_counter()
    img = Image.new("I", (W, H), 0)
    draw = ImageDraw.Draw(img)
    for e in polys:
        for p in e["polygons"]:
            draw.polygon([(float(x), float(y)) for y, x in p["exterior"]], fill=int(e["label"]))
            for h in p["holes"]:
                draw.polygon([(float(x), float(y)) for y, x in h], fill=0)
    got = np.asarray(img, dtype=np.int32)
    res["burn_us"] = (time.perf_counter() - t0) * 1e6
    res["total_us"] = res["burn_us"] + res["upload_us"]
    res["rule"] = "PIL.ImageDraw.polygon: PIL's scanline fill, holes painted over with 0; not the top-left rule"
    res["differs"] = int((got != want).sum())
    return res


def measure(name: str, mask: torch.Tensor, connectivity: int, min_area: int, rounds: int, warmup: int) -> dict:
    H, W = mask.shape
    dev = mask.device
    for _ in range(warmup):
        reg = iu.label_regions(mask, connectivity=connectivity, min_area=min_area)
    label_us = median([wall(lambda: iu.label_regions(mask, connectivity=connectivity, min_area=min_area)) for _ in range(rounds)])
    labels = reg["labels"]
    outl = iu.region_outlines(labels, connectivity=connectivity, max_edges=1 << 26, max_vertices=1 << 26, max_rings=1 << 22)
    polys = iu.to_polygons(outl)
    t0 = time.perf_counter()
    table = iu.pack_polygons(polys)
    pack_us = (time.perf_counter() - t0) * 1e6
    n_cross = table.crossings(H)
    scratch = iu.RasterScratch(H, W, dev, n_cross)
    want = labels.cpu().numpy()
    res = {"case": name, "scene": [H, W], "connectivity": connectivity, "min_area": min_area, "regions": reg["count"],
           "rings": outl["ring_count"], "edges": len(table), "crossings": n_cross, "band_rows": rs.band_rows(W),
           "launches_per_call": rs.launches(), "pack_us": pack_us, "label_regions_us": label_us}
    for dt, key in ((torch.int32, "int32"), (torch.uint8, "uint8")):
        run = lambda: iu.rasterise_polygons(table, H, W, dtype=dt, device=dev, scratch=scratch)
        for _ in range(warmup):
            out = run()
        if dt == torch.int32:
            res["round_trip_exact"] = bool((out["labels"].cpu().numpy() == want).all())
            res["overlap_pixels"] = int(out["overlap_pixels"])
        res[key] = {"device_us": median([timed(run) for _ in range(rounds)]),
                    "call_scratch_us": median([wall(run) for _ in range(rounds)]),
                    "call_us": median([wall(lambda: iu.rasterise_polygons(table, H, W, dtype=dt, device=dev)) for _ in range(rounds)])}
    res["host_route"] = host_route(polys, want, dev)
    print(f"{name}: {res['edges']} edges, {n_cross} crossings, int32 {res['int32']['device_us']:.0f} us on the device, "
          f"{res['int32']['call_us']:.0f} us per call, exact {res['round_trip_exact']}", file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rasterise_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    rng.random((S, S))                                   # the draw regions_bench.py spends on its confidence field
    mask = torch.from_numpy(lab).to(dev)
    speckle = torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev)
    cases = [measure("bowls", mask, 8, 16, a.rounds, a.warmup), measure("speckle", speckle, 4, 64, a.rounds, a.warmup)]
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
    scene = torch.from_numpy(img).to(dev)
    for _ in range(a.warmup):
        pred.predict(scene)
    predict_ms = median([wall(lambda: pred.predict(scene)) for _ in range(max(3, a.rounds // 2))]) * 1e-3
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup, "predict_ms": predict_ms,
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16", "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

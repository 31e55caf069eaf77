"""Sieving class maps on one GPU, in one process: `sieve_regions` of the two 4096 x 4096 maps of tools/regions_bench.py,

  bowls    the bowls task's class map, connectivity 8, min_area {1: 64, 0: 16} (drop small sites, fill small holes)
  speckle  the adversarial case: random classes at 50 % fill, connectivity 4, min_area 64 for both classes (a million regions)

phase by phase and as a whole call, next to `label_regions` and `ScenePredictor.predict` of the same scene measured in the same
run, with the HBM-only floors of the two pixel passes at 5.5 TB/s. The floors are arithmetic, not measurements: the pairs pass
reads 4 B per pixel of labels (its clear and compact launches also write and read the pair table, 16 B per slot and 2^k >= 2
max_pairs slots, `pair_table_bytes`: max_pairs is 2^20 for bowls and 2^22 for speckle, which has 3.7 million pairs), the apply
pass reads 4 B of labels and 1 B of the class map and writes 1 B. If scipy is
importable, the start of the host route a user has today is timed as context (labels.cpu(), scipy.ndimage.label per class,
areas by bincount, find_objects); the Python loop over the small regions that follows it is not, so the figure is a lower bound.

`pairs_us`, `rounds_us` (the piece state and one batch of four rounds), `apply_us`, `label_us` (remap and the seven labelling
launches): events around those launches alone, median over rounds. `device_us`: events around all launches of one sieve with no
read-back between them. `call_us`: the host clock around the whole sieve_regions call.

    python tools/sieve_bench.py [--size 4096] [--rounds 5] [--warmup 2] [--out profiles/sieve.json]
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
from insar_unet_ca_amd import _lib, sieve  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from insar_unet_ca_amd.regions import _launch as label_launch  # noqa: E402
from regions_bench import bowls, median, timed  # noqa: E402

MAX_REGIONS = 1 << 22
HBM_BYTES_PER_US = 5.5e6                                          # 5.5 TB/s


def host_path(mask: torch.Tensor, connectivity: int) -> dict:
    from scipy import ndimage
    structure = np.ones((3, 3), dtype=bool) if connectivity == 8 else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mask.cpu().numpy()
    t1 = time.perf_counter()
    n_all = 0
    for c in np.unique(m):
        lab, n = ndimage.label(m == c, structure=structure)
        np.bincount(lab.ravel(), minlength=n + 1)
        ndimage.find_objects(lab, max_label=n)
        n_all += n
    t2 = time.perf_counter()
    return {"copy_us": (t1 - t0) * 1e6, "label_area_boxes_us": (t2 - t1) * 1e6, "total_us": (t2 - t0) * 1e6, "regions": int(n_all),
            "not_included": "the Python loop over the small regions (neighbour search and rewrite per region)"}


def measure(name: str, mask: torch.Tensor, min_area, connectivity: int, max_pairs: int, rounds: int, warmup: int, with_host: bool) -> dict:
    H, W = mask.shape
    dev = mask.device
    sc = sieve.SieveScratch(H, W, dev, MAX_REGIONS, max_pairs, 64)
    kw = dict(min_area=min_area, connectivity=connectivity, max_regions=MAX_REGIONS, max_pairs=max_pairs, scratch=sc)
    for _ in range(max(1, warmup)):
        out = iu.sieve_regions(mask, **kw)
    batches = max(1, -(-(out["rounds"] + 1) // sieve.ROUNDS_PER_READ))
    pairs_found = int(sc.state_host.numpy()[:8].view(np.int32)[0])
    s = _lib.stream_ptr()
    labels, cleaned = torch.empty_like(out["labels_in"]), torch.empty_like(mask)
    args = (MAX_REGIONS, max_pairs, 64, ptr(sc.scratch))
    thr = sc.thresholds

    def label():
        call("insar_sieve_remap", ptr(mask), H, W, 255, *args, s)
        label_launch(sc.remap, None, connectivity, 1, 0.0, MAX_REGIONS, sc.regions.scratch, sc.regions.table, labels, cleaned)

    def pairs():
        call("insar_sieve_pairs", ptr(labels), H, W, MAX_REGIONS, *args, s)

    def batch(b=0):
        call("insar_sieve_rounds", ptr(sc.regions.table), ptr(mask), ptr(thr), H, W, b * sieve.ROUNDS_PER_READ, sieve.ROUNDS_PER_READ,
             *args, s)

    def apply():
        call("insar_sieve_apply", ptr(labels), ptr(mask), H, W, *args, ptr(cleaned), None, s)

    def launches():
        label()
        pairs()
        for b in range(batches):
            batch(b)
        apply()

    t = {k: [] for k in ("label_us", "pairs_us", "rounds_us", "apply_us", "device_us", "call_us")}
    for _ in range(rounds):
        t["label_us"].append(timed(label))
        t["pairs_us"].append(timed(pairs))
        t["rounds_us"].append(timed(batch))
        t["apply_us"].append(timed(apply))
        t["device_us"].append(timed(launches))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = iu.sieve_regions(mask, **kw)
        t["call_us"].append((time.perf_counter() - t0) * 1e6)
    assert torch.equal(cleaned, out["mask"])
    npix = H * W
    res = {"case": name, "map": [H, W], "connectivity": connectivity, "min_area": {str(k): v for k, v in min_area.items()},
           "regions_in": out["regions_in"], "pairs": pairs_found, "absorbed": out["absorbed"], "changed_pixels": out["changed_pixels"],
           "rounds": out["rounds"], "converged": out["converged"], "launches": 12 + 1 + 3 * sieve.ROUNDS_PER_READ * batches,
           **{k: median(v) for k, v in t.items()},
           "pairs_floor_us": 4 * npix / HBM_BYTES_PER_US, "apply_floor_us": 6 * npix / HBM_BYTES_PER_US,
           "floors": "arithmetic at 5.5 TB/s, not measurements", "max_pairs": max_pairs,
           "pair_table_bytes": 32 * (1 << (2 * max_pairs - 1).bit_length()) // 2, "scratch_bytes": int(sc.scratch.numel()), "all_rounds": t}
    res["pairs_over_floor"] = res["pairs_us"] / res["pairs_floor_us"]
    res["apply_over_floor"] = res["apply_us"] / res["apply_floor_us"]
    if with_host:
        res["host_path"] = host_path(mask, connectivity)
    print(f"{name}: {res['regions_in']} regions, {res['pairs']} pairs, {res['absorbed']} absorbed in {res['rounds']} rounds; label "
          f"{res['label_us']:.0f} us, pairs {res['pairs_us']:.0f} us ({res['pairs_over_floor']:.1f} x floor), four rounds "
          f"{res['rounds_us']:.0f} us, apply {res['apply_us']:.0f} us ({res['apply_over_floor']:.1f} x floor), device "
          f"{res['device_us']:.0f} us, call {res['call_us']:.0f} us"
          + (f"; host route >= {res['host_path']['total_us']:.0f} us" if with_host else ""), file=sys.stderr)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sieve_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    img, lab = bowls(S)
    rng = np.random.default_rng(0)
    maps = {"bowls": (torch.from_numpy(lab).to(dev), {1: 64, 0: 16}, 8, 1 << 20, dict(connectivity=8, min_area=16)),
            "speckle": (torch.from_numpy((rng.random((S, S)) < 0.5).astype(np.uint8)).to(dev), {1: 64, 0: 64}, 4,
                        1 << 22, dict(connectivity=4, min_area=64))}
    try:
        import scipy  # noqa: F401
        with_host = True
    except ImportError:
        with_host = False

    cases = []
    for name, (m, min_area, conn, max_pairs, kw) in maps.items():
        for _ in range(max(1, a.warmup)):
            iu.label_regions(m, None, max_regions=MAX_REGIONS, **kw)
        us = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            iu.label_regions(m, None, max_regions=MAX_REGIONS, **kw)
            us.append((time.perf_counter() - t0) * 1e6)
        res = measure(name, m, min_area, conn, max_pairs, a.rounds, a.warmup, with_host)
        res["label_regions_call_us"] = median(us)
        cases.append(res)

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
           "predict_model": "UNet(use_se=True) bf16, tile 256, overlap 32, batch 16",
           "host_path": "labels.cpu(), scipy.ndimage.label per class, bincount, find_objects (context and a lower bound)" if with_host
                        else "not yet measured (scipy is not importable here)", "cases": cases}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

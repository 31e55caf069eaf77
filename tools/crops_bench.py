"""Training from scenes on one GPU, in one process: a 4096 x 4096 uint8 scene with the bowls task's label map, K = 2,
cell 8 and cell 1, batches of 16 x 256 x 256.

  index_build_us      CropIndex: insar_crops_cells + insar_crops_sat (3 launches), with the table's bytes
  batch_us            one batch: insar_crops_draw + insar_crops_gather (2 launches; images float32 + masks int64)
  torch_index_us      the same table by torch ops on the device (one-hot planes, reshape-sum, two cumsums)
  torch_batch_us      a batch by torch ops at the SAME origins (indexed gather of images and masks, the normalisation):
                      the draw itself has no torch form without a read-back, so this leg is the gather alone
  host_route          what a user does today: .cpu() of scene and labels (once), then per batch numpy rejection sampling
                      (up to `tries` uniform origins per sample, counted by slicing) + slicing + .to(device)

Device times are medians over rounds of event pairs around the calls (no read-back inside), the least and the largest round
beside them. They are recorded next to the training step they must hide behind (6.6 - 6.9 ms, profiles/r04_bench.json).

    python tools/crops_bench.py [--size 4096] [--rounds 9] [--warmup 3] [--out profiles/crops.json]
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
from insar_unet_ca_amd import crops  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

K, TILE, BATCH, TRIES = 2, 256, 16, 16


def rounds(fn, n: int, warmup: int) -> dict:
    for _ in range(warmup):
        fn()
    v = [timed(fn) for _ in range(n)]
    return {"median_us": round(median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def torch_index(labels: torch.Tensor, g: int) -> torch.Tensor:
    H, W = labels.shape
    Hc, Wc = H // g, W // g
    lab = labels[:Hc * g, :Wc * g]
    planes = [(lab == p) for p in range(K)] + [lab >= K]
    cells = torch.stack([p.reshape(Hc, g, Wc, g).sum(dim=(1, 3), dtype=torch.int32) for p in planes])
    table = torch.zeros(K + 1, Hc + 1, Wc + 1, dtype=torch.int32, device=labels.device)
    table[:, 1:, 1:] = cells.cumsum(1, dtype=torch.int32).cumsum(2, dtype=torch.int32)
    return table


def torch_batch(scene: torch.Tensor, labels: torch.Tensor, origins: torch.Tensor):
    ar = torch.arange(TILE, device=scene.device)
    ys = (origins[:, 0:1].long() + ar)[:, :, None]
    xs = (origins[:, 1:2].long() + ar)[:, None, :]
    x = scene[ys, xs].float().div_(255.0).sub_(0.5).div_(0.5)[:, None]
    return x, labels[ys, xs].long()


def host_batch(scene: np.ndarray, labels: np.ndarray, rng, min_count: int, max_void: int, device):
    H, W = labels.shape
    xs, ms = [], []
    for _ in range(BATCH):
        cls = int(rng.integers(0, K))
        for _ in range(TRIES):
            y, x = int(rng.integers(0, H - TILE + 1)), int(rng.integers(0, W - TILE + 1))
            box = labels[y:y + TILE, x:x + TILE]
            if int((box == cls).sum()) >= min_count and int((box >= K).sum()) <= max_void:
                break
        xs.append(scene[y:y + TILE, x:x + TILE])
        ms.append(box)
    x = (np.stack(xs).astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    return torch.from_numpy(x[:, None]).to(device), torch.from_numpy(np.stack(ms).astype(np.int64)).to(device)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    img, lab = bowls(a.size)
    scene_np = np.clip((img * 0.5 + 0.5) * 255.0, 0, 255).astype(np.uint8)
    lab[: a.size // 16, : a.size // 8] = 255                               # a void corner, so that the void plane is not empty
    scene, labels = torch.from_numpy(scene_np).to(dev), torch.from_numpy(lab).to(dev)
    min_count, max_void = crops.count_limits(TILE, 0.01, 0.5)
    cum = crops.cumulative([1.0] * K)
    res = {"scene": [a.size, a.size], "num_classes": K, "tile": TILE, "batch": BATCH, "tries": TRIES, "rounds": a.rounds,
           "class_fraction": [float((lab == p).mean()) for p in range(K)], "void_fraction": float((lab >= K).mean()),
           "min_count": min_count, "max_void": max_void, "step_ms_to_hide_behind": [6.6, 6.9], "cells": {}}
    for g in (8, 1):
        idx = iu.CropIndex(labels, K, cell=g)
        same = bool(torch.equal(idx.table, torch_index(labels, g)))
        step = [0]

        def batch():
            origins, _ = iu.draw_crops(idx, crops.batch_key(0, 0, step[0]), BATCH, TILE, cum, min_count, max_void, TRIES)
            step[0] += 1
            return iu.gather_crops(scene, labels, origins, TILE)

        origins, info = iu.draw_crops(idx, crops.batch_key(0, 0, 0), BATCH, TILE, cum, min_count, max_void, TRIES)
        x, m = iu.gather_crops(scene, labels, origins, TILE)
        tx, tm = torch_batch(scene, labels, origins)
        leg = {"table_bytes": idx.nbytes, "torch_table_equal": same,
               "torch_batch_equal": bool(torch.equal(m, tm) and torch.allclose(x, tx, atol=1e-6)),
               "accepted_of_first_batch": int((info[:, 1] >= 0).sum()),
               "index_build_us": rounds(lambda: iu.CropIndex(labels, K, cell=g), a.rounds, a.warmup),
               "batch_us": rounds(batch, a.rounds, a.warmup),
               "draw_us": rounds(lambda: iu.draw_crops(idx, 1, BATCH, TILE, cum, min_count, max_void, TRIES), a.rounds, a.warmup),
               "gather_us": rounds(lambda: iu.gather_crops(scene, labels, origins, TILE), a.rounds, a.warmup),
               "torch_index_us": rounds(lambda: torch_index(labels, g), a.rounds, a.warmup),
               "torch_batch_us": rounds(lambda: torch_batch(scene, labels, origins), a.rounds, a.warmup)}
        res["cells"][str(g)] = leg
        del idx
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s_host, l_host = scene.cpu().numpy(), labels.cpu().numpy()
    t1 = time.perf_counter()
    rng = np.random.default_rng(0)
    per = []
    for _ in range(a.rounds):
        t = time.perf_counter()
        host_batch(s_host, l_host, rng, min_count, max_void, dev)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t) * 1e6)
    res["host_route"] = {"copy_to_host_once_us": round((t1 - t0) * 1e6, 1), "batch_us": {"median_us": round(median(per), 1),
                         "min_us": round(min(per), 1), "max_us": round(max(per), 1)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

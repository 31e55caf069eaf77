"""Whole-scene inference on one GPU, in one process: a seeded synthetic uint8 scene through ScenePredictor with
UNet(use_se=True) bf16 (seeded weights), tile 256, overlap 32, batch 16.

Records (a) ms per scene and tiles/s end to end (host clock around predict + device synchronise); (b) the three scene
kernels per scene by device events (every launch of a scene between one pair of events, so the launch gaps between the
per-batch launches are inside the figure), with the algorithmic bytes of each and the achieved GB/s against the HBM figures
of BASELINE.md (8.0 TB/s spec, 6.29 TB/s measured); (c) the same stitch (clear, softmax, window, slice-add per tile,
divide, max / argmax) written with torch ops on the same logits, interleaved round by round with ours.

    python tools/scene_bench.py [--size 4096] [--rounds 5] [--warmup 2] [--out profiles/scene_predict.json]
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
from insar_unet_ca_amd import infer  # noqa: E402

HBM_SPEC_TBS, HBM_MEASURED_TBS = 8.0, 6.29


def algorithmic_bytes(origins: np.ndarray, H: int, W: int, K: int, T: int, batch: int) -> dict:
    N = len(origins)
    covered = 0                                   # pixels whose acc / wsum a batch reads and writes, summed over batches
    for i in range(0, N, batch):
        m = np.zeros((H, W), dtype=bool)
        for y, x in origins[i:i + batch]:
            m[y:y + T, x:x + T] = True
        covered += int(m.sum())
    return {"gather": N * T * T * (1 + 4),
            "blend": N * K * T * T * 4 + covered * (K + 1) * 4 * 2,
            "finalize": (K + 1) * H * W * 4 + (K + 1) * H * W * 4 + H * W,
            "clear": (K + 1) * H * W * 4}


def timed(fn) -> float:
    """ms between two events on the current stream around fn()."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_stitch(logits, origins, H, W, T, w2, batch):
    """The stitch a user would write around the modules today."""
    K = logits.shape[1]
    acc = torch.zeros(K, H, W, dtype=torch.float32, device=logits.device)
    wsum = torch.zeros(H, W, dtype=torch.float32, device=logits.device)
    for i in range(0, len(origins), batch):
        p = torch.softmax(logits[i:i + batch], 1) * w2
        for j, (y, x) in enumerate(origins[i:i + batch]):
            acc[:, y:y + T, x:x + T] += p[j]
            wsum[y:y + T, x:x + T] += w2
    prob = acc / wsum
    conf, mask = prob.max(0)
    return prob, conf, mask.to(torch.uint8)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    H = W = a.size
    T, o, B, K = a.tile, a.overlap, a.batch, 2
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=K, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    scene = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(H, W), dtype=np.uint8)).to(dev)
    origins = iu.plan_tiles(H, W, T, o)
    N = len(origins)
    o_dev = torch.from_numpy(origins).to(dev)
    pred = iu.ScenePredictor(net, tile=T, overlap=o, batch=B, num_classes=K)
    for _ in range(a.warmup):
        pred.predict(scene)
    torch.cuda.synchronize()

    # the logits of the scene once, for the kernel timings and the torch-op baseline
    with torch.no_grad():
        tiles = torch.empty(B, 1, T, T, dtype=torch.float32, device=dev)
        logits = torch.cat([net(infer.gather_tiles(scene, o_dev[i:i + B], T, out=tiles[:min(B, N - i)])).float()
                            for i in range(0, N, B)])
    buf, acc, wsum = infer._accumulators(K, H, W, dev)
    w2 = torch.from_numpy(np.outer(iu.window_1d(T, o), iu.window_1d(T, o))).to(dev)

    def gather_all():
        for i in range(0, N, B):
            infer.gather_tiles(scene, o_dev[i:i + B], T, out=tiles[:min(B, N - i)])

    def blend_all():
        for i in range(0, N, B):
            infer._blend(logits[i:i + B], origins, o_dev, i, K, T, o, acc, wsum)

    fin = {}

    def finalize():
        fin.update(infer._finalize(acc, wsum, True))

    def ours():
        buf.zero_()
        blend_all()
        finalize()

    base = {}

    def theirs():
        base["prob"], base["conf"], base["mask"] = torch_stitch(logits, origins, H, W, T, w2, B)

    for _ in range(a.warmup):
        gather_all(), ours(), theirs()
    torch.cuda.synchronize()
    agree = float((fin["prob"] - base["prob"]).abs().max())
    mask_diff = int((fin["mask"] != base["mask"]).sum())

    t = {k: [] for k in ("scene_ms", "gather_ms", "clear_ms", "blend_ms", "finalize_ms", "stitch_ms", "torch_stitch_ms")}
    for _ in range(a.rounds):                        # interleaved: every round measures every leg
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred.predict(scene)
        torch.cuda.synchronize()
        t["scene_ms"].append((time.perf_counter() - t0) * 1e3)
        t["gather_ms"].append(timed(gather_all))
        t["clear_ms"].append(timed(buf.zero_))
        t["blend_ms"].append(timed(blend_all))
        t["finalize_ms"].append(timed(finalize))
        t["stitch_ms"].append(timed(ours))
        t["torch_stitch_ms"].append(timed(theirs))
    med = {k: median(v) for k, v in t.items()}
    nbytes = algorithmic_bytes(origins, H, W, K, T, B)
    kernels = {}
    for name in ("gather", "clear", "blend", "finalize"):
        gbs = nbytes[name] / (med[name + "_ms"] * 1e-3) / 1e9
        kernels[name] = {"ms_per_scene": med[name + "_ms"], "algorithmic_bytes": nbytes[name], "GBps": gbs,
                         "of_hbm_spec_8.0TBps": gbs / (HBM_SPEC_TBS * 1e3), "of_hbm_measured_6.29TBps": gbs / (HBM_MEASURED_TBS * 1e3),
                         "launches_per_scene": 1 if name in ("clear", "finalize") else (N + B - 1) // B}
    stitch_share = (med["gather_ms"] + med["stitch_ms"]) / med["scene_ms"]
    out = {"scene": [H, W], "scene_dtype": "uint8", "model": "UNet(use_se=True) bf16", "tile": T, "overlap": o, "batch": B,
           "num_classes": K, "tiles": N, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ms_per_scene": med["scene_ms"], "tiles_per_s": N / (med["scene_ms"] * 1e-3),
           "kernels": kernels,
           "stitch_ms": med["stitch_ms"], "torch_stitch_ms": med["torch_stitch_ms"],
           "torch_over_ours": med["torch_stitch_ms"] / med["stitch_ms"],
           "gather_plus_stitch_share_of_scene": stitch_share,
           "torch_vs_ours_max_abs_prob_diff": agree, "torch_vs_ours_mask_pixels_differing": mask_diff,
           "all_rounds": t}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Detections through a stack of dates on one GPU, in one process: a 4096 x 4096 grid, words = 1, 64 dates.

  push1      one date (class map + confidence) into a stack that holds others: read-modify-write of one plane of hit and valid
  push64     64 dates in one call: the plane is written whole and not read
  shift      the oldest date dropped
  summary    all eight planes; `persistent` alone (min_run = 1: no run scan; min_run = 3: with it)
  series     `site_series` on the persistent map's regions of a synthetic bowls stack, and on one region covering the map
  follow     a whole `follow_sites` call (summary, label_regions, series, two read-backs)

The bowls stack: the label map of the bowls task (tools/regions_bench.py) is the footprint; at each date 85 % of the pixels
are observed, a footprint pixel is a hit with probability 0.9 from its own onset date on, any pixel with 0.03.

`device_us`: events around `reps` back-to-back launches, divided by reps, median over rounds. `floor_us`: the bytes the call
must move (stated per case in `bytes_spec`) at the 5.5 TB/s the repository's streaming kernels report (README): an HBM-only
bound; 268 MB of planes do not fit the 256 MB Infinity Cache together with the inputs. `torch_us`: the same result by torch
ops on the device (bit tests per date). `host`: the route a user has today (state to the host, numpy over the dates), measured
on a 1024 x 1024 crop and scaled by 16 (context, not parity).

    python tools/stack_bench.py [--size 4096] [--rounds 7] [--reps 10] [--warmup 2] [--out profiles/stack.json]
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
from insar_unet_ca_amd import _lib, stack  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from regions_bench import bowls, median, timed  # noqa: E402

STREAM_BYTES_PER_S = 5.5e12          # README: the streaming kernels of this repository, HBM-bound
RULE = dict(min_hits=8, min_run=3, min_valid=16, min_fraction=(1, 4))
T = 64


def many(fn, reps):
    def run():
        for _ in range(reps):
            fn()
    return run


def device_us(fn, rounds, reps, warmup):
    for _ in range(warmup):
        fn()
    us = [timed(many(fn, reps)) / reps for _ in range(rounds)]
    return median(us), us


def case(name, fn, nbytes, what, rounds, reps, warmup, torch_fn=None):
    d, allr = device_us(fn, rounds, reps, warmup)
    floor = nbytes / STREAM_BYTES_PER_S * 1e6
    res = {"case": name, "device_us": d, "bytes_spec": int(nbytes), "bytes_are": what, "floor_us": floor, "over_floor": d / floor,
           "all_rounds": allr}
    if torch_fn is not None:
        res["torch_us"], _ = device_us(torch_fn, max(3, rounds // 2), 1, 1)
    print(f"{name}: {d:.1f} us, {d / floor:.2f} x the floor of {floor:.1f} us" + (f"; torch ops {res['torch_us']:.0f} us" if torch_fn else ""),
          file=sys.stderr)
    return res


def torch_summary(hit, valid, with_runs):
    """n_valid, n_hit (and the longest run with its start) by bit tests per date: what torch offers without a kernel."""
    h, v = hit[0] & valid[0], valid[0]
    z = lambda: torch.zeros_like(h, dtype=torch.int16)
    n_valid, n_hit, best, cur = z(), z(), z(), z()
    for t in range(T):
        vb, hb = ((v >> t) & 1).to(torch.int16), ((h >> t) & 1).to(torch.int16)
        n_valid += vb
        n_hit += hb
        if with_runs:
            cur = torch.where(vb == 1, (cur + hb) * hb, cur)
            best = torch.maximum(best, cur)
    return n_valid, n_hit, best


def host_route(st, crop):
    """State to the host, then numpy over the dates (the scan of tests/stack_ref.py, without first / last)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hit, valid = st.hit.cpu().numpy().view(np.uint64), st.valid.cpu().numpy().view(np.uint64)
    t1 = time.perf_counter()
    h, v = hit[0, :crop, :crop] & valid[0, :crop, :crop], valid[0, :crop, :crop]
    n_valid, n_hit = np.zeros(h.shape, np.int16), np.zeros(h.shape, np.int16)
    best, cur = np.zeros(h.shape, np.int16), np.zeros(h.shape, np.int16)
    for t in range(T):
        vb, hb = ((v >> np.uint64(t)) & np.uint64(1)).astype(np.int16), ((h >> np.uint64(t)) & np.uint64(1)).astype(np.int16)
        n_valid += vb
        n_hit += hb
        cur = np.where(vb == 1, (cur + hb) * hb, cur)
        best = np.maximum(best, cur)
    t2 = time.perf_counter()
    scale = (st.H * st.W) / float(crop * crop)
    return {"copy_us": (t1 - t0) * 1e6, "crop": crop, "scan_crop_us": (t2 - t1) * 1e6, "scan_scaled_us": (t2 - t1) * 1e6 * scale,
            "total_scaled_us": (t1 - t0) * 1e6 + (t2 - t1) * 1e6 * scale}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stack_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    npix = S * S
    _, lab = bowls(S)
    foot = torch.from_numpy(lab != 0).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda: torch.rand(S, S, device=dev, generator=g)
    onset = (rnd() * (T // 2)).to(torch.int16)
    masks = torch.empty(T, S, S, dtype=torch.uint8, device=dev)
    for t in range(T):
        hit = (foot & (onset <= t) & (rnd() < 0.9)) | (rnd() < 0.03)
        masks[t] = torch.where(rnd() < 0.85, hit.to(torch.uint8), torch.full_like(hit, 255, dtype=torch.uint8))
    conf = (0.5 + 0.5 * rnd()).contiguous()
    st = iu.DetectionStack(S, S, dev, 1)
    st.push(masks)
    s = _lib.stream_ptr()
    R = stack.DEFAULT_MAX_REGIONS
    kw = (a.rounds, a.reps, a.warmup)
    cw = stack.class_words(1)
    cases = []

    def push(n, t, c):
        call("insar_stack_push", ptr(masks), None, ptr(c), 0.6, cw[0], cw[1], cw[2], cw[3], 255, n, t, 1, S, S, ptr(st.hit), ptr(st.valid), s)

    def torch_push1():
        v = masks[5] != 255
        h = v & (masks[5] == 1) & (conf >= 0.6)
        bit = 1 << 5
        st.hit[0] = (st.hit[0] & ~bit) | (h.to(torch.int64) << 5)
        st.valid[0] = (st.valid[0] & ~bit) | (v.to(torch.int64) << 5)

    keep = (st.hit.clone(), st.valid.clone())
    cases.append(case("push1", lambda: push(1, 5, conf), npix * (1 + 4 + 32), "mask 1 + conf 4 + hit and valid read and written 32 per pixel",
                      *kw, torch_fn=torch_push1))
    cases.append(case("push64", lambda: push(64, 0, None), npix * (64 + 16), "64 class maps 64 + hit and valid written 16 per pixel", *kw))
    cases.append(case("shift", lambda: call("insar_stack_shift", ptr(st.hit), ptr(st.valid), 1, S, S, 1, s), npix * 32,
                      "hit and valid read and written 32 per pixel", *kw))
    st.hit.copy_(keep[0])
    st.valid.copy_(keep[1])
    st.n_dates = T
    del keep

    planes = {p: torch.empty(S, S, dtype=stack._PLANE_DTYPE[p], device=dev) for p in stack.SUMMARY_PLANES}

    def summary(want, min_run):
        call("insar_stack_summary", ptr(st.hit), ptr(st.valid), 1, S, S, 0, T, RULE["min_hits"], min_run, RULE["min_valid"], 1, 4,
             *[ptr(planes[p]) if p in want else None for p in stack.SUMMARY_PLANES], s)

    cases.append(case("summary_all", lambda: summary(stack.SUMMARY_PLANES, 3), npix * (16 + 14), "hit and valid 16 + six int16 and two uint8 planes 14",
                      *kw, torch_fn=lambda: torch_summary(st.hit, st.valid, True)))
    cases.append(case("summary_persistent_no_runs", lambda: summary(("persistent",), 1), npix * 17, "hit and valid 16 + one uint8 plane", *kw,
                      torch_fn=lambda: torch_summary(st.hit, st.valid, False)))
    cases.append(case("summary_persistent_runs", lambda: summary(("persistent",), 3), npix * 17, "hit and valid 16 + one uint8 plane", *kw))

    out = iu.follow_sites(st, min_area=16, **RULE)
    sc = stack.StackScratch(dev, R, T)
    one = torch.ones(S, S, dtype=torch.int32, device=dev)

    def series(labels):
        call("insar_stack_series_clear", ptr(sc.table), R, T, s)
        call("insar_stack_series", ptr(st.hit), ptr(st.valid), 1, ptr(labels), S, S, 0, T, R, ptr(sc.table), s)

    def torch_series(labels, count):
        flat = labels.reshape(-1).to(torch.int64)
        h, v = (st.hit[0] & st.valid[0]).reshape(-1), st.valid[0].reshape(-1)
        for t in range(T):
            torch.bincount(flat, weights=((h >> t) & 1).to(torch.float64), minlength=count + 1)
            torch.bincount(flat, weights=((v >> t) & 1).to(torch.float64), minlength=count + 1)

    clear_us, _ = device_us(lambda: call("insar_stack_series_clear", ptr(sc.table), R, T, s), *kw)
    for name, labels, count in (("series_bowls", out["labels"], out["count"]), ("series_single", one, 1)):
        c = case(name, lambda: series(labels), npix * 20, "labels 4 + hit and valid 16 per pixel (under background only the label is read)", *kw,
                 torch_fn=lambda: torch_series(labels, count))
        c.update(regions=int(count), labelled_share=float((labels > 0).float().mean()), clear_us=clear_us, series_us=c["device_us"] - clear_us,
                 series_over_floor=(c["device_us"] - clear_us) / c["floor_us"], table_bytes=int(sc.table.numel()))
        cases.append(c)

    call_us = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iu.follow_sites(st, min_area=16, scratch=sc, **RULE)
        call_us.append((time.perf_counter() - t0) * 1e6)
    follow = {"case": "follow_sites", "call_us": median(call_us), "all_rounds": call_us, "regions": int(out["count"]),
              "persistent_share": float(out["summary"]["persistent"].float().mean()), "rule": {k: list(v) if isinstance(v, tuple) else v for k, v in RULE.items()},
              "floor_us": npix * (30 + 20) / STREAM_BYTES_PER_S * 1e6, "floor_is": "summary_all + series; label_regions and the read-backs not counted"}
    print(f"follow_sites: {follow['call_us']:.0f} us per call, {follow['regions']} sites", file=sys.stderr)
    res = {"device": torch.cuda.get_device_name(0), "grid": [S, S], "words": 1, "dates": T, "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup,
           "stream_bytes_per_s_assumed": STREAM_BYTES_PER_S, "cases": cases, "follow_sites": follow, "host": host_route(st, min(1024, S))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

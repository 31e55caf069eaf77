"""Grey-scale reconstruction on 4096 x 4096 float32 rasters on one GPU, in one process:

  fill_sinks         the bowls scene of tools/regions_bench.py as a displacement-like field (5 cm of amplitude on a gentle ramp)
  h_dome             the probability plane of predict on that scene, h = 0.2
  regional_extrema   the smooth 8-level field of tools/contours_bench.py, maxima

Per case: device-event medians over rounds in which the cases are interleaved, for the whole call (with its read-backs of the
round counters) and for the three phases launched back to back without a read-back (prepare, `rounds` round launches, finish);
`rounds`; the share of tile-rounds that were active; the wall time per call. In the same run, for scale: `smooth_raster` under
gaussian_taps(1.5) and `predict` of the same scene.

The floor is ARITHMETIC, not a measurement: 12 B per pixel (J read, G read, J written) per ACTIVE tile-round at the 5.5 TB/s
README.md quotes, plus prepare (12 B per pixel: the raster read, two key planes written) and finish (the key plane and the
raster read and 4 B written per output plane: 16 B for fill_sinks with its depth, 12 B for h_dome; regional_extrema is counted
as two key planes read and 1 B written, 9 B).

Context, not parity, ONE run: `.cpu()` plus the Jacobi iteration of tests/reconstruct_ref.py on a 1024 x 1024 crop of the h_dome
case (full size would take minutes), given up after --host-seconds.

    python tools/reconstruct_bench.py [--size 4096] [--rounds 7] [--warmup 2] [--out profiles/reconstruct.json]
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
from insar_unet_ca_amd import _lib, reconstruct as rc  # noqa: E402
from insar_unet_ca_amd._lib import call, ptr  # noqa: E402
from tools.contours_bench import smooth_field  # noqa: E402
from tools.regions_bench import bowls, median, timed  # noqa: E402

HBM_BYTES_PER_S = 5.5e12
F32 = _lib.ZONAL_F32


def scene_and_probability(S: int, dev):
    """(the bowls scene, the predictor, plane 1 of predict on it), as tools/focal_bench.py builds them."""
    img, _ = bowls(S)
    torch.manual_seed(0)
    net = iu.UNet(in_channels=1, num_classes=2, use_se=True, compute_dtype=torch.bfloat16).to(dev).eval()
    pred = iu.ScenePredictor(net, tile=256, overlap=32, batch=16, num_classes=2)
    scene = torch.from_numpy(img).to(dev)
    p = pred.predict(scene, return_prob=True)["prob"]
    with torch.no_grad():
        net.outc.bias[1] += torch.log(p[0].clamp_min(1e-30) / p[1].clamp_min(1e-30)).median()
    return scene, pred, pred.predict(scene, return_prob=True)["prob"][1].contiguous()


def phases(raster, mode, flip, h, rounds, scratch, outs):
    """us of prepare, of `rounds` round launches and of finish, each between two events, nothing read back."""
    H, W = raster.shape
    s, buf = _lib.stream_ptr(), ptr(scratch.scratch)
    t_prepare = timed(lambda: call("insar_reconstruct_prepare", None, ptr(raster), F32, 1, H, W, mode, flip, 8, h, rounds, 0, 0.0, None, buf, s))
    t_rounds = timed(lambda: call("insar_reconstruct_rounds", 1, H, W, 8, 0, rounds, buf, s))
    t_finish = timed(lambda: call("insar_reconstruct_finish", None, ptr(raster), F32, 1, H, W, mode, flip, 0, 0.0, None, rounds, 0, buf,
                                  ptr(outs.get("out")), ptr(outs.get("residue")), ptr(outs.get("extrema")), None, s))
    return t_prepare, t_rounds, t_finish


def host_route(prob: torch.Tensor, h: float, crop: int, seconds: float) -> dict:
    """.cpu() plus a whole-raster Jacobi iteration in numpy on a crop, once; given up after `seconds`."""
    from tests import reconstruct_ref as ref
    t0 = time.perf_counter()
    z = prob[:crop, :crop].contiguous().cpu().numpy()
    t1 = time.perf_counter()
    J, G, _ok = ref.prepare(ref.HDOME, z, h=h)
    J, G = J[0], G[0]
    H, W = J.shape
    its, finished = 0, False
    while time.perf_counter() - t1 < seconds:
        p = np.pad(J, 1, constant_values=0)
        m = J
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                m = np.maximum(m, p[dy:dy + H, dx:dx + W])
        new = np.minimum(G, m)
        its += 1
        if np.array_equal(new, J):
            finished = True
            break
        J = new
    t2 = time.perf_counter()
    return {"crop": [crop, crop], "cpu_copy_us": (t1 - t0) * 1e6, "jacobi_us": (t2 - t1) * 1e6, "iterations": its, "finished": finished,
            "runs": 1}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reconstruct_bench: needs a ROCm device (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = a.size
    scene, pred, prob = scene_and_probability(S, dev)
    ramp = torch.arange(S, device=dev, dtype=torch.float32) * 1e-5
    disp = (0.05 * scene + ramp[None, :]).contiguous()
    field = smooth_field(S, dev)
    scratch = rc.ReconstructScratch(S, S, 1, dev)
    T = rc.reconstruct_tile()
    tiles = ((S + T - 1) // T) ** 2
    out_f, out_d, out_e = torch.empty_like(disp), torch.empty_like(disp), torch.empty(S, S, dtype=torch.uint8, device=dev)
    gauss = iu.gaussian_taps(1.5)
    # name -> (the public call, the raster, mode, flip, h, the outputs of finish, bytes per pixel of prepare + finish)
    cases = {
        "fill_sinks": (lambda: iu.fill_sinks(disp, return_depth=True, return_info=True, scratch=scratch, out=out_f),
                       disp, _lib.RECONSTRUCT_FILL, 1, 0.0, {"out": out_f, "residue": out_d}, 12.0 + 16.0),
        "h_dome": (lambda: iu.h_dome(prob, 0.2, return_info=True, scratch=scratch, out=out_d),
                   prob, _lib.RECONSTRUCT_HDOME, 0, 0.2, {"residue": out_d}, 12.0 + 12.0),
        "regional_extrema": (lambda: iu.regional_extrema(field, "max", return_info=True, scratch=scratch, out=out_e),
                             field, _lib.RECONSTRUCT_EXTREMA, 0, 0.0, {"extrema": out_e}, 12.0 + 9.0),
    }
    info = {}
    for _ in range(max(1, a.warmup)):
        for k, c in cases.items():
            info[k] = c[0]()[-1]
        iu.smooth_raster(scene, gauss, out=out_f)
        pred.predict(scene)
    t = {k: {"call": [], "wall": [], "prepare": [], "rounds": [], "finish": []} for k in cases}
    other = {"smooth_raster_gauss_1.5": [], "predict": []}
    for _ in range(a.rounds):                                       # interleaved: one call of every leg per round
        for k, c in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t[k]["call"].append(timed(c[0]))
            torch.cuda.synchronize()
            t[k]["wall"].append((time.perf_counter() - t0) * 1e6)
            p, r, f = phases(c[1], c[2], c[3], c[4], info[k]["rounds"], scratch, c[5])
            t[k]["prepare"].append(p), t[k]["rounds"].append(r), t[k]["finish"].append(f)
        other["smooth_raster_gauss_1.5"].append(timed(lambda: iu.smooth_raster(scene, gauss, out=out_f)))
        other["predict"].append(timed(lambda: pred.predict(scene)))
    px = float(S) * S
    res = {}
    for k, c in cases.items():
        rounds, active = info[k]["rounds"], info[k]["active_tile_rounds"]
        floor_rounds = 12.0 * active * T * T / HBM_BYTES_PER_S * 1e6
        floor_ends = c[6] * px / HBM_BYTES_PER_S * 1e6
        res[k] = {"device_us": median(t[k]["call"]), "wall_us": median(t[k]["wall"]), "prepare_us": median(t[k]["prepare"]),
                  "rounds_us": median(t[k]["rounds"]), "finish_us": median(t[k]["finish"]), "rounds": rounds,
                  "converged": info[k]["converged"], "active_tile_rounds": active, "active_share": active / float(tiles * rounds),
                  "hbm_floor_us": floor_rounds + floor_ends, "hbm_floor_rounds_us": floor_rounds,
                  "over_floor": (median(t[k]["prepare"]) + median(t[k]["rounds"]) + median(t[k]["finish"])) / (floor_rounds + floor_ends),
                  "all_rounds": t[k]}
        print(f"{k}: {res[k]['device_us']:.0f} us per call ({res[k]['wall_us']:.0f} us wall), phases {res[k]['prepare_us']:.0f} + "
              f"{res[k]['rounds_us']:.0f} + {res[k]['finish_us']:.0f} us, {rounds} rounds, {100 * res[k]['active_share']:.1f} % of tile-rounds "
              f"active, floor {res[k]['hbm_floor_us']:.0f} us (arithmetic)", file=sys.stderr)
    out = {"device": torch.cuda.get_device_name(0), "raster": [S, S], "tile": T, "rounds": a.rounds, "warmup": a.warmup, "cases": res,
           "same_run": {k: {"device_us": median(v), "all_rounds": v} for k, v in other.items()},
           "floor": "arithmetic, not a measurement: 12 B per pixel per active tile-round plus prepare and finish, at 5.5 TB/s",
           "context": "not yet measured"}

    def write():
        line = json.dumps(out)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    write()                                                         # the context leg comes last: what is measured is kept whatever it does
    out["context"] = {"host_route_h_dome": host_route(prob, 0.2, min(1024, S), a.host_seconds),
                      "what": "context, not parity: one run; .cpu() plus a whole-raster numpy Jacobi iteration on a crop"}
    print(write())


if __name__ == "__main__":
    main()

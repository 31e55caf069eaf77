"""The SA U-Net (spatial.UNet) against UNet(use_se=False) and UNet(use_se=True) at config-2 geometry (16 x 2 x 256 x 256,
bf16), in one process, the three models alternating over several rounds; and stand-alone times of the SpatialAttention
passes (csrc/spatial_attn.hip) at the four skip-concat shapes.

Timed step as in bench.py: zero_grad -> forward -> Dice+CE -> backward -> Adam, device-synchronised around the K steps
(eager launches with launch tapes; bench.py additionally replays a captured graph). GB/s of a pass from its algorithmic
bytes: compress reads x; gate reads x and writes the gated copy; dscale reads dy and x; dx reads and writes dy (the 1-channel
fp32 maps are counted too).

usage: python tools/sa_bench.py [--steps 30] [--warmup 10] [--rounds 3] [--reps 20]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = [(256, 128), (128, 256), (64, 512), (32, 1024)]     # skip-concat (H = W, channels) at config 2


def step_times(args):
    import torch
    import insar_unet_ca_amd as iu
    from insar_unet_ca_amd.data import make_batch
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    builders = {"unet_sa": lambda: iu.UNetSpatialAttention(2, 2, compute_dtype=dt),
                "unet_plain": lambda: iu.UNet(2, 2, use_se=False, compute_dtype=dt),
                "unet_ca": lambda: iu.UNet(2, 2, use_se=True, compute_dtype=dt)}
    batches = [tuple(v.to(dev) for v in make_batch(16 * b, 16, 256)) for b in range(2)]
    crit = iu.DiceCELoss(ignore_index=255)
    models = {}
    for name, build in builders.items():
        torch.manual_seed(0)
        net = build().to(dev).train()
        models[name] = (net, iu.Adam(net.parameters(), lr=1e-4))

    def run(name, k):
        net, opt = models[name]
        for i in range(k):
            x, y = batches[i % 2]
            opt.zero_grad(set_to_none=True)
            loss = crit(net(x), y)
            loss.backward()
            opt.step()
        return loss

    for name in models:
        run(name, args.settle)
    torch.cuda.synchronize()
    res = {n: [] for n in models}
    for r in range(args.rounds):
        order = list(models) if r % 2 == 0 else list(reversed(list(models)))
        for name in order:
            run(name, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    return res


def pass_times(args):
    import torch
    from insar_unet_ca_amd import engine, _lib, spatial
    from insar_unet_ca_amd._lib import call
    dev, dt, B = torch.device("cuda:0"), torch.bfloat16, 16
    s = _lib.stream_ptr()
    out = []

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3

    for hw, c in LEVELS:
        x = engine.Act.alloc(B, hw, hw, c, dt, dev)
        y = engine.Act.alloc(B, hw, hw, c, dt, dev)
        dy = engine.Act.alloc(B, hw, hw, c, dt, dev)
        x.buf[:, 1:-1, 1:-1].normal_()
        dy.buf[:, 1:-1, 1:-1].normal_()
        sa = spatial.SpatialAttention().to(dev).train()
        ctx = engine.Ctx(dev, dt)
        unit = engine.SAUnit(ctx, sa, x, y, "sa")
        sink = engine.GradSink(ctx, unit.params())
        unit.forward(True)
        unit.backward(dy, sink, True)          # every buffer valid (dy is overwritten: the dx pass keeps rewriting it)
        f = unit._desc()
        f.training = 1
        d = unit._desc()
        d.y, d.training = dy.desc, 1
        v = lambda p: sink.view(p).data_ptr()
        d.dw1, d.db1, d.dgamma1, d.dbeta1 = v(unit.conv1.weight), v(unit.conv1.bias), v(unit.bn1.weight), v(unit.bn1.bias)
        d.dw2, d.db2, d.dgamma2, d.dbeta2 = v(unit.conv2.weight), v(unit.conv2.bias), v(unit.bn2.weight), v(unit.bn2.bias)
        fwd, bwd = C.byref(f), C.byref(d)
        M = B * hw * hw
        xb, mb = M * c * 2, M * 4
        runs = {
            "compress": (lambda: call("insar_sa_compress", fwd, s), xb + 2 * mb + M * 2),
            "gate": (lambda: call("insar_sa_gate", fwd, s), 2 * xb + 2 * mb),
            "dscale": (lambda: call("insar_sa_dscale", bwd, s), 2 * xb + 3 * mb),
            "dx": (lambda: call("insar_sa_dx", bwd, s), 2 * xb + 3 * mb + M * 2),
        }
        tag = f"{hw}^2 x{c}"
        for name, (fn, nbytes) in runs.items():
            us = timed(fn)
            out.append((f"{name} {tag}", us, nbytes / us / 1e3))
        # the stencil chain of one unit, forward + backward (the launches between the C-channel passes)
        def chain():
            call("insar_sa_conv", fwd, 1, s)
            unit._finalize(unit.conv1, unit.bn1, unit.stat1, 0, True, s)
            call("insar_sa_conv", fwd, 2, s)
            unit._finalize(unit.conv2, unit.bn2, unit.stat2, 1, True, s)
            call("insar_sa_bwd_coef", bwd, 2, s)
            call("insar_sa_bwd_stencil", bwd, 2, s)
            call("insar_sa_bwd_coef", bwd, 1, s)
            call("insar_sa_bwd_stencil", bwd, 1, s)
            call("insar_sa_bwd_coef", bwd, 0, s)
        out.append((f"stencil chain fwd+bwd {tag}", timed(chain), 0.0))
        # the whole unit, forward + backward
        def whole():
            unit.forward(True)
            unit.backward(dy, sink, True)
        out.append((f"SA unit fwd+bwd {tag}", timed(whole), 0.0))
        del unit, x, y, dy
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--settle", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    import torch
    print(f"device: {torch.cuda.get_device_name(0)}")
    if not args.skip_steps:
        res = step_times(args)
        print(f"\nms/step, config-2 geometry (16 x 2 x 256 x 256, bf16, Dice+CE, Adam), {args.rounds} alternating rounds of "
              f"{args.steps} steps:")
        for name, v in res.items():
            print(f"  {name:11s} " + "  ".join(f"{t:7.3f}" for t in v) + f"   min {min(v):7.3f}")
        d = min(res["unet_sa"]) - min(res["unet_plain"])
        print(f"  unet_sa - unet_plain = {d:+.3f} ms/step (min over rounds)")
    print("\nstand-alone passes (HIP events, bf16, B = 16):")
    for name, us, gbs in pass_times(args):
        print(f"  {name:34s} {us:9.1f} us" + (f"  {gbs:8.1f} GB/s" if gbs else ""))


if __name__ == "__main__":
    main()

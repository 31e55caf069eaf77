"""insar_adam_step (csrc/loss_optim.hip) on the same 4096 (p, g, m, v) elements two ways: as one tensor (its float4 body)
and as 4096 one-element tensors (its scalar tail); two steps; prints how many elements end up with different bits.
usage: python tools/adam_tail_paths.py   (needs a ROCm device)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from insar_unet_ca_amd import _lib
from insar_unet_ca_amd.parallel import _hip_adam_rows
dev = torch.device("cuda:0")
_lib.load()
N = 1 << 16
gen = torch.Generator().manual_seed(0)
base = {k: torch.randn(N, generator=gen) * s for k, s in (("p", 0.1), ("g", 1e-3), ("m", 1e-4), ("v", 1e-7))}
base["v"] = base["v"].abs()
def run(mode):
    t = {k: v.clone().to(dev) for k, v in base.items()}
    if mode == "vec":
        rows = [(t["p"], t["g"], t["m"], t["v"])]
    else:   # one-element rows: every element goes through the scalar tail (4-float stride keeps the rows 16-byte aligned)
        t = {k: torch.zeros(4 * N, device=dev) for k in base}
        for k in base:
            t[k].view(N, 4)[:, 0] = base[k].to(dev)
        rows = [tuple(t[k][4 * i:4 * i + 1] for k in "pgmv") for i in range(4096)]
    for step in (1, 2):
        _hip_adam_rows(rows, 1e-3, 0.9, 0.999, 1e-8, 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5)
    torch.cuda.synchronize()
    if mode == "vec":
        return {k: t[k][:4096].cpu() for k in "pmv"}
    return {k: t[k].view(N, 4)[:4096, 0].cpu() for k in "pmv"}
a, b = run("vec"), run("tail")
for k in "pmv":
    d = (a[k] != b[k])
    print(k, "elements differing:", int(d.sum()), "of 4096; max |diff|", float((a[k] - b[k]).abs().max()),
          "example", [(float(a[k][i]), float(b[k][i])) for i in d.nonzero().flatten()[:2].tolist()])

"""GPU: insar_adam_step and insar_adam_step_dev (csrc/loss_optim.hip) called directly on the pointer table / chunk list layout
of optim.py, against tail_ref.adam_reference in float64: tensor sizes around the 4-element vector width and the CHUNK
boundary, 16-byte aligned (the float4 path) and one float off (the scalar path), grad_scale, a tensor that must not move, and
the device-side step state."""
import math

import numpy as np
import pytest
import torch

from tests import tail_ref as tr
from tests.helpers import max_rel

pytestmark = pytest.mark.gpu
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
STEPS = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    from insar_unet_ca_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _sizes():
    from insar_unet_ca_amd.optim import CHUNK
    return [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]


class Tensors:
    """p, g, m, v for every size of _sizes() plus one tensor with g = 0 and v = 0, each inside a NaN-guarded store at
    `offset` floats from a 16-byte boundary; the pointer table and the chunk list as optim.Adam._table builds them."""

    def __init__(self, dev, offset, seed=5):
        from insar_unet_ca_amd.optim import CHUNK
        self.dev, self.offset, self.chunk = dev, offset, CHUNK
        self.sizes = _sizes() + [CHUNK + 3]                       # the last one is the still tensor
        self.still = len(self.sizes) - 1
        gen = torch.Generator().manual_seed(seed)
        self.host = []                                            # float64 (p, m, v) per tensor: the reference state
        self.stores, self.views = [], []
        for i, n in enumerate(self.sizes):
            p = torch.randn(n, generator=gen)
            p = p + torch.where(p < 0, -0.5, 0.5)                 # |p| >= 0.5: max-rel is not a statement about cancellation
            self.host.append([p.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)])
            quad = []
            for init in (p, torch.zeros(n), torch.zeros(n), torch.zeros(n)):        # p, g, m, v
                store = torch.full((n + 12,), float("nan"), device=dev)
                view = store[4 + offset:4 + offset + n]
                view.copy_(init.to(dev))
                assert view.data_ptr() % 16 == 4 * offset
                self.stores.append(store)
                quad.append(view)
            self.views.append(quad)
        rows, chunks = [], []
        for ti, (p, g, m, v) in enumerate(self.views):
            rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()])
            chunks += [[ti, ci] for ci in range((p.numel() + CHUNK - 1) // CHUNK)]
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.chunks = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self.nchunks = len(chunks)

    def grads(self, step):
        gen = torch.Generator().manual_seed(1000 + step)
        out = [torch.randn(n, generator=gen) * (10.0 ** (i % 3 - 1)) for i, n in enumerate(self.sizes)]
        out[self.still].zero_()
        return out

    def load_grads(self, gl):
        for (p, g, m, v), src in zip(self.views, gl):
            g.copy_(src.to(self.dev))

    def reference_step(self, gl, step, gscale):
        for st, g in zip(self.host, gl):
            st[0], st[1], st[2] = tr.adam_reference(st[0], g, st[1], st[2], step, LR, B1, B2, EPS, gscale)

    def guards_intact(self):
        for store, n in zip(self.stores, [n for n in self.sizes for _ in range(4)]):
            t = store.clone()
            t[4 + self.offset:4 + self.offset + n] = float("nan")
            if not bool(torch.isnan(t).all()):
                return False
        return True

    def params(self):
        return [q[0].cpu().clone() for q in self.views]


def _host_step(t, step, gscale):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    call("insar_adam_step", ptr(t.table), ptr(t.chunks), t.nchunks, t.chunk, LR, B1, B2, EPS, 1.0 - B1 ** step,
         math.sqrt(1.0 - B2 ** step), gscale, _lib.stream_ptr())


def _dev_step(t, state, gscale):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import call, ptr
    call("insar_adam_step_dev", ptr(t.table), ptr(t.chunks), t.nchunks, t.chunk, LR, B1, B2, EPS, ptr(state), gscale, _lib.stream_ptr())


def _check_against_reference(t, tag):
    """p within 1e-6 (max-rel, the bound of test_adam_kernel_against_oracle); m within 1e-6; v within 1e-4: the kernel holds
    beta2 in fp32, and 1 - fl32(0.999) differs from 0.001 by 1.3e-5 of its value (p sees sqrt(v) against O(1) values: 1e-8)."""
    worst = [0.0, 0.0, 0.0]
    for (p, g, m, v), (rp, rm, rv) in zip(t.views, t.host):
        for i, (a, b) in enumerate(((p, rp), (m, rm), (v, rv))):
            worst[i] = max(worst[i], max_rel(a, b))
    print("ADAMFIG %s offset %d: p %.2e m %.2e v %.2e" % (tag, t.offset, worst[0], worst[1], worst[2]))
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6 and worst[2] <= 1e-4, worst
    assert t.guards_intact()


@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("offset", [0, 1])
def test_adam_step_four_steps_against_float64(dev, offset, gscale):
    t = Tensors(dev, offset)
    still0 = t.views[t.still][0].cpu().clone()
    for step in range(1, STEPS + 1):
        gl = t.grads(step)
        t.load_grads(gl)
        _host_step(t, step, gscale)
        t.reference_step(gl, step, gscale)
        _check_against_reference(t, "host-args step %d gscale %g" % (step, gscale))
    assert torch.equal(t.views[t.still][0].cpu(), still0)                         # g = 0 on v = 0: p is not touched by rounding
    assert float(t.views[t.still][2].abs().max()) == 0.0 and float(t.views[t.still][3].abs().max()) == 0.0


@pytest.mark.parametrize("offset", [0, 1])
def test_adam_step_dev_state_and_parameters(dev, offset):
    """After n calls the state block is {n, fp32(1 - b1^n), fp32(sqrt(1 - b2^n))}; the parameters follow the float64 reference
    and the host-argument entry point."""
    t, h = Tensors(dev, offset), Tensors(dev, offset)
    state = torch.zeros(4, dtype=torch.float32, device=dev)
    for step in range(1, STEPS + 1):
        gl = t.grads(step)
        t.load_grads(gl)
        h.load_grads(gl)
        _dev_step(t, state, 0.25)
        _host_step(h, step, 0.25)
        t.reference_step(gl, step, 0.25)
        want = np.array([step, 1.0 - B1 ** step, math.sqrt(1.0 - B2 ** step)], dtype=np.float64).astype(np.float32)
        got = state.cpu().numpy()
        assert got[:3].tobytes() == want.tobytes(), (step, got, want)
        assert got[3] == 0.0
        _check_against_reference(t, "device-state step %d" % step)
        for a, b in zip(t.params(), h.params()):
            assert max_rel(a, b) <= 1e-6


def test_adam_aligned_and_unaligned_paths_agree(dev):
    """The float4 path and the scalar path run the same expression per element: held to 1e-6 of each other; whether they are
    bitwise equal is printed and reported in DESIGN.md, not asserted."""
    a, u = Tensors(dev, 0), Tensors(dev, 1)
    for step in range(1, STEPS + 1):
        gl = a.grads(step)
        for t in (a, u):
            t.load_grads(gl)
            _host_step(t, step, 1.0)
    same = all(torch.equal(x, y) for x, y in zip(a.params(), u.params()))
    same_mv = all(torch.equal(qa[i].cpu(), qu[i].cpu()) for qa, qu in zip(a.views, u.views) for i in (2, 3))
    print("ADAMFIG aligned vs unaligned after %d steps: p bitwise equal %s, m and v bitwise equal %s" % (STEPS, same, same_mv))
    for x, y in zip(a.params(), u.params()):
        assert max_rel(x, y) <= 1e-6


def test_adam_refuses_bad_chunking(dev):
    from insar_unet_ca_amd import _lib
    from insar_unet_ca_amd._lib import ptr
    lib = _lib.load()
    t = Tensors(dev, 0)
    before = t.params()
    for chunk in (0, 2, 6):
        assert lib.insar_adam_step(ptr(t.table), ptr(t.chunks), t.nchunks, chunk, LR, B1, B2, EPS, 0.1, 0.03, 1.0, _lib.stream_ptr()) == -1001
        assert "insar_adam_step" in lib.insar_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, t.params()))

"""CPU-only: the pointer table / chunk list pair of the Adam family (optim.build_tables), its cache (optim.TableCache) and
the three callers — Adam.step, AdamW.step, parallel._hip_adam_rows — on CPU tensors of numel 1, CHUNK - 1, CHUNK, CHUNK + 1
and 2 * CHUNK + 3, the sizes at which the chunk arithmetic can go wrong. Expected tables are written out from data_ptr() and
numel(); the chunk list is a literal."""
import numpy as np
import pytest
import torch

from insar_unet_ca_amd import _lib, optim, parallel
from insar_unet_ca_amd.optim import CHUNK

SIZES = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
CHUNKS = [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2]]
WD, MULT = [1e-2, 1e-2, 0.0, 0.0, 1e-2], [1.0, 1.0, 0.5, 0.5, 1.0]
WD_BITS = {1e-2: 0x3C23D70A, 0.0: 0}                       # float32 bit patterns
MULT_BITS = {1.0: 0x3F800000, 0.5: 0x3F000000}


def _quads(sizes=SIZES):
    return [tuple(torch.zeros(n) for _ in range(4)) for n in sizes]


def _check_pair(table, chunk_t, nchunks, rows):
    assert table.dtype == torch.int64 and table.shape == (len(rows), len(rows[0])) and table.tolist() == rows
    assert chunk_t.dtype == torch.int32 and chunk_t.shape == (8, 2) and chunk_t.tolist() == CHUNKS and nchunks == 8
    assert table.device.type == "cpu" and chunk_t.device.type == "cpu"


def test_five_word_rows():
    quads = _quads()
    rows = [[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, g, m, v in quads]
    assert [r[4] for r in rows] == SIZES
    _check_pair(*optim.build_tables(rows, SIZES, torch.device("cpu")), rows)
    cache = optim.TableCache()
    hit = optim.adam_tables(cache, quads)
    _check_pair(*hit, rows)
    again = optim.adam_tables(cache, quads)                       # the same rows: the identical tensors
    assert all(a is b for a, b in zip(hit, again)) and len(cache) == 1
    named = optim.adam_tables(cache, quads, key=("early", 1, 2, 3))
    assert named[0] is not hit[0] and named[0].tolist() == rows and len(cache) == 2
    assert optim.adam_tables(cache, _quads([3]), key=("early", 1, 2, 3)) is named       # a caller's own key is taken as it is


def test_eight_word_rows_with_float_bits():
    quads, emas = _quads(), [torch.zeros(n) for n in SIZES]
    emas[2] = None                                                # no EMA tensor: a null pointer word
    rows = [[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if e is None else e.data_ptr(), p.numel(), WD_BITS[wd], MULT_BITS[mu]]
            for (p, g, m, v), e, wd, mu in zip(quads, emas, WD, MULT)]
    bits = lambda x: int(np.float32(x).view(np.uint32))
    assert [r[6] for r in rows] == [bits(w) for w in WD] and [r[7] for r in rows] == [bits(m) for m in MULT]
    _check_pair(*optim.build_tables(rows, SIZES, torch.device("cpu")), rows)
    for norm in (None, 1.0):
        opt = optim.AdamW([torch.nn.Parameter(q[0]) for q in quads], lr=1e-3, max_grad_norm=norm)
        tensors = [q + (e, wd, mu) for q, e, wd, mu in zip(quads, emas, WD, MULT)]
        table, chunk_t, nchunks, partials, cfg = opt._table(tensors)
        _check_pair(table, chunk_t, nchunks, rows)
        assert (partials is None) if norm is None else (partials.shape == (8,) and partials.dtype == torch.float32)
        assert isinstance(cfg, _lib.InsarOptwConfig) and cfg.max_norm == (-1.0 if norm is None else 1.0)
        assert opt._table(tensors)[0] is table and len(opt._tables) == 1


def test_cache_stays_bounded():
    cache = optim.TableCache()
    held, sizes = [], []
    for i in range(10):
        held.append(_quads([2]))                                  # held: ten distinct sets of addresses
        hit = optim.adam_tables(cache, held[-1])
        sizes.append(len(cache))
        assert optim.adam_tables(cache, held[-1]) is hit
    assert sizes == [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]                # everything goes once it holds more than 8 entries


class _AsIfOnRocm(torch.Tensor):
    is_cuda = True                                                # passes _hip_adam_rows' device refusal; the memory stays on the CPU


@pytest.fixture
def launches(monkeypatch):
    """The ABI replaced by a recorder of (entry, arguments); the device requirement of the optimizers lifted."""
    seen = []

    def fake_call(name, *a):
        seen.append((name, a))
        return 0

    monkeypatch.setattr(optim, "call", fake_call)
    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(optim, "_require_device", lambda *a, **k: None)
    return seen


def _tables_of(cache, address):
    return next(e for e in cache.values() if e[0].data_ptr() == address)


@pytest.mark.parametrize("caller", ["Adam", "AdamW", "_hip_adam_rows"])
def test_moved_gradient_builds_a_new_table(launches, caller):
    """The gradient pointer of one row changes, its parameter pointer does not: every caller builds a new table (keyed on
    the parameter pointers alone, _hip_adam_rows used to replay the old one)."""
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (3, CHUNK + 1)]
    for p in ps:
        p.grad = torch.ones_like(p)
    if caller == "_hip_adam_rows":
        moments = [(torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
        cache = parallel._row_tables
        cache.clear()

        def step():
            rows = [(p.detach().as_subclass(_AsIfOnRocm), p.grad, m, v) for p, (m, v) in zip(ps, moments)]
            parallel._hip_adam_rows(rows, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03)
    else:
        opt = getattr(optim, caller)(ps, lr=1e-3)
        cache, step = opt._tables, opt.step
    step()
    step()
    assert len(cache) == 1 and len({a[0] for n, a in launches if n in ("insar_adam_step", "insar_adamw_step")}) == 1
    first = _tables_of(cache, launches[-1][1][0])
    old_grad = ps[1].grad                                         # kept alive: its address cannot be handed out again
    ps[1].grad = old_grad.clone()
    step()
    assert len(cache) == 2
    second = _tables_of(cache, launches[-1][1][0])
    assert second[0] is not first[0] and launches[-1][1][1] == second[1].data_ptr()
    assert [r[0] for r in second[0].tolist()] == [r[0] for r in first[0].tolist()] == [p.data_ptr() for p in ps]
    assert [r[1] for r in first[0].tolist()] == [ps[0].grad.data_ptr(), old_grad.data_ptr()]
    assert [r[1] for r in second[0].tolist()] == [ps[0].grad.data_ptr(), ps[1].grad.data_ptr()]
    assert second[1].tolist() == [[0, 0], [1, 0], [1, 1]] and second[2] == 3

"""CPU-only: the launch plan of engine._wgrad_conv3 (the 3x3 weight gradient) for the 3x3 layers of the benchmarked U-Net
configurations — bf16 at batch 16 x 256^2 and fp32 at batch 8 x 512^2 (its levels up to 256 pixels wide), plus one 90-pixel
grid that only the per-tap kernel takes — under the defaults and every switch that routes between the four row-of-taps
kernels (csrc/wgrad3*.hip), with and without a side stream.

Per case: the entry point launched, its nsplit, the floats asked of ctx.wgrad_part, the arguments of ctx.wgrad_finish, the
order of ALL ABI calls (the count-only `_tile` queries answered by the library itself, launches recorded instead of run),
and, under a recording profiler that keeps the step's launch configuration (alone = False), the tag, flops and bytes.

TABLE and SEQS were recorded from the code BEFORE the four branches of _wgrad_conv3 were folded into one body
(`python -m tests.test_wgrad_conv3_plan_host` prints them); they are never regenerated from the code under test."""
import pytest
import torch

from insar_unet_ca_amd import _lib, engine

# (cin, cout, W) as the U-Net has them: at a level with c channels c/2 -> c (encoder), c -> c, 2c -> c (decoder, after the concat)
LAYERS_BF16 = [(16, 256, 256, ci, co) for ci, co in ((64, 64), (128, 64))] + \
              [(16, 128, 128, ci, co) for ci, co in ((64, 128), (128, 128), (256, 128))] + \
              [(16, 64, 64, ci, co) for ci, co in ((128, 256), (256, 256), (512, 256))] + \
              [(16, 32, 32, ci, co) for ci, co in ((256, 512), (512, 512), (1024, 512))] + \
              [(16, 16, 16, ci, co) for ci, co in ((512, 1024), (1024, 1024))]
LAYERS_F32 = [(8, 256, 256, ci, co) for ci, co in ((64, 128), (128, 128), (256, 128))] + \
             [(8, 128, 128, ci, co) for ci, co in ((128, 256), (256, 256), (512, 256))] + \
             [(8, 64, 64, ci, co) for ci, co in ((256, 512), (512, 512), (1024, 512))] + \
             [(8, 32, 32, ci, co) for ci, co in ((512, 1024), (1024, 1024))]
CASES = [("bf16",) + l for l in LAYERS_BF16 + [(2, 90, 90, 64, 64)]] + [("f32",) + l for l in LAYERS_F32]
SETTINGS = {
    "defaults": {},
    "x0": {"WGRAD_X": False},
    "y1": {"WGRAD_Y": 1},
    "y2": {"WGRAD_Y": 2},
    "y3": {"WGRAD_Y": 3},
    "k": {"WGRAD_K": True},
    "k4": {"WGRAD_K": True, "WGRAD_K_TILES": {"128x64", "128x128", "64x128", "64x64"}},
    "rows0": {"WGRAD_ROWS": False},
}
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


class FakeCtx:
    """What _wgrad_conv3 uses of engine.Ctx, recording instead of allocating."""

    def __init__(self, dtype: torch.dtype, side: bool):
        self.code = _lib.dtype_code(dtype)
        self.esize = 2 if dtype == torch.bfloat16 else 4
        self.side = object() if side else None
        self.part_floats, self.finish = None, None

    def wgrad_part(self, floats: int):
        assert self.part_floats is None
        self.part_floats = floats
        return None

    def wgrad_finish(self, part, grad, nsplit, ntaps, cout, cin, layout) -> None:
        assert self.finish is None
        self.finish = (nsplit, ntaps, cout, cin, layout)

    def pixel_table(self, B, H, W, s, Hb, Wb, tail) -> torch.Tensor:
        return torch.empty(engine._round_up(B * H * W, engine.WG_BKP), dtype=torch.int32)


class RecordingProfiler:
    alone = False

    def __init__(self):
        self.runs = []

    def run(self, tag, flops, fn, nbytes=0.0):
        self.runs.append((tag, float(flops), float(nbytes)))
        fn()


def plan(monkeypatch, case, setting: str, side: bool, profiled: bool):
    """One _wgrad_conv3 call: (names of all ABI calls in order, entry launched, nsplit, part floats, wgrad_finish arguments,
    profiler record or None)."""
    dtype, B, H, W, cin, cout = case
    names, launches = [], []
    real_call = _lib.call

    def fake_call(name, *a):
        names.append(name)
        if name in _lib._COUNT_ONLY:
            return real_call(name, *a)
        launches.append((name, a[0]._obj.nsplit if name == "insar_wgrad" else a[3]))
        return 0

    monkeypatch.setattr(engine, "call", fake_call)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setattr(engine, k, v)
    prof = RecordingProfiler() if profiled else None
    monkeypatch.setattr(engine, "PROFILER", prof)
    ctx = FakeCtx(DTYPES[dtype], side)
    x = engine.Act(torch.empty(1, dtype=DTYPES[dtype]), B, H, W, cin, 0, cin)
    dy = engine.Act(torch.empty(1, dtype=DTYPES[dtype]), B, H, W, cout, 0, cout)
    engine._wgrad_conv3(ctx, x, dy, None)
    assert len(launches) == 1 and (prof is None or len(prof.runs) == 1)
    return tuple(names), launches[0][0], launches[0][1], ctx.part_floats, ctx.finish, (prof.runs[0] if prof else None)


def record_all(monkeypatch_factory):
    """{(case, setting, side): row} and the de-duplicated call sequences; a row is (entry, nsplit, part floats, finish
    arguments, sequence index unprofiled, (tag, flops, bytes), sequence index profiled)."""
    seqs, table = [], {}

    def seq_id(s):
        if s not in seqs:
            seqs.append(s)
        return seqs.index(s)

    for case in CASES:
        for setting in SETTINGS:
            for side in (True, False):
                with monkeypatch_factory() as mp:
                    plain = plan(mp, case, setting, side, False)
                with monkeypatch_factory() as mp:
                    prof = plan(mp, case, setting, side, True)
                assert plain[1:5] == prof[1:5], "a profiler that keeps the step's configuration changed the plan"
                table[(case, setting, side)] = plain[1:5] + (seq_id(plain[0]), prof[5], seq_id(prof[0]))
    return seqs, table


def test_the_table_covers_every_case():
    assert set(TABLE) == {(c, s, side) for c in CASES for s in SETTINGS for side in (True, False)}
    # every kernel family and the per-tap kernel occur
    assert {r[0] for r in TABLE.values()} == {"insar_wgrad_conv3", "insar_wgrad_conv3x", "insar_wgrad_conv3y", "insar_wgrad_conv3k", "insar_wgrad"}


@pytest.mark.parametrize("side", [True, False], ids=["side", "noside"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_wgrad_conv3_launch_plan_matches_the_recording(monkeypatch, setting, side):
    for case in CASES:
        entry, nsplit, floats, finish, seq, prof, seq_prof = TABLE[(case, setting, side)]
        what = f"{case} {setting} side={side}"
        with monkeypatch.context() as mp:
            got = plan(mp, case, setting, side, False)
        assert got[1] == entry, what
        assert got[2] == nsplit, what
        assert got[3] == floats, what
        assert got[4] == finish, what                    # (slabs, 9, cout, cin, layout 0)
        assert got[0] == SEQS[seq], what
        assert got[5] is None
        with monkeypatch.context() as mp:
            got = plan(mp, case, setting, side, True)
        assert got[1:5] == (entry, nsplit, floats, finish), what
        assert got[5] == prof, what                      # tag, flops, bytes
        assert got[0] == SEQS[seq_prof], what


if __name__ == "__main__":
    import pprint
    seqs, table = record_all(pytest.MonkeyPatch.context)
    print("SEQS = " + pprint.pformat(seqs, width=160, compact=True))
    print("TABLE = {")
    for k, v in table.items():
        print(f"    {k!r}: {v!r},")
    print("}")


# ---- the recording (parent of the commit that folded _wgrad_conv3's branches). Key: ((dtype, B, H, W, cin, cout), setting, side stream);
# row: entry, nsplit, floats of ctx.wgrad_part, wgrad_finish arguments, SEQS index, profiler (tag, flops, bytes), SEQS index when profiled
SEQS = [('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3'), ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3y_tile', 'insar_wgrad_conv3'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3k_tile', 'insar_wgrad_conv3'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3k_tile', 'insar_wgrad_conv3k_slices', 'insar_wgrad_conv3k'),
 ('insar_wgrad_tile_pair', 'insar_wgrad'), ('insar_wgrad_tile_pair', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3y_tile', 'insar_wgrad_conv3y'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3x'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_tile_pair', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_tile_pair', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3y_tile', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3y_tile', 'insar_wgrad_tile_pair', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3k_tile', 'insar_wgrad_tile_pair', 'insar_wgrad'),
 ('insar_wgrad_conv3_tile', 'insar_wgrad_conv3x_tile', 'insar_wgrad_conv3k_tile', 'insar_wgrad_tile_pair', 'insar_wgrad_tile_pair', 'insar_wgrad')]
TABLE = {
    (('bf16', 16, 256, 256, 64, 64), 'defaults', True): ('insar_wgrad_conv3', 169, 6230016, (169, 9, 64, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 293355520.0), 0),
    (('bf16', 16, 256, 256, 64, 64), 'defaults', False): ('insar_wgrad_conv3', 256, 9437184, (256, 9, 64, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 306184192.0), 0),
    (('bf16', 16, 256, 256, 64, 64), 'x0', True): ('insar_wgrad_conv3', 169, 6230016, (169, 9, 64, 64, 0), 1, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 293355520.0), 1),
    (('bf16', 16, 256, 256, 64, 64), 'x0', False): ('insar_wgrad_conv3', 256, 9437184, (256, 9, 64, 64, 0), 1, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 306184192.0), 1),
    (('bf16', 16, 256, 256, 64, 64), 'y1', True): ('insar_wgrad_conv3', 169, 6230016, (169, 9, 64, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 293355520.0), 0),
    (('bf16', 16, 256, 256, 64, 64), 'y1', False): ('insar_wgrad_conv3', 256, 9437184, (256, 9, 64, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 306184192.0), 0),
    (('bf16', 16, 256, 256, 64, 64), 'y2', True): ('insar_wgrad_conv3', 169, 6230016, (169, 9, 64, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 293355520.0), 2),
    (('bf16', 16, 256, 256, 64, 64), 'y2', False): ('insar_wgrad_conv3', 256, 9437184, (256, 9, 64, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 306184192.0), 2),
    (('bf16', 16, 256, 256, 64, 64), 'y3', True): ('insar_wgrad_conv3', 169, 6230016, (169, 9, 64, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 293355520.0), 2),
    (('bf16', 16, 256, 256, 64, 64), 'y3', False): ('insar_wgrad_conv3', 256, 9437184, (256, 9, 64, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 306184192.0), 2),
    (('bf16', 16, 256, 256, 64, 64), 'k', True): ('insar_wgrad_conv3', 169, 6230016, (169, 9, 64, 64, 0), 3, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 293355520.0), 3),
    (('bf16', 16, 256, 256, 64, 64), 'k', False): ('insar_wgrad_conv3', 256, 9437184, (256, 9, 64, 64, 0), 3, ('wgrad3_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 306184192.0), 3),
    (('bf16', 16, 256, 256, 64, 64), 'k4', True): ('insar_wgrad_conv3k', 42, 12386304, (336, 9, 64, 64, 0), 4, ('wgrad3k_kernel<64, 64>', 77309411328.0, 317980672.0), 4),
    (('bf16', 16, 256, 256, 64, 64), 'k4', False): ('insar_wgrad_conv3k', 85, 25067520, (680, 9, 64, 64, 0), 4, ('wgrad3k_kernel<64, 64>', 77309411328.0, 368705536.0), 4),
    (('bf16', 16, 256, 256, 64, 64), 'rows0', True): ('insar_wgrad', 113, 4165632, (113, 9, 64, 64, 0), 5, ('wgrad_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 285097984.0), 6),
    (('bf16', 16, 256, 256, 64, 64), 'rows0', False): ('insar_wgrad', 113, 4165632, (113, 9, 64, 64, 0), 5, ('wgrad_kernel<bf16_t, 64, 64, 4>', 77309411328.0, 285097984.0), 6),
    (('bf16', 16, 256, 256, 128, 64), 'defaults', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 64, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 440401920.0), 0),
    (('bf16', 16, 256, 256, 128, 64), 'defaults', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 64, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 478150656.0), 0),
    (('bf16', 16, 256, 256, 128, 64), 'x0', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 64, 128, 0), 1, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 440401920.0), 1),
    (('bf16', 16, 256, 256, 128, 64), 'x0', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 64, 128, 0), 1, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 478150656.0), 1),
    (('bf16', 16, 256, 256, 128, 64), 'y1', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 64, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 440401920.0), 0),
    (('bf16', 16, 256, 256, 128, 64), 'y1', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 64, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 478150656.0), 0),
    (('bf16', 16, 256, 256, 128, 64), 'y2', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 64, 128, 0), 2, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 440401920.0), 2),
    (('bf16', 16, 256, 256, 128, 64), 'y2', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 64, 128, 0), 2, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 478150656.0), 2),
    (('bf16', 16, 256, 256, 128, 64), 'y3', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 64, 128, 0), 2, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 440401920.0), 2),
    (('bf16', 16, 256, 256, 128, 64), 'y3', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 64, 128, 0), 2, ('wgrad3_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 478150656.0), 2),
    (('bf16', 16, 256, 256, 128, 64), 'k', True): ('insar_wgrad_conv3k', 42, 12386304, (168, 9, 64, 128, 0), 4, ('wgrad3k_kernel<128, 64>', 154618822656.0, 452198400.0), 4),
    (('bf16', 16, 256, 256, 128, 64), 'k', False): ('insar_wgrad_conv3k', 85, 25067520, (340, 9, 64, 128, 0), 4, ('wgrad3k_kernel<128, 64>', 154618822656.0, 502923264.0), 4),
    (('bf16', 16, 256, 256, 128, 64), 'k4', True): ('insar_wgrad_conv3k', 42, 12386304, (168, 9, 64, 128, 0), 4, ('wgrad3k_kernel<128, 64>', 154618822656.0, 452198400.0), 4),
    (('bf16', 16, 256, 256, 128, 64), 'k4', False): ('insar_wgrad_conv3k', 85, 25067520, (340, 9, 64, 128, 0), 4, ('wgrad3k_kernel<128, 64>', 154618822656.0, 502923264.0), 4),
    (('bf16', 16, 256, 256, 128, 64), 'rows0', True): ('insar_wgrad', 85, 6266880, (85, 9, 64, 128, 0), 5, ('wgrad_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 427720704.0), 6),
    (('bf16', 16, 256, 256, 128, 64), 'rows0', False): ('insar_wgrad', 85, 6266880, (85, 9, 64, 128, 0), 5, ('wgrad_kernel<bf16_t, 128, 64, 4>', 154618822656.0, 427720704.0), 6),
    (('bf16', 16, 128, 128, 64, 128), 'defaults', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 128, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 138412032.0), 0),
    (('bf16', 16, 128, 128, 64, 128), 'defaults', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 128, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 176160768.0), 0),
    (('bf16', 16, 128, 128, 64, 128), 'x0', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 128, 64, 0), 1, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 138412032.0), 1),
    (('bf16', 16, 128, 128, 64, 128), 'x0', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 128, 64, 0), 1, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 176160768.0), 1),
    (('bf16', 16, 128, 128, 64, 128), 'y1', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 128, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 138412032.0), 0),
    (('bf16', 16, 128, 128, 64, 128), 'y1', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 128, 64, 0), 0, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 176160768.0), 0),
    (('bf16', 16, 128, 128, 64, 128), 'y2', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 128, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 138412032.0), 2),
    (('bf16', 16, 128, 128, 64, 128), 'y2', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 128, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 176160768.0), 2),
    (('bf16', 16, 128, 128, 64, 128), 'y3', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 128, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 138412032.0), 2),
    (('bf16', 16, 128, 128, 64, 128), 'y3', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 128, 64, 0), 2, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 176160768.0), 2),
    (('bf16', 16, 128, 128, 64, 128), 'k', True): ('insar_wgrad_conv3', 128, 9437184, (128, 9, 128, 64, 0), 3, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 138412032.0), 3),
    (('bf16', 16, 128, 128, 64, 128), 'k', False): ('insar_wgrad_conv3', 256, 18874368, (256, 9, 128, 64, 0), 3, ('wgrad3_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 176160768.0), 3),
    (('bf16', 16, 128, 128, 64, 128), 'k4', True): ('insar_wgrad_conv3k', 42, 12386304, (168, 9, 128, 64, 0), 4, ('wgrad3k_kernel<64, 128>', 38654705664.0, 150208512.0), 4),
    (('bf16', 16, 128, 128, 64, 128), 'k4', False): ('insar_wgrad_conv3k', 85, 25067520, (340, 9, 128, 64, 0), 4, ('wgrad3k_kernel<64, 128>', 38654705664.0, 200933376.0), 4),
    (('bf16', 16, 128, 128, 64, 128), 'rows0', True): ('insar_wgrad', 84, 6193152, (84, 9, 128, 64, 0), 5, ('wgrad_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 125435904.0), 6),
    (('bf16', 16, 128, 128, 64, 128), 'rows0', False): ('insar_wgrad', 84, 6193152, (84, 9, 128, 64, 0), 5, ('wgrad_kernel<bf16_t, 64, 128, 4>', 38654705664.0, 125435904.0), 6),
    (('bf16', 16, 128, 128, 128, 128), 'defaults', True): ('insar_wgrad_conv3', 42, 6193152, (42, 9, 128, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 158990336.0), 0),
    (('bf16', 16, 128, 128, 128, 128), 'defaults', False): ('insar_wgrad_conv3', 84, 12386304, (84, 9, 128, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 183762944.0), 0),
    (('bf16', 16, 128, 128, 128, 128), 'x0', True): ('insar_wgrad_conv3', 42, 6193152, (42, 9, 128, 128, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 158990336.0), 1),
    (('bf16', 16, 128, 128, 128, 128), 'x0', False): ('insar_wgrad_conv3', 84, 12386304, (84, 9, 128, 128, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 183762944.0), 1),
    (('bf16', 16, 128, 128, 128, 128), 'y1', True): ('insar_wgrad_conv3', 42, 6193152, (42, 9, 128, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 158990336.0), 0),
    (('bf16', 16, 128, 128, 128, 128), 'y1', False): ('insar_wgrad_conv3', 84, 12386304, (84, 9, 128, 128, 0), 0, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 183762944.0), 0),
    (('bf16', 16, 128, 128, 128, 128), 'y2', True): ('insar_wgrad_conv3y', 85, 12533760, (85, 9, 128, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 184352768.0), 7),
    (('bf16', 16, 128, 128, 128, 128), 'y2', False): ('insar_wgrad_conv3y', 170, 25067520, (170, 9, 128, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 234487808.0), 7),
    (('bf16', 16, 128, 128, 128, 128), 'y3', True): ('insar_wgrad_conv3y', 85, 12533760, (85, 9, 128, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 184352768.0), 7),
    (('bf16', 16, 128, 128, 128, 128), 'y3', False): ('insar_wgrad_conv3y', 170, 25067520, (170, 9, 128, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 234487808.0), 7),
    (('bf16', 16, 128, 128, 128, 128), 'k', True): ('insar_wgrad_conv3k', 42, 12386304, (84, 9, 128, 128, 0), 4, ('wgrad3k_kernel<128, 128>', 77309411328.0, 183762944.0), 4),
    (('bf16', 16, 128, 128, 128, 128), 'k', False): ('insar_wgrad_conv3k', 85, 25067520, (170, 9, 128, 128, 0), 4, ('wgrad3k_kernel<128, 128>', 77309411328.0, 234487808.0), 4),
    (('bf16', 16, 128, 128, 128, 128), 'k4', True): ('insar_wgrad_conv3k', 42, 12386304, (84, 9, 128, 128, 0), 4, ('wgrad3k_kernel<128, 128>', 77309411328.0, 183762944.0), 4),
    (('bf16', 16, 128, 128, 128, 128), 'k4', False): ('insar_wgrad_conv3k', 85, 25067520, (170, 9, 128, 128, 0), 4, ('wgrad3k_kernel<128, 128>', 77309411328.0, 234487808.0), 4),
    (('bf16', 16, 128, 128, 128, 128), 'rows0', True): ('insar_wgrad', 56, 8257536, (56, 9, 128, 128, 0), 5, ('wgrad_kernel<bf16_t, 128, 128, 4>', 77309411328.0, 167247872.0), 6),
    (('bf16', 16, 128, 128, 128, 128), 'rows0', False): ('insar_wgrad', 56, 8257536, (56, 9, 128, 128, 0), 5, ('wgrad_kernel<bf16_t, 128, 128, 4>', 77309411328.0, 167247872.0), 6),
    (('bf16', 16, 128, 128, 256, 128), 'defaults', True): ('insar_wgrad_conv3x', 42, 12386304, (42, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 250871808.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'defaults', False): ('insar_wgrad_conv3x', 84, 24772608, (84, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 300417024.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'x0', True): ('insar_wgrad_conv3', 21, 6193152, (21, 9, 128, 256, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 154618822656.0, 226099200.0), 1),
    (('bf16', 16, 128, 128, 256, 128), 'x0', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 154618822656.0, 250871808.0), 1),
    (('bf16', 16, 128, 128, 256, 128), 'y1', True): ('insar_wgrad_conv3y', 42, 12386304, (42, 9, 128, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 250871808.0), 7),
    (('bf16', 16, 128, 128, 256, 128), 'y1', False): ('insar_wgrad_conv3y', 85, 25067520, (85, 9, 128, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 301596672.0), 7),
    (('bf16', 16, 128, 128, 256, 128), 'y2', True): ('insar_wgrad_conv3x', 42, 12386304, (42, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 250871808.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'y2', False): ('insar_wgrad_conv3x', 84, 24772608, (84, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 300417024.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'y3', True): ('insar_wgrad_conv3y', 42, 12386304, (42, 9, 128, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 250871808.0), 7),
    (('bf16', 16, 128, 128, 256, 128), 'y3', False): ('insar_wgrad_conv3y', 85, 25067520, (85, 9, 128, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 301596672.0), 7),
    (('bf16', 16, 128, 128, 256, 128), 'k', True): ('insar_wgrad_conv3x', 42, 12386304, (42, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 250871808.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'k', False): ('insar_wgrad_conv3x', 84, 24772608, (84, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 300417024.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'k4', True): ('insar_wgrad_conv3x', 42, 12386304, (42, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 250871808.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'k4', False): ('insar_wgrad_conv3x', 84, 24772608, (84, 9, 128, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 300417024.0), 8),
    (('bf16', 16, 128, 128, 256, 128), 'rows0', True): ('insar_wgrad', 28, 8257536, (28, 9, 128, 256, 0), 5, ('wgrad_kernel<bf16_t, 128, 128, 4>', 154618822656.0, 234356736.0), 6),
    (('bf16', 16, 128, 128, 256, 128), 'rows0', False): ('insar_wgrad', 28, 8257536, (28, 9, 128, 256, 0), 5, ('wgrad_kernel<bf16_t, 128, 128, 4>', 154618822656.0, 234356736.0), 6),
    (('bf16', 16, 64, 64, 128, 256), 'defaults', True): ('insar_wgrad_conv3x', 41, 12091392, (41, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 98697216.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'defaults', False): ('insar_wgrad_conv3x', 79, 23298048, (79, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 143523840.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'x0', True): ('insar_wgrad_conv3', 21, 6193152, (21, 9, 256, 128, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 38654705664.0, 75104256.0), 1),
    (('bf16', 16, 64, 64, 128, 256), 'x0', False): ('insar_wgrad_conv3', 41, 12091392, (41, 9, 256, 128, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 38654705664.0, 98697216.0), 1),
    (('bf16', 16, 64, 64, 128, 256), 'y1', True): ('insar_wgrad_conv3y', 42, 12386304, (42, 9, 256, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 99876864.0), 7),
    (('bf16', 16, 64, 64, 128, 256), 'y1', False): ('insar_wgrad_conv3y', 85, 25067520, (85, 9, 256, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 150601728.0), 7),
    (('bf16', 16, 64, 64, 128, 256), 'y2', True): ('insar_wgrad_conv3x', 41, 12091392, (41, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 98697216.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'y2', False): ('insar_wgrad_conv3x', 79, 23298048, (79, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 143523840.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'y3', True): ('insar_wgrad_conv3y', 42, 12386304, (42, 9, 256, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 99876864.0), 7),
    (('bf16', 16, 64, 64, 128, 256), 'y3', False): ('insar_wgrad_conv3y', 85, 25067520, (85, 9, 256, 128, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 150601728.0), 7),
    (('bf16', 16, 64, 64, 128, 256), 'k', True): ('insar_wgrad_conv3x', 41, 12091392, (41, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 98697216.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'k', False): ('insar_wgrad_conv3x', 79, 23298048, (79, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 143523840.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'k4', True): ('insar_wgrad_conv3x', 41, 12091392, (41, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 98697216.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'k4', False): ('insar_wgrad_conv3x', 79, 23298048, (79, 9, 256, 128, 0), 8, ('wgrad3x_kernel<128, 256>', 38654705664.0, 143523840.0), 8),
    (('bf16', 16, 64, 64, 128, 256), 'rows0', True): ('insar_wgrad', 28, 8257536, (28, 9, 256, 128, 0), 5, ('wgrad_kernel<bf16_t, 128, 128, 4>', 38654705664.0, 83361792.0), 6),
    (('bf16', 16, 64, 64, 128, 256), 'rows0', False): ('insar_wgrad', 28, 8257536, (28, 9, 256, 128, 0), 5, ('wgrad_kernel<bf16_t, 128, 128, 4>', 38654705664.0, 83361792.0), 6),
    (('bf16', 16, 64, 64, 256, 256), 'defaults', True): ('insar_wgrad_conv3x', 21, 12386304, (21, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 116654080.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'defaults', False): ('insar_wgrad_conv3x', 41, 24182784, (41, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 163840000.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'x0', True): ('insar_wgrad_conv3', 10, 5898240, (10, 9, 256, 256, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 90701824.0), 1),
    (('bf16', 16, 64, 64, 256, 256), 'x0', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 116654080.0), 1),
    (('bf16', 16, 64, 64, 256, 256), 'y1', True): ('insar_wgrad_conv3y', 21, 12386304, (21, 9, 256, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 116654080.0), 7),
    (('bf16', 16, 64, 64, 256, 256), 'y1', False): ('insar_wgrad_conv3y', 42, 24772608, (42, 9, 256, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 166199296.0), 7),
    (('bf16', 16, 64, 64, 256, 256), 'y2', True): ('insar_wgrad_conv3x', 21, 12386304, (21, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 116654080.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'y2', False): ('insar_wgrad_conv3x', 41, 24182784, (41, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 163840000.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'y3', True): ('insar_wgrad_conv3y', 21, 12386304, (21, 9, 256, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 116654080.0), 7),
    (('bf16', 16, 64, 64, 256, 256), 'y3', False): ('insar_wgrad_conv3y', 42, 24772608, (42, 9, 256, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 166199296.0), 7),
    (('bf16', 16, 64, 64, 256, 256), 'k', True): ('insar_wgrad_conv3x', 21, 12386304, (21, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 116654080.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'k', False): ('insar_wgrad_conv3x', 41, 24182784, (41, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 163840000.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'k4', True): ('insar_wgrad_conv3x', 21, 12386304, (21, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 116654080.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'k4', False): ('insar_wgrad_conv3x', 41, 24182784, (41, 9, 256, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 163840000.0), 8),
    (('bf16', 16, 64, 64, 256, 256), 'rows0', True): ('insar_wgrad', 28, 16515072, (28, 9, 256, 256, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 77309411328.0, 133169152.0), 6),
    (('bf16', 16, 64, 64, 256, 256), 'rows0', False): ('insar_wgrad', 28, 16515072, (28, 9, 256, 256, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 77309411328.0, 133169152.0), 6),
    (('bf16', 16, 64, 64, 512, 256), 'defaults', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 147849216.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'defaults', False): ('insar_wgrad_conv3x', 21, 24772608, (21, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 199753728.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'x0', True): ('insar_wgrad_conv3', 5, 5898240, (5, 9, 256, 512, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 154618822656.0, 124256256.0), 1),
    (('bf16', 16, 64, 64, 512, 256), 'x0', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 154618822656.0, 147849216.0), 1),
    (('bf16', 16, 64, 64, 512, 256), 'y1', True): ('insar_wgrad_conv3y', 10, 11796480, (10, 9, 256, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 147849216.0), 7),
    (('bf16', 16, 64, 64, 512, 256), 'y1', False): ('insar_wgrad_conv3y', 21, 24772608, (21, 9, 256, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 199753728.0), 7),
    (('bf16', 16, 64, 64, 512, 256), 'y2', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 147849216.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'y2', False): ('insar_wgrad_conv3x', 21, 24772608, (21, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 199753728.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'y3', True): ('insar_wgrad_conv3y', 10, 11796480, (10, 9, 256, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 147849216.0), 7),
    (('bf16', 16, 64, 64, 512, 256), 'y3', False): ('insar_wgrad_conv3y', 21, 24772608, (21, 9, 256, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 199753728.0), 7),
    (('bf16', 16, 64, 64, 512, 256), 'k', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 147849216.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'k', False): ('insar_wgrad_conv3x', 21, 24772608, (21, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 199753728.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'k4', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 147849216.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'k4', False): ('insar_wgrad_conv3x', 21, 24772608, (21, 9, 256, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 199753728.0), 8),
    (('bf16', 16, 64, 64, 512, 256), 'rows0', True): ('insar_wgrad', 14, 16515072, (14, 9, 256, 512, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 154618822656.0, 166723584.0), 6),
    (('bf16', 16, 64, 64, 512, 256), 'rows0', False): ('insar_wgrad', 14, 16515072, (14, 9, 256, 512, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 154618822656.0, 166723584.0), 6),
    (('bf16', 16, 32, 32, 256, 512), 'defaults', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 72351744.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'defaults', False): ('insar_wgrad_conv3x', 20, 23592960, (20, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 119537664.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'x0', True): ('insar_wgrad_conv3', 5, 5898240, (5, 9, 512, 256, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 38654705664.0, 48758784.0), 1),
    (('bf16', 16, 32, 32, 256, 512), 'x0', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 38654705664.0, 72351744.0), 1),
    (('bf16', 16, 32, 32, 256, 512), 'y1', True): ('insar_wgrad_conv3y', 10, 11796480, (10, 9, 512, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 72351744.0), 7),
    (('bf16', 16, 32, 32, 256, 512), 'y1', False): ('insar_wgrad_conv3y', 21, 24772608, (21, 9, 512, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 124256256.0), 7),
    (('bf16', 16, 32, 32, 256, 512), 'y2', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 72351744.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'y2', False): ('insar_wgrad_conv3x', 20, 23592960, (20, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 119537664.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'y3', True): ('insar_wgrad_conv3y', 10, 11796480, (10, 9, 512, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 72351744.0), 7),
    (('bf16', 16, 32, 32, 256, 512), 'y3', False): ('insar_wgrad_conv3y', 21, 24772608, (21, 9, 512, 256, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 124256256.0), 7),
    (('bf16', 16, 32, 32, 256, 512), 'k', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 72351744.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'k', False): ('insar_wgrad_conv3x', 20, 23592960, (20, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 119537664.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'k4', True): ('insar_wgrad_conv3x', 10, 11796480, (10, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 72351744.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'k4', False): ('insar_wgrad_conv3x', 20, 23592960, (20, 9, 512, 256, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 119537664.0), 8),
    (('bf16', 16, 32, 32, 256, 512), 'rows0', True): ('insar_wgrad', 14, 16515072, (14, 9, 512, 256, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 38654705664.0, 91226112.0), 6),
    (('bf16', 16, 32, 32, 256, 512), 'rows0', False): ('insar_wgrad', 14, 16515072, (14, 9, 512, 256, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 38654705664.0, 91226112.0), 6),
    (('bf16', 16, 32, 32, 512, 512), 'defaults', True): ('insar_wgrad_conv3x', 5, 11796480, (5, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 80740352.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'defaults', False): ('insar_wgrad_conv3x', 10, 23592960, (10, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 127926272.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'x0', True): ('insar_wgrad_conv3', 4, 9437184, (4, 9, 512, 512, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 71303168.0), 1),
    (('bf16', 16, 32, 32, 512, 512), 'x0', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 80740352.0), 1),
    (('bf16', 16, 32, 32, 512, 512), 'y1', True): ('insar_wgrad_conv3y', 5, 11796480, (5, 9, 512, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 80740352.0), 7),
    (('bf16', 16, 32, 32, 512, 512), 'y1', False): ('insar_wgrad_conv3y', 10, 23592960, (10, 9, 512, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 127926272.0), 7),
    (('bf16', 16, 32, 32, 512, 512), 'y2', True): ('insar_wgrad_conv3x', 5, 11796480, (5, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 80740352.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'y2', False): ('insar_wgrad_conv3x', 10, 23592960, (10, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 127926272.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'y3', True): ('insar_wgrad_conv3y', 5, 11796480, (5, 9, 512, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 80740352.0), 7),
    (('bf16', 16, 32, 32, 512, 512), 'y3', False): ('insar_wgrad_conv3y', 10, 23592960, (10, 9, 512, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 127926272.0), 7),
    (('bf16', 16, 32, 32, 512, 512), 'k', True): ('insar_wgrad_conv3x', 5, 11796480, (5, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 80740352.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'k', False): ('insar_wgrad_conv3x', 10, 23592960, (10, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 127926272.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'k4', True): ('insar_wgrad_conv3x', 5, 11796480, (5, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 80740352.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'k4', False): ('insar_wgrad_conv3x', 10, 23592960, (10, 9, 512, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 127926272.0), 8),
    (('bf16', 16, 32, 32, 512, 512), 'rows0', True): ('insar_wgrad', 7, 16515072, (7, 9, 512, 512, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 77309411328.0, 99614720.0), 6),
    (('bf16', 16, 32, 32, 512, 512), 'rows0', False): ('insar_wgrad', 7, 16515072, (7, 9, 512, 512, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 77309411328.0, 99614720.0), 6),
    (('bf16', 16, 32, 32, 1024, 512), 'defaults', True): ('insar_wgrad_conv3x', 4, 18874368, (4, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 125829120.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'defaults', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 144703488.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'x0', True): ('insar_wgrad_conv3', 2, 9437184, (2, 9, 512, 1024, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 154618822656.0, 88080384.0), 1),
    (('bf16', 16, 32, 32, 1024, 512), 'x0', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 512, 1024, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 154618822656.0, 144703488.0), 1),
    (('bf16', 16, 32, 32, 1024, 512), 'y1', True): ('insar_wgrad_conv3y', 2, 9437184, (2, 9, 512, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 88080384.0), 7),
    (('bf16', 16, 32, 32, 1024, 512), 'y1', False): ('insar_wgrad_conv3y', 5, 23592960, (5, 9, 512, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 144703488.0), 7),
    (('bf16', 16, 32, 32, 1024, 512), 'y2', True): ('insar_wgrad_conv3x', 4, 18874368, (4, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 125829120.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'y2', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 144703488.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'y3', True): ('insar_wgrad_conv3y', 2, 9437184, (2, 9, 512, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 88080384.0), 7),
    (('bf16', 16, 32, 32, 1024, 512), 'y3', False): ('insar_wgrad_conv3y', 5, 23592960, (5, 9, 512, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 154618822656.0, 144703488.0), 7),
    (('bf16', 16, 32, 32, 1024, 512), 'k', True): ('insar_wgrad_conv3x', 4, 18874368, (4, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 125829120.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'k', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 144703488.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'k4', True): ('insar_wgrad_conv3x', 4, 18874368, (4, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 125829120.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'k4', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 512, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 154618822656.0, 144703488.0), 8),
    (('bf16', 16, 32, 32, 1024, 512), 'rows0', True): ('insar_wgrad', 7, 33030144, (7, 9, 512, 1024, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 154618822656.0, 182452224.0), 6),
    (('bf16', 16, 32, 32, 1024, 512), 'rows0', False): ('insar_wgrad', 7, 33030144, (7, 9, 512, 1024, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 154618822656.0, 182452224.0), 6),
    (('bf16', 16, 16, 16, 512, 1024), 'defaults', True): ('insar_wgrad_conv3x', 2, 9437184, (2, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 50331648.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'defaults', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 106954752.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'x0', True): ('insar_wgrad_conv3', 1, 4718592, (1, 9, 1024, 512, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 38654705664.0, 31457280.0), 1),
    (('bf16', 16, 16, 16, 512, 1024), 'x0', False): ('insar_wgrad_conv3', 2, 9437184, (2, 9, 1024, 512, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 38654705664.0, 50331648.0), 1),
    (('bf16', 16, 16, 16, 512, 1024), 'y1', True): ('insar_wgrad_conv3y', 2, 9437184, (2, 9, 1024, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 50331648.0), 7),
    (('bf16', 16, 16, 16, 512, 1024), 'y1', False): ('insar_wgrad_conv3y', 5, 23592960, (5, 9, 1024, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 106954752.0), 7),
    (('bf16', 16, 16, 16, 512, 1024), 'y2', True): ('insar_wgrad_conv3x', 2, 9437184, (2, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 50331648.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'y2', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 106954752.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'y3', True): ('insar_wgrad_conv3y', 2, 9437184, (2, 9, 1024, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 50331648.0), 7),
    (('bf16', 16, 16, 16, 512, 1024), 'y3', False): ('insar_wgrad_conv3y', 5, 23592960, (5, 9, 1024, 512, 0), 7, ('wgrad3y_kernel<128, 128>', 38654705664.0, 106954752.0), 7),
    (('bf16', 16, 16, 16, 512, 1024), 'k', True): ('insar_wgrad_conv3x', 2, 9437184, (2, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 50331648.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'k', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 106954752.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'k4', True): ('insar_wgrad_conv3x', 2, 9437184, (2, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 50331648.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'k4', False): ('insar_wgrad_conv3x', 5, 23592960, (5, 9, 1024, 512, 0), 8, ('wgrad3x_kernel<256, 128>', 38654705664.0, 106954752.0), 8),
    (('bf16', 16, 16, 16, 512, 1024), 'rows0', True): ('insar_wgrad', 3, 14155776, (3, 9, 1024, 512, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 38654705664.0, 69206016.0), 6),
    (('bf16', 16, 16, 16, 512, 1024), 'rows0', False): ('insar_wgrad', 3, 14155776, (3, 9, 1024, 512, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 38654705664.0, 69206016.0), 6),
    (('bf16', 16, 16, 16, 1024, 1024), 'defaults', True): ('insar_wgrad_conv3x', 1, 9437184, (1, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 54525952.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'defaults', False): ('insar_wgrad_conv3x', 2, 18874368, (2, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 92274688.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'x0', True): ('insar_wgrad_conv3', 1, 9437184, (1, 9, 1024, 1024, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 54525952.0), 1),
    (('bf16', 16, 16, 16, 1024, 1024), 'x0', False): ('insar_wgrad_conv3', 1, 9437184, (1, 9, 1024, 1024, 0), 1, ('wgrad3_kernel<bf16_t, 128, 128, 8>', 77309411328.0, 54525952.0), 1),
    (('bf16', 16, 16, 16, 1024, 1024), 'y1', True): ('insar_wgrad_conv3y', 1, 9437184, (1, 9, 1024, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 54525952.0), 7),
    (('bf16', 16, 16, 16, 1024, 1024), 'y1', False): ('insar_wgrad_conv3y', 2, 18874368, (2, 9, 1024, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 92274688.0), 7),
    (('bf16', 16, 16, 16, 1024, 1024), 'y2', True): ('insar_wgrad_conv3x', 1, 9437184, (1, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 54525952.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'y2', False): ('insar_wgrad_conv3x', 2, 18874368, (2, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 92274688.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'y3', True): ('insar_wgrad_conv3y', 1, 9437184, (1, 9, 1024, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 54525952.0), 7),
    (('bf16', 16, 16, 16, 1024, 1024), 'y3', False): ('insar_wgrad_conv3y', 2, 18874368, (2, 9, 1024, 1024, 0), 7, ('wgrad3y_kernel<128, 128>', 77309411328.0, 92274688.0), 7),
    (('bf16', 16, 16, 16, 1024, 1024), 'k', True): ('insar_wgrad_conv3x', 1, 9437184, (1, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 54525952.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'k', False): ('insar_wgrad_conv3x', 2, 18874368, (2, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 92274688.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'k4', True): ('insar_wgrad_conv3x', 1, 9437184, (1, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 54525952.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'k4', False): ('insar_wgrad_conv3x', 2, 18874368, (2, 9, 1024, 1024, 0), 8, ('wgrad3x_kernel<256, 128>', 77309411328.0, 92274688.0), 8),
    (('bf16', 16, 16, 16, 1024, 1024), 'rows0', True): ('insar_wgrad', 3, 28311552, (3, 9, 1024, 1024, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 77309411328.0, 130023424.0), 6),
    (('bf16', 16, 16, 16, 1024, 1024), 'rows0', False): ('insar_wgrad', 3, 28311552, (3, 9, 1024, 1024, 0), 5, ('wgrad_kernel<bf16_t, 256, 256, 8>', 77309411328.0, 130023424.0), 6),
    (('bf16', 2, 90, 90, 64, 64), 'defaults', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 9, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 10),
    (('bf16', 2, 90, 90, 64, 64), 'defaults', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 9, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 10),
    (('bf16', 2, 90, 90, 64, 64), 'x0', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 11, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 12),
    (('bf16', 2, 90, 90, 64, 64), 'x0', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 11, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 12),
    (('bf16', 2, 90, 90, 64, 64), 'y1', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 9, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 10),
    (('bf16', 2, 90, 90, 64, 64), 'y1', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 9, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 10),
    (('bf16', 2, 90, 90, 64, 64), 'y2', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 13, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 14),
    (('bf16', 2, 90, 90, 64, 64), 'y2', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 13, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 14),
    (('bf16', 2, 90, 90, 64, 64), 'y3', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 13, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 14),
    (('bf16', 2, 90, 90, 64, 64), 'y3', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 13, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 14),
    (('bf16', 2, 90, 90, 64, 64), 'k', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 15, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 16),
    (('bf16', 2, 90, 90, 64, 64), 'k', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 15, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 16),
    (('bf16', 2, 90, 90, 64, 64), 'k4', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 15, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 16),
    (('bf16', 2, 90, 90, 64, 64), 'k4', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 15, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 16),
    (('bf16', 2, 90, 90, 64, 64), 'rows0', True): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 5, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 6),
    (('bf16', 2, 90, 90, 64, 64), 'rows0', False): ('insar_wgrad', 51, 1880064, (51, 9, 64, 64, 0), 5, ('wgrad_kernel<bf16_t, 64, 64, 4>', 1194393600.0, 11667456.0), 6),
    (('f32', 8, 256, 256, 64, 128), 'defaults', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 0, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 0),
    (('f32', 8, 256, 256, 64, 128), 'defaults', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 0, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 0),
    (('f32', 8, 256, 256, 64, 128), 'x0', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 1, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 1),
    (('f32', 8, 256, 256, 64, 128), 'x0', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 1, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 1),
    (('f32', 8, 256, 256, 64, 128), 'y1', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 0, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 0),
    (('f32', 8, 256, 256, 64, 128), 'y1', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 0, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 0),
    (('f32', 8, 256, 256, 64, 128), 'y2', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 2, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 2),
    (('f32', 8, 256, 256, 64, 128), 'y2', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 2, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 2),
    (('f32', 8, 256, 256, 64, 128), 'y3', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 2, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 2),
    (('f32', 8, 256, 256, 64, 128), 'y3', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 2, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 2),
    (('f32', 8, 256, 256, 64, 128), 'k', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 3, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 3),
    (('f32', 8, 256, 256, 64, 128), 'k', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 3, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 3),
    (('f32', 8, 256, 256, 64, 128), 'k4', True): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 3, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 3),
    (('f32', 8, 256, 256, 64, 128), 'k4', False): ('insar_wgrad_conv3', 85, 6266880, (85, 9, 128, 64, 0), 3, ('wgrad3_kernel<float, 64, 64, 4>', 77309411328.0, 427720704.0), 3),
    (('f32', 8, 256, 256, 64, 128), 'rows0', True): ('insar_wgrad', 28, 2064384, (28, 9, 128, 64, 0), 5, ('wgrad_kernel<float, 64, 64, 4>', 77309411328.0, 410910720.0), 6),
    (('f32', 8, 256, 256, 64, 128), 'rows0', False): ('insar_wgrad', 28, 2064384, (28, 9, 128, 64, 0), 5, ('wgrad_kernel<float, 64, 64, 4>', 77309411328.0, 410910720.0), 6),
    (('f32', 8, 256, 256, 128, 128), 'defaults', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 0),
    (('f32', 8, 256, 256, 128, 128), 'defaults', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 0),
    (('f32', 8, 256, 256, 128, 128), 'x0', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 1),
    (('f32', 8, 256, 256, 128, 128), 'x0', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 1),
    (('f32', 8, 256, 256, 128, 128), 'y1', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 0),
    (('f32', 8, 256, 256, 128, 128), 'y1', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 0),
    (('f32', 8, 256, 256, 128, 128), 'y2', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 2),
    (('f32', 8, 256, 256, 128, 128), 'y2', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 2),
    (('f32', 8, 256, 256, 128, 128), 'y3', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 2),
    (('f32', 8, 256, 256, 128, 128), 'y3', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 2),
    (('f32', 8, 256, 256, 128, 128), 'k', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 3),
    (('f32', 8, 256, 256, 128, 128), 'k', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 3),
    (('f32', 8, 256, 256, 128, 128), 'k4', True): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 3),
    (('f32', 8, 256, 256, 128, 128), 'k4', False): ('insar_wgrad_conv3', 85, 12533760, (85, 9, 128, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 587005952.0), 3),
    (('f32', 8, 256, 256, 128, 128), 'rows0', True): ('insar_wgrad', 28, 4128768, (28, 9, 128, 128, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 553385984.0), 6),
    (('f32', 8, 256, 256, 128, 128), 'rows0', False): ('insar_wgrad', 28, 4128768, (28, 9, 128, 128, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 553385984.0), 6),
    (('f32', 8, 256, 256, 256, 128), 'defaults', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 0),
    (('f32', 8, 256, 256, 256, 128), 'defaults', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 0),
    (('f32', 8, 256, 256, 256, 128), 'x0', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 1),
    (('f32', 8, 256, 256, 256, 128), 'x0', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 1),
    (('f32', 8, 256, 256, 256, 128), 'y1', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 0),
    (('f32', 8, 256, 256, 256, 128), 'y1', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 0),
    (('f32', 8, 256, 256, 256, 128), 'y2', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 2),
    (('f32', 8, 256, 256, 256, 128), 'y2', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 2),
    (('f32', 8, 256, 256, 256, 128), 'y3', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 2),
    (('f32', 8, 256, 256, 256, 128), 'y3', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 2),
    (('f32', 8, 256, 256, 256, 128), 'k', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 3),
    (('f32', 8, 256, 256, 256, 128), 'k', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 3),
    (('f32', 8, 256, 256, 256, 128), 'k4', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 3),
    (('f32', 8, 256, 256, 256, 128), 'k4', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 128, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 854851584.0), 3),
    (('f32', 8, 256, 256, 256, 128), 'rows0', True): ('insar_wgrad', 14, 4128768, (14, 9, 128, 256, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 309237645312.0, 821821440.0), 6),
    (('f32', 8, 256, 256, 256, 128), 'rows0', False): ('insar_wgrad', 14, 4128768, (14, 9, 128, 256, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 309237645312.0, 821821440.0), 6),
    (('f32', 8, 128, 128, 128, 256), 'defaults', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 0),
    (('f32', 8, 128, 128, 128, 256), 'defaults', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 0),
    (('f32', 8, 128, 128, 128, 256), 'x0', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 1),
    (('f32', 8, 128, 128, 128, 256), 'x0', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 1),
    (('f32', 8, 128, 128, 128, 256), 'y1', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 0),
    (('f32', 8, 128, 128, 128, 256), 'y1', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 0),
    (('f32', 8, 128, 128, 128, 256), 'y2', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 2),
    (('f32', 8, 128, 128, 128, 256), 'y2', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 2),
    (('f32', 8, 128, 128, 128, 256), 'y3', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 2),
    (('f32', 8, 128, 128, 128, 256), 'y3', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 2),
    (('f32', 8, 128, 128, 128, 256), 'k', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 3),
    (('f32', 8, 128, 128, 128, 256), 'k', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 3),
    (('f32', 8, 128, 128, 128, 256), 'k4', True): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 3),
    (('f32', 8, 128, 128, 128, 256), 'k4', False): ('insar_wgrad_conv3', 42, 12386304, (42, 9, 256, 128, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 250871808.0), 3),
    (('f32', 8, 128, 128, 128, 256), 'rows0', True): ('insar_wgrad', 14, 4128768, (14, 9, 256, 128, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 77309411328.0, 217841664.0), 6),
    (('f32', 8, 128, 128, 128, 256), 'rows0', False): ('insar_wgrad', 14, 4128768, (14, 9, 256, 128, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 77309411328.0, 217841664.0), 6),
    (('f32', 8, 128, 128, 256, 256), 'defaults', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 0),
    (('f32', 8, 128, 128, 256, 256), 'defaults', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 0),
    (('f32', 8, 128, 128, 256, 256), 'x0', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 1),
    (('f32', 8, 128, 128, 256, 256), 'x0', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 1),
    (('f32', 8, 128, 128, 256, 256), 'y1', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 0),
    (('f32', 8, 128, 128, 256, 256), 'y1', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 0),
    (('f32', 8, 128, 128, 256, 256), 'y2', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 2),
    (('f32', 8, 128, 128, 256, 256), 'y2', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 2),
    (('f32', 8, 128, 128, 256, 256), 'y3', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 2),
    (('f32', 8, 128, 128, 256, 256), 'y3', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 2),
    (('f32', 8, 128, 128, 256, 256), 'k', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 3),
    (('f32', 8, 128, 128, 256, 256), 'k', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 3),
    (('f32', 8, 128, 128, 256, 256), 'k4', True): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 3),
    (('f32', 8, 128, 128, 256, 256), 'k4', False): ('insar_wgrad_conv3', 21, 12386304, (21, 9, 256, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 317980672.0), 3),
    (('f32', 8, 128, 128, 256, 256), 'rows0', True): ('insar_wgrad', 7, 4128768, (7, 9, 256, 256, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 284950528.0), 6),
    (('f32', 8, 128, 128, 256, 256), 'rows0', False): ('insar_wgrad', 7, 4128768, (7, 9, 256, 256, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 284950528.0), 6),
    (('f32', 8, 128, 128, 512, 256), 'defaults', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 0),
    (('f32', 8, 128, 128, 512, 256), 'defaults', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 0),
    (('f32', 8, 128, 128, 512, 256), 'x0', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 1),
    (('f32', 8, 128, 128, 512, 256), 'x0', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 1),
    (('f32', 8, 128, 128, 512, 256), 'y1', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 0),
    (('f32', 8, 128, 128, 512, 256), 'y1', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 0),
    (('f32', 8, 128, 128, 512, 256), 'y2', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 2),
    (('f32', 8, 128, 128, 512, 256), 'y2', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 2),
    (('f32', 8, 128, 128, 512, 256), 'y3', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 2),
    (('f32', 8, 128, 128, 512, 256), 'y3', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 2),
    (('f32', 8, 128, 128, 512, 256), 'k', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 3),
    (('f32', 8, 128, 128, 512, 256), 'k', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 3),
    (('f32', 8, 128, 128, 512, 256), 'k4', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 3),
    (('f32', 8, 128, 128, 512, 256), 'k4', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 256, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 449839104.0), 3),
    (('f32', 8, 128, 128, 512, 256), 'rows0', True): ('insar_wgrad', 7, 8257536, (7, 9, 256, 512, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 309237645312.0, 435683328.0), 6),
    (('f32', 8, 128, 128, 512, 256), 'rows0', False): ('insar_wgrad', 7, 8257536, (7, 9, 256, 512, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 309237645312.0, 435683328.0), 6),
    (('f32', 8, 64, 64, 256, 512), 'defaults', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 0),
    (('f32', 8, 64, 64, 256, 512), 'defaults', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 0),
    (('f32', 8, 64, 64, 256, 512), 'x0', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 1),
    (('f32', 8, 64, 64, 256, 512), 'x0', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 1),
    (('f32', 8, 64, 64, 256, 512), 'y1', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 0),
    (('f32', 8, 64, 64, 256, 512), 'y1', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 0),
    (('f32', 8, 64, 64, 256, 512), 'y2', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 2),
    (('f32', 8, 64, 64, 256, 512), 'y2', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 2),
    (('f32', 8, 64, 64, 256, 512), 'y3', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 2),
    (('f32', 8, 64, 64, 256, 512), 'y3', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 2),
    (('f32', 8, 64, 64, 256, 512), 'k', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 3),
    (('f32', 8, 64, 64, 256, 512), 'k', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 3),
    (('f32', 8, 64, 64, 256, 512), 'k4', True): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 3),
    (('f32', 8, 64, 64, 256, 512), 'k4', False): ('insar_wgrad_conv3', 10, 11796480, (10, 9, 512, 256, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 147849216.0), 3),
    (('f32', 8, 64, 64, 256, 512), 'rows0', True): ('insar_wgrad', 7, 8257536, (7, 9, 512, 256, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 77309411328.0, 133693440.0), 6),
    (('f32', 8, 64, 64, 256, 512), 'rows0', False): ('insar_wgrad', 7, 8257536, (7, 9, 512, 256, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 77309411328.0, 133693440.0), 6),
    (('f32', 8, 64, 64, 512, 512), 'defaults', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 0),
    (('f32', 8, 64, 64, 512, 512), 'defaults', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 0),
    (('f32', 8, 64, 64, 512, 512), 'x0', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 1),
    (('f32', 8, 64, 64, 512, 512), 'x0', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 1),
    (('f32', 8, 64, 64, 512, 512), 'y1', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 0),
    (('f32', 8, 64, 64, 512, 512), 'y1', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 0),
    (('f32', 8, 64, 64, 512, 512), 'y2', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 2),
    (('f32', 8, 64, 64, 512, 512), 'y2', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 2),
    (('f32', 8, 64, 64, 512, 512), 'y3', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 2),
    (('f32', 8, 64, 64, 512, 512), 'y3', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 2),
    (('f32', 8, 64, 64, 512, 512), 'k', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 3),
    (('f32', 8, 64, 64, 512, 512), 'k', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 3),
    (('f32', 8, 64, 64, 512, 512), 'k4', True): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 3),
    (('f32', 8, 64, 64, 512, 512), 'k4', False): ('insar_wgrad_conv3', 5, 11796480, (5, 9, 512, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 181403648.0), 3),
    (('f32', 8, 64, 64, 512, 512), 'rows0', True): ('insar_wgrad', 7, 16515072, (7, 9, 512, 512, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 200278016.0), 6),
    (('f32', 8, 64, 64, 512, 512), 'rows0', False): ('insar_wgrad', 7, 16515072, (7, 9, 512, 512, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 200278016.0), 6),
    (('f32', 8, 64, 64, 1024, 512), 'defaults', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 0),
    (('f32', 8, 64, 64, 1024, 512), 'defaults', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 0),
    (('f32', 8, 64, 64, 1024, 512), 'x0', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 1),
    (('f32', 8, 64, 64, 1024, 512), 'x0', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 1),
    (('f32', 8, 64, 64, 1024, 512), 'y1', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 0),
    (('f32', 8, 64, 64, 1024, 512), 'y1', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 0),
    (('f32', 8, 64, 64, 1024, 512), 'y2', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 2),
    (('f32', 8, 64, 64, 1024, 512), 'y2', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 2),
    (('f32', 8, 64, 64, 1024, 512), 'y3', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 2),
    (('f32', 8, 64, 64, 1024, 512), 'y3', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 2),
    (('f32', 8, 64, 64, 1024, 512), 'k', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 3),
    (('f32', 8, 64, 64, 1024, 512), 'k', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 3),
    (('f32', 8, 64, 64, 1024, 512), 'k4', True): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 3),
    (('f32', 8, 64, 64, 1024, 512), 'k4', False): ('insar_wgrad_conv3', 8, 37748736, (8, 9, 512, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 3),
    (('f32', 8, 64, 64, 1024, 512), 'rows0', True): ('insar_wgrad', 8, 37748736, (8, 9, 512, 1024, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 6),
    (('f32', 8, 64, 64, 1024, 512), 'rows0', False): ('insar_wgrad', 8, 37748736, (8, 9, 512, 1024, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 309237645312.0, 352321536.0), 6),
    (('f32', 8, 32, 32, 512, 1024), 'defaults', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 0),
    (('f32', 8, 32, 32, 512, 1024), 'defaults', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 0),
    (('f32', 8, 32, 32, 512, 1024), 'x0', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 1),
    (('f32', 8, 32, 32, 512, 1024), 'x0', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 1),
    (('f32', 8, 32, 32, 512, 1024), 'y1', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 0),
    (('f32', 8, 32, 32, 512, 1024), 'y1', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 0),
    (('f32', 8, 32, 32, 512, 1024), 'y2', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 2),
    (('f32', 8, 32, 32, 512, 1024), 'y2', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 2),
    (('f32', 8, 32, 32, 512, 1024), 'y3', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 2),
    (('f32', 8, 32, 32, 512, 1024), 'y3', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 2),
    (('f32', 8, 32, 32, 512, 1024), 'k', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 3),
    (('f32', 8, 32, 32, 512, 1024), 'k', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 3),
    (('f32', 8, 32, 32, 512, 1024), 'k4', True): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 3),
    (('f32', 8, 32, 32, 512, 1024), 'k4', False): ('insar_wgrad_conv3', 5, 23592960, (5, 9, 1024, 512, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 77309411328.0, 144703488.0), 3),
    (('f32', 8, 32, 32, 512, 1024), 'rows0', True): ('insar_wgrad', 4, 18874368, (4, 9, 1024, 512, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 77309411328.0, 125829120.0), 6),
    (('f32', 8, 32, 32, 512, 1024), 'rows0', False): ('insar_wgrad', 4, 18874368, (4, 9, 1024, 512, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 77309411328.0, 125829120.0), 6),
    (('f32', 8, 32, 32, 1024, 1024), 'defaults', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 0),
    (('f32', 8, 32, 32, 1024, 1024), 'defaults', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 0),
    (('f32', 8, 32, 32, 1024, 1024), 'x0', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 1),
    (('f32', 8, 32, 32, 1024, 1024), 'x0', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 1, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 1),
    (('f32', 8, 32, 32, 1024, 1024), 'y1', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 0),
    (('f32', 8, 32, 32, 1024, 1024), 'y1', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 0, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 0),
    (('f32', 8, 32, 32, 1024, 1024), 'y2', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 2),
    (('f32', 8, 32, 32, 1024, 1024), 'y2', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 2),
    (('f32', 8, 32, 32, 1024, 1024), 'y3', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 2),
    (('f32', 8, 32, 32, 1024, 1024), 'y3', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 2, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 2),
    (('f32', 8, 32, 32, 1024, 1024), 'k', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 3),
    (('f32', 8, 32, 32, 1024, 1024), 'k', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 3),
    (('f32', 8, 32, 32, 1024, 1024), 'k4', True): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 3),
    (('f32', 8, 32, 32, 1024, 1024), 'k4', False): ('insar_wgrad_conv3', 4, 37748736, (4, 9, 1024, 1024, 0), 3, ('wgrad3_kernel<float, 128, 128, 8>', 154618822656.0, 218103808.0), 3),
    (('f32', 8, 32, 32, 1024, 1024), 'rows0', True): ('insar_wgrad', 2, 18874368, (2, 9, 1024, 1024, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 142606336.0), 6),
    (('f32', 8, 32, 32, 1024, 1024), 'rows0', False): ('insar_wgrad', 2, 18874368, (2, 9, 1024, 1024, 0), 5, ('wgrad_kernel<float, 128, 128, 8>', 154618822656.0, 142606336.0), 6),
}

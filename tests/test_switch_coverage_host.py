"""CPU: every kernel-selecting switch and every library knob is held by a named test, or exempt for a stated reason.

COVERAGE maps every INSAR_* variable the package reads (switches.declared()) and every knob of csrc/api.hip to
(what it selects, the tests that flip it, how they hold it). A hold is "exact" (integer operands, torch.equal against an
integer reference), "bitwise" (bit for bit the default path's result), "tolerance" (the parity tolerances of the named test)
or "exempt"; an exempt entry names no test and gives one of the allowed reasons: host-only, path-only, a scheduling hint, a
list of knobs (each held on its own) or experiment builds only. The test fails when a declared switch or knob is missing from
the table, when the table names something that no longer exists, when a named test does not exist, and when the table in
DESIGN.md ("Switches and the tests that hold them") differs from the one rendered here."""
import importlib
import os
import re

from insar_unet_ca_amd import switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, W, S, P = "tests.test_switch_routes_gpu", "tests.test_switch_wgrad_gpu", "tests.test_switch_streams_gpu", "tests.test_parity_gpu"
EXEMPT_REASONS = ("host-only", "path-only", "scheduling hint", "knob list", "experiment builds only")

# name -> (what it selects, [module::test, ...] or an exemption reason, hold)
COVERAGE = {
    "INSAR_C64": ("64 -> 64 register-weight kernel: both directions / 0 none / fwd / bwd", [R + "::test_insar_c64"], "exact"),
    "INSAR_BSTAT_C64": ("the 64 -> 64 kernel's BatchNorm-backward sums epilogue", [R + "::test_bstat_c64_off"], "exact"),
    "INSAR_BSTAT_FUSE": ("BatchNorm-backward sums in the producer GEMM's epilogue",
                         ["tests.test_bstat_gpu::test_training_step_with_and_without_the_fusion"], "tolerance"),
    "INSAR_FLAT_ROWS": ("flat kernel's row tiles instead of the per-tap GEMM", [R + "::test_flat_rows_off"], "exact"),
    "INSAR_FLAT2": ("two-work-group flat kernel: 0 8-wave / 1 row tiles / 2 one group per tile / 3 flat geometry",
                    [R + "::test_flat2", R + "::test_flat2_kmax", "tests.test_bstat_gpu::test_flat_kernel_epilogue_sums_against_the_reduce_pass"], "exact"),
    "INSAR_FLAT2_KMAX": ("two-work-group row tiles instead of 256 x 256 per-tap tiles up to this K", [R + "::test_flat2_kmax"], "exact"),
    "INSAR_FLAT2_PERSIST": ("persistent grids of the two-work-group kernel: 0 never / 1 forward / 2 all", [R + "::test_flat2_persist"], "exact"),
    "INSAR_FLAT_PP": ("8-wave flat kernel: ping-pong tap steps or the plain loop", [R + "::test_flat_pp_off"], "exact"),
    "INSAR_FLAT_PERSIST": ("8-wave flat kernel: persistent work-groups 0 never / 1 forward / 2 all", [R + "::test_flat_persist"], "exact"),
    "INSAR_STAT_PREFOLD_ROWS": ("statistics slabs above this many rows are pre-folded (insar_colsum_partial)", [R + "::test_stat_prefold_rows"], "exact"),
    "INSAR_IGEMM_PP": ("256 x 256 per-tap tiles: ping-pong K loop or the plain loop", [P + "::test_pingpong_k_loop_is_bitwise_the_plain_loop"], "bitwise"),
    "INSAR_WGRAD_ROWS": ("row-of-taps weight-gradient kernels or the per-tap kernel", [W + "::test_wgrad_rows_off"], "exact"),
    "INSAR_WGRAD_X": ("wgrad3x (256 x 128 tiles) or wgrad3 (128 x 128)", [W + "::test_wgrad_x_off"], "exact"),
    "INSAR_WGRAD_Y": ("wgrad3y instead of wgrad3x (bit 0) / of wgrad3<128,128> (bit 1)", [W + "::test_wgrad_y"], "exact"),
    "INSAR_WGRAD_K": ("wgrad3k for the tiles INSAR_WGRAD_K_TILES names", [W + "::test_wgrad_k"], "exact"),
    "INSAR_WGRAD_K_TILES": ("the (Cin x Cout) tiles that take wgrad3k; a tile left out keeps the default kernel (that case changes nothing by construction)",
                            [W + "::test_wgrad_k"], "exact"),
    "INSAR_WGRAD_GRID_CAP": ("largest grid of an 8-wave weight gradient beside the dgrad chain (bf16: fp32 fills every slot and is never capped)",
                             [W + "::test_wgrad_grid_cap"], "exact"),
    "INSAR_WGRAD_FILL": ("slot share of wgrad3x / 3y / 3k beside a side stream (without one it does not apply: asserted unchanged)", [W + "::test_wgrad_fill"], "exact"),
    "INSAR_WGRAD_FILL_SMALL": ("slot share of wgrad3 beside a side stream (without one it does not apply: asserted unchanged)",
                               [W + "::test_wgrad_fill", W + "::test_wgrad_fill_alone_fp32"], "exact"),
    "INSAR_WGRAD_FILL_ALONE": ("slot share of the 3x3 weight gradients without a side stream (with one it does not apply: asserted unchanged)",
                               [W + "::test_wgrad_fill", W + "::test_wgrad_fill_alone_fp32"], "exact"),
    "INSAR_WGRAD_FILL_T": ("slot share of the transposed convs' weight gradient (bf16 beside a side stream; elsewhere asserted unchanged)", [W + "::test_wgrad_fill_t"], "exact"),
    "INSAR_WGRAD_FILL_DL": ("slot share of DeepLabV3-CA's per-tap weight gradients (bf16 beside a side stream; elsewhere asserted unchanged)", [W + "::test_wgrad_fill_dl"], "exact"),
    "INSAR_WGRAD_ORDER": ("weight gradient issued before or after the unit's input gradient",
                          ["tests.test_conv_transpose_gpu::test_up_plan_gradients_do_not_depend_on_the_issue_order"], "bitwise"),
    "INSAR_SIDE_STREAM": ("weight gradients and re-layouts on a second stream or all on one",
                          [S + "::test_stream_placement_is_bitwise_neutral", S + "::test_deeplab_step_without_a_side_stream_is_bitwise",
                           W + "::test_wgrad_fill", W + "::test_wgrad_fill_t", W + "::test_wgrad_fill_dl"], "bitwise"),
    "INSAR_PREP_SIDE": ("U-Net plan: weight re-layout on the side or the main stream (the DeepLabV3-CA plan does not read it)",
                        [S + "::test_stream_placement_is_bitwise_neutral"], "bitwise"),
    "INSAR_SMALL_WGRAD_MAIN": ("U-Net's first layer: weight gradient on the main or the side stream (no such layer in DeepLabV3-CA)",
                               [S + "::test_stream_placement_is_bitwise_neutral"], "bitwise"),
    "INSAR_SMALL_WGRAD_FUSE": ("first layer: BatchNorm-backward apply pass inside the weight-gradient kernel",
                               [P + "::test_first_layer_weight_gradient_with_the_apply_pass_inside_is_bitwise"], "bitwise"),
    "INSAR_ADAM_CHUNK": ("elements per work-group of the multi-tensor optimizer launches", [S + "::test_adam_chunk_size_is_bitwise_neutral"], "bitwise"),
    "INSAR_COEF_SIMPLE": ("channel-parallel coefficient kernel or the ticket kernel",
                          [P + "::test_channel_parallel_coefficient_kernel_against_the_two_stage_kernels",
                           P + "::test_single_launch_coefficient_stages_are_bitwise_the_two_launches"], "tolerance"),
    "INSAR_COEF_FUSE": ("coefficient stages in one launch or two", [P + "::test_single_launch_coefficient_stages_are_bitwise_the_two_launches"], "bitwise"),
    "INSAR_SPLIT_COEF": ("batch fold of the coefficients on the side stream", [P + "::test_split_backward_coefficients_are_bitwise_the_fused_launch"], "bitwise"),
    "INSAR_OUTC_FUSE": ("outc's input gradient recomputed or materialised", [P + "::test_recomputed_outc_gradient_is_bitwise_the_materialised_one"], "bitwise"),
    "INSAR_OUTC_WGRAD_FUSE": ("outc's weight gradient from the reduce pass or a pass of its own",
                              [P + "::test_outc_weight_gradient_from_the_reduce_pass"], "tolerance"),
    "INSAR_POOL_FUSE": ("max-pool gradient inside BatchNorm backward or insar_maxpool2_bwd",
                        [P + "::test_pool_gradient_inside_bn_backward_is_bitwise_maxpool2_bwd"], "bitwise"),
    "INSAR_GATE_FUSE": ("residual ReLU gate in the dgrad GEMM's epilogue", ["tests.test_deeplab_gpu::test_residual_relu_gate_in_the_gemm_epilogue"], "tolerance"),
    "INSAR_GATE_STATS": ("BatchNorm-backward sums from the gating GEMM", ["tests.test_deeplab_gpu::test_residual_relu_gate_in_the_gemm_epilogue"], "tolerance"),
    "INSAR_TAPE": ("launch tapes off / on / verify: replays the same launches", "host-only", "exempt"),
    "INSAR_HIP_LIB": ("another build of the library", "path-only", "exempt"),
    "INSAR_TUNE": ("sets the knobs below when the library is loaded", "knob list", "exempt"),
    "INSAR_SIDE_PRIORITY": ("HIP priority of the side stream", "scheduling hint", "exempt"),
    "INSAR_SIDE_CU_MASK": ("compute units the side stream may use", "scheduling hint", "exempt"),
    # library knobs (insar_tune_set)
    "wgrad3_m32": ("wgrad3<128,128>: 32x32x16 MFMA fragments", ["tests.test_wgrad3_exact_gpu::test_wgrad_conv3_bf16_32x32x16_fragments"], "exact"),
    "igemm_xwide_min": ("work-groups from which the per-tap GEMM takes 256 x 256 tiles",
                        [R + "::test_knobs_igemm_wide_tiles_lowered", R + "::test_knobs_igemm_wide_tiles_raised"], "exact"),
    "igemm_wide_min": ("work-groups from which the per-tap GEMM takes 256 x 128 tiles",
                       [R + "::test_knobs_igemm_wide_tiles_lowered", R + "::test_knobs_igemm_wide_tiles_raised"], "exact"),
    "wgrad_tile_max": ("largest tile edge of the per-tap weight gradient (bf16 only: fp32 never takes 256 x 256)", [W + "::test_knob_wgrad_tile_max"], "exact"),
    "c64_grid_bwd": ("work-groups of the 64 -> 64 kernel's input-gradient launches", [R + "::test_knob_c64_grid_bwd"], "exact"),
    "wgrad3x_var": ("timing ablations of wgrad3x.hip's K loop; the product library ignores it", "experiment builds only", "exempt"),
}

BEGIN, END = "<!-- switch coverage: begin -->", "<!-- switch coverage: end -->"


def knob_names():
    """The knob list of csrc/api.hip, read as text (the way switches.py reads its own package)."""
    src = open(os.path.join(ROOT, "insar_unet_ca_amd", "csrc", "api.hip")).read()
    body = re.search(r"g_knob_names\[KNOB_COUNT\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    names = re.findall(r'^\s*"([a-z0-9_]+)"\s*,', body, re.M)
    assert names
    return names


def render():
    """The table of DESIGN.md, one row per COVERAGE entry."""
    rows = ["| switch / knob | selects | held by | hold |", "|---|---|---|---|"]
    for name, (selects, held, hold) in COVERAGE.items():
        by = held if isinstance(held, str) else ", ".join("`%s`" % t.replace("tests.", "").replace("::", ".py::") for t in held)
        rows.append(f"| `{name}` | {selects} | {by} | {hold} |")
    return "\n".join(rows)


def test_every_switch_and_knob_is_in_the_table():
    declared = set(switches.declared()) | set(knob_names())
    missing = sorted(declared - set(COVERAGE))
    assert not missing, f"no test and no reason for {missing}: add a GPU test that flips it, then a row here and in DESIGN.md"
    stale = sorted(set(COVERAGE) - declared)
    assert not stale, f"the table names {stale}, which the package no longer declares"


def test_every_named_test_exists_and_every_exemption_has_an_allowed_reason():
    for name, (selects, held, hold) in COVERAGE.items():
        assert selects and hold in ("exact", "bitwise", "tolerance", "exempt"), name
        if hold == "exempt":
            assert held in EXEMPT_REASONS, f"{name}: {held!r} is not an allowed reason"
            continue
        assert isinstance(held, list) and held, name
        for ref in held:
            mod, fn = ref.split("::")
            assert callable(getattr(importlib.import_module(mod), fn, None)), f"{name}: {ref} does not exist"


def test_kernel_selecting_switches_are_not_exempt_as_host_only():
    """switches.HOST_ONLY (what bench.py lets through) and the table's host-only exemptions are the same set."""
    assert {n for n, (_, held, _) in COVERAGE.items() if held == "host-only"} == set(switches.HOST_ONLY)


def test_design_md_carries_this_table():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert BEGIN in text and END in text, "DESIGN.md lost its switch coverage table"
    got = text.split(BEGIN)[1].split(END)[0].strip()
    assert got == render(), "DESIGN.md's switch table differs from tests/test_switch_coverage_host.py: paste render()'s output between the markers"

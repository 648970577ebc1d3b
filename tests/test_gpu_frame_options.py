"""-m gpu: what rt_set_option refuses, what it puts back, how it lays the per-path buffers out, and that the banks of RT_OPT_SAMPLES_AHEAD follow
every option they are documented to follow.

  * Refusals: every `return fail(...)` of rt_set_option that a caller can reach (the one for a bank -- "RT_OPT_SAMPLES_AHEAD on a bank" -- needs a
    bank's handle, which no entry point hands out), with the exact message; the frame's layout statistics are what they were, and the frame then
    renders the golden radiance bit for bit.
  * Rollback: a layout that fails under RT_OPT_DEBUG_ALLOC_LIMIT leaves the old option and the old statistics.
  * Layout grid: the five layout statistics over a fixed grid of options, against tests/golden/frame_layout.json -- recorded from the build BEFORE
    the frame code was refactored (`python -m tests.test_gpu_frame_options --record > tests/golden/frame_layout.json`) -- and against the rule
    include/rt_hip.h documents: path_state_bytes = chunk_pixels x samples_in_flight x pipelines x bytes per path (412 at 8 bounces, full layout).
  * Banks: one case per followed option, written out here (not read from the library)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from raytracing_amd import capi, scenes as S, types as T   # noqa: E402

pytestmark = pytest.mark.gpu

CASE = ("coverage_64_b6_s2", "coverage", 64, 64, 6, 2)
FIVE = ("samples_in_flight", "chunk_pixels", "pipelines", "log_inline_entries", "path_state_bytes")
LAYOUT_JSON = os.path.join(ROOT, "tests", "golden", "frame_layout.json")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def five(fr):
    st = fr.stats()
    return tuple(int(getattr(st, k)) for k in FIVE)


def stage_sample(fr, bounces, started=False):
    if not started:
        fr.generate_rays()
    for b in range(bounces + 1):
        fr.intersect(b); fr.shade(b); fr.intersect_shadow(b)
    fr.advance_sample()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
DENOISER_ON_TILES = ("rt_set_option: the temporal denoiser reprojects across rows and needs the whole image on one GPU (tile_count == 1); "
                     "on tiles use RT_OPT_DENOISER = 2 + rt_group_denoise")
# name: (option, value, message, what the frame is in the middle of: None / "sample" (a stage sample in flight) / "recorded" (RT_OPT_FRAME_KERNEL: recorded))
REFUSALS = {
    "samples_ahead_65": (capi.OPT_SAMPLES_AHEAD, 65, "rt_set_option: RT_OPT_SAMPLES_AHEAD is 0 (off), 1 (automatic depth) or 2..64 samples per batch (+ 256: one stream per bank)", None),
    "samples_ahead_256_plus_200": (capi.OPT_SAMPLES_AHEAD, 256 + 200, "rt_set_option: RT_OPT_SAMPLES_AHEAD is 0 (off), 1 (automatic depth) or 2..64 samples per batch (+ 256: one stream per bank)", None),
    "max_bounces": (capi.OPT_MAX_BOUNCES, 63, "rt_set_option: max_bounces above RT_MAX_BOUNCES_LIMIT", None),
    "samples_in_flight": (capi.OPT_SAMPLES_IN_FLIGHT, 1025, "rt_set_option: samples in flight must be 0 (auto) or 1..1024", None),
    "sampler_value": (capi.OPT_SAMPLER, 2, "rt_set_option: sampler must be 0 (kRandom) or 1 (kBlueNoise)", None),
    "sampler_without_tables": (capi.OPT_SAMPLER, 1, "rt_set_option: SamplerType::kBlueNoise needs rt_upload_blue_noise_tables first", None),
    "aov": (capi.OPT_AOV, 5, "rt_set_option: AOV index must be 0..4", None),
    "denoiser_value": (capi.OPT_DENOISER, 3, "rt_set_option: RT_OPT_DENOISER is 0, 1 or 2", None),
    "packet_bounces": (capi.OPT_PACKET_BOUNCES, 1, "rt_set_option: the packet kernel was removed (RT_OPT_TRACE_PACKET_BOUNCES accepts only 0)", None),
    "pipelines_0": (capi.OPT_PIPELINES, 0, "rt_set_option: pipelines must be 1..RT_MAX_PIPES", None),
    "pipelines_5": (capi.OPT_PIPELINES, 5, "rt_set_option: pipelines must be 1..RT_MAX_PIPES", None),
    "frame_kernel_mid_sample": (capi.OPT_FRAME_KERNEL, 0, "rt_set_option: RT_OPT_FRAME_KERNEL cannot change while a sample is in flight (rt_advance_sample first)", "recorded"),
    "stage_pipes_0": (capi.OPT_STAGE_PIPES, 0, "rt_set_option: stage pipes must be 1..RT_MAX_PIPES", None),
    "stage_pipes_5": (capi.OPT_STAGE_PIPES, 5, "rt_set_option: stage pipes must be 1..RT_MAX_PIPES", None),
    "stage_pipes_mid_sample": (capi.OPT_STAGE_PIPES, 2, "rt_set_option: RT_OPT_STAGE_PIPES cannot change while a sample is in flight (rt_advance_sample first)", "sample"),
    "log_pool_div": (capi.OPT_DEBUG_LOG_POOL_DIV, 0, "rt_set_option: RT_OPT_DEBUG_LOG_POOL_DIV must be >= 1", None),
    "compact_log": (capi.OPT_COMPACT_LOG, 3, "rt_set_option: RT_OPT_COMPACT_LOG is 0, 1 or 2", None),
    "trace_variant": (capi.OPT_TRACE_VARIANT, 3, "rt_set_option: unknown trace kernel variant (0, 5, 8..11)", None),
    "unknown_option": (99, 0, "rt_set_option: unknown option", None),
}


def golden_frame(ctx, golden, tile_count=1):
    name, _, w, h, bounces, _ = CASE
    fr = capi.Frame(ctx, w, h, tile_count=tile_count)
    fr.set_camera(golden[name + "/camera"])
    fr.set_max_bounces(bounces)
    return fr


@pytest.mark.parametrize("refusal", sorted(REFUSALS))
def test_a_refused_option_leaves_the_frame_as_it_was(refusal, ctx, golden_scenes, golden_radiance):
    option, value, message, mid = REFUSALS[refusal]
    name, key, _, _, bounces, spp = CASE
    ctx.upload_scene(golden_scenes[key])                  # (this module's context never gets the blue-noise tables)
    fr = golden_frame(ctx, golden_radiance)
    if mid == "recorded":
        fr.set_option(capi.OPT_FRAME_KERNEL, 1)
    before = five(fr)                                     # (rt_frame_get_stats replays recorded stages: read before the sample starts)
    if mid:
        fr.generate_rays()
    with pytest.raises(capi.RtError) as e:
        fr.set_option(option, value)
    assert str(e.value) == message
    if mid:                                               # the sample in flight goes on, the rest follow through the stages
        stage_sample(fr, bounces, started=True)           # (rt_frame_get_stats folds the live queue counters: not between two stages)
        assert five(fr) == before
        for _ in range(spp - 1):
            stage_sample(fr, bounces)
    else:
        assert five(fr) == before
        fr.integrate(spp)
    assert np.array_equal(fr.radiance()[..., :3], golden_radiance[name + "/radiance"])
    assert five(fr)[1:4] == before[1:4]
    fr.close()


def test_the_temporal_denoiser_is_refused_on_a_tile(ctx, golden_scenes, golden_radiance):
    name, key, w, h, bounces, spp = CASE
    ctx.upload_scene(golden_scenes[key])
    fr = golden_frame(ctx, golden_radiance, tile_count=2)
    whole = golden_frame(ctx, golden_radiance)
    before = five(fr)
    with pytest.raises(capi.RtError) as e:
        fr.set_option(capi.OPT_DENOISER, 1)
    assert str(e.value) == DENOISER_ON_TILES
    assert five(fr) == before
    fr.integrate(spp); whole.integrate(spp)
    assert np.array_equal(whole.radiance()[..., :3], golden_radiance[name + "/radiance"])
    assert np.array_equal(fr.radiance(), whole.radiance()[fr.global_rows()])
    fr.close(); whole.close()


def test_a_null_frame_is_refused(ctx, golden_scenes, golden_radiance):
    name, key, _, _, _, spp = CASE
    ctx.upload_scene(golden_scenes[key])
    fr = golden_frame(ctx, golden_radiance)
    before = five(fr)
    lib = capi.load()
    assert lib.rt_set_option(None, capi.OPT_MAX_BOUNCES, 1) != 0
    assert lib.rt_last_error(None).decode() == "rt_set_option: frame is NULL"
    assert five(fr) == before
    fr.integrate(spp)
    assert np.array_equal(fr.radiance()[..., :3], golden_radiance[name + "/radiance"])
    fr.close()


# ---- rollback ---------------------------------------------------------------------------------------------------------------------------
ALLOC_LIMIT = "out of device memory for the per-path buffers (RT_OPT_DEBUG_ALLOC_LIMIT)"


@pytest.mark.parametrize("k", [1, 2, 5])
def test_samples_in_flight_beyond_the_alloc_limit_are_put_back(k, ctx, golden_scenes, golden_radiance):
    name, key, _, _, _, spp = CASE
    ctx.upload_scene(golden_scenes[key])
    fr, untouched = golden_frame(ctx, golden_radiance), golden_frame(ctx, golden_radiance)
    if k > 1:
        fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, k)      # an explicit count that fits: the one to come back to
    fr.set_option(capi.OPT_DEBUG_ALLOC_LIMIT, k)
    before = five(fr)
    with pytest.raises(capi.RtError) as e:
        fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, k + 1)
    assert str(e.value) == ALLOC_LIMIT
    assert five(fr) == before
    fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, k if k > 1 else 0)          # the old value is still the frame's: nothing happens
    assert five(fr) == before
    fr.integrate(spp); untouched.integrate(spp)
    assert np.array_equal(fr.radiance(), untouched.radiance())
    assert np.array_equal(fr.radiance()[..., :3], golden_radiance[name + "/radiance"])
    fr.close(); untouched.close()


def test_a_path_state_limit_that_cannot_be_laid_out_is_put_back(ctx, golden_scenes, golden_radiance):
    name, key, _, _, _, spp = CASE
    ctx.upload_scene(golden_scenes[key])
    fr, untouched = golden_frame(ctx, golden_radiance), golden_frame(ctx, golden_radiance)
    fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 4)
    fr.set_option(capi.OPT_DEBUG_ALLOC_LIMIT, 2)          # from here on no layout for the frame's four samples in flight succeeds
    before = five(fr)
    with pytest.raises(capi.RtError) as e:
        fr.set_option(capi.OPT_PATH_STATE_LIMIT_MB, 1)
    assert str(e.value) == ALLOC_LIMIT
    assert five(fr) == before
    # the old limit (none) is back: setting it again is no change, so it succeeds although no layout would
    fr.set_option(capi.OPT_PATH_STATE_LIMIT_MB, 0)
    assert five(fr) == before
    # (the hook refused the rollback's own layout as well: the frame gets its buffers with the next layout -- ask for one before anything is launched)
    fr.set_option(capi.OPT_DEBUG_ALLOC_LIMIT, 0)
    fr.set_option(capi.OPT_SAMPLES_IN_FLIGHT, 3)
    fr.integrate(spp); untouched.integrate(spp)
    assert np.array_equal(fr.radiance(), untouched.radiance())
    assert np.array_equal(fr.radiance()[..., :3], golden_radiance[name + "/radiance"])
    fr.close(); untouched.close()


# ---- layout grid ------------------------------------------------------------------------------------------------------------------------
# (side of a square frame, RT_OPT_MAX_BOUNCES, RT_OPT_SAMPLES_IN_FLIGHT, RT_OPT_PATH_STATE_LIMIT_MB, RT_OPT_COMPACT_LOG, RT_OPT_PIPELINES, RT_OPT_STAGE_PIPES),
# set in the order bounces, compact log, pipelines, stage pipes, limit, samples in flight.  No point holds more than ~220 MiB of path state.
GRID = [
    (64, 3, 0, 0, 2, 1, 1), (64, 8, 1, 0, 2, 1, 1), (64, 8, 8, 0, 0, 1, 1), (64, 8, 8, 0, 2, 1, 1),
    (64, 8, 8, 0, 1, 1, 1),       # compact on: asked for, 8 in flight, 18 entries
    (64, 8, 7, 0, 1, 1, 1),       # ... not with 7 in flight
    (64, 3, 8, 0, 1, 1, 1),       # ... nor with 8 log entries
    (64, 4, 8, 0, 1, 1, 1),       # ... 10 are the fewest
    (64, 8, 8, 8, 2, 1, 1),       # compact on: the caller bounds the path state
    (64, 8, 16, 8, 2, 2, 1),      # ... not with two pipelines
    (64, 16, 16, 0, 1, 1, 1), (64, 16, 16, 1, 0, 1, 1),                   # (a limit cannot cut below 4096 pixels)
    (256, 8, 1, 0, 2, 1, 1), (256, 8, 8, 0, 2, 1, 1),
    (256, 8, 8, 64, 2, 1, 1), (256, 8, 8, 64, 0, 1, 1), (256, 8, 8, 8, 2, 1, 1),      # the limit cuts the tile into chunks: compact, full, down to 4096 pixels
    (256, 8, 4, 8, 2, 1, 1), (256, 3, 16, 64, 2, 1, 1), (256, 16, 16, 64, 1, 1, 1), (256, 8, 16, 64, 2, 2, 1),
    (512, 8, 1, 0, 2, 1, 1), (512, 8, 2, 0, 2, 1, 1), (512, 8, 2, 0, 2, 2, 1),
    (512, 8, 1, 0, 2, 1, 2), (512, 8, 1, 0, 2, 1, 4), (512, 8, 1, 8, 2, 1, 2),        # one sample per pixel in flight on stage pipes
    (512, 8, 16, 64, 2, 1, 1), (512, 8, 16, 64, 0, 1, 1), (512, 16, 16, 64, 1, 1, 1), (512, 3, 16, 64, 2, 1, 1),
    (512, 8, 16, 64, 2, 2, 1), (512, 8, 16, 64, 2, 4, 1), (512, 8, 16, 8, 2, 2, 2),   # >= 4 M paths: the chunks are dealt to the pipelines
]


def layout_of(ctx, point):
    side, bounces, slots, limit_mb, compact, pipelines, stage_pipes = point
    fr = capi.Frame(ctx, side, side)
    for opt, v in ((capi.OPT_MAX_BOUNCES, bounces), (capi.OPT_COMPACT_LOG, compact), (capi.OPT_PIPELINES, pipelines), (capi.OPT_STAGE_PIPES, stage_pipes),
                   (capi.OPT_PATH_STATE_LIMIT_MB, limit_mb), (capi.OPT_SAMPLES_IN_FLIGHT, slots)):
        fr.set_option(opt, v)
    got = five(fr)
    fr.close()
    return got


def documented_bytes_per_path(bounces, compact, pool_div=8):
    """include/rt_hip.h, RT_OPT_PATH_STATE_LIMIT_MB / RT_OPT_COMPACT_LOG: 412 / 290 bytes per path at 8 bounces, 604 / 314 at 16"""
    fixed = 11 * 16 + 5 * 4
    entries = 2 * (bounces + 1)
    if not compact:
        return fixed + 12 * entries
    return fixed + 4 + 12 * 6 + (12 * (entries - 6) + pool_div - 1) // pool_div


def test_the_documented_bytes_per_path():
    assert [documented_bytes_per_path(b, c) for b, c in ((8, False), (8, True), (16, False), (16, True))] == [412, 290, 604, 314]


@pytest.mark.parametrize("point", GRID, ids=["%dpx_b%d_s%d_l%d_c%d_p%d_sp%d" % p for p in GRID])
def test_the_layout_over_a_grid_of_options(point, ctx):
    with open(LAYOUT_JSON) as fh:
        recorded = {tuple(r["point"]): tuple(r[k] for k in FIVE) for r in json.load(fh)}
    got = layout_of(ctx, point)
    assert got == recorded[point], dict(zip(FIVE, got))
    slots, chunk_pixels, pipelines, log_inline, path_state_bytes = got
    assert log_inline in (0, 6)
    assert path_state_bytes == chunk_pixels * slots * pipelines * documented_bytes_per_path(point[1], log_inline != 0)
    assert slots == max(1, point[2]) and chunk_pixels <= point[0] * point[0]
    if point[3]:
        assert path_state_bytes <= point[3] << 20 or chunk_pixels == 4096


# ---- the banks of RT_OPT_SAMPLES_AHEAD follow the frame's options --------------------------------------------------------------------------
# every option of the class "followed by the banks" (raytracing_amd/csrc/frame_schedule.cpp) with a value that is not the default
FOLLOWED = {
    "max_bounces": (capi.OPT_MAX_BOUNCES, 2), "sampler": (capi.OPT_SAMPLER, 1), "white_furnace": (capi.OPT_WHITE_FURNACE, 1),
    "drop_last": (capi.OPT_DROP_LAST, 0), "overlap_shadow": (capi.OPT_OVERLAP_SHADOW, 0), "trace_variant": (capi.OPT_TRACE_VARIANT, 8),
    "trace_tune": (capi.OPT_TRACE_TUNE, 0x0810), "shade_partition": (capi.OPT_SHADE_PARTITION, 0), "trace_tail_lanes": (capi.OPT_TRACE_TAIL_LANES, 0),
    "chunk_refill": (capi.OPT_CHUNK_REFILL, 0), "trace_waves_per_cu": (capi.OPT_TRACE_WAVES, 4), "select_form_box": (capi.OPT_SELECT_FORM_BOX, 1),
    "small_launch_paths": (capi.OPT_SMALL_LAUNCH_PATHS, 0), "trace_tail_paths": (capi.OPT_TRACE_TAIL_PATHS, 0),
}


@pytest.mark.parametrize("followed", sorted(FOLLOWED))
def test_the_banks_follow_an_option_changed_while_they_hold_samples(followed, golden_scenes):
    option, value = FOLLOWED[followed]
    w, h, bounces = 80, 56, 3
    c = capi.Context(0)                                   # (a context of its own: one case uploads the blue-noise tables)
    try:
        c.upload_scene(golden_scenes["coverage"])
        if option == capi.OPT_SAMPLER:
            c.upload_blue_noise_tables(*S.blue_noise_tables())
        cam = T.default_camera(w, h)
        plain, fr = capi.Frame(c, w, h), capi.Frame(c, w, h)
        for f in (plain, fr):
            f.set_camera(cam); f.set_max_bounces(bounces)
        fr.set_option(capi.OPT_SAMPLES_AHEAD, 4)
        for i in range(7):
            stage_sample(plain, bounces); stage_sample(fr, bounces)
            assert np.array_equal(fr.radiance(), plain.radiance(), equal_nan=True), "frame %d" % i
        st = fr.stats()
        assert st.samples_from_banks == 4 and st.samples_ahead >= 1       # a batch is in the banks when the option changes
        banked = st.samples_from_banks
        for f in (plain, fr):
            f.set_option(option, value)
        if option == capi.OPT_MAX_BOUNCES:
            bounces = value
        for i in range(10):
            stage_sample(plain, bounces); stage_sample(fr, bounces)
            assert np.array_equal(fr.radiance(), plain.radiance(), equal_nan=True), "frame %d after the change" % i
            assert fr.sample_count() == plain.sample_count() == 8 + i
        assert fr.stats().samples_from_banks > banked
        assert np.array_equal(fr.resolve(), plain.resolve(), equal_nan=True)
        fr.close(); plain.close()
    finally:
        c.close()


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_gpu_frame_options --record > tests/golden/frame_layout.json")
    context = capi.Context(0)
    rows = [dict(point=list(p), **dict(zip(FIVE, layout_of(context, p)))) for p in GRID]
    context.close()
    print("[\n" + ",\n".join("  " + json.dumps(r) for r in rows) + "\n]")

// frame_host_units.cpp -- the host-only units behind the context and the frames (context.cpp, frame_layout.cpp, frame_schedule.cpp, frame_fold_hooks.cpp)
// as a stand-alone program, for AddressSanitizer + UBSan (tests/test_frame_host_units_sanitized.py builds it with the four units and the HIP runtime, which
// is linked and never asked for a device).  Everything of frame_launch.h that is rt_hip.hip's is a stub here that counts its call and returns RT_OK; so is
// what the link needs of the scene's and the queries' units.  The program
//   1. has the entries refuse on their arguments alone and compares each message with the text tests/test_schedule_entry_messages.py pins, and
//   2. runs the pure planning functions -- log_is_compact, bytes_per_path, chunk_plan, chunk_for, slot_cap, ahead_depth, ahead_wanted, frame_kernel_eligible --
//      on hand-made rt_frame records (a one-pixel tile, a tile without a pixel, a 1080p tile cut into chunks by RT_OPT_PATH_STATE_LIMIT_MB, max_bounces at 0
//      and at its limit, two pipelines, stage pipes, the compact log, the banks' depths) and compares every value with PARENT below.
// PARENT was obtained once by running this same body (plan_values) against the text of those functions as they stood in rt_hip.hip and
// samples_ahead_impl.h in the commit before they moved (-DFRAME_PLAN_PARENT_TEXT=<a file holding that text>, then `--print`); the functions moved word for
// word, so the values are constants.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include "rt_hip.h"
#include "context.h"
#include "frame.h"
#ifdef FRAME_PLAN_PARENT_TEXT
#include FRAME_PLAN_PARENT_TEXT
#else
#include "frame_launch.h"
#include "fold_adapt.h"
#include "wide_bvh.h"
#include "region_host.h"
using namespace frame;
using namespace launch;

// ---- stubs: rt_hip.hip's side of frame_launch.h ------------------------------------------------------------------------------------------
static int g_stub_calls = 0;
namespace launch
{
int generate_rays(rt_frame*, PathPipe&, uint32_t, uint32_t, bool, bool) { ++g_stub_calls; return RT_OK; }
bool primary_fusable(const rt_frame*) { ++g_stub_calls; return false; }
int intersect_pipe(rt_frame*, PathPipe&, uint32_t) { ++g_stub_calls; return RT_OK; }
int shade_pipe(rt_frame*, PathPipe&, uint32_t, bool) { ++g_stub_calls; return RT_OK; }
int shadow_pipe(rt_frame*, PathPipe&, uint32_t) { ++g_stub_calls; return RT_OK; }
int flush_log(rt_frame*, PathPipe&, bool) { ++g_stub_calls; return RT_OK; }
int flush_log_keep(rt_frame*, PathPipe&) { ++g_stub_calls; return RT_OK; }
int replay_bank_slot(rt_frame*, rt_frame*, uint32_t) { ++g_stub_calls; return RT_OK; }
int launch_frame_kernel(rt_frame*) { ++g_stub_calls; return RT_OK; }
DLog dlog(const rt_frame*, const PathPipe&) { ++g_stub_calls; return DLog{}; }
} // namespace launch
namespace context
{
void fill_gamma_lut(rt_ctx*) { ++g_stub_calls; }
// ... and scene_upload.cpp's
void free_scene(Scene&) { ++g_stub_calls; }
void fold_adapt_set_interval(FoldAdapt*, uint32_t) { ++g_stub_calls; }
void fold_adapt_set_wait(FoldAdapt*, bool) { ++g_stub_calls; }
void fold_adapt_worker(FoldAdapt*) { ++g_stub_calls; }
bool fold_view_left(const FoldAdapt&, const rt_camera&) { ++g_stub_calls; return false; }
void replace_report_line(std::string&, const char*, const std::string&) { ++g_stub_calls; }
} // namespace context
namespace frame
{
void free_filter_state(rt_frame*) { ++g_stub_calls; }
} // namespace frame
// the queries' units and wide_bvh.cpp
namespace query
{
void release(Scratch&) { ++g_stub_calls; }
rt_ray pick_ray(const rt_camera&, uint32_t, uint32_t, uint32_t, uint32_t) { ++g_stub_calls; return rt_ray{}; }
} // namespace query
namespace region
{
const char* rect_refused(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { ++g_stub_calls; return nullptr; }
rt_region rect_region(const rt_camera&, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, float, float) { ++g_stub_calls; return rt_region{}; }
} // namespace region
namespace rtw
{
uint64_t truncated_walks_exchange() { ++g_stub_calls; return 0; }
} // namespace rtw
extern "C" {
int rt_scene_trace(rt_ctx*, const rt_ray*, uint32_t, uint32_t, rt_hit*, uint32_t*, rt_surface*) { ++g_stub_calls; return RT_OK; }
int rt_scene_trace_all(rt_ctx*, const rt_ray*, uint32_t, uint32_t, rt_ray_hits*, rt_hit*, rt_surface*) { ++g_stub_calls; return RT_OK; }
int rt_scene_select(rt_ctx*, const rt_region*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*) { ++g_stub_calls; return RT_OK; }
int rt_compute_aovs(rt_frame*) { ++g_stub_calls; return RT_OK; }
int rt_denoise(rt_frame*) { ++g_stub_calls; return RT_OK; }
int rt_copy_history(rt_frame*) { ++g_stub_calls; return RT_OK; }
}
#endif

// ---- the planning functions on hand-made records ------------------------------------------------------------------------------------------
// a frame as rt_frame_create would leave it for this tile (no device: nothing is allocated), on a context with a scene the wide walk can use
static rt_frame* make_frame(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks)
{
    rt_frame* f = new rt_frame();
    f->ctx = ctx;
    f->tile.width = width; f->tile.height = height; f->tile.band_h = 1; f->tile.rank = rank; f->tile.nranks = nranks;
    uint32_t rows = 0;
    for (uint32_t band = rank; band < height; band += nranks) ++rows;
    f->tile.local_rows = rows;
    f->n_local = rows * width;
    f->trace_blocks = 8;
    f->chunk_pixels = tile_pixels(f);
    return f;
}

static std::vector<uint64_t> plan_values()
{
    std::vector<uint64_t> v;
    rt_ctx* ctx = new rt_ctx();
    memset(&ctx->prop, 0, sizeof(ctx->prop));
    ctx->scene.valid = true;
    ctx->scene.wide_ok = true;
    auto probe = [&](rt_frame* f)
    {
        for (uint32_t s : {1u, 8u, 64u}) v.push_back(log_is_compact(f, s));
        v.push_back(full_bytes_per_path(f->max_bounces));
        for (uint32_t s : {1u, 16u}) v.push_back(bytes_per_path(f, s));
        for (uint32_t s : {0u, 1u, 2u, 16u, 128u})
        {
            uint32_t np = 99, cp = 99;
            chunk_plan(f, s, np, cp);
            v.push_back(np); v.push_back(cp);
        }
        v.push_back(chunk_for(f, 16));
        v.push_back(slot_cap(f));
        v.push_back(ahead_depth(f));
        v.push_back(ahead_wanted(f));
        v.push_back(frame_kernel_eligible(f));
    };
    struct Tile { uint32_t w, h, rank, nranks; };
    // one pixel; no pixel (rank 1 of 2 of a one-row image); a small odd tile; 1080p; 4K
    for (const Tile& t : {Tile{1, 1, 0, 1}, Tile{4, 1, 1, 2}, Tile{63, 47, 0, 1}, Tile{1920, 1080, 0, 1}, Tile{3840, 2160, 1, 2}})
        for (uint32_t bounces : {0u, 3u, 8u, (uint32_t)RT_MAX_BOUNCES_LIMIT})
        {
            rt_frame* f = make_frame(ctx, t.w, t.h, t.rank, t.nranks);
            f->max_bounces = bounces;
            probe(f);                                                   // the defaults
            f->state_limit_mb = 256; probe(f);                          // RT_OPT_PATH_STATE_LIMIT_MB cuts the tile into chunks (and asks for the compact log)
            f->compact_log_opt = 0; probe(f);
            f->state_limit_mb = 0; f->compact_log_opt = 1; f->log_pool_div = 3; probe(f);
            f->log_full_forced = true; f->fallback_limit_mb = 144u << 10; probe(f);
            f->log_full_forced = false; f->fallback_limit_mb = 0; f->compact_log_opt = 2;
            f->pipelines = 2; probe(f);
            f->pipelines = 1; f->stage_pipes = 4; probe(f);
            f->aov = 1; probe(f);
            f->aov = 0; f->stage_pipes = 1;
            f->slots_opt = 24; f->slots_limit = 6; probe(f);
            f->slots_opt = 0; f->slots_limit = 0;
            for (uint32_t ahead : {1u, 2u, 64u, 255u | 256u}) { f->ahead_opt = ahead; probe(f); f->state_limit_mb = 4096; probe(f); f->state_limit_mb = 0; }
            f->ahead_opt = 0;
            for (uint32_t fk : {1u, 4u, 255u})
            {
                f->frame_kernel = fk;
                probe(f);
                f->fk_auto.frames = 4; probe(f);
                f->fk_auto.frames = 6; probe(f);
                f->fk_auto.skip = true; probe(f);
                f->fk_auto.skip = false; f->fk_auto.decided = true; f->fk_auto.use_kernel = true; probe(f);
                f->log_ovf_blocks = 64; probe(f);
                f->log_ovf_blocks = 0; f->fk_auto = {};
            }
            delete f;
        }
    delete ctx;
    return v;
}

#ifndef FRAME_PLAN_PARENT_TEXT
#include "frame_host_units_parent.inc"       // static const uint64_t PARENT[]: what plan_values returned on the parent's text

// ---- the refusals, as tests/test_schedule_entry_messages.py pins them ------------------------------------------------------------------------------------
static int g_failures = 0;
static void said(int rc, const char* text)
{
    const char* got = rt_last_error(nullptr);
    if (rc != RT_ERROR || strcmp(got, text) != 0) { printf("FAILED: rc %d, \"%s\" where \"%s\" was expected\n", rc, got, text); ++g_failures; }
}

static int refusals()
{
    uint8_t scratch[64] = {};
    void* B = scratch;
    rt_ctx* no_ctx = nullptr; rt_buffer* no_buf = nullptr; rt_frame* no_frame = nullptr;
    rt_buffer* buf_out = nullptr; rt_frame* frame_out = nullptr;
    rt_frame_desc desc = {8, 8, 0, 1, 8};
    uint32_t reserved = 0;
    int n = 0;
#define SAID(call, text) do { said((call), text); ++n; } while (0)
    SAID(rt_ctx_create(0, nullptr), "rt_ctx_create: out is NULL");
    SAID(rt_finish(no_ctx), "rt_finish: ctx is NULL");
    SAID(rt_ctx_device_info(no_ctx, nullptr, 0, nullptr, nullptr), "rt_ctx_device_info: ctx is NULL");
    SAID(rt_ctx_set_option(no_ctx, 0, 0), "rt_ctx_set_option: ctx is NULL");
    SAID(rt_host_register(no_ctx, B, 64), "rt_host_register: bad argument");
    SAID(rt_host_unregister(no_ctx, B), "rt_host_unregister: bad argument");
    SAID(rt_upload_blue_noise_tables(no_ctx, (const int*)B, (const int*)B, (const int*)B), "rt_upload_blue_noise_tables: NULL argument");
    SAID(rt_buffer_create(no_ctx, 16, nullptr, &buf_out), "rt_buffer_create: NULL argument");
    SAID(rt_buffer_write(no_buf, 0, B, 4), "rt_buffer_write: NULL argument");
    SAID(rt_buffer_read(no_buf, 0, B, 4), "rt_buffer_read: NULL argument");
    SAID(rt_buffer_copy(no_buf, no_buf, 0, 0, 0), "rt_buffer_copy: NULL argument");
    SAID(rt_frame_create(no_ctx, &desc, &frame_out), "rt_frame_create: NULL argument");
    SAID(rt_frame_create(no_ctx, nullptr, nullptr), "rt_frame_create: NULL argument");
    SAID(rt_set_option(no_frame, 0, 0), "rt_set_option: frame is NULL");
    SAID(rt_set_camera(no_frame, (const rt_camera*)B), "rt_set_camera: NULL argument");
    SAID(rt_reset(no_frame), "rt_reset: frame is NULL");
    SAID(rt_frame_reserve_samples(no_frame, 4, &reserved), "rt_frame_reserve_samples: frame is NULL");
    SAID(rt_frame_pick(no_frame, 0, 0, nullptr, nullptr, nullptr), "rt_frame_pick: frame is NULL");
    SAID(rt_frame_pick_all(no_frame, 0, 0, 4, nullptr, nullptr, nullptr, nullptr), "rt_frame_pick_all: frame is NULL");
    SAID(rt_frame_pick_rect(no_frame, 0, 0, 1, 1, 0.0f, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr), "rt_frame_pick_rect: frame is NULL");
    SAID(rt_generate_rays(no_frame), "rt_generate_rays: frame is NULL");
    SAID(rt_intersect(no_frame, 0), "rt_intersect: frame is NULL");
    SAID(rt_shade_miss(no_frame, 0), "rt_shade_miss: frame is NULL");
    SAID(rt_clear_outgoing_counter(no_frame, 0), "rt_clear_outgoing_counter: frame is NULL");
    SAID(rt_clear_shadow_counter(no_frame), "rt_clear_shadow_counter: frame is NULL");
    SAID(rt_shade(no_frame, 0), "rt_shade: frame is NULL");
    SAID(rt_intersect_shadow(no_frame, 0), "rt_intersect_shadow: frame is NULL");
    SAID(rt_accumulate_direct(no_frame), "rt_accumulate_direct: frame is NULL");
    SAID(rt_advance_sample(no_frame), "rt_advance_sample: frame is NULL");
    SAID(rt_integrate(no_frame, 1), "rt_integrate: frame is NULL");
#undef SAID
    // the entries that answer a NULL handle without a message
    if (rt_ctx_destroy(no_ctx) != RT_OK || rt_buffer_destroy(no_buf) != RT_OK || rt_frame_destroy(no_frame) != RT_OK || rt_ctx_stream(no_ctx) ||
        rt_buffer_device_ptr(no_buf) || rt_buffer_size(no_buf) != 0 || rt_frame_local_rows(no_frame) != 0 || rt_frame_global_row(no_frame, 5) != 0 || buf_out || frame_out)
    {
        printf("FAILED: a NULL handle was not answered as before\n");
        ++g_failures;
    }
    for (uint8_t b : scratch) if (b) { printf("FAILED: a refused call wrote through its arguments\n"); ++g_failures; break; }
    return n;
}
#endif

int main(int argc, char** argv)
{
    const std::vector<uint64_t> v = plan_values();
#ifdef FRAME_PLAN_PARENT_TEXT
    (void)argc; (void)argv;
    printf("// %zu values of plan_values() on the parent commit's text of the planning functions\nstatic const uint64_t PARENT[] = {", v.size());
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lluu", i % 24 ? ", " : ",\n    " + (i ? 0 : 1), (unsigned long long)v[i]);
    printf("};\n");
    return 0;
#else
    if (argc > 1 && strcmp(argv[1], "--print") == 0) { for (uint64_t x : v) printf("%llu\n", (unsigned long long)x); return 0; }
    const int n = refusals();
    const size_t n_parent = sizeof(PARENT) / sizeof(PARENT[0]);
    size_t differ = v.size() == n_parent ? 0 : 1;
    for (size_t i = 0; i < v.size() && i < n_parent; ++i)
        if (v[i] != PARENT[i]) { if (differ++ < 8) printf("FAILED: planning value %zu is %llu, the parent's %llu\n", i, (unsigned long long)v[i], (unsigned long long)PARENT[i]); }
    if (differ || g_failures) { printf("FAILED: %zu planning values differ (%zu here, %zu recorded), %d refusals\n", differ, v.size(), n_parent, g_failures); return 1; }
    printf("ok: %d refusals as pinned, %zu planning values equal the parent's, %d stub calls\n", n, v.size(), g_stub_calls);
    return 0;
#endif
}

// frame_launch.h -- what the units that schedule a frame's samples call on rt_hip.hip, and on each other.  Internal, used like frame.h (plain C++, no device
// code), by rt_hip.hip, context.cpp, frame_layout.cpp and frame_schedule.cpp; the feature units (frame_filters.cpp, frame_readers.cpp) do not include it and
// keep frame.h's narrower list.
//   namespace launch   rt_hip.hip's: every launch of the hot path's code object a sample needs, one function per launch site, with the grid and the
//                      arguments that launch takes.  How a trace launch picks its kernel (TraceTarget, launch_trace*, persistent_blocks, tune_thresholds),
//                      the kernel spans and the blue-noise tables' arguments stay private to that file.
//   namespace frame    the rest of it: how the per-path buffers are laid out (frame_layout.cpp) and what of the banks' and the measuring schedule's
//                      state another unit has to reach (frame_schedule.cpp).
#pragma once
#include "frame.h"

// What RT_OPT_TRACE_SELECT_FORM_BOX stores in a frame (rt_set_option): the bit the trace kernels test.  The same definition, token for token, as
// kernels_common.h's, which plain C++ cannot include; rt_hip.hip sees both, and the compiler reports a redefinition that differs.
#define RT_SIGN_SLOW 8u

namespace launch
{
// Primary rays for `n_slots` consecutive samples (sample indices sample_count .. sample_count + n_slots - 1) in one launch on pipe `p`; they then travel
// through that pipe's queues.  fused: only the prologue runs (one block); the pipe's bounce-0 launches make the rays (intersect_pipe, shade_pipe)
int generate_rays(rt_frame* f, PathPipe& p, uint32_t n_slots, uint32_t chunk_base = 0, bool later_chunk_on_this_pipe = false, bool fused = false);
// RT_OPT_FUSED_RAYGEN: may a batch of rt_integrate leave its bounce-0 queue unwritten?
bool primary_fusable(const rt_frame* f);
// The three stages, one pipe's work each.  IntersectRays: the closest-hit trace of pipe p's ray queue of `bounce`
int intersect_pipe(rt_frame* f, PathPipe& p, uint32_t bounce);
// ShadeMissedRays + ShadeSurfaceHits.  count_in_ray: whole samples (rt_integrate, the banks) -- nothing reads the radiance between their stages
int shade_pipe(rt_frame* f, PathPipe& p, uint32_t bounce, bool count_in_ray);
// IntersectShadowRays + AccumulateDirectSamples: the trace of pipe p's shadow queue of `bounce`, on the side stream where the shade step chose it
int shadow_pipe(rt_frame* f, PathPipe& p, uint32_t bounce);
// Adds the logged contributions of the batch in flight on pipe `p` to the running sum (keep_open: a compact log's overflow blocks stay with their paths)
int flush_log(rt_frame* f, PathPipe& p, bool keep_open = false);
// ... mid-sample (the stage API, the device groups' gather): what has been logged so far is applied and the sample stays open
int flush_log_keep(rt_frame* f, PathPipe& p);
// RT_OPT_SAMPLES_AHEAD: slot `slot` of bank h's log replayed into the radiance of its owner f, on the context's stream (ahead_consume's one launch)
int replay_bank_slot(rt_frame* f, rt_frame* h, uint32_t slot);
// RT_OPT_FRAME_KERNEL: the stage API's sample as one launch (k_frame), its grid and buffers made at the first one
int launch_frame_kernel(rt_frame* f);
// the radiance log of a pipe as the kernels see it
DLog dlog(const rt_frame* f, const PathPipe& p);

// ---- RT_OPT_FRAME_KERNEL: the stage API's sample as one launch (k_frame) ---------------------------------------------------------
// Can this frame's next sample go through k_frame?  One sample in flight over the whole tile in one chunk on one pipe, the full log layout,
// the wide tree in place, no per-frame feature that reads between the stages, and none of the paths k_frame has no instance for.
// (Defined here: it reads the record only, and states which frames launch_frame_kernel has an instance for.)
inline bool frame_kernel_eligible(const rt_frame* f)
{
    const rt_ctx* ctx = f->ctx;
    const uint32_t n_local = tile_pixels(f);
    // (fk_auto.frames has been advanced past the frame being started: frame k = frames - 1)
    const int fk = f->fk_auto.frames - 1;
    const bool wanted = f->frame_kernel == 255u ? (f->fk_auto.decided ? f->fk_auto.use_kernel : (!f->fk_auto.skip && (fk == 2 || fk == 3 || (fk >= 4 && (fk & 1))))) : f->frame_kernel != 0u;
    return wanted && f->n_local != 0u && !(f->denoiser || f->aov != 0) && ctx->scene.wide_ok && !ctx->scene.slow_shadow &&
           ctx->scene.d.emissive_nee == 0u && f->log_ovf_blocks == 0u && f->n_pipes == 1u && f->chunk_pixels >= n_local && f->stage_chunks <= 1u &&
           (f->trace_variant == 5u || f->trace_variant == 10u) && !f->profile && !f->timeline && f->select_form_box == 0u && f->max_bounces < 63u;
}
} // namespace launch

namespace context
{
// the gamma table of a new context, filled on its stream (k_fill_gamma_lut: the one launch rt_ctx_create makes)
void fill_gamma_lut(rt_ctx* ctx);
} // namespace context

namespace frame
{
// ---- frame_layout.cpp: the per-path buffers ------------------------------------------------------------------------------------------------
// may a batch of `slots` samples in flight use the compact log layout?
bool log_is_compact(const rt_frame* f, uint32_t slots);
// a path's bytes in the full layout, and in the layout a batch of `slots` samples in flight gets
size_t full_bytes_per_path(uint32_t max_bounces);
size_t bytes_per_path(const rt_frame* f, uint32_t slots);
// the most samples rt_integrate will trace together
uint32_t slot_cap(const rt_frame* f);
// how the tile is cut for `slots` samples in flight: number of pipes and pixels per chunk (chunk_for: the latter alone)
void chunk_plan(const rt_frame* f, uint32_t slots, uint32_t& n_pipes, uint32_t& chunk_pixels);
uint32_t chunk_for(const rt_frame* f, uint32_t slots);
// the per-path buffers, freed and made again for `slots` samples in flight
int alloc_path_buffers(rt_frame* f, uint32_t slots);
// grows them to hold `want` samples in flight (clamped to slot_cap); re-allocates for one sample of the whole tile
int ensure_slots(rt_frame* f, uint32_t want);
int ensure_whole_tile(rt_frame* f);
// the pipes' own streams wait for everything enqueued on the context's stream so far
int fork_pipes(rt_frame* f);
// the pipe's main stream waits for the shadow trace that last used its shadow queue `q`
int wait_shadow(rt_frame* f, PathPipe& p, uint32_t q);
// does the shadow trace of this bounce go to the pipe's side stream?
bool side_on(const rt_frame* f);
// rt_frame_create; borrowed_main_stream != NULL: pipe 0 launches there instead of on the context's stream (a bank of RT_OPT_SAMPLES_AHEAD)
int create_frame(rt_ctx* ctx, const rt_frame_desc* fd, rt_frame** out, hipStream_t borrowed_main_stream);

// ---- frame_schedule.cpp: the banks and the measuring schedule --------------------------------------------------------------------------------
// RT_OPT_SAMPLES_AHEAD: samples per batch (0: the mode cannot run); is the stage API's next sample one the mode may serve?; the banks freed with their frame
uint32_t ahead_depth(const rt_frame* f);
bool ahead_wanted(const rt_frame* f);
void ahead_destroy(rt_frame* f);
// RT_OPT_FRAME_KERNEL = 255 measures again: another workload, or another grid
void fk_auto_restart(rt_frame* f);
} // namespace frame

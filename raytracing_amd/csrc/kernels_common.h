// kernels_common.h -- device-side records, counters and the ray producer's helpers shared by
// the wavefront path-tracing kernels (hand-written for gfx950).  The kernels themselves:
//   raygen_kernels.h  trace_kernels.h  shade_kernels.h  aov_kernels.h  relayout_kernels.h
//
// Reference kernels replaced (src/kernels/cl/):
//   raygeneration.cl:65-139                        -> k_raygen
//   trace_bvh.cl:99-211                            -> k_trace_w4<false> (k_trace2<false>, k_trace_v1<false>)
//   trace_bvh.cl (-D SHADOW_RAYS) + accumulate_direct_samples.cl:27-53
//                                                  -> k_trace_w4<true>  (k_trace2<true>,  k_trace_v1<true>)
//   miss.cl:41-77 + hit_surface.cl:30-186 + clear_counter.cl (x2)
//                                                  -> k_shade
//   resolve_radiance.cl:31-86                      -> k_resolve
//   reset_radiance.cl / increment_counter.cl       -> hipMemsetAsync / host scalar
//
// Device data layout (HBM), chosen for coalesced 16-byte accesses:
//   ray queues   SoA: o4[i] = (origin.xyz, t_max), d4[i] = (dir.xyz, path id bits), thr[i] = (throughput.xyz,
//                log entries so far).  1/dir and the direction signs are computed by the CONSUMER when a lane starts
//                the ray (three IEEE divides per ray in the traversal kernel's refill phase): rounds 1-2 kept a third
//                16-byte record per ray for them, written by the producer -- 56 bytes of per-path state and one access
//                per ray more than this.
//                path id = slot * n_pixels + pixel, where `slot` numbers the samples in flight
//                (RT_OPT_SAMPLES_IN_FLIGHT); a shadow ray also carries the radiance-log entry
//                of its deferred direct sample in sh_aux[i]
//   radiance log per path: cnt[id] + log[k][id] (3 floats, 12 bytes) = the path's radiance
//                contributions in the order the reference adds them (miss or emission,
//                then direct light, per bounce).  k_flush replays them pixel by pixel,
//                sample by sample, so the fp32 sum is associated exactly as in the
//                reference although several samples are traced concurrently.
//   BVH          wnodes: one 64-byte record per folded piece of the reference BVH2 (a node and up to two more interior
//                nodes below it: 4 slots = the piece's frontier, 8-bit boxes on an exactly representable grid, per-octant
//                visit order): the tree k_trace_w4 walks (build_wide_bvh, rt_hip.hip);
//                nodes: one 64-byte "child-pair" record per INTERIOR node of the reference BVH2: both children's exact
//                boxes + refs in one line (k_trace2, k_trace_v1).  Topology, near/far rule and cull decisions are
//                exactly the reference's (trace_kernels.h).
//   trace tris   64 B, line aligned: (p1, last-in-leaf flag), e1 = p2-p1, e2 = p3-p1, spare
//   shade tris   128 B, line aligned: p1..p3, n1..n3, uv1..uv3, material
#pragma once
#include "device_math.h"
#include "rt_types.h"
#include "device_scene.h"     // DScene, the kernels' view of an uploaded scene (shared with the host units that hold one: context.h); DCounters

#define RT_LEAF_BIT 0x80000000u
#define RT_EMPTY_REF 0xFFFFFFFFu
// (RT_TRACE_STACK_LDS, RT_TRACE_STACK_MAX: device_scene.h, where the frame's host units size the spill areas by them)
// A shadow ray carries its path id in direction.w and the radiance-log entry of its deferred direct sample in sh_aux.

// one entry of the radiance log: RGB, 12 bytes (global_load/store_dwordx3)
struct rt_rgb { float x, y, z; };
RT_DEV void log_store(float* __restrict__ rlog, size_t index, float x, float y, float z)
{
    rt_rgb v = {x, y, z};
    *reinterpret_cast<rt_rgb*>(rlog + 3 * index) = v;
}

// Non-temporal queue accesses (round 6).  A trace launch reads every ray of its queue and writes every hit exactly once; marked non-temporal (the `nt` bit of
// global_load / global_store) those streams do not push the trees' records out of an XCD's 4 MB of L2.  Measured as build variants on the same box, two runs
// each (profiles/r06/call02.log, call03.log): the 10 M-triangle config, whose closest-hit walk misses the L2 for 45 % of its record fetches, 3785 / 3788 ->
// 3864 / 3870 Mrays/s (closest-hit trace 10.31 -> 10.02 ms per sample) and again 3766 / 3780 -> 3833 / 3859; the 2.8 M-triangle headline 6940 / 6946 ->
// 6915 / 6928 on one box, 6800 / 6812 -> 6871 / 6888 on the next.  The same hint on k_shade's streams moved nothing on either (dropped); on the leaf loop's
// triangle records it LOSES 9 % / 22 % (6308 / 2994: those records are re-read by the neighbouring rays of the wave and the next waves -- dropped).
typedef float rt_v4f __attribute__((ext_vector_type(4)));
RT_DEV float4 q_load(const float4* p) { const rt_v4f t = __builtin_nontemporal_load((const rt_v4f*)p); return make_float4(t.x, t.y, t.z, t.w); }
RT_DEV void q_store(float4* p, const float4& v) { const rt_v4f t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, (rt_v4f*)p); }

// Where the entries of a path's radiance log live.  FULL layout (inline_entries = 2 (B + 1), the worst case a path can
// log): entry k of path id at row-major index k * stride + id.  COMPACT layout (round 3; rt_integrate with many samples in
// flight): only the first inline_entries (6) rows exist for every path -- a path of the benchmark scene logs 2.7 entries on
// average, 1 % of the paths more than 6 -- and a path that is about to need a 7th gets an OVERFLOW BLOCK for its entries
// inline_entries .. 2 (B + 1) - 1 from a bump-allocated pool of ovf_blocks blocks (k_shade, one bounce ahead, one atomic per
// 512-path block): entry k >= inline_entries of a path with block `slot` at inline_entries * stride + (k - inline_entries) *
// ovf_blocks + slot.  A pool that runs dry raises DCounters::log_ovf_flag; the host then discards the batch and repeats it in
// the full layout (rt_integrate), so the sum is exact either way.  (The record itself, DLog: device_scene.h.)
// index of entry k of path id (in entries), or ~0 when the entry has no home (pool dry: the batch is being discarded)
RT_DEV size_t log_index(const DLog& L, uint32_t k, uint32_t id, uint32_t slot)
{
    if (k < L.inline_entries) return (size_t)k * L.stride + id;
    if (slot >= L.ovf_blocks) return ~(size_t)0;
    return (size_t)L.inline_entries * L.stride + (size_t)(k - L.inline_entries) * L.ovf_blocks + slot;
}
RT_DEV void log_put(const DLog& L, uint32_t k, uint32_t id, uint32_t slot, float x, float y, float z)
{
    const size_t i = log_index(L, k, id, slot);
    if (i != ~(size_t)0) log_store(L.rlog, i, x, y, z);
}

// (DTile, which pixels of the full image a frame owns: device_scene.h)
RT_DEV uint32_t tile_global_row(const DTile& t, uint32_t ly)
{
    uint32_t band = ly / t.band_h;
    return (band * t.nranks + t.rank) * t.band_h + (ly - band * t.band_h);
}

// (DCounters, the frame's counters -- one per frame, device memory -- and RT_LOG_SUBPOOLS: device_scene.h, where the scene's host unit finds them too)

// ray_inv_dir and ray_sign of TraceBvh (trace_bvh.cl:125-129), packed as (inv.xyz, sign bits)
#define RT_SIGN_SLOW 8u
RT_DEV float4 ray_inverse(f3 dir)
{
    f3 inv = F3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    uint32_t sign_bits = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
    // a non-finite component (dir component 0, denormal or NaN) can make the slab test produce
    // 0 * inf = NaN: such rays keep the select-form min/max of the reference (box_test).  So do rays with a
    // component of 1/dir beyond 2^96: k_trace_w4's one-fma slab distances must not overflow (trace_kernels.h).
    const float lim = 0x1p96f;
    if (!(__builtin_fabsf(inv.x) < lim && __builtin_fabsf(inv.y) < lim && __builtin_fabsf(inv.z) < lim))
        sign_bits |= RT_SIGN_SLOW;
    return make_float4(inv.x, inv.y, inv.z, __uint_as_float(sign_bits));
}

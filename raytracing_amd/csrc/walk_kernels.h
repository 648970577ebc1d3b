// walk_kernels.h -- what the kernels of the caller-facing queries share (DESIGN.md sections 7h - 7l): k_query_trace (query_kernels.h), k_bake (bake_kernels.h),
// k_nearest (nearest_kernels.h), k_all_hits (all_hits_kernels.h), k_within (within_kernels.h) and k_region (region_kernels.h) are built from the pieces below.  The frame's own walks (trace_kernels.h, rt_hip.hip's code
// object) are not: this header is included by query.hip, bake.hip, nearest.hip, all_hits.hip, within.hip and region.hip only.
//
//   Stack          a lane's traversal stack: push, and a pop that takes the walk's re-test
//   Ray, ray_setup a ray as its walk needs it: 1/dir, the sign bits, the octant, and which records it walks
//   volume_step    one pass of a walk that is no ray's (a point's: k_nearest, k_within): the fetch of the record, the leaf chain and the `last` rule; what a
//                  triangle and a box record do to the walk are the caller's functors (k_region keeps a copy of it: region_kernels.h says why)
//   decode_slots   a box record's references and boxes: the four quantised slots of a 4-wide record or the two children of a child-pair record
//   point_box_step one pass of a point's walk (nearest, within) at a box record: the slots keyed by nearest_box_d2, nearest first
//   region_box_step one pass of a region's walk (overlap) at a box record: every slot region.h's box test passes is visited, in no particular order
//   cross_box_step  one pass of a probe's walk (cross, cross_kernels.h) at a box record: the probe's closed box and the two half-spaces of its plane
//   probe_box_step  one pass of a probe's nearest-first walk (separation, separation_kernels.h) at a box record: point_box_step's ordering, keyed by the
//                  caller's box-to-box bound
//   point_surface, ray_surface   the rt_surface of one found record (a nearest point, a hit): the body of the four surface kernels
//   ray_step       one pass of a ray's fused loop: the fetch of one 64-byte record and its leaf, child-pair or 4-wide step; what an accepted triangle does
//                  to the walk is the step's mode (closest, any hit, all hits)
//   read_shading_triangle, store_surface, store_nearest, triangle_corners   the records' readers and writers
//
// Why the frame's walks are not borrowed: v1_trace_ray, k_trace2 and w4_trace_body fix t_min = 0, take rays in the queues' layout (o4.w = t_max, d4.w = a path
// id) and live on the frame's persistent queues, radiance log and slow lists.  A caller's rt_ray carries its own t_min (trace_bvh.cl:148 honours it), so the
// step below is these kernels' own; the tests it is made of -- box_test, box_test_fast, w4_test_slots, ray_triangle -- are trace_kernels.h's, which take a t_min.
//
// The ray walk.  A lane's ray is at a reference: a 4-wide record, a child-pair record, or a triangle of a leaf.  Every pass of the one loop fetches the lane's next
// 64-byte record -- the same four 16-byte loads whichever kind -- and takes its step (the shape of w4_trace_body's loop D: one memory round trip per step):
//   * a ray the wide walk can take walks the 4-wide records: w4_test_slots' conservative slab tests with the ray's t_min, slots in the record's order table
//     (closest) or in stored order (any-hit); the first passing slot is visited next, the later ones wait on the stack with their entry distances; a leaf is
//     re-tested with its exact BVH2 bounds and the current t_max when it is reached and its triangles are tested in array order; an accepted hit lowers t_max
//     (trace_bvh.cl:157-162).  Per ray that is w4_trace_body's sequence of nodes, leaves and t_max, which is the reference's (trace_kernels.h, "Exactness"):
//     t_min only enters the two max(..., t_min) and the accept rule, and the pop-time re-test t_max >= entry stays equivalent to the full box test.
//   * RT_SIGN_SLOW rays (a non-finite or huge 1/dir component), rays from beyond 2^29, and every ray when the scene has no 4-wide tree (RT_CTX_OPT_WIDE_BVH = 0,
//     a tree that does not qualify) walk the exact child-pair records: trace_bvh.cl's loop, both children box-tested at their parent (select-form box_test for
//     the slow rays), near child first by the split axis, the far child pushed with its entry distance.  A leaf reached this way has had its exact box tested
//     at its parent, so it arrives with RT_LEAF_CONT_BIT set and shares the leaf step.  Any-hit slow rays walk this (the reference's) tree: any tree over the
//     reference's leaves gives the reference's verdict.
//   * a ray with a non-finite component or an all-zero direction is not walked: a miss.
//
// Stack: RT_QUERY_STACK_LDS entries of (ref, key) per lane in LDS, lane-major, the rest in the lane's slice of a spill area, RT_W4_STACK_MAX entries in all -- the
// bound k_trace_w4 has with its argument (at most three pending slots per wide level, at most 33 levels: build_wide_bvh refuses deeper folds), which also covers
// the child-pair walk's RT_TRACE_STACK_MAX = 64 (one pending child per level; the reference's own nodesToVisit[64], trace_bvh.cl:142).  A push beyond it is not
// written; it raises *status, which the host forms and rt_finish report -- never a silent limit, never a store out of bounds.  A ray's key is its entry
// distance, a nearest-point walk's the box's nearest_box_d2.
//
// Grid: persistent-style, blocks = min(number of 64-lane groups, what is resident); block b takes groups b, b + blocks, ... and finishes one before it takes
// the next.  So the spill area is sized by the grid, not by n: block b's lane l owns entries (b * 64 + l) * RT_QUERY_SPILL_PER_LANE onward.
#pragma once
#include "trace_kernels.h"
#include "query.h"
#include "all_hits.h"
#include "nearest.h"
#include "region.h"

#define RT_QUERY_STACK_LDS 12
#define RT_QUERY_SPILL_PER_LANE (RT_W4_STACK_MAX - RT_QUERY_STACK_LDS)
static_assert(RT_W4_STACK_MAX >= RT_TRACE_STACK_MAX, "the one stack serves both walks");

namespace walk
{
typedef uint2 StackLds[RT_QUERY_STACK_LDS][64];          // a kernel declares one, __shared__

struct Stack
{
    StackLds& lds;
    uint2* spill;                                         // this lane's slice
    uint32_t lane;
    int sp;
    bool overflow;

    RT_DEV Stack(StackLds& lds_, uint2* spill_area) : lds(lds_), spill(spill_area + (size_t)(blockIdx.x * 64u + threadIdx.x) * RT_QUERY_SPILL_PER_LANE),
        lane(threadIdx.x), sp(0), overflow(false) {}
    RT_DEV void push(uint32_t ref, float key)
    {
        const uint2 e = make_uint2(ref, __float_as_uint(key));
        if (sp < RT_QUERY_STACK_LDS) lds[sp][lane] = e;
        else if (sp < RT_W4_STACK_MAX) spill[sp - RT_QUERY_STACK_LDS] = e;
        else { overflow = true; return; }
        ++sp;
    }
    // the topmost entry whose key passes keep(key) (the box re-test at pop time; wide entries: conservative, a pre-cull); RT_IDLE_REF when none is left
    template <class Keep>
    RT_DEV uint32_t pop(Keep keep)
    {
        while (sp > 0)
        {
            --sp;
            const uint2 e = sp < RT_QUERY_STACK_LDS ? lds[sp][lane] : spill_load64(spill + (sp - RT_QUERY_STACK_LDS));
            if (keep(__uint_as_float(e.y))) return e.x;
        }
        return RT_IDLE_REF;
    }
    // at the kernel's end.  *status is pinned host memory: the host reads it after it has waited for the stream
    RT_DEV void report(uint32_t* status) const { if (overflow) *status = 1u; }
};

// a ray that is walked: every component finite and a direction that is not all zeros
RT_DEV bool ray_walkable(const float4 o, const float4 d)
{
    const bool finite = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) && __builtin_isfinite(o.w) &&
                        __builtin_isfinite(d.x) && __builtin_isfinite(d.y) && __builtin_isfinite(d.z) && __builtin_isfinite(d.w);
    return finite && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}

struct Ray
{
    f3 org, dir, inv;
    uint32_t sign_bits, octant4;
    bool pairs;                                           // this ray walks the child-pair records
};

RT_DEV Ray ray_idle() { return Ray{F3s(0.0f), F3s(0.0f), F3s(0.0f), 0u, 0u, false}; }

RT_DEV Ray ray_setup(const f3 org, const f3 dir, uint32_t use_wide)
{
    Ray r;
    r.org = org; r.dir = dir;
    const float4 q = ray_inverse(dir);                                        // trace_bvh.cl:125-129
    r.inv = F3(q.x, q.y, q.z);
    r.sign_bits = __float_as_uint(q.w) & 0xFFu;
    r.octant4 = 4u * (r.sign_bits & 7u);
    r.pairs = use_wide == 0u || (r.sign_bits & RT_SIGN_SLOW) != 0u ||
              !(hw_max3(__builtin_fabsf(org.x), __builtin_fabsf(org.y), __builtin_fabsf(org.z)) < 0x1p29f);
    return r;
}

// where a ray's walk starts: the child-pair records' entry or the 4-wide records' (ANY_HIT: the shadow rays' tree)
template <bool ANY_HIT>
RT_DEV uint32_t ray_entry(const DScene& sc, const Ray& r) { return r.pairs ? sc.entry_ref : (ANY_HIT ? sc.w_sh_entry_ref : sc.w_entry_ref); }

// what a walk does with a triangle it accepts.  RAY_CLOSEST (= false, as k_query_trace<false> names it): t_max is lowered to it and the walk goes on.
// RAY_ANY_HIT (= true): the walk ends there.  RAY_ALL_HITS: the triangle is handed to the caller's sink, t_max stays, the walk goes on -- an any-hit walk
// (the shadow rays' tree, stored order) that does not stop; its triangle test is all_hits.h's two-sided one.
enum { RAY_CLOSEST = 0, RAY_ANY_HIT = 1, RAY_ALL_HITS = 2 };
struct NoSink { RT_DEV void operator()(uint32_t, float, float) const {} };

// One pass of the fused loop for a lane whose ray is at `ref` (not RT_IDLE_REF): the record's fetch and its step.  `ref` becomes the next reference, or
// RT_IDLE_REF when the ray has ended.  true: a triangle was accepted in this pass -- hit_u, hit_v and hit_prim are its, t_max its distance (an any-hit walk ends
// there, so a caller of ANY_HIT that only wants the verdict may hand in copies and drop them).  RAY_ALL_HITS: sink(prim, t, det) for the accepted triangle;
// hit_u, hit_v, hit_prim and t_max are left alone.
template <int MODE, class Sink = NoSink>
RT_DEV bool ray_step(const DScene& sc, const Ray& ray, const float t_min, float& t_max, uint32_t& ref, Stack& stack, float& hit_u, float& hit_v, uint32_t& hit_prim,
    Sink&& sink = Sink())
{
    constexpr bool ANY_HIT = MODE != RAY_CLOSEST;          // which tree, and the 4-wide slots in stored order
    const float INF = __builtin_inff();
    // (read from the kernel's argument here: handed in as a struct of three, the per-lane choice among them became an indexed load from scratch)
    const char* const wide_base = reinterpret_cast<const char*>(ANY_HIT ? sc.wnodes_sh : sc.wnodes);
    const char* const pair_base = reinterpret_cast<const char*>(sc.nodes);
    const char* const tri_base = reinterpret_cast<const char*>(sc.tris_rt);
    const f3 org = ray.org, dir = ray.dir, inv = ray.inv;
    const uint32_t sign_bits = ray.sign_bits;
    const bool pairs = ray.pairs;
    auto pop = [&]() { ref = stack.pop([&](float entry) { return t_max >= entry; }); };
    // a child-pair walk tests a leaf's exact box at its parent: the leaf step must not test it again
    auto tested = [](uint32_t r) { return (int)r < -1 ? r | RT_LEAF_CONT_BIT : r; };

    const bool at_leaf = (int)ref < -1;
    const uint32_t prim = ref & ~(RT_LEAF_BIT | RT_LEAF_CONT_BIT);
    const float4* rp = reinterpret_cast<const float4*>(at_leaf ? tri_base + ((size_t)prim << 6) : (pairs ? pair_base : wide_base) + ((size_t)ref << 6));
    const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3];
    bool accepted = false;
    if (at_leaf)
    {
        bool inside = true;
        if (!(ref & RT_LEAF_CONT_BIT))
        {
            // the reference's RayBounds on the leaf node (trace_bvh.cl:146-148) with the current t_max
            float entry;
            inside = box_test_fast(q1.w, q2.w, q3.x, q3.y, q3.z, q3.w, org, inv, t_min, t_max, entry);
        }
        if (!inside) pop();
        else
        {
            const bool last = q0.w != 0.0f;
            float t = 0.0f;
            if constexpr (MODE == RAY_ALL_HITS)
            {
                const float o[3] = {org.x, org.y, org.z}, d[3] = {dir.x, dir.y, dir.z};
                const float p1[3] = {q0.x, q0.y, q0.z}, e1[3] = {q1.x, q1.y, q1.z}, e2[3] = {q2.x, q2.y, q2.z};
                float u, v, det;
                accepted = ah_triangle(o, d, p1, e1, e2, t_min, t_max, &u, &v, &t, &det);
                if (accepted) sink(prim, t, det);
                if (last) pop();
                else ref = (RT_LEAF_BIT | RT_LEAF_CONT_BIT) | (prim + 1u);
            }
            else
            {
                accepted = ray_triangle(org, dir, F3(q0.x, q0.y, q0.z), F3(q1.x, q1.y, q1.z), F3(q2.x, q2.y, q2.z), t_min, t_max, hit_u, hit_v, t);
                if (accepted) { hit_prim = prim; t_max = t; }            // trace_bvh.cl:159-162
                if (ANY_HIT && accepted) ref = RT_IDLE_REF;              // goto endtrace, :164-167
                else if (last) pop();
                else ref = (RT_LEAF_BIT | RT_LEAF_CONT_BIT) | (prim + 1u);
            }
        }
    }
    else if (pairs)
    {
        // one interior node of the reference's tree: both children's exact boxes (trace_bvh.cl:146-148), near child first (:181-190)
        const uint32_t c0 = __float_as_uint(q3.x), c1 = __float_as_uint(q3.y), axis = __float_as_uint(q3.z);
        float a0, a1;
        bool h0, h1;
        if (sign_bits & RT_SIGN_SLOW)
        {
            h0 = box_test(RT_NODE_C0(q0, q1, q2), org, inv, t_min, t_max, a0);
            h1 = box_test(RT_NODE_C1(q0, q1, q2), org, inv, t_min, t_max, a1);
        }
        else
        {
            h0 = box_test_fast(RT_NODE_C0(q0, q1, q2), org, inv, t_min, t_max, a0);
            h1 = box_test_fast(RT_NODE_C1(q0, q1, q2), org, inv, t_min, t_max, a1);
        }
        h1 = h1 && c1 != RT_EMPTY_REF;
        const bool swap = ((sign_bits >> axis) & 1u) != 0u;
        const uint32_t near_ref = swap ? c1 : c0, far_ref = swap ? c0 : c1;
        const bool near_hit = swap ? h1 : h0, far_hit = swap ? h0 : h1;
        if (near_hit && far_hit) stack.push(tested(far_ref), swap ? a0 : a1);
        if (near_hit) ref = tested(near_ref);
        else if (far_hit) ref = tested(far_ref);
        else pop();
    }
    else
    {
        uint32_t r[4];
        float e[4];
        w4_test_slots<ANY_HIT>(q0, q1, q2, q3, org, inv, sign_bits, ray.octant4, t_min, t_max, r, e);
        // the first passing position is visited next, the later ones wait on the stack (deepest first)
        const bool v0 = e[0] < INF, v1 = e[1] < INF, v2 = e[2] < INF, v3 = e[3] < INF;
        if (v3 && (v0 || v1 || v2)) stack.push(r[3], e[3]);
        if (v2 && (v0 || v1)) stack.push(r[2], e[2]);
        if (v1 && v0) stack.push(r[1], e[1]);
        if (v0) ref = r[0];
        else if (v1) ref = r[1];
        else if (v2) ref = r[2];
        else if (v3) ref = r[3];
        else pop();
    }
    return accepted;
}

// One pass of a volume walk -- a point's or a region's descent, not a ray's -- for a lane whose `ref` is not RT_IDLE_REF: a 4-wide record (WIDE), a child-pair
// record (!WIDE), or a triangle of a leaf, fetched with the same four 16-byte loads whichever it is.  At a leaf: leaf(prim, p1, p2, p3) with the corners of the
// 128-byte SHADING record (its first 64 bytes; the 64-byte trace record holds the rounded edges, from which p2 and p3 cannot be had bit for bit, and is read for
// its `last` flag alone, one dword issued with the four loads), then the leaf chain: the next triangle in array order, or after the `last` one a pop that
// re-tests keep(entry) -- evaluated after leaf, so a bound the leaf has just lowered is the one that prunes.  At a box record: box(q0, q1, q2, q3), which sets
// `ref` (point_box_step, region_box_step).  (The bases are read from the kernel's argument here, as ray_step reads them.)
template <bool WIDE, class Leaf, class Box, class Keep>
RT_DEV void volume_step(const DScene& sc, uint32_t& ref, Stack& stack, Leaf&& leaf, Box&& box, Keep&& keep)
{
    const bool at_leaf = (int)ref < -1;
    const uint32_t prim = ref & ~RT_LEAF_BIT;
    float last = 0.0f;
    if (at_leaf) last = reinterpret_cast<const float*>(sc.tris_rt)[((size_t)prim << 4) + 3u];
    const float4* rp = reinterpret_cast<const float4*>(at_leaf ? reinterpret_cast<const char*>(sc.tris_sh) + ((size_t)prim << 7)
                                                               : reinterpret_cast<const char*>(WIDE ? sc.wnodes : sc.nodes) + ((size_t)ref << 6));
    const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3];
    if (at_leaf)
    {
        const float p1[3] = {q0.x, q0.y, q0.z}, p2[3] = {q1.x, q1.y, q1.z}, p3[3] = {q2.x, q2.y, q2.z};
        leaf(prim, p1, p2, p3);
        if (last != 0.0f) ref = stack.pop(keep);
        else ref = RT_LEAF_BIT | (prim + 1u);
    }
    else box(q0, q1, q2, q3);
}

// A box record's (q0 .. q3 = its 64 bytes) references and boxes: the four slots of a 4-wide record, origin + q * cell, or the two children of a child-pair
// record.  An empty slot has the reference RT_EMPTY_REF.
template <bool WIDE>
RT_DEV void decode_slots(const float4 q0, const float4 q1, const float4 q2, const float4 q3, uint32_t (&r)[WIDE ? 4 : 2], float (&lo)[WIDE ? 4 : 2][3],
    float (&hi)[WIDE ? 4 : 2][3])
{
    if constexpr (WIDE)
    {
        const uint32_t meta = __float_as_uint(q0.w);
        const float cell[3] = {__uint_as_float((meta & 0xFFu) << 23), __uint_as_float(((meta >> 8) & 0xFFu) << 23), __uint_as_float(((meta >> 16) & 0xFFu) << 23)};
        const float origin[3] = {q0.x, q0.y, q0.z};
        const uint32_t low[3] = {__float_as_uint(q1.x), __float_as_uint(q1.y), __float_as_uint(q1.z)};
        const uint32_t high[3] = {__float_as_uint(q1.w), __float_as_uint(q2.x), __float_as_uint(q2.y)};
        r[0] = __float_as_uint(q2.z); r[1] = __float_as_uint(q2.w); r[2] = __float_as_uint(q3.x); r[3] = __float_as_uint(q3.y);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a)
            {
                lo[k][a] = (float)((low[a] >> (8 * k)) & 0xFFu) * cell[a] + origin[a];       // exact (wide_frame)
                hi[k][a] = (float)((high[a] >> (8 * k)) & 0xFFu) * cell[a] + origin[a];
            }
    }
    else
    {
        lo[0][0] = q0.x; lo[0][1] = q0.y; lo[0][2] = q2.x; hi[0][0] = q0.z; hi[0][1] = q0.w; hi[0][2] = q2.y;
        lo[1][0] = q1.x; lo[1][1] = q1.y; lo[1][2] = q2.z; hi[1][0] = q1.z; hi[1][1] = q1.w; hi[1][2] = q2.w;
        r[0] = __float_as_uint(q3.x); r[1] = __float_as_uint(q3.y);
    }
}

// One pass of a point's walk at a box record: its slots (decode_slots), each keyed by nearest_box_d2; those that pass !(key > best) ascending by key, the
// nearest visited next, the others pushed farthest deepest; none: a pop that re-tests !(entry > best).
//k_nearest's (nearest_kernels.h) and k_within's (within_kernels.h) step alike: `best` is whatever bound the caller's walk prunes by.
template <bool WIDE>
RT_DEV void point_box_step(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const float (&p)[3], const float best, uint32_t& ref, Stack& stack)
{
    constexpr int N = WIDE ? 4 : 2;
    const float INF = __builtin_inff();
    uint32_t rn[N], r[4] = {RT_EMPTY_REF, RT_EMPTY_REF, RT_EMPTY_REF, RT_EMPTY_REF};
    float lo[N][3], hi[N][3], e[4] = {INF, INF, INF, INF};
    decode_slots<WIDE>(q0, q1, q2, q3, rn, lo, hi);
    // a slot that is empty or too far leaves the step: marked by RT_EMPTY_REF, keyed +inf
#pragma unroll
    for (int k = 0; k < N; ++k)
    {
        const float key = nearest_box_d2(p, lo[k], hi[k]);
        const bool pass = rn[k] != RT_EMPTY_REF && !(key > best);
        r[k] = pass ? rn[k] : RT_EMPTY_REF;
        e[k] = pass ? key : INF;
    }
    // ascending by nearest_box_d2 (five exchanges; two candidates need the first only)
    auto exchange = [&](int a, int b)
    {
        const bool s = e[b] < e[a];
        const float te = s ? e[b] : e[a]; e[b] = s ? e[a] : e[b]; e[a] = te;
        const uint32_t tr = s ? r[b] : r[a]; r[b] = s ? r[a] : r[b]; r[a] = tr;
    };
    exchange(0, 1);
    if (WIDE) { exchange(2, 3); exchange(0, 2); exchange(1, 3); exchange(1, 2); }
    // the nearest passing slot is visited next, the others wait on the stack, farthest deepest
    uint32_t next = RT_IDLE_REF;
    float next_e = 0.0f;
#pragma unroll
    for (int k = WIDE ? 3 : 1; k >= 0; --k)
        if (r[k] != RT_EMPTY_REF)
        {
            if (next != RT_IDLE_REF) stack.push(next, next_e);
            next = r[k]; next_e = e[k];
        }
    if (next != RT_IDLE_REF) ref = next;
    else ref = stack.pop([&](float entry) { return !(entry > best); });
}

// A region's planes as its walk keeps them: 16 bytes per plane and lane in LDS, lane-major (8 KiB per block).  Eight planes are 32 registers and a loop to
// num_planes would index them per lane -- scratch; a lane reads its own column only, so no barrier is needed.
typedef float4 RegionLds[RT_REGION_MAX_PLANES][64];          // a kernel declares one, __shared__

// One pass of a region's walk at a box record: its slots (decode_slots), each tested against the lane's planes (region.h's box test).  A counting walk
// visits every passing slot, so there is no key and no sort: all passing slots but one are pushed, that one is visited next; none: a pop, which always accepts.
template <bool WIDE>
RT_DEV void region_box_step(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const RegionLds& planes, const uint32_t num_planes, uint32_t& ref,
    Stack& stack)
{
    constexpr int N = WIDE ? 4 : 2;
    uint32_t r[N];
    float lo[N][3], hi[N][3];
    decode_slots<WIDE>(q0, q1, q2, q3, r, lo, hi);
    bool pass[N];
#pragma unroll
    for (int k = 0; k < N; ++k) pass[k] = r[k] != RT_EMPTY_REF;
    for (uint32_t j = 0; j < num_planes; ++j)
    {
        const float4 p4 = planes[j][threadIdx.x];
        const float pl[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
        for (int k = 0; k < N; ++k) pass[k] = pass[k] && !region_plane_rejects_box(pl, lo[k], hi[k]);
    }
    uint32_t next = RT_IDLE_REF;
#pragma unroll
    for (int k = N - 1; k >= 0; --k)
        if (pass[k])
        {
            if (next != RT_IDLE_REF) stack.push(next, 0.0f);
            next = r[k];
        }
    if (next != RT_IDLE_REF) ref = next;
    else ref = stack.pop([](float) { return true; });
}

// One pass of a probe's walk (cross) at a box record: its slots (decode_slots), each tested against the probe's closed box (plain comparisons) and, when
// `plane`, against the two half-spaces of the probe's plane pl = (n, d) and (-n, -d) (region.h's box test; cross.h has the argument).  A counting walk like
// region_box_step: all passing slots but one are pushed, that one is visited next; none: a pop, which always accepts.  The probe's 10 floats are registers.
template <bool WIDE>
RT_DEV void cross_box_step(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const float (&qlo)[3], const float (&qhi)[3], const float (&pl)[4],
    const bool plane, uint32_t& ref, Stack& stack)
{
    constexpr int N = WIDE ? 4 : 2;
    uint32_t r[N];
    float lo[N][3], hi[N][3];
    decode_slots<WIDE>(q0, q1, q2, q3, r, lo, hi);
    const float neg[4] = {-pl[0], -pl[1], -pl[2], -pl[3]};
    bool pass[N];
#pragma unroll
    for (int k = 0; k < N; ++k)
    {
        pass[k] = r[k] != RT_EMPTY_REF && qlo[0] <= hi[k][0] && lo[k][0] <= qhi[0] && qlo[1] <= hi[k][1] && lo[k][1] <= qhi[1] && qlo[2] <= hi[k][2] && lo[k][2] <= qhi[2];
        pass[k] = pass[k] && !(plane && (region_plane_rejects_box(pl, lo[k], hi[k]) || region_plane_rejects_box(neg, lo[k], hi[k])));
    }
    uint32_t next = RT_IDLE_REF;
#pragma unroll
    for (int k = N - 1; k >= 0; --k)
        if (pass[k])
        {
            if (next != RT_IDLE_REF) stack.push(next, 0.0f);
            next = r[k];
        }
    if (next != RT_IDLE_REF) ref = next;
    else ref = stack.pop([](float) { return true; });
}

// One pass of a probe's nearest-first walk (separation, separation_kernels.h) at a box record: point_box_step's ordering with the box-to-box bound
// key(lo, hi) = sep_box_d2(the probe's box, the slot's box) (separation.h) as the key -- the slots that pass !(key > best) ascending by key, the nearest
// visited next, the others pushed with their bound, farthest deepest; none: a pop that re-tests !(entry > best).  The probe's 6 box floats are registers.
template <bool WIDE, class Key>
RT_DEV void probe_box_step(const float4 q0, const float4 q1, const float4 q2, const float4 q3, Key&& key_of, const float best, uint32_t& ref, Stack& stack)
{
    constexpr int N = WIDE ? 4 : 2;
    const float INF = __builtin_inff();
    uint32_t rn[N], r[4] = {RT_EMPTY_REF, RT_EMPTY_REF, RT_EMPTY_REF, RT_EMPTY_REF};
    float lo[N][3], hi[N][3], e[4] = {INF, INF, INF, INF};
    decode_slots<WIDE>(q0, q1, q2, q3, rn, lo, hi);
#pragma unroll
    for (int k = 0; k < N; ++k)
    {
        const float key = key_of(lo[k], hi[k]);
        const bool pass = rn[k] != RT_EMPTY_REF && !(key > best);
        r[k] = pass ? rn[k] : RT_EMPTY_REF;
        e[k] = pass ? key : INF;
    }
    auto exchange = [&](int a, int b)
    {
        const bool s = e[b] < e[a];
        const float te = s ? e[b] : e[a]; e[b] = s ? e[a] : e[b]; e[a] = te;
        const uint32_t tr = s ? r[b] : r[a]; r[b] = s ? r[a] : r[b]; r[a] = tr;
    };
    exchange(0, 1);
    if (WIDE) { exchange(2, 3); exchange(0, 2); exchange(1, 3); exchange(1, 2); }
    uint32_t next = RT_IDLE_REF;
    float next_e = 0.0f;
#pragma unroll
    for (int k = WIDE ? 3 : 1; k >= 0; --k)
        if (r[k] != RT_EMPTY_REF)
        {
            if (next != RT_IDLE_REF) stack.push(next, next_e);
            next = r[k]; next_e = e[k];
        }
    if (next != RT_IDLE_REF) ref = next;
    else ref = stack.pop([&](float entry) { return !(entry > best); });
}

// a triangle's 128-byte shading record (p1 uv1.x | p2 uv1.y | p3 uv2.x | n1 uv2.y | n2 uv3.x | n3 uv3.y | mtl_index ...) as query_surface reads it
RT_DEV QsTriangle read_shading_triangle(const float4* __restrict__ tris_sh, uint32_t prim)
{
    const float4* tp = tris_sh + (size_t)prim * 8;
    const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2], q3 = tp[3], q4 = tp[4], q5 = tp[5], q6 = tp[6];
    QsTriangle t;
    t.p1[0] = q0.x; t.p1[1] = q0.y; t.p1[2] = q0.z; t.p2[0] = q1.x; t.p2[1] = q1.y; t.p2[2] = q1.z; t.p3[0] = q2.x; t.p3[1] = q2.y; t.p3[2] = q2.z;
    t.n1[0] = q3.x; t.n1[1] = q3.y; t.n1[2] = q3.z; t.n2[0] = q4.x; t.n2[1] = q4.y; t.n2[2] = q4.z; t.n3[0] = q5.x; t.n3[1] = q5.y; t.n3[2] = q5.z;
    t.uv1[0] = q0.w; t.uv1[1] = q1.w; t.uv2[0] = q2.w; t.uv2[1] = q3.w; t.uv3[0] = q4.w; t.uv3[1] = q5.w;
    t.mtl_index = __float_as_uint(q6.x);
    return t;
}

// an rt_surface as four 16-byte pieces
RT_DEV void store_surface(float4* o, const rt_surface& s)
{
    o[0] = make_float4(s.position[0], s.position[1], s.position[2], __uint_as_float(s.primitive_id));
    o[1] = make_float4(s.geometric_normal[0], s.geometric_normal[1], s.geometric_normal[2], __uint_as_float(s.mtl_index));
    o[2] = make_float4(s.shading_normal[0], s.shading_normal[1], s.shading_normal[2], __uint_as_float(s.object));
    o[3] = make_float4(s.texcoord[0], s.texcoord[1], s.t, __uint_as_float(s.flags));
}

// The rt_surface of found record k -- found[k * found_stride .. + 1], an rt_nearest -- of the point *point, by query.h's query_surface along q - p, the
// direction from the point to the surface.  The record may be the first 32 bytes of out[k] itself: it is read before out[k] is written.
RT_DEV void point_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle, const float4* __restrict__ point,
    const float4* found, uint32_t found_stride, size_t k, float4* out)
{
    const float4 f0 = found[k * found_stride], f1 = found[k * found_stride + 1];
    const uint32_t prim = __float_as_uint(f1.z);
    rt_surface s = qs_miss();
    if (prim < n_tris)                                           // RT_INVALID_ID (nothing found, no member listed here) is above every count
    {
        const QsTriangle t = read_shading_triangle(tris, prim);
        const float4 pt = *point;
        const float d[3] = {f0.x - pt.x, f0.y - pt.y, f0.z - pt.z};
        s = query_surface(t, d, f1.x, f1.y, f0.w, prim, object_of_triangle ? object_of_triangle[prim] : RT_INVALID_ID);
    }
    store_surface(out + k * 4, s);
}

// The same of hit k -- hits[k * hit_stride], an rt_hit -- of the ray at ray[0 .. 1].  RECORDS: `tris` = the scene's 128-byte shading records; otherwise
// rt_triangle[] (rt_debug_query_surface: they stand in for the records).  The hit may be the first 16 bytes of out[k] itself.
template <bool RECORDS>
RT_DEV void ray_surface(const float4* __restrict__ tris, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle, const float4* __restrict__ ray,
    const float4* hits, uint32_t hit_stride, size_t k, float4* out)
{
    const float4 hit = hits[k * hit_stride];
    const uint32_t prim = __float_as_uint(hit.z);
    rt_surface s = qs_miss();
    if (prim < n_tris)                                           // RT_INVALID_ID (a miss, no hit stored here) is above every count
    {
        const QsTriangle t = RECORDS ? read_shading_triangle(tris, prim) : qs_triangle(reinterpret_cast<const rt_triangle*>(tris)[prim]);
        const float4 rd = ray[1];
        const float d[3] = {rd.x, rd.y, rd.z};
        s = query_surface(t, d, hit.x, hit.y, hit.w, prim, object_of_triangle ? object_of_triangle[prim] : RT_INVALID_ID);
    }
    store_surface(out + k * 4, s);
}

// an rt_nearest as two 16-byte pieces, past the cache as q_store does (nothing reads it again on the device before a later launch or the host does)
RT_DEV void store_nearest(float4* o, const rt_nearest& r)
{
    q_store(o, make_float4(r.position[0], r.position[1], r.position[2], r.distance));
    q_store(o + 1, make_float4(r.bc[0], r.bc[1], __uint_as_float(r.primitive_id), __uint_as_float(r.flags)));
}

// the corners of an rt_triangle, on the device (k_nearest_brute) and the host (nearest.hip's brute force and walk)
__host__ __device__ inline void triangle_corners(const rt_triangle& t, float (&p1)[3], float (&p2)[3], float (&p3)[3])
{
    p1[0] = t.v1.position.x; p1[1] = t.v1.position.y; p1[2] = t.v1.position.z;
    p2[0] = t.v2.position.x; p2[1] = t.v2.position.y; p2[2] = t.v2.position.z;
    p3[0] = t.v3.position.x; p3[1] = t.v3.position.y; p3[2] = t.v3.position.z;
}
} // namespace walk

// refit.hip -- the scene's trees refitted ON THE DEVICE when its triangles move (rt_scene_refit / rt_scene_refit_buffer).
//
// Topology, split axes, slot placement and visit orders stay; every bound is made again from the leaves: a leaf's box = min / max over its vertices, an interior
// box = min / max of its two children, a 4-wide record's box = the union of its slots' exact boxes -- whatever fold the record belongs to, because every fold is
// over the reference's leaves and node bounds are exact unions.  So nothing here needs a host tree: the leaves are the runs of triangle records up to the
// last-in-leaf flag, the child-pair records and the 4-wide records carry their own child references.
//
//   k_refit_validate     read-only: positions finite, material indices in range (a refused refit leaves the scene untouched)
//   k_refit_triangles    k_relayout_triangles' records for the new triangles; the first triangle of a leaf makes the leaf's box and writes it into the spare
//                        floats of the leaf's trace records (where k_trace_w4 and the kernels below read it)
//   k_refit_pair_links / k_refit_wide_links    once per tree: who holds each record
//   k_refit_pairs        the exact child-pair records k_trace2 / k_trace_v1 walk, bottom-up
//   k_refit_wide         a 4-wide tree, bottom-up: exact box per record, then frame and 8-bit planes by wide_quant.h (build_wide_bvh's and k_fold_emit's function)
//
// Bottom-up by arrival counters (k_fold_dp's scheme): a thread starts at every record without interior children and climbs; at a parent it adds one to the
// parent's counter and goes on only if it is the last child to arrive -- nobody waits or spins.  What the earlier arrivals wrote is stored write-through at
// agent scope and drained before the add, and read past this CU's L1 at agent scope after it (eight XCDs, eight L2s).  Only min and max are taken, in one fixed operand
// order, so the result does not depend on who arrives when.  -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>
#include <string.h>
#include <cmath>
#include <vector>
#include "refit.h"
#include "wide_quant.h"
#include "device_memory.h"

#ifndef RT_LEAF_BIT
#define RT_LEAF_BIT 0x80000000u
#define RT_EMPTY_REF 0xFFFFFFFFu
#endif

namespace refit
{
#define RF_NONE 0xFFFFFFFFu
#define RF_HD __host__ __device__ inline
#define RF_DEV __device__ inline

struct Box { float mn[3], mx[3]; };

// min / max in ONE operand order for the kernels and the host restatement (the sign of a zero is the only thing the order could change)
RF_HD float rf_min(float a, float b) { return b < a ? b : a; }
RF_HD float rf_max(float a, float b) { return b > a ? b : a; }
RF_HD Box rf_union(const Box& a, const Box& b)
{
    Box u;
    for (int k = 0; k < 3; ++k) { u.mn[k] = rf_min(a.mn[k], b.mn[k]); u.mx[k] = rf_max(a.mx[k], b.mx[k]); }
    return u;
}
RF_HD void rf_grow(Box& b, const rt_float3& p)
{
    b.mn[0] = rf_min(b.mn[0], p.x); b.mn[1] = rf_min(b.mn[1], p.y); b.mn[2] = rf_min(b.mn[2], p.z);
    b.mx[0] = rf_max(b.mx[0], p.x); b.mx[1] = rf_max(b.mx[1], p.y); b.mx[2] = rf_max(b.mx[2], p.z);
}
// the box of the triangles first .. first + n - 1: v1, v2, v3 of each in turn
RF_HD Box rf_box_of(const rt_triangle& t)
{
    Box b = {{t.v1.position.x, t.v1.position.y, t.v1.position.z}, {t.v1.position.x, t.v1.position.y, t.v1.position.z}};
    rf_grow(b, t.v2.position); rf_grow(b, t.v3.position);
    return b;
}
RF_HD bool rf_interior(uint32_t ref) { return ref != RT_EMPTY_REF && !(ref & RT_LEAF_BIT); }
RF_HD bool rf_finite3(const rt_float3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------------------
// values another thread (another CU) has written and published with a fence: read past this CU's L1
RF_DEV float rf_read(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// ... and values handed to another thread: stored write-through at agent scope, so no release fence (an L2 write-back per step of every climb: measured, 14 ms
// of the 26 ms a 2.8 M-triangle refit took with __threadfence() on both sides) -- the stores are drained before the arrival is counted
RF_DEV void rf_write(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
RF_DEV void rf_drain()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // (no instruction: the compiler keeps the stores above)
    __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0): gfx9 counts stores there
}
// after the counter add that made this thread the last arrival: every handed-off value is read by rf_read (past L1), so no L1 invalidate either; the add's
// result decides a branch before any of those loads is issued
RF_DEV void rf_arrived() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

// the exact box of the leaf whose first triangle is `first` (written by k_refit_triangles in an earlier launch): r[1].w, r[2].w, r[3]
RF_DEV Box rf_leaf_box(const float4* __restrict__ trt, uint32_t first)
{
    const float* r = reinterpret_cast<const float*>(trt + (size_t)first * 4);
    return Box{{r[7], r[11], r[12]}, {r[13], r[14], r[15]}};
}

__global__ __launch_bounds__(256) void k_refit_validate(const rt_triangle* __restrict__ tris, uint32_t nt, uint32_t num_materials, int* __restrict__ status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nt) return;
    const rt_triangle& t = tris[i];
    if (!rf_finite3(t.v1.position) || !rf_finite3(t.v2.position) || !rf_finite3(t.v3.position)) atomicCAS(&status[0], (int)OK, (int)BAD_POSITION);
    else if (t.mtl_index >= num_materials) atomicCAS(&status[0], (int)OK, (int)BAD_MATERIAL);
}

// one thread per triangle: the 64-byte trace record (p1, e1, e2) and the 128-byte shading record of k_relayout_triangles; the last-in-leaf flag (r[0].w) stays.
// The thread of a leaf's FIRST triangle (the one after a flag) also makes the leaf's box and writes it to every record of the leaf, as k_relayout_leaf_bounds does.
__global__ __launch_bounds__(256) void k_refit_triangles(const rt_triangle* __restrict__ tris, uint32_t nt, float4* __restrict__ trt, float4* __restrict__ tsh)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nt) return;
    const rt_triangle t = tris[i];
    const rt_float3 p1 = t.v1.position, p2 = t.v2.position, p3 = t.v3.position;
    float* r = reinterpret_cast<float*>(trt + (size_t)i * 4);
    r[0] = p1.x; r[1] = p1.y; r[2] = p1.z;                                        // r[3]: the flag
    r[4] = p2.x - p1.x; r[5] = p2.y - p1.y; r[6] = p2.z - p1.z;                   // e1, trace_bvh.cl:30
    r[8] = p3.x - p1.x; r[9] = p3.y - p1.y; r[10] = p3.z - p1.z;                  // e2, trace_bvh.cl:31
    if (tsh)
    {
        float4* q = tsh + (size_t)i * 8;
        q[0] = make_float4(p1.x, p1.y, p1.z, t.v1.texcoord.x);
        q[1] = make_float4(p2.x, p2.y, p2.z, t.v1.texcoord.y);
        q[2] = make_float4(p3.x, p3.y, p3.z, t.v2.texcoord.x);
        q[3] = make_float4(t.v1.normal.x, t.v1.normal.y, t.v1.normal.z, t.v2.texcoord.y);
        q[4] = make_float4(t.v2.normal.x, t.v2.normal.y, t.v2.normal.z, t.v3.texcoord.x);
        q[5] = make_float4(t.v3.normal.x, t.v3.normal.y, t.v3.normal.z, t.v3.texcoord.y);
        q[6] = make_float4(__uint_as_float(t.mtl_index), 0.0f, 0.0f, 0.0f);
        q[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const float* flags = reinterpret_cast<const float*>(trt);
    if (i != 0u && flags[(size_t)(i - 1u) * 16 + 3] == 0.0f) return;              // not the first of its leaf
    Box b = rf_box_of(t);
    uint32_t last = i;
    while (last + 1u < nt && flags[(size_t)last * 16 + 3] == 0.0f)
    {
        ++last;
        const rt_triangle& u = tris[last];
        rf_grow(b, u.v1.position); rf_grow(b, u.v2.position); rf_grow(b, u.v3.position);
    }
    for (uint32_t k = i; k <= last; ++k)
    {
        float* w = reinterpret_cast<float*>(trt + (size_t)k * 4);
        w[7] = b.mn[0]; w[11] = b.mn[1];
        w[12] = b.mn[2]; w[13] = b.mx[0]; w[14] = b.mx[1]; w[15] = b.mx[2];
    }
}

// child-pair record (relayout_kernels.h): [0] = child 0's (min.x, min.y, max.x, max.y), [1] = child 1's, [2] = (min.z, max.z) of both, [3] = (ref 0, ref 1, axis, -)
__global__ __launch_bounds__(256) void k_refit_pair_links(const float4* __restrict__ pairs, uint32_t n, uint32_t* __restrict__ parent)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    const float4 refs = pairs[(size_t)w * 4 + 3];
    const uint32_t r[2] = {__float_as_uint(refs.x), __float_as_uint(refs.y)};
    for (uint32_t c = 0; c < 2u; ++c)
        if (rf_interior(r[c]) && r[c] < n) parent[r[c]] = w * 2u + c;
}

__global__ __launch_bounds__(256) void k_refit_pairs(float4* __restrict__ pairs, uint32_t n, const uint32_t* __restrict__ parent, uint32_t* __restrict__ arrived,
    const float4* __restrict__ trt, uint32_t nt, int* __restrict__ status)
{
    uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    float* P = reinterpret_cast<float*>(pairs);
    uint32_t r[2] = {__float_as_uint(P[(size_t)w * 16 + 12]), __float_as_uint(P[(size_t)w * 16 + 13])};
    if (r[0] == RT_EMPTY_REF && r[1] == RT_EMPTY_REF) return;                     // not a record (rt_debug_refit's stand-ins for leaves)
    if (rf_interior(r[0]) || rf_interior(r[1])) return;                           // done by the last of its children to arrive
    for (uint32_t guard = 0;; ++guard)
    {
        if (guard > 4096u) { atomicExch(&status[1], (int)NOT_A_TREE); return; }
        Box c[2];
        for (int k = 0; k < 2; ++k)
        {
            if (r[k] == RT_EMPTY_REF) { c[k] = Box{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}; continue; }      // the super-root's second child, as upload writes it
            if (r[k] & RT_LEAF_BIT)
            {
                const uint32_t first = r[k] & ~RT_LEAF_BIT;
                if (first >= nt) { atomicExch(&status[1], (int)NOT_A_TREE); return; }
                c[k] = rf_leaf_box(trt, first);
                continue;
            }
            if (r[k] >= n) { atomicExch(&status[1], (int)NOT_A_TREE); return; }
            const float* q = P + (size_t)r[k] * 16;
            const Box a = {{rf_read(q + 0), rf_read(q + 1), rf_read(q + 8)}, {rf_read(q + 2), rf_read(q + 3), rf_read(q + 9)}};
            const Box b = {{rf_read(q + 4), rf_read(q + 5), rf_read(q + 10)}, {rf_read(q + 6), rf_read(q + 7), rf_read(q + 11)}};
            c[k] = rf_union(a, b);
        }
        float* o = P + (size_t)w * 16;
        rf_write(o + 0, c[0].mn[0]); rf_write(o + 1, c[0].mn[1]); rf_write(o + 2, c[0].mx[0]); rf_write(o + 3, c[0].mx[1]);
        rf_write(o + 4, c[1].mn[0]); rf_write(o + 5, c[1].mn[1]); rf_write(o + 6, c[1].mx[0]); rf_write(o + 7, c[1].mx[1]);
        rf_write(o + 8, c[0].mn[2]); rf_write(o + 9, c[0].mx[2]); rf_write(o + 10, c[1].mn[2]); rf_write(o + 11, c[1].mx[2]);
        const uint32_t p = parent[w];
        if (p == RF_NONE) return;
        const uint32_t pw = p >> 1;
        const uint32_t pr[2] = {__float_as_uint(P[(size_t)pw * 16 + 12]), __float_as_uint(P[(size_t)pw * 16 + 13])};
        const uint32_t need = (rf_interior(pr[0]) ? 1u : 0u) + (rf_interior(pr[1]) ? 1u : 0u);
        rf_drain();                                                // this record's boxes, before the arrival that may hand them on
        if (atomicAdd(&arrived[pw], 1u) + 1u < need) return;       // not the last: the other one goes on
        rf_arrived();
        w = pw; r[0] = pr[0]; r[1] = pr[1];
    }
}

__global__ __launch_bounds__(256) void k_refit_wide_links(const WideNode* __restrict__ recs, uint32_t n, uint32_t* __restrict__ parent)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    for (uint32_t k = 0; k < 4u; ++k)
    {
        const uint32_t ref = recs[w].ref[k];
        if (rf_interior(ref) && ref < n) parent[ref] = w * 4u + k;
    }
}

// status[flag_at] = 1: a record no longer qualifies for k_trace_w4 (wide_frame's conditions); its bytes stay as they were, its exact box is still handed on
__global__ __launch_bounds__(256) void k_refit_wide(WideNode* __restrict__ recs, uint32_t n, uint32_t entry, const uint32_t* __restrict__ parent, uint32_t* __restrict__ arrived,
    float* __restrict__ boxes, const float4* __restrict__ trt, uint32_t nt, int* __restrict__ status, int flag_at)
{
    uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    uint32_t ref[4];
    uint32_t n_int = 0, n_occ = 0;
    for (int k = 0; k < 4; ++k) { ref[k] = recs[w].ref[k]; n_int += rf_interior(ref[k]) ? 1u : 0u; n_occ += ref[k] != RT_EMPTY_REF ? 1u : 0u; }
    if (n_occ == 0u || n_int != 0u) return;
    if (parent[w] == RF_NONE && w != entry) return;                // not part of the tree
    for (uint32_t guard = 0;; ++guard)
    {
        if (guard > 256u) { atomicExch(&status[1], (int)NOT_A_TREE); return; }
        Box s[4], u;
        bool have = false;
        for (int k = 0; k < 4; ++k)
        {
            if (ref[k] == RT_EMPTY_REF) continue;
            if (ref[k] & RT_LEAF_BIT)
            {
                const uint32_t first = ref[k] & ~RT_LEAF_BIT;
                if (first >= nt) { atomicExch(&status[1], (int)NOT_A_TREE); return; }
                s[k] = rf_leaf_box(trt, first);
            }
            else
            {
                if (ref[k] >= n) { atomicExch(&status[1], (int)NOT_A_TREE); return; }
                const float* q = boxes + (size_t)ref[k] * 8;
                s[k] = Box{{rf_read(q + 0), rf_read(q + 1), rf_read(q + 2)}, {rf_read(q + 4), rf_read(q + 5), rf_read(q + 6)}};
            }
            u = have ? rf_union(u, s[k]) : s[k];
            have = true;
        }
        float* o = boxes + (size_t)w * 8;
        rf_write(o + 0, u.mn[0]); rf_write(o + 1, u.mn[1]); rf_write(o + 2, u.mn[2]); rf_write(o + 4, u.mx[0]); rf_write(o + 5, u.mx[1]); rf_write(o + 6, u.mx[2]);
        float origin[3]; int exps[3];
        bool ok = wide_frame(u.mn, u.mx, origin, exps);
        uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        for (int k = 0; k < 4 && ok; ++k)
        {
            if (ref[k] == RT_EMPTY_REF) { for (int a = 0; a < 3; ++a) lo[a] |= 255u << (8 * k); continue; }      // lo 255 > hi 0: never hit
            uint32_t l[3], h[3];
            ok = wide_quantise(s[k].mn, s[k].mx, origin, exps, l, h);
            for (int a = 0; a < 3 && ok; ++a) { lo[a] |= l[a] << (8 * k); hi[a] |= h[a] << (8 * k); }
        }
        if (ok)
        {
            WideNode& r = recs[w];                                 // ref, order, pad: untouched
            r.ox = origin[0]; r.oy = origin[1]; r.oz = origin[2];
            r.meta = wide_meta(exps, r.meta >> 24);
            for (int a = 0; a < 3; ++a) { r.lo[a] = lo[a]; r.hi[a] = hi[a]; }
        }
        else atomicExch(&status[flag_at], 1);
        const uint32_t p = parent[w];
        if (p == RF_NONE) return;
        const uint32_t pw = p >> 2;
        uint32_t pref[4], need = 0;
        for (int k = 0; k < 4; ++k) { pref[k] = recs[pw].ref[k]; need += rf_interior(pref[k]) ? 1u : 0u; }
        rf_drain();                                                // this record's exact box, before the arrival that may hand it on
        if (atomicAdd(&arrived[pw], 1u) + 1u < need) return;
        rf_arrived();
        w = pw;
        for (int k = 0; k < 4; ++k) ref[k] = pref[k];
    }
}

// ---- rt_debug_refit's own: a reference-layout node array <-> the records above ----------------------------------------------------------------------
// one thread per LinearBVHNode: a leaf marks its last triangle; an interior node writes child-pair record i (k_relayout_nodes with the identity for a record
// order); node 0 also writes the super-root, record nn
__global__ __launch_bounds__(256) void k_refit_debug_records(const rt_bvh_node* __restrict__ nodes, uint32_t nn, float4* __restrict__ trt, float4* __restrict__ pairs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nn) return;
    const rt_bvh_node nd = nodes[i];
    const uint32_t n = nd.num_primitives_axis >> 16;
    auto ref_of = [&](uint32_t c) { return (nodes[c].num_primitives_axis >> 16) ? (RT_LEAF_BIT | nodes[c].offset) : c; };
    if (i == 0u) pairs[(size_t)nn * 4 + 3] = make_float4(__uint_as_float(ref_of(0u)), __uint_as_float(RT_EMPTY_REF), 0.0f, 0.0f);
    if (n != 0u) { reinterpret_cast<float*>(trt + (size_t)(nd.offset + n - 1u) * 4)[3] = 1.0f; return; }
    pairs[(size_t)i * 4 + 3] = make_float4(__uint_as_float(ref_of(i + 1u)), __uint_as_float(ref_of(nd.offset)), __uint_as_float(nd.num_primitives_axis & 0xFFFFu), 0.0f);
}

// ... and back: a leaf's box from its first trace record, an interior node's = the union of the two boxes its record holds
__global__ __launch_bounds__(256) void k_refit_debug_nodes(const rt_bvh_node* __restrict__ nodes, uint32_t nn, const float4* __restrict__ trt, const float4* __restrict__ pairs,
    rt_bvh_node* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nn) return;
    rt_bvh_node nd = nodes[i];
    Box b;
    if ((nd.num_primitives_axis >> 16) != 0u) b = rf_leaf_box(trt, nd.offset);
    else
    {
        const float* q = reinterpret_cast<const float*>(pairs + (size_t)i * 4);
        b = rf_union(Box{{q[0], q[1], q[8]}, {q[2], q[3], q[9]}}, Box{{q[4], q[5], q[10]}, {q[6], q[7], q[11]}});
    }
    nd.bounds_min.x = b.mn[0]; nd.bounds_min.y = b.mn[1]; nd.bounds_min.z = b.mn[2];
    nd.bounds_max.x = b.mx[0]; nd.bounds_max.y = b.mx[1]; nd.bounds_max.z = b.mx[2];
    out[i] = nd;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------------
// every array here gets 16 bytes of tail beyond its elements (dev::alloc); the bookkeeping for the tree report counts the elements only
enum { TAIL = 16 };

bool prepare(hipStream_t stream, State& st, const float4* pairs, uint32_t n_pairs)
{
    release(st);
    st.n_pairs = n_pairs;
    if (!dev::get(st.d_status, 4 * 4 + TAIL) || !dev::get(st.pair_parent, (size_t)n_pairs * 4 + TAIL) || !dev::get(st.pair_arrived, (size_t)n_pairs * 4 + TAIL)) { release(st); return false; }
    st.bytes = 4 * 4 + (size_t)n_pairs * 8;
    if (hipMemsetAsync(st.pair_parent, 0xFF, (size_t)n_pairs * 4, stream) != hipSuccess) { release(st); return false; }
    hipLaunchKernelGGL(k_refit_pair_links, dim3(dev::blocks_for(n_pairs, 256u)), dim3(256), 0, stream, pairs, n_pairs, st.pair_parent);
    if (!dev::clean()) { release(st); return false; }
    return true;
}

bool link_tree(hipStream_t stream, State& st, int which, WideNode* records, uint32_t n, uint32_t entry)
{
    Tree& t = st.trees[which];
    if (records && n != 0u && t.linked_for == records && t.linked_n == n) { t.entry = entry; return true; }
    dev::drop(t.parent); dev::drop(t.boxes); dev::drop(t.arrived);
    if (t.linked_n) st.bytes -= (size_t)t.linked_n * 40;
    t = Tree();
    if (!records || n == 0u) return true;
    bool ok = dev::get(t.parent, (size_t)n * 4 + TAIL) && dev::get(t.arrived, (size_t)n * 4 + TAIL) && dev::get(t.boxes, (size_t)n * 32 + TAIL) &&
              hipMemsetAsync(t.parent, 0xFF, (size_t)n * 4, stream) == hipSuccess;
    if (ok)
    {
        hipLaunchKernelGGL(k_refit_wide_links, dim3(dev::blocks_for(n, 256u)), dim3(256), 0, stream, (const WideNode*)records, n, t.parent);
        ok = dev::clean();
    }
    if (!ok) { dev::drop(t.parent); dev::drop(t.arrived); dev::drop(t.boxes); return false; }
    t.records = records; t.n = n; t.entry = entry; t.linked_for = records; t.linked_n = n;
    st.bytes += (size_t)n * 40;
    return true;
}

void release(State& st)
{
    for (Tree& t : st.trees) { dev::drop(t.parent); dev::drop(t.boxes); dev::drop(t.arrived); t = Tree(); }
    dev::drop(st.pair_parent); dev::drop(st.pair_arrived); dev::drop(st.d_status);
    st.n_pairs = 0; st.bytes = 0;
}

int validate(hipStream_t stream, State& st, const rt_triangle* d_tris, uint32_t nt, uint32_t num_materials)
{
    int status = -1;
    if (hipMemsetAsync(st.d_status, 0, 4 * sizeof(int), stream) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_refit_validate, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, d_tris, nt, num_materials, st.d_status);
    if (!dev::clean() || hipMemcpyAsync(&status, st.d_status, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return -1;
    return status;
}

bool run(hipStream_t stream, State& st, const rt_triangle* d_tris, uint32_t nt, float4* tris_rt, float4* tris_sh, float4* pairs, uint32_t super_root, Result& out)
{
    if (hipMemsetAsync(st.d_status, 0, 4 * sizeof(int), stream) != hipSuccess || hipMemsetAsync(st.pair_arrived, 0, (size_t)st.n_pairs * 4, stream) != hipSuccess) return false;
    for (Tree& t : st.trees)
        if (t.n && hipMemsetAsync(t.arrived, 0, (size_t)t.n * 4, stream) != hipSuccess) return false;
    hipLaunchKernelGGL(k_refit_triangles, dim3(dev::blocks_for(nt, 256u)), dim3(256), 0, stream, d_tris, nt, tris_rt, tris_sh);
    hipLaunchKernelGGL(k_refit_pairs, dim3(dev::blocks_for(st.n_pairs, 256u)), dim3(256), 0, stream, pairs, st.n_pairs, (const uint32_t*)st.pair_parent, st.pair_arrived, (const float4*)tris_rt, nt, st.d_status);
    for (int w = 0; w < 2; ++w)
    {
        Tree& t = st.trees[w];
        if (t.n == 0u) continue;
        hipLaunchKernelGGL(k_refit_wide, dim3(dev::blocks_for(t.n, 256u)), dim3(256), 0, stream, t.records, t.n, t.entry, (const uint32_t*)t.parent, t.arrived, t.boxes, (const float4*)tris_rt, nt, st.d_status, 2 + w);
    }
    int status[4] = {0, 0, 0, 0};
    float root[12];
    if (!dev::clean() || hipMemcpyAsync(status, st.d_status, sizeof(status), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(root, pairs + (size_t)super_root * 4, sizeof(root), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return false;
    out.error = status[1];
    out.wide_bad[0] = status[2] != 0; out.wide_bad[1] = status[3] != 0;
    out.root_min[0] = root[0]; out.root_min[1] = root[1]; out.root_min[2] = root[8];
    out.root_max[0] = root[2]; out.root_max[1] = root[3]; out.root_max[2] = root[9];
    return true;
}

// A leaf is found again as the run of triangle records up to the last-in-leaf flag: that needs the leaves to be consecutive ranges that cover the array
bool leaves_partition(const rt_bvh_node* nodes, uint32_t nn, uint32_t nt)
{
    std::vector<uint8_t> first(nt, 0), last(nt, 0);
    for (uint32_t i = 0; i < nn; ++i)
    {
        const uint32_t n = nodes[i].num_primitives_axis >> 16;
        if (n == 0u) continue;
        if ((uint64_t)nodes[i].offset + n > nt) return false;
        first[nodes[i].offset] = 1; last[nodes[i].offset + n - 1u] = 1;
    }
    for (uint32_t i = 0; i < nt; ++i)
        if ((first[i] != 0) != (i == 0u || last[i - 1u] != 0)) return false;
    return nt != 0u && last[nt - 1u] != 0;
}

// ---- rt_debug_refit ----------------------------------------------------------------------------------------------------------------------------------
// what both sides ask of their input: the node array is a tree in the reference's layout (first child at i + 1, second child at offset > i + 1, every node
// held by at most one parent, leaf ranges inside the triangle array), positions finite, the records a tree over ALL n_records whose leaf slots are leaves of
// the node array.  order: the records parents first.
static bool check_input(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t nt, const WideNode* records, uint32_t n_records, uint32_t entry,
    std::vector<uint32_t>& order, std::string& error)
{
    if (!nodes || nn == 0u || !tris || nt == 0u) { error = "no nodes or no triangles"; return false; }
    if (!leaves_partition(nodes, nn, nt)) { error = "the leaves do not partition the triangle array"; return false; }
    std::vector<uint8_t> held(nn, 0), leaf_first(nt, 0);
    for (uint32_t i = 0; i < nn; ++i)
    {
        const uint32_t n = nodes[i].num_primitives_axis >> 16;
        if (n != 0u) { leaf_first[nodes[i].offset] = 1; continue; }
        const uint32_t c1 = nodes[i].offset;
        if (i + 1u >= nn || c1 >= nn || c1 <= i + 1u) { error = "children do not follow their parent (not the reference's layout)"; return false; }
        if (held[i + 1u]++ || held[c1]++) { error = "the node array is not a tree"; return false; }
    }
    for (uint32_t i = 0; i < nt; ++i)
        if (!rf_finite3(tris[i].v1.position) || !rf_finite3(tris[i].v2.position) || !rf_finite3(tris[i].v3.position)) { error = "a triangle has a non-finite position"; return false; }
    order.clear();
    if (n_records == 0u) return true;
    if (!records || !rf_interior(entry) || entry >= n_records) { error = "bad entry reference"; return false; }
    std::vector<uint8_t> seen(n_records, 0);
    std::vector<uint32_t> todo{entry};
    seen[entry] = 1;
    while (!todo.empty())
    {
        const uint32_t w = todo.back();
        todo.pop_back();
        order.push_back(w);
        for (uint32_t ref : records[w].ref)
        {
            if (ref == RT_EMPTY_REF) continue;
            if (ref & RT_LEAF_BIT)
            {
                const uint32_t first = ref & ~RT_LEAF_BIT;
                if (first >= nt || !leaf_first[first]) { error = "a leaf slot is not a leaf of the node array"; return false; }
                continue;
            }
            if (ref >= n_records || seen[ref]) { error = "the records are not a tree"; return false; }
            seen[ref] = 1;
            todo.push_back(ref);
        }
    }
    if (order.size() != n_records) { error = "records that the entry does not reach"; return false; }
    return true;
}

bool debug_host(const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t nt, const WideNode* records, uint32_t n_records, uint32_t entry,
    rt_bvh_node* out_nodes, WideNode* out_records, bool* wide_bad, std::string& error)
{
    std::vector<uint32_t> order;
    if (!check_input(nodes, nn, tris, nt, records, n_records, entry, order, error)) return false;
    // the nodes: children have larger indices than their parent, so one pass from the last node to the first
    std::vector<Box> box(nn);
    std::vector<uint32_t> leaf_at(nt, RF_NONE);                     // first triangle -> leaf node
    for (uint32_t i = nn; i-- > 0;)
    {
        const uint32_t n = nodes[i].num_primitives_axis >> 16;
        if (n == 0u) { box[i] = rf_union(box[i + 1u], box[nodes[i].offset]); continue; }
        Box b = rf_box_of(tris[nodes[i].offset]);
        for (uint32_t k = 1; k < n; ++k) { const rt_triangle& u = tris[nodes[i].offset + k]; rf_grow(b, u.v1.position); rf_grow(b, u.v2.position); rf_grow(b, u.v3.position); }
        box[i] = b;
        leaf_at[nodes[i].offset] = i;
    }
    if (out_nodes)
        for (uint32_t i = 0; i < nn; ++i)
        {
            rt_bvh_node nd = nodes[i];
            nd.bounds_min.x = box[i].mn[0]; nd.bounds_min.y = box[i].mn[1]; nd.bounds_min.z = box[i].mn[2];
            nd.bounds_max.x = box[i].mx[0]; nd.bounds_max.y = box[i].mx[1]; nd.bounds_max.z = box[i].mx[2];
            out_nodes[i] = nd;
        }
    // the records: children first (the reverse of a parents-first order)
    bool bad = false;
    std::vector<Box> rbox(n_records);
    std::vector<WideNode> out(records, records + n_records);
    for (size_t at = order.size(); at-- > 0;)
    {
        const uint32_t w = order[at];
        WideNode& r = out[w];
        Box s[4], u;
        bool have = false;
        for (int k = 0; k < 4; ++k)
        {
            if (r.ref[k] == RT_EMPTY_REF) continue;
            s[k] = (r.ref[k] & RT_LEAF_BIT) ? box[leaf_at[r.ref[k] & ~RT_LEAF_BIT]] : rbox[r.ref[k]];
            u = have ? rf_union(u, s[k]) : s[k];
            have = true;
        }
        if (!have) { error = "a record without slots"; return false; }
        rbox[w] = u;
        float origin[3]; int exps[3];
        bool ok = wide_frame(u.mn, u.mx, origin, exps);
        uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        for (int k = 0; k < 4 && ok; ++k)
        {
            if (r.ref[k] == RT_EMPTY_REF) { for (int a = 0; a < 3; ++a) lo[a] |= 255u << (8 * k); continue; }
            uint32_t l[3], h[3];
            ok = wide_quantise(s[k].mn, s[k].mx, origin, exps, l, h);
            for (int a = 0; a < 3 && ok; ++a) { lo[a] |= l[a] << (8 * k); hi[a] |= h[a] << (8 * k); }
        }
        if (!ok) { bad = true; continue; }
        r.ox = origin[0]; r.oy = origin[1]; r.oz = origin[2];
        r.meta = wide_meta(exps, r.meta >> 24);
        for (int a = 0; a < 3; ++a) { r.lo[a] = lo[a]; r.hi[a] = hi[a]; }
    }
    if (out_records && n_records) memcpy(out_records, out.data(), (size_t)n_records * sizeof(WideNode));
    if (wide_bad) *wide_bad = bad;
    return true;
}

bool debug_device(hipStream_t stream, const rt_bvh_node* nodes, uint32_t nn, const rt_triangle* tris, uint32_t nt, const WideNode* records, uint32_t n_records, uint32_t entry,
    rt_bvh_node* out_nodes, WideNode* out_records, bool* wide_bad, std::string& error)
{
    std::vector<uint32_t> order;
    if (!check_input(nodes, nn, tris, nt, records, n_records, entry, order, error)) return false;
    State st;
    dev::Temps tmp(stream, TAIL);
    const uint32_t n_pairs = nn + 1u;                               // record i = node i (leaves: stand-ins nobody refers to), record nn = the super-root
    rt_bvh_node* const d_nodes = (rt_bvh_node*)tmp.get(nodes, (size_t)nn * sizeof(rt_bvh_node));
    rt_triangle* const d_tris = (rt_triangle*)tmp.get(tris, (size_t)nt * sizeof(rt_triangle));
    WideNode* const d_recs = n_records ? (WideNode*)tmp.get(records, (size_t)n_records * sizeof(WideNode)) : nullptr;
    rt_bvh_node* d_out = nullptr;
    float4 *trt = nullptr, *pairs = nullptr;
    bool ok = d_nodes && d_tris && (d_recs || n_records == 0u) && tmp.array(d_out, nn) && tmp.array(trt, (size_t)nt * 4) && tmp.array(pairs, (size_t)n_pairs * 4) &&
              hipMemsetAsync(trt, 0, (size_t)nt * 64, stream) == hipSuccess && hipMemsetAsync(pairs, 0xFF, (size_t)n_pairs * 64, stream) == hipSuccess;
    Result res;
    if (ok)
    {
        hipLaunchKernelGGL(k_refit_debug_records, dim3(dev::blocks_for(nn, 256u)), dim3(256), 0, stream, (const rt_bvh_node*)d_nodes, nn, trt, pairs);
        ok = dev::clean() && prepare(stream, st, pairs, n_pairs) && link_tree(stream, st, 0, d_recs, n_records, entry) &&
             run(stream, st, d_tris, nt, trt, nullptr, pairs, nn, res);
    }
    if (ok)
    {
        hipLaunchKernelGGL(k_refit_debug_nodes, dim3(dev::blocks_for(nn, 256u)), dim3(256), 0, stream, (const rt_bvh_node*)d_nodes, nn, (const float4*)trt, (const float4*)pairs, d_out);
        ok = dev::clean() && (!out_nodes || hipMemcpyAsync(out_nodes, d_out, (size_t)nn * sizeof(rt_bvh_node), hipMemcpyDeviceToHost, stream) == hipSuccess) &&
             (!out_records || n_records == 0u || hipMemcpyAsync(out_records, d_recs, (size_t)n_records * sizeof(WideNode), hipMemcpyDeviceToHost, stream) == hipSuccess);
    }
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;
    (void)hipGetLastError();
    release(st);
    if (!ok) { error = "the device path failed (allocation, copy or launch)"; return false; }
    if (res.error != OK) { error = "the kernels met a reference outside the arrays"; return false; }
    if (wide_bad) *wide_bad = res.wide_bad[0];
    return true;
}
} // namespace refit

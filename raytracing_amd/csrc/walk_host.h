// walk_host.h -- what the host forms of the caller-facing queries share (nearest.hip, within.hip, region.hip, all_hits.hip): how a brute force shares its
// items out among threads, and a tree as the host restatements of the volume walks (nearest::walk_points, region::walk_host) descend it -- the host side of
// walk_kernels.h's volume_step and decode_slots.
#pragma once
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>
#include "walk_kernels.h"          // the references and their bits
#include "wide_bvh.h"

namespace walk
{
// body(first, end) over [0, n): on this thread while `work` (the pairs a brute force tests) is below a million, shared out among up to 16 threads above
// that.  Every item is on its own, so no result depends on the split.
template <class Body>
void split_range(uint32_t n, uint64_t work, Body&& body)
{
    const uint32_t threads = work < (1u << 20) ? 1u : (n < 16u ? n : 16u);
    if (threads <= 1u) { body(0u, n); return; }
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([&body, n, t, threads]() { body((uint32_t)((uint64_t)n * t / threads), (uint32_t)((uint64_t)n * (t + 1u) / threads)); });
    for (std::thread& t : pool) t.join();
}

// The references are the device's: an interior node's index or a 4-wide record's, RT_LEAF_BIT | triangle for a triangle of a leaf.
struct HostTree
{
    const rt_bvh_node* nodes = nullptr;
    bool wide = false;
    std::vector<uint8_t> last;           // the `last` flags of the trace records: this triangle ends its leaf
    std::vector<WideNode> recs;          // wide: build_wide_bvh's records of `nodes`
    uint32_t wide_entry = 0;

    // nullptr, or why the tree is refused
    const char* prepare(const rt_bvh_node* nodes_, uint32_t nn, uint32_t n_tris, bool wide_)
    {
        nodes = nodes_; wide = wide_;
        last.assign(n_tris, 0);
        for (uint32_t i = 0; i < nn; ++i)
        {
            const uint32_t np = nodes[i].num_primitives_axis >> 16;
            if (np > 0u)
            {
                if ((uint64_t)nodes[i].offset + np > n_tris) return "a leaf's triangles lie outside the array";
                last[nodes[i].offset + np - 1u] = 1;
            }
            else if (i + 1u >= nn || nodes[i].offset <= i || nodes[i].offset >= nn) return "an interior node's children lie outside the array";
        }
        if (wide && !rtw::build_wide_bvh(nodes, nn, rtw::RT_WIDE_SAH, recs, wide_entry)) return "the tree does not qualify for the 4-wide layout";
        return nullptr;
    }
    uint32_t node_ref(uint32_t c) const { return (nodes[c].num_primitives_axis >> 16) != 0u ? RT_LEAF_BIT | nodes[c].offset : c; }
    static void box_of(const rt_bvh_node& b, float (&lo)[3], float (&hi)[3])
    {
        lo[0] = b.bounds_min.x; lo[1] = b.bounds_min.y; lo[2] = b.bounds_min.z; hi[0] = b.bounds_max.x; hi[1] = b.bounds_max.y; hi[2] = b.bounds_max.z;
    }
    // where a walk starts: the 4-wide entry, or what the super-root record gives (child 0 = (the root's box, the root), child 1 empty)
    template <class Passes>
    uint32_t entry(Passes&& passes) const
    {
        if (wide) return wide_entry;
        float lo[3], hi[3];
        box_of(nodes[0], lo, hi);
        return passes(lo, hi) ? node_ref(0) : RT_IDLE_REF;
    }
    // the box record at `ref` as decode_slots gives it: four slots' references and boxes (a child pair: two, the others RT_EMPTY_REF with no box).  nullptr, or a refusal
    const char* slots(uint32_t ref, uint32_t (&r)[4], float (&lo)[4][3], float (&hi)[4][3]) const
    {
        if (!wide)
        {
            const uint32_t c[2] = {ref + 1u, nodes[ref].offset};
            for (int k = 0; k < 2; ++k) { r[k] = node_ref(c[k]); box_of(nodes[c[k]], lo[k], hi[k]); }
            r[2] = r[3] = RT_EMPTY_REF;
            return nullptr;
        }
        if (ref >= recs.size()) return "a record reference lies outside the 4-wide tree";
        const WideNode& w = recs[ref];
        const float origin[3] = {w.ox, w.oy, w.oz};
        float cell[3];
        for (int a = 0; a < 3; ++a) { const uint32_t bits = ((w.meta >> (8 * a)) & 0xFFu) << 23; memcpy(&cell[a], &bits, 4); }
        for (int k = 0; k < 4; ++k)
        {
            r[k] = w.ref[k];
            for (int a = 0; a < 3; ++a)
            {
                lo[k][a] = (float)((w.lo[a] >> (8 * k)) & 0xFFu) * cell[a] + origin[a];
                hi[k][a] = (float)((w.hi[a] >> (8 * k)) & 0xFFu) * cell[a] + origin[a];
            }
        }
        return nullptr;
    }
};
} // namespace walk

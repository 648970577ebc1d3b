// wide_node.h -- the 64-byte record of the 4-wide quantized tree k_trace_w4 walks (layout: wide_bvh.cpp, "Record").  Plain header: host and device code share it.
#pragma once
#include <stdint.h>

#ifndef RT_LEAF_BIT
#define RT_LEAF_BIT 0x80000000u
#define RT_EMPTY_REF 0xFFFFFFFFu
#endif

struct WideNode { float ox, oy, oz; uint32_t meta; uint32_t lo[3]; uint32_t hi[3]; uint32_t ref[4]; uint32_t order; uint32_t pad; };
static_assert(sizeof(WideNode) == 64, "wide node record");

// The adaptation's crossing counts (k_count_box_passes in fold_kernels.h, rtw::count_box_passes in wide_bvh.cpp; compared count for count by rt_debug_count_box_passes):
// a walk keeps at most this many pending nodes.  A node whose box passes while more than RT_COUNT_STACK - 3 are pending is counted, its children are not walked, and
// the walk is counted as truncated once per such node -- the same rule on the host and on the device, so that a deep tree gets the same weights from either.
// The rule is the device kernel's as it always stood (64 entries, `sp > 61`: one entry more cautious than two pushes need), so what the default path computes has not
// changed; the HOST's walk used to keep 128 entries (`sp > 125`) and now cuts short where the device does -- coarser weights from host threads on trees with more than
// 61 nodes pending, a change of behaviour (weights only: no rendered bit depends on them).
#define RT_COUNT_STACK 64

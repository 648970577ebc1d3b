// moved_tile.h -- the tile of the kernels that move the scene's triangles (k_pose_triangles, k_skin_triangles, k_morph_triangles, k_morph_skin_triangles; DESIGN.md
// section 7g, "The tile"): a block's 256 triangles, 40 KB of contiguous 16-byte pieces, go through LDS, piece k loaded and stored by thread k mod 256, and a thread
// moves its own triangle at tile[threadIdx.x * 10] in between.  Device code, shared by inclusion.  The two barriers stay in the kernels: the first also covers
// what a kernel stages beside the tile.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_types.h"

namespace moved
{
static_assert(sizeof(rt_triangle) == 10 * sizeof(float4), "rt_triangle = ten 16-byte pieces");

// this block's part of nt triangles: the first (< nt: the grid is ceil(nt / 256) blocks), how many (256, fewer in the last block), their pieces, the first piece
struct Tile { uint32_t first, n, pieces; size_t base; };

__device__ inline Tile block_tile(uint32_t nt)
{
    const uint32_t first = blockIdx.x * 256u, n = nt - first < 256u ? nt - first : 256u;
    return Tile{first, n, n * 10u, (size_t)first * 10};
}

__device__ inline void load_tile(const Tile& b, const float4* __restrict__ rest, float4* tile)
{
    for (uint32_t k = threadIdx.x; k < b.pieces; k += 256u) tile[k] = rest[b.base + k];
}

__device__ inline void store_tile(const Tile& b, const float4* tile, float4* __restrict__ out)
{
    for (uint32_t k = threadIdx.x; k < b.pieces; k += 256u) out[b.base + k] = tile[k];
}
} // namespace moved

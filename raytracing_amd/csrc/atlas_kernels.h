// atlas_kernels.h -- the kernels of the UV atlas (rt_scene_atlas / rt_scene_atlas_surfaces / rt_scene_atlas_bake / rt_debug_atlas): the
// scene's triangles rasterised in UV space.  The rule is atlas.h's, in integers; no tree is walked.
//
//   k_atlas_cover<RECORDS>    one lane per triangle, 256-thread blocks of four independent waves: the owner and count planes (one uint32 per texel each)
//   k_atlas_resolve<RECORDS>  one lane per texel: the owner's barycentrics re-derived, rt_texel (16 bytes) out, the texel statistics
//   k_atlas_gutter            one lane per texel: one ping-pong pass of the gutter
//   k_atlas_surfaces          one lane per record: rt_surface (64 bytes) by query.h's query_surface from the scene's 128-byte shading records
//
// k_atlas_cover.  A mesh in an atlas is millions of triangles whose texel boxes hold a centre or two and a few that span thousands, so the work per triangle
// differs by orders of magnitude.  Every lane sets its triangle up (atlas_setup: the snapped corners and the texel box CLAMPED to the atlas, so no loop below
// is bounded by a UV).  A lane whose box is at most 2 x 2 texels tests those centres itself.  The wave then takes the ballot of its lanes with larger boxes
// and sweeps each of them together: the set-up is broadcast from its lane, the box is cut into 8 x 8 tiles, sixty-four tiles at a time get one lane each
// for the reject test (an edge function that is negative at the four corner centres of a tile is negative at every centre in it), and every tile that survives
// is swept by the whole wave, one texel per lane.  Those loops are wave-uniform: every ballot in them sees all 64 lanes.
// Owner by atomicMin, count by atomicAdd: integers, so the order the triangles arrive in changes nothing.  A triangle's covered centres are summed over the
// sweep's ballots and handed to its lane, for triangles_without_texel; the statistics cost one atomicAdd per wave and field.
// RECORDS: the UVs are the scene's own, the .w of the first six 16-byte pieces of a 128-byte shading record (walk::read_shading_triangle's layout); otherwise
// `uv` holds six floats per triangle.
#pragma once
#include "walk_kernels.h"
#include "atlas.h"

namespace atlas
{
enum { ST_COVERED = 0, ST_OVERLAPPED = 1, ST_GUTTER = 2, ST_SKIPPED = 3, ST_WITHOUT_TEXEL = 4, ST_FILTERED = 5 };   // rt_atlas_stats' fields

// *p += the lanes of the wave for which flag holds; called where the whole wave is active
RT_DEV void wave_count(uint32_t* p, bool flag, uint32_t lane)
{
    const unsigned long long m = __ballot(flag);
    if (m != 0ull && lane == 0u) atomicAdd(p, (uint32_t)__popcll(m));
}

template <bool RECORDS>
RT_DEV void load_uv(const float* __restrict__ uv, const float4* __restrict__ tris_sh, size_t i, float q[6])
{
    if (RECORDS)
    {
        const float* r = reinterpret_cast<const float*>(tris_sh + i * 8);
        for (int k = 0; k < 6; ++k) q[k] = r[4 * k + 3];
    }
    else
        for (int k = 0; k < 6; ++k) q[k] = uv[i * 6 + k];
}

RT_DEV void mark(uint32_t* __restrict__ owner, uint32_t* __restrict__ count, uint32_t width, int32_t x, int32_t y, uint32_t id)
{
    const uint32_t idx = (uint32_t)y * width + (uint32_t)x;      // inside the clamped box: below width * height <= 2^26
    atomicMin(owner + idx, id);
    atomicAdd(count + idx, 1u);
}

// tile (tx, ty) of 8 x 8 texels holds no covered centre: some edge function is negative at its four corner centres, so -- affine -- at all of them
RT_DEV bool tile_rejected(const AtlasTri& t, int32_t tx, int32_t ty)
{
    int64_t a[3], b[3], c[3], d[3];
    atlas_weights(t, tx * 8, ty * 8, a); atlas_weights(t, tx * 8 + 7, ty * 8, b); atlas_weights(t, tx * 8, ty * 8 + 7, c); atlas_weights(t, tx * 8 + 7, ty * 8 + 7, d);
    for (int k = 0; k < 3; ++k) if (a[k] < 0 && b[k] < 0 && c[k] < 0 && d[k] < 0) return true;
    return false;
}

template <bool RECORDS>
__global__ __launch_bounds__(256) void k_atlas_cover(const float* __restrict__ uv, const float4* __restrict__ tris_sh, uint32_t n_tris,
    const uint32_t* __restrict__ object_of_triangle, uint32_t object, uint32_t width, uint32_t height, uint32_t* __restrict__ owner, uint32_t* __restrict__ count,
    uint32_t* __restrict__ stats)
{
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    AtlasTri t = {};
    bool live = false, filtered = false, skipped = false;
    if (i < n_tris)
    {
        filtered = object != RT_INVALID_ID && object_of_triangle[i] != object;
        if (!filtered)
        {
            float q[6];
            load_uv<RECORDS>(uv, tris_sh, (size_t)i, q);
            live = atlas_setup(q, width, height, &t);
            skipped = !live;
        }
    }
    const bool boxed = live && t.x0 <= t.x1 && t.y0 <= t.y1;
    const bool small = boxed && t.x1 - t.x0 <= 1 && t.y1 - t.y0 <= 1;
    uint32_t mine = 0u;              // the centres my triangle covers

    if (small)
        for (int32_t y = t.y0; y <= t.y1; ++y)
            for (int32_t x = t.x0; x <= t.x1; ++x)
                if (atlas_covers(t, x, y)) { mark(owner, count, width, x, y, (uint32_t)i); ++mine; }

    // the larger boxes, one after the other, by the whole wave (the loops below are wave-uniform)
    for (unsigned long long todo = __ballot(boxed && !small); todo != 0ull; todo &= todo - 1ull)
    {
        const int src = __ffsll((long long)todo) - 1;
        AtlasTri b;
        for (int k = 0; k < 3; ++k) { b.x[k] = __shfl(t.x[k], src); b.y[k] = __shfl(t.y[k], src); }
        b.s = __shfl(t.s, src);
        b.x0 = __shfl(t.x0, src); b.y0 = __shfl(t.y0, src); b.x1 = __shfl(t.x1, src); b.y1 = __shfl(t.y1, src);
        b.area = 0;                  // (not read by the cover test)
        const uint32_t id = (uint32_t)(i - lane) + (uint32_t)src;
        const int32_t tx0 = b.x0 >> 3, ty0 = b.y0 >> 3;
        const uint32_t nx = (uint32_t)((b.x1 >> 3) - tx0 + 1), ny = (uint32_t)((b.y1 >> 3) - ty0 + 1);
        const uint32_t n_tiles = nx * ny;                         // at most 2048 each, and the clamped box holds at most 2^26 texels: no overflow
        uint32_t covered = 0u;
        for (uint32_t base = 0u; base < n_tiles; base += 64u)
        {
            const uint32_t tile = base + lane;
            bool keep = false;
            if (tile < n_tiles) keep = !tile_rejected(b, tx0 + (int32_t)(tile % nx), ty0 + (int32_t)(tile / nx));
            for (unsigned long long tiles = __ballot(keep); tiles != 0ull; tiles &= tiles - 1ull)
            {
                const uint32_t k = base + (uint32_t)(__ffsll((long long)tiles) - 1);
                const int32_t x = (tx0 + (int32_t)(k % nx)) * 8 + (int32_t)(lane & 7u), y = (ty0 + (int32_t)(k / nx)) * 8 + (int32_t)(lane >> 3);
                const bool c = x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1 && atlas_covers(b, x, y);
                if (c) mark(owner, count, width, x, y, id);
                covered += (uint32_t)__popcll(__ballot(c));
            }
        }
        if ((int)lane == src) mine = covered;
    }

    wave_count(stats + ST_SKIPPED, skipped, lane);
    wave_count(stats + ST_FILTERED, filtered, lane);
    wave_count(stats + ST_WITHOUT_TEXEL, live && mine == 0u, lane);
}

// texel idx from the planes: the owner's set-up again (it passed once: it passes), its barycentrics at the centre
template <bool RECORDS>
__global__ __launch_bounds__(256) void k_atlas_resolve(const float* __restrict__ uv, const float4* __restrict__ tris_sh, uint32_t width, uint32_t height,
    const uint32_t* __restrict__ owner, const uint32_t* __restrict__ count, float4* __restrict__ texels, uint32_t* __restrict__ stats)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = width * height, idx = blockIdx.x * 256u + threadIdx.x;      // n <= 2^26
    uint32_t c = 0u;
    if (idx < n)
    {
        c = count[idx];
        rt_texel r = atlas_uncovered();
        if (c != 0u)
        {
            const uint32_t prim = owner[idx];
            float q[6];
            AtlasTri t;
            load_uv<RECORDS>(uv, tris_sh, prim, q);
            (void)atlas_setup(q, width, height, &t);
            atlas_bc(t, (int32_t)(idx % width), (int32_t)(idx / width), r.bc);
            r.primitive_id = prim; r.count = (uint16_t)(c < 65535u ? c : 65535u); r.flags = (uint16_t)RT_TEXEL_COVERED;
        }
        texels[idx] = make_float4(r.bc[0], r.bc[1], __uint_as_float(r.primitive_id), __uint_as_float((uint32_t)r.count | ((uint32_t)r.flags << 16)));
    }
    wave_count(stats + ST_COVERED, c != 0u, lane);
    wave_count(stats + ST_OVERLAPPED, c > 1u, lane);
}

// one pass: in -> out, never in place.  A record's last dword is count | flags << 16: 0 exactly when the texel has no record yet.
__global__ __launch_bounds__(256) void k_atlas_gutter(uint32_t width, uint32_t height, const float4* __restrict__ in, float4* __restrict__ out, uint32_t* __restrict__ stats)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = width * height, idx = blockIdx.x * 256u + threadIdx.x;
    bool filled = false;
    if (idx < n)
    {
        float4 r = in[idx];
        if (__float_as_uint(r.w) == 0u)
        {
            const int32_t x = (int32_t)(idx % width), y = (int32_t)(idx / width);
            const int nb[8][2] = RT_ATLAS_NEIGHBOURS;
            for (int k = 0; k < 8 && !filled; ++k)
            {
                const int32_t nx = x + nb[k][0], ny = y + nb[k][1];
                if (nx < 0 || ny < 0 || nx >= (int32_t)width || ny >= (int32_t)height) continue;
                const float4 q = in[(uint32_t)ny * width + (uint32_t)nx];
                if (__float_as_uint(q.w) != 0u) { r = make_float4(q.x, q.y, q.z, __uint_as_float(RT_TEXEL_GUTTER << 16)); filled = true; }
            }
        }
        out[idx] = r;
    }
    wave_count(stats + ST_GUTTER, filled, lane);
}

// surfaces[i] of texels[i]: query_surface with an all-zero direction and t = 0; a primitive_id not below n_tris (RT_INVALID_ID: uncovered) gives a miss record
__global__ __launch_bounds__(256) void k_atlas_surfaces(const float4* __restrict__ tris_sh, uint32_t n_tris, const uint32_t* __restrict__ object_of_triangle,
    const float4* __restrict__ texels, uint32_t n, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 tx = texels[i];
    const uint32_t prim = __float_as_uint(tx.z);
    rt_surface s = qs_miss();
    if (prim < n_tris)
    {
        const float d[3] = {0.0f, 0.0f, 0.0f};
        s = query_surface(walk::read_shading_triangle(tris_sh, prim), d, tx.x, tx.y, 0.0f, prim, object_of_triangle ? object_of_triangle[prim] : RT_INVALID_ID);
    }
    walk::store_surface(out + (size_t)i * 4, s);
}
} // namespace atlas

// primary_rays.h -- the primary ray of a pixel and of a queue entry (raygeneration.cl:92-133), as device functions: k_raygen writes them to the bounce-0
// queue (raygen_kernels.h), k_frame and the PRIMARY instances of k_trace_w4 and k_shade (RT_OPT_FUSED_RAYGEN) make them in registers.  One definition,
// every unit built with -ffp-contract=off: the same bits wherever it is inlined.
#pragma once
#include "kernels_common.h"

// The primary ray of global pixel (pixel_x, pixel_y) for sample `sample_idx` (raygeneration.cl:92-133): origin on the lens, direction through the
// focus plane.  Shared by k_raygen, k_frame (frame_kernels.h) and the primary instances below.
RT_DEV void raygen_ray(const DTile& tile, const rt_camera& cam, float tan_half_fov, uint32_t pixel_x, uint32_t pixel_y, uint32_t sample_idx,
    f3& new_pos, f3& d)
{
    uint32_t pixel_idx = pixel_y * tile.width + pixel_x;                 // GLOBAL pixel index
    float inv_width = 1.0f / (float)tile.width;
    float inv_height = 1.0f / (float)tile.height;
    uint32_t seed = pixel_idx + (1103515245u * sample_idx + 12345u);     // :61,98

    float x = ((float)pixel_x + GetRandomFloat(seed)) * inv_width;
    float y = ((float)pixel_y + GetRandomFloat(seed)) * inv_height;

    float angle = tan_half_fov;                                          // rt_tanf(0.5f * fov), host-evaluated
    x = (x * 2.0f - 1.0f) * angle * cam.aspect_ratio;
    y = (y * 2.0f - 1.0f) * angle;

    f3 front = F3(cam.front.x, cam.front.y, cam.front.z);
    f3 up = F3(cam.up.x, cam.up.y, cam.up.z);
    f3 pos = F3(cam.position.x, cam.position.y, cam.position.z);
    f3 right = cross3(front, up);
    f3 dir = normalize3(right * x + up * y + front);

    f3 point_aimed = pos + dir * cam.focus_distance;
    // PointInHexagon :40-49 (index 3 = the reference's out-of-bounds read, defined as (0,0))
    int hidx = (int)__builtin_floorf(GetRandomFloat(seed) * 3.0f);
    int h1 = hidx > 3 ? 3 : hidx;
    int h2 = (hidx + 1) % 3;
    float hx1 = h1 == 0 ? -1.0f : (h1 == 3 ? 0.0f : 0.5f);
    float hy1 = h1 == 1 ? 0.866f : (h1 == 2 ? -0.866f : 0.0f);
    float hx2 = h2 == 0 ? -1.0f : 0.5f;
    float hy2 = h2 == 1 ? 0.866f : (h2 == 2 ? -0.866f : 0.0f);
    float p1 = GetRandomFloat(seed);
    float p2 = GetRandomFloat(seed);
    float dofx = p1 * hx1 + p2 * hx2;
    float dofy = p1 * hy1 + p2 * hy2;
    float r = cam.aperture;
    new_pos = pos + right * (dofx * r) + up * (dofy * r);
    d = normalize3(point_aimed - new_pos);

}

// Queue entry `i` of a k_raygen launch: which sample slot and which pixel it is, and its path id.  The queue order is PIXEL-major (see k_raygen),
// the path id slot-major and chunk-relative (slot * chunk_stride + pixel in chunk).  Shared by k_raygen and by the kernels that make their primary
// rays themselves (RT_OPT_FUSED_RAYGEN: primary_ray below).
RT_DEV void primary_index(const DTile& tile, uint32_t i, uint32_t n_slots, uint32_t chunk_base, uint32_t chunk_stride, uint32_t& slot, uint32_t& id,
    uint32_t& pixel_x, uint32_t& pixel_y)
{
    uint32_t cp = i / n_slots;                                           // pixel of this chunk
    slot = i - cp * n_slots;
    uint32_t lp = chunk_base + cp;                                       // local pixel of this tile
    uint32_t ly = lp / tile.width;
    pixel_x = lp - ly * tile.width;
    pixel_y = tile_global_row(tile, ly);
    id = slot * chunk_stride + cp;
}

// RT_OPT_FUSED_RAYGEN: what the bounce-0 closest-hit launch of an rt_integrate batch needs to make queue entry i's primary ray in registers instead of
// reading what k_raygen wrote (k_raygen's own arguments).  d4: the bounce-0 queue's directions and path ids, which the launch writes for bounce 0's k_shade;
// o4: its origins, written ONLY for the (normally no) rays the wide walk hands to k_trace2's list, which reads its rays by index.
struct PrimaryGen
{
    DTile tile; rt_camera cam; float tan_half_fov;
    uint32_t sample_base, n_slots, chunk_base, chunk_stride;
    float4* o4; float4* d4;
};
RT_DEV void primary_ray(const PrimaryGen& g, uint32_t i, float4& o4, float4& d4)
{
    uint32_t slot, id, pixel_x, pixel_y;
    primary_index(g.tile, i, g.n_slots, g.chunk_base, g.chunk_stride, slot, id, pixel_x, pixel_y);
    f3 new_pos, d;
    raygen_ray(g.tile, g.cam, g.tan_half_fov, pixel_x, pixel_y, g.sample_base + slot, new_pos, d);
    o4 = make_float4(new_pos.x, new_pos.y, new_pos.z, RT_MAX_RENDER_DIST);
    d4 = make_float4(d.x, d.y, d.z, __uint_as_float(id));               // path id
}

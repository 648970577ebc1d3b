// morph.h -- the arithmetic of rt_scene_morph and rt_scene_morph_skin: sparse morph targets (blend shapes) applied to a triangle of the
// rest pose.  k_morph_triangles, k_morph_skin_triangles and the host restatement (rt_debug_morph with ctx == NULL) all call the functions below, in binary32
// with -ffp-contract=off, so they agree bit for bit.
//
// A triangle's ROW is its records in ascending key order, key = target << 2 | corner (corner 0, 1, 2 = v1, v2, v3): so every corner meets its records in
// ascending target order.  weights[target] is the caller's weight, used as given; nothing normalises the weights.
//   a record whose weight is +0 or -0      skipped entirely
//   otherwise                              p.x = p.x + w * dp.x, likewise y and z: sequential, in this operand order
//   ... and if a word of dn is not zero    n.x = n.x + w * dn.x, likewise y and z (a dn of three +0.0 words never touches the normal; a -0.0 is another word)
//   a corner whose normal was touched      renormalised once, after its last record, by pose::pose_normal's rule: l = (x^2 + y^2) + z^2, every lane divided by
//                                          sqrtf(l) if l > 0 and finite, else left as summed
//   a corner with no applied record        copied byte for byte
//   the .w lanes, texture coordinates, mtl_index and padding: copied
// What follows from that:
//   * all-zero weights give the rest pose back byte for byte, a -0.0 in it included
//   * a position-only target never touches a normal's bytes
//   * a non-finite result is refused by the refit's own read-only validation with the scene untouched, as for a pose or a skin
// The fused call morphs first and skins the result (skin.h), as glTF, FBX and Alembic do.
#pragma once
#include "pose.h"
#include "skin.h"

namespace morph
{
// one delta of one target at one corner, as the library keeps it on the device: 32 bytes, two 16-byte pieces
struct alignas(16) Record
{
    uint32_t key;       // target << 2 | corner
    float dp[3];
    float dn[3];
    uint32_t pad;
};
static_assert(sizeof(Record) == 32, "morph::Record");

// one record at its corner; 1: the normal was touched
POSE_HD uint32_t apply(rt_vertex& v, float w, const Record& r)
{
    if (w == 0.0f) return 0u;                                          // +0 and -0
    v.position.x = v.position.x + w * r.dp[0];
    v.position.y = v.position.y + w * r.dp[1];
    v.position.z = v.position.z + w * r.dp[2];
    if ((skin::word_of(r.dn[0]) | skin::word_of(r.dn[1]) | skin::word_of(r.dn[2])) == 0u) return 0u;
    v.normal.x = v.normal.x + w * r.dn[0];
    v.normal.y = v.normal.y + w * r.dn[1];
    v.normal.z = v.normal.z + w * r.dn[2];
    return 1u;
}

// pose::pose_normal's last step on a summed normal
POSE_HD void renormalise(rt_float3& n)
{
    const float l = (n.x * n.x + n.y * n.y) + n.z * n.z;
    if (l > 0.0f && l <= 3.402823466e+38f)          // finite (a NaN fails l > 0)
    {
        const float d = sqrtf(l);
        n.x = n.x / d; n.y = n.y / d; n.z = n.z / d;
    }
}

// in place: a triangle's row of `count` records, wherever they and the weights live.  A record that names no corner or no target is skipped (rt_scene_set_morph
// has checked every one).
POSE_HD void morph_triangle(const Record* records, uint32_t count, const float* weights, uint32_t n_targets, rt_triangle& t)
{
    rt_vertex* const corners = &t.v1;               // v1, v2, v3 lie one after the other (rt_types.h)
    uint32_t touched = 0u;
    for (uint32_t k = 0; k < count; ++k)
    {
        const Record r = records[k];
        const uint32_t c = r.key & 3u, target = r.key >> 2;
        if (c > 2u || target >= n_targets) continue;
        touched |= apply(corners[c], weights[target], r) << c;
    }
    if (touched & 1u) renormalise(t.v1.normal);
    if (touched & 2u) renormalise(t.v2.normal);
    if (touched & 4u) renormalise(t.v3.normal);
}
} // namespace morph

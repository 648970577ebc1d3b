"""numpy dtypes mirroring include/rt_types.h (reference:
src/kernels/common/shared_structures.h:56-181).  Host-side plumbing only."""
import numpy as np

float3 = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<f4")])
float4 = float3
float2 = np.dtype([("x", "<f4"), ("y", "<f4")])

ray = np.dtype([("origin", float4), ("direction", float4)])
hit = np.dtype([("bc", float2), ("primitive_id", "<u4"), ("t", "<f4")])
scene_info = np.dtype([("analytic_light_count", "<u4"), ("emissive_count", "<u4"),
                       ("environment_map_index", "<u4"), ("padding", "<u4")])
packed_material = np.dtype([("diffuse_albedo", "<u4"), ("specular_albedo", "<u4"), ("emission", "<u4"),
                            ("roughness_metalness", "<u4"), ("ior_emission_idx_transparency", "<u4")])
light = np.dtype([("origin", float3), ("radiance", float3), ("type", "<u4"), ("padding", "<u4", (3,))])
texture = np.dtype([("data_start", "<i4"), ("width", "<i4"), ("height", "<i4"), ("padding", "<i4")])
vertex = np.dtype([("position", float3), ("texcoord", float3), ("normal", float3)])
triangle = np.dtype([("v1", vertex), ("v2", vertex), ("v3", vertex), ("mtl_index", "<u4"),
                     ("padding", "<u4", (3,))])
bvh_node = np.dtype([("bounds_min", float3), ("bounds_max", float3), ("offset", "<u4"),
                     ("num_primitives_axis", "<u4"), ("padding", "<u4", (2,))])
# rt_surface (include/rt_hip.h): what a ray query reports of a hit; a miss is primitive_id = 0xFFFFFFFF and zeros
surface = np.dtype([("position", "<f4", (3,)), ("primitive_id", "<u4"), ("geometric_normal", "<f4", (3,)), ("mtl_index", "<u4"),
                    ("shading_normal", "<f4", (3,)), ("object", "<u4"), ("texcoord", "<f4", (2,)), ("t", "<f4"), ("flags", "<u4")])
# rt_bake_result (include/rt_hip.h): what an occlusion bake reports of a point; a skipped point is unoccluded = 0xFFFFFFFF and zeros
bake_result = np.dtype([("bent_normal", "<f4", (3,)), ("unoccluded", "<u4")])
# rt_light_bake_result (include/rt_hip.h): what a light bake reports of a point -- the irradiance from the sky and from the scene's analytic lights, and how many
# sky rays and lights reached it; a skipped point is zeros and both counts 0xFFFFFFFF
light_bake_result = np.dtype([("sky", "<f4", (3,)), ("sky_unoccluded", "<u4"), ("lights", "<f4", (3,)), ("lights_unshadowed", "<u4")])
# rt_texel / rt_atlas_stats (include/rt_hip.h): what a UV atlas reports of a texel -- the lowest triangle that covers its centre, where on it, how many do;
# flags 1 covered, 2 copied by the gutter; uncovered is primitive_id = 0xFFFFFFFF and zeros -- and of the whole cover
texel = np.dtype([("bc", "<f4", (2,)), ("primitive_id", "<u4"), ("count", "<u2"), ("flags", "<u2")])
atlas_stats = np.dtype([("covered", "<u4"), ("overlapped", "<u4"), ("gutter", "<u4"), ("triangles_skipped", "<u4"), ("triangles_without_texel", "<u4"),
                        ("triangles_filtered", "<u4"), ("reserved", "<u4", (2,))])
assert texel.itemsize == 16 and atlas_stats.itemsize == 32
# rt_point / rt_nearest (include/rt_hip.h): a nearest-point query's point (max_distance may be +inf) and its answer; nothing found is primitive_id = 0xFFFFFFFF and zeros
point = np.dtype([("position", "<f4", (3,)), ("max_distance", "<f4")])
nearest = np.dtype([("position", "<f4", (3,)), ("distance", "<f4"), ("bc", "<f4", (2,)), ("primitive_id", "<u4"), ("flags", "<u4")])
# rt_ray_hits (include/rt_hip.h): what an all-hits query reports of a ray: the crossings, how many of them enter, how many are listed; flags bit 0 = walked, bit 8 + j = listed hit j is an exit
ray_hits = np.dtype([("count", "<u4"), ("entering", "<u4"), ("stored", "<u4"), ("flags", "<u4")])
# rt_point_hits (include/rt_hip.h): what a within query reports of a point: the triangles within its radius, how many of them are listed, the nearest one; flags bit 0 = searched, bit 1 = a k-nearest answer
point_hits = np.dtype([("count", "<u4"), ("stored", "<u4"), ("nearest_primitive", "<u4"), ("flags", "<u4")])
# rt_region / rt_region_hits / rt_region_member (include/rt_hip.h): an overlap query's convex region -- num_planes half-spaces, plane k = (nx, ny, nz, d), a point x is
# outside when ((nx x0 + ny x1) + nz x2) + d > 0 --, what it reports of it (the touching and the inside triangles; flags bit 0 = searched) and a listed member
# (flags bit 0 = inside, bit 8 + k = plane k has 1 or 2 corners outside)
region = np.dtype([("num_planes", "<u4"), ("reserved", "<u4", (3,)), ("planes", "<f4", (8, 4))])
region_hits = np.dtype([("count", "<u4"), ("inside", "<u4"), ("stored", "<u4"), ("flags", "<u4")])
region_member = np.dtype([("primitive_id", "<u4"), ("flags", "<u4")])
# rt_probe / rt_probe_hits / rt_cross_member (include/rt_hip.h): a crossing query's triangle (every fourth component is ignored), what it reports of it (the
# crossing triangles, how many are listed, the lowest id; flags bit 0 = searched, bit 1 = an any-mode answer) and a listed member (flags bits 0..2: the probe's
# edges cut the triangle, bits 3..5: the triangle's edges cut the probe; c0, c1: the contact points of the two lowest set bits)
probe = np.dtype([("p1", "<f4", (4,)), ("p2", "<f4", (4,)), ("p3", "<f4", (4,))])
probe_hits = np.dtype([("count", "<u4"), ("stored", "<u4"), ("first_primitive", "<u4"), ("flags", "<u4")])
cross_member = np.dtype([("primitive_id", "<u4"), ("flags", "<u4"), ("c0", "<f4", (3,)), ("c1", "<f4", (3,))])
# rt_separation (include/rt_hip.h): a separation query's answer -- the two closest points, their distance, the nearest triangle, flags (bit 0 searched, bit 1
# found, bit 2 the pair crosses) and the winning candidate (0..2 a probe corner, 3..5 a corner of the triangle, 6 + 3 i + j an edge pair, 15 a crossing)
separation = np.dtype([("on_probe", "<f4", (3,)), ("distance", "<f4"), ("on_scene", "<f4", (3,)), ("primitive_id", "<u4"), ("flags", "<u4"), ("feature", "<u4"),
                       ("pad", "<u4", (2,))])
# rt_skin_influence (include/rt_hip.h): one triangle corner's four bones and weights (rt_scene_set_skin); an unused slot is weight 0 on any valid bone
skin_influence = np.dtype([("bone", "<u2", (4,)), ("weight", "<f4", (4,))])
# rt_morph_delta (include/rt_hip.h): one morph target's delta at one triangle corner (rt_scene_set_morph); corner = 3 * triangle + c, pad = 0
morph_delta = np.dtype([("corner", "<u4"), ("position", "<f4", (3,)), ("normal", "<f4", (3,)), ("pad", "<u4")])
camera = np.dtype([("position", float3), ("front", float3), ("up", float3), ("fov", "<f4"),
                   ("aspect_ratio", "<f4"), ("aperture", "<f4"), ("focus_distance", "<f4")])

assert ray.itemsize == 32 and hit.itemsize == 16 and scene_info.itemsize == 16
assert packed_material.itemsize == 20 and light.itemsize == 48 and texture.itemsize == 16
assert vertex.itemsize == 48 and triangle.itemsize == 160 and bvh_node.itemsize == 48
assert camera.itemsize == 64 and surface.itemsize == 64 and bake_result.itemsize == 16 and light_bake_result.itemsize == 32
assert point.itemsize == 16 and nearest.itemsize == 32 and ray_hits.itemsize == 16 and point_hits.itemsize == 16
assert region.itemsize == 144 and region_hits.itemsize == 16 and region_member.itemsize == 8
assert probe.itemsize == 48 and probe_hits.itemsize == 16 and cross_member.itemsize == 32
assert separation.itemsize == 48 and skin_influence.itemsize == 24 and morph_delta.itemsize == 32


def influences(bones, weights):
    """types.skin_influence[n, 3] of bones int[n, 3, 4] (each 0 .. 65535) and weights float[n, 3, 4]: (triangle, corner, slot), the order rt_scene_set_skin
    takes them in when flattened"""
    b, w = np.asarray(bones), np.asarray(weights, np.float32)
    if b.ndim != 3 or b.shape[1:] != (3, 4) or w.shape != b.shape:
        raise ValueError("influences: bones and weights must both be [n, 3, 4]")
    if b.size and (b.min() < 0 or b.max() > 0xFFFF):
        raise ValueError("influences: a bone index does not fit 16 bits")
    out = np.zeros((len(b), 3), skin_influence)
    out["bone"], out["weight"] = b, w
    return out


def morph_targets(targets):
    """(types.morph_delta[total], uint32[len(targets) + 1]) of a list of sparse targets, each (corners int[k], dpos float[k, 3], dnormal float[k, 3] or None):
    what rt_scene_set_morph takes.  corners are 3 * triangle + c in the uploaded order; dnormal None = a position-only target (zeros: the normals stay)."""
    counts = []
    parts = []
    for t, target in enumerate(targets):
        if len(target) != 3:
            raise ValueError("morph_targets: target %d is not (corners, dpos, dnormal)" % t)
        corners = np.asarray(target[0])
        if corners.ndim != 1 or (corners.size and (not np.issubdtype(corners.dtype, np.integer) or corners.min() < 0 or corners.max() > 0xFFFFFFFF)):
            raise ValueError("morph_targets: target %d's corners must be a flat array of unsigned 32-bit indices" % t)
        dp = np.asarray(target[1], np.float32).reshape(-1, 3) if np.size(target[1]) else np.zeros((0, 3), np.float32)
        dn = np.zeros_like(dp) if target[2] is None else (np.asarray(target[2], np.float32).reshape(-1, 3) if np.size(target[2]) else np.zeros((0, 3), np.float32))
        if len(dp) != len(corners) or len(dn) != len(corners):
            raise ValueError("morph_targets: target %d wants one position delta (and one normal delta) per corner" % t)
        d = np.zeros(len(corners), morph_delta)
        d["corner"], d["position"], d["normal"] = corners, dp, dn
        parts.append(d)
        counts.append(len(d))
    offsets = np.zeros(len(counts) + 1, np.uint64)
    offsets[1:] = np.cumsum(np.asarray(counts, np.uint64))
    if offsets[-1] > 0xFFFFFFFF:
        raise ValueError("morph_targets: more than 2^32 - 1 deltas")
    deltas = np.concatenate(parts) if parts else np.zeros(0, morph_delta)
    return deltas, offsets.astype(np.uint32)


def probes_from_corners(corners):
    """types.probe[n] of float[n, 3, 3] corners (probe, corner, coordinate)"""
    c = np.asarray(corners, np.float32).reshape(-1, 3, 3)
    out = np.zeros(len(c), probe)
    for k, name in enumerate(("p1", "p2", "p3")):
        out[name][:, :3] = c[:, k]
    return out


def probes_from_triangles(vertices, faces):
    """types.probe[len(faces)] of an indexed mesh: vertices float[nv, 3], faces int[nf, 3]"""
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    return probes_from_corners(v[f])


def planes_region(planes):
    """a types.region scalar of 1 to 8 planes (nx, ny, nz, d): the points with nx x + ny y + nz z + d <= 0 on every one"""
    pl = np.asarray(planes, np.float32).reshape(-1, 4)
    if not 1 <= len(pl) <= 8:
        raise ValueError("planes_region: a region has 1 to 8 planes, not %d" % len(pl))
    g = np.zeros((), region)
    g["num_planes"] = len(pl)
    g["planes"][:len(pl)] = pl
    return g


def box_region(lo, hi):
    """the axis-aligned box lo <= x <= hi as a types.region scalar: six planes, -x, -y, -z, then +x, +y, +z"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    pl = np.zeros((6, 4), np.float32)
    for a in range(3):
        pl[a, a], pl[a, 3] = -1.0, lo[a]              # lo - x > 0: outside
        pl[3 + a, a], pl[3 + a, 3] = 1.0, -hi[a]      # x - hi > 0: outside
    return planes_region(pl)


def oriented_box_region(matrix3x4, half_extents):
    """the box |u_a| <= half_extents[a] in the frame of a 3x4 matrix (rt_scene_pose's layout: x_world = M[:, :3] u + M[:, 3], columns orthogonal, any
    length) as a types.region scalar of six planes: per axis n = +-column / |column|, through centre +- column * half_extent"""
    m = np.asarray(matrix3x4, np.float64).reshape(3, 4)
    h = np.asarray(half_extents, np.float64)
    pl = np.zeros((6, 4))
    for a in range(3):
        col = m[:, a]
        ln = np.linalg.norm(col)
        n = col / ln
        for side, sign in ((a, -1.0), (3 + a, 1.0)):
            pl[side, :3] = sign * n
            pl[side, 3] = -(sign * n) @ m[:, 3] - h[a] * ln
    return planes_region(pl.astype(np.float32))


def default_camera(width, height):
    """The reference's start-up camera (src/utils/camera_controller.cpp:30-41,77-80):
    position (0,-1,1), yaw = pitch = MATH_PIDIV2, fov = 75*3.1415/180, Z-up."""
    f32 = np.float32
    yaw = f32(1.570796327)
    pitch = f32(1.570796327)
    # std::cosf/std::sinf in binary32 (glibc); values below are what the
    # reference computes, stored as exact binary32 literals so that no libm
    # is involved at run time (pinned by tests/test_ref_pin.py).
    cy, sy = f32(np.cos(yaw, dtype=f32)), f32(np.sin(yaw, dtype=f32))
    cp, sp = f32(np.cos(pitch, dtype=f32)), f32(np.sin(pitch, dtype=f32))
    front = np.array([f32(cy * sp), f32(sy * sp), cp], dtype=f32)
    up0 = np.array([0, 0, 1], dtype=f32)

    def cross(a, b):
        return np.array([f32(f32(a[1] * b[2]) - f32(a[2] * b[1])),
                         f32(f32(a[2] * b[0]) - f32(a[0] * b[2])),
                         f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))], dtype=f32)

    r = cross(front, up0)
    ln = f32(np.sqrt(f32(f32(f32(r[0] * r[0]) + f32(r[1] * r[1])) + f32(r[2] * r[2]))))
    right = np.array([f32(r[0] / ln), f32(r[1] / ln), f32(r[2] / ln)], dtype=f32)
    up = cross(right, front)
    cam = np.zeros((), dtype=camera)
    cam["position"]["x"], cam["position"]["y"], cam["position"]["z"] = 0.0, -1.0, 1.0
    for k, v in zip("xyz", front):
        cam["front"][k] = v
    for k, v in zip("xyz", up):
        cam["up"][k] = v
    cam["fov"] = f32(f32(f32(75.0) * f32(3.1415)) / f32(180.0))
    cam["aspect_ratio"] = f32(f32(width) / f32(height))
    cam["aperture"] = 0.0
    cam["focus_distance"] = 10.0
    return cam


def _strip(a):
    """Field-wise view of a structured array without padding members (the
    reference leaves float3 padding uninitialised, mathlib.hpp:74-76)."""
    import numpy.lib.recfunctions as rfn
    out = []

    def walk(arr, dt):
        for name in dt.names:
            sub = dt.fields[name][0]
            if name in ("w", "padding", "pad"):
                continue
            if sub.names:
                walk(arr[name], sub)
            else:
                out.append(np.ascontiguousarray(arr[name]).reshape(len(arr), -1).view(np.uint32))
    walk(a, a.dtype)
    return np.concatenate(out, axis=1) if out else np.zeros((len(a), 0), np.uint32)


def records_equal(a, b):
    """Bitwise equality of two record arrays over their payload fields."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.size == 0:
        return True
    if a.dtype.names is None:
        return np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return np.array_equal(_strip(a), _strip(b))

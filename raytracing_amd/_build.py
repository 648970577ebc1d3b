"""Build recipes for the native parts (called by __graft_entry__.build()).

  librt_hip.so   HIP kernels + C-ABI, hipcc --offload-arch=gfx950 (cross-compiles without a GPU); its translation units: HIP_UNITS below
  librt_host.so  C++ host layer (Scene, Bvh, Integrator, HIPPathTraceIntegrator, Render) + flat C API
  rt_render      headless CLI with the reference's flags
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
HOST = os.path.join(HERE, "host")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + HOST]

# -ffp-contract=off + correctly rounded divide/sqrt + no fast-math: the
# arithmetic contract that makes GPU results bit-identical to the CPU oracle.
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-fPIC", "-shared", "-ldl"]
CXX_FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fPIC"]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd):
    subprocess.check_call(cmd, cwd=ROOT)


def hipcc():
    for c in ("hipcc", "/opt/rocm/bin/hipcc"):
        try:
            subprocess.check_output([c, "--version"], stderr=subprocess.STDOUT)
            return c
        except Exception:
            continue
    raise RuntimeError("hipcc not found")


# librt_hip.so = several translation units.  Who owns what:
#   rt_hip.hip holds every launch of the hot path's code object and nothing else: the units that schedule a frame's samples call it through frame_launch.h, and
#   codeobj.code_object_sha256 identifies its code object, so no host bookkeeping rebuilds or re-hashes the hot path.
#   Each other family of kernels -- the tree work on the device, the filters, the refit, pose / skin / morph, the eight scene queries -- is a unit with a code
#   object of its own: its kernels and its launch driver.
#   Everything else is host-only units (device=False: plain C++, no code object), each on the internal header that gives it what it needs and no more:
#   on context.h the context and the buffers (context.cpp), the scene's upload, trees and adaptation worker (scene_upload.cpp), the entry points of pose, skin and
#   morph (scene_moved.cpp) and of the queries (scene_queries.cpp); on frame.h + frame_launch.h what a frame is made of and how it is laid out (frame_layout.cpp)
#   and when its samples run (frame_schedule.cpp); on frame.h alone the fold adaptation's render-thread side (frame_fold_hooks.cpp), the filters' entry points
#   (frame_filters.cpp) and the kernel-less readers (frame_readers.cpp); and the host side of the tree work (wide_bvh.cpp).
HIP_UNITS = [
    ("rt_hip", "rt_hip.hip", True),            # every launch of kernels.h (the hot path), with its grid and arguments: namespace launch of frame_launch.h, the one-launch entries (rt_compute_aovs .. rt_debug_eval), the device groups
    ("device_fold", "device_fold.hip", True),  # fold_kernels.h + its host driver
    ("filters", "filters.hip", True),          # the guide pass, the spatial filter's a-trous passes, the temporal filter's stages (a code object of its own, like device_fold's)
    ("refit", "refit.hip", True),              # the refit of the scene's trees when its triangles move: kernels + their host driver + the host restatement (a code object of its own)
    ("moved", "moved.hip", True),              # what pose, skin and morph keep in common beside the scene, a rest pose and a staging area (moved::Stage), and the one kernel that makes a rest pose (a small code object of its own); the tile their kernels share is moved_tile.h, by inclusion
    ("pose", "pose.hip", True),                # the scene's objects posed from one matrix per object: kernels + host driver + the host restatement (a code object of its own)
    ("skin", "skin.hip", True),                # the scene's triangles skinned from a palette of bone matrices, four bones per corner: kernels + host driver + the host restatement (a code object of its own)
    ("morph", "morph.hip", True),              # the scene's triangles morphed from one weight per sparse morph target, alone or fused with the skin in one pass: kernels + host driver + the host restatement (a code object of its own)
    ("query", "query.hip", True),              # caller-supplied rays traced against the uploaded scene, the surface record of a hit: kernels (the walk itself: walk_kernels.h, shared with bake and nearest) + the host driver core of all three + the host restatement (a code object of its own)
    ("bake", "bake.hip", True),                # ambient occlusion and bent normals at caller-supplied points: kernels on walk_kernels.h + host driver on query.hip's core + the host restatement (a code object of its own)
    ("light_bake", "light_bake.hip", True),    # the irradiance of the sky and of the scene's analytic lights at caller-supplied points, direct terms only: kernels on walk_kernels.h + host driver on query.hip's core + the host restatement (a code object of its own: bake.hip's does not change)
    ("nearest", "nearest.hip", True),          # the nearest surface point to caller-supplied points: kernels on walk_kernels.h's stack + host driver on query.hip's core + the host's brute force and walk (a code object of its own)
    ("within", "within.hip", True),            # every triangle within a radius of caller-supplied points, counted and sorted: kernels on walk_kernels.h's stack and point_box_step + host driver on query.hip's core + the host's brute force and walk (a code object of its own)
    ("region", "region.hip", True),            # every triangle a caller-supplied convex region (up to 8 half-spaces) touches or encloses, counted and listed, and the per-triangle select of a few regions: kernels on walk_kernels.h's stack and region_box_step + host driver on query.hip's core + the host's brute force and walk (a code object of its own)
    ("cross", "cross.hip", True),              # every scene triangle a caller-supplied triangle crosses (boxes, the probe's plane, six segment tests) with contact points, and the scene's self-crossings: kernels on walk_kernels.h's stack, volume_step and cross_box_step + host driver on query.hip's core + the host's brute force and walk (a code object of its own)
    ("separation", "separation.hip", True),    # the nearest scene triangle to a caller-supplied triangle (the crossing verdict, then fifteen point-triangle and edge-edge candidates) with the two closest points, and the scene's clearances: kernels on walk_kernels.h's stack, volume_step and probe_box_step + host driver on query.hip's core + the host's brute force and walk (a code object of its own)
    ("all_hits", "all_hits.hip", True),        # every surface a caller-supplied ray crosses, counted and sorted: kernels on walk_kernels.h + host driver on query.hip's core + the host's brute force (a code object of its own)
    ("atlas", "atlas.hip", True),              # the scene's triangles rasterised into a UV atlas (no tree walked: one lane per triangle, the wave sweeps the large ones in 8 x 8 tiles), the gutter, the surfaces its texels show: kernels + host driver + the host restatement of atlas.h's integer rule (a code object of its own)
    ("scene_queries", "scene_queries.cpp", False),   # the C entry points of the eight query families and the atlas above (rt_scene_trace* .. rt_scene_separation*, rt_scene_atlas* / rt_scene_atlas_bake, rt_scene_light_bake* / rt_scene_atlas_bake_light, their rt_debug_* forms) on context.h: an edit to a query's bookkeeping rebuilds no kernel (no device code)
    ("scene_upload", "scene_upload.cpp", False),     # rt_scene_upload and its stages, tree choice, FoldAdapt's worker, rt_scene_refit* / export_folds / import_folds / tree_report, the tree work's rt_debug_* forms, on context.h + fold_adapt.h (no device code)
    ("scene_moved", "scene_moved.cpp", False),       # the C entry points of pose, skin and morph (rt_scene_set_objects .. rt_scene_morph_skin, their rt_debug_* forms) on context.h; each ends in scene_upload.cpp's refit_device (no device code)
    ("context", "context.cpp", False),               # the context and the buffers: context::fail and the thread's message, dev_fill / scene_array / query_check_status / quiesce, rt_ctx_* / rt_finish / rt_host_* / rt_upload_blue_noise_tables, every rt_buffer_*, on context.h + frame.h (no device code)
    ("frame_layout", "frame_layout.cpp", False),     # what a frame is made of: rt_frame_create / destroy, the per-path buffers' layout (chunk_plan, alloc_path_buffers, ensure_slots), the pipes' streams, rt_set_option / rt_set_camera / rt_reset / rt_frame_reserve_samples, the three picks, on frame.h + frame_launch.h (no device code)
    ("frame_schedule", "frame_schedule.cpp", False), # when a frame's samples run: the stage entries' record-or-run logic, the RT_OPT_FRAME_KERNEL = 255 measuring schedule, rt_advance_sample, rt_integrate's batches and compact-log fallback, the banks of RT_OPT_SAMPLES_AHEAD, on frame.h + frame_launch.h (no device code)
    ("frame_fold_hooks", "frame_fold_hooks.cpp", False),   # the render thread's side of RT_CTX_OPT_ADAPTIVE_FOLD: probe frame, hand-over to the worker, adoption (frame::fold_adapt_hook), on frame.h + fold_adapt.h through the public rt_* entries (no device code)
    ("frame_filters", "frame_filters.cpp", False),   # the spatial and temporal filters' entry points on a frame and on caller arrays (rt_frame_filter* .. rt_frame_read_guide_motion, rt_debug_filter*, rt_debug_guide_motion) and the three states a filtered frame keeps, on frame.h + filters_host.h (no device code)
    ("frame_readers", "frame_readers.cpp", False),   # the frame's readers that launch no kernel: rt_frame_read_radiance / copy_radiance / get_profile and the rt_frame_debug_* readers, on frame.h (no device code)
    ("wide_bvh", "wide_bvh.cpp", False),     # build_wide_bvh, pair layout, the adaptation's host walks (no device code)
]


def _unit_sources(src):
    """what a unit is rebuilt for: its source and every header of csrc/ + include/ (coarse, like the single-unit build was)"""
    srcs = [os.path.join(CSRC, src)] + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
    return srcs + [os.path.join(ROOT, "include", f) for f in ("rt_hip.h", "rt_types.h")]


def build_hip(force=False, extra_flags=(), out=None, obj_dir=None):
    out = out or os.path.join(HERE, "librt_hip.so")
    obj_dir = obj_dir or os.path.join(HERE, "build")
    os.makedirs(obj_dir, exist_ok=True)
    compile_flags = [f for f in HIP_FLAGS if f not in ("-shared", "-ldl")] + ["-c"] + list(extra_flags)
    objs, procs = [], []
    for name, src, device in HIP_UNITS:
        obj = os.path.join(obj_dir, name + ".o")
        objs.append(obj)
        if force or _newer(obj, _unit_sources(src)):
            flags = compile_flags if device else [f for f in compile_flags if not f.startswith("--offload-arch") and not f.startswith("-fhip")]
            procs.append(subprocess.Popen([hipcc()] + flags + INC + [os.path.join(CSRC, src), "-o", obj], cwd=ROOT))
    failed = [p.args for p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    if force or _newer(out, objs):
        _run([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", out])
    return out


def build_host(force=False):
    out = os.path.join(HERE, "librt_host.so")
    cpps = [os.path.join(HOST, f) for f in ("bvh.cpp", "scene.cpp", "scene_cache.cpp", "png_loader.cpp", "jpeg_loader.cpp", "integrator.cpp",
                                            "hip_pt_integrator.cpp", "render.cpp", "host_capi.cpp")]
    deps = cpps + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".hpp")]
    deps += [os.path.join(ROOT, "include", f) for f in ("rt_hip.h", "rt_types.h")]
    hip = os.path.join(HERE, "librt_hip.so")
    if force or _newer(out, deps + [hip]):
        _run(["g++"] + CXX_FLAGS + ["-shared"] + INC + cpps + ["-o", out, "-L" + HERE, "-lrt_hip", "-lz", "-pthread", "-Wl,-rpath,$ORIGIN"])
    exe = os.path.join(HERE, "rt_render")
    main = os.path.join(HOST, "main.cpp")
    if force or _newer(exe, [main, out]):
        _run(["g++"] + CXX_FLAGS[:-1] + INC + [main, "-o", exe, "-L" + HERE, "-lrt_host", "-lrt_hip",
                                               "-Wl,-rpath,$ORIGIN"])
    return out


def build_oracle():
    """The CPU checkers (test infrastructure): oracle/liboracle.so always,
    oracle/_ref/*.so when the reference checkout is present."""
    _run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle"])
    if os.path.isdir("/root/reference/src/kernels/cl"):
        _run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])


def build_all(force=False):
    build_hip(force)
    build_host(force)
    build_oracle()

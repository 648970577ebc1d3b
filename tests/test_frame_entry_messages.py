"""The exact text of what the frame's filters and kernel-less readers (frame_filters.cpp, frame_readers.cpp) refuse without a frame or a context: every
such rt_frame_* entry with its frame NULL, every NULL-argument refusal of the four rt_debug_* forms of the filters, and what the two filter descriptors
turn down -- iterations, flags, alphas, sigmas.  No device is needed: each call is refused before anything is launched or read.  One call is accepted:
the spatial filter with no iterations is a copy."""
import ctypes as C
import numpy as np
from raytracing_amd import capi

NULL_ARG = "NULL argument"
SPATIAL_SIGMAS = ("sigma_color", "sigma_normal", "sigma_depth")
TEMPORAL_SIGMAS = ("sigma_luminance", "sigma_normal", "sigma_depth")
SPATIAL_SIGMA_TEXT = "sigma_color, sigma_normal and sigma_depth must be > 0 and finite"
TEMPORAL_SIGMA_TEXT = "sigma_luminance, sigma_normal and sigma_depth must be > 0 and finite"
BAD_SIGMAS = (0.0, -1.0, float("nan"), float("inf"))


def test_every_refusal_without_a_frame_or_a_context_keeps_its_text():
    lib = capi.load()
    scratch = np.zeros(64, np.uint8)
    B = scratch.ctypes.data                     # stands for any array that is passed but never read
    U = C.cast(B, C.POINTER(C.c_uint32))        # ... where the prototype wants a typed pointer
    sd = C.byref(capi.filter_desc(None))        # the header's defaults: both descriptors pass their checks
    td = C.byref(capi.temporal_filter_desc(None))
    profile = capi.rt_profile()

    def spatial(**kw):
        return C.byref(capi.filter_desc(kw))

    def temporal(**kw):
        return C.byref(capi.temporal_filter_desc(kw))

    def debug_filter(desc, w=1, h=1):
        return (None, w, h, B, B, B, B, desc, B)

    def debug_temporal(desc, w=1, h=1):
        return (None, w, h, B, B) + (B,) * 8 + (desc, B, B, B)

    def debug_temporal_motion(desc, w=1, h=1):
        return (None, w, h, B, B) + (B,) * 10 + (desc, B, B, B)

    def without(args, i):
        return args[:i] + (None,) + args[i + 1:]

    # (entry, arguments, who the message names, text)
    table = [
        # the moved frame entries, frame NULL
        ("rt_frame_filter", (None, sd, B), None, NULL_ARG),
        ("rt_frame_filter", (None, None, None), None, NULL_ARG),
        ("rt_frame_read_guides", (None, B, B, B, U), None, NULL_ARG),
        ("rt_frame_read_guides", (None, None, None, None, None), None, NULL_ARG),
        ("rt_frame_filter_temporal", (None, td, B), None, NULL_ARG),
        ("rt_frame_filter_temporal", (None, None, None), None, NULL_ARG),
        ("rt_frame_filter_history_reset", (None,), None, NULL_ARG),
        ("rt_frame_read_filter_history", (None, B, B), None, NULL_ARG),
        ("rt_frame_read_filter_history", (None, None, None), None, NULL_ARG),
        ("rt_frame_read_guide_motion", (None, B, B), None, NULL_ARG),
        ("rt_frame_read_guide_motion", (None, None, None), None, NULL_ARG),
        ("rt_frame_read_radiance", (None, B), None, NULL_ARG),
        ("rt_frame_read_radiance", (None, None), None, NULL_ARG),
        ("rt_frame_copy_radiance", (None, B), None, NULL_ARG),
        ("rt_frame_copy_radiance", (None, None), None, NULL_ARG),
        ("rt_frame_get_profile", (None, C.byref(profile)), None, NULL_ARG),
        ("rt_frame_get_profile", (None, None), None, NULL_ARG),
        ("rt_frame_debug_read_queue", (None, 0, 0, B, B, B, 1, U), None, NULL_ARG),
        ("rt_frame_debug_read_queue", (None, 1, 0, None, None, None, 0, None), None, NULL_ARG),
        ("rt_frame_debug_read_hits", (None, B, 1), None, NULL_ARG),
        ("rt_frame_debug_read_hits", (None, None, 0), None, NULL_ARG),
        ("rt_frame_debug_frame_rows", (None, B, 1, U, U), None, NULL_ARG),
        ("rt_frame_debug_frame_rows", (None, None, 0, None, None), None, NULL_ARG),
        ("rt_frame_debug_timeline", (None, 1, None), None, "frame is NULL"),
        ("rt_frame_debug_timeline", (None, 0, B), None, "frame is NULL"),
        # the motion images on caller arrays, ctx NULL
        ("rt_debug_guide_motion", (None, 1, None, B, 1, B, B), None, NULL_ARG),
        ("rt_debug_guide_motion", (None, 1, B, None, 1, B, B), None, NULL_ARG),
        ("rt_debug_guide_motion", (None, 1, B, B, 1, None, B), None, NULL_ARG),
        ("rt_debug_guide_motion", (None, 1, B, B, 1, B, None), None, NULL_ARG),
    ]
    # the spatial filter on caller arrays, ctx NULL: each of its six arrays (the descriptor among them) missing, an empty image, the descriptor
    for i in (3, 4, 5, 6, 7, 8):
        table.append(("rt_debug_filter", without(debug_filter(sd), i), None, NULL_ARG))
    for w, h in ((0, 1), (1, 0), (0, 0)):
        table.append(("rt_debug_filter", debug_filter(sd, w, h), None, "empty image"))
    # ... and the temporal filter's two forms (prev_cam, argument 4, may be NULL; so may the motion form's two motion images, 13 and 14): the motion form's
    # refusals name rt_debug_filter_temporal, the family
    family = "rt_debug_filter_temporal"
    for i in (3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16):
        table.append(("rt_debug_filter_temporal", without(debug_temporal(td), i), family, NULL_ARG))
    for i in (3, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 18):
        table.append(("rt_debug_filter_temporal_motion", without(debug_temporal_motion(td), i), family, NULL_ARG))
    for w, h in ((0, 1), (1, 0), (0, 0)):
        table.append(("rt_debug_filter_temporal", debug_temporal(td, w, h), family, "empty image"))
        table.append(("rt_debug_filter_temporal_motion", debug_temporal_motion(td, w, h), family, "empty image"))
    # what both descriptors turn down, through every form that checks one without a frame
    forms = [("rt_debug_filter", debug_filter, spatial, SPATIAL_SIGMAS, SPATIAL_SIGMA_TEXT, None),
             ("rt_debug_filter_temporal", debug_temporal, temporal, TEMPORAL_SIGMAS, TEMPORAL_SIGMA_TEXT, family),
             ("rt_debug_filter_temporal_motion", debug_temporal_motion, temporal, TEMPORAL_SIGMAS, TEMPORAL_SIGMA_TEXT, family)]
    for name, args, desc, sigmas, sigma_text, who in forms:
        table.append((name, args(desc(iterations=9)), who, "iterations must be 0 .. 8"))
        table.append((name, args(desc(iterations=0xFFFFFFFF)), who, "iterations must be 0 .. 8"))
        table.append((name, args(desc(flags=2)), who, "unknown flags (RT_FILTER_DEMODULATE is the only one)"))
        table.append((name, args(desc(flags=3)), who, "unknown flags (RT_FILTER_DEMODULATE is the only one)"))
        for sigma in sigmas:
            for bad in BAD_SIGMAS:
                table.append((name, args(desc(**{sigma: bad})), who, sigma_text))
        # the order of the checks: iterations, flags, (alphas,) sigmas
        table.append((name, args(desc(iterations=9, flags=2, **{sigmas[0]: 0.0})), who, "iterations must be 0 .. 8"))
        table.append((name, args(desc(flags=2, **{sigmas[0]: 0.0})), who, "unknown flags (RT_FILTER_DEMODULATE is the only one)"))
    for name, args, desc, sigmas, sigma_text, who in forms[1:]:
        for alpha in ("alpha_color", "alpha_moments"):
            for bad in (-0.1, 1.1, float("nan")):
                table.append((name, args(desc(**{alpha: bad})), who, "alpha_color and alpha_moments must be in 0 .. 1"))
        table.append((name, args(desc(flags=2, alpha_color=1.1)), who, "unknown flags (RT_FILTER_DEMODULATE is the only one)"))
        table.append((name, args(desc(alpha_color=1.1, sigma_luminance=0.0)), who, "alpha_color and alpha_moments must be in 0 .. 1"))

    moved = {"rt_frame_filter", "rt_frame_read_guides", "rt_frame_filter_temporal", "rt_frame_filter_history_reset", "rt_frame_read_filter_history",
             "rt_frame_read_guide_motion", "rt_frame_read_radiance", "rt_frame_copy_radiance", "rt_frame_get_profile", "rt_frame_debug_read_queue",
             "rt_frame_debug_read_hits", "rt_frame_debug_frame_rows", "rt_frame_debug_timeline", "rt_debug_filter", "rt_debug_filter_temporal",
             "rt_debug_filter_temporal_motion", "rt_debug_guide_motion"}
    assert {name for name, _, _, _ in table} == moved and moved <= set(capi.EXPORTS)
    for name, args, who, text in table:
        rc = getattr(lib, name)(*args)
        said = lib.rt_last_error(None).decode()
        assert rc == 1 and said == (who or name) + ": " + text, (name, args, rc, said)
    # the two that answer a NULL frame without a message
    assert lib.rt_frame_radiance_device_ptr(None) is None and lib.rt_frame_sample_count(None) == 0
    assert lib.rt_last_error(None).decode() == table[-1][2] + ": " + table[-1][3]
    assert not scratch.any()                    # nothing was written through a refused call's arguments

    # accepted: no motion images to make for no pixels, and the spatial filter without iterations returns its input
    assert lib.rt_debug_guide_motion(None, 0, B, None, 0, B, B) == 0
    hdr = np.arange(16, dtype=np.float32).reshape(2, 2, 4) * 0.37 - 1.0
    hdr[1, 1] = (np.nan, np.inf, -0.0, 1e-42)                               # bytes, not values: nothing is computed
    zeros4, zeros1 = np.zeros((2, 2, 4), np.float32), np.zeros((2, 2), np.float32)
    out = np.full((2, 2, 4), 7.0, np.float32)
    assert lib.rt_debug_filter(None, 2, 2, hdr.ctypes.data, zeros4.ctypes.data, zeros4.ctypes.data, zeros1.ctypes.data, spatial(iterations=0),
                               out.ctypes.data) == 0
    assert out.tobytes() == hdr.tobytes()
    assert not scratch.any()

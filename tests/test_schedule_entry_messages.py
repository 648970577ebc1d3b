"""The exact text of what the context's, the buffers' and the frames' own entries (context.cpp, frame_layout.cpp, frame_schedule.cpp) refuse on their
arguments alone: rt_ctx_create without an out pointer, the context entries without a context, every rt_buffer_* without a buffer, rt_frame_create without a
context, a descriptor or an out pointer, and the options, camera, reset, stage, sample, reservation and pick entries without a frame.  No device is needed:
each call is refused before anything is launched, allocated or read.  The entries that accept a NULL handle answer it as they always have."""
import ctypes as C
import numpy as np
from raytracing_amd import capi

NULL_ARG = "NULL argument"
NULL_FRAME = "frame is NULL"
NULL_CTX = "ctx is NULL"


def test_every_refusal_on_arguments_alone_keeps_its_text():
    lib = capi.load()
    scratch = np.zeros(64, np.uint8)
    B = scratch.ctypes.data                     # stands for any array that is passed but never read
    U = C.cast(B, C.POINTER(C.c_uint32))        # ... where the prototype wants a typed pointer
    out = C.c_void_p(0x5A5A)                    # an out handle: a refused rt_frame_create leaves it alone (it was never a handle of this library)
    desc = capi.rt_frame_desc()

    # (entry, arguments, text)
    table = [
        # context.cpp
        ("rt_ctx_create", (0, None), "out is NULL"),
        ("rt_ctx_create", (7, None), "out is NULL"),
        ("rt_finish", (None,), NULL_CTX),
        ("rt_ctx_device_info", (None, None, 0, None, None), NULL_CTX),
        ("rt_ctx_set_option", (None, 0, 0), NULL_CTX),
        ("rt_ctx_set_option", (None, 12345, 7), NULL_CTX),
        ("rt_host_register", (None, B, 64), "bad argument"),
        ("rt_host_register", (None, None, 0), "bad argument"),
        ("rt_host_unregister", (None, B), "bad argument"),
        ("rt_host_unregister", (None, None), "bad argument"),
        ("rt_upload_blue_noise_tables", (None, B, B, B), NULL_ARG),
        ("rt_upload_blue_noise_tables", (None, None, None, None), NULL_ARG),
        ("rt_buffer_create", (None, 16, None, C.byref(out)), NULL_ARG),
        ("rt_buffer_create", (None, 16, B, None), NULL_ARG),
        ("rt_buffer_write", (None, 0, B, 4), NULL_ARG),
        ("rt_buffer_write", (None, 0, None, 0), NULL_ARG),
        ("rt_buffer_read", (None, 0, B, 4), NULL_ARG),
        ("rt_buffer_read", (None, 0, None, 0), NULL_ARG),
        ("rt_buffer_copy", (None, None, 0, 0, 0), NULL_ARG),
        ("rt_buffer_copy", (None, None, 4, 8, 16), NULL_ARG),
        # frame_layout.cpp
        ("rt_frame_create", (None, C.byref(desc), C.byref(out)), NULL_ARG),
        ("rt_frame_create", (None, None, C.byref(out)), NULL_ARG),
        ("rt_frame_create", (None, None, None), NULL_ARG),
        ("rt_set_option", (None, 0, 0), NULL_FRAME),
        ("rt_set_option", (None, 12345, 7), NULL_FRAME),
        ("rt_set_camera", (None, B), NULL_ARG),
        ("rt_set_camera", (None, None), NULL_ARG),
        ("rt_reset", (None,), NULL_FRAME),
        ("rt_frame_reserve_samples", (None, 4, U), NULL_FRAME),
        ("rt_frame_reserve_samples", (None, 0, None), NULL_FRAME),
        ("rt_frame_pick", (None, 0, 0, B, B, B), NULL_FRAME),
        ("rt_frame_pick", (None, 9, 9, None, None, None), NULL_FRAME),
        ("rt_frame_pick_all", (None, 0, 0, 4, B, B, B, B), NULL_FRAME),
        ("rt_frame_pick_all", (None, 9, 9, 0, None, None, None, None), NULL_FRAME),
        ("rt_frame_pick_rect", (None, 0, 0, 1, 1, 0.0, 1.0, B, B, B, B, B), NULL_FRAME),
        ("rt_frame_pick_rect", (None, 3, 3, 1, 1, 0.0, 1.0, None, None, None, None, None), NULL_FRAME),
        # frame_schedule.cpp
        ("rt_generate_rays", (None,), NULL_FRAME),
        ("rt_intersect", (None, 0), NULL_FRAME),
        ("rt_intersect", (None, 99), NULL_FRAME),
        ("rt_shade_miss", (None, 0), NULL_FRAME),
        ("rt_clear_outgoing_counter", (None, 0), NULL_FRAME),
        ("rt_clear_shadow_counter", (None,), NULL_FRAME),
        ("rt_shade", (None, 0), NULL_FRAME),
        ("rt_shade", (None, 99), NULL_FRAME),
        ("rt_intersect_shadow", (None, 0), NULL_FRAME),
        ("rt_intersect_shadow", (None, 99), NULL_FRAME),
        ("rt_accumulate_direct", (None,), NULL_FRAME),
        ("rt_advance_sample", (None,), NULL_FRAME),
        ("rt_integrate", (None, 1), NULL_FRAME),
        ("rt_integrate", (None, 0), NULL_FRAME),
    ]
    moved = {"rt_ctx_create", "rt_finish", "rt_ctx_device_info", "rt_ctx_set_option", "rt_host_register", "rt_host_unregister", "rt_upload_blue_noise_tables",
             "rt_buffer_create", "rt_buffer_write", "rt_buffer_read", "rt_buffer_copy", "rt_frame_create", "rt_set_option", "rt_set_camera", "rt_reset",
             "rt_frame_reserve_samples", "rt_frame_pick", "rt_frame_pick_all", "rt_frame_pick_rect", "rt_generate_rays", "rt_intersect", "rt_shade_miss",
             "rt_clear_outgoing_counter", "rt_clear_shadow_counter", "rt_shade", "rt_intersect_shadow", "rt_accumulate_direct", "rt_advance_sample", "rt_integrate"}
    assert {name for name, _, _ in table} == moved and moved <= set(capi.EXPORTS)
    for name, args, text in table:
        rc = getattr(lib, name)(*args)
        said = lib.rt_last_error(None).decode()
        assert rc == 1 and said == name + ": " + text, (name, args, rc, said)
    assert out.value == 0x5A5A                  # refused before `*out = nullptr`
    # the moved entries that answer a NULL handle without a message
    assert lib.rt_ctx_destroy(None) == 0 and lib.rt_buffer_destroy(None) == 0 and lib.rt_frame_destroy(None) == 0
    assert lib.rt_ctx_stream(None) is None and lib.rt_buffer_device_ptr(None) is None and lib.rt_buffer_size(None) == 0
    assert lib.rt_frame_local_rows(None) == 0 and lib.rt_frame_global_row(None, 5) == 0
    assert lib.rt_last_error(None).decode() == table[-1][0] + ": " + table[-1][2]
    assert not scratch.any()                    # nothing was written through a refused call's arguments

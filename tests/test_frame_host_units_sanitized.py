"""The host-only units behind the context and the frames -- context.cpp, frame_layout.cpp, frame_schedule.cpp, frame_fold_hooks.cpp -- under AddressSanitizer +
UBSan, as a stand-alone program (tests/native/frame_host_units.cpp): g++ compiles the four units as plain C++ against stubs of what rt_hip.hip, the scene's and
the queries' units give them, the HIP runtime is linked and never asked for a device.  The program has the entries refuse on their arguments alone as
tests/test_schedule_entry_messages.py pins them, and runs the pure planning functions (log_is_compact, bytes_per_path, chunk_plan, chunk_for, slot_cap,
ahead_depth, ahead_wanted, frame_kernel_eligible) on hand-made frames -- one pixel, no pixel, chunks under RT_OPT_PATH_STATE_LIMIT_MB, max_bounces 0 and 62 --
against the values the same functions gave before they left rt_hip.hip."""
import os
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = "/opt/rocm"


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h"))
                    or not os.path.exists(os.path.join(ROCM, "lib", "libamdhip64.so")), reason="no g++ or no HIP runtime")
def test_the_context_and_frame_units_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "frame_host_units")
    csrc = os.path.join(ROOT, "raytracing_amd", "csrc")
    units = [os.path.join(csrc, u) for u in ("context.cpp", "frame_layout.cpp", "frame_schedule.cpp", "frame_fold_hooks.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "native", "frame_host_units.cpp")] + units + \
          ["-o", exe, "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ok: 30 refusals as pinned, 14700 planning values equal the parent's" in run.stdout, (run.stdout[-1000:], run.stderr[-3000:])

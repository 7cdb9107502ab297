"""movba_pose_opt_batch without a GPU: its host side (mov-slam_amd/csrc/pose_opt.cpp) with the rest of libmovba's host
code, against the stand-in runtime and fake device of tests/hipstub (fake_pose_batch.cpp: the two batched launch wrappers),
under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer; and the C-ABI's argument checks through the
real libmovba.so."""
import os
import subprocess

from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "hipstub")


def _build_and_run(target, env):
    subprocess.check_call(["make", "-C", STUB, "-s", target])
    return subprocess.run([os.path.join(STUB, target)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)


def test_pose_batch_host_side_under_address_and_undefined_behaviour_sanitizers():
    """Mixed frame sizes (beyond the LDS limit, fewer than 4 matches, batches that grow the staging buffer and the pose arena),
    invalid calls, a batch between an LBA upload and its run, two threads on two handles: the host's layout of every frame,
    its packing and unpacking overrun nothing, and each frame's results come back to its own arrays."""
    p = _build_and_run("pose_batch_asan", {"ASAN_OPTIONS": "detect_leaks=0 abort_on_error=0 exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[:4000]
    assert p.returncode == 0 and p.stdout.strip().endswith("POSE-BATCH OK"), p.stderr[-2000:]


def test_pose_batch_host_side_is_race_free():
    """The same driver under ThreadSanitizer: the staging buffer a batch reuses is handed over by the stream and the upload's
    copy event, and two handles on two threads share nothing unordered."""
    p = _build_and_run("pose_batch_tsan", {"TSAN_OPTIONS": "halt_on_error=0 exitcode=66"})
    assert "WARNING: ThreadSanitizer" not in p.stderr, p.stderr[:4000]
    assert p.returncode == 0 and p.stdout.strip().endswith("POSE-BATCH OK"), p.stderr[-2000:]


def test_pose_batch_refuses_a_null_handle_without_a_device(built_lib):
    L = built_lib.lib()
    d = (built_lib.PoseDesc * 1)()
    r = (built_lib.PoseResult * 1)()
    assert L.movba_pose_opt_batch(None, d, r, 1) == -1
    assert L.movba_pose_opt_batch(None, None, None, 0) == -1

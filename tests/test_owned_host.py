"""The owning types of the C-ABI implementation (gpusimilarity_amd/csrc/capi_owned.h) on the host, without a GPU.

tests/cpp/owned_check.cpp includes that header alone and IS the HIP runtime it calls: counting allocators for device
blocks, pinned blocks, events and streams that fail the n-th call on request and end the run on a free of anything not
live.  It checks the two grow operations (a size already held: no allocator call; a successful grow: the old block freed
once, the new size reported; a failed free-first grow: empty, size 0; a failed allocate-then-swap grow: pointer and size
as they were), moves (the source is empty and frees nothing), that everything allocated is freed exactly once, and one
scenario per allocation-failure defect the hand-written grow code had: a result block after a failed regrow and a smaller
request, candidate segments beside a capacity counter, many buffers behind one first-use guard, the pair buffer, two ensure functions
that share a buffer and its capacity.

The scenarios rebuild the SHAPE of each call site around the buffer type; they do not call ensure_result_capacity,
grow_batch_segments and the others themselves (those need a device), so the order in which the real functions assign their
capacity counters is checked by reading them, not by this test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "owned_check")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "owned_check.cpp")
    deps = [src, os.path.join(ROOT, "gpusimilarity_amd", "csrc", "capi_owned.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                               "-o", BIN, src])  # (no -l: the checker defines the HIP entry points the header calls)
    return BIN


def test_owned_types_release_exactly_once_and_stay_consistent_when_an_allocation_fails(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stdout + r.stderr


def test_the_checker_links_no_hip_runtime(checker):
    """The allocators under test are the checker's own: the binary must not have picked up the real runtime."""
    needed = subprocess.run(["readelf", "-d", checker], capture_output=True, text=True, timeout=60).stdout
    assert "NEEDED" in needed and "amdhip" not in needed and "hiprtc" not in needed, needed

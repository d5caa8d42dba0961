"""The streamed pipeline's slot board (vcf2prot_amd/csrc/pipe_slots.hpp) on the CPU: tests/pipe_slots_stress.cpp plays the protocol --
8 submitters, a runner, a reserving thread, 2 slots -- as a program of its own, once plain and once under ThreadSanitizer.  A hand-off
without happens-before or a lock-order inversion is a ThreadSanitizer report; a slot with two owners, or a FREE slot with work left on
its streams, fails one of the program's checks; a deadlock is the timeout."""
import os
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "vcf2prot_amd", "csrc")
CXX = ["g++", "-std=c++17", "-O1", "-g", "-pthread"]


def _tsan_works(tmp_path):
    """can this machine build and start a ThreadSanitizer program at all (a one-line one)?"""
    src = tmp_path / "one_line.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = tmp_path / "one_line"
    try:
        if subprocess.run(CXX + ["-fsanitize=thread", str(src), "-o", str(exe)], capture_output=True, timeout=120).returncode != 0:
            return False
        return subprocess.run([str(exe)], capture_output=True, timeout=120).returncode == 0
    except (OSError, subprocess.TimeoutExpired):
        return False


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "tsan"])
def test_slot_protocol_under_threads(tmp_path, sanitize):
    if sanitize and not _tsan_works(tmp_path):
        pytest.skip("g++ -fsanitize=thread does not build or start a one-line program here")
    exe = tmp_path / "pipe_slots_stress"
    cmd = CXX + (["-fsanitize=thread"] if sanitize else []) + ["-I", CSRC, os.path.join(TESTS, "pipe_slots_stress.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    try:
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the slot protocol deadlocked (no end within 120 s)")
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("ok:"), r.stdout

"""CPU: the host machinery every lockstep entry shares (stereo-vision_amd/csrc/batch_rec.h, batch_rec.cpp) over a stub
device layer -- tests/cxx/lockstep_check.cpp links no HIP runtime.  The recorder: one launch per call position with the
jobs in object order, grid and LDS the maxima, 256-aligned tables that a second phase does not overwrite before
synced(), an arena that grows without losing a job.  run_recorded: its success path for K = 1, 2, 5; the fallback for a
call-sequence mismatch (another function, another job size), which no product input reaches; what an error of an
enqueue, the flush or the wait leaves behind, and a clean phase after each.  check_batch: null objects, the same object
twice, one object, mixed devices."""
import os
import subprocess

import helpers as H

CXX = os.path.join(H.ROOT, "tests", "cxx")


def run(target):
    subprocess.check_call(["make", "-C", CXX, target], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(CXX, target)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lockstep_check: 0 failed checks" in r.stdout, r.stdout


def test_lockstep_core():
    run("lockstep_check")


def test_lockstep_core_under_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined"""
    run("lockstep_check_san")

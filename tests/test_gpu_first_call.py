"""First-call latency.  A JVM pays a context's first call once per context: the runtime loads a
kernel file's code object at the first launch of any kernel in it, and the scan's buffers are allocated at first use.
rsh_ctx_create now does both (capi.cpp ctx_warm), so the first scan on a fresh context costs what the next ones do.

The check runs in a fresh process (java-rsync_amd/tools/first_call.py): in this one, other tests have loaded the code
objects already."""
import json
import os
import statistics
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_first_step_on_a_fresh_context_costs_what_the_next_ones_do():
    """rsh_ctx_create in a new process, then BASELINE config 5 as written (16 GiB, B = 131072, dl = 4, every other
    block of the basis replaced; the device-resident Generator + Sender step) five times.  Before ctx_warm the first
    step took 7.5-11.1 ms against ~3.8 (code objects loaded and copy paths set up on first use, buffers allocated).
    Now the library's own part of the step -- everything but the Generator's K1, timed by its dispatch events -- is
    within 50 % + 0.1 ms of the later steps' median (round 6, profiles/r6/first_calls.json: 0.72-0.85 ms against
    0.55-0.64 -- the remaining ~0.15 ms is spread over the prep wait, the lead check and the first probe, tens of
    microseconds each, after ctx_warm and warm_calls ran every path once), and the whole step within 25 %: the first
    K1 itself runs a few % slower, the chip's clocks ramping under the first heavy kernel after idle."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "java-rsync_amd", "tools", "first_call.py"), "--only", "5",
                        "--reps", "5"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    steps, k1 = out["config5_half_step_ms"], out["config5_generator_k1_ms"]
    own = [s - k for s, k in zip(steps, k1)]
    assert min(k1) > 0, out
    assert own[0] <= 1.5 * statistics.median(own[1:]) + 0.1, out
    assert steps[0] <= 1.25 * statistics.median(steps[1:]), out


def test_segment_scan_first_and_after_trim():
    """the segment path.  In a fresh process, config 4's shard (128 x 128 MiB, 50%-modified bases)
    through the batched Generator + Sender five times, then rsh_ctx_trim and once more.  rsh_ctx_create pre-sizes the
    batched scan's state for that shard (option batch_warm; its first call allocated ~11 ms of pinned buffers before)
    and trim keeps it; rsh_ctx_create also runs one small batched pass (warm_calls) and the scratch its chain walk
    needs.  The scan after the trim costs what the others do (1.15x + 0.1 ms of the later scans' median; the whole call
    is the library's); the first one within 1.35x + 0.1 ms (round 6 boxes: 1.97 / 2.03 ms against 1.62 / 1.58, from 6.9
    ms before).  From host memory (rsh_block_sums_batch + rsh_match_scan_batch, the JVM's calls, ~0.31 s each) the
    first segment and the one after trim are within 1.25x of the others."""
    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "java-rsync_amd", "tools", "first_call.py"), "--only", "4",
                            "--trim", *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    out = run("--reps", "5")
    scan = out["config4_half_scan_ms"]
    med = statistics.median(scan[1:5])
    assert scan[0] <= 1.35 * med + 0.1, out
    assert scan[5] <= 1.15 * med + 0.1, out  # after rsh_ctx_trim
    out = run("--reps", "3", "--host")
    for k in ("config4_host_generator_ms", "config4_host_scan_ms"):
        t = out[k]
        med = statistics.median(t[1:3])
        assert t[0] <= 1.25 * med and t[3] <= 1.25 * med, out


def test_batch_warm_presizes_at_context_creation():
    """Option batch_warm (default 128 files): rsh_ctx_create holds the batched scan's state for config 4's shard
    (~0.25 GiB of HBM, ~50 MiB pinned); batch_warm = 0 leaves it to the first segment call.  Each context is the first
    of a fresh process (the runtime's memory pool would let a second context reuse what a first one freed)."""
    code = ("import sys, torch; sys.path.insert(0, 'java-rsync_amd'); import rsync_hip as R; torch.cuda.init(); "
            "R.set_option('batch_warm', int(sys.argv[1])); torch.cuda.synchronize(); "
            "f0 = torch.cuda.mem_get_info(0)[0]; c = R.Context(0); print(f0 - torch.cuda.mem_get_info(0)[0]); c.close()")
    free = []
    for warm in (0, 128):
        r = subprocess.run([sys.executable, "-c", code, str(warm)], capture_output=True, text=True, timeout=300,
                           cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        free.append(int(r.stdout.strip().splitlines()[-1]))
    assert free[1] - free[0] >= 150 << 20, free


def test_first_segment_scan_allocates_nothing():
    """The batched scan sizes its buffers in one place (batch.cpp SegmentLayout), which rsh_ctx_create's warm-up calls
    with config 4's shard: a fresh context's first segment scan within that shape -- four of its 128 MiB files here --
    allocates nothing.  first_call.py --trace-allocs sets scan_trace = 1 around that scan alone, which prints one line
    per device or pinned allocation.  The control: the same run with the warm-up off (--no-warm: batch_warm = 0) must
    print such lines, so the empty list is neither tracing left off nor a changed line format."""
    import re

    def allocs(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "java-rsync_amd", "tools", "first_call.py"), "--only", "4",
                            "--files", "4", "--reps", "1", "--trace", "--trace-allocs", *extra], capture_output=True,
                           text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "[rsh-batch] 4 files: enqueued" in r.stderr, r.stderr[-3000:]  # the scan was traced
        return [ln for ln in r.stderr.splitlines() if re.match(r"\[rsh\] (dev_alloc|pin_alloc)\b", ln)]
    assert allocs("--no-warm") != []
    assert allocs() == []

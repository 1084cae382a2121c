"""CPU: the launch trace of the RDN plan.  bin_amd/csrc/binhip_plan.hip is host code only: it issues every launch of a
sub-network, about 67 forward and 200 backward, and a swapped offset in it would otherwise show on a GPU alone.  Here the real
source is compiled host-only and linked with recording stand-ins for everything it calls (tests/plan_trace/stubs.hip) and a
driver that walks the smallest cases reaching each of its branches with fake, distinct pointers (tests/plan_trace/driver.cpp);
the program prints one line per call with every argument.  tests/golden/plan_trace.txt is that text as recorded from the plan
BEFORE it was given named tensors and layer calls: whoever changes the plan's host logic on purpose records it again from the
commit before theirs and reviews the diff; it is never regenerated from the code under test."""
import difflib
import os
import subprocess

from conftest import REPO

HERE = os.path.join(REPO, "tests", "plan_trace")
CSRC = os.path.join(REPO, "bin_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "plan_trace.txt")


def build_recorder(out_dir, plan_source=os.path.join(CSRC, "binhip_plan.hip"), extra=()):
    """Compile `plan_source` host-only, link it with the stand-ins and the driver (no HIP runtime, no GPU); returns the program.
    `plan_source`: another commit's plan, to record the golden text from; `extra`: flags for every compile and the link, such as
    -fsanitize=address,undefined (the program has its own main, so that run needs nothing preloaded)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    host = [hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-fPIC", "-I" + CSRC, *extra]
    jobs = [(host + ["-c", plan_source], "plan.o"), (host + ["-c", os.path.join(HERE, "stubs.hip")], "stubs.o"),
            ([hipcc, "-x", "c++", "-std=c++17", "-fPIC", "-I" + os.path.join(REPO, "include"), *extra, "-c", os.path.join(HERE, "driver.cpp")],
             "driver.o")]
    objs = [os.path.join(out_dir, o) for _, o in jobs]
    procs = [subprocess.Popen(cmd + ["-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for (cmd, _), obj in zip(jobs, objs)]
    for p in procs:
        log = p.communicate()[0]
        assert p.returncode == 0, log[-4000:]
    exe = os.path.join(out_dir, "plan_trace")
    subprocess.run([hipcc, "-no-hip-rt", *extra, "-o", exe] + objs, check=True)
    return exe


def test_plan_issues_the_recorded_launch_sequence(tmp_path):
    exe = build_recorder(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(GOLDEN) as f:
        want = f.read()
    if r.stdout != want:
        diff = list(difflib.unified_diff(want.splitlines(), r.stdout.splitlines(), "tests/golden/plan_trace.txt", "this tree", n=1, lineterm=""))
        print("\n".join(diff[:400]))
        raise AssertionError(f"the plan's launch trace differs from the recorded one ({len(diff)} diff lines, the first 400 above)")
    # the refusals: a return code and not one launch ("[s..." lines) — the fused-UPNet slots included, which are looked at with
    # the other pointers, before the gradient scale is queued
    cases = want.split("\n== ")
    refusals = [c for c in cases if c.startswith("i ")]
    assert len(refusals) == 10
    for c in refusals:
        launches = [ln for ln in c.splitlines() if ln.startswith("[s")]
        assert len(launches) == 0, c
        assert " rc-" in c

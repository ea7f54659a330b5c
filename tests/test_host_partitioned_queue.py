"""PartitionedRedisQueueingTokenBucketRateLimiter through the C++ host classes
(tests/host/partitioned_queue_test.cpp).  CPU: option validation (QueueingClasses on the
non-partitioned and the approximate limiters, the inherited Classes, bad classes).  GPU: two
classes with periods of 1 s and 30 s behind ClassOf, one replenish timer per period whose tick
completes the queued waits of its own classes alone (TickTimer and OnRefresh, no waiting on wall
time), TryReplenish over both, eviction and failure under each class's QueueLimit, a canceled
wait, GetAvailablePermits of an unseen name, an out-of-range ClassOf (it needs a constructed
limiter, so it runs here), GetStatistics, ReclaimExpired and a reused key's class.  The program
is built by __graft_entry__.build() (relative rpaths, so the binary built on the build machine
runs on the GPU machine)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "distributedratelimiting.redis_amd")
SRC = os.path.join(ROOT, "tests", "host", "partitioned_queue_test.cpp")
BIN = os.path.join(ROOT, "tests", "host", "partitioned_queue_test")


def build_partitioned_queue_test() -> str:
    """Compile the test program against libtbe_host.so and libtbe.so."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tbe_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build_host()
    deps = [SRC, mod.HOST_LIB, os.path.join(PKG, "host", "rate_limiting.hpp"), os.path.join(ROOT, "include", "tbe.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(PKG, "host"), "-o", BIN + ".tmp", SRC,
           "-L", PKG, "-ltbe_host", "-ltbe", "-L", "/opt/rocm/lib",
           "-Wl,-rpath,$ORIGIN/../../distributedratelimiting.redis_amd"]
    subprocess.run(cmd, check=True)
    os.replace(BIN + ".tmp", BIN)
    return BIN


def _run(exe: str, mode: str) -> str:
    p = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failed" in p.stdout
    return p.stdout


def test_host_partitioned_queue_cpu():
    out = _run(build_partitioned_queue_test(), "cpu")
    assert "10 checks passed" in out


@pytest.mark.gpu
def test_host_partitioned_queue_gpu(gpu):
    if not os.path.exists(BIN):
        pytest.fail("tests/host/partitioned_queue_test is not built (run __graft_entry__.build())")
    _run(BIN, "gpu")

"""Approximate limit classes on PartitionedRedisApproximateTokenBucketRateLimiter through the
C++ host classes (tests/host/approx_classes_test.cpp).  CPU: option validation.  GPU: two
classes with different periods and QueueLimits behind ClassOf, the first request of a new name
decided under its class, an out-of-range ClassOf, GetAvailablePermits of an unseen name, the
per-period timers' ticks (TickTimer and OnRefresh, no waiting on wall time), TryReplenish over
both classes, a reused key that takes its new name's class.  The program is built by
__graft_entry__.build() (relative rpaths, so the binary built on the build machine runs on
the GPU machine)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "distributedratelimiting.redis_amd")
SRC = os.path.join(ROOT, "tests", "host", "approx_classes_test.cpp")
BIN = os.path.join(ROOT, "tests", "host", "approx_classes_test")


def build_approx_classes_test() -> str:
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


def test_host_approx_classes_cpu():
    out = _run(build_approx_classes_test(), "cpu")
    assert "7 checks passed" in out


@pytest.mark.gpu
def test_host_approx_classes_gpu(gpu):
    if not os.path.exists(BIN):
        pytest.fail("tests/host/approx_classes_test is not built (run __graft_entry__.build())")
    _run(BIN, "gpu")

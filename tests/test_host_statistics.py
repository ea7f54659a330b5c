"""GetStatistics() through the C++ host classes (tests/host/statistics_test.cpp):
RateLimiterStatistics and Options.TrackStatistics.  CPU: the struct's and the option's
defaults, and the base classes' GetStatistics returning nullopt.  GPU, on an injected clock:
hand-checked grant / deny sequences on all five limiters; a queued wait that is drained counts
successful, one evicted counts failed, one canceled counts nothing; an unseen name reads zeros
and takes no key (PartitionLimit 1); a key reclaimed and reused reads zeros.  The program is
built by __graft_entry__.build() (relative rpaths, so the binary built on the build machine
runs on the GPU machine)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "distributedratelimiting.redis_amd")
SRC = os.path.join(ROOT, "tests", "host", "statistics_test.cpp")
BIN = os.path.join(ROOT, "tests", "host", "statistics_test")


def build_statistics_test() -> str:
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


def test_host_statistics_cpu():
    out = _run(build_statistics_test(), "cpu")
    assert "6 checks passed" in out


@pytest.mark.gpu
def test_host_statistics_gpu(gpu):
    if not os.path.exists(BIN):
        pytest.fail("tests/host/statistics_test is not built (run __graft_entry__.build())")
    out = _run(BIN, "gpu")
    assert "62 checks passed" in out

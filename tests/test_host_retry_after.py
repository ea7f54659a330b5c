"""RetryAfter of the approximate limiter's failed leases through the C++ host classes
(tests/host/retry_after_test.cpp): each failed lease carries the value decided at its own
position in the micro-batch, and a denial-heavy micro-batch makes no tbe_approx_query call.
The program is built by __graft_entry__.build() (relative rpaths, so the binary built on
the build machine runs on the GPU machine)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "distributedratelimiting.redis_amd")
SRC = os.path.join(ROOT, "tests", "host", "retry_after_test.cpp")
BIN = os.path.join(ROOT, "tests", "host", "retry_after_test")


def build_retry_after_test() -> str:
    """Compile the test program against libtbe_host.so and libtbe.so.  -rdynamic: the
    program's own tbe_approx_query must be visible to the dynamic linker, which then binds
    libtbe_host.so's calls to it (the call counter)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tbe_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build_host()
    deps = [SRC, mod.HOST_LIB, os.path.join(PKG, "host", "rate_limiting.hpp"), os.path.join(ROOT, "include", "tbe.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-rdynamic", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(PKG, "host"), "-o", BIN + ".tmp", SRC,
           "-L", PKG, "-ltbe_host", "-ltbe", "-ldl", "-L", "/opt/rocm/lib",
           "-Wl,-rpath,$ORIGIN/../../distributedratelimiting.redis_amd"]
    subprocess.run(cmd, check=True)
    os.replace(BIN + ".tmp", BIN)
    return BIN


def test_program_counts_the_host_library_queries():
    """No GPU: the built program exports tbe_approx_query, so libtbe_host.so's calls bind to
    its counting wrapper."""
    exe = build_retry_after_test()
    out = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "tbe_approx_query" for line in out.splitlines() if line.strip())


@pytest.mark.gpu
def test_host_retry_after_gpu(gpu):
    if not os.path.exists(BIN):
        pytest.fail("tests/host/retry_after_test is not built (run __graft_entry__.build())")
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failed" in p.stdout
    assert "0 tbe_approx_query calls" in p.stdout

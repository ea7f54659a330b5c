"""The approximate kind's RetryAfter arithmetic (csrc/tbe_retry.hpp: the int32 wrap of the
deficit, the two f64 multiplies, the truncation and the overflow edge at 2^63) on the host:
tests/host/retry_ticks_test.cpp includes the header the kernels compile and compares it with
a plain statement of A:390-395.  A stand-alone program built with AddressSanitizer and
UBSan.  No GPU and no engine library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "retry_ticks_test.cpp")
HDR = os.path.join(ROOT, "distributedratelimiting.redis_amd", "csrc", "tbe_retry.hpp")
BIN = os.path.join(ROOT, "tests", "host", "retry_ticks_test")


def build_retry_ticks_test() -> str:
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in (SRC, HDR)):
        return BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", BIN + ".tmp", SRC], check=True)
    os.replace(BIN + ".tmp", BIN)
    return BIN


def test_retry_ticks_match_plain_formula():
    p = subprocess.run([build_retry_ticks_test()], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failed" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr

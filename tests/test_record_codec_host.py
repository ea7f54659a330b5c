"""The last partition pass's per-batch record codec against the generic packer, on the host:
tests/host/codec_test.cpp includes csrc/tbe_codec.hpp and compares the two over every format
(equal packed bits, equal decoded fields, and that a time inside a narrow record's window is
always inside the fold record's).  No GPU and no engine library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "codec_test.cpp")
HDR = os.path.join(ROOT, "distributedratelimiting.redis_amd", "csrc", "tbe_codec.hpp")
BIN = os.path.join(ROOT, "tests", "host", "codec_test")


def build_codec_test() -> str:
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in (SRC, HDR)):
        return BIN
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", BIN + ".tmp", SRC], check=True)
    os.replace(BIN + ".tmp", BIN)
    return BIN


def test_codec_matches_generic_packer():
    p = subprocess.run([build_codec_test()], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failed" in p.stdout and "11008 formats" in p.stdout

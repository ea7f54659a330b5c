"""The masked replenish ticks of the queueing kind (tbe_refresh_classes,
tbe_refresh_classes_device, tbe_wait_batch_tick_classes_device in include/tbe.h): what is
decidable without a device.  Every other TBE_EINVAL case -- a NULL mask, a bit at or above the
class count, another kind of engine, ts_us < 0, a NULL n_granted or d_count -- is checked
behind a NULL-engine test, so it needs a live engine, which needs the device:
tests/test_gpu_queue_tick_mask.py::test_refusals."""
import os
import shutil
import subprocess
from ctypes import byref, c_uint64

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tbe_refresh_classes", "tbe_refresh_classes_device", "tbe_wait_batch_tick_classes_device")


@pytest.fixture(scope="module")
def capi(engine_lib):
    from distributedratelimiting.redis_amd import _capi
    return _capi.load(), _capi


def test_exported_and_listed(capi):
    lib, c = capi
    for name in NEW:
        assert name in c.EXPORTED and hasattr(lib, name), name


def test_null_engine(capi):
    lib, c = capi
    m = c.class_mask([0])
    n = c_uint64()
    assert lib.tbe_refresh_classes(None, 0, m, byref(n)) == c.TBE_EINVAL
    assert lib.tbe_refresh_classes(None, 0, None, None) == c.TBE_EINVAL
    assert lib.tbe_refresh_classes_device(None, 0, m, None, None, None, 0, None, None) == c.TBE_EINVAL
    assert lib.tbe_wait_batch_tick_classes_device(None, None, None, None, 0, 0, 1, None, None, 0, m, None, None,
                                                  None, 0, None, None) == c.TBE_EINVAL


def test_declarations_compile_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    decl = tmp_path / "decl.c"   # compiled only: the declarations have these C types
    decl.write_text('#include "tbe.h"\n'
                    'tbe_status (*a)(tbe_engine *, int64_t, const uint64_t *, uint64_t *) = tbe_refresh_classes;\n'
                    'tbe_status (*b)(tbe_engine *, int64_t, const uint64_t *, uint64_t *, int64_t *, int32_t *,\n'
                    '                uint64_t, uint32_t *, void *) = tbe_refresh_classes_device;\n'
                    'tbe_status (*c)(tbe_engine *, const uint64_t *, const int32_t *, const int64_t *, uint64_t,\n'
                    '                int64_t, int32_t, uint8_t *, int32_t *, int64_t, const uint64_t *, uint64_t *,\n'
                    '                int64_t *, int32_t *, uint64_t, uint32_t *, void *) =\n'
                    '    tbe_wait_batch_tick_classes_device;\n')
    subprocess.run([cc, "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "decl.o"), str(decl)],
                   check=True)


def test_python_keyword_builds_the_mask():
    """`classes` goes through _capi.class_mask: a class number outside [0, 256) never reaches C."""
    import inspect

    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine as Q
    for f in (Q.refresh, Q.refresh_device, Q.wait_batch_tick_device):
        p = inspect.signature(f).parameters
        assert "classes" in p and p["classes"].default is None, f.__name__

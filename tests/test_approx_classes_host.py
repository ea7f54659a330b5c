"""tbe_create_approx_classes and the class mask of the tbe_approx_*_classes calls
(include/tbe.h): every TBE_EINVAL case is decided before the device is touched, so the checks
run without a GPU."""
import ctypes
import os
import shutil
import subprocess
from ctypes import byref, c_uint64, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = [(5, 2, 20_000_000, 3, 1), (16383, 1000, 10_000_000, 0, 0), (3, 1, 5_000_000, 16, 1)]


@pytest.fixture(scope="module")
def capi(engine_lib):
    from distributedratelimiting.redis_amd import _capi
    return _capi.load(), _capi


def _cfg(c, kind=2, zero_wait_slots=4):
    return c.make_config(64, 20, 10, 10_000_000, kind=kind, queue_limit=8, zero_wait_slots=zero_wait_slots)


def _create(lib, c, cfg, classes, n_extra=None, null_extra=False):
    extra = (c.TbeQueueClass * max(1, len(classes)))(*[c.TbeQueueClass(*q) for q in classes])
    h = c_void_p()
    st = lib.tbe_create_approx_classes(byref(cfg), None if null_extra else extra,
                                       len(classes) if n_extra is None else n_extra, byref(h))
    assert not h.value, "a refused create hands out no engine"
    return st


@pytest.mark.parametrize("kind", [0, 1, 7])
def test_other_kinds(capi, kind):
    lib, c = capi
    assert _create(lib, c, _cfg(c, kind, 0), GOOD) == c.TBE_EINVAL


def test_null_extra(capi):
    lib, c = capi
    assert _create(lib, c, _cfg(c), [], n_extra=2, null_extra=True) == c.TBE_EINVAL


def test_too_many_classes(capi):
    lib, c = capi
    assert _create(lib, c, _cfg(c), [GOOD[0]] * 256) == c.TBE_EINVAL
    assert "256" in lib.tbe_last_error(None).decode()


@pytest.mark.parametrize("bad", [(0, 1, 10_000_000, 3, 0), (-3, 1, 10_000_000, 3, 0), (5, 0, 10_000_000, 3, 0),
                                 (5, -1, 10_000_000, 3, 0), (5, 1, 0, 3, 0), (5, 1, -7, 3, 0),
                                 (5, 1, 10_000_000, -1, 0), (5, 1, 10_000_000, 65536, 0),
                                 (5, 1, 10_000_000, 3, 2), (2**30 - 1, 1, 10_000_000, 3, 0),
                                 # the ring-length bound: max(1, QueueLimit) + zero_wait_slots <= 65535
                                 (5, 1, 10_000_000, 65532, 0)])
@pytest.mark.parametrize("at", [0, 2])
def test_bad_class(capi, bad, at):
    lib, c = capi
    classes = list(GOOD)
    classes[at] = bad
    assert _create(lib, c, _cfg(c), classes) == c.TBE_EINVAL


def test_ring_length_bound_counts_the_configs_zero_wait_slots(capi):
    """QueueLimit 65532 is refused with 4 zero-wait slots (65536 ring entries) and is a
    valid class with 3 (65535): only the bound is checked here, before the device."""
    lib, c = capi
    assert _create(lib, c, _cfg(c, zero_wait_slots=4), [(5, 1, 10_000_000, 65532, 0)]) == c.TBE_EINVAL
    assert "65535" in lib.tbe_last_error(None).decode()
    assert _create(lib, c, _cfg(c, zero_wait_slots=4), [(5, 1, 10_000_000, 65531, 2)]) == c.TBE_EINVAL   # the order
    assert "QueueProcessingOrder" in lib.tbe_last_error(None).decode()


def test_null_config_and_out(capi):
    lib, c = capi
    extra = (c.TbeQueueClass * 1)(c.TbeQueueClass(*GOOD[0]))
    h = c_void_p()
    assert lib.tbe_create_approx_classes(None, extra, 1, byref(h)) == c.TBE_EINVAL
    cfg = _cfg(c)
    assert lib.tbe_create_approx_classes(byref(cfg), extra, 1, None) == c.TBE_EINVAL


def test_class_struct_layout(capi, tmp_path):
    """An approximate class is tbe_queue_class: sizeof and field offsets of the ctypes struct
    against the C compiler's view of tbe.h, and the new entry points' declarations compile as C."""
    _, c = capi
    q = c.TbeQueueClass
    assert ctypes.sizeof(q) == 24
    got = [q.token_limit.offset, q.tokens_per_period.offset, q.replenishment_period_ticks.offset,
           q.queue_limit.offset, q.queue_order.offset]
    assert got == [0, 4, 8, 16, 20]
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    decl = tmp_path / "decl.c"   # compiled only: the declarations have these C types
    decl.write_text('#include "tbe.h"\n'
                    'tbe_status (*create)(const tbe_config *, const tbe_queue_class *, uint32_t, tbe_engine **) =\n'
                    '    tbe_create_approx_classes;\n'
                    'tbe_status (*classes)(const tbe_engine *, tbe_queue_class *, uint32_t, uint32_t *) =\n'
                    '    tbe_approx_classes;\n'
                    'tbe_status (*refresh)(tbe_engine *, int64_t, const uint64_t *, uint64_t *) =\n'
                    '    tbe_approx_refresh_classes;\n')
    subprocess.run([cc, "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "decl.o"), str(decl)],
                   check=True)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tbe.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tbe_queue_class),\n'
                   '  offsetof(tbe_queue_class, token_limit), offsetof(tbe_queue_class, tokens_per_period),\n'
                   '  offsetof(tbe_queue_class, replenishment_period_ticks), offsetof(tbe_queue_class, queue_limit),\n'
                   '  offsetof(tbe_queue_class, queue_order)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [24] + got


def test_class_mask_helper(capi):
    _, c = capi
    m = c.class_mask([0, 3, 64, 255])
    assert list(m) == [0b1001, 1, 0, 1 << 63]
    assert list(c.class_mask([])) == [0, 0, 0, 0]
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            c.class_mask([bad])


def test_masked_calls_refuse_null_engine(capi):
    """What is decidable of the masked calls without an engine: a NULL engine is TBE_EINVAL
    (the check of a bit at or above the class count needs an engine, which needs the device:
    tests/test_gpu_approx_classes.py::test_refusals_layout_and_recreate)."""
    lib, c = capi
    m = c.class_mask([0])
    n = c_uint64()
    assert lib.tbe_approx_collect_classes(None, None, m, None) == c.TBE_EINVAL
    assert lib.tbe_approx_sync_classes(None, None, 1, 0, 0, 0, m, byref(n)) == c.TBE_EINVAL
    assert lib.tbe_approx_sync_classes_stream(None, None, 1, 0, 0, 0, m, None, byref(n)) == c.TBE_EINVAL
    assert lib.tbe_approx_refresh_classes(None, 0, m, byref(n)) == c.TBE_EINVAL
    assert lib.tbe_approx_classes(None, None, 0, None) == c.TBE_EINVAL

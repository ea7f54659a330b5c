"""tbe_create_queue_classes (include/tbe.h): every TBE_EINVAL case is decided before the
device is touched, so the checks run without a GPU."""
import ctypes
import os
import shutil
import subprocess
from ctypes import byref, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = [(2, 1, 30_000_000, 3, 1), (3, 1, 10_000_000, 0, 0), (6, 10, 10_000_000, 40, 1)]


@pytest.fixture(scope="module")
def capi(engine_lib):
    from distributedratelimiting.redis_amd import _capi
    return _capi.load(), _capi


def _cfg(c, kind=1):
    return c.make_config(64, 4, 1, 10_000_000, kind=kind, queue_limit=16)


def _create(lib, c, cfg, classes, n_extra=None, null_extra=False):
    extra = (c.TbeQueueClass * max(1, len(classes)))(*[c.TbeQueueClass(*q) for q in classes])
    h = c_void_p()
    st = lib.tbe_create_queue_classes(byref(cfg), None if null_extra else extra,
                                      len(classes) if n_extra is None else n_extra, byref(h))
    assert not h.value, "a refused create hands out no engine"
    return st


@pytest.mark.parametrize("kind", [0, 2, 7])
def test_other_kinds(capi, kind):
    lib, c = capi
    assert _create(lib, c, _cfg(c, kind), GOOD) == c.TBE_EINVAL


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
                                 (5, 1, 10_000_000, 3, 2)])
@pytest.mark.parametrize("at", [0, 2])
def test_bad_class(capi, bad, at):
    lib, c = capi
    classes = list(GOOD)
    classes[at] = bad
    assert _create(lib, c, _cfg(c), classes) == c.TBE_EINVAL


def test_null_config_and_out(capi):
    lib, c = capi
    extra = (c.TbeQueueClass * 1)(c.TbeQueueClass(*GOOD[0]))
    h = c_void_p()
    assert lib.tbe_create_queue_classes(None, extra, 1, byref(h)) == c.TBE_EINVAL
    cfg = _cfg(c)
    assert lib.tbe_create_queue_classes(byref(cfg), extra, 1, None) == c.TBE_EINVAL


def test_queue_class_struct_layout(capi, tmp_path):
    """sizeof and field offsets of TbeQueueClass against the C compiler's view of tbe.h."""
    _, c = capi
    q = c.TbeQueueClass
    assert ctypes.sizeof(q) == 24
    got = [q.token_limit.offset, q.tokens_per_period.offset, q.replenishment_period_ticks.offset,
           q.queue_limit.offset, q.queue_order.offset]
    assert got == [0, 4, 8, 16, 20]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
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

"""tbe_create_classes (include/tbe.h): every TBE_EINVAL case is decided before the device
is touched, so the checks run without a GPU."""
import ctypes
from ctypes import byref, c_void_p

import pytest


def _create(lib, capi, cfg, classes, n_extra=None, null_extra=False):
    extra = (capi.TbeClass * max(1, len(classes)))(*[capi.TbeClass(*c) for c in classes])
    h = c_void_p()
    st = lib.tbe_create_classes(byref(cfg), None if null_extra else extra,
                                len(classes) if n_extra is None else n_extra, byref(h))
    assert not h.value, "a refused create hands out no engine"
    return st, lib.tbe_last_error(None).decode()


@pytest.fixture(scope="module")
def capi(engine_lib):
    from distributedratelimiting.redis_amd import _capi
    return _capi.load(), _capi


def test_too_many_classes(capi):
    lib, c = capi
    cfg = c.make_config(64, 10, 1, 10_000_000)
    st, msg = _create(lib, c, cfg, [(3, 1, 30_000_000)] * 256)
    assert st == c.TBE_EINVAL and "256" in msg


def test_null_extra(capi):
    lib, c = capi
    cfg = c.make_config(64, 10, 1, 10_000_000)
    st, _ = _create(lib, c, cfg, [], n_extra=2, null_extra=True)
    assert st == c.TBE_EINVAL


@pytest.mark.parametrize("bad", [(0, 1, 10_000_000), (-3, 1, 10_000_000), (5, 0, 10_000_000),
                                 (5, -1, 10_000_000), (5, 1, 0), (5, 1, -7)])
@pytest.mark.parametrize("at", [0, 2])
def test_bad_class(capi, bad, at):
    lib, c = capi
    cfg = c.make_config(64, 10, 1, 10_000_000)
    classes = [(3, 1, 30_000_000), (100, 50, 1_000_000), (5, 10, 10_000_000)]
    classes[at] = bad
    st, _ = _create(lib, c, cfg, classes)
    assert st == c.TBE_EINVAL


@pytest.mark.parametrize("kind", [1, 2, 7])
def test_other_kinds(capi, kind):
    lib, c = capi
    cfg = c.make_config(64, 10, 1, 10_000_000, kind=kind, queue_limit=4)
    st, _ = _create(lib, c, cfg, [(3, 1, 30_000_000)])
    assert st == c.TBE_EINVAL


def test_null_config_and_out(capi):
    lib, c = capi
    extra = (c.TbeClass * 1)(c.TbeClass(3, 1, 30_000_000))
    h = c_void_p()
    assert lib.tbe_create_classes(None, extra, 1, byref(h)) == c.TBE_EINVAL
    cfg = c.make_config(64, 10, 1, 10_000_000)
    assert lib.tbe_create_classes(byref(cfg), extra, 1, None) == c.TBE_EINVAL


def test_class_struct_layout(capi):
    _, c = capi
    assert ctypes.sizeof(c.TbeClass) == 16
    assert c.TbeClass.replenishment_period_ticks.offset == 8

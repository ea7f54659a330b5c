"""cluster.migrate for text-keyed buckets with the HIP engine: two rank processes share the one
GPU of the test box (each with its own engine and string directory on cuda:0) and exchange
over gloo, as in tests/test_gpu_migrate.py.  Two steps routed by text under the hash
partition, a live change to map B, two steps under B, against the serial reference of
tests/_text_migrate_workers.py, on the host path (numpy, HostStringDirectory, export_state /
import_state) and on the device path (tbe_sdir_route_keys_device, tbe_migrate_out_ids_device,
the StringDirectory's text calls, tbe_import_rows_device), plain and classed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _migrate_workers as M
from tests import _text_migrate_workers as T
from tests import test_dist_gloo as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2


def _run_ranks(out_dir, *args: str, timeout: int = 150):
    """Both ranks as child processes (never exec'd from this GPU-initialised process)."""
    port = G._port()
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_text_migrate_workers.py"),
                               "text_migrate_worker_hip", str(r), str(WORLD), str(port), str(out_dir), *args],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(WORLD)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed ({p.returncode}):\n{o[-4000:]}"
    return [np.load(os.path.join(out_dir, f"tmig_{r}.npz")) for r in range(WORLD)]


@pytest.mark.gpu
@pytest.mark.parametrize("classed", ["plain", "classed"])
@pytest.mark.parametrize("path", ["host", "device"])
def test_text_migrate_two_hip_ranks(gpu, oracle_lib, tmp_path, path, classed):
    res = _run_ranks(tmp_path, path, "ok", classed)
    T.check_text_migrate(res, classed=classed == "classed", device_path=path == "device", moved=516)


@pytest.mark.gpu
def test_text_migrate_after_every_row_lapsed(gpu, oracle_lib, tmp_path):
    """ts_us 6 s after step 1: every row has lapsed, so no row is exchanged while 516 names
    change hands, and steps 2-3 (6 s later too) still match the serial reference."""
    res = _run_ranks(tmp_path, "device", "lapse", "plain")
    assert sum(int(x["sent"]) for x in res) == 0
    T.check_text_migrate(res, shift=M.LAPSE_SHIFT, device_path=True, moved=516)


@pytest.mark.gpu
def test_tight_capacity_is_refused_on_every_rank(gpu, tmp_path):
    T.check_refused(_run_ranks(tmp_path, "device", "tight", "plain"), device_path=True)


@pytest.mark.gpu
def test_tight_arena_is_refused_and_leaves_the_directory_usable(gpu, tmp_path):
    """The rank whose padded key text grows under map B has an arena of exactly what it holds:
    every rank raises, usage(), directory contents and table are unchanged everywhere, and the
    directory is not in TBE_ERANGE (the worker assigns a known name again afterwards)."""
    r, used = T.tight_arena_rank(WORLD, 0)
    assert used > 0
    res = _run_ranks(tmp_path, "device", "arena", "plain")
    T.check_refused(res, device_path=True)
    assert int(res[r]["before_arena_used"]) == used       # the arena was full to the byte

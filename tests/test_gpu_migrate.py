"""cluster.migrate with the HIP engine: two rank processes share the one GPU of the test box
(each with its own engine and directory on cuda:0) and exchange over gloo, as in
tests/test_gpu_dist.py.  Two routed steps under the hash partition, a live change to map B,
two routed steps under B, against the serial reference of tests/test_migrate_gloo.py, on the
host path (numpy, HostDirectory, export_state / import_state) and on the device path
(tbe_migrate_out_device, DeviceDirectory, tbe_import_rows_device), plain and classed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _migrate_workers as M
from tests import test_dist_gloo as G
from tests import test_migrate_gloo as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2


def _run_ranks(out_dir, *args: str, timeout: int = 150):
    """Both ranks as child processes (never exec'd from this GPU-initialised process)."""
    port = G._port()
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_migrate_workers.py"), "migrate_worker_hip",
                               str(r), str(WORLD), str(port), str(out_dir), *args],
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
    return [np.load(os.path.join(out_dir, f"mig_{r}.npz")) for r in range(WORLD)]


@pytest.mark.gpu
@pytest.mark.parametrize("classed", ["plain", "classed"])
@pytest.mark.parametrize("path", ["host", "device"])
def test_migrate_two_hip_ranks(gpu, oracle_lib, tmp_path, path, classed):
    res = _run_ranks(tmp_path, path, "ok", classed)
    MG.check_migrate(res, classed=classed == "classed", device_path=path == "device")


@pytest.mark.gpu
@pytest.mark.parametrize("classed", ["plain", "classed"])
def test_migrate_after_every_row_lapsed(gpu, oracle_lib, tmp_path, classed):
    """ts_us 6 s after step 1: every row has lapsed, so no row is exchanged while 494 keys
    change hands, and steps 2-3 (6 s later too) still match the serial reference."""
    res = _run_ranks(tmp_path, "device", "lapse", classed)
    assert sum(int(x["sent"]) for x in res) == 0
    MG.check_migrate(res, classed=classed == "classed", shift=M.LAPSE_SHIFT, device_path=True)


@pytest.mark.gpu
def test_preflight_failure_two_hip_ranks(gpu, tmp_path):
    MG.check_refused(_run_ranks(tmp_path, "device", "tight", "plain"))

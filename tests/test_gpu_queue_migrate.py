"""cluster.migrate_queueing with the HIP engine: two rank processes share the one GPU of the
test box (each with its own engine and directory on cuda:0) and exchange over gloo, as in
tests/test_gpu_migrate.py.  Two routed wait steps with a tick each under the hash partition, a
live change to map B that takes the queued waits along, a routed cancel of requests queued
before the move, two more steps under B, against the serial reference of
tests/test_queue_migrate_gloo.py, on the host path (numpy, HostDirectory, host-buffer queue
calls) and on the device path (tbe_queue_migrate_out_ids_device, tbe_queue_export_ids_device,
DeviceDirectory, tbe_queue_import_ids_device), plain and classed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import test_dist_gloo as G
from tests import test_queue_migrate_gloo as QG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2


def _run_ranks(out_dir, *args: str, timeout: int = 150):
    """Both ranks as child processes (never exec'd from this GPU-initialised process)."""
    port = G._port()
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_queue_migrate_workers.py"),
                               "queue_migrate_worker_hip", str(r), str(WORLD), str(port), str(out_dir), *args],
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
    return [np.load(os.path.join(out_dir, f"qmig_{r}.npz")) for r in range(WORLD)]


@pytest.mark.gpu
@pytest.mark.parametrize("classed", ["plain", "classed"])
@pytest.mark.parametrize("path", ["host", "device"])
def test_migrate_queueing_two_hip_ranks(gpu, tmp_path, path, classed):
    res = _run_ranks(tmp_path, path, "ok", classed)
    QG.check_queue_migrate(res, classed=classed == "classed")
    assert all(int(x["moved"][2]) > 0 and int(x["moved"][3]) > 0 for x in res)   # every rank sends and receives entries


@pytest.mark.gpu
def test_preflight_failure_two_hip_ranks(gpu, tmp_path):
    QG.check_refused(_run_ranks(tmp_path, "device", "tight", "plain"))

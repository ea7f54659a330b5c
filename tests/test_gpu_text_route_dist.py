"""Two HIP ranks on one GPU route batches keyed by resourceID text (cluster.route_text_batch)
over gloo, by the pattern of tests/test_gpu_dist.py: fresh child processes, each under its own
timeout, the HIP engine deciding.  Host path (numpy, HostStringDirectory) and device path (CUDA
tensors, tbe_route_text_* kernels, StringDirectory), hash partition and balanced map, against
the serial reference of tests/test_text_route_gloo.py.  One device-path step is also checked
against the u64 route of the keys its names were made from."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _text_route_workers as T
from tests.test_dist_gloo import _port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2


def _run_ranks(out_dir, *args: str, timeout: int = 150):
    """Both ranks as child processes (never exec'd from this GPU-initialised process)."""
    port = _port()
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_text_route_workers.py"),
                               "tx_route_worker_hip", str(r), str(WORLD), str(port), str(out_dir), *args],
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
    return [np.load(os.path.join(out_dir, f"tx_{r}.npz")) for r in range(WORLD)]


@pytest.mark.gpu
@pytest.mark.parametrize("path,map_kind", [("host", "hash"), ("host", "balanced"), ("device", "hash"), ("device", "balanced")])
def test_route_text_batch_two_hip_ranks(gpu, oracle_lib, tmp_path, path, map_kind):
    res = _run_ranks(tmp_path, path, map_kind)
    T.check_text_route(res)
    if path == "device" and map_kind == "hash":
        # by text and by the u64 keys the text was made from: per key, the same replies
        for r in res:
            by_text = sorted(zip(r["xkeys"].tolist(), r["xt_g"].tolist(), r["xt_r"].tolist()))
            by_key = sorted(zip(r["xkeys"].tolist(), r["xu_g"].tolist(), r["xu_r"].tolist()))
            assert by_text == by_key
            assert r["xt_g"].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_malformed_batch_on_one_hip_rank(gpu, oracle_lib, tmp_path, path):
    """Rank 1's batch of one step is malformed: it raises the designed ValueError (the worker
    checks the message), rank 0 finishes, and all replies equal the reference without it."""
    res = _run_ranks(tmp_path, path, "hash", "1")
    assert int(res[1]["raised"]) == T.BAD_STEP and int(res[0]["raised"]) == -1
    T.check_text_route(res, bad_rank=1)

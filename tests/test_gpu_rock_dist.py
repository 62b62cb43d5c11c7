"""GPU: rock regions in a decomposed run -- two real ranks on one GPU over the shared-memory test transport (as
tests/test_gpu_killough_dist.py runs them).  opmgpu_set_rock_regions and opmgpu_update_rock_history are rank-local: every rank holds the
regions and pressures of its local cells, ghosts included, and the same kernels form each cell's history and multipliers from the same
numbers on whichever rank holds it.  So the ranks hold the single-domain planes bit for bit, ghosts included (a ghost's trans_mult enters
the owner's flux).  No Newton iteration is run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from opmgpu import capi
from opmgpu.model import GpuBlackoilModel

from _rock_dist_worker import PARAMS, planes, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_rock_dist_worker.py")


def test_two_ranks_hold_the_single_domain_rock_planes(gpu_lib, tmp_path):
    g, t, reg, a, b = problem()
    m = GpuBlackoilModel(g, t, capi.default_params(**PARAMS))
    single = planes(m, reg, a, b)
    m.close()
    assert np.array_equal(single[0], a.p)                                                # the history took state A
    off = b.p > a.p
    assert off.sum() > g.nc // 4 and (~off).sum() > g.nc // 4 and np.abs(single[2] - 1.0).max() > 0.1
    env = dict(os.environ, OPMGPU_COMM_TRANSPORT="shm")
    env["PYTHONPATH"] = os.path.join(ROOT, "opm-simulators-legacy_amd") + os.pathsep + env.get("PYTHONPATH", "")
    code = "from opmgpu import partition; print(partition.make_unique_id().hex())"
    uid = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
    world = 2
    outs = [str(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, logs[r][-6000:])
    seen = np.zeros(g.nc, int)
    for o in outs:
        q = np.load(o)
        loc, n = q["local"], int(q["n_owned"])
        assert loc.size > n                                                              # the rank holds ghosts
        assert np.array_equal(q["planes"], single[:, loc])                               # bit for bit, ghosts included
        seen[loc[:n]] += 1
    assert np.all(seen == 1)

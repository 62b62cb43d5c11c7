"""GPU: opmgpu_set_swatinit_scaling in a decomposed run -- two real ranks on one GPU over the shared-memory test transport (as
tests/test_gpu_thpres_dist.py runs them).  The setter is rank-local: every rank passes its local cells, ghosts included, and no rank
talks to another; each cell's PCW is computed by the same kernel from the same numbers on whichever rank holds it, so it must be the
single-domain value bit for bit, ghosts included (a ghost's PCW enters the owner's flux).  One Newton iteration then matches the
single-domain one at the tolerance of tests/test_gpu_dist_shm.py for one Newton step: 1e-6 relative in pressure, 1e-6 in saturation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from opmgpu import capi
from opmgpu.model import GpuBlackoilModel

import swatinit_cases as cases
from _swatinit_dist_worker import PARAMS, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_swatinit_dist_worker.py")


def test_two_ranks_scale_like_one_domain(gpu_lib, tmp_path):
    g, t, st, (sw, pcow) = problem()
    m = GpuBlackoilModel(g, t, capi.default_params(**PARAMS))
    pcw0 = m.getPcw()
    sw_out = m.setSwatInitScaling(sw, pcow)
    pcw = m.getPcw()
    m.prepareStep(cases.DT, st)
    m.nonlinearIteration(0, single_precision=False)
    single = m.getState()
    m.close()
    assert (pcw != pcw0).sum() > g.nc // 2
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
        assert np.array_equal(q["pcw"], pcw[loc]) and np.array_equal(q["sw_out"], sw_out[loc])      # bit for bit, ghosts included
        seen[loc[:n]] += 1
        own = loc[:n]
        dp, ds = np.abs(q["p"] - single.p[own]).max() / np.abs(single.p).max(), np.abs(q["sat"] - single.sat[own]).max()
        print("rank: %d owned + %d ghost cells, one Newton iteration against the single domain: dp %.2e, ds %.2e" % (n, loc.size - n, dp, ds))
        assert dp <= 1e-6 and ds <= 1e-6
    assert np.all(seen == 1)

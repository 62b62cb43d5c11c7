"""GPU: opmgpu_compute_max_dp in a decomposed run -- two real ranks on one GPU over the shared-memory test transport (as
tests/test_gpu_dist_shm.py runs them).  The call is collective: every rank scans its local face connections and receives the maxima over
all ranks, which must be EXACTLY the single-domain table (every face is evaluated by the same kernel from the same cell values, on
whichever rank; a maximum does not care about the order)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from opmgpu import capi
from opmgpu.model import GpuBlackoilModel

import thpres_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_thpres_dist_worker.py")


def test_two_ranks_return_the_single_domain_table(gpu_lib, oracle, tmp_path):
    (g, t, eq, nreg, nface, st), want_max, want_dp, _ = cases.reference(oracle, "wog", cases.THREE_PHASE_CASES[2])
    m = GpuBlackoilModel(g, t, capi.default_params())
    m.setState(st)
    single_max, single_dp = m.computeMaxDp(eq, nreg, nface, conns=True)
    m.close()
    env = dict(os.environ, OPMGPU_COMM_TRANSPORT="shm")
    env["PYTHONPATH"] = os.path.join(ROOT, "opm-simulators-legacy_amd") + os.pathsep + env.get("PYTHONPATH", "")
    code = "from opmgpu import partition; print(partition.make_unique_id().hex())"
    uid = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
    world, axis = 2, 0               # cut in x: the slabs of regions 1 / 2 / 3 land on different ranks, no rank sees every pair
    outs = [str(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(axis), str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE,
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
    parts = [np.load(o) for o in outs]
    seen = np.zeros(g.nconn, bool)
    local_pairs = []
    for q in parts:
        assert np.array_equal(q["max_dp"], single_max)                                   # the global table, on every rank
        assert np.array_equal(q["dp"], single_dp[q["conn_index"]])                       # the plane stays local: the rank's connections
        seen[q["conn_index"]] = True
        lo, hi = np.sort(eq[g.conn_cells[q["conn_index"]]], axis=1).T
        local_pairs.append({(a, b) for a, b, f in zip(lo.tolist(), hi.tolist(), q["conn_index"].tolist()) if a != b and f < nface})
    assert seen.all()
    assert local_pairs[0] != local_pairs[1]                                              # the reduction had something to combine

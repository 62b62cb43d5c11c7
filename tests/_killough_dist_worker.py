"""One rank of a two-process Killough-hysteresis run over the shared-memory TEST transport (started by tests/test_gpu_killough_dist.py;
every rank uses cuda:0): the scaled case of tests/killough_cases.py cut into two slabs, the model set and the history updated with the
rank's local cells, ghosts included -- both are rank-local, no rank talks to another.  Writes the rank's history and scanning planes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opmgpu import capi, partition  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402

import killough_cases as kc  # noqa: E402

PARAMS = dict(linear_solver_reduction=1e-10, linear_solver_maxiter=1500)      # tests/test_gpu_dist_shm.py, case "ilu0"
DT = 2 * 86400.0
SEEDS = (1, 3)


def problem():
    tab, grid = kc.tables(), kc.grid_of("all")
    return grid, tab, [kc.history_state(grid, tab, s) for s in SEEDS]


def planes(model, states, local_state=lambda st: st):
    """the model switched to Killough BEFORE the first and the history updated with every state: [10][nc]"""
    model.setHysteresisModel(capi.HYST_KILLOUGH, kc.A)
    for st in states:
        model.prepareStep(DT, local_state(st))
        model.updateHysteresis()
    return np.stack(list(model.getHysteresis()) + list(model.getHysteresisScanning()))


def run(rank, world, uid, out):
    g, t, states = problem()
    part = partition.slab_partition(g, world, axis=2)
    dom = partition.LocalDomain(g, part, rank)
    model = GpuBlackoilModel(dom.grid, t, capi.default_params(**PARAMS))
    partition.attach_comm(model, dom, rank, world, uid)
    pl = planes(model, states, dom.local_state)
    np.savez(out, local=dom.global_of_local, n_owned=dom.n_owned, planes=pl)
    model.close()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4])

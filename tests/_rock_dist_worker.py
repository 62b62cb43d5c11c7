"""One rank of a two-process rock-region run over the shared-memory TEST transport (started by tests/test_gpu_rock_dist.py; every rank
uses cuda:0): a Cartesian grid cut into two slabs, the regions set with the rank's local cells, ghosts included, state A set, the history
updated, state B set -- all rank-local, no rank talks to another, no Newton iteration is run.  Writes the rank's p_min and multipliers."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opmgpu import capi, decks, partition  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402

import rock_cases as RC  # noqa: E402

PARAMS = dict(linear_solver_reduction=1e-10, linear_solver_maxiter=1500)      # tests/test_gpu_dist_shm.py, case "ilu0"
BAR = decks.BAR


def problem():
    """(grid, tables, regions over all cells, state A, state B): B lies below A in about half of the cells, above it in the others"""
    tab = decks.satfunc_standard_tables()
    grid = decks.cartesian_grid(6, 5, 8, lognormal_sigma=0.3)
    rng = np.random.default_rng(9)
    reg = RC.regions(rng.integers(0, RC.NREG, grid.nc))
    a = decks.random_state(grid, tab, seed=2)
    a.p[:] = rng.uniform(80.0, 430.0, grid.nc) * BAR
    b = decks.State(a.p + rng.uniform(-40.0, 40.0, grid.nc) * BAR, a.sat, a.rs, a.rv, a.hc)
    b.p[::7] = a.p[::7]                                                       # ties
    return grid, tab, reg, a, b


def planes(model, regions, a, b):
    """[3][nc]: p_min, pv_mult, trans_mult after set A, update, set B"""
    model.setRockRegions(regions)
    model.setState(a)
    model.updateRockHistory()
    model.setState(b)
    return np.stack([model.rockHistory()] + list(model.rockMultipliers()))


def run(rank, world, uid, out):
    g, t, reg, a, b = problem()
    part = partition.slab_partition(g, world, axis=2)
    dom = partition.LocalDomain(g, part, rank)
    model = GpuBlackoilModel(dom.grid, t, capi.default_params(**PARAMS))
    partition.attach_comm(model, dom, rank, world, uid)
    local, _ = dom.local_rock_regions(reg)
    pl = planes(model, local, dom.local_state(a), dom.local_state(b))
    np.savez(out, local=dom.global_of_local, n_owned=dom.n_owned, planes=pl)
    model.close()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4])

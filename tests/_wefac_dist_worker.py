"""One rank of a two-process assembly over the shared-memory TEST transport (started by tests/test_gpu_wefac.py; every rank uses cuda:0):
the deck and the two wells of tests/_dist_shm_worker.py, the injector with efficiency factor 0.5 and the producer with 0.8, cut into two
slabs of layers so that each rank owns one well.  The factor travels with the well (LocalDomain.local_wells), DeviceWellModel sets it on the
rank that owns the well (no communication); the rank assembles once, without the well pre-solve, and writes the residual of its owned cells.
The test computes the single-domain residual of the same deck with owned_residual() in its own process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opmgpu import capi, decks, partition  # noqa: E402
from opmgpu import wells as W  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402

import _dist_shm_worker as base  # noqa: E402

CFG = dict(nx=10, ny=9, nz=16, sigma=0.7, seed=21, perturb=0.004, rate=30.0 / 86400.0)          # the deck of tests/test_gpu_dist_shm.py
EFF = (0.5, 0.8)
DT = 2 * decks.DAY


def wells(grid, eff=EFF):
    wl = base.wells_of(grid, CFG)
    wl.efficiency = [float(e) for e in eff]
    return wl


def params():
    return capi.default_params(solve_welleq_initially=0)


def owned_residual(model, wl, lst, n_owned):
    driver = W.DeviceWellModel(model, wl, W.WellState(wl, lst.p))
    driver.prepareStep(DT, lst)
    model.setSolvePrecision(False)
    model.assemble(True)
    return model.residual().reshape(3, -1)[:, :n_owned]


def run(rank, world, uid, out):
    grid, tab, st = base.deck(CFG)
    part = partition.slab_partition(grid, world, axis=2)
    dom = partition.LocalDomain(grid, part, rank)
    model = GpuBlackoilModel(dom.grid, tab, params())
    partition.attach_comm(model, dom, rank, world, uid)
    wl = dom.local_wells(wells(grid), part)
    lst = dom.local_state(st)
    res = owned_residual(model, wl, lst, dom.n_owned)
    eff = model.getWellEfficiency() if wl.nw else np.zeros(0)
    np.savez(out, ids=dom.global_of_local[:dom.n_owned], residual=res, names=np.array(wl.name), eff=eff)
    model.close()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4])

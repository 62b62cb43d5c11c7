"""One rank of a two-process assembly over the shared-memory TEST transport (started by tests/test_gpu_pvcdo.py; every rank uses cuda:0):
the default three-phase case of tests/pvcdo_cases.py cut into slabs.  The rank creates its context on tables with the analytic oil, so the
model sets its own copy of the PVCDO rows (no communication), assembles once and writes the residual of its owned cells."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opmgpu import capi, decks, partition  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402

import pvcdo_cases as cases  # noqa: E402


def run(axis, rank, world, uid, out):
    g = cases.grid()
    own, _ = cases.tables("default")
    st = cases.smooth_state(g, "default")
    part = partition.slab_partition(g, world, axis=axis)
    dom = partition.LocalDomain(g, part, rank)
    model = GpuBlackoilModel(dom.grid, own, capi.default_params())
    partition.attach_comm(model, dom, rank, world, uid)
    model.prepareStep(5 * decks.DAY, dom.local_state(st))
    model.assemble(True)
    res = model.residual().reshape(3, dom.grid.nc)[:, :dom.n_owned]
    np.savez(out, ids=dom.global_of_local[:dom.n_owned], residual=res)
    model.close()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), bytes.fromhex(sys.argv[4]), sys.argv[5])

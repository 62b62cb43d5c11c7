"""One rank of a two-process SWATINIT run over the shared-memory TEST transport (started by tests/test_gpu_swatinit_dist.py; every rank uses
cuda:0): the 7 x 5 x 9 fixture of tests/swatinit_cases.py with its end points cut into two index ranges, the setter called with the
rank's local cells, ghosts included, then one Newton iteration.  Writes the rank's PCW and its owned cells' state."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opmgpu import capi, partition  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402

import swatinit_cases as cases  # noqa: E402

PARAMS = dict(linear_solver_reduction=1e-10, linear_solver_maxiter=1500)      # tests/test_gpu_dist_shm.py, case "ilu0"


def problem():
    g, t = cases.grid(arrays="eps"), cases.three_phase_tables()
    from opmgpu import decks
    st = decks.initial_state(g, t, perturb=0.002, seed=4)
    return g, t, st, cases.imposed(g, t)


def run(rank, world, uid, out):
    g, t, st, (sw, pcow) = problem()
    part = partition.slab_partition(g, world, axis=2)
    dom = partition.LocalDomain(g, part, rank)
    model = GpuBlackoilModel(dom.grid, t, capi.default_params(**PARAMS))
    partition.attach_comm(model, dom, rank, world, uid)
    loc = dom.global_of_local
    sw_out = model.setSwatInitScaling(sw[loc], pcow[loc])                        # no communication: a ghost's PCW is computed here too
    pcw = model.getPcw()
    model.prepareStep(cases.DT, dom.local_state(st))
    conv, lin = model.nonlinearIteration(0, single_precision=False)
    s = model.getState()
    n = dom.n_owned
    np.savez(out, local=loc, n_owned=n, pcw=pcw, sw_out=sw_out, p=s.p[:n], sat=s.sat[:n], lin=lin)
    model.close()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4])

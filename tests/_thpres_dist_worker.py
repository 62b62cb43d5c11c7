"""One rank of a two-process computeMaxDp over the shared-memory TEST transport (started by tests/test_gpu_thpres_dist.py; every rank uses
cuda:0): the first three-phase case of tests/thpres_cases.py cut into slabs, the rank's local cells (ghosts included) and local face
connections, the GLOBAL number of regions.  Writes the table the collective call returned and the rank's per-connection plane."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from opmgpu import capi, partition  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402

import thpres_cases as cases  # noqa: E402


def run(axis, rank, world, uid, out):
    g, t, eq, nreg, nface, st = cases.three_phase(*cases.THREE_PHASE_CASES[2])
    g.n_face_conn = nface
    part = partition.slab_partition(g, world, axis=axis)
    dom = partition.LocalDomain(g, part, rank)
    model = GpuBlackoilModel(dom.grid, t, capi.default_params())
    partition.attach_comm(model, dom, rank, world, uid)
    model.setState(dom.local_state(st))
    max_dp, dp = model.computeMaxDp(eq[dom.global_of_local], nreg, dom.grid.n_face_conn, conns=True)
    np.savez(out, max_dp=max_dp, dp=dp, conn_index=dom.conn_index)
    model.close()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), bytes.fromhex(sys.argv[4]), sys.argv[5])

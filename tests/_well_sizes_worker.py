"""One setting of OPMGPU_WELL_WOODBURY in a process of its own (test_gpu_well_sizes.py::test_woodbury_correction_leaves_the_newton_increment):
the variable is read when the solver is set up.  argv: the deck's name (long | manyNW) and the .npy file the Newton increment of the first
iteration goes to.  CPR + GMRES(40) with the true-residual check, device wells, reduction 1e-10.  Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import well_size_decks as D  # noqa: E402
from opmgpu import capi, wells as W  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402


def main():
    name, out = sys.argv[1], sys.argv[2]
    deck = D.long_deck() if name == "long" else D.many_deck(int(name[4:]))
    prm = capi.default_params(**dict(capi.CPR_AMG_VCYCLE, newton_use_gmres=1, gmres_verify_residual=1, linear_solver_reduction=1e-10, linear_solver_maxiter=2000))
    gm = GpuBlackoilModel(deck.grid, deck.tab, prm)
    md = W.DeviceWellModel(gm, deck.wl, W.WellState(deck.wl, deck.st.p))
    md.prepareStep(deck.dt, deck.st)
    gm.setSolvePrecision(False)
    gm.assemble(True)
    gm.getConvergence()
    md.wellConvergence()
    dx = gm.solveJacobianSystem(want_dx=True, single_precision=False)
    np.save(out, np.asarray(dx))
    res = {"woodbury": int(os.environ.get("OPMGPU_WELL_WOODBURY", "0")), "iterations": int(gm.linear_iterations), "reduction": float(gm.linear_reduction)}
    gm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

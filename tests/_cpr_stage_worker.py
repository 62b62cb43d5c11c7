"""One knob of the CPR pressure stage in a process of its own (test_gpu_cpr_stages.py::test_knobs_in_subprocesses): OPMGPU_AMG_SUB and
OPMGPU_AMG_GALERKIN_LPE are read once per process.  argv: the knob's name and value (also set in the environment by the caller).  Runs
the stage checks on a 30^3 deck without wells on the model path and prints one JSON line with the level sizes."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "opm-simulators-legacy_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_cpr_stages as T  # noqa: E402

KEYS = {"OPMGPU_AMG_SUB": "sub", "OPMGPU_AMG_FUSE": "fuse", "OPMGPU_AMG_GALERKIN_LPE": "lpe", "OPMGPU_AMG_NPRE": "npre", "OPMGPU_AMG_GS": "gs"}


def main():
    name, value = sys.argv[1], sys.argv[2]
    assert os.environ.get(name) == value
    key = KEYS[name]
    knob = (key, value.split(",")[0] if key == "lpe" else value)
    gm = T._model((30, 30, 30), False, wells=False)
    rowptr, col, val = gm.jacobian()
    kw = {}
    if key == "npre":
        kw["npre"] = int(value)
    if key == "gs":
        _, lev, nlev = gm.ordering()
        assert nlev == 2
        kw["gs_first"] = lev == 0
    n = T.check_hierarchy(gm, rowptr, col, val, False, "knob %s=%s" % (name, value), knobs=(knob,), **kw)
    _, nnz, nw = gm.cpr_levels()
    gm.close()
    print(json.dumps({"n": [int(v) for v in n], "nw": int(nw), "nnz": [int(v) for v in nnz], "knobs": [list(knob)]}))


if __name__ == "__main__":
    main()

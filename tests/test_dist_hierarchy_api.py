"""CPU-side checks of the switch of the distributed CPR pressure hierarchy: the exports exist, refuse a context without a communicator,
and the Python helpers pass the mode through."""
import ctypes as C

import pytest

from opmgpu import capi, partition


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_pressure_hierarchy_exports(lib):
    for name in ("opmgpu_comm_set_pressure_hierarchy", "opmgpu_cpr_dist_levels", "opmgpu_cpr_dist_level_get"):
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    # no context / no communicator: refused, nothing dereferenced
    assert lib.opmgpu_comm_set_pressure_hierarchy(None, 1) == capi.EINVAL
    nl, nd = C.c_int32(0), C.c_int32(0)
    assert lib.opmgpu_cpr_dist_levels(None, C.byref(nl), C.byref(nd)) == capi.EINVAL
    assert lib.opmgpu_cpr_dist_level_get(None, 0, None, None, None, None, None, None) == capi.EINVAL


def test_attach_comm_takes_the_mode():
    import inspect
    assert "pressure_hierarchy" in inspect.signature(partition.attach_comm).parameters
    assert callable(partition.set_pressure_hierarchy)

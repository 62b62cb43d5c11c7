"""The shapes the two assembly kernels are compiled in: (default, Stone II, oil-water) x (tables staged in LDS, tables read from the device
blob) x (double, float, double with the float copy written alongside).  Every shape assembles the SAME system: the table set past the
24 KiB the kernels stage is the small one with its regions repeated, on the 7 x 6 x 5 grid and the states of
test_gpu_assembly.py::test_table_set_too_large_for_lds.  The baseline of each model is (fits LDS, double); every other cell of the matrix
gives its residual within RTOL_JAC and its Jacobian within RTOL_JAC (double) or 2e-6 (float), the two bounds test_gpu_assembly.py uses
for exactly these comparisons.  Mixed precision: the double Jacobian is the baseline's, and one solve returns a dx that solves the
baseline's system to test_update_equations_scaling's bound.  One hysteresis case (default model; refused with the others) sends a
history through the assembly and through a kernel that takes the state as the CellPlanes bundle (the output record)."""
import numpy as np
import pytest

import twophase
from opmgpu import capi, decks
from opmgpu.model import GpuBlackoilModel
from util import rel_err

pytestmark = pytest.mark.gpu

RTOL_JAC = 1e-11          # tests/test_gpu_assembly.py: Jacobian blocks / residual in f64
RTOL_JAC_F32 = 2e-6       # tests/test_gpu_assembly.py: a float Jacobian against a double one
LDS_BYTES = 24 * 1024     # what the property kernels stage (BlackoilDevice::kTabLdsMaxBytes)
DT = 3 * decks.DAY
SEEDS = (1, 2)


def _f64_bytes(tab):
    return sum(a.nbytes for a in vars(tab).values() if isinstance(a, np.ndarray) and a.dtype == np.float64)


def _all_bytes(tab):
    return sum(a.nbytes for a in vars(tab).values() if isinstance(a, np.ndarray))


def _oil_water_tables(regions):
    """`regions` copies of the first region of tests/twophase.py"""
    return decks.FluidTables(density_wog=twophase.DENSITY_WO[:1] * regions, pvtw=twophase.PVTW[:1] * regions,
                             pvto=[twophase._dead_oil(twophase.PVDO[0])] * regions, pvtg=None, swof=twophase.SWOF[:1] * regions, sgof=None,
                             rock=twophase.ROCK, phases="wo")


def _hyst_tables(pairs):
    """`pairs` copies of (drainage region, imbibition region) of tests/test_satfunc_options.py::_hyst_tables, PVT regions alike"""
    t = decks.satfunc_standard_tables()
    swof = [list(zip(t.swof_sw, t.swof_krw, t.swof_krow, t.swof_pcow / decks.BAR)),
            [(0.1, 0.0, 1.0, 0.9), (0.2, 0.0, 0.7, 0.8), (0.3, 0.1, 0.45, 0.7), (0.4, 0.2, 0.25, 0.6), (0.6, 0.4, 0.0, 0.4), (0.9, 0.7, 0.0, 0.1)]]
    sgof = [list(zip(t.sgof_sg, t.sgof_krg, t.sgof_krog, t.sgof_pcgo / decks.BAR)),
            [(0.0, 0.0, 1.0, 0.2), (0.3, 0.0, 0.5, 0.8), (0.5, 0.2, 0.3, 1.2), (0.8, 0.6, 0.0, 2.0), (0.9, 1.0, 0.0, 2.1)]]
    n = 2 * pairs
    return decks.FluidTables(density_wog=[[1000.0, 700.0, 1.0]] * n, pvtw=[[1.0, 1.0, 4.0e-5, 0.96, 0.0]] * n,
                             pvto=[[(0, [(1., 1.0, 1.2)]), (200, [(400., 1.12, .94), (500., 1.1189, .94)])]] * n,
                             pvtg=[[(100, [(0.0001, 0.010, 0.1), (0.0, 0.0104, 0.1)]), (200, [(0.0004, 0.005, 0.2), (0.0, 0.0054, 0.2)])]] * n,
                             swof=swof * pairs, sgof=sgof * pairs, rock=(1.0, 5.0e-5))


# model -> (tables(copies), copies of the large set, regions per copy)
MODELS = {
    "default": (lambda r: decks.satfunc_standard_tables(regions=r), 24, 1),
    "stone2": (lambda r: decks.satfunc_standard_tables(regions=r, threephase_model=capi.KRO_STONE2), 24, 1),
    "oilwater": (_oil_water_tables, 48, 1),
    "hysteresis": (_hyst_tables, 20, 2),
}


def _deck(model, large):
    """(grid, tables) of one table set: the single copy with every cell in region 0 (imbibition: 1), or the repeated set with random
    region numbers.  The byte counts on both sides of the LDS limit are asserted: a case must not silently take the other path."""
    make, copies, per = MODELS[model]
    tab = make(copies if large else 1)
    if large:
        assert _f64_bytes(tab) > LDS_BYTES, (model, _f64_bytes(tab))       # the blob holds at least the caller's float64 arrays
    else:
        assert 2 * _all_bytes(tab) < LDS_BYTES, (model, _all_bytes(tab))    # the single copy fits, slopes (and an oil-water deck's stand-in gas) included
    base = decks.cartesian_grid(7, 6, 5, lognormal_sigma=0.7)
    nc = base.nc
    rng = np.random.default_rng(12)
    c_sat, c_pvt = (rng.integers(0, copies, nc), rng.integers(0, copies, nc)) if large else (np.zeros(nc, int), np.zeros(nc, int))
    if large:
        assert len(set(c_sat)) > 1 and len(set(c_pvt)) > 1 and (c_sat != c_pvt).any()
    kw = dict(imbnum=(per * c_sat + 1).astype(np.int32)) if model == "hysteresis" else {}
    grid = decks.GridData(nc, base.conn_cells, base.trans, base.pv, base.z, gravity=base.gravity, dims=base.dims,
                          pvtnum=(per * c_pvt).astype(np.int32), satnum=(per * c_sat).astype(np.int32), **kw)
    return grid, tab


def _states(model):
    grid, tab = _deck(model, False)
    if model == "oilwater":
        return [twophase.state(grid, seed=s) for s in SEEDS]
    return [decks.random_state(grid, tab, seed=s) for s in SEEDS]


def _history(nc, seed):
    """smallest wetting saturations seen so far (2.0 = none), so that cells sit on both the drainage and the imbibition curves"""
    rng = np.random.default_rng(100 + seed)
    mdc = [np.where(rng.random(nc) < 0.3, 2.0, 0.2 + 0.7 * rng.random(nc)) for _ in range(2)]
    return mdc


def _run(model, large, precision, want_dx=False):
    """per state: (residual, Jacobian blocks, output record, dx or None) of one shape"""
    grid, tab = _deck(model, large)
    prm = capi.default_params(preconditioner_single=int(precision == "mixed"), linear_solver_reduction=1e-10, linear_solver_maxiter=400)
    m = GpuBlackoilModel(grid, tab, prm)
    out = []
    for seed, st in zip(SEEDS, _states(model)):
        m.prepareStep(DT, st)
        if model == "hysteresis":
            m.setHysteresis(*_history(grid.nc, seed))
        m.setSolvePrecision(precision == "float")
        m.assemble(True)
        rowptr, col, val = m.jacobian()
        res = m.residual()
        rec = np.stack([v for _, v in sorted(m.simulatorData().items())])
        dx = None
        if want_dx:
            m.getConvergence()
            dx = m.solveJacobianSystem(want_dx=True, single_precision=False)
        out.append((res, val, rec, dx, rowptr, col))
    m.close()
    return out


_BASELINE = {}


def _baseline(model):
    """(fits LDS, double) of a model, computed once and shared"""
    if model not in _BASELINE:
        _BASELINE[model] = _run(model, False, "double")
        for res, val, rec, _, _, _ in _BASELINE[model]:
            for a in (res, val, rec):
                a.setflags(write=False)
    return _BASELINE[model]


def _bsr_matvec(rowptr, col, val, x):
    """y = A x for 3 x 3 blocks val[k] (row-major: equation, variable) and x [nc][3]"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    y = np.zeros_like(x)
    np.add.at(y, rows, np.einsum("kav,kv->ka", val.reshape(-1, 3, 3), x[col]))
    return y


def _check(model, large, precision):
    base = _baseline(model)
    got = _run(model, large, precision, want_dx=precision == "mixed")
    scale = np.array(capi.default_params().matbalscale[:])
    for seed, (r0, v0, rec0, _, rowptr, col), (r, v, rec, dx, rowptr_g, col_g) in zip(SEEDS, base, got):
        assert np.array_equal(rowptr_g, rowptr) and np.array_equal(col_g, col)
        e_r, e_v, e_rec = rel_err(r, r0), rel_err(v, v0), max(rel_err(a, b) for a, b in zip(rec, rec0))
        print("%s large=%d %s seed %d: residual %.3e Jacobian %.3e output record %.3e" % (model, large, precision, seed, e_r, e_v, e_rec))
        assert e_r < RTOL_JAC, (seed, e_r)
        assert e_v < (RTOL_JAC_F32 if precision == "float" else RTOL_JAC), (seed, e_v)       # mixed: the DOUBLE Jacobian
        assert e_rec < RTOL_JAC, (seed, e_rec)                  # the same f64 evaluation of equal tables, whatever the region numbers
        if dx is not None:
            nc = len(rowptr) - 1
            b = (r0.reshape(3, nc) * scale[:, None]).T
            y = _bsr_matvec(rowptr, col, v0, np.ascontiguousarray(dx.reshape(3, nc).T))
            print("    solve: max|A dx - b| / max|b| = %.3e" % (np.abs(y - b).max() / np.abs(b).max()))
            assert np.abs(y - b).max() <= 1e-7 * np.abs(b).max(), seed


@pytest.mark.parametrize("precision", ["double", "float", "mixed"])
@pytest.mark.parametrize("large", [False, True], ids=["lds", "blob"])
@pytest.mark.parametrize("model", ["default", "stone2", "oilwater"])
def test_assembly_shape_gives_the_baseline_system(gpu_lib, model, large, precision):
    if not large and precision == "double":
        # the baseline itself: a second run of it must give the same bits (nothing in the assembly depends on an order of arrival)
        for (r0, v0, rec0, *_), (r, v, rec, *_) in zip(_baseline(model), _run(model, False, "double")):
            assert np.array_equal(r, r0) and np.array_equal(v, v0) and np.array_equal(rec, rec0)
        return
    _check(model, large, precision)


def test_hysteresis_through_the_blob_path_and_the_bundle(gpu_lib):
    """HystArgs through every shape of the default model at once: tables read from the blob, mixed precision, against (LDS, double);
    the output record reads the same history through the CellPlanes bundle"""
    _check("hysteresis", True, "mixed")

"""GPU: the per-cell output record of a report step (BlackoilModelBase's SimulatorData: b, density, viscosity, kr, RsSat / RvSat,
Pb / Pd; k_simulator_data behind opmgpu_get_simulator_data) against the CPU oracle, the Pb / Pd inversion against a restatement of its
rule, and the way through RPTRST into the restart file.

Pb / Pd are taken at the SOLUTION state's rs / rv like the reference's (BlackoilModelBase_impl.hpp:678-683 pass state.rs / state.rv of the
SolutionState): the state's own rs in an OIL_ONLY cell (rv in a GAS_ONLY cell), the saturated value elsewhere -- the oracle's `rs` / `rv`
columns.  After updateState a state holds exactly these, so for a simulator's states "the state's rs" and this are the same numbers; the
random states here carry arbitrary rs in cells with free gas, where the distinction shows."""
import os

import numpy as np
import pytest

from opmgpu import capi, decks, eclio
from opmgpu.model import GpuBlackoilModel
from opmgpu.simulator import Simulator

pytestmark = pytest.mark.gpu
DECK = os.path.join(os.path.dirname(__file__), "golden", "decks", "SCHEDULE_SMALL.DATA")
ORDERINGS = [capi.ORDER_NATURAL, capi.ORDER_MULTICOLOR]
# tests/test_gpu_assembly.py::test_perf_props_and_well_terms on the same eval_cell outputs: rtol 1e-11, absolute floor 1e-13 of the property's
# largest magnitude
RTOL, ATOL_REL = 1e-11, 1e-13


def _with_regions(g, seed):
    rng = np.random.default_rng(seed)
    r = decks.GridData(g.nc, g.conn_cells, g.trans, g.pv, g.z, gravity=g.gravity, thpres=g.thpres, dims=g.dims,
                       pvtnum=rng.integers(0, 2, g.nc), satnum=rng.integers(0, 2, g.nc))
    assert set(r.pvtnum) == {0, 1} and set(r.satnum) == {0, 1} and (r.pvtnum != r.satnum).any()
    return r


def _grids():
    act = np.random.default_rng(5).random(7 * 6 * 5) > 0.3
    return [("60 cells", _with_regions(decks.cartesian_grid(5, 4, 3), 1), 3),           # less than one wavefront
            ("432 cells", _with_regions(decks.cartesian_grid(9, 8, 6), 2), 4),          # more than one block, the last one partial
            ("actnum", _with_regions(decks.cartesian_grid(7, 6, 5, actnum=act), 3), 5)]  # holes: the cell permutation is not the identity


def _state(grid, tab, seed):
    st = decks.random_state(grid, tab, seed=seed)
    assert set(st.hc) == {capi.HC_GAS_ONLY, capi.HC_GAS_AND_OIL, capi.HC_OIL_ONLY}       # all three phase states occur
    return st


def _close(got, ref):
    return np.allclose(got, ref, rtol=RTOL, atol=ATOL_REL * np.abs(ref).max())


def _scan(x, y, v):
    """The inversion rule, restated: segments from the lowest pressure upwards, the first and the last unbounded on their outer side; the
    first whose value range contains v gives x_i + (v - y_i) / slope_i; 0 when none does, when it is flat or the result is not finite."""
    n = len(x)
    for i in range(n - 1):
        y0, y1 = y[i], y[i + 1]
        d = np.sign(y1 - y0)
        inside = (v == y0) if d == 0 else ((i == 0 or (v - y0) * d >= 0) and (i == n - 2 or (y1 - v) * d >= 0))
        if inside:
            with np.errstate(all="ignore"):
                p = x[i] + (v - y0) / ((y1 - y0) / (x[i + 1] - x[i])) if d != 0 else 0.0
            return float(p) if np.isfinite(p) else 0.0
    return 0.0


def _scan_cells(ptr, x, y, reg, v):
    return np.array([_scan(x[ptr[r]:ptr[r + 1]], y[ptr[r]:ptr[r + 1]], vi) for r, vi in zip(reg, v)])


def _simdata(grid, tab, st, ordering, so_max=None):
    m = GpuBlackoilModel(grid, tab, capi.default_params(ilu_ordering=ordering))
    m.setState(st)
    if so_max is not None:
        m.setSatOilMax(so_max)
    sd = m.simulatorData()
    m.close()
    assert list(sd) == list(capi.SIMDATA_NAMES) and all(v.shape == (grid.nc,) for v in sd.values())
    return sd


@pytest.fixture(scope="module")
def tab2():
    return decks.satfunc_standard_tables(regions=2)


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_values_against_the_oracle(gpu_lib, oracle, tab2, ordering):
    names = oracle.PROP_NAMES
    cases = [(name, grid, seed) for name, grid, seed in _grids()]
    g0 = cases[0][1]
    cases.append(("end-point scaling", decks.with_endpoints(g0, decks.random_endpoints(g0, seed=3)), 3))
    for name, grid, seed in cases:
        st = _state(grid, tab2, seed)
        sd = _simdata(grid, tab2, st, ordering)
        ref = oracle.cell_props(grid, tab2, st)
        for k, ph in enumerate("wog"):
            for out, col in ((capi.SIMDATA_NAMES[k], "b_"), (capi.SIMDATA_NAMES[3 + k], "rho_"), (capi.SIMDATA_NAMES[6 + k], "mu_"),
                             (capi.SIMDATA_NAMES[9 + k], "kr_")):
                assert _close(sd[out], ref[:, names.index(col + ph), 0]), (name, out)
    # the scaled end points matter for kr in the last case
    plain = oracle.cell_props(g0, tab2, st)
    assert np.abs(plain[:, names.index("kr_w"), 0] - ref[:, names.index("kr_w"), 0]).max() > 1e-3
    assert capi.SIMDATA_NAMES[:12] == ("1OVERBW", "1OVERBO", "1OVERBG", "WAT_DEN", "OIL_DEN", "GAS_DEN", "WAT_VISC", "OIL_VISC", "GAS_VISC",
                                       "WATKR", "OILKR", "GASKR")


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_saturated_ratios_for_every_cell(gpu_lib, oracle, tab2, ordering):
    """RSSAT / RVSAT of every cell whatever its phase state = the oracle's rs / rv of the same state with every cell GAS_AND_OIL (there
    rs and rv ARE the saturated values; sw, sg, so, p_g do not change for a consistent state)."""
    names = oracle.PROP_NAMES

    def check(name, grid, tab, st, so_max):
        forced = st.copy()
        forced.hc[:] = capi.HC_GAS_AND_OIL
        sd = _simdata(grid, tab, st, ordering, so_max)
        ref = oracle.cell_props(grid, tab, forced)
        assert _close(sd["RSSAT"], ref[:, names.index("rs"), 0]) and _close(sd["RVSAT"], ref[:, names.index("rv"), 0]), name
        assert (sd["RSSAT"] > 0).all() and (sd["RVSAT"] > 0).any()
        return sd
    for name, grid, seed in _grids():
        check(name, grid, tab2, _state(grid, tab2, seed), None)
    # VAPPARS: the factor (so / soMax)^vap is part of the saturated values
    name, grid, seed = _grids()[0]
    vap = decks.satfunc_standard_tables(regions=2, vappars=(0.7, 1.3))
    st = _state(grid, vap, seed)
    so_max = np.maximum(st.sat[:, 1], np.random.default_rng(21).uniform(0.2, 0.9, grid.nc))
    without = check(name, grid, tab2, st, None)
    try:
        oracle.set_sat_oil_max(so_max)
        with_vap = check("vappars", grid, vap, st, so_max)
    finally:
        oracle.set_sat_oil_max(None)
    assert np.abs(with_vap["RSSAT"] - without["RSSAT"]).max() > 1e-3 * without["RSSAT"].max()


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_bubble_and_dew_point_round_trip(gpu_lib, oracle, tab2, ordering):
    """(a) Where Pb > 0 the forward evaluation of the saturated curve at Pb gives the rs it was inverted from, within 1e-12 of the table's
    largest rs (a handful of roundings on table-sized operands); the same for Pd and rv."""
    names = oracle.PROP_NAMES
    t = tab2
    for name, grid, seed in _grids():
        st = _state(grid, t, seed)
        ref = oracle.cell_props(grid, t, st)
        rs, rv = ref[:, names.index("rs"), 0], ref[:, names.index("rv"), 0]      # the solution state's rs / rv (module docstring)
        oil, gas = st.hc == capi.HC_OIL_ONLY, st.hc == capi.HC_GAS_ONLY
        assert np.array_equal(rs[oil], st.rs[oil]) and np.array_equal(rv[gas], st.rv[gas])
        # on the CPU first: the rule leaves at most 10 % of these cells without a bubble point, so the round trip cannot pass by skipping
        pb_cpu = _scan_cells(t.oil_node_ptr, t.oil_psat, t.oil_rs, grid.pvtnum, rs)
        pd_cpu = _scan_cells(t.gas_node_ptr, t.gas_pg, t.gas_rvsat, grid.pvtnum, rv)
        assert (pb_cpu == 0).mean() <= 0.10 and (pd_cpu == 0).mean() <= 0.10, name
        sd = _simdata(grid, t, st, ordering)
        pb, pd = sd["PBUB"], sd["PDEW"]
        assert (pb == 0).mean() <= 0.10 and np.array_equal(pb == 0, pb_cpu == 0) and np.array_equal(pd == 0, pd_cpu == 0), name
        k = pb > 0
        back = oracle.pvt(t, "rsSat", pb[k], pvtnum=grid.pvtnum[k])[:, 0]
        print(name, "Pb round trip, worst |rs' - rs| / max(table rs):", np.abs(back - rs[k]).max() / t.oil_rs.max())
        assert np.abs(back - rs[k]).max() <= 1e-12 * t.oil_rs.max(), name
        assert np.abs(back[oil[k]] - st.rs[oil & k]).max() <= 1e-12 * t.oil_rs.max(), name          # the state's own rs where it is the variable
        k = pd > 0
        back = oracle.pvt(t, "rvSat", pd[k], pvtnum=grid.pvtnum[k])[:, 0]
        print(name, "Pd round trip, worst |rv' - rv| / max(table rv):", np.abs(back - rv[k]).max() / t.gas_rvsat.max())
        assert np.abs(back - rv[k]).max() <= 1e-12 * t.gas_rvsat.max(), name
        assert np.abs(back[gas[k]] - st.rv[gas & k]).max() <= 1e-12 * t.gas_rvsat.max(), name


def _hand_made_tables():
    """Two PVT regions.  Oil: first node at rs = 10 (so rs can lie below it).  Gas, region 0: RvSat rises, stays FLAT over 100-150 bar,
    rises, FALLS over 200-250 bar and rises again (non-monotone: 4.5e-4 lies in the segments 150-200 and 200-250); region 1: flat FIRST
    segment."""
    pvto = [[(10, [(50., 1.05, 1.10)]), (60, [(150., 1.15, 1.00)]), (120, [(300., 1.30, 0.90), (400., 1.29, 0.90)])]] * 2
    col = lambda rv, b: [(rv, b, 0.02), (0.0, b * 1.04, 0.02)]      # noqa: E731
    pvtg = [[(50, col(1e-4, 0.020)), (100, col(3e-4, 0.010)), (150, col(3e-4, 0.0070)), (200, col(5e-4, 0.0050)), (250, col(2e-4, 0.0042)),
             (300, col(4e-4, 0.0035))],
            [(50, col(2e-4, 0.020)), (120, col(2e-4, 0.0090)), (300, col(4e-4, 0.0035))]]
    std = decks.satfunc_standard_tables()
    swof = [list(zip(std.swof_sw, std.swof_krw, std.swof_krow, std.swof_pcow / decks.BAR))] * 2
    sgof = [list(zip(std.sgof_sg, std.sgof_krg, std.sgof_krog, std.sgof_pcgo / decks.BAR))] * 2
    return decks.FluidTables(density_wog=[[1000.0, 700.0, 1.0]] * 2, pvtw=[[1.0, 1.0, 4.0e-5, 0.96, 0.0]] * 2, pvto=pvto, pvtg=pvtg,
                             swof=swof, sgof=sgof, rock=(1.0, 5.0e-5))


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_bubble_and_dew_point_scan_rule(gpu_lib, ordering):
    """(b) Against the restatement of the rule on a hand-made table set, within 1e-12 of the table's pressure span: below the first node,
    above the last, exactly on a node, a flat segment, and a non-monotone curve where the lower-pressure segment wins."""
    t = _hand_made_tables()
    grid = decks.cartesian_grid(5, 4, 3)
    n = grid.nc
    pvtnum = (np.arange(n) // 2) % 2
    grid = decks.GridData(n, grid.conn_cells, grid.trans, grid.pv, grid.z, gravity=grid.gravity, dims=grid.dims, pvtnum=pvtnum, satnum=pvtnum)
    rs_list = np.array([2.0, 150.0, 60.0, 10.0, 120.0, 35.0, 90.0])                  # below the first node, above the last, on nodes, inside
    rv_list = np.array([4.5e-4, 3e-4, 2.5e-4, 6e-4, 0.5e-4, 2e-4, 1e-4, 3.5e-4, 5e-4])   # two segments hold 4.5e-4; 3e-4 is a node and a flat segment
    oil = np.arange(n) < n // 2
    st = decks.State(np.linspace(80.0, 350.0, n) * decks.BAR, np.where(oil[:, None], [0.3, 0.7, 0.0], [0.3, 0.0, 0.7]),
                     np.where(oil, rs_list[np.arange(n) % rs_list.size], 50.0), np.where(oil, 1e-4, rv_list[np.arange(n) % rv_list.size]),
                     np.where(oil, capi.HC_OIL_ONLY, capi.HC_GAS_ONLY))
    sd = _simdata(grid, t, st, ordering)
    pb_ref = _scan_cells(t.oil_node_ptr, t.oil_psat, t.oil_rs, pvtnum, st.rs)
    pd_ref = _scan_cells(t.gas_node_ptr, t.gas_pg, t.gas_rvsat, pvtnum, st.rv)
    span_o, span_g = np.ptp(t.oil_psat), np.ptp(t.gas_pg)
    assert np.abs(sd["PBUB"][oil] - pb_ref[oil]).max() <= 1e-12 * span_o
    assert np.abs(sd["PDEW"][~oil] - pd_ref[~oil]).max() <= 1e-12 * span_g
    # the restatement itself gives what the rule says for the named cases (region 0 unless stated)
    bar = decks.BAR
    x, y = t.gas_pg[:6], t.gas_rvsat[:6]
    assert _scan(t.oil_psat[:3], t.oil_rs[:3], 2.0) == pytest.approx(34.0 * bar, rel=1e-14)        # outer extrapolation below the first node
    assert _scan(t.oil_psat[:3], t.oil_rs[:3], 150.0) == pytest.approx(375.0 * bar, rel=1e-14)     # above the last node
    assert _scan(t.oil_psat[:3], t.oil_rs[:3], 60.0) == pytest.approx(150.0 * bar, rel=1e-14)      # exactly on a node
    assert _scan(x, y, 4.5e-4) == pytest.approx(187.5 * bar, rel=1e-14)                            # not 208.33 bar: the lower-pressure segment
    assert _scan(x, y, 3e-4) == pytest.approx(100.0 * bar, rel=1e-14)                              # the node before the flat segment
    assert _scan(x, y, 6e-4) == pytest.approx(350.0 * bar, rel=1e-14)                              # last segment, unbounded above
    assert _scan(t.gas_pg[6:], t.gas_rvsat[6:], 2e-4) == 0.0                                       # region 1: the matching segment is flat
    assert _scan(t.gas_pg[6:], t.gas_rvsat[6:], 1e-4) == 0.0                                       # region 1: no segment contains the value
    # ... and every one of them is among the cells compared above
    r0, r1 = pvtnum == 0, pvtnum == 1
    for v in (2.0, 150.0, 60.0):
        assert (st.rs[oil & r0] == v).any()
    for v in (4.5e-4, 3e-4, 6e-4):
        assert (st.rv[~oil & r0] == v).any()
    assert (st.rv[~oil & r1] == 2e-4).any() and (st.rv[~oil & r1] == 1e-4).any()
    flat = ~oil & r1 & ((st.rv == 2e-4) | (st.rv == 1e-4))
    assert (sd["PDEW"][flat] == 0.0).all() and (sd["PDEW"][~oil & r0] > 0).all()


def test_dead_oil_dry_gas_have_no_saturation_pressure(gpu_lib):
    """(c) PVCDO / PVDG: no DISGAS, no VAPOIL -> RSSAT, RVSAT, PBUB, PDEW exactly 0."""
    tab = decks.fluid_data_tables()
    grid = decks.cartesian_grid(5, 4, 3)
    sd = _simdata(grid, tab, decks.random_state(grid, tab, seed=3), capi.ORDER_MULTICOLOR)
    for name in ("RSSAT", "RVSAT", "PBUB", "PDEW"):
        assert np.array_equal(sd[name], np.zeros(grid.nc)), name
    assert (sd["1OVERBO"] > 0).all() and (sd["OIL_VISC"] > 0).all()


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_no_side_effects(gpu_lib, tab2, ordering):
    name, grid, seed = _grids()[1]
    st = _state(grid, tab2, seed)
    m = GpuBlackoilModel(grid, tab2, capi.default_params(ilu_ordering=ordering))
    m.prepareStep(3 * decks.DAY, st)
    m.assemble(True)
    r0, j0 = m.residual().copy(), m.jacobian()[2].copy()
    a = m.simulatorData()
    b = m.simulatorData()
    for k in capi.SIMDATA_NAMES:
        assert np.array_equal(a[k], b[k]), k                      # twice: bit-identical
    m.assemble(True)
    assert np.array_equal(m.residual(), r0) and np.array_equal(m.jacobian()[2], j0)
    g = m.getState()
    assert np.array_equal(g.p, st.p) and np.array_equal(g.sat, st.sat) and np.array_equal(g.hc, st.hc)
    m.close()


def test_contract(gpu_lib, tab2):
    grid = decks.cartesian_grid(5, 4, 3)
    m = GpuBlackoilModel(grid, tab2, capi.default_params())
    out = np.zeros((capi.SIMDATA_K, grid.nc))
    assert m.lib.opmgpu_get_simulator_data(m.ctx, capi.dptr(out)) == capi.EINVAL          # before a state has been set
    assert not out.any()
    m.setState(decks.random_state(grid, tab2, seed=3))
    assert m.lib.opmgpu_get_simulator_data(m.ctx, None) == capi.EINVAL                    # NULL out
    assert m.lib.opmgpu_get_simulator_data(None, capi.dptr(out)) == capi.EINVAL
    assert m.lib.opmgpu_get_simulator_data(m.ctx, capi.dptr(out)) == capi.OK and out[3].min() > 0
    m.close()


def _run(tmp_path, tag, solution=None, schedule=None):
    text = open(DECK).read()
    if solution is not None:
        text = text.replace("SCHEDULE\n", "RPTRST\n %s /\nSCHEDULE\n" % solution, 1)
    if schedule is not None:                                         # after the first report step
        text = text.replace("TSTEP\n 10 20 /", "RPTRST\n %s /\nTSTEP\n 10 20 /" % schedule, 1)
    assert (text != open(DECK).read()) == (solution is not None or schedule is not None)
    path, base = str(tmp_path / (tag + ".DATA")), str(tmp_path / tag)
    open(path, "w").write(text)
    prm = capi.default_params(cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1, tolerance_mb=1e-9, tolerance_cnv=1e-5, tolerance_wells=1e-8,
                              linear_solver_reduction=1e-6, linear_solver_maxiter=200)
    sim = Simulator(path, params=prm, output_base=base)
    calls, orig = [], sim.model.simulatorData

    def recording():
        calls.append(orig())
        return calls[-1]
    sim.model.simulatorData = recording
    reps = sim.run(max_steps=2)
    assert [r["days"] for r in reps] == [10.0, 20.0]
    last = orig()
    sim.close()
    return base, calls, last


def _solution_sections(base):
    """per report (SEQNUM): the keywords after RV up to ENDSOL, and all arrays"""
    out, cur = {}, None
    for name, _, data in eclio.read_arrays(base + ".UNRST"):
        if name == "SEQNUM":
            cur = int(data[0]); out[cur] = {}
        else:
            out[cur][name] = data
    order = {k: list(v)[list(v).index("RV") + 1:list(v).index("ENDSOL")] for k, v in out.items()}
    return order, out


def test_through_the_restart_file(gpu_lib, tmp_path):
    base, calls, last = _run(tmp_path, "RPT", solution="BASIC=2 BO DEN VISC KRW KRG RSSAT PBPD", schedule="BASIC=2 BW")
    assert len(calls) == 2                                           # once per report step
    order, arrays = _solution_sections(base)
    first = ["1OVERBO", "WAT_DEN", "OIL_DEN", "GAS_DEN", "WAT_VISC", "OIL_VISC", "GAS_VISC", "WATKR", "GASKR", "RSSAT", "PBUB", "PDEW"]
    # SEQNUM 1 is the initial state (no per-cell data, like SimulatorBase_impl.hpp:184-186), 2 and 3 the two report steps
    assert order == {1: [], 2: first, 3: ["1OVERBW"]}                # the SCHEDULE list REPLACES the SOLUTION one
    for seq, sd in ((2, calls[0]), (3, calls[1])):
        for name in order[seq]:
            assert np.array_equal(arrays[seq][name], np.float32(eclio.simdata_to_deck_units(name, sd[name]))), (seq, name)
    assert np.array_equal(arrays[3]["1OVERBW"], np.float32(last["1OVERBW"]))               # the final state's record
    # deck units: bar and cP next to the state's own pressure
    assert np.all(np.abs(arrays[2]["PBUB"] - arrays[2]["PRESSURE"]) < 400.0) and 0.1 < arrays[2]["OIL_VISC"].mean() < 10.0
    assert 500.0 < arrays[2]["OIL_DEN"].mean() < 1000.0
    # no mnemonic set: the file is byte for byte what it is without the keyword
    base_a, calls_a, _ = _run(tmp_path, "ABSENT")
    base_b, calls_b, _ = _run(tmp_path, "BASIC", solution="BASIC=2")
    assert calls_a == [] and calls_b == []
    ua, ub = open(base_a + ".UNRST", "rb").read(), open(base_b + ".UNRST", "rb").read()
    assert len(ua) > 1000 and ua == ub
    oa, _ = _solution_sections(base_a)
    assert oa == {1: [], 2: [], 3: []}
    # ... and the selected arrays are additions: the solution arrays of the run with RPTRST are those of the run without
    _, plain = _solution_sections(base_a)
    for seq in (1, 2, 3):
        for name in ("PRESSURE", "SWAT", "SGAS", "RS", "RV"):
            assert np.array_equal(arrays[seq][name], plain[seq][name]), (seq, name)

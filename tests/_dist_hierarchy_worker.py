"""One rank of a multi-process run over the shared-memory TEST transport with the distributed CPR pressure hierarchy
(opmgpu_comm_set_pressure_hierarchy).  Started by tests/test_gpu_dist_hierarchy.py with a JSON config, the rank, the world size, the
unique id and the output file.  Runs `newton` Newton iterations of the synthetic deck of tests/_dist_shm_worker.py (or of the Norne-like deck) and writes this rank's
owned state, its part of every level of the hierarchy of the last CPR solve in global numbering, and one collective V-cycle on a seeded
right-hand side."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opm-simulators-legacy_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import _dist_shm_worker as base  # noqa: E402
from opmgpu import baseline_decks, capi, decks, partition  # noqa: E402
from opmgpu import wells as W  # noqa: E402
from opmgpu.model import GpuBlackoilModel  # noqa: E402


def deck(cfg):
    """(grid, tables, state, global wells or None): the synthetic deck of tests/_dist_shm_worker.py, or the Norne-like one with its own wells"""
    if cfg.get("deck") == "nornelike":
        grid, tab, st, wl = baseline_decks.norne_like()
        return grid, tab, st, (wl if cfg.get("wells") else None)
    grid, tab, st = base.deck(cfg)
    return grid, tab, st, (base.wells_of(grid, cfg) if cfg.get("wells") else None)


def run(cfg, rank, world, uid, out):
    grid, tab, st, wl = deck(cfg)
    prm = capi.default_params(**cfg["params"])
    comm = world > 1 or cfg.get("comm1")
    if not comm:
        model, lst = GpuBlackoilModel(grid, tab, prm), st
        gol, n_owned, n_local = np.arange(grid.nc), grid.nc, grid.nc
        well_index = np.arange(wl.nw if wl is not None else 0)
    else:
        part = partition.slab_partition(grid, world, axis=cfg.get("axis", 2))
        dom = partition.LocalDomain(grid, part, rank)
        model = GpuBlackoilModel(dom.grid, tab, prm)
        partition.attach_comm(model, dom, rank, world, uid, pressure_hierarchy=cfg.get("mode"))
        if cfg.get("check_api"):
            lib = model.lib
            assert lib.opmgpu_comm_set_pressure_hierarchy(model.ctx, 2) == capi.EINVAL
            assert lib.opmgpu_comm_set_pressure_hierarchy(model.ctx, -1) == capi.EINVAL
            os.environ["OPMGPU_AMG_GS"] = "1"
            assert lib.opmgpu_comm_set_pressure_hierarchy(model.ctx, 1) == capi.EINVAL      # Gauss-Seidel by colour: out of scope
            del os.environ["OPMGPU_AMG_GS"]
            assert lib.opmgpu_comm_set_pressure_hierarchy(model.ctx, cfg.get("mode") or 0) == capi.OK
        lst = dom.local_state(st)
        gol, n_owned, n_local = dom.global_of_local, dom.n_owned, dom.grid.nc
        if wl is not None:
            wl = dom.local_wells(wl, part)
        well_index = np.asarray(getattr(dom, "well_index", []), np.int64)
    nw_global = int(cfg.get("nw_global", 0))
    driver = model
    if wl is not None:
        driver = W.DeviceWellModel(model, wl, W.WellState(wl, lst.p))
    driver.prepareStep(cfg["dt_days"] * decks.DAY, lst)
    hist = []
    for it in range(cfg["newton"]):
        conv, lin = driver.nonlinearIteration(it, single_precision=cfg.get("single", False))
        hist.append([bool(conv), int(lin)])
    s = model.getState()
    res = dict(ids=gol[:n_owned], p=s.p[:n_owned], sat=s.sat[:n_owned], hc=s.hc[:n_owned], hist=np.array(hist, dtype=np.int64))
    nl, nd = model.cpr_dist_levels()
    res["nl"], res["nd"] = nl, nd
    if cfg.get("hierarchy"):
        res["factors"] = np.array(model.cpr_correction_factors())
        res["well_gid"] = grid.nc + well_index
        for l in range(nl):
            rows, rowptr, cols, val, agg = model.cpr_dist_level(l)
            if l == 0 and nd > 0:          # caller-local cells -> global ids, the wells after all cells in the global deck's order
                glob = np.concatenate([gol, grid.nc + well_index])
                assert rows.max() < glob.size and cols.max() < glob.size
                rows, cols = glob[rows], glob[cols]
            res.update({"L%d_rows" % l: rows, "L%d_rowptr" % l: rowptr, "L%d_cols" % l: cols, "L%d_val" % l: val, "L%d_agg" % l: agg})
        inv = model.cpr_level(nl - 1)[4]
        if inv is not None:
            res["inv"] = inv
        if nd == 0:                        # a single-domain hierarchy: level 0 as opmgpu_cpr_level_get reports it
            rowptr, col, val, _, _ = model.cpr_level(0)
            res.update({"S0_rowptr": rowptr, "S0_col": col, "S0_val": val})
        b = np.random.default_rng(7).standard_normal(grid.nc + nw_global)
        x = model.cpr_vcycle_apply(np.concatenate([b[gol[:n_owned]], b[grid.nc + well_index]]))
        res["x"], res["x_ids"] = x, np.concatenate([gol[:n_owned], grid.nc + well_index])
    np.savez(out, **res)
    model.close()


if __name__ == "__main__":
    cfg = json.loads(sys.argv[1])
    rank, world = int(sys.argv[2]), int(sys.argv[3])
    uid = bytes.fromhex(sys.argv[4]) if sys.argv[4] != "-" else None
    run(cfg, rank, world, uid, sys.argv[5])

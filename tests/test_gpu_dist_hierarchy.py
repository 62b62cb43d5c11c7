"""GPU: the distributed CPR pressure hierarchy (opmgpu_comm_set_pressure_hierarchy mode 1) with 2 and 4 REAL ranks on
one GPU over the shared-memory test transport (tests/support/shm_transport.cpp), launched like tests/test_gpu_dist_shm.py.

* the levels are global: level 0 gathered from the ranks' owned rows is the single-domain level 0; every coarser level, gathered, is the
  float64 Galerkin product P^T A P of the gathered level above and the gathered aggregates (tests/amg_reference.py); the replicated
  levels are the same bits on every rank;
* one collective V-cycle is the float64 restatement's cycle on the gathered hierarchy -- and not the cycle with the cross-rank couplings
  dropped (control);
* the Newton path of the decomposed runs in mode 1 is the single-domain one;
* on one rank the switch changes nothing;
* on the weak-scaling deck it needs fewer GMRES columns than the rank-local cycle."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_dist_hierarchy_worker.py")

CPR = dict(linear_solver_reduction=1e-10, linear_solver_maxiter=500, cpr_use_amg=1, cpr_max_ell_iter=0, use_cpr=1)
DECK = dict(nx=10, ny=9, nz=16, sigma=0.7, seed=21, perturb=0.004, dt_days=3.0, rate=30.0 / 86400.0)


def _launch(worker, cfg, world, tmp, extra_env=None, tag=""):
    """world processes of `worker` (one rank each); returns their output files' arrays"""
    env = dict(os.environ)
    env["OPMGPU_COMM_TRANSPORT"] = "shm"
    env.pop("OPMGPU_CPR_GLOBAL_AMG", None)
    env.update(extra_env or {})
    env["PYTHONPATH"] = os.path.join(ROOT, "opm-simulators-legacy_amd") + os.pathsep + env.get("PYTHONPATH", "")
    code = ("import sys; sys.path.insert(0, %r); from opmgpu import partition; print(partition.make_unique_id().hex())"
            % os.path.join(ROOT, "opm-simulators-legacy_amd"))
    uid = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
    procs, outs = [], []
    for r in range(world):
        out = os.path.join(tmp, "%s_w%d_r%d.npz" % (tag, world, r))
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, worker, json.dumps(cfg), str(r), str(world), uid, out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, logs[r][-8000:])
    return [dict(np.load(o)) for o in outs]


def _state(parts):
    n = sum(int(q["ids"].size) for q in parts)
    p, sat = np.zeros(n), np.zeros((n, 3))
    for q in parts:
        p[q["ids"]], sat[q["ids"]] = q["p"], q["sat"]
    return p, sat, parts[0]["hist"]


def _gather(parts, l, n):
    """level l from the ranks' owned rows, in global numbering: (matrix, aggregate of every row)"""
    rows, cols, vals, agg = [], [], [], np.full(n, -1, np.int64)
    for q in parts:
        r, rp = q["L%d_rows" % l], q["L%d_rowptr" % l]
        rows.append(np.repeat(r, np.diff(rp)))
        cols.append(q["L%d_cols" % l])
        vals.append(q["L%d_val" % l])
        agg[r] = q["L%d_agg" % l]
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return A, agg


def _rel(A, B):
    return abs(A - B).max() / abs(B).max()


# Hierarchy cases.  OPMGPU_AMG_TAIL_ROWS=64 keeps level 1 of the 1440-cell deck (~200 global rows) distributed, so that these cases run at
# least two distributed levels (ghost lists of a coarse level, its exchanges and Galerkin sums with ghost columns); the Norne-like deck
# (45 000 active cells, 36 wells, j-row slabs) reaches them with the default threshold.
HIER_CASES = {
    "cart": dict(DECK, params=CPR, wells=False, env={"OPMGPU_AMG_TAIL_ROWS": "64"}),
    "cart_wells": dict(DECK, params=CPR, wells=True, nw_global=2, env={"OPMGPU_AMG_TAIL_ROWS": "64"}),
    "cart_f32": dict(DECK, params=dict(CPR, preconditioner_single=1), wells=False, single_prec=True, env={"OPMGPU_AMG_TAIL_ROWS": "64"}),
    "nornelike": dict(params=CPR, deck="nornelike", wells=True, nw_global=36, axis=1, dt_days=3.0, env={}),
}
TOL = {False: 1e-12, True: 5e-5}


@pytest.mark.parametrize("case", sorted(HIER_CASES))
def test_distributed_levels_and_cycle_are_the_global_ones(gpu_lib, case):
    c = dict(HIER_CASES[case])
    env, f32 = c.pop("env"), c.pop("single_prec", False)
    tol = TOL[f32]
    cfg = dict(c, newton=1, hierarchy=True, mode=1)
    with tempfile.TemporaryDirectory() as tmp:
        sd = _launch(WORKER, dict(cfg, mode=None), 1, tmp, env, tag="sd")[0]
        for world in (2, 4):
            parts = _launch(WORKER, dict(cfg, check_api=True), world, tmp, env, tag="d")
            _check_hierarchy(sd, parts, tol, "%s/%d" % (case, world))


def _check_hierarchy(sd, parts, tol, tag):
    n0 = int(sd["S0_rowptr"].size - 1)            # cells + wells of the global deck
    nl, nd = int(parts[0]["nl"]), int(parts[0]["nd"])
    assert nd >= 2 and nl > nd and all(int(q["nl"]) == nl and int(q["nd"]) == nd for q in parts), (tag, nl, nd)
    print("%s: %d levels, %d distributed" % (tag, nl, nd))
    # level 0: the single-domain pressure matrix of the same (initial) state, well border included
    A0, agg0 = _gather(parts, 0, n0)
    S0 = ref.csr(sd["S0_rowptr"], sd["S0_col"], sd["S0_val"], n0)
    assert _rel(A0, S0) <= tol, (tag, _rel(A0, S0))
    owner = np.full(n0, -1, np.int64)
    for r, q in enumerate(parts):
        owner[q["x_ids"]] = r
    assert (owner >= 0).all()
    # aggregates stay inside a rank, on every distributed level
    aggs, A, own = [], [A0], owner
    for l in range(nl):
        n = n0 if l == 0 else int(aggs[-1].max()) + 1
        if l < nd:
            Al, agg = _gather(parts, l, n) if l else (A0, agg0)
            assert (agg >= 0).all(), (tag, l)
            oc = np.full(int(agg.max()) + 1, -1, np.int64)
            oc[agg] = own
            assert np.array_equal(oc[agg], own), (tag, l)            # every aggregate has ONE owner
            own = oc
        else:          # replicated: the same bits on every rank
            q0 = parts[0]
            for q in parts[1:]:
                for k in ("rows", "rowptr", "cols", "val", "agg"):
                    assert np.array_equal(q["L%d_%s" % (l, k)], q0["L%d_%s" % (l, k)]), (tag, l, k)
            Al = ref.csr(q0["L%d_rowptr" % l], q0["L%d_cols" % l], q0["L%d_val" % l], n)
            agg = q0["L%d_agg" % l]
        if l:
            G = (ref.prolongation(aggs[-1], n).T @ A[-1] @ ref.prolongation(aggs[-1], n)).tocsr()
            assert Al.shape == G.shape and _rel(Al, G) <= tol, (tag, l, _rel(Al, G))
            A.append(Al)
        if l < nl - 1:
            aggs.append(agg)
    if "inv" in parts[0]:                          # the coarsest level's dense inverse: the same bits on every rank
        for q in parts[1:]:
            assert np.array_equal(q["inv"], parts[0]["inv"]), tag
    # one collective V-cycle = the restatement's cycle on the gathered hierarchy (BiCGStab: two post-sweeps on level 0)
    b = np.random.default_rng(7).standard_normal(n0)
    x = np.zeros(n0)
    for q in parts:
        x[q["x_ids"]] = q["x"]
    pd0, pd = parts[0]["factors"]
    want = ref.Hierarchy(A0, aggs).vcycle(b, pdamp0=pd0, pdamp=pd, npost0=2)
    err = np.abs(x - want).max() / np.abs(want).max()
    assert err <= tol, (tag, err)
    # control: the same restatement without the couplings between ranks lands far outside the tolerance
    C0 = A0.tocoo()
    keep = owner[C0.row] == owner[C0.col]
    Ablk = sp.csr_matrix((C0.data[keep], (C0.row[keep], C0.col[keep])), shape=A0.shape)
    ctrl = ref.Hierarchy(Ablk, aggs).vcycle(b, pdamp0=pd0, pdamp=pd, npost0=2)
    off = np.abs(ctrl - want).max() / np.abs(want).max()
    print("%s: cycle error %.2e, control %.2e" % (tag, err, off))
    assert off >= 100 * tol, (tag, off)


NEWTON_CASES = {
    "cpr": dict(DECK, params=CPR, wells=False, newton=4),
    "cpr_wells": dict(DECK, params=CPR, wells=True, newton=4),
    "cpr_gmres_wells": dict(DECK, params=dict(CPR, newton_use_gmres=1), wells=True, newton=4),
    "nornelike": dict(params=CPR, deck="nornelike", wells=True, axis=1, dt_days=3.0, newton=2),
}


@pytest.mark.parametrize("case", sorted(NEWTON_CASES))
def test_mode1_runs_walk_the_single_domain_newton_path(gpu_lib, case):
    cfg = dict(NEWTON_CASES[case], mode=1)
    with tempfile.TemporaryDirectory() as tmp:
        p0, s0, h0 = _state(_launch(WORKER, cfg, 1, tmp, tag="sd"))
        for world in (2, 4):
            parts = _launch(WORKER, cfg, world, tmp, tag="d")
            assert all(int(q["nd"]) >= 1 for q in parts), (case, world)          # the hierarchy WAS distributed
            p, s, h = _state(parts)
            assert np.array_equal(h[:, 0], h0[:, 0]), (case, world)
            assert np.abs(p - p0).max() <= 1e-6 * np.abs(p0).max(), (case, world)
            assert np.abs(s - s0).max() <= 1e-6, (case, world)


def test_mode1_on_one_rank_is_mode0(gpu_lib):
    cfg = dict(DECK, params=CPR, newton=2, wells=True, comm1=True)
    with tempfile.TemporaryDirectory() as tmp:
        a = _launch(WORKER, dict(cfg, mode=0), 1, tmp, tag="m0")[0]
        b = _launch(WORKER, dict(cfg, mode=1, check_api=True), 1, tmp, tag="m1")[0]
    assert int(b["nd"]) == 0
    for k in ("p", "sat", "hc", "hist"):
        assert np.array_equal(a[k], b[k]), k


def test_fewer_gmres_columns_than_the_rank_local_cycle_on_the_weak_deck(gpu_lib):
    """bench.py's 2-rank weak deck (two copies of a 24^3 5-spot side by side along j), GMRES at the default tolerance: the distributed
    hierarchy needs strictly fewer columns per solve than the rank-local cycle (7.5 -> 4.1 at 40^3 per rank)."""
    env = dict(os.environ)
    env["OPMGPU_COMM_TRANSPORT"] = "shm"
    env["PYTHONPATH"] = os.path.join(ROOT, "opm-simulators-legacy_amd") + os.pathsep + env.get("PYTHONPATH", "")
    cols = {}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in (0, 1):
            env["OPMGPU_CPR_GLOBAL_AMG"] = str(mode)
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                   "--master-port", str(29640 + mode), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--nx", "24", "--ny", "24", "--nz", "24",
                   "--steps", "8", "--warmup", "2", "--detail", os.path.join(tmp, "detail%d.json" % mode)]
            out = subprocess.run(cmd, env=env, cwd=tmp, capture_output=True, text=True, timeout=400)
            assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            cols[mode] = json.loads(line)["config"]["linear_its_per_solve"]
    print("GMRES columns per solve, 2 ranks: rank-local %.2f, distributed %.2f" % (cols[0], cols[1]))
    assert cols[1] < cols[0], cols

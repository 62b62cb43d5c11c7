// cpr_inspect.inl -- diagnostics of the CPR pressure hierarchy (the opmgpu_cpr_* entry points; tests/test_gpu_cpr_stages.py); part of linsolver.hip.
// They read the hierarchy of the last CPR solve in the precision it ran in and leave the solver's state as they found it: the x / x2 roles
// of every level and level 0's right-hand side are restored, the correction factors and `factors_kept` are not touched.
template <class S> AmgHierarchy<S>* LinSolver::cpr_hierarchy()
{
    SolverWork<S>& w = work<S>();
    return (w.amg && w.amg->ready()) ? w.amg.get() : nullptr;
}

// a distributed level 0 (collective calls): the rank's owned cells come first, its ghost cells behind them
template <class S> static int owned_cells(const AmgLevel<S>& L0) { return int(std::count(L0.h_owned.begin(), L0.h_owned.end(), int8_t(1))); }

template <class S> int LinSolver::cpr_levels(int32_t* nlevels, int32_t* n, int64_t* nnz, int32_t* nw)
{
    AmgHierarchy<S>* H = cpr_hierarchy<S>();
    if (!H) return OPMGPU_EINVAL;
    const int nl = int(H->levels.size());
    const int cap = *nlevels;
    *nlevels = nl;
    if (nw) *nw = H->levels[0]->nw;
    for (int l = 0; l < nl && l < cap; ++l) {
        const AmgLevel<S>& F = *H->levels[l];
        int64_t cnt = 2 * int64_t(F.nperf) + F.nw;
        if (l == 0) for (int r = 0; r < F.n; ++r) cnt += plan.rowlen[r];
        else for (int r = 0; r < F.n; ++r) cnt += F.h_rowlen[r];
        if (n) n[l] = F.ntot();
        if (nnz) nnz[l] = cnt;
    }
    return OPMGPU_OK;
}

template <class S> int LinSolver::cpr_level_get(int level, int32_t* rowptr, int32_t* col, double* val, int32_t* agg, double* dense_inv)
{
    AmgHierarchy<S>* H = cpr_hierarchy<S>();
    if (!H || level < 0 || level >= int(H->levels.size())) return OPMGPU_EINVAL;
    const hipStream_t st = stream;
    H->join_inverse();
    const AmgLevel<S>& F = *H->levels[level];
    const int n = F.n, nw = F.nw, nt = F.ntot(), nperf = F.nperf;
    std::vector<int32_t> sp(F.nslices + 1), sc(F.nentries), connpos(nw + 1, 0), perf_row(nperf);
    std::vector<S> sv(F.nentries + 2 * size_t(nperf) + nw);
    OPMGPU_HIP(hipMemcpyAsync(sp.data(), F.slice_ptr, sp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OPMGPU_HIP(hipMemcpyAsync(sc.data(), F.col, sc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    F.val.download(sv.data(), sv.size(), st);
    if (nw) {
        OPMGPU_HIP(hipMemcpyAsync(connpos.data(), F.b_connpos, connpos.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        OPMGPU_HIP(hipMemcpyAsync(perf_row.data(), F.b_perf_row, perf_row.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    const bool last = level + 1 == int(H->levels.size());
    std::vector<int32_t> ag;
    if (!last) { ag.resize(nt); F.agg.download(ag.data(), nt, st); }
    std::vector<double> inv;
    if (last && H->n_coarsest <= 96) { inv.resize(size_t(nt) * nt); H->dense_inv.download(inv.data(), inv.size(), st); }
    OPMGPU_HIP(hipStreamSynchronize(st));
    // numbering of the output: level 0 in caller order (cells), then the wells; coarse levels their own
    std::vector<int32_t> internal(nt), outer(nt);
    for (int i = 0; i < nt; ++i) internal[i] = outer[i] = i;
    if (level == 0) for (int i = 0; i < n; ++i) { internal[i] = plan.pos[i]; outer[plan.pos[i]] = i; }
    // a row's perforations as a chain in ascending perforation index: one border column per well of the cell
    std::vector<int32_t> perf_of(n, -1), perf_nx(nperf, -1), well_of(nperf, 0);
    for (int k = 0; k < nw; ++k) for (int j = connpos[k]; j < connpos[k + 1]; ++j) well_of[j] = k;
    for (int j = nperf - 1; j >= 0; --j) { perf_nx[j] = perf_of[perf_row[j]]; perf_of[perf_row[j]] = j; }
    const S* bcol = sv.data() + F.nentries; const S* crow = bcol + nperf; const S* dw = crow + nperf;
    int64_t q = 0;
    if (rowptr) rowptr[0] = 0;
    auto put = [&](int c, double v) { if (col) col[q] = c < nt ? outer[c] : c; if (val) val[q] = v; ++q; };
    for (int o = 0; o < nt; ++o) {
        const int r = internal[o];
        if (r < n) {
            const int len = level == 0 ? int(plan.rowlen[r]) : F.h_rowlen[r];
            for (int k = 0; k < len; ++k) { const long e = long(sp[r >> 6] + k) * 64 + (r & 63); put(sc[e], double(sv[e])); }
            if (nw) for (int j = perf_of[r]; j >= 0; j = perf_nx[j]) put(n + well_of[j], double(bcol[j]));
        } else {
            const int k = r - n;
            for (int j = connpos[k]; j < connpos[k + 1]; ++j) put(perf_row[j], double(crow[j]));
            put(r, double(dw[k]));
        }
        if (rowptr) rowptr[o + 1] = int32_t(q);
    }
    if (agg && !last) for (int o = 0; o < nt; ++o) agg[o] = ag[internal[o]];
    if (dense_inv && !inv.empty())          // the device keeps it transposed (k_dense_apply): inv[j * n + i] = Ainv(i, j)
        for (int i = 0; i < nt; ++i) for (int j = 0; j < nt; ++j) dense_inv[size_t(outer[i]) * nt + outer[j]] = inv[size_t(j) * nt + i];
    return OPMGPU_OK;
}

// the x / x2 buffers of every level (a cycle swaps them; the solver's captured cycle relies on their roles)
template <class S> static std::vector<std::pair<S*, S*>> cpr_roles(AmgHierarchy<S>& H)
{
    std::vector<std::pair<S*, S*>> r;
    for (auto& L : H.levels) r.emplace_back(L->x.p, L->x2.p);
    return r;
}
template <class S> static void cpr_restore_roles(AmgHierarchy<S>& H, const std::vector<std::pair<S*, S*>>& r)
{
    for (size_t l = 0; l < r.size(); ++l) { H.levels[l]->x.p = r[l].first; H.levels[l]->x2.p = r[l].second; }
}

template <class S> int LinSolver::cpr_vcycle_apply_host(const double* b, double* x)
{
    AmgHierarchy<S>* H = cpr_hierarchy<S>();
    if (!H) return OPMGPU_EINVAL;
    AmgLevel<S>& L0 = *H->levels[0];
    const int n = L0.n, nt = L0.ntot();
    const hipStream_t st = stream;
    std::vector<S> hb(nt), hx(nt);
    // a distributed hierarchy (collective call): the rank's owned cells, then its wells; the ghost rows follow their owners inside the cycle
    const int nown = H->ndist > 0 ? owned_cells(L0) : n;
    for (int i = 0; i < nown; ++i) hb[plan.pos[i]] = S(b[i]);
    for (int k = n; k < nt; ++k) hb[k] = S(b[nown + k - n]);
    DevArray<S> keep; keep.alloc(nt);
    OPMGPU_HIP(hipMemcpyAsync(keep.p, L0.b.p, nt * sizeof(S), hipMemcpyDeviceToDevice, st));
    const auto roles = cpr_roles(*H);
    L0.b.upload(hb.data(), nt, st);
    H->vcycle_graph(nullptr, false);
    OPMGPU_HIP(hipMemcpyAsync(hx.data(), L0.x.p, nt * sizeof(S), hipMemcpyDeviceToHost, st));
    cpr_restore_roles(*H, roles);
    OPMGPU_HIP(hipMemcpyAsync(L0.b.p, keep.p, nt * sizeof(S), hipMemcpyDeviceToDevice, st));
    OPMGPU_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < nown; ++i) x[i] = double(hx[plan.pos[i]]);
    for (int k = n; k < nt; ++k) x[nown + k - n] = double(hx[k]);
    return OPMGPU_OK;
}

// A distributed hierarchy in global numbering (tests/test_gpu_dist_hierarchy.py).  Rows of a distributed level: this rank's owned ones (level 0:
// owned cells in caller order, ids in caller-local numbering with the wells at n_local + k, as opmgpu_cpr_level_get); coarse levels: global
// ids.  agg_gid: the global id of every row's aggregate (-1 on the coarsest level).  A tail level comes back whole.
template <class S> int LinSolver::cpr_dist_level_get(int level, int64_t* counts, int64_t* row_gid, int32_t* rowptr, int64_t* col_gid, double* val, int64_t* agg_gid)
{
    AmgHierarchy<S>* H = cpr_hierarchy<S>();
    if (!H || level < 0 || level >= int(H->levels.size())) return OPMGPU_EINVAL;
    int32_t nl = int32_t(H->levels.size());
    std::vector<int32_t> n(nl); std::vector<int64_t> nnz(nl);
    int st = cpr_levels<S>(&nl, n.data(), nnz.data(), nullptr);
    if (st != OPMGPU_OK) return st;
    const int nt = n[level];
    std::vector<int32_t> rp(nt + 1), cl(nnz[level]), ag(nt, -1);
    std::vector<double> vl(nnz[level]);
    st = cpr_level_get<S>(level, rp.data(), cl.data(), vl.data(), ag.data(), nullptr);
    if (st != OPMGPU_OK) return st;
    const AmgLevel<S>& F = *H->levels[level];
    const bool last = level + 1 == nl;
    auto agg_g = [&](int o) -> int64_t {
        if (last) return -1;
        const AmgLevel<S>& C = *H->levels[level + 1];
        return C.dist ? C.h_gid[ag[o]] : int64_t(ag[o]);
    };
    std::vector<int> rows;
    int64_t cnt = 0;
    const int nown0 = level == 0 && F.dist ? owned_cells(F) : 0;
    for (int o = 0; o < nt; ++o) {
        if (level == 0 && F.dist && o >= nown0 && o < F.n) continue;          // a ghost cell
        rows.push_back(o); cnt += rp[o + 1] - rp[o];
    }
    if (counts) { counts[0] = int64_t(rows.size()); counts[1] = cnt; }
    int64_t q = 0;
    if (rowptr) rowptr[0] = 0;
    for (size_t k = 0; k < rows.size(); ++k) {
        const int o = rows[k];
        if (row_gid) row_gid[k] = (F.dist && level > 0) ? F.h_gid[o] : int64_t(o);
        if (agg_gid) agg_gid[k] = agg_g(o);
        for (int e = rp[o]; e < rp[o + 1]; ++e, ++q) {
            if (col_gid) col_gid[q] = (F.dist && level > 0) ? F.h_gid[cl[e]] : int64_t(cl[e]);
            if (val) val[q] = vl[e];
        }
        if (rowptr) rowptr[k + 1] = int32_t(q);
    }
    return OPMGPU_OK;
}

template <class S> int LinSolver::cpr_apply_host(const double* d3, double* v3, double relax)
{
    AmgHierarchy<S>* H = cpr_hierarchy<S>();
    if (!H) return OPMGPU_EINVAL;
    SolverWork<S>& w = work<S>();
    const auto roles = cpr_roles(*H);
    vec_from_host<S>(d3, VEC_BLOCK_INTERLEAVED, w.p.p);
    cpr_apply<S>(w.p.p, w.y.p, relax, nullptr);
    vec_to_host<S>(w.y.p, VEC_BLOCK_INTERLEAVED, v3);
    cpr_restore_roles(*H, roles);
    return OPMGPU_OK;
}

template <class S> int LinSolver::cpr_elliptic_ilu_apply_host(const double* b, double* x)
{
    AmgHierarchy<S>* H = cpr_hierarchy<S>();
    SolverWork<S>& w = work<S>();
    if (!H || !w.plu.p || !ell.inner || ell.use_amg) return OPMGPU_EINVAL;
    const AmgLevel<S>& L0 = *H->levels[0];
    const int n = L0.n, nt = L0.ntot();
    const hipStream_t st = stream;
    std::vector<S> hb(nt), hx(nt);
    for (int i = 0; i < n; ++i) hb[plan.pos[i]] = S(b[i]);
    for (int k = n; k < nt; ++k) hb[k] = S(b[k]);
    DevArray<S> db, dx; db.alloc(nt); dx.alloc(nt);
    db.upload(hb.data(), nt, st);
    dx.zero(st);
    elliptic_ilu_apply<S>(db.p, dx.p);
    dx.download(hx.data(), nt, st);
    OPMGPU_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) x[i] = double(hx[plan.pos[i]]);
    for (int k = n; k < nt; ++k) x[k] = double(hx[k]);
    return OPMGPU_OK;
}

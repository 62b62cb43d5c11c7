// blackoil_setup.inl -- host-only set-up of BlackoilDevice, included by blackoil.hip: the table blob and its two forms (upload_tables),
// re-planning (rebuild_structure, set_wells), the end-point scaling planes and region tables (build_eps_planes, eps_region_table,
// upload_drainage_eps, get_pcw) and the threshold-pressure plane (upload_thpres_plane, set_threshold_pressures).  No kernel is defined here.

void BlackoilDevice::upload_tables(const opmgpu_tables* t)
{
    // all table arrays live in ONE device blob (8-byte words) so that a kernel can stage them in LDS with one cooperative copy.  Built here
    // is the OFFSET form: every pointer field holds the word offset of its array in the blob (resolve_tables)
    // A deck without a gas phase brings no gas tables (its pointers may be NULL).  No kernel of the oil-water instantiations reads one,
    // but the host code below sizes the blob and reads the regions' end points through them: it gets a stand-in of two rows per region,
    // b_g = mu_g = 1 and SGOF [(0, 0, krow(Swco), 0), (1 - Swco, 0, 0, 0)] (krg = pcgo = 0, Sgl = Sgcr = 0).
    // Lengths the code below expects (whoever adds a gas array: give it its stand-in here):
    //   gas_node_ptr [np + 1] -> ngn = gas_node_ptr[np] nodes;  gas_pg, gas_rvsat, gas_invb_sat, gas_invbmu_sat [ngn]
    //   gas_col_ptr [ngn + 1] -> ngc = gas_col_ptr[ngn] samples; gas_col_rv, gas_col_invb, gas_col_invbmu [ngc]
    //   sgof_ptr [ns + 1] -> nsg = sgof_ptr[ns] rows;            sgof_sg, sgof_krg, sgof_krog, sgof_pcgo [nsg]
    // The constant arrays (zeros, ones) are sized from those counts, not from the region numbers.
    opmgpu_tables standin;
    std::vector<int32_t> si_node, si_col, si_sg;
    std::vector<double> sd_pg, sd_zero, sd_one, sd_crv, sd_sg, sd_krog;
    if (t->active_phases == OPMGPU_PHASES_OIL_WATER) {
        const int np_ = t->n_pvt_regions, ns_ = t->n_sat_regions;
        for (int r = 0; r <= np_; ++r) si_node.push_back(2 * r);                     // two nodes per PVT region
        const int ngn_ = si_node.back();
        for (int n = 0; n <= ngn_; ++n) si_col.push_back(2 * n);                     // two column samples per node
        const int ngc_ = si_col.back();
        for (int r = 0; r <= ns_; ++r) si_sg.push_back(2 * r);                       // two SGOF rows per saturation region
        const int nsg_ = si_sg.back();
        sd_zero.assign(size_t(std::max(std::max(ngn_, ngc_), nsg_)), 0.0); sd_one.assign(size_t(std::max(ngn_, ngc_)), 1.0);
        for (int n = 0; n < ngn_; ++n) { sd_pg.push_back(n % 2 ? 1.0e8 : 1.0e5); sd_crv.push_back(0.0); sd_crv.push_back(1.0); }
        for (int r = 0; r < ns_; ++r) {
            const int a = t->swof_ptr[r];
            sd_sg.push_back(0.0); sd_sg.push_back(1.0 - t->swof_sw[a]);
            sd_krog.push_back(t->swof_krow[a]); sd_krog.push_back(0.0);
        }
        standin = *t;
        standin.gas_node_ptr = si_node.data(); standin.gas_pg = sd_pg.data(); standin.gas_rvsat = sd_zero.data();
        standin.gas_invb_sat = sd_one.data(); standin.gas_invbmu_sat = sd_one.data();
        standin.gas_col_ptr = si_col.data(); standin.gas_col_rv = sd_crv.data(); standin.gas_col_invb = sd_one.data(); standin.gas_col_invbmu = sd_one.data();
        standin.sgof_ptr = si_sg.data(); standin.sgof_sg = sd_sg.data(); standin.sgof_krg = sd_zero.data(); standin.sgof_krog = sd_krog.data();
        standin.sgof_pcgo = sd_zero.data();
        t = &standin;
    }
    DevTables& o = dto_;
    o.t = *t;
    std::vector<double> blob;
    auto upd = [&](const double* src, size_t n) {
        const size_t off = blob.size();
        blob.insert(blob.end(), src, src + n);
        if (n == 0) blob.push_back(0.0);
        return reinterpret_cast<const double*>(off);
    };
    auto upi = [&](const int32_t* src, size_t n) {
        const size_t off = blob.size();
        blob.resize(off + (n + 1) / 2 + 1, 0.0);
        std::memcpy(&blob[off], src, n * sizeof(int32_t));
        return reinterpret_cast<const int32_t*>(off);
    };
    const int np = t->n_pvt_regions, ns = t->n_sat_regions;
    const int non = t->oil_node_ptr[np], ngn = t->gas_node_ptr[np];
    const int noc = t->oil_col_ptr[non], ngc = t->gas_col_ptr[ngn];
    const int nsw = t->swof_ptr[ns], nsg = t->sgof_ptr[ns];
    h_surface_density.assign(t->surface_density, t->surface_density + 3 * size_t(np));
    o.t.surface_density = upd(t->surface_density, 3 * np); o.t.pvtw = upd(t->pvtw, 5 * np);
    o.t.oil_node_ptr = upi(t->oil_node_ptr, np + 1);
    o.t.oil_rs = upd(t->oil_rs, non); o.t.oil_psat = upd(t->oil_psat, non);
    o.t.oil_invb_sat = upd(t->oil_invb_sat, non); o.t.oil_invbmu_sat = upd(t->oil_invbmu_sat, non);
    o.t.oil_col_ptr = upi(t->oil_col_ptr, non + 1);
    o.t.oil_col_p = upd(t->oil_col_p, noc); o.t.oil_col_invb = upd(t->oil_col_invb, noc); o.t.oil_col_invbmu = upd(t->oil_col_invbmu, noc);
    o.t.gas_node_ptr = upi(t->gas_node_ptr, np + 1);
    o.t.gas_pg = upd(t->gas_pg, ngn); o.t.gas_rvsat = upd(t->gas_rvsat, ngn);
    o.t.gas_invb_sat = upd(t->gas_invb_sat, ngn); o.t.gas_invbmu_sat = upd(t->gas_invbmu_sat, ngn);
    o.t.gas_col_ptr = upi(t->gas_col_ptr, ngn + 1);
    o.t.gas_col_rv = upd(t->gas_col_rv, ngc); o.t.gas_col_invb = upd(t->gas_col_invb, ngc); o.t.gas_col_invbmu = upd(t->gas_col_invbmu, ngc);
    o.t.swof_ptr = upi(t->swof_ptr, ns + 1);
    o.t.swof_sw = upd(t->swof_sw, nsw); o.t.swof_krw = upd(t->swof_krw, nsw); o.t.swof_krow = upd(t->swof_krow, nsw); o.t.swof_pcow = upd(t->swof_pcow, nsw);
    o.t.sgof_ptr = upi(t->sgof_ptr, ns + 1);
    o.t.sgof_sg = upd(t->sgof_sg, nsg); o.t.sgof_krg = upd(t->sgof_krg, nsg); o.t.sgof_krog = upd(t->sgof_krog, nsg); o.t.sgof_pcgo = upd(t->sgof_pcgo, nsg);
    // no ROCKTAB: offset 0, whatever the caller's fields hold -- a valid address in every form, read by nobody (rocktab_n == 0)
    o.t.rocktab_p = o.t.rocktab_pvmult = o.t.rocktab_transmult = nullptr;
    if (t->rocktab_n > 0) {
        if (t->rocktab_n < 2) throw HipError(OPMGPU_EINVAL, "ROCKTAB needs at least two rows");
        o.t.rocktab_p = upd(t->rocktab_p, t->rocktab_n); o.t.rocktab_pvmult = upd(t->rocktab_pvmult, t->rocktab_n);
        o.t.rocktab_transmult = upd(t->rocktab_transmult, t->rocktab_n);
    }
    {   // STONE1EX, one exponent per saturation region (NULL: 1.0)
        std::vector<double> eta(size_t(ns), 1.0);
        if (t->stone1_exponent) eta.assign(t->stone1_exponent, t->stone1_exponent + ns);
        o.t.stone1_exponent = upd(eta.data(), ns);
    }
    o.stone_som = nullptr;
    // slopes of every 1-D table (TabX): (y[i+1] - y[i]) / (x[i+1] - x[i]) per segment, segments never cross the tables of a CSR-style array
    auto slopes = [&](const double* x, const double* y, const int32_t* ptr, int ntab) {
        const int n = ptr[ntab];
        std::vector<double> d(size_t(std::max(n, 1)), 0.0);
        for (int t_ = 0; t_ < ntab; ++t_)
            for (int i = ptr[t_]; i + 1 < ptr[t_ + 1]; ++i) d[i] = (y[i + 1] - y[i]) / (x[i + 1] - x[i]);
        return upd(d.data(), size_t(n));
    };
    o.x.swof_dkrw = slopes(t->swof_sw, t->swof_krw, t->swof_ptr, ns); o.x.swof_dkrow = slopes(t->swof_sw, t->swof_krow, t->swof_ptr, ns);
    o.x.swof_dpcow = slopes(t->swof_sw, t->swof_pcow, t->swof_ptr, ns);
    o.x.sgof_dkrg = slopes(t->sgof_sg, t->sgof_krg, t->sgof_ptr, ns); o.x.sgof_dkrog = slopes(t->sgof_sg, t->sgof_krog, t->sgof_ptr, ns);
    o.x.sgof_dpcgo = slopes(t->sgof_sg, t->sgof_pcgo, t->sgof_ptr, ns);
    o.x.oil_drs = slopes(t->oil_psat, t->oil_rs, t->oil_node_ptr, np); o.x.oil_dinvb_sat = slopes(t->oil_psat, t->oil_invb_sat, t->oil_node_ptr, np);
    o.x.oil_dinvbmu_sat = slopes(t->oil_psat, t->oil_invbmu_sat, t->oil_node_ptr, np);
    o.x.oil_col_dinvb = slopes(t->oil_col_p, t->oil_col_invb, t->oil_col_ptr, non); o.x.oil_col_dinvbmu = slopes(t->oil_col_p, t->oil_col_invbmu, t->oil_col_ptr, non);
    o.x.gas_drvsat = slopes(t->gas_pg, t->gas_rvsat, t->gas_node_ptr, np); o.x.gas_dinvb_sat = slopes(t->gas_pg, t->gas_invb_sat, t->gas_node_ptr, np);
    o.x.gas_dinvbmu_sat = slopes(t->gas_pg, t->gas_invbmu_sat, t->gas_node_ptr, np);
    o.x.gas_col_dinvb = slopes(t->gas_col_rv, t->gas_col_invb, t->gas_col_ptr, ngn); o.x.gas_col_dinvbmu = slopes(t->gas_col_rv, t->gas_col_invbmu, t->gas_col_ptr, ngn);
    o.x.oil_pvcdo = nullptr;
    plain_rock_ = o.t;      // (its rock fields: what set_rock_regions(nullptr) puts back)
    h_tab = blob;
    upload_blob(blob);
    // unscaled end points of every saturation region (what opm-material's EclEpsScalingPointsInfo::extractUnscaled reads off the
    // tables): Swl Swcr Swu Sowcr Sgl Sgcr Sgu Sogcr
    h_unscaled.assign(8 * size_t(ns), 0.0);
    for (int r = 0; r < ns; ++r) {
        const int a = t->swof_ptr[r], nw = t->swof_ptr[r + 1] - a, b = t->sgof_ptr[r], ng = t->sgof_ptr[r + 1] - b;
        auto last_zero = [](const double* x, const double* y, int n) { int i = 0; while (i + 1 < n && y[i + 1] == 0.0) ++i; return x[i]; };
        auto first_zero = [](const double* x, const double* y, int n) { int i = 0; while (i < n - 1 && y[i] != 0.0) ++i; return x[i]; };
        double* u = &h_unscaled[8 * size_t(r)];
        u[0] = t->swof_sw[a]; u[1] = last_zero(t->swof_sw + a, t->swof_krw + a, nw); u[2] = t->swof_sw[a + nw - 1];
        u[3] = 1.0 - first_zero(t->swof_sw + a, t->swof_krow + a, nw);
        u[4] = t->sgof_sg[b]; u[5] = last_zero(t->sgof_sg + b, t->sgof_krg + b, ng); u[6] = t->sgof_sg[b + ng - 1];
        u[7] = 1.0 - first_zero(t->sgof_sg + b, t->sgof_krog + b, ng);
    }
    // table maxima the vertical scaling refers to, per region in curve order: krw(Swu), krow(Swl), pcow(Swl), krg(Sgu), krog(Sgl), pcgo(Sgu)
    h_tabmax.assign(6 * size_t(ns), 0.0);
    for (int r = 0; r < ns; ++r) {
        const int a = t->swof_ptr[r], nw = t->swof_ptr[r + 1] - a, b = t->sgof_ptr[r], ng = t->sgof_ptr[r + 1] - b;
        double* m = &h_tabmax[6 * size_t(r)];
        m[0] = t->swof_krw[a + nw - 1]; m[1] = t->swof_krow[a]; m[2] = t->swof_pcow[a];
        m[3] = t->sgof_krg[b + ng - 1]; m[4] = t->sgof_krog[b]; m[5] = t->sgof_pcgo[b + ng - 1];
    }
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// the blob onto the device and, from the offset form dto_, the device-pointer form for the kernels off the Newton path, which read the
// blob where it lies
void BlackoilDevice::upload_blob(const std::vector<double>& blob)
{
    d_tab.upload(blob, stream);
    tab_words = int(blob.size());
    dtp_ = dto_;
    auto rb = [&](auto*& p) { rebase(p, d_tab.p); };
    for_each_table(dtp_, rb, rb);
    if (!dto_.x.oil_pvcdo) dtp_.x.oil_pvcdo = nullptr;      // word 0 of the offset form = no PVCDO rows: NULL to the kernels that branch on it
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// The dead oil of constant compressibility (PVCDO; the rule: include/opmgpu.h at opmgpu_set_pvcdo): one row p_ref, B_ref, C_o, mu_ref, C_v
// per PVT region, appended to the table blob (so a kernel that stages the blob in LDS stages the rows with it); nullptr takes them off
// again.  The tables are no part of the plan or of the state: a re-plan, save / restore and a change of precision leave them alone.
void BlackoilDevice::set_pvcdo(const double* pvcdo)
{
    const int np = dto_.t.n_pvt_regions;
    if (rock_on()) {        // the regions' tables lie where the PVCDO rows would: the two are never set together, so there are no rows to take off either
        if (pvcdo) throw HipError(OPMGPU_EINVAL, "setPvcdo: the context has rock regions (opmgpu_set_rock_regions); the PVCDO oil is not supported with them");
        return;
    }
    std::vector<double> blob = h_tab;
    if (pvcdo) {
        if (drdt_on()) throw HipError(OPMGPU_EINVAL, "setPvcdo: the context has dissolution limits (opmgpu_set_dissolution_limits); the PVCDO oil is not supported with them");
        if (dto_.t.has_disgas) throw HipError(OPMGPU_EINVAL, "setPvcdo: the context has dissolved gas (has_disgas); the PVCDO oil is dead");
        for (int r = 0; r < np; ++r) {
            const double* o = pvcdo + 5 * size_t(r);
            for (int k = 0; k < 5; ++k)
                if (!std::isfinite(o[k])) throw HipError(OPMGPU_EINVAL, "setPvcdo: entry " + std::to_string(k) + " of PVT region " + std::to_string(r) + " is not finite");
            if (!(o[1] > 0.0)) throw HipError(OPMGPU_EINVAL, "setPvcdo: B_ref of PVT region " + std::to_string(r) + " is not positive");
            if (!(o[3] > 0.0)) throw HipError(OPMGPU_EINVAL, "setPvcdo: the reference viscosity of PVT region " + std::to_string(r) + " is not positive");
        }
        dto_.x.oil_pvcdo = reinterpret_cast<const double*>(blob.size());       // a word offset, never 0: the blob begins with the densities
        blob.insert(blob.end(), pvcdo, pvcdo + 5 * size_t(np));
    } else dto_.x.oil_pvcdo = nullptr;
    OPMGPU_HIP(hipStreamSynchronize(stream));        // no kernel in flight reads the blob that upload may replace
    upload_blob(blob);
}

// pattern = stencil U well cliques -> solver plan -> internal numbering of every per-cell array
void BlackoilDevice::rebuild_structure()
{
    std::vector<int32_t> rowptr, col, code;
    const int nw = device_wells ? 0 : int(h_well_connpos.size()) - 1;     // device wells: factored operator, no clique fill
    const int st = build_reservoir_pattern(nc, nconn, h_conn.data(), nw, h_well_connpos.data(), h_well_cells.data(), rowptr, col, code);
    if (st != OPMGPU_OK) throw HipError(st, "invalid grid connections / wells (out of range or duplicate cell pair)");
    // keep the state across a re-plan (wells change between report steps)
    std::vector<double> sp, ssat, srs, srv; std::vector<int8_t> shc;
    std::vector<double> smax;
    // (the hysteresis history likewise, read in the OLD numbering: after set_pattern the plan is the new one)
    std::vector<double> hist;
    if (use_hyst && d_hist.p && has_state) { hist.resize(4 * size_t(nc)); get_hysteresis(hist.data(), hist.data() + nc, hist.data() + 2 * size_t(nc), hist.data() + 3 * size_t(nc)); }
    const bool hyst_carried = !hist.empty();
    if (d_somax.p) { smax.resize(nc); get_sat_oil_max(smax.data()); }
    std::vector<double> caps;       // (the dissolution caps too)
    if (d_somax.p && drdt_on()) { caps.resize(2 * size_t(nc)); get_dissolution_caps(caps.data(), caps.data() + nc); }
    std::vector<double> pmin;       // (and the compaction history of the rock regions)
    if (d_somax.p && rock_on()) { pmin.resize(nc); get_rock_history(pmin.data()); }
    if (has_state) { sp.resize(nc); ssat.resize(3 * size_t(nc)); srs.resize(nc); srv.resize(nc); shc.resize(nc); get_state(sp.data(), ssat.data(), srs.data(), srv.data(), shc.data()); }
    const int st2 = ls.set_pattern(nc, rowptr.data(), col.data(), prm.ilu_ordering);
    if (st2 != OPMGPU_OK) throw HipError(st2, "sparsity plan failed");
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    // per SELL entry: transmissibility with the row's side of the connection in the sign bit (NaN: well fill, 0: diagonal / padding),
    // g (z_c1 - z_c2) of the connection, its threshold pressure (k_assemble_rows reads them coalesced next to the column index)
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> te(P.nentries, 0.0);
        h_entry_conn.assign(P.nentries, -1);
        for (int b = 0; b < P.nnzb; ++b) {
            const int e = P.entry_of_block[b], c = code[b];
            if (c >= 0) {
                const int f = c >> 1;
                te[e] = std::copysign(h_trans[f], (c & 1) ? -1.0 : 1.0);
                h_entry_conn[e] = f;
            } else if (c == -2) te[e] = nan;
        }
        d_tr_e.upload(te, stream);
        upload_thpres_plane();
        // cell depths in internal numbering: g (z_c1 - z_c2) of a connection is formed in the kernel (gravity * (z[c1] - z[c2]), the same
        // expression the reference's geometry evaluates once per face)
        std::vector<double> zi(P.nbp, 0.0);
        for (int r = 0; r < nc; ++r) zi[r] = h_z[P.nat[r]];
        d_zc.upload(zi, stream);
    }
    std::vector<double> pvi(nbp, 1.0); std::vector<int32_t> pn(nbp, 0);
    for (int r = 0; r < nc; ++r) { pvi[r] = h_pv[P.nat[r]]; pn[r] = h_pvtnum[P.nat[r]]; }
    d_pv.upload(pvi, stream); d_pvtnum.upload(pn, stream);
    upload_region_numbers();
    if (use_eps) {
        std::vector<double> planes;
        upload_drainage_eps();
        if (use_hyst) {
            d_ieps_u0.upload(eps_region_table(has_iendpoints || has_endpoints), stream);
            build_eps_planes(has_iendpoints ? h_ieps : h_eps, has_iendpoints || has_endpoints, true, planes);
            d_ieps.upload(planes, stream);
            std::vector<int32_t> im(nbp, 0);
            for (int r = 0; r < nc; ++r) im[r] = h_imbnum[P.nat[r]];
            d_imbnum.upload(im, stream);
            std::vector<double> hp = hist_planes();             // no history
            if (!hist.empty())
                for (int r = 0; r < nc; ++r) for (int k = 0; k < 4; ++k) hp[size_t(k) * nbp + r] = hist[size_t(k) * nc + P.nat[r]];
            d_hist.upload(hp, stream);
        }
    }
    if (dto_.t.threephase_model == OPMGPU_KRO_STONE1) {
        // Som = min(SOWCR, SOGCR) per cell: its scaled end points, or the critical oil saturations read off its region's tables
        std::vector<double> som(nbp, 0.0);
        for (int r = 0; r < nc; ++r) {
            const int c = P.nat[r];
            const double* u = &h_unscaled[8 * size_t(h_satnum[c])];
            som[r] = has_endpoints ? std::min(h_eps[3][c], h_eps[7][c]) : std::min(u[3], u[7]);
        }
        d_stone_som.upload(som, stream);
        dto_.stone_som = dtp_.stone_som = d_stone_som.p;
    }
    std::vector<int32_t> pc(std::max<size_t>(h_well_cells.size(), 1), 0);
    for (size_t i = 0; i < h_well_cells.size(); ++i) pc[i] = P.pos[h_well_cells[i]];
    d_perf_cells.upload(pc, stream);
    nperf = int(h_well_cells.size());
    d_perf.alloc(std::max(nperf, 1) * size_t(OPMGPU_PERF_K));
    DevArray<double>* planes[] = { &d_p, &d_sw, &d_so, &d_sg, &d_rs, &d_rv };
    for (DevArray<double>* a : planes) { a->alloc(nbp); a->zero(stream); }
    d_hc.alloc(nbp); d_hc.zero(stream);
    d_vals.alloc(size_t(VP_COUNT) * nbp); d_vals.zero(stream);
    d_accum0.alloc(3 * size_t(nbp)); d_accum0.zero(stream);
    d_R.alloc(3 * size_t(nbp)); d_R.zero(stream);
    d_bpart.alloc(3 * size_t(grid_for(nc))); d_bpart.zero(stream);
    d_dx.alloc(3 * size_t(nbp)); d_dx.zero(stream);
    d_dx_old.alloc(3 * size_t(nbp)); d_dx_old.zero(stream);
    d_red.alloc(13 * size_t(kMaxRedBlocks) + kRedPart);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    has_dx = false; has_saved = false;
    d_somax.alloc(nbp); d_somax.zero(stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
    resize_somax(drdt_on());
    if (!smax.empty()) set_sat_oil_max(smax.data());
    if (!caps.empty()) set_dissolution_caps(caps.data(), caps.data() + nc);
    if (!pmin.empty()) set_rock_history(pmin.data());
    wells_rebind();
    aquifer_rebind();
    if (has_state) set_state(sp.data(), ssat.data(), srs.data(), srv.data(), shc.data());
    // Killough: the scanning parameters follow from the two history planes in the new numbering (the force path of k_hyst_update)
    if (hyst_carried && hyst_model == OPMGPU_HYST_KILLOUGH) { launch_hyst_update(1); OPMGPU_HIP(hipStreamSynchronize(stream)); }
}

// per region: unscaled fixed points of every curve (u0 | u1).  A set of curves WITHOUT scaled end points keeps the saturation exactly
// (S_u = 0 + (S - 0) * 1: states that sit on a table breakpoint must not move by an ulp), so its region table is zero and
// build_eps_planes writes s0 = 0, k = 1.
std::vector<double> BlackoilDevice::eps_region_table(bool have_points) const
{
    const int ns = dto_.t.n_sat_regions;
    std::vector<double> ureg(size_t(kEpsRegion) * ns, 0.0);
    for (int r = 0; r < ns && have_points; ++r) {
        const double* u = &h_unscaled[8 * size_t(r)];
        double* o = &ureg[size_t(kEpsRegion) * r];
        o[EC_KRW] = u[1]; o[EC_KROW] = u[0] + u[4]; o[EC_PCOW] = u[0]; o[EC_KRG] = u[5]; o[EC_KROG] = u[7]; o[EC_PCGO] = u[4];
        double* m = o + EC_COUNT;   // middle points (SCALECRS): krw 1-Sowcr-Sgl, krow Swcr+Sgl, krg 1-Sogcr-Swl, krog 1-Sgcr-Swl
        m[EC_KRW] = 1.0 - u[3] - u[4]; m[EC_KROW] = u[1] + u[4]; m[EC_PCOW] = 0.0; m[EC_KRG] = 1.0 - u[7] - u[0]; m[EC_KROG] = 1.0 - u[5] - u[0]; m[EC_PCGO] = 0.0;
    }
    return ureg;
}

// the drainage curves' region table and per-cell planes (the maps and the vertical factors, build_eps_planes) from the host copies, for
// the current plan: THE path onto the device for them (rebuild_structure, set_swatinit_scaling)
void BlackoilDevice::upload_drainage_eps()
{
    d_eps_u0.upload(eps_region_table(has_endpoints), stream);
    std::vector<double> planes;
    build_eps_planes(h_eps, has_endpoints, false, planes);
    d_eps.upload(planes, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// each cell's maximum oil-water capillary pressure (caller numbering): its PCW where the context holds vertical scaling of that curve,
// else the first pcow node of its region's SWOF table (also where that node is zero: such a curve is not scaled, build_eps_planes)
void BlackoilDevice::get_pcw(double* pcw) const
{
    for (int c = 0; c < nc; ++c) {
        const double tm = h_tabmax[6 * size_t(h_satnum[c]) + EC_PCOW];
        pcw[c] = (h_eps_v[3].empty() || tm == 0.0) ? tm : h_eps_v[3][c];
    }
}

// per-cell planes [s0 | k | s1 | k1 | v] x 6 curves (internal numbering) for the table of the cell's region `reg_of` against the end
// points ep8 (caller numbering; have_points = false: identity maps); imbibition planes use the IMBNUM region's table
void BlackoilDevice::build_eps_planes(const std::vector<double>* ep8, bool have_points, bool imbibition, std::vector<double>& ep) const
{
    const Plan& P = ls.plan;
    const int nbp = P.nbp;
    ep.assign(size_t(kEpsPlanes) * nbp, 0.0);
    for (int r = 0; r < nbp; ++r) {
        const int c = r < nc ? P.nat[r] : -1;
        // which table: the drainage region, or (planes built for the imbibition curves) the IMBNUM region
        const int reg = c < 0 ? 0 : (imbibition ? h_imbnum[c] : h_satnum[c]);
        const double* u = &h_unscaled[8 * size_t(reg)];
        double e[8];
        for (int k = 0; k < 8; ++k) e[k] = (c < 0 || !have_points) ? u[k] : ep8[k][c];
        const double SWL = e[0], SWCR = e[1], SWU = e[2], SOWCR = e[3], SGL = e[4], SGCR = e[5], SGU = e[6], SOGCR = e[7];
        const double s0[EC_COUNT] = { SWCR, SWL + SGL, SWL, SGCR, SOGCR, SGL };
        const double s1[EC_COUNT] = { 1.0 - SOWCR - SGL, SWCR + SGL, 0.0, 1.0 - SOGCR - SWL, 1.0 - SGCR - SWL, 0.0 };
        const double s2[EC_COUNT] = { SWU, 1.0 - SOWCR - SGL, SWU, SGU, 1.0 - SWL - SGL, SGU };
        const double u0c[EC_COUNT] = { u[1], u[0] + u[4], u[0], u[5], u[7], u[4] };
        const double u1c[EC_COUNT] = { 1.0 - u[3] - u[4], u[1] + u[4], 0.0, 1.0 - u[7] - u[0], 1.0 - u[5] - u[0], 0.0 };
        const double u2c[EC_COUNT] = { u[2], 1.0 - u[3] - u[4], u[2], u[6], 1.0 - u[0] - u[4], u[6] };
        for (int k = 0; k < EC_COUNT && !have_points; ++k) {          // identity map, exact
            ep[size_t(k) * nbp + r] = 0.0; ep[size_t(EC_COUNT + k) * nbp + r] = 1.0; ep[size_t(2 * EC_COUNT + k) * nbp + r] = 1e300; ep[size_t(3 * EC_COUNT + k) * nbp + r] = 1.0;
        }
        for (int k = 0; k < EC_COUNT && have_points; ++k) {
            if (oil_water() && k >= EC_KRG) {       // no gas phase: the gas curves are read by nobody; the identity map, unchecked
                ep[size_t(k) * nbp + r] = 0.0; ep[size_t(EC_COUNT + k) * nbp + r] = 1.0; ep[size_t(2 * EC_COUNT + k) * nbp + r] = 1e300; ep[size_t(3 * EC_COUNT + k) * nbp + r] = 1.0;
                continue;
            }
            if (c >= 0 && !(s2[k] > s0[k])) throw HipError(OPMGPU_EINVAL, "ENDSCALE end points of a cell are not increasing");
            const bool three = scalecrs && have_points && k != EC_PCOW && k != EC_PCGO;
            if (three && c >= 0 && !(s1[k] > s0[k] && s2[k] > s1[k])) throw HipError(OPMGPU_EINVAL, "SCALECRS: a cell's critical saturation is not between its end points");
            ep[size_t(k) * nbp + r] = s0[k];
            ep[size_t(EC_COUNT + k) * nbp + r] = three ? (u1c[k] - u0c[k]) / (s1[k] - s0[k]) : (u2c[k] - u0c[k]) / (s2[k] - s0[k]);
            ep[size_t(2 * EC_COUNT + k) * nbp + r] = three ? s1[k] : 1e300;
            ep[size_t(3 * EC_COUNT + k) * nbp + r] = three ? (u2c[k] - u1c[k]) / (s2[k] - s1[k]) : 1.0;
        }
        // vertical factors: cell maximum / table maximum (KRW at Swu, KRO at Swl resp. Sgl, KRG at Sgu, PCW at Swl, PCG at Sgu)
        double* v[EC_COUNT];
        for (int k = 0; k < EC_COUNT; ++k) { v[k] = &ep[size_t(4 * EC_COUNT + k) * nbp + r]; *v[k] = 1.0; }
        if (c >= 0) {
            const double* tm = &h_tabmax[6 * size_t(reg)];
            const int src[EC_COUNT] = { 0, 1, 3, 2, 1, 4 };     // KRW, KRO, PCW, KRG, KRO, PCG
            for (int k = 0; k < EC_COUNT; ++k) if (!h_eps_v[src[k]].empty() && tm[k] != 0.0) *v[k] = h_eps_v[src[k]][c] / tm[k];
        }
    }
}

int BlackoilDevice::set_wells(int nw, const int32_t* connpos, const int32_t* cells)
{
    if (nw < 0 || (nw > 0 && (!connpos || !cells))) return OPMGPU_EINVAL;
    std::vector<int32_t> cp(1, 0), wc;
    if (nw > 0) { cp.assign(connpos, connpos + nw + 1); wc.assign(cells, cells + connpos[nw]); }
    if (cp == h_well_connpos && wc == h_well_cells) return OPMGPU_OK;
    h_well_connpos = cp; h_well_cells = wc;
    rebuild_structure();
    return OPMGPU_OK;
}

// the per-SELL-entry plane of the connections' threshold pressures (what k_assemble_rows reads next to the column index) from h_thpres
void BlackoilDevice::upload_thpres_plane()
{
    if (!use_thpres) return;
    std::vector<double> he(h_entry_conn.size(), 0.0);
    for (size_t e = 0; e < he.size(); ++e) if (h_entry_conn[e] >= 0) he[e] = h_thpres[h_entry_conn[e]];
    d_thp_e.upload(he, stream);
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

// BlackoilModelBase::setThresholdPressures (BlackoilModelBase_impl.hpp:421-443): the thresholds of ALL connections, in the connection order
// of the grid; nullptr = none.  The host copy is what rebuild_structure() builds the plane from, so a later re-plan (wells) keeps them.
void BlackoilDevice::set_threshold_pressures(const double* thpres)
{
    if (thpres)
        for (int f = 0; f < nconn; ++f)
            if (!(thpres[f] >= 0.0) || !std::isfinite(thpres[f]))
                throw HipError(OPMGPU_EINVAL, "setThresholdPressures: the threshold pressure of connection " + std::to_string(f) + " is negative or not finite");
    use_thpres = thpres != nullptr;
    if (use_thpres) h_thpres.assign(thpres, thpres + nconn);
    else h_thpres.clear();
    upload_thpres_plane();
}

"""Reference for group rate control shared by guide rates (GCONPROD / GCONINJE; opmgpu_set_well_groups).

The sharing rule is the library's own (WellCollection / WellsGroup of opm-core are not in the reference tree); it is stated in
include/opmgpu.h and restated here from that text alone, with every sum taken by math.fsum (exactly rounded):

    r_w = e_w (d_g . qs_w);   I = {w in M_g : current[w] != s_w};   C = M_g \\ I
    w in C:  Gamma   = sum_{v in C} gamma_v,             rem   = max(0, T_g - s_g sum_{v in I} r_v),           target_w = s_g (gamma_w / Gamma)   rem   / e_w
    w in I:  Gamma_w = gamma_w + sum_{v in C} gamma_v,   rem_w = max(0, T_g - s_g sum_{v in I, v != w} r_v),   target_w = s_g (gamma_w / Gamma_w) rem_w / e_w

`slot_targets` is that; `GroupOracleModel` is the oracle's coupled model (through tests/wefac_reference.py, which adds the efficiency
factors) with the rule applied where the reference calls its group logic: before and behind updateWellControls at every assembly
(applyGroupControls of setupGroupControl, updateWellTargets: BlackoilModelBase_impl.hpp:779-792) and behind the control update of every
pre-solve iteration (:1090-1093)."""
import math

import numpy as np

from wefac_reference import WefacOracleModel, arrays  # noqa: F401  (arrays: re-exported for the tests)


def slot_targets(groups, slot, current, qs, eff):
    """groups: objects with sign, target, distr[3], wells, guide (opmgpu.wells.WellGroup); slot[nw] = index of the group slot within each
    well; current[nw]; qs[nw, 3]; eff[nw].  Returns (target[nw] with NaN for a well in no group, terms[nw], group_rate[ngroups]):
    terms[w] = (gamma_w / Gamma_w) (T_g + sum |r_v| over the v the target's remainder sums) / e_w, the magnitude an absolute error
    bound of the target scales with."""
    qs = np.asarray(qs, float)
    nw = qs.shape[0]
    target, terms, rate = np.full(nw, np.nan), np.zeros(nw), np.zeros(len(groups))
    for k, g in enumerate(groups):
        d = [float(x) for x in g.distr]
        r = {w: float(eff[w]) * math.fsum(d[a] * float(qs[w, a]) for a in range(3)) for w in g.wells}
        gam = dict(zip(g.wells, (float(x) for x in g.guide)))
        indiv = [w for w in g.wells if int(current[w]) != int(slot[w])]
        on_slot = [w for w in g.wells if int(current[w]) == int(slot[w])]
        gamma_c = math.fsum(gam[w] for w in on_slot)
        rate[k] = math.fsum(r[w] for w in g.wells)
        for w in g.wells:
            if w in on_slot:
                others, share = indiv, gam[w] / gamma_c
            else:
                others, share = [v for v in indiv if v != w], gam[w] / (gam[w] + gamma_c)
            rem = max(0.0, g.target - g.sign * math.fsum(r[v] for v in others))
            target[w] = g.sign * share * rem / float(eff[w])
            terms[w] = share * (g.target + math.fsum(abs(r[v]) for v in others) + (abs(r[w]) if w in indiv else 0.0)) / float(eff[w])
    return target, terms, rate


class GroupOracleModel(WefacOracleModel):
    """the coupled oracle model with controlled groups: `groups` as for slot_targets, every member's LAST control being its slot"""

    def __init__(self, grid, tables, params, wells, well_state, groups, efficiency=None, dbhp_max_rel=1.0):
        e = np.ones(len(wells.type)) if efficiency is None else np.asarray(efficiency, float)
        super().__init__(grid, tables, params, wells, well_state, e, dbhp_max_rel=dbhp_max_rel)
        self.groups = list(groups)
        self.slot = np.asarray([len(cl) - 1 for cl in self.controls])
        for g in self.groups:
            for w in g.wells:
                typ, _, distr = self.controls[w][-1]
                assert typ == 1 and np.array_equal(distr, g.distr), "a member's last control is not the group's slot"

    def share_group_targets(self):
        target, _, _ = slot_targets(self.groups, self.slot, self.ws.current, self.ws.qs, self.eff)
        for g in self.groups:
            for w in g.wells:
                typ, _, distr = self.controls[w][-1]
                self.controls[w][-1] = (typ, float(target[w]), distr)
        return target

    def update_well_controls(self):
        super().update_well_controls()
        self.share_group_targets()                # updateWellTargets, behind every updateWellControls (:791, :1093)

    def solve_well_eq(self, vals, B_avg):
        converged = super().solve_well_eq(vals, B_avg)
        if not converged:
            self.share_group_targets()            # the well state was put back: the slot targets follow the state they are a function of
        return converged

    def assemble(self, initial):
        self.share_group_targets()                # applyGroupControls (setupGroupControl, :779-783)
        super().assemble(initial)

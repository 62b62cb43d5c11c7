"""SCHEDULE ingest: what `flow_legacy` gets from opm-parser's Schedule + opm-core's WellsManager, restricted to the
keywords a standard-well black-oil run needs:

  WELSPECS  name group I J ref-depth preferred-phase            COMPDAT  name I J K1 K2 OPEN|SHUT satnum CF diameter Kh skin D dir
  WCONPROD  name OPEN|SHUT mode ORAT WRAT GRAT LRAT RESV BHP THP VFP ALQ     WCONINJE  name phase OPEN|SHUT mode RATE RESV BHP THP VFP
  WELOPEN   name OPEN|SHUT|STOP [I J K]                            WELTARG  name ORAT|WRAT|GRAT|LRAT|BHP|THP|RATE value
  WEFAC     name-or-template factor            the well's efficiency factor in (0, 1], in force from its report step on until replaced
            (item 3, the network flag, is not read); GEFAC is refused: groups have no efficiency factor here
  GRUPTREE  child parent                          the group tree; a group WELSPECS or GCONPROD / GCONINJE names without a parent hangs under FIELD
  GCONPROD  group mode ORAT WRAT GRAT LRAT exceed-action ...     mode ORAT | WRAT | GRAT | LRAT with its target, or NONE | FLD (no target of
            its own); exceed action RATE or defaulted
  GCONINJE  group phase mode rate ...             phase WATER | GAS, mode RATE with its target, or NONE | FLD
  WGRUPCON  well YES|NO guide-rate                NO: the well is no member of a controlled group (it runs on its own limits and its rate is
            not counted against the group's target); guide rate defaulted or <= 0: taken from the well potentials (items 4, 5 are not read)
  DRSDT     value [ALL|FREE]                      the largest rate at which Rs of a cell may rise [sm3/sm3/day]; FREE: only in cells that hold
            free gas.  DRVDT value: the same for Rv, no option.  In force from their report step on until replaced; per report step in
            `Schedule.dissolution` (rates per SECOND).  The rule they feed is the device's own (opmgpu_set_dissolution_limits in
            include/opmgpu.h).  ValueError naming the keyword: either one in a deck without GAS, DRSDT without DISGAS, DRVDT without VAPOIL, a
            negative or missing value, an option other than ALL / FREE; and DRSDTR, DRVDTR (regional rates), DRSDTCON (convective
            dissolution), which are not supported
  DATES / TSTEP (report steps), START (RUNSPEC)
  RPTRST    mnemonic list (opmgpu/deck.py:parse_rptrst): REPLACES the list in force (RestartConfig::getRestartKeywords) for the report steps
            that follow it; the SOLUTION section's list holds until then

Every report step gets a `Wells` object (opmgpu/wells.py) the way WellsManager builds opm-core's `Wells` struct: one control per limit
the deck gives, the deck's control mode is the initial current control, the others are the inequality constraints
updateWellControls switches to (StandardWells_impl.hpp:709-800).  Producer rate targets are negative (flow into the wellbore).
A defaulted connection factor is Peaceman's for a vertical well in a block-centred cell (WellsManager::createWellsFromSpecs ->
computeWellIndices, opm-core, external: restated from the published formula).  METRIC units.
Group rate control: a well's CONTROLLING GROUP is its nearest ancestor (its own group first) with an active target of the well's kind
-- a production target controls producers, an injection target the injectors of its phase.  Every member gets the group slot as its last
control and starts on it when its deck mode is GRUP (Wells.add_group; the sharing rule is stated in include/opmgpu.h).  Refused with a
ValueError naming keyword and item: RESV / CRAT / PRBL (GCONPROD), RESV / REIN / VREP (GCONINJE), a rate limit of GCONPROD other than the
mode's own target, an exceed action other than RATE, two ancestors with an active target for one well, GRUP on a well without a
controlling group, a gas group in a deck without GAS, GEFAC.
Not read: WCONHIST, multi-segment wells, horizontal completions (dir X / Y).  A RESV target becomes a
RESERVOIR_RATE control with distr {1, 1, 1}; opmgpu/rateconverter.py's computeRESV gives it the conversion coefficients once per report
step (SimulatorBase_impl.hpp:196, :476-553).
A deck without a gas phase (RUNSPEC: OIL WATER; Deck.phases() == "wo"): a GRAT target (WCONPROD item 6, WELTARG GRAT), a GAS injector and a
THP limit are refused with a ValueError naming them; the RESV control's distr is {1, 1, 0}.
"""
import datetime

import numpy as np

from . import wells as W
from .deck import parse_rptrst
from .decks import BAR, DAY

CP_RM3_PER_DAY_BAR = 1e-3 / (DAY * BAR)         # connection factor: cP rm3 / (day bar) -> SI
MONTHS = {m: i + 1 for i, m in enumerate(["JAN", "FEB", "MAR", "APR", "MAY", "JUN", "JUL", "AUG", "SEP", "OCT", "NOV", "DEC"])}
MONTHS["JLY"] = 7


def _get(rec, i, default=None):
    return rec[i] if len(rec) > i and rec[i] is not None else default


def _date(rec):
    return datetime.date(int(rec[2]), MONTHS[str(rec[1]).upper()[:3]], int(rec[0]))


class WellSpec:
    def __init__(self, name, i, j, ref_depth, phase, group="FIELD"):
        self.name, self.i, self.j, self.ref_depth, self.phase, self.group = name, i, j, ref_depth, phase, group
        self.group_available, self.guide_rate = True, None      # WGRUPCON: available for group control; guide rate (None: from the potentials)
        self.completions = []           # (i, j, k, open, CF or None, diameter, Kh or None, skin)
        self.control = None             # ("PROD", open, mode, limits dict) / ("INJ", phase, open, mode, limits dict)
        self.efficiency = 1.0           # WEFAC


class Schedule:
    def __init__(self, deck, grid, perm_md=None, dz=None, dxdy=None, ntg=None):
        """deck: opmgpu.deck.Deck (already read); grid: the GridData made from it (active_index maps Cartesian -> active cell);
        perm_md = (kx, ky) per Cartesian cell [mD], dz / dxdy = (dx, dy) / ntg per Cartesian cell for the Peaceman factor."""
        self.deck, self.grid = deck, grid
        self.nx, self.ny, self.nz = deck.dims
        self.perm, self.dz, self.dxdy, self.ntg = perm_md, dz, dxdy, ntg
        self.start = _date(deck.records("START")[0]) if deck.has("START") else datetime.date(1983, 1, 1)
        self.two_phase = deck.phases() == "wo"
        self.steps = []                 # [(length in s, {name: WellSpec snapshot})]
        self.rptrst = []                # per report step: {RPTRST mnemonic: int} in force for the restart file written at its end
        self.groups = []                # per report step: {"parent": {group: parent}, "prod": {group: (mode, target)}, "inje": {(group, phase): target}}
        self.dissolution = []           # per report step: (DRSDT rate [1/s] or None, its option FREE, DRVDT rate [1/s] or None)
        self._build()

    def _build(self):
        import copy
        specs = {}
        order = []
        now = self.start
        rptrst = self.deck.rptrst()
        groups = {"parent": {}, "prod": {}, "inje": {}}
        drsdt, free_only, drvdt = None, False, None
        for name, recs in self.deck.schedule:
            if name == "RPTRST":
                rptrst = parse_rptrst(recs[0] if recs else [])
                continue
            if name == "WELSPECS":
                for r in recs:
                    if not r:
                        continue
                    wn = str(r[0])
                    if wn not in specs:
                        order.append(wn)
                    specs[wn] = WellSpec(wn, int(r[2]) - 1, int(r[3]) - 1, _get(r, 4), str(_get(r, 5, "OIL")).upper(), str(_get(r, 1, "FIELD")).upper())
            elif name == "COMPDAT":
                for r in recs:
                    if not r:
                        continue
                    ws = specs[str(r[0])]
                    i = int(_get(r, 1, ws.i + 1) or ws.i + 1) - 1 if _get(r, 1, 0) not in (0, None) else ws.i
                    j = int(_get(r, 2, ws.j + 1) or ws.j + 1) - 1 if _get(r, 2, 0) not in (0, None) else ws.j
                    direction = str(_get(r, 12, "Z")).upper()
                    if direction != "Z":
                        raise ValueError("COMPDAT %s: only vertical completions (direction Z) are supported" % ws.name)
                    for k in range(int(r[3]) - 1, int(r[4])):
                        ws.completions = [c for c in ws.completions if (c[0], c[1], c[2]) != (i, j, k)]
                        ws.completions.append((i, j, k, str(_get(r, 5, "OPEN")).upper() == "OPEN", _get(r, 7), _get(r, 8, 0.3048), _get(r, 9), _get(r, 10, 0.0)))
                    ws.completions.sort(key=lambda c: c[2])
            elif name == "WCONPROD":
                for r in recs:
                    if not r:
                        continue
                    lim = {"ORAT": _get(r, 3), "WRAT": _get(r, 4), "GRAT": _get(r, 5), "LRAT": _get(r, 6), "RESV": _get(r, 7), "BHP": _get(r, 8, 1.01325),
                           "THP": _get(r, 9), "VFP": int(_get(r, 10, 0) or 0), "ALQ": _get(r, 11, 0.0)}
                    if self.two_phase:
                        self._refuse_gas("WCONPROD", str(r[0]), GRAT=lim["GRAT"], THP=lim["THP"], mode=str(_get(r, 2, "")).upper())
                    for wn in self._match(specs, str(r[0])):
                        specs[wn].control = ("PROD", str(_get(r, 1, "OPEN")).upper() == "OPEN", str(_get(r, 2, "")).upper(), lim)
            elif name == "WCONINJE":
                for r in recs:
                    if not r:
                        continue
                    lim = {"RATE": _get(r, 4), "RESV": _get(r, 5), "BHP": _get(r, 6, 6895.0), "THP": _get(r, 7), "VFP": int(_get(r, 8, 0) or 0)}
                    if self.two_phase:
                        self._refuse_gas("WCONINJE", str(r[0]), GAS=True if str(r[1]).upper() == "GAS" else None, THP=lim["THP"],
                                         mode=str(_get(r, 3, "")).upper())
                    for wn in self._match(specs, str(r[0])):
                        specs[wn].control = ("INJ", str(r[1]).upper(), str(_get(r, 2, "OPEN")).upper() == "OPEN", str(_get(r, 3, "")).upper(), lim)
            elif name == "WELOPEN":          # name OPEN|SHUT|STOP [I J K C1 C2]: the whole well, or the completions that match (defaults / 0 = any)
                for r in recs:
                    if not r:
                        continue
                    status = str(_get(r, 1, "OPEN")).upper()
                    sel = [int(_get(r, q, 0) or 0) for q in (2, 3, 4)]
                    for wn in self._match(specs, str(r[0])):
                        ws = specs[wn]
                        if any(v > 0 for v in sel):
                            ws.completions = [(ci, cj, ck, status == "OPEN" if all(v <= 0 or v - 1 == c for v, c in zip(sel, (ci, cj, ck))) else op, cf, dia, kh, sk)
                                              for (ci, cj, ck, op, cf, dia, kh, sk) in ws.completions]
                        elif ws.control is not None:
                            c = list(ws.control)
                            c[2 if c[0] == "INJ" else 1] = status == "OPEN"          # STOP (shut above the formation) is treated as SHUT: no crossflow model
                            ws.control = tuple(c)
            elif name == "WEFAC":            # name-or-template factor: resolved like WELOPEN's names, but a name that matches no well is an error
                for r in recs:
                    if not r:
                        continue
                    if len(r) < 2 or r[1] is None:
                        raise ValueError("WEFAC %s: the record has no efficiency factor" % r[0])
                    try:
                        e = float(r[1])
                    except (TypeError, ValueError):
                        raise ValueError("WEFAC %s: efficiency factor %r is not a number" % (r[0], r[1]))
                    if not (np.isfinite(e) and 0.0 < e <= 1.0):
                        raise ValueError("WEFAC %s: efficiency factor %r is outside (0, 1]" % (r[0], r[1]))
                    matched = [wn for wn in self._match(specs, str(r[0])) if wn in specs]
                    if not matched:
                        raise ValueError("WEFAC %s: unknown well (no WELSPECS before it names or matches it)" % r[0])
                    for wn in matched:
                        specs[wn].efficiency = e
            elif name in ("DRSDT", "DRVDT"):
                rate, opt = self._dissolution_rate(name, recs)
                if name == "DRSDT":
                    drsdt, free_only = rate, opt == "FREE"
                else:
                    drvdt = rate
            elif name in ("DRSDTR", "DRVDTR", "DRSDTCON"):
                raise ValueError("%s: %s is not supported (DRSDT / DRVDT set one rate for the whole field)"
                                 % (name, "convective dissolution" if name == "DRSDTCON" else "a rate per region"))
            elif name == "GEFAC":
                raise ValueError("GEFAC: group efficiency factors are not supported (WEFAC sets a well's factor)")
            elif name == "GRUPTREE":
                for r in recs:
                    if r:
                        groups["parent"][str(r[0]).upper()] = str(_get(r, 1, "FIELD")).upper()
            elif name == "GCONPROD":
                for r in recs:
                    if r:
                        self._gconprod(groups, r)
            elif name == "GCONINJE":
                for r in recs:
                    if r:
                        self._gconinje(groups, r)
            elif name == "WGRUPCON":
                for r in recs:
                    if not r:
                        continue
                    avail = str(_get(r, 1, "YES")).upper()
                    if avail not in ("YES", "NO", "Y", "N"):
                        raise ValueError("WGRUPCON %s: item 2 (available for group control) is %r, not YES or NO" % (r[0], avail))
                    gr = _get(r, 2)
                    matched = [wn for wn in self._match(specs, str(r[0])) if wn in specs]
                    if not matched:
                        raise ValueError("WGRUPCON %s: unknown well (no WELSPECS before it names or matches it)" % r[0])
                    for wn in matched:
                        specs[wn].group_available = avail.startswith("Y")
                        specs[wn].guide_rate = float(gr) if gr is not None and float(gr) > 0.0 else None
            elif name == "WELTARG":          # name control value: one limit of the current WCONPROD / WCONINJE record changed
                for r in recs:
                    if not r:
                        continue
                    key, val = str(r[1]).upper(), float(r[2])
                    if self.two_phase:
                        self._refuse_gas("WELTARG", str(r[0]), mode=key)
                    for wn in self._match(specs, str(r[0])):
                        ws = specs[wn]
                        if ws.control is None:
                            raise ValueError("WELTARG %s before WCONPROD / WCONINJE" % wn)
                        lim = dict(ws.control[-1])
                        if ws.control[0] == "INJ" and key in ("ORAT", "WRAT", "GRAT"):
                            key = "RATE"
                        if key not in lim:
                            raise ValueError("WELTARG %s: control %s is not supported" % (wn, key))
                        lim[key] = val
                        ws.control = ws.control[:-1] + (lim,)
            elif name == "DATES":
                for r in recs:
                    if not r:
                        continue
                    d = _date(r)
                    self.steps.append(((d - now).days * DAY, copy.deepcopy({n: specs[n] for n in order})))
                    self.rptrst.append(dict(rptrst))
                    self.groups.append(copy.deepcopy(groups))
                    self.dissolution.append((drsdt, free_only, drvdt))
                    now = d
            elif name == "TSTEP":
                for r in recs:
                    for dt in r:
                        self.steps.append((float(dt) * DAY, copy.deepcopy({n: specs[n] for n in order})))
                        self.rptrst.append(dict(rptrst))
                        self.groups.append(copy.deepcopy(groups))
                        self.dissolution.append((drsdt, free_only, drvdt))
                        now = now + datetime.timedelta(days=float(dt))

    def _dissolution_rate(self, name, recs):
        """DRSDT value [ALL|FREE] / DRVDT value -> (rate per second, option); METRIC: the value is per day"""
        r = recs[0] if recs else []
        if self.two_phase:
            raise ValueError("%s in a deck without GAS (RUNSPEC: OIL WATER)" % name)
        need = "DISGAS" if name == "DRSDT" else "VAPOIL"
        if not self.deck.has(need):
            raise ValueError("%s in a deck without %s" % (name, need))
        v = _get(r, 0)
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s: item 1, the rate, is %r, not a number" % (name, v))
        if not np.isfinite(v) or v < 0.0:
            raise ValueError("%s: item 1, the rate %r, is negative or not finite" % (name, v))
        opt = str(_get(r, 1, "ALL")).upper()
        if name == "DRVDT":
            if _get(r, 1) is not None:
                raise ValueError("DRVDT: item 2 (%r): DRVDT has no option" % r[1])
        elif opt not in ("ALL", "FREE"):
            raise ValueError("DRSDT: item 2, the option, is %r, not ALL or FREE" % opt)
        return v / DAY, opt

    PROD_DISTR = {"ORAT": (0.0, 1.0, 0.0), "WRAT": (1.0, 0.0, 0.0), "GRAT": (0.0, 0.0, 1.0), "LRAT": (1.0, 1.0, 0.0)}
    INJE_DISTR = {"WATER": (1.0, 0.0, 0.0), "GAS": (0.0, 0.0, 1.0)}

    def _gconprod(self, groups, r):
        """GCONPROD: 1 group, 2 mode, 3-6 ORAT WRAT GRAT LRAT, 7 exceed action, (8-13 not read), 14 RESV"""
        g, mode = str(r[0]).upper(), str(_get(r, 1, "NONE")).upper()
        if mode in ("RESV", "CRAT", "PRBL"):
            raise ValueError("GCONPROD %s: item 2, control mode %s, is not supported (ORAT, WRAT, GRAT, LRAT, NONE or FLD)" % (g, mode))
        if mode not in ("ORAT", "WRAT", "GRAT", "LRAT", "NONE", "FLD"):
            raise ValueError("GCONPROD %s: item 2, control mode %r, is unknown" % (g, mode))
        items = {"ORAT": 2, "WRAT": 3, "GRAT": 4, "LRAT": 5, "RESV": 13}
        for key, i in items.items():
            if key != mode and _get(r, i) is not None:
                raise ValueError("GCONPROD %s: item %d, a %s limit next to control mode %s, is not supported (only the mode's own target)" % (g, i + 1, key, mode))
        action = str(_get(r, 6, "RATE")).upper()
        if action != "RATE":
            raise ValueError("GCONPROD %s: item 7, exceed action %s, is not supported (RATE or defaulted)" % (g, action))
        if mode in ("NONE", "FLD"):
            groups["prod"].pop(g, None)
            return
        if self.two_phase and mode == "GRAT":
            raise ValueError("GCONPROD %s: item 2, GRAT, in a deck without GAS (RUNSPEC: OIL WATER)" % g)
        target = _get(r, items[mode])
        if target is None or not np.isfinite(float(target)) or float(target) < 0.0:
            raise ValueError("GCONPROD %s: item %d, the %s target, is missing or negative" % (g, items[mode] + 1, mode))
        groups["prod"][g] = (mode, float(target))
        groups["parent"].setdefault(g, "FIELD")

    def _gconinje(self, groups, r):
        """GCONINJE: 1 group, 2 phase, 3 mode, 4 surface rate target"""
        g, phase, mode = str(r[0]).upper(), str(_get(r, 1, "")).upper(), str(_get(r, 2, "NONE")).upper()
        phase = "WATER" if phase == "WAT" else phase
        if mode in ("RESV", "REIN", "VREP"):
            raise ValueError("GCONINJE %s: item 3, control mode %s, is not supported (RATE, NONE or FLD)" % (g, mode))
        if mode not in ("RATE", "NONE", "FLD"):
            raise ValueError("GCONINJE %s: item 3, control mode %r, is unknown" % (g, mode))
        if phase not in ("WATER", "GAS"):
            raise ValueError("GCONINJE %s: item 2, phase %r, is not supported (WATER or GAS)" % (g, phase))
        if self.two_phase and phase == "GAS":
            raise ValueError("GCONINJE %s: item 2, GAS, in a deck without GAS (RUNSPEC: OIL WATER)" % g)
        if mode in ("NONE", "FLD"):
            groups["inje"].pop((g, phase), None)
            return
        target = _get(r, 3)
        if target is None or not np.isfinite(float(target)) or float(target) < 0.0:
            raise ValueError("GCONINJE %s: item 4, the RATE target, is missing or negative" % g)
        groups["inje"][(g, phase)] = float(target)
        groups["parent"].setdefault(g, "FIELD")

    def group_tree(self, step):
        """{group: parent} of report step `step`: GRUPTREE, and FIELD as the parent of every other group a well or a target names"""
        G = self.groups[step]
        tree = dict(G["parent"])
        for ws in self.steps[step][1].values():
            tree.setdefault(ws.group, "FIELD")
        for g in list(tree.values()):
            if g != "FIELD":
                tree.setdefault(g, "FIELD")
        tree.pop("FIELD", None)
        return tree

    def controlling_group(self, step, group, kind):
        """the nearest ancestor of `group` (itself first) with an active target of `kind` ("PROD", or the injection phase "WATER" / "GAS"):
        (name, sign, target in SI, distr) or None.  Two such ancestors: ValueError."""
        G, tree = self.groups[step], self.group_tree(step)
        found, g, seen = [], group, set()
        while g is not None and g not in seen:
            seen.add(g)
            if kind == "PROD" and g in G["prod"]:
                mode, t = G["prod"][g]
                found.append((g, -1.0, t / DAY, self.PROD_DISTR[mode]))
            elif kind != "PROD" and (g, kind) in G["inje"]:
                found.append((g, 1.0, G["inje"][(g, kind)] / DAY, self.INJE_DISTR[kind]))
            g = tree.get(g) if g != "FIELD" else None
        if len(found) > 1:
            kw = "GCONPROD" if kind == "PROD" else "GCONINJE"
            raise ValueError("%s: groups %s and %s, one above the other, both have an active target (item %d); nested targets are not supported"
                             % (kw, found[0][0], found[1][0], 2 if kind == "PROD" else 3))
        return found[0] if found else None

    @staticmethod
    def _refuse_gas(keyword, well, mode="", **items):
        """a deck without a gas phase: no gas rate target, no gas injector, no THP limit (its VFP tables have a gas-fraction axis)"""
        for name, value in list(items.items()) + [(mode, True if mode in ("GRAT", "THP") else None)]:
            if value is not None:
                raise ValueError("%s %s: %s in a deck without GAS (RUNSPEC: OIL WATER)" % (keyword, well, name))

    @staticmethod
    def _match(specs, pattern):
        if pattern.endswith("*"):
            return [n for n in specs if n.startswith(pattern[:-1])]
        return [pattern]

    def _peaceman(self, cart, diameter, skin):
        """connection factor of a vertical well in a block-centred cell [SI]: 2 pi sqrt(kx ky) dz ntg / (ln(r0 / rw) + skin),
        r0 = 0.28 sqrt(sqrt(ky/kx) dx^2 + sqrt(kx/ky) dy^2) / ((ky/kx)^(1/4) + (kx/ky)^(1/4))"""
        from .decks import MD
        kx, ky = self.perm[0][cart] * MD, self.perm[1][cart] * MD
        dx, dy, dz = self.dxdy[0][cart], self.dxdy[1][cart], self.dz[cart]
        r0 = 0.28 * np.sqrt(np.sqrt(ky / kx) * dx ** 2 + np.sqrt(kx / ky) * dy ** 2) / ((ky / kx) ** 0.25 + (kx / ky) ** 0.25)
        return 2.0 * np.pi * np.sqrt(kx * ky) * dz * (self.ntg[cart] if self.ntg is not None else 1.0) / (np.log(r0 / (0.5 * diameter)) + skin)

    def wells(self, step):
        """The `Wells` of report step `step` (open wells with open completions in active cells only; order of WELSPECS)."""
        out = W.Wells()
        act = np.asarray(self.grid.active_index)
        members = {}                    # controlling group -> [(well index, guide rate or NaN, starts on GRUP)], in the wells' order
        for name, ws in self.steps[step][1].items():
            if ws.control is None:
                continue
            is_inj = ws.control[0] == "INJ"
            is_open = ws.control[2] if is_inj else ws.control[1]
            if not is_open:
                continue
            cells, wi = [], []
            for (i, j, k, copen, cf, diam, kh, skin) in ws.completions:
                cart = i + self.nx * (j + self.ny * k)
                if not copen or act[cart] < 0:
                    continue
                cells.append(int(act[cart]))
                wi.append(cf * CP_RM3_PER_DAY_BAR if cf is not None else self._peaceman(cart, diam, skin))
            if not cells:
                continue
            ref = ws.ref_depth if ws.ref_depth is not None else float(self.grid.z[cells[0]])
            if is_inj:
                _, phase, _, mode, lim = ws.control
                comp = {"WATER": (1.0, 0.0, 0.0), "WAT": (1.0, 0.0, 0.0), "OIL": (0.0, 1.0, 0.0), "GAS": (0.0, 0.0, 1.0)}[phase]
                ctrls = {}
                if lim["RATE"] is not None:
                    ctrls["RATE"] = (W.SURFACE_RATE, lim["RATE"] / DAY, comp)
                if lim["RESV"] is not None:          # distr {1, 1, 1} until SimulatorBase::computeRESV fills in the conversion coefficients
                    ctrls["RESV"] = (W.RESERVOIR_RATE, lim["RESV"] / DAY, (1.0, 1.0, 0.0 if self.two_phase else 1.0))
                if lim["BHP"] is not None:
                    ctrls["BHP"] = (W.BHP, lim["BHP"] * BAR)
                if lim["THP"] is not None and lim["VFP"] > 0:
                    ctrls["THP"] = (W.THP, lim["THP"] * BAR, None, lim["VFP"], 0.0)
                kind = "WATER" if phase == "WAT" else phase
                wtype = W.INJECTOR
            else:
                _, _, mode, lim = ws.control
                comp = (0.0, 1.0, 0.0)
                ctrls = {}
                for key, distr in (("ORAT", (0.0, 1.0, 0.0)), ("WRAT", (1.0, 0.0, 0.0)), ("GRAT", (0.0, 0.0, 1.0)), ("LRAT", (1.0, 1.0, 0.0))):
                    if lim[key] is not None:
                        ctrls[key] = (W.SURFACE_RATE, -lim[key] / DAY, distr)
                if lim["RESV"] is not None:
                    ctrls["RESV"] = (W.RESERVOIR_RATE, -lim["RESV"] / DAY, (1.0, 1.0, 0.0 if self.two_phase else 1.0))
                if lim["BHP"] is not None:
                    ctrls["BHP"] = (W.BHP, lim["BHP"] * BAR)
                if lim["THP"] is not None and lim["VFP"] > 0:
                    ctrls["THP"] = (W.THP, lim["THP"] * BAR, None, lim["VFP"], lim["ALQ"] or 0.0)
                if mode == "CRAT":
                    raise ValueError("WCONPROD %s: control mode %s is not supported" % (name, mode))
                kind = "PROD"
                wtype = W.PRODUCER
            keyword = "WCONINJE" if is_inj else "WCONPROD"
            ctl = self.controlling_group(step, ws.group, kind) if ws.group_available and kind in ("PROD", "WATER", "GAS") else None
            if mode == "GRUP":
                if ctl is None:
                    raise ValueError("%s %s: item %d, control mode GRUP, but the well has no controlling group (no ancestor of group %s has an "
                                     "active target for it%s)" % (keyword, name, 4 if is_inj else 3, ws.group, "" if ws.group_available else "; WGRUPCON makes it unavailable"))
                if not ctrls:
                    raise ValueError("%s %s: control mode GRUP needs at least one limit of the well's own (a BHP limit)" % (keyword, name))
            elif mode not in ctrls:
                raise ValueError("well %s: control mode %r has no target in the deck" % (name, mode))
            if ctl is not None:
                members.setdefault(ctl, []).append((out.nw, float("nan") if ws.guide_rate is None else ws.guide_rate, mode == "GRUP"))
            # WellsManager's fixed order (ORAT, WRAT, GRAT, LRAT, [RESV], BHP, THP; injectors RATE, [RESV], BHP, THP) with the deck's
            # control mode as the index of the current control: updateWellControls switches to the FIRST broken constraint, so the
            # order decides which one wins when two are broken (and the index goes into the restart file)
            order = list(ctrls.values())
            out.add_well(name, wtype, ref, cells, wi, comp, order[0], limits=order[1:], current=0 if mode == "GRUP" else list(ctrls).index(mode),
                         efficiency=ws.efficiency)
        # the controlled groups in the order of their first member: the slot behind every member's own controls, GRUP wells on it
        for (gname, sign, target, distr), mem in members.items():
            out.add_group(gname, sign, target, distr, [m[0] for m in mem], [m[1] for m in mem], on_group=[m[0] for m in mem if m[2]])
        return out

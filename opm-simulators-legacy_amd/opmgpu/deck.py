"""Minimal ECLIPSE deck ingest for the hot path's static inputs.

What `flow_legacy` gets from opm-parser + `DerivedGeology` (opm/autodiff/GeoProps.hpp:84-195) + `BlackoilPropsAdFromDeck`
(opm/autodiff/BlackoilPropsAdFromDeck.cpp:60-240), restricted to what the device path consumes:

  RUNSPEC   DIMENS TABDIMS EQLDIMS OIL WATER GAS DISGAS VAPOIL METRIC ENDSCALE EQLOPTS (THPRES; IRREVERS is refused)
            The active phases are the ones RUNSPEC names: OIL WATER GAS, or OIL WATER -- a deck without a gas phase (Deck.phases() ==
            "wo").  Such a deck needs and reads no gas keyword (PVTG / PVDG, SGOF, the gas end points and KRG / PCG, a gas DENSITY);
            DISGAS, VAPOIL, VAPPARS, STONE / STONE1 / STONE2, SATOPTS HYSTER and SGAS / RS / RV in SOLUTION are refused (ValueError
            naming the keyword); its initial oil saturation is 1 - Sw.  Oil-gas, gas-water and single-phase decks are refused.  A deck
            that names none of the three (a fragment) counts as three-phase.
  GRID      DX DY DZ / DXV DYV DZV, TOPS (+BOX for the top layer) or DEPTHZ (flat) -- or COORD / ZCORN (corner-point, no faults) --, PORO PERMX PERMY PERMZ NTG ACTNUM MINPV, FAULTS + MULTFLT
            MULTX MULTY MULTZ MULTX- MULTY- MULTZ- MULTPV NNC
  PROPS     SWOF SGOF PVTO PVDO PVCDO PVTG PVDG PVTW DENSITY ROCK ROCKTAB VAPPARS SCALECRS (NO and YES) EHYSTR
            ROCK / ROCKTAB: the first record, for every cell -- unless RUNSPEC holds ROCKCOMP (REVERS or IRREVERS; item 2 the number of
            rock tables): then every record is read, ROCKOPTS item 3 (PVTNUM, SATNUM or ROCKNUM) names the region array that picks a
            cell's record, and `rock_regions()` returns them for GpuBlackoilModel.setRockRegions (the rule is stated in include/opmgpu.h)
            PVCDO: one record per PVT region (TABDIMS; too few is a ValueError).  With Co = Cv = 0 in every record it is a constant
            two-node dead-oil table; otherwise the tables carry the rows as `FluidTables.pvcdo` (SI) next to that table as a stand-in,
            and the device evaluates the oil in closed form (opmgpu_set_pvcdo; the rule is stated in include/opmgpu.h).  Not with DISGAS.
            STONE1 STONE2 STONE (= STONE2) STONE1EX: the three-phase oil relative permeability model (none of them: the default model;
            two of them, or one together with SATOPTS HYSTER, is refused)
            SWL SWCR SWU SOWCR SGL SGCR SGU SOGCR  KRW KRO KRG PCW PCG  ISWL ISWCR ISWU ISOWCR ISGL ISGCR ISGU ISOGCR
            SWATINIT (an imposed initial water saturation per cell; read like SWL, `swatinit()`; EQUIL then rescales each cell's PCW,
            opmgpu/equil.py; needs EQUIL and a water phase)
            (SATOPTS HYSTER in RUNSPEC switches the hysteresis on; EHYSTR item 2 = 0 -- Carlson -- or 2 -- Killough, with item 4 its
            curvature parameter -- and item 5 = KR, relative permeabilities only, are the models the device implements:
            `hysteresis_model()`; items 1 and 3 are read past, the wetting-phase models 1, 3, 4 are refused)
  REGIONS   ROCKNUM (with ROCKCOMP and ROCKOPTS item 3 = ROCKNUM)
            PVTNUM SATNUM IMBNUM FIPNUM (fluid-in-place regions of computeFluidInPlace; 1-based in the deck and in `fipnum()`)
            EQLNUM (equilibration regions: EQUIL's, and the regions THPRES puts barriers between; 1-based in `eqlnum()`)
  SOLUTION  PRESSURE SWAT SGAS RS RV (explicit initial state; EQUIL is outside the hot path)
            THPRES (threshold pressures between EQLNUM regions, with EQLOPTS THPRES in RUNSPEC: `thpres()` / `threshold_pressures()`
            restate opm/simulators/thresholdPressures.hpp:320-417; a defaulted item 3 takes the model's computeMaxDp of the initial state)
            RPTRST (the mnemonics that select derived per-cell arrays for the restart file, RPTRST_MNEMONICS; also read in SCHEDULE)
            AQUFETP AQUCT AQUANCON, with AQUTAB in PROPS and AQUDIMS in RUNSPEC read past (analytic aquifers: `aquifers()`, which states
            the items read and the refusals; AQUFLUX, AQUNUM and AQUCON are refused)

Block-centred Cartesian geometry only (corner-point COORD/ZCORN needs opm-grid's processing, out of scope).  TPFA
transmissibilities as `tpfa_htrans_compute` / `tpfa_trans_compute` do for such cells: half-transmissibility
K A / (d/2) per side (horizontal ones times NTG, DerivedGeology :135-160), harmonic sum, times the MULT? of the face.
Everything else (SUMMARY, other report keywords) is skipped; SCHEDULE is kept in deck order for opmgpu/schedule.py (which reads, among the
rest, DRSDT / DRVDT: the limits on re-dissolution and re-vaporisation).  METRIC units only.
"""
import re

import numpy as np

from . import capi, decks
from .decks import BAR, DAY, FluidTables, GridData, MD, State

FLAG_KEYWORDS = {"RUNSPEC", "GRID", "EDIT", "PROPS", "REGIONS", "SOLUTION", "SUMMARY", "SCHEDULE", "END", "NOECHO", "ECHO", "OIL", "WATER",
                 "GAS", "DISGAS", "VAPOIL", "METRIC", "FIELD", "LAB", "FMTOUT", "FMTIN", "UNIFOUT", "UNIFIN", "RUNSUM", "SEPARATE", "ALL",
                 "INIT", "NOSIM", "ENDBOX", "EXCEL", "NOGGF", "NEWTRAN", "OLDTRAN", "STONE", "STONE1", "STONE2"}
# RPTRST mnemonics that select arrays of the model's output record (getRestartData, SimulatorFullyImplicitBlackoilOutput.hpp:585-845);
# BASIC and every other mnemonic are not kept
RPTRST_MNEMONICS = ("BW", "BO", "BG", "DEN", "VISC", "VWAT", "VOIL", "VGAS", "KRW", "KRO", "KRG", "RSSAT", "RVSAT", "PBPD")
_KW = re.compile(r"^[A-Z][A-Z0-9_+\-]{0,7}$")
EPS_NAMES = GridData.EPS_NAMES


def _tokens(text):
    """comment-stripped tokens; quoted strings stay single tokens; '/' is its own token"""
    out = []
    for line in text.splitlines():
        # cut '--' comments outside quotes
        q, cut = False, len(line)
        for i, ch in enumerate(line):
            if ch == "'":
                q = not q
            elif not q and line.startswith("--", i):
                cut = i
                break
        line = line[:cut]
        toks = re.findall(r"'[^']*'|/|[^\s/']+", line)
        out.append(toks)
    return out


def _expand(tok):
    """'3*0.2' -> [0.2]*3 ; '2*' -> [None]*2 ; number / string otherwise"""
    m = re.match(r"^(\d+)\*(.*)$", tok)
    if m:
        n, v = int(m.group(1)), m.group(2)
        return [(_value(v) if v != "" else None)] * n
    return [_value(tok)]


def _value(tok):
    if tok.startswith("'"):
        return tok.strip("'")
    try:
        return float(tok.replace("D", "E").replace("d", "e"))
    except ValueError:
        return tok


def parse_rptrst(record):
    """One RPTRST record -> {mnemonic: int} over RPTRST_MNEMONICS (absent = 0).  Items are NAME or NAME=int (also written NAME = int); a bare
    name counts as 1.  A record of integers only (the old positional form) selects none of them."""
    items, toks, i = {}, [str(t) for t in record if t is not None], 0
    words = []
    for t in toks:                       # 'DEN', 'BASIC=2', 'BASIC', '=', '2', 'BASIC=', '2', ...
        words.extend(w for w in re.split(r"(=)", t) if w != "")
    while i < len(words):
        name = words[i].upper()
        if i + 2 < len(words) and words[i + 1] == "=":
            value, i = int(float(words[i + 2])), i + 3
        else:
            value, i = 1, i + 1
        if name in RPTRST_MNEMONICS:
            items[name] = value
    return {k: items.get(k, 0) for k in RPTRST_MNEMONICS}


class Deck:
    def __init__(self, keywords, schedule=None, solution_rptrst=None):
        self.kw = keywords              # name -> list of records (each a list of values), last occurrence wins; BOX-scoped ones keep their box
        self.schedule = schedule or []  # SCHEDULE section in deck order: [(keyword, records)], every occurrence (opmgpu/schedule.py)
        self._solution_rptrst = solution_rptrst      # records of the last RPTRST before SCHEDULE (self.kw keeps the deck's last one only)

    def rptrst(self):
        """The RPTRST mnemonics in force when the SCHEDULE begins (parse_rptrst; all 0 without the keyword)."""
        recs = self._solution_rptrst
        return parse_rptrst(recs[0] if recs else [])

    def has(self, name):
        return name in self.kw

    def records(self, name):
        return self.kw[name]["records"]

    def array(self, name, n=None, default=None):
        if name not in self.kw:
            return default
        v = [x for x in self.kw[name]["records"][0]]
        a = np.asarray([np.nan if x is None else x for x in v], dtype=float)
        if n is not None and a.size != n:
            raise ValueError("%s holds %d values, expected %d" % (name, a.size, n))
        return a

    # ---------------------------------------------------------------- RUNSPEC
    @property
    def dims(self):
        r = self.records("DIMENS")[0]
        return int(r[0]), int(r[1]), int(r[2])

    def tabdims(self):
        r = self.records("TABDIMS")[0] if self.has("TABDIMS") else []
        get = lambda i, d: int(r[i]) if len(r) > i and r[i] is not None else d
        return get(0, 1), get(1, 1)          # NTSFUN, NTPVT

    def phases(self):
        """"wog", or "wo" for a deck whose RUNSPEC names OIL and WATER but not GAS; every other set of phases is refused"""
        if getattr(self, "_phases", None) is None:
            self._phases = self._find_phases()           # once per deck: the refusals are not re-run by every caller
        return self._phases

    def _find_phases(self):
        named = [k for k in ("OIL", "WATER", "GAS") if self.has(k)]
        if not named or len(named) == 3:
            return "wog"
        if named != ["OIL", "WATER"]:
            raise ValueError("RUNSPEC names the phases %s: only OIL WATER GAS and OIL WATER are supported" % " ".join(named))
        for k in ("DISGAS", "VAPOIL", "VAPPARS", "STONE", "STONE1", "STONE2"):
            if self.has(k):
                raise ValueError("%s in a deck without GAS (RUNSPEC: OIL WATER)" % k)
        if self.has("SATOPTS") and any(str(x).upper().startswith("HYST") for r in self.records("SATOPTS") for x in r):
            raise ValueError("SATOPTS HYSTER in a deck without GAS (RUNSPEC: OIL WATER) is not supported")
        return "wo"

    # ---------------------------------------------------------------- PROPS
    def tables(self):
        if self.has("FIELD") or self.has("LAB"):
            raise ValueError("only METRIC decks are supported")
        ntsfun, ntpvt = self.tabdims()
        two_phase = self.phases() == "wo"
        # deck order oil water gas -> (w, o, g); a deck without GAS may leave the gas density out
        dens = [[r[1], r[0], r[2] if len(r) > 2 and r[2] is not None else 0.0] for r in self.records("DENSITY")[:ntpvt]]
        pvtw = [[r[0], r[1], r[2], r[3], r[4] if len(r) > 4 and r[4] is not None else 0.0] for r in self.records("PVTW")[:ntpvt]]
        disgas, vapoil = self.has("DISGAS"), self.has("VAPOIL")
        pvcdo = None            # PVCDO rows (deck units) when any of them has a non-zero compressibility or viscosibility
        # oil
        if self.has("PVTO"):
            pvto = []
            for tab in _split_tables(self.records("PVTO")):
                rows = []
                for rec in tab:
                    rs, rest = rec[0], rec[1:]
                    rows.append((rs, [tuple(rest[i:i + 3]) for i in range(0, len(rest), 3)]))
                pvto.append(rows)
        elif self.has("PVDO"):
            pvto = [[(0.0, [tuple(rec[i:i + 3])]) for i in range(0, len(rec), 3)] for rec in self.records("PVDO")[:ntpvt]]
            disgas = False
        elif self.has("PVCDO"):
            # constant compressibility dead oil, one record per PVT region.  Co = Cv = 0 everywhere (the reference's tests/fluid.data): two
            # nodes far apart reproduce it, a plain table.  Otherwise the tables cannot express it: FluidTables(pvcdo=...) carries the rows
            # to opmgpu_set_pvcdo and keeps the same two-node table as a stand-in
            recs = self.records("PVCDO")
            if len(recs) < ntpvt:
                raise ValueError("PVCDO holds %d records, expected one per PVT region (%d)" % (len(recs), ntpvt))
            pvto = []
            for r in recs[:ntpvt]:
                pref, bo, co, mu = r[0], r[1], r[2], r[3]
                cv = r[4] if len(r) > 4 and r[4] is not None else 0.0
                if pvcdo is None and (co != 0.0 or cv != 0.0):
                    pvcdo = []
                pvto.append([(0.0, [(pref, bo, mu)]), (0.0, [(pref + 800.0, bo, mu)])])
            if pvcdo is not None:
                if disgas:
                    raise ValueError("PVCDO (a dead oil) in a deck with DISGAS")
                pvcdo = [[r[0], r[1], r[2], r[3], r[4] if len(r) > 4 and r[4] is not None else 0.0] for r in recs[:ntpvt]]
            disgas = False
        else:
            raise ValueError("no oil PVT keyword (PVTO / PVDO / PVCDO)")
        # gas
        if two_phase:
            pvtg = None
        elif self.has("PVTG"):
            pvtg = []
            for tab in _split_tables(self.records("PVTG")):
                rows = []
                for rec in tab:
                    pg, rest = rec[0], rec[1:]
                    rows.append((pg, [tuple(rest[i:i + 3]) for i in range(0, len(rest), 3)]))
                pvtg.append(rows)
        elif self.has("PVDG"):
            pvtg = [[(rec[i], [(0.0, rec[i + 1], rec[i + 2])]) for i in range(0, len(rec), 3)] for rec in self.records("PVDG")[:ntpvt]]
            vapoil = False
        else:
            raise ValueError("no gas PVT keyword (PVTG / PVDG)")
        swof = [[tuple(rec[i:i + 4]) for i in range(0, len(rec), 4)] for rec in self.records("SWOF")[:ntsfun]]
        sgof = None if two_phase else [[tuple(rec[i:i + 4]) for i in range(0, len(rec), 4)] for rec in self.records("SGOF")[:ntsfun]]
        rock = (1.0, 0.0)
        if self.has("ROCK"):
            r = self.records("ROCK")[0]
            rock = (r[0], r[1])
        rocktab = None
        if self.has("ROCKTAB"):
            rec = self.records("ROCKTAB")[0]
            ncol = 5 if len(rec) % 5 == 0 and len(rec) % 3 != 0 else 3
            rocktab = [(rec[i], rec[i + 1], rec[i + 2]) for i in range(0, len(rec), ncol)]
        vappars = (0.0, 0.0)
        if self.has("VAPPARS"):
            r = self.records("VAPPARS")[0]
            vappars = (r[0], r[1])
        model, eta = self.threephase()
        oil = {} if pvcdo is None else {"pvcdo": pvcdo}        # (a PVCDO deck with Co = Cv = 0 passes nothing: the tables it always made)
        if two_phase:
            return FluidTables(density_wog=dens, pvtw=pvtw, pvto=pvto, pvtg=None, swof=swof, sgof=None, rock=rock, rocktab=rocktab, phases="wo",
                               **oil)
        return FluidTables(density_wog=dens, pvtw=pvtw, pvto=pvto, pvtg=pvtg, swof=swof, sgof=sgof, rock=rock, disgas=disgas, vapoil=vapoil,
                           vappars=vappars, rocktab=rocktab, threephase_model=model, stone1_exponent=eta, **oil)

    def threephase(self):
        """(opmgpu_tables.threephase_model, STONE1EX exponents or None): STONE1 -> Stone I with one exponent per saturation region (STONE1EX,
        default 1), STONE2 or STONE -> Stone II, none of them -> the default model."""
        named = [k for k in ("STONE1", "STONE2", "STONE") if self.has(k)]
        if not named:
            return capi.KRO_DEFAULT, None
        if len(named) > 1:
            raise ValueError("more than one three-phase model keyword: " + " ".join(named))
        if self.hysteresis():
            raise ValueError("%s together with SATOPTS HYSTER is not supported" % named[0])
        if named[0] != "STONE1":
            return capi.KRO_STONE2, None
        ntsfun = self.tabdims()[0]
        eta = [1.0] * ntsfun
        if self.has("STONE1EX"):
            recs = self.records("STONE1EX")
            if len(recs) < ntsfun:
                raise ValueError("STONE1EX holds %d records, expected one per saturation region (%d)" % (len(recs), ntsfun))
            eta = [float(r[0]) if len(r) > 0 and r[0] is not None else 1.0 for r in recs[:ntsfun]]
            if any(not e > 0.0 for e in eta):
                raise ValueError("STONE1EX: the exponent must be positive")
        return capi.KRO_STONE1, eta

    # ---------------------------------------------------------------- GRID
    # ---------------------------------------------------------------- corner-point geometry (COORD / ZCORN)
    def _corner_point(self):
        """Geometry of a corner-point grid WITHOUT faults: what the reference takes from opm-grid (processEclipseFormat + compute_geometry; a
        dependency outside its tree) for `DerivedGeology` (GeoProps.hpp:84-195), restated from the published algorithm: a cell is the
        hexahedron of its eight corners (the ZCORN depths on the four COORD pillars around it); every face is triangulated about the mean
        of its four nodes (area vector = sum of the triangle normals, centroid = area-weighted mean of the triangle centroids), the cell
        about the mean of its face centroids (volume = sum of the tetrahedra, centroid = volume-weighted mean).  Neighbouring columns
        whose shared pillar depths differ (faults) are connected cell by cell through the OVERLAP of their faces on the common pillar pair
        (`_fault_connections`); gaps between layers of one column are refused.
        Pinned only by consistency: the corner-point description of a block-centred grid reproduces the DX / DY / DZ / TOPS result
        (tests/test_deck_ingest.py)."""
        if getattr(self, "_cp", None) is not None:
            return self._cp
        nx, ny, nz = self.dims
        coord = self.array("COORD", 6 * (nx + 1) * (ny + 1)).reshape(ny + 1, nx + 1, 6)
        zc = self.array("ZCORN", 8 * nx * ny * nz).reshape(nz, 2, ny, 2, nx, 2)            # (k, top/bottom, j, y-side, i, x-side)
        # corner coordinates P[k, j, i, tb, ys, xs, xyz]
        P = np.zeros((nz, ny, nx, 2, 2, 2, 3))
        for ys in (0, 1):
            for xs in (0, 1):
                pil = coord[ys:ys + ny, xs:xs + nx]                                        # pillar of that corner, [ny, nx, 6]
                for tb in (0, 1):
                    z = zc[:, tb, :, ys, :, xs]                                            # [nz, ny, nx]
                    dzp = pil[..., 5] - pil[..., 2]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        t = np.where(dzp != 0.0, (z - pil[..., 2]) / dzp, 0.0)
                    P[:, :, :, tb, ys, xs, 0] = pil[..., 0] + t * (pil[..., 3] - pil[..., 0])
                    P[:, :, :, tb, ys, xs, 1] = pil[..., 1] + t * (pil[..., 4] - pil[..., 1])
                    P[:, :, :, tb, ys, xs, 2] = z
        # faults: neighbouring columns whose shared pillar depths differ are connected through the overlaps of their faces (_fault_connections)
        tol = 1e-6 * max(1.0, float(np.abs(P[..., 2]).max()))
        fault_x = (np.abs(P[:, :, :-1, :, :, 1] - P[:, :, 1:, :, :, 0]).max(axis=(0, 3, 4, 5)) > tol) if nx > 1 else np.zeros((ny, 0), bool)      # [ny, nx-1]
        fault_y = (np.abs(P[:, :-1, :, :, 1] - P[:, 1:, :, :, 0]).max(axis=(0, 3, 4, 5)) > tol) if ny > 1 else np.zeros((0, nx), bool)            # [ny-1, nx]
        if nz > 1 and np.abs(P[:-1, :, :, 1] - P[1:, :, :, 0]).max() > tol:
            raise ValueError("corner-point grid with gaps between layers: not supported")

        def face(a, b, c, d):                        # nodes in order around the face, each [..., 3]
            m = 0.25 * (a + b + c + d)
            nodes = (a, b, c, d)
            N = np.zeros_like(m); cw = np.zeros_like(m); aw = np.zeros(m.shape[:-1])
            for q in range(4):
                u, v = nodes[q] - m, nodes[(q + 1) % 4] - m
                tn = 0.5 * np.cross(u, v)
                ta = np.linalg.norm(tn, axis=-1)
                N += tn; aw += ta
                cw += ta[..., None] * (m + nodes[q] + nodes[(q + 1) % 4]) / 3.0
            return cw / np.maximum(aw, 1e-300)[..., None], N, (m, nodes)
        c = lambda tb, ys, xs: P[:, :, :, tb, ys, xs]                                      # noqa: E731
        faces = {"x-": face(c(0, 0, 0), c(0, 1, 0), c(1, 1, 0), c(1, 0, 0)), "x+": face(c(0, 0, 1), c(0, 1, 1), c(1, 1, 1), c(1, 0, 1)),
                 "y-": face(c(0, 0, 0), c(0, 0, 1), c(1, 0, 1), c(1, 0, 0)), "y+": face(c(0, 1, 0), c(0, 1, 1), c(1, 1, 1), c(1, 1, 0)),
                 "z-": face(c(0, 0, 0), c(0, 0, 1), c(0, 1, 1), c(0, 1, 0)), "z+": face(c(1, 0, 0), c(1, 0, 1), c(1, 1, 1), c(1, 1, 0))}
        inner = sum(f[0] for f in faces.values()) / 6.0
        vol = np.zeros(inner.shape[:-1]); cen = np.zeros_like(inner)
        for fc, _, (m, nodes) in faces.values():
            for q in range(4):
                a, b = nodes[q], nodes[(q + 1) % 4]
                tv = np.abs(np.einsum("...i,...i->...", np.cross(a - inner, b - inner), m - inner)) / 6.0
                vol += tv
                cen += tv[..., None] * (inner + a + b + m) / 4.0
        cen /= np.maximum(vol, 1e-300)[..., None]
        ext = lambda lo, hi: np.linalg.norm(faces[hi][0] - faces[lo][0], axis=-1)           # noqa: E731  (cube dimensions between face centroids)
        self._cp = dict(vol=vol, cen=cen, faces=faces, dx=ext("x-", "x+"), dy=ext("y-", "y+"), dz=ext("z-", "z+"), ztop=faces["z-"][0][..., 2], zbot=faces["z+"][0][..., 2],
                        P=P, fault_x=fault_x, fault_y=fault_y)
        return self._cp

    @staticmethod
    def _face_overlap(A, B):
        """Overlap of two faces that lie between the same two pillars.  A, B: [2 (top, bottom), 2 (pillar), 3] corner points.  In the
        pillar-pair plane a face is the region between its top edge and its bottom edge, both straight from pillar 0 (u = 0) to pillar 1
        (u = 1); the overlap is the region between the deeper of the two top edges and the shallower of the two bottom edges where that
        gap is positive -- one interval of u, because the gap is concave in u.  Returns (area vector, centroid) or None."""
        lines = {"tA": A[0], "bA": A[1], "tB": B[0], "bB": B[1]}                  # name -> [2 (u = 0, 1), 3]
        zat = lambda name, u: lines[name][0][2] + u * (lines[name][1][2] - lines[name][0][2])       # noqa: E731
        us = {0.0, 1.0}
        names = list(lines)
        for a in range(4):
            for b in range(a + 1, 4):
                la, lb = lines[names[a]], lines[names[b]]
                d0, d1 = la[0][2] - lb[0][2], la[1][2] - lb[1][2]
                if d0 * d1 < 0.0:
                    us.add(d0 / (d0 - d1))
        us = sorted(us)
        gap = lambda u: min(zat("bA", u), zat("bB", u)) - max(zat("tA", u), zat("tB", u))            # noqa: E731
        eps = 1e-12 * max(1.0, abs(A[0][0][2]))
        pos = [u for u in us if gap(u) > eps]
        if not pos:
            return None
        lo, hi = us.index(pos[0]), us.index(pos[-1])
        u0 = us[lo - 1] if lo > 0 and gap(us[lo - 1]) > -eps else pos[0]           # the zero of the gap next to the positive stretch is a breakpoint
        u1 = us[hi + 1] if hi + 1 < len(us) and gap(us[hi + 1]) > -eps else pos[-1]
        span = [u for u in us if u0 <= u <= u1]
        if len(span) < 2 and gap(span[0]) <= eps:
            return None

        def pt(name, u):
            return lines[name][0] + u * (lines[name][1] - lines[name][0])
        upper = [pt("tA" if zat("tA", u) >= zat("tB", u) else "tB", u) for u in span]
        lower = [pt("bA" if zat("bA", u) <= zat("bB", u) else "bB", u) for u in reversed(span)]
        poly = []
        for q in upper + lower:
            if not poly or np.abs(q - poly[-1]).max() > eps:
                poly.append(q)
        if len(poly) > 1 and np.abs(poly[0] - poly[-1]).max() <= eps:
            poly.pop()
        if len(poly) < 3:
            return None
        poly = np.array(poly)
        m = poly.mean(0)
        N = np.zeros(3); cw = np.zeros(3); aw = 0.0
        for q in range(len(poly)):
            a, b = poly[q], poly[(q + 1) % len(poly)]
            tn = 0.5 * np.cross(a - m, b - m)
            ta = np.linalg.norm(tn)
            N += tn; aw += ta; cw += ta * (m + a + b) / 3.0
        if aw <= 0.0:
            return None
        return N, cw / aw

    def _fault_connections(self, cp, perm, ntg, mult, mult_minus, direction):
        """connections across the faulted column pairs of one direction: [(cell a, cell b, transmissibility)] with a on the - side"""
        nx, ny, nz = self.dims
        P, cen = cp["P"], cp["cen"]
        out = []
        mask = cp["fault_x"] if direction == "x" else cp["fault_y"]
        for j, i in zip(*np.nonzero(mask)):
            ja, ia, jb, ib = (j, i, j, i + 1) if direction == "x" else (j, i, j + 1, i)
            for ka in range(nz):
                # face of A towards B / of B towards A as [top / bottom][pillar 0 / 1]
                if direction == "x":
                    FA = np.array([[P[ka, ja, ia, tb, ys, 1] for ys in (0, 1)] for tb in (0, 1)])
                else:
                    FA = np.array([[P[ka, ja, ia, tb, 1, xs] for xs in (0, 1)] for tb in (0, 1)])
                for kb in range(nz):
                    if direction == "x":
                        FB = np.array([[P[kb, jb, ib, tb, ys, 0] for ys in (0, 1)] for tb in (0, 1)])
                    else:
                        FB = np.array([[P[kb, jb, ib, tb, 0, xs] for xs in (0, 1)] for tb in (0, 1)])
                    if FB[0, :, 2].min() >= FA[1, :, 2].max() or FB[1, :, 2].max() <= FA[0, :, 2].min():
                        continue                                                      # depth ranges do not meet
                    ov = self._face_overlap(FA, FB)
                    if ov is None:
                        continue
                    N, cf = ov
                    a, b = ia + nx * (ja + ny * ka), ib + nx * (jb + ny * kb)
                    h = []
                    for (kk, jj, ii), cell in (((ka, ja, ia), a), ((kb, jb, ib), b)):
                        cvec = cf - cen[kk, jj, ii]
                        h.append(abs(float(np.dot(cvec * perm[kk, jj, ii], N))) / float(np.dot(cvec, cvec)) * ntg[cell])
                    if h[0] <= 0.0 or h[1] <= 0.0:
                        continue
                    t = 1.0 / (1.0 / h[0] + 1.0 / h[1])
                    if mult is not None and not np.isnan(mult[a]):
                        t *= mult[a]
                    if mult_minus is not None and not np.isnan(mult_minus[b]):
                        t *= mult_minus[b]
                    out.append((a, b, t))
        return out

    def _cell_sizes(self):
        nx, ny, nz = self.dims
        n = nx * ny * nz
        if self.has("ZCORN"):
            cp = self._corner_point()
            return cp["dx"], cp["dy"], cp["dz"]

        def axis(full, vec, count, shape):
            if self.has(full):
                return self.array(full, n).reshape(nz, ny, nx)
            v = self.array(vec, count)
            return np.broadcast_to(v.reshape(shape), (nz, ny, nx)).copy()
        dx = axis("DX", "DXV", nx, (1, 1, nx)); dy = axis("DY", "DYV", ny, (1, ny, 1)); dz = axis("DZ", "DZV", nz, (nz, 1, 1))
        return dx, dy, dz

    def _face_multipliers(self):
        """MULTX / MULTX- / ... arrays combined with the fault multipliers: FAULTS (name I1 I2 J1 J2 K1 K2 face) names sets of cell faces,
        MULTFLT (name factor) multiplies the transmissibility of every connection through them (regular faces and the overlaps of a
        faulted corner-point pillar pair alike).  {"X": per-cell factor of its X+ face, "X-": of its X- face, ...}"""
        nx, ny, nz = self.dims
        n = nx * ny * nz
        out = {}
        for key in ("X", "X-", "Y", "Y-", "Z", "Z-"):
            a = self.array("MULT" + key, n)
            out[key] = np.ones(n) if a is None else np.where(np.isnan(a), 1.0, a)
        if self.has("FAULTS") and self.has("MULTFLT"):
            fac = {}
            for r in self.records("MULTFLT"):
                if r:
                    fac[str(r[0]).upper()] = fac.get(str(r[0]).upper(), 1.0) * float(r[1])
            idx = np.arange(n).reshape(nz, ny, nx)
            for r in self.records("FAULTS"):
                if not r or str(r[0]).upper() not in fac:
                    continue
                i1, i2, j1, j2, k1, k2 = (int(v) for v in r[1:7])
                face = str(r[7]).upper().replace("I", "X").replace("J", "Y").replace("K", "Z")
                cells = idx[k1 - 1:k2, j1 - 1:j2, i1 - 1:i2].ravel()
                out[face][cells] *= fac[str(r[0]).upper()]
        return out

    def grid(self, gravity=decks.GRAVITY):
        """GridData of the active cells: connections x- then y- then z-normal faces (grid face order), then the NNCs."""
        nx, ny, nz = self.dims
        n = nx * ny * nz
        dx, dy, dz = self._cell_sizes()
        cp = self._corner_point() if self.has("ZCORN") else None
        if cp is not None:
            top = None
        elif self.has("TOPS"):
            t = self.array("TOPS")
            top = t[:nx * ny].reshape(ny, nx) if t.size >= nx * ny else np.full((ny, nx), t[0])
        elif self.has("DEPTHZ"):
            top = np.full((ny, nx), self.array("DEPTHZ")[0])
        else:
            top = np.zeros((ny, nx))
        if cp is not None:
            zc = cp["cen"][..., 2].ravel()
        else:
            ztop = top[None, :, :] + np.concatenate([np.zeros((1, ny, nx)), np.cumsum(dz, axis=0)[:-1]], axis=0)
            zc = (ztop + 0.5 * dz).ravel()
        poro = self.array("PORO", n, np.full(n, 0.0))
        ntg = self.array("NTG", n, np.ones(n))
        kx = self.array("PERMX", n, np.zeros(n)) * MD
        ky = self.array("PERMY", n, kx / MD) * MD
        kz = self.array("PERMZ", n, kx / MD) * MD
        multpv = self.array("MULTPV", n, np.ones(n))
        act = self.array("ACTNUM", n, np.ones(n)) > 0
        vol = cp["vol"].ravel() if cp is not None else (dx * dy * dz).ravel()
        pv = poro * ntg * multpv * vol
        minpv = float(self.records("MINPV")[0][0]) if self.has("MINPV") and self.records("MINPV")[0] else 0.0
        act &= (pv > 0.0) & (pv >= minpv)                          # MINPV: cells below it are inactive (no PINCH connection across them)
        idx = np.arange(n).reshape(nz, ny, nx)
        dxr, dyr, dzr = dx.ravel(), dy.ravel(), dz.ravel()

        def faces(a, b, kperm, area_a, area_b, da, db, horiz, mult, mult_minus):
            a, b = a.ravel(), b.ravel()
            h1 = kperm[a] * area_a[a] / (da[a] / 2.0); h2 = kperm[b] * area_b[b] / (db[b] / 2.0)
            if horiz:
                h1, h2 = h1 * ntg[a], h2 * ntg[b]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = 1.0 / (1.0 / h1 + 1.0 / h2)
            t = np.where(np.isfinite(t), t, 0.0)
            if mult is not None:
                t = t * np.where(np.isnan(mult[a]), 1.0, mult[a])              # MULTX: the face towards +x of the cell it is given for
            if mult_minus is not None:
                t = t * np.where(np.isnan(mult_minus[b]), 1.0, mult_minus[b])  # MULTX-: the face towards -x of that cell
            return np.stack([a, b], 1), t
        ayz, axz, axy = dyr * dzr, dxr * dzr, dxr * dyr
        fm = self._face_multipliers()
        if cp is not None:
            # tpfa_htrans_compute (opm-core, restated): hT = |c . K n| / (c . c) with c = face centroid - cell centroid, n = the face's area
            # vector, K the diagonal permeability tensor; NTG on the horizontal faces (DerivedGeology, GeoProps.hpp:121-159)
            perm = np.stack([kx, ky, kz], -1).reshape(nz, ny, nx, 3)

            def cp_faces(a, b, lo, hi, horiz, mult, mult_minus):
                def half(sel, which):
                    fc, N, _ = cp["faces"][which]
                    cvec = fc[sel] - cp["cen"][sel]
                    h = np.abs(np.einsum("...i,...i->...", cvec * perm[sel], N[sel])) / np.einsum("...i,...i->...", cvec, cvec)
                    return h.ravel()
                sa = (slice(None, -1) if lo == "z+" else slice(None), slice(None, -1) if lo == "y+" else slice(None), slice(None, -1) if lo == "x+" else slice(None))
                sb = (slice(1, None) if lo == "z+" else slice(None), slice(1, None) if lo == "y+" else slice(None), slice(1, None) if lo == "x+" else slice(None))
                a, b = a.ravel(), b.ravel()
                h1, h2 = half(sa, lo), half(sb, hi)
                if horiz:
                    h1, h2 = h1 * ntg[a], h2 * ntg[b]
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = 1.0 / (1.0 / h1 + 1.0 / h2)
                t = np.where(np.isfinite(t), t, 0.0)
                if mult is not None:
                    t = t * np.where(np.isnan(mult[a]), 1.0, mult[a])
                if mult_minus is not None:
                    t = t * np.where(np.isnan(mult_minus[b]), 1.0, mult_minus[b])
                return np.stack([a, b], 1), t
            cx, tx = cp_faces(idx[:, :, :-1], idx[:, :, 1:], "x+", "x-", True, fm["X"], fm["X-"])
            cy, ty = cp_faces(idx[:, :-1, :], idx[:, 1:, :], "y+", "y-", True, fm["Y"], fm["Y-"])
            cz, tz = cp_faces(idx[:-1, :, :], idx[1:, :, :], "z+", "z-", False, fm["Z"], fm["Z-"])
            # faulted column pairs: their layer-to-layer faces do not coincide; the connections come from the face overlaps instead
            tx = np.where(np.broadcast_to(cp["fault_x"][None], (nz,) + cp["fault_x"].shape).ravel(), 0.0, tx)
            ty = np.where(np.broadcast_to(cp["fault_y"][None], (nz,) + cp["fault_y"].shape).ravel(), 0.0, ty)
            fc = (self._fault_connections(cp, perm, ntg, fm["X"], fm["X-"], "x") + self._fault_connections(cp, perm, ntg, fm["Y"], fm["Y-"], "y"))
            if fc:
                cz = np.concatenate([cz, np.array([[a, b] for a, b, _ in fc], dtype=cz.dtype)])
                tz = np.concatenate([tz, np.array([t for _, _, t in fc])])
        else:
            cx, tx = faces(idx[:, :, :-1], idx[:, :, 1:], kx, ayz, ayz, dxr, dxr, True, fm["X"], fm["X-"])
            cy, ty = faces(idx[:, :-1, :], idx[:, 1:, :], ky, axz, axz, dyr, dyr, True, fm["Y"], fm["Y-"])
            cz, tz = faces(idx[:-1, :, :], idx[1:, :, :], kz, axy, axy, dzr, dzr, False, fm["Z"], fm["Z-"])
        conn = np.concatenate([cx, cy, cz]); trans = np.concatenate([tx, ty, tz])
        n_faces = conn.shape[0]
        if self.has("NNC"):
            for r in self.records("NNC"):
                if not r:
                    continue
                c1 = int(r[0]) - 1 + nx * (int(r[1]) - 1) + nx * ny * (int(r[2]) - 1)
                c2 = int(r[3]) - 1 + nx * (int(r[4]) - 1) + nx * ny * (int(r[5]) - 1)
                conn = np.concatenate([conn, [[c1, c2]]]); trans = np.concatenate([trans, [r[6] * decks.CP * 1.0 / (DAY * BAR)]])
        newid = -np.ones(n, dtype=np.int64); newid[act] = np.arange(int(act.sum()))
        keep = act[conn[:, 0]] & act[conn[:, 1]] & (trans > 0.0)
        conn = newid[conn[keep]]; trans = trans[keep]
        self.active = np.flatnonzero(act)
        reg = lambda name: None if not self.has(name) else (self.array(name, n)[act].astype(np.int32) - 1)
        eps = self.endpoints()
        if eps is not None:
            eps = {k: v[act] for k, v in eps.items()}
        more = {}
        if eps is not None and self.has("SCALECRS") and str(self.records("SCALECRS")[0][0]).upper().startswith("Y"):
            more["scalecrs"] = True
        ev = {k: self.array(k, n)[act] * (BAR if k.startswith("PC") else 1.0) for k in GridData.EPSV_NAMES
              if self.has(k) and not (self.phases() == "wo" and k in ("KRG", "PCG"))}
        if ev:
            if any(np.isnan(v).any() for v in ev.values()):
                raise ValueError("vertical scaling arrays (KRW KRO KRG PCW PCG) must be given for every cell")
            more["eps_v"] = ev
        if self.hysteresis():
            imb = reg("IMBNUM")
            more["imbnum"] = imb if imb is not None else (reg("SATNUM") if reg("SATNUM") is not None else np.zeros(int(act.sum()), np.int32))
            ieps = self.endpoints(prefix="I", regions="IMBNUM")
            if ieps is not None and any(self.has("I" + k) for k in EPS_NAMES):
                more["ieps"] = {k: v[act] for k, v in ieps.items()}
        g = GridData(int(act.sum()), conn, trans, pv[act], zc[act], gravity=gravity, pvtnum=reg("PVTNUM"), satnum=reg("SATNUM"),
                     dims=(nx, ny, nz), eps=eps, **more)
        g.active_index = newid
        # host-only: the first n_face_conn connections are grid faces (fault overlaps included), the rest NNCs -- what computeMaxDp scans
        g.n_face_conn = int(np.count_nonzero(keep[:n_faces]))
        self._grid = g
        return g

    def fipnum(self):
        """FIPNUM of the active cells, 1-based as computeFluidInPlace takes it (0 = in no region); None without the keyword -- the
        reference then reports the whole field as one region (SimulatorBase_impl.hpp:140-150)."""
        if not self.has("FIPNUM"):
            return None
        nx, ny, nz = self.dims
        self.grid()                                   # (fixes the set of active cells)
        full = self.array("FIPNUM", nx * ny * nz)[self.active]
        return np.where(np.isnan(full), 0, full).astype(np.int32)

    def eqlnum(self):
        """EQLNUM of the active cells, 1-based (all ones without the keyword), like fipnum()"""
        nx, ny, nz = self.dims
        if getattr(self, "active", None) is None:
            self.grid()                               # (fixes the set of active cells)
        if not self.has("EQLNUM"):
            return np.ones(self.active.size, np.int32)
        full = self.array("EQLNUM", nx * ny * nz)[self.active]
        if np.isnan(full).any():
            raise ValueError("EQLNUM must be given for every active cell")
        return full.astype(np.int32)

    def thpres(self):
        """The barriers of THPRES: {(r1, r2) with r1 < r2: threshold in Pa, or None when item 3 is defaulted (the value is then the
        largest phase-potential difference between the two regions in the initial state, computeMaxDp)}; None without the keyword.  A
        later record for the same pair wins.  The reference keeps them in opm-common's ThresholdPressure, which is outside its tree, so
        the refusals are OURS -- all ValueErrors naming the keyword: THPRES without EQLOPTS naming THPRES; EQLOPTS naming IRREVERS
        (directional thresholds, whether or not THPRES follows); a region below 1 or above EQLDIMS item 1; a record with r1 == r2 or
        fewer than two items; a negative value."""
        opts = [str(x).upper() for r in (self.records("EQLOPTS") if self.has("EQLOPTS") else []) for x in r if x is not None]
        if "IRREVERS" in opts:
            raise ValueError("EQLOPTS IRREVERS (direction-dependent threshold pressures) is not supported")
        if not self.has("THPRES"):
            return None
        if "THPRES" not in opts:
            raise ValueError("THPRES in SOLUTION needs EQLOPTS naming THPRES in RUNSPEC")
        r = self.records("EQLDIMS")[0] if self.has("EQLDIMS") and self.records("EQLDIMS") else []
        ntequl = int(r[0]) if len(r) > 0 and r[0] is not None else 1
        out = {}
        for rec in self.records("THPRES"):
            if not rec:
                continue
            if len(rec) < 2 or rec[0] is None or rec[1] is None:
                raise ValueError("THPRES: a record needs two region numbers")
            r1, r2 = int(rec[0]), int(rec[1])
            for reg in (r1, r2):
                if reg < 1 or reg > ntequl:
                    raise ValueError("THPRES: region %d outside 1 .. %d (EQLDIMS item 1)" % (reg, ntequl))
            if r1 == r2:
                raise ValueError("THPRES: a barrier between region %d and itself" % r1)
            value = float(rec[2]) * BAR if len(rec) > 2 and rec[2] is not None else None
            if value is not None and not value >= 0.0:
                raise ValueError("THPRES: negative threshold pressure between regions %d and %d" % (r1, r2))
            out[(min(r1, r2), max(r1, r2))] = value
        return out

    def threshold_pressures(self, grid, max_dp=None):
        """Threshold pressure [Pa] of every connection of `grid` (this deck's grid()), faces then NNCs: thresholdPressures and
        thresholdPressuresNNC (opm/simulators/thresholdPressures.hpp:320-369, :383-417).  A connection between two regions with a
        barrier takes the explicit value; for a defaulted barrier max_dp[pair] -- max_dp is computeMaxDp's [nregions][nregions] table
        (-1 = no face joins the pair) or a dict {(r1, r2) with r1 < r2: value} -- and a FACE whose pair is absent from it takes 0; every
        connection without a barrier takes 0.  max_dp may be None when no barrier is defaulted.  None without THPRES.
        Ours, not the reference's: a defaulted barrier on an NNC whose pair no face joins is a ValueError naming THPRES (the reference's
        maxDp.at() throws there); and the NNC's pair is looked up ORDERED (r1 < r2), where the reference looks it up as given,
        (eq1, eq2), in a map that only holds ordered pairs."""
        barriers = self.thpres()
        if barriers is None:
            return None
        eq = self.eqlnum()
        c = grid.conn_cells
        e1, e2 = eq[c[:, 0]], eq[c[:, 1]]
        lo, hi = np.minimum(e1, e2), np.maximum(e1, e2)
        nface = grid.n_face_conn
        out = np.zeros(grid.nconn)
        for (r1, r2), value in barriers.items():
            m = (lo == r1) & (hi == r2)
            if value is None:
                if max_dp is None:
                    raise ValueError("THPRES: the barrier between regions %d and %d is defaulted: max_dp is needed" % (r1, r2))
                if isinstance(max_dp, dict):
                    value = max_dp.get((r1, r2))
                else:
                    value = float(np.asarray(max_dp)[r1 - 1, r2 - 1])
                    value = None if value < 0.0 else value
                if value is None:
                    if m[nface:].any():
                        raise ValueError("THPRES: the defaulted barrier between regions %d and %d lies on an NNC, but no grid face joins "
                                         "the two regions: there is no potential difference to take" % (r1, r2))
                    value = 0.0
            out[m] = value
        return out

    def hysteresis(self):
        """SATOPTS HYSTER with an EHYSTR model the device implements: item 2 = 0 (Carlson) or 2 (Killough) for the non-wetting phases,
        drainage curves for the wetting phases, item 5 = KR (relative permeabilities only).  Which of the two: hysteresis_model()."""
        if not self.has("SATOPTS") or not any(str(x).upper().startswith("HYST") for r in self.records("SATOPTS") for x in r):
            return False
        self.hysteresis_model()          # (refuses what the device does not implement)
        return True

    def hysteresis_model(self):
        """(model, a) of EHYSTR: item 2 as capi.HYST_CARLSON (0, also without the keyword) or capi.HYST_KILLOUGH (2), and item 4, Killough's
        curvature parameter (default 0.1; Carlson does not use it).  Items 1 and 3 (capillary-pressure curvature, the wetting-phase
        modification) are read past.  ValueError naming EHYSTR for item 2 in 1, 3, 4 (the wetting-phase models), any other model number,
        and item 5 other than KR."""
        model, a = capi.HYST_CARLSON, 0.1
        if self.has("EHYSTR"):
            r = self.records("EHYSTR")[0]
            model = int(r[1]) if len(r) > 1 and r[1] is not None else 0
            if len(r) > 3 and r[3] is not None:
                a = float(r[3])
            what = str(r[4]).upper() if len(r) > 4 and r[4] is not None else "BOTH"
            if model in (1, 3, 4):
                raise ValueError("EHYSTR: item 2 = %d (hysteresis of the wetting phase) is not supported; 0 (Carlson) and 2 (Killough) are" % model)
            if model not in (capi.HYST_CARLSON, capi.HYST_KILLOUGH):
                raise ValueError("EHYSTR: item 2 = %d is not a model; 0 (Carlson) and 2 (Killough) are supported" % model)
            if what != "KR":
                raise ValueError("EHYSTR: item 5 = %s is not supported, only KR (no capillary-pressure hysteresis)" % what)
        return model, a

    def endpoints(self, prefix="", regions="SATNUM"):
        """ENDSCALE: per-cell scaled end points; the ones the deck does not give default to the cell's table values
        (EclEpsScalingPointsInfo::extractScaled falls back to the unscaled points).  prefix "I" / regions "IMBNUM": the
        imbibition curves' points (ISWL ...)."""
        if not self.has("ENDSCALE"):
            return None
        nx, ny, nz = self.dims
        n = nx * ny * nz
        t = self.tables()
        regkw = regions if self.has(regions) else "SATNUM"
        sat = (self.array(regkw, n).astype(int) - 1) if self.has(regkw) else np.zeros(n, int)
        un = np.zeros((t.n_sat, 8))
        for r in range(t.n_sat):
            a, b = t.swof_ptr[r], t.swof_ptr[r + 1]
            sw, krw, krow = t.swof_sw[a:b], t.swof_krw[a:b], t.swof_krow[a:b]
            if t.phases == "wo":
                un[r, :4] = [sw[0], last_zero(sw, krw), sw[-1], 1.0 - first_zero(sw, krow)]
                continue
            a, b = t.sgof_ptr[r], t.sgof_ptr[r + 1]
            sg, krg, krog = t.sgof_sg[a:b], t.sgof_krg[a:b], t.sgof_krog[a:b]
            un[r] = [sw[0], last_zero(sw, krw), sw[-1], 1.0 - first_zero(sw, krow), sg[0], last_zero(sg, krg), sg[-1], 1.0 - first_zero(sg, krog)]
        out = {}
        for k, name in enumerate(EPS_NAMES):
            a = self.array(prefix + name, n, None) if not (t.phases == "wo" and k >= 4) else None
            dflt = un[sat, k]
            out[name] = dflt if a is None else np.where(np.isnan(a), dflt, a)
        if t.phases == "wo":        # no gas phase: the gas end points are not the deck's (no gas curve is ever scaled); SGL = 0 is what counts
            out["SGL"], out["SGCR"], out["SGU"], out["SOGCR"] = np.zeros(n), np.zeros(n), 1.0 - out["SWL"], out["SOWCR"].copy()
        return out

    def swatinit(self):
        """SWATINIT of the active cells (the imposed initial water saturation EQUIL honours by rescaling each cell's PCW); None without
        the keyword.  Refused with a ValueError naming the keyword: an array that does not hold one value for every cell of the grid or
        leaves an active cell defaulted, a value outside [0, 1], a deck without EQUIL or without a water phase."""
        if not self.has("SWATINIT"):
            return None
        named = [k for k in ("OIL", "WATER", "GAS") if self.has(k)]
        if named and "WATER" not in named:
            raise ValueError("SWATINIT in a deck without a water phase")
        if not self.has("EQUIL"):
            raise ValueError("SWATINIT needs EQUIL: it acts on the equilibration, a deck with an explicit initial state has no use for it")
        nx, ny, nz = self.dims
        if getattr(self, "active", None) is None:
            self.grid()                               # (fixes the set of active cells)
        v = self.array("SWATINIT", nx * ny * nz)[self.active]
        if np.isnan(v).any():
            raise ValueError("SWATINIT must be given for every active cell")
        if (v < 0.0).any() or (v > 1.0).any():
            raise ValueError("SWATINIT outside [0, 1]")
        return v

    # ---------------------------------------------------------------- analytic aquifers
    def aquifers(self, tables=None):
        """The deck's analytic aquifers as a list of Aquifer (SI; cells in the numbering of grid()), in ascending aquifer id; [] without
        AQUFETP / AQUCT.  The device rule they feed is stated in include/opmgpu.h at opmgpu_set_aquifers.
          AQUFETP  id, datum depth, initial pressure, V_0, C_t, J, PVTW table, [salt], [temperature]      -> CtV0 = C_t V_0, J
          AQUCT    id, datum depth, initial pressure, k_a, phi, C_t, r_o, h, theta (default 360), PVTW table (default 1), influence
                   table, [salt], [temperature]    -> beta = 2 pi (theta / 360) h phi C_t r_o^2,  T_c = mu_w phi C_t r_o^2 / k_a, with mu_w the
                   water viscosity of the named PVTW record at the initial pressure (the rule csrc/fluid_eval.hpp states for water:
                   mu_w = mu_ref B_ref b_w / (1 + Y (1 + Y / 2)), Y = (C_w - C_v)(p - p_ref), b_w = (1 + X (1 + X / 2)) / B_ref, X = C_w (p - p_ref))
          AQUTAB   one record per influence table, pairs (t_D, P_D); the first record is table 2 (table 1 is the built-in one of an
                   infinite aquifer, which is not carried here)
          AQUANCON id, I1 I2 J1 J2 K1 K2, face (I- I+ J- J+ K- K+), influx coefficient (default: the face area from DX / DY / DZ),
                   multiplier (default 1), connect interior faces (default NO: only faces whose outward neighbour lies outside the grid
                   or is inactive)
        Several faces of one cell towards the same aquifer merge into one connection; alpha_j = coefficient_j multiplier_j / their sum.
        Refused with a ValueError naming keyword and item: a defaulted initial pressure (items 3), AQUCT with influence table 1 or a
        table AQUTAB does not hold (item 11), a defaulted influx coefficient on a corner-point grid (AQUANCON item 9), an AQUANCON for an
        unknown aquifer (item 1), an aquifer without connections, salt items (AQUFETP 8, AQUCT 12), and AQUFLUX / AQUNUM / AQUCON."""
        for k in ("AQUFLUX", "AQUNUM", "AQUCON"):
            if self.has(k):
                raise ValueError("%s is not supported (analytic aquifers: AQUFETP, AQUCT with AQUANCON)" % k)
        if not (self.has("AQUFETP") or self.has("AQUCT")):
            if self.has("AQUANCON"):
                raise ValueError("AQUANCON item 1: no aquifer is defined (AQUFETP / AQUCT)")
            return []
        if tables is None:
            tables = self.tables()
        item = lambda r, i, d=None: r[i] if len(r) > i and r[i] is not None else d         # noqa: E731
        nx, ny, nz = self.dims
        if getattr(self, "active", None) is None:
            self.grid()
        n = nx * ny * nz
        act = np.zeros(n, bool); act[self.active] = True
        newid = -np.ones(n, np.int64); newid[self.active] = np.arange(self.active.size)
        aq = {}

        def pvt_record(kw, r, i):
            reg = int(item(r, i, 1))
            if reg < 1 or reg > tables.n_pvt:
                raise ValueError("%s item %d: PVTW table %d outside 1 .. %d" % (kw, i + 1, reg, tables.n_pvt))
            return reg - 1
        for r in (self.records("AQUFETP") if self.has("AQUFETP") else []):
            if not r:
                continue
            aid = int(r[0])
            if item(r, 2) is None:
                raise ValueError("AQUFETP item 3: a defaulted initial pressure (equilibrium with the reservoir) is not supported")
            if item(r, 7) is not None:
                raise ValueError("AQUFETP item 8: a salt concentration is not supported")
            for i, what in ((1, "datum depth"), (3, "initial water volume"), (4, "total compressibility"), (5, "productivity index")):
                if item(r, i) is None:
                    raise ValueError("AQUFETP item %d: the %s must be given" % (i + 1, what))
            pvt_record("AQUFETP", r, 6)
            aq[aid] = Aquifer(aid, capi.AQUIFER_FETKOVICH, p_a0=float(r[2]) * BAR, datum=float(r[1]), CtV0=float(r[3]) * float(r[4]) / BAR,
                              J=float(r[5]) / (DAY * BAR))
        tabs = [[]]                     # table 1: the built-in one, not carried
        for r in (self.records("AQUTAB") if self.has("AQUTAB") else []):
            if r:
                tabs.append((np.asarray(r[0::2], float), np.asarray(r[1::2], float)))
        for r in (self.records("AQUCT") if self.has("AQUCT") else []):
            if not r:
                continue
            aid = int(r[0])
            if aid in aq:
                raise ValueError("AQUCT item 1: aquifer %d is defined twice" % aid)
            if item(r, 2) is None:
                raise ValueError("AQUCT item 3: a defaulted initial pressure (equilibrium with the reservoir) is not supported")
            if item(r, 11) is not None:
                raise ValueError("AQUCT item 12: a salt concentration is not supported")
            for i, what in ((1, "datum depth"), (3, "permeability"), (4, "porosity"), (5, "total compressibility"), (6, "external radius"), (7, "thickness")):
                if item(r, i) is None:
                    raise ValueError("AQUCT item %d: the %s must be given" % (i + 1, what))
            tno = int(item(r, 10, 1))
            if tno == 1:
                raise ValueError("AQUCT item 11: the built-in influence table 1 is not carried; give the table in AQUTAB and name it (2 = the first AQUTAB record)")
            if tno < 1 or tno > len(tabs):
                raise ValueError("AQUCT item 11: influence table %d is not in AQUTAB (it holds the tables 2 .. %d)" % (tno, len(tabs)))
            td, pd = tabs[tno - 1]
            if td.size != pd.size or td.size < 2 or not np.all(np.diff(td) > 0):
                raise ValueError("AQUTAB table %d: at least 2 rows (t_D, P_D) with strictly increasing t_D are needed" % tno)
            w = tables.pvtw[pvt_record("AQUCT", r, 9)]
            p0 = float(r[2]) * BAR
            mu = water_viscosity(w, p0)
            k_a, phi, ct, ro, h = float(r[3]) * MD, float(r[4]), float(r[5]) / BAR, float(r[6]), float(r[7])
            theta = float(item(r, 8, 360.0))
            aq[aid] = Aquifer(aid, capi.AQUIFER_CARTER_TRACY, p_a0=p0, datum=float(r[1]),
                              beta=2.0 * np.pi * (theta / 360.0) * h * phi * ct * ro * ro, Tc=mu * phi * ct * ro * ro / k_a, td=td, pd=pd)
        # AQUANCON: per aquifer {cell: coefficient x multiplier}, cells in order of first appearance
        dx, dy, dz = (a.ravel() for a in self._cell_sizes())
        idx = np.arange(n).reshape(nz, ny, nx)
        area = {"I": dy * dz, "J": dx * dz, "K": dx * dy}
        conn = {aid: {} for aid in aq}
        for r in (self.records("AQUANCON") if self.has("AQUANCON") else []):
            if not r:
                continue
            aid = int(r[0])
            if aid not in aq:
                raise ValueError("AQUANCON item 1: aquifer %d is not defined (AQUFETP / AQUCT)" % aid)
            if any(item(r, i) is None for i in range(1, 8)):
                raise ValueError("AQUANCON items 2-8: the box and the face must be given")
            i1, i2, j1, j2, k1, k2 = (int(r[i]) for i in range(1, 7))
            if not (1 <= i1 <= i2 <= nx and 1 <= j1 <= j2 <= ny and 1 <= k1 <= k2 <= nz):
                raise ValueError("AQUANCON items 2-7: the box %s lies outside the grid" % ((i1, i2, j1, j2, k1, k2),))
            face = str(r[7]).upper().replace("X", "I").replace("Y", "J").replace("Z", "K")
            if len(face) != 2 or face[0] not in "IJK" or face[1] not in "+-":
                raise ValueError("AQUANCON item 8: face %r is none of I- I+ J- J+ K- K+" % r[7])
            coeff, mult = item(r, 8), float(item(r, 9, 1.0))
            if coeff is None and self.has("ZCORN"):
                raise ValueError("AQUANCON item 9: a defaulted influx coefficient on a corner-point grid is not supported")
            interior = str(item(r, 10, "NO")).upper().startswith("Y")
            axis, step = "KJI".index(face[0]), (1 if face[1] == "+" else -1)
            for c in idx[k1 - 1:k2, j1 - 1:j2, i1 - 1:i2].ravel():
                if not act[c]:
                    continue
                kji = [c // (nx * ny), (c // nx) % ny, c % nx]
                kji[axis] += step
                inside = 0 <= kji[0] < nz and 0 <= kji[1] < ny and 0 <= kji[2] < nx
                if inside and act[idx[kji[0], kji[1], kji[2]]] and not interior:
                    continue                    # the outward neighbour is an active cell
                v = (float(coeff) if coeff is not None else float(area[face[0]][c])) * mult
                if not v > 0.0:
                    raise ValueError("AQUANCON items 9-10: coefficient x multiplier must be positive")
                cell = int(newid[c])
                conn[aid][cell] = conn[aid].get(cell, 0.0) + v
        out = []
        for aid in sorted(aq):
            if not conn[aid]:
                raise ValueError("%s item 1: aquifer %d has no connections (AQUANCON)" % ("AQUFETP" if aq[aid].kind == capi.AQUIFER_FETKOVICH else "AQUCT", aid))
            a = aq[aid]
            a.cells = np.fromiter(conn[aid].keys(), np.int64, len(conn[aid]))
            w = np.fromiter(conn[aid].values(), float, len(conn[aid]))
            a.alpha = w / w.sum()
            out.append(a)
        return out

    # ---------------------------------------------------------------- rock regions and compaction
    def rock_regions(self):
        """The deck's rock regions as a decks.RockRegions (cells in the numbering of grid()), or None without ROCKCOMP in RUNSPEC -- then
        tables() carries the first ROCK / ROCKTAB record for every cell, as ever.  The device rule they feed is stated in include/opmgpu.h
        at opmgpu_set_rock_regions.
          ROCKCOMP  item 1 REVERS (the default) or IRREVERS; item 2 the number of rock tables (default 1); item 3 water-induced
                    compaction, NO or defaulted
          ROCKOPTS  item 1 PRESSURE (the default); item 2 NOSTORE (the default); item 3 the region array that picks a cell's ROCK /
                    ROCKTAB record: PVTNUM (the default), SATNUM or ROCKNUM
          ROCKNUM   (REGIONS) 1-based region per cell, when ROCKOPTS item 3 names it
          ROCKTAB   one record per region, rows (p, pv_mult, trans_mult); a region whose record is missing or empty takes the ROCK form
          ROCK      one record (p_ref, compressibility) per region
        Refused with a ValueError naming keyword and item: ROCKCOMP item 1 HYSTER, BOBERG, REVLIMIT, PALM-MAN (or anything else), item 3
        other than NO; ROCKOPTS item 1 other than PRESSURE, item 2 STORE, an unknown item 3; a region number outside 1 .. the number of
        tables; a region with neither a ROCKTAB nor a ROCK record."""
        if not self.has("ROCKCOMP"):
            return None
        item = lambda r, i, d=None: r[i] if len(r) > i and r[i] is not None else d         # noqa: E731
        rc = self.records("ROCKCOMP")[0] if self.records("ROCKCOMP") else []
        model = str(item(rc, 0, "REVERS")).upper()
        if model in ("HYSTER", "BOBERG", "REVLIMIT", "PALM-MAN"):
            raise ValueError("ROCKCOMP item 1: the %s compaction model is not supported (REVERS, IRREVERS)" % model)
        if model not in ("REVERS", "IRREVERS"):
            raise ValueError("ROCKCOMP item 1: %r is neither REVERS nor IRREVERS" % item(rc, 0))
        ntab = int(item(rc, 1, 1))
        if ntab < 1:
            raise ValueError("ROCKCOMP item 2: the number of rock tables must be at least 1")
        if str(item(rc, 2, "NO")).upper() != "NO":
            raise ValueError("ROCKCOMP item 3: water-induced compaction (%s) is not supported" % item(rc, 2))
        ro = self.records("ROCKOPTS")[0] if self.has("ROCKOPTS") and self.records("ROCKOPTS") else []
        if str(item(ro, 0, "PRESSURE")).upper() != "PRESSURE":
            raise ValueError("ROCKOPTS item 1: %s is not supported (PRESSURE)" % item(ro, 0))
        if str(item(ro, 1, "NOSTORE")).upper() != "NOSTORE":
            raise ValueError("ROCKOPTS item 2: %s is not supported (NOSTORE)" % item(ro, 1))
        regkw = str(item(ro, 2, "PVTNUM")).upper()
        if regkw not in ("PVTNUM", "SATNUM", "ROCKNUM"):
            raise ValueError("ROCKOPTS item 3: %r is none of PVTNUM, SATNUM, ROCKNUM" % item(ro, 2))
        nx, ny, nz = self.dims
        if getattr(self, "active", None) is None:
            self.grid()
        if self.has(regkw):
            num = self.array(regkw, nx * ny * nz)[self.active]
            if np.isnan(num).any():
                raise ValueError("%s must be given for every active cell (ROCKOPTS item 3 names it)" % regkw)
            num = num.astype(np.int64) - 1
        else:
            num = np.zeros(self.active.size, np.int64)
        if num.size and (num.min() < 0 or num.max() >= ntab):
            raise ValueError("%s: region %d is outside 1 .. %d (ROCKCOMP item 2)" % (regkw, int(num.max() + 1 if num.max() >= ntab else num.min() + 1), ntab))
        rocks = self.records("ROCK") if self.has("ROCK") else []
        tabs = self.records("ROCKTAB") if self.has("ROCKTAB") else []
        rock, tables = [], []
        for r in range(ntab):
            rec = tabs[r] if r < len(tabs) else []
            if rec:
                ncol = 5 if len(rec) % 5 == 0 and len(rec) % 3 != 0 else 3
                tables.append([(rec[i], rec[i + 1], rec[i + 2]) for i in range(0, len(rec), ncol)])
            else:
                tables.append(None)
            if r < len(rocks) and len(rocks[r]) >= 2:
                rock.append((rocks[r][0], rocks[r][1]))
            elif tables[-1] is None:
                raise ValueError("ROCK: no record for region %d, which has no ROCKTAB record either (ROCKCOMP item 2 = %d)" % (r + 1, ntab))
            else:
                rock.append((1.0, 0.0))
        return decks.RockRegions(num, rock, tables, irreversible=(model == "IRREVERS"))

    # ---------------------------------------------------------------- SOLUTION
    def initial_state(self, tables):
        """EQUIL (opmgpu/equil.py), else explicit PRESSURE / SWAT / SGAS / RS / RV arrays (active cells) with the hydrocarbon state from the
        saturations (FlowMain.hpp:626-673 takes the same two routes)"""
        if self.has("EQUIL") and not self.has("PRESSURE"):
            from . import equil
            return equil.from_deck(self, self._grid, tables)
        nx, ny, nz = self.dims
        n = nx * ny * nz
        act = self.active
        if tables.phases == "wo":
            for k in ("SGAS", "RS", "RV"):
                if self.has(k):
                    raise ValueError("%s in the SOLUTION section of a deck without GAS (RUNSPEC: OIL WATER)" % k)
            p = self.array("PRESSURE", n)[act] * BAR
            sw = self.array("SWAT", n, np.zeros(n))[act]
            z = np.zeros_like(sw)
            return State(p, np.stack([sw, 1.0 - sw, z], 1), z, z, np.full(sw.size, capi.HC_GAS_AND_OIL, np.int8))
        p = self.array("PRESSURE", n)[act] * BAR
        sw = self.array("SWAT", n, np.zeros(n))[act]; sg = self.array("SGAS", n, np.zeros(n))[act]
        rs = self.array("RS", n, np.zeros(n))[act]; rv = self.array("RV", n, np.zeros(n))[act]
        sat = np.stack([sw, 1.0 - sw - sg, sg], 1)
        hc = np.where(sg > 0, np.where(sat[:, 1] > 0, capi.HC_GAS_AND_OIL, capi.HC_GAS_ONLY), capi.HC_OIL_ONLY).astype(np.int8)
        if not tables.has_disgas:
            hc[hc == capi.HC_OIL_ONLY] = capi.HC_GAS_AND_OIL
        return State(p, sat, rs, rv, hc)


class Aquifer:
    """One analytic aquifer in SI as GpuBlackoilModel.setAquifers takes it: kind (capi.AQUIFER_FETKOVICH / AQUIFER_CARTER_TRACY), p_a0,
    datum, CtV0 and J (Fetkovich) or beta, Tc and the influence table td / pd (Carter-Tracy), and the connections: cells (indices of the
    grid's active cells) with their fractions alpha (summing to 1)."""

    def __init__(self, id, kind, p_a0, datum, CtV0=0.0, J=0.0, beta=0.0, Tc=0.0, td=(), pd=(), cells=(), alpha=()):
        self.id, self.kind, self.p_a0, self.datum = int(id), int(kind), float(p_a0), float(datum)
        self.CtV0, self.J, self.beta, self.Tc = float(CtV0), float(J), float(beta), float(Tc)
        self.td, self.pd = np.asarray(td, float), np.asarray(pd, float)
        self.cells, self.alpha = np.asarray(cells, np.int64), np.asarray(alpha, float)


def water_viscosity(w, p):
    """mu_w(p) of one PVTW row in SI (p_ref, B_ref, C_w, mu_ref, C_v), by the rule csrc/fluid_eval.hpp states for water (water_pvt)"""
    X = w[2] * (p - w[0])
    bw = (1.0 + X * (1.0 + X / 2.0)) / w[1]
    Y = (w[2] - w[4]) * (p - w[0])
    return w[3] * w[1] * bw / (1.0 + Y * (1.0 + Y / 2.0))


def last_zero(x, y):
    """abscissa of the last leading zero of y (critical saturation: the curve leaves zero after it)"""
    i = 0
    while i + 1 < len(y) and y[i + 1] == 0.0:
        i += 1
    return x[i]


def first_zero(x, y):
    i = 0
    while i < len(y) - 1 and y[i] != 0.0:
        i += 1
    return x[i]


def _split_tables(records):
    """PVTO / PVTG: records of one table are closed by an empty record"""
    tabs, cur = [], []
    for r in records:
        if len(r) == 0:
            if cur:
                tabs.append(cur)
            cur = []
        else:
            cur.append(r)
    if cur:
        tabs.append(cur)
    return tabs


def read_deck(path):
    text = open(path).read()
    lines = _tokens(text)
    kws, cur, open_record = {}, None, False
    box = None
    skip_line = False
    schedule, in_schedule = [], False
    solution_rptrst = None
    for toks in lines:
        if not toks:
            continue
        if skip_line:                 # TITLE: the next line is free text without a terminating slash
            skip_line = False
            continue
        first = toks[0]
        expects_data = cur is not None and not cur["closed"] and not cur["records"] and not cur["pending"]   # e.g. SCALECRS \n NO /
        if not open_record and not expects_data and _KW.match(first) and not _is_data(first):
            name = first
            cur = {"records": [], "pending": [], "closed": False, "box": box}
            if name == "ENDBOX":
                box = None
            kws[name] = cur
            if name == "SCHEDULE":
                in_schedule = True
            elif in_schedule:
                schedule.append((name, cur["records"]))
            elif name == "RPTRST":
                solution_rptrst = cur["records"]
            toks = toks[1:]
            if name == "TITLE":
                cur["closed"] = True
                skip_line = True
                continue
            if name in FLAG_KEYWORDS:
                cur["closed"] = True
                continue
        if cur is None:
            continue
        for t in toks:
            if t == "/":
                cur["records"].append(cur["pending"]); cur["pending"] = []
                open_record = False
            else:
                cur["pending"].extend(_expand(t))
                open_record = True
    return Deck(kws, schedule, solution_rptrst)


def _is_data(tok):
    try:
        float(tok.replace("D", "E"))
        return True
    except ValueError:
        return False

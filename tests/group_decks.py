"""Decks for tests/test_gpu_group_control.py (group rate control, opmgpu_set_well_groups).

  sizes_case(seed)   450 one-perforation wells on a 12 x 12 x 2 grid (several wells per cell) in controlled groups of 1, 63, 64, 65 and
                     257 members -- across the wavefront (64) and the workgroup (256) of k_group_targets -- with a random well state:
                     group 0 (1 well)   on its slot: I is empty
                     group 1 (63)       every well under individual control: C is empty
                     group 2 (64)       water injection group whose individual wells exceed the target: a negative remainder
                     group 3 (65)       LRAT, mixed
                     group 4 (257)      ORAT, mixed, e_w < 1 on a third of the wells
  field_deck(...)    10 x 10 x 3 cells, four oil producers in the corners under one ORAT group and a water injector in the centre
  inject_deck(...)   the same grid, three water injectors under one injection group and two BHP producers"""
import numpy as np

from opmgpu import decks, wells as W

WATER, OIL = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
SIZES = (1, 63, 64, 65, 257)
DAY = decks.DAY


def sizes_case(seed=0):
    rng = np.random.default_rng(seed)
    grid = decks.cartesian_grid(12, 12, 2, dx=100.0, dy=100.0, dz=5.0, tops=2500.0, poro=0.25, permx_md=150.0)
    tab = decks.satfunc_standard_tables()
    nw = sum(SIZES)
    group_of = np.repeat(np.arange(len(SIZES)), SIZES)
    order = rng.permutation(nw)                      # the members of a group are scattered over the well list
    group_of_well = np.empty(nw, int); group_of_well[order] = group_of
    eff = np.ones(nw)
    g4 = np.flatnonzero(group_of_well == 4)
    eff[g4[::3]] = rng.uniform(0.3, 0.95, g4[::3].size)
    wl = W.Wells()
    for w in range(nw):
        cell = int(rng.integers(0, grid.nc))
        if group_of_well[w] == 2:
            wl.add_well("I%d" % w, W.INJECTOR, grid.z[cell], [cell], 1e-12, WATER, (W.SURFACE_RATE, 500.0 / DAY, WATER), limits=[(W.BHP, 400 * decks.BAR)], efficiency=eff[w])
        else:
            # every third producer has a liquid-rate limit as well: the slot's index differs from member to member inside a group
            more = [(W.SURFACE_RATE, -900.0 / DAY, (1.0, 1.0, 0.0))] if w % 3 == 0 else []
            wl.add_well("P%d" % w, W.PRODUCER, grid.z[cell], [cell], 1e-12, OIL, (W.SURFACE_RATE, -500.0 / DAY, OIL), limits=[(W.BHP, 150 * decks.BAR)] + more, efficiency=eff[w])
    spec = [(-1, 40.0, (0, 1, 0)), (-1, 63 * 30.0, (0, 1, 0)), (+1, 200.0, (1, 0, 0)), (-1, 65 * 30.0, (1, 1, 0)), (-1, 257 * 25.0, (0, 1, 0))]
    for g, (sign, T, d) in enumerate(spec):
        members = rng.permutation(np.flatnonzero(group_of_well == g))          # ... and not in ascending order inside it
        wl.add_group("G%d" % g, sign, T / DAY, d, members, rng.uniform(0.05, 20.0, members.size))
    slot = np.asarray([len(c) - 1 for c in wl.controls])
    current = np.where(rng.random(nw) < 0.5, slot, rng.integers(0, 2, nw))
    current[group_of_well == 0] = slot[group_of_well == 0]
    current[group_of_well == 1] = rng.integers(0, 2, SIZES[1])
    current[np.flatnonzero(group_of_well == 2)[:40]] = 0          # 40 injectors of about 30 m3/day each against a target of 200
    sign = np.where(np.asarray(wl.type) == W.PRODUCER, -1.0, 1.0)
    qs = sign[:, None] * rng.uniform(5.0, 60.0, (nw, 3)) / DAY
    qs[np.asarray(wl.type) == W.INJECTOR, 1:] = 0.0
    bhp = rng.uniform(150.0, 400.0, nw) * decks.BAR
    return grid, tab, wl, slot, current.astype(np.int32), qs, bhp, group_of_well


def _grid_state():
    nx, ny, nz = 10, 10, 3
    grid = decks.cartesian_grid(nx, ny, nz, dx=300.0, dy=300.0, dz=10.0, tops=2500.0, poro=0.3, permx_md=200.0, lognormal_sigma=0.3)
    tab = decks.satfunc_standard_tables()
    st = decks.initial_state(grid, tab, p_ref=250 * decks.BAR, z_ref=2500.0, gas_cap_fraction=0.0, gas_only_fraction=0.0)
    col = lambda i, j: [i + nx * j + nx * ny * k for k in range(nz)]          # noqa: E731
    return grid, tab, st, col, 5.0 * float(np.median(grid.trans))


def field_deck(target=400.0, bhp_limits_bar=(150.0, 150.0, 150.0, 150.0), own_orat=300.0, on_group=(0, 1, 2, 3), guide=(1.0, 2.0, 3.0, 4.0),
               eff=(1.0, 1.0, 1.0, 1.0)):
    """Producers 0..3 (ORAT `own_orat` m3/day each with a BHP limit; members of the ORAT group FIELD, `target` m3/day) and the water
    injector 4.  on_group: the producers that start on their slot (deck mode GRUP)."""
    grid, tab, st, col, WI = _grid_state()
    wl = W.Wells()
    for k, (i, j) in enumerate([(0, 0), (9, 0), (0, 9), (9, 9)]):
        wl.add_well("P%d" % k, W.PRODUCER, grid.z[col(i, j)[0]], col(i, j)[:2], WI, OIL, (W.SURFACE_RATE, -own_orat / DAY, OIL),
                    limits=[(W.BHP, bhp_limits_bar[k] * decks.BAR)], efficiency=eff[k])
    wl.add_well("INJ", W.INJECTOR, grid.z[col(5, 5)[0]], col(5, 5), WI, WATER, (W.SURFACE_RATE, 300.0 / DAY, WATER), limits=[(W.BHP, 400 * decks.BAR)])
    wl.add_group("FIELD", -1, target / DAY, OIL, [0, 1, 2, 3], list(guide), on_group=on_group)
    return grid, tab, st, wl


def inject_deck(target=600.0, bhp_limits_bar=(400.0, 400.0, 400.0), on_group=(0, 1, 2), guide=(1.0, 1.0, 2.0)):
    """Water injectors 0..2 (RATE 500 m3/day each with a BHP limit; members of the injection group INJ) and the BHP producers 3, 4."""
    grid, tab, st, col, WI = _grid_state()
    wl = W.Wells()
    for k, (i, j) in enumerate([(0, 0), (9, 0), (4, 9)]):
        wl.add_well("I%d" % k, W.INJECTOR, grid.z[col(i, j)[0]], col(i, j), WI, WATER, (W.SURFACE_RATE, 500.0 / DAY, WATER),
                    limits=[(W.BHP, bhp_limits_bar[k] * decks.BAR)])
    for k, (i, j) in enumerate([(9, 9), (0, 5)]):
        wl.add_well("P%d" % k, W.PRODUCER, grid.z[col(i, j)[0]], col(i, j)[:2], WI, OIL, (W.BHP, 220 * decks.BAR))
    wl.add_group("INJ", +1, target / DAY, WATER, [0, 1, 2], list(guide), on_group=on_group)
    return grid, tab, st, wl

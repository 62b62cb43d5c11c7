"""CPU: the sharing rule of group rate control (include/opmgpu.h, opmgpu_set_well_groups) -- hand-worked cases on the numpy
restatement tests/group_reference.py and on the host well model's update_group_targets, and the two against each other."""
import numpy as np
import pytest

from opmgpu import wells as W
from group_reference import slot_targets


def _wells(n_prod, n_inj=0, eff=None):
    """n_prod oil producers (ORAT + BHP limit) and n_inj water injectors (RATE + BHP limit), one perforation each"""
    wl = W.Wells()
    for w in range(n_prod + n_inj):
        e = 1.0 if eff is None else eff[w]
        if w < n_prod:
            wl.add_well("P%d" % w, W.PRODUCER, 0.0, [w], 1.0, (0.0, 1.0, 0.0), (W.SURFACE_RATE, -1000.0, (0.0, 1.0, 0.0)), limits=[(W.BHP, 1e7)], efficiency=e)
        else:
            wl.add_well("I%d" % w, W.INJECTOR, 0.0, [w], 1.0, (1.0, 0.0, 0.0), (W.SURFACE_RATE, 1000.0, (1.0, 0.0, 0.0)), limits=[(W.BHP, 5e7)], efficiency=e)
    return wl


def _both(wl, current, qs):
    """the slot targets by the restatement and by the host model"""
    nw = wl.nw
    slot = np.asarray([len(c) - 1 for c in wl.controls])
    ref, terms, rate = slot_targets(wl.groups, slot, current, qs, wl.efficiency_factors())
    host = W.StandardWellsHost(wl, np.zeros(nw), (1000.0, 800.0, 1.0))
    ws = W.WellState(wl, np.full(nw, 2e7))
    ws.current[:] = current
    ws.qs[:] = qs
    got = host.update_group_targets(ws)
    out = np.full(nw, np.nan)
    for w, t in got.items():
        out[w] = t
        assert wl.controls[w][-1][1] == t and wl.controls[w][-1][0] == W.SURFACE_RATE          # written into the slot, nothing else changed
    return ref, out, terms, rate


def test_three_producers_share_by_guide_rate():
    wl = _wells(3).add_group("G", -1, 600.0, (0, 1, 0), [0, 1, 2], [1.0, 2.0, 3.0], on_group=[0, 1, 2])
    assert [len(c) for c in wl.controls] == [3, 3, 3] and wl.current0 == [2, 2, 2]
    qs = np.zeros((3, 3)); qs[:, 1] = [-10.0, -20.0, -30.0]              # what the wells produce does not matter while all are on the slot
    ref, host, _, rate = _both(wl, [2, 2, 2], qs)
    assert np.array_equal(ref, [-100.0, -200.0, -300.0]) and np.array_equal(host, ref)
    assert rate[0] == -60.0


def test_a_well_under_individual_control_takes_its_rate_out_of_the_target():
    wl = _wells(3).add_group("G", -1, 600.0, (0, 1, 0), [0, 1, 2], [1.0, 2.0, 3.0], on_group=[0, 2])
    assert wl.current0 == [2, 0, 2]
    qs = np.zeros((3, 3)); qs[:, 1] = [-1.0, -50.0, -2.0]; qs[:, 0] = -7.0       # water is no part of an ORAT group's rate
    ref, host, _, _ = _both(wl, [2, 0, 2], qs)
    assert np.array_equal(ref[[0, 2]], [-137.5, -412.5]) and np.array_equal(host, ref)
    # the well under individual control: what it would get if it joined -- 2 / 6 of the whole target, its own rate no longer counted
    assert ref[1] == -200.0
    # on its BHP limit (control 1) it is under individual control just the same
    ref2, host2, _, _ = _both(wl, [2, 1, 2], qs)
    assert np.array_equal(ref2, ref) and np.array_equal(host2, ref)


def test_individual_wells_beyond_the_target_leave_nothing():
    wl = _wells(3).add_group("G", -1, 600.0, (0, 1, 0), [0, 1, 2], [1.0, 2.0, 3.0])
    qs = np.zeros((3, 3)); qs[:, 1] = [-400.0, -300.0, -5.0]
    ref, host, _, _ = _both(wl, [0, 0, 2], qs)
    assert ref[2] == 0.0 and host[2] == 0.0                              # 600 - 700 < 0: clamped
    assert np.array_equal(ref[:2], [-(1.0 / 4.0) * 300.0, -(2.0 / 5.0) * 200.0]) and np.array_equal(host, ref)
    # C empty: every well is offered its share of what the others leave
    ref, host, _, _ = _both(wl, [0, 0, 0], qs)
    assert np.array_equal(ref, [-295.0, -195.0, 0.0]) and np.array_equal(host, ref)


def test_the_efficiency_factor_divides_the_wells_own_target():
    e = [0.5, 1.0, 0.8]
    wl = _wells(3, eff=e).add_group("G", -1, 600.0, (0, 1, 0), [0, 1, 2], [1.0, 1.0, 2.0])
    qs = np.zeros((3, 3)); qs[:, 1] = [-100.0, -100.0, -100.0]
    ref, host, _, rate = _both(wl, [2, 2, 0], qs)
    # well 2 delivers 0.8 * 100 = 80 to the group; 520 remain, half each; well 0 is up half of the time, so it must flow twice its share
    assert np.allclose(ref, [-520.0, -260.0, -(2.0 / 4.0) * 600.0 / 0.8], rtol=1e-15) and np.array_equal(host, ref)
    assert rate[0] == -(50.0 + 100.0 + 80.0)
    assert sum(e[w] * ref[w] for w in (0, 1)) + e[2] * qs[2, 1] == pytest.approx(-600.0, rel=1e-15)


def test_an_injection_group():
    wl = _wells(1, 3).add_group("INJ", +1, 900.0, (1, 0, 0), [1, 2, 3], [1.0, 1.0, 4.0], on_group=[1, 3])
    assert wl.current0 == [0, 2, 0, 2]
    qs = np.zeros((4, 3)); qs[1:, 0] = [10.0, 300.0, 20.0]
    ref, host, _, rate = _both(wl, [0, 2, 0, 2], qs)
    assert np.isnan(ref[0]) and np.isnan(host[0])                        # the producer is in no group
    assert np.array_equal(ref[1:], [120.0, 150.0, 480.0]) and np.array_equal(host[1:], ref[1:]) and rate[0] == 330.0
    with pytest.raises(ValueError, match="two controlled groups"):
        wl.add_group("AGAIN", +1, 1.0, (1, 0, 0), [2], [1.0])
    with pytest.raises(ValueError, match="injection group does not control"):
        wl.add_group("P", +1, 1.0, (1, 0, 0), [0], [1.0])


def test_guide_rates_from_the_potentials():
    wl = _wells(3).add_group("G", -1, 600.0, (1, 1, 0), [0, 1, 2], [float("nan"), 5.0, float("nan")])
    pot = np.array([[-1.0, -2.0, -50.0], [-9.0, -9.0, -9.0], [0.0, 0.0, -3.0]])
    calls = []
    W.resolve_guide_rates(wl.groups, lambda: calls.append(1) or pot)
    assert wl.groups[0].guide == [3.0, 5.0, W.GUIDE_RATE_FLOOR] and calls == [1] and W.GUIDE_RATE_FLOOR > 0
    W.resolve_guide_rates(wl.groups, lambda: calls.append(1) or pot)      # nothing left to the potentials: not asked again
    assert calls == [1]


@pytest.mark.parametrize("seed", range(6))
def test_host_model_matches_the_restatement(seed):
    """random groups of 1 to 40 wells, two of them (40 producers, 20 injectors) with every well on its slot.  The host model sums left
    to right in double precision, the restatement exactly.  With n <= 40 members and u = 2^-53 the host's target carries at most
    (n + 3) u terms of error: n - 1 additions in each of the two sums, the products d . qs and e r, share, remainder and the final
    product and quotient -- terms = share (T + sum |r|) / e being the magnitude the remainder T - s sum r is formed from.  Held to the
    1e-14 RELATIVE the rule's statement asks: every target whose remainder does not cancel, terms <= 2 |target| (then the error is at
    most 2 * 43 u = 9.6e-15 of the target) -- all wells of the groups without a well under individual control among them, where
    terms = |target|.  Where the remainder cancels further, a relative bound is not what floating point gives: those are held to
    1e-14 of the terms."""
    rng = np.random.default_rng(100 + seed)
    n_prod, n_inj = 60, 25
    eff = np.where(rng.random(n_prod + n_inj) < 0.5, 1.0, rng.uniform(0.2, 1.0, n_prod + n_inj))
    wl = _wells(n_prod, n_inj, eff=eff)
    perm_p, perm_i = rng.permutation(n_prod), n_prod + rng.permutation(n_inj)
    sizes_p, sizes_i = [1, 40, 7, 9], [20, 3]
    pos = 0
    for k, n in enumerate(sizes_p):
        d = [(0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 1, 0)][k]
        wl.add_group("P%d" % k, -1, rng.uniform(20.0, 80.0) * n, d, perm_p[pos:pos + n], rng.uniform(0.1, 10.0, n))
        pos += n
    pos = 0
    for k, n in enumerate(sizes_i):
        wl.add_group("I%d" % k, +1, rng.uniform(20.0, 80.0) * n, (1, 0, 0), perm_i[pos:pos + n], rng.uniform(0.1, 10.0, n))
        pos += n
    nw = wl.nw
    slot = np.asarray([len(c) - 1 for c in wl.controls])
    current = np.where(rng.random(nw) < 0.5, slot, rng.integers(0, 2, nw))
    all_on_slot = list(wl.groups[1].wells) + list(wl.groups[4].wells)       # the 40 producers of P1 and the 20 injectors of I0
    current[all_on_slot] = slot[all_on_slot]
    sign = np.where(np.asarray(wl.type) == W.PRODUCER, -1.0, 1.0)
    qs = sign[:, None] * rng.uniform(0.0, 40.0, (nw, 3))
    ref, host, terms, _ = _both(wl, current, qs)
    member = ~np.isnan(ref)
    assert member.sum() == sum(sizes_p) + sum(sizes_i) and np.array_equal(np.isnan(host), ~member)
    err = np.abs(host - ref)
    strict = member & (terms <= 2.0 * np.abs(ref))
    assert strict[all_on_slot].all() and np.array_equal(terms[all_on_slot], np.abs(ref[all_on_slot])) and strict.sum() >= 61
    assert np.all(err[strict] <= 1e-14 * np.abs(ref[strict])), (err[strict] / np.abs(ref[strict])).max()
    assert np.all(err[member] <= 1e-14 * terms[member])
    assert (ref[member] != 0).sum() > member.sum() // 2


def test_a_decomposed_run_refuses_a_well_list_with_groups():
    """partition.LocalDomain.local_wells hands each rank its wells: a group's members may end up on several ranks, and dropping the groups
    there would let the field over-produce without a word"""
    from opmgpu import decks, partition
    grid = decks.cartesian_grid(4, 4, 2)
    wl = W.Wells()
    for w, cell in enumerate((0, 15)):
        wl.add_well("P%d" % w, W.PRODUCER, grid.z[cell], [cell], 1.0, (0.0, 1.0, 0.0), (W.BHP, 2e7))
    part = partition.slab_partition(grid, 2, axis=1)
    dom = partition.LocalDomain(grid, part, 0)
    assert dom.local_wells(wl, part).nw == 1
    wl.add_group("G", -1, 1.0, (0, 1, 0), [0, 1], [1.0, 1.0])
    with pytest.raises(ValueError, match="controlled groups \\(G\\).*decomposed run"):
        dom.local_wells(wl, part)

"""Finite-temperature state list and twin sectors, host logic (no GPU).

state_list replays es_add_state / es_pop_state (ED_EIGENSPACE.f90:138-218,
:231-295) and post_diag the data part of ed_post_diag (ED_DIAG.f90:494-565).
Checked on hand-worked lists and on SectorResults made from the dense spectrum
of the Ns = 5 model of finite_t_truth, where the thermal set is known exactly.
"""
import json
import os
import warnings

import numpy as np
import pytest

import finite_t_truth as ft
from edgpu.diag import DiagOptions, SectorResult, StateList, lanczos_params, post_diag, state_list
from edgpu.params import make_config
from edgpu.sectors import diag_sectors, get_sector, twin_sector

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _res(cfg, q, energies):
    s = get_sector(cfg)[q]
    return SectorResult(s.isector, q, s.dim, np.asarray(energies, dtype=float), len(energies))


def _entries(cfg, sl):
    by = {s.isector: (s.q1, s.q2) for s in get_sector(cfg).values()}
    return [(by[i], e, t is not None) for i, e, t in zip(sl.sectors, sl.energies, sl.twin_of)]


CFG3 = make_config(Norb=1, Nbath=2)     # Ns = 3: sectors (nup, ndw), isector = nup*4 + ndw + 1


def test_cap_passed_by_one_with_twin_pair():
    """cap 4: (1,1) [-1.0, 0.2] then (2,1) with twin [-1.5, 0.1] -> size 5."""
    opt = DiagOptions(lanc_nstates_total=4, ed_twin=True)
    sl = state_list([_res(CFG3, (1, 1), [-1.0, 0.2]), _res(CFG3, (2, 1), [-1.5, 0.1])], opt, CFG3)
    assert _entries(CFG3, sl) == [((2, 1), -1.5, False), ((1, 2), -1.5, True), ((1, 1), -1.0, False),
                                  ((2, 1), 0.1, False), ((1, 2), 0.1, True)]
    assert sl.twin_of == [None, 0, None, None, 3] and sl.vectors[1] is None and sl.finite_t
    assert sl.size == 5


def test_twin_pair_popped_together():
    """cap 2: (2,1) with twin [-1.5], then (2,2) [-2.0, -1.7]: the pair leaves as one."""
    opt = DiagOptions(lanc_nstates_total=2, ed_twin=True)
    sl = state_list([_res(CFG3, (2, 1), [-1.5]), _res(CFG3, (2, 2), [-2.0, -1.7])], opt, CFG3)
    assert _entries(CFG3, sl) == [((2, 2), -2.0, False), ((2, 2), -1.7, False)]


def test_cap_without_twins():
    opt = DiagOptions(lanc_nstates_total=4)
    res = [SectorResult(1, (0, 0), 9, np.array([-1.0, 0.5]), 2), SectorResult(2, (0, 1), 9, np.array([-2.0, 0.0]), 2),
           SectorResult(3, (0, 2), 9, np.array([-0.5, 3.0]), 2)]
    sl = state_list(reversed(res), opt)            # any input order: replayed in isector order
    assert sl.energies == [-2.0, -1.0, -0.5, 0.0] and sl.sectors == [2, 1, 3, 2]
    assert sl.twin_of == [None] * 4


def test_equal_energy_goes_in_front():
    """e <= c%e (ED_EIGENSPACE.f90:180): the later sector's equal level precedes."""
    opt = DiagOptions(lanc_nstates_total=6)
    res = [SectorResult(1, (0, 0), 9, np.array([-1.0, 0.0]), 2), SectorResult(2, (0, 1), 9, np.array([-1.0, 0.0]), 2)]
    sl = state_list(res, opt)
    assert sl.energies == [-1.0, -1.0, 0.0, 0.0] and sl.sectors == [2, 1, 2, 1]
    # a full list does not take a state equal to its last energy (e < last only)
    sl = state_list(res, DiagOptions(lanc_nstates_total=2))
    assert sl.energies == [-1.0, -1.0] and sl.sectors == [2, 1]


def test_zero_temperature_branch_carries_the_twin_flag():
    """ED_DIAG.f90:230,233: with ed_twin a kept ground state of an asymmetric
    sector brings its twin entry; weights are 1 each, zeta the size."""
    res = [_res(CFG3, (1, 1), [-1.0]), _res(CFG3, (2, 1), [-1.5, 0.1])]
    sl = state_list(res, DiagOptions(ed_twin=True), CFG3)
    assert _entries(CFG3, sl) == [((2, 1), -1.5, False), ((1, 2), -1.5, True)]
    assert not sl.finite_t and list(sl.weights()) == [1.0, 1.0] and sl.zeta == 2.0
    assert post_diag(sl, DiagOptions(ed_twin=True))[0] is sl
    with pytest.raises(ValueError):
        state_list(res, DiagOptions(ed_twin=True))       # the twin's isector needs the configuration


def test_options_setup_rounds_to_even():
    """ED_SETUP.f90:261-278: T=0 iff lanc_nstates_total == 1; otherwise both counts even."""
    d = DiagOptions()
    assert not d.finite_t and d.lanc_nstates_sector == 6 and d.lanc_nstates_total == 1
    o = DiagOptions(lanc_nstates_total=7, lanc_nstates_sector=5)
    assert o.finite_t and o.lanc_nstates_total == 8 and o.lanc_nstates_sector == 6
    assert lanczos_params(100, o)[0] == 6
    assert lanczos_params(100, DiagOptions(neigen_sector={4: 3}), 4)[0] == 3
    assert lanczos_params(100, DiagOptions(neigen_sector={4: 3}), 5)[0] == 6
    assert lanczos_params(2, DiagOptions(neigen_sector={4: 3}), 4)[0] == 2      # min(dim, .) ED_DIAG.f90:90


def test_diag_sectors_twin_mask():
    cfg = ft.config()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        secs = diag_sectors(cfg, ed_twin=True)
    assert len(diag_sectors(cfg)) == 36 and len(secs) == 21
    assert all(s.q1 >= s.q2 for s in secs)
    s = get_sector(cfg)[(3, 1)]
    assert (twin_sector(cfg, s).q1, twin_sector(cfg, s).q2) == (1, 3)
    sc = make_config(Norb=1, Nbath=2, ed_mode="superc")
    assert [s.q1 for s in diag_sectors(sc, True)] == [-3, -2, -1, 0]
    assert twin_sector(sc, get_sector(sc)[(-2, 0)]).q1 == 2
    ns = make_config(Norb=1, Nbath=2, Nspin=2, ed_mode="nonsu2")
    with pytest.warns(RuntimeWarning):                     # Nspin > 1 (ED_SETUP.f90:69-70)
        assert [s.q1 for s in diag_sectors(ns, True)] == [0, 1, 2, 3]
    assert twin_sector(ns, get_sector(ns)[(1, 0)]).q1 == 5
    import cases

    with pytest.raises(NotImplementedError):
        diag_sectors(cases.nonsu2_jz(), True)
    # configs[3] (Ns = 12): 91 of its 169 sectors
    from golden.golden_configs import c4_config

    assert len(diag_sectors(c4_config("flat"), True)) == 91


@pytest.mark.parametrize("ed_twin", [False, True])
def test_thermal_set_of_the_dense_spectrum(ed_twin):
    """state_list + post_diag on the 6 lowest dense levels of every sector
    keep exactly {E : exp(-beta (E - E0)) > cutoff} of the full spectrum."""
    T = ft.truth()
    per_sector = {}
    for _, i, _ in T.kept:
        per_sector[i] = per_sector.get(i, 0) + 1
    # preconditions on the truth itself: 6 per sector and a cap of 40 lose nothing
    assert max(per_sector.values()) <= 5 and len(T.kept) <= 38
    assert len(T.kept) == 15 and len(per_sector) == 8 and max(per_sector.values()) == 4
    allw = np.sort(np.concatenate(list(T.w.values())))
    gap = np.min(np.abs(-np.log(ft.CUTOFF) / ft.BETA - (allw - T.e0)))
    print(f"thermal set: {len(T.kept)} states, nearest level {gap:.3f} from the threshold")
    assert gap > 0.05

    opt = DiagOptions(lanc_nstates_total=ft.NTOTAL, beta=ft.BETA, cutoff=ft.CUTOFF, ed_twin=ed_twin)
    res = T.sector_results(6, ed_twin)
    assert len(res) == (21 if ed_twin else 36)
    sl = state_list(res, opt, T.cfg)
    assert sl.energies == sorted(sl.energies) and sl.size > 15
    sl2, opt2 = post_diag(sl, opt, T.cfg)
    print("kept:", [f"{e:.6f}" for e in sl2.energies])
    assert sl2.size == 15
    # twin-symmetric to 1.5e-14: a twin entry reports its partner's energy
    assert np.max(np.abs(np.sort(sl2.energies) - T.energies)) < 1e-12
    assert sorted(sl2.sectors) == sorted(i for _, i, _ in T.kept)
    assert opt2.lanc_nstates_total == max(15, 2) + 2
    assert abs(sl2.zeta - T.zeta) < 1e-12 and np.all(sl2.weights() > ft.CUTOFF)
    if ed_twin:
        ntw = 0
        for k, p in enumerate(sl2.twin_of):
            if p is None:
                continue
            ntw += 1
            a, b = T.secs[sl2.sectors[p] - 1], T.secs[sl2.sectors[k] - 1]
            assert p == k - 1 and (b.q1, b.q2) == (a.q2, a.q1) and a.q1 > a.q2
            assert sl2.energies[k] == sl2.energies[p] and sl2.vectors[k] is None
        assert ntw == sum(1 for _, i, _ in T.kept if T.secs[i - 1].q1 < T.secs[i - 1].q2)
    else:
        assert sl2.twin_of == [None] * 15
    # neigen_sector (ED_DIAG.f90:505-515): min(dim, 6) + 1 clamped to count + 1 where present;
    # elsewhere min(dim, 6) - 1, which exceeds the count 0 and is clamped to 0 + 1 as well.
    # The counts are those of the list before it is trimmed (:494-502 precede :533-556).
    for s in T.secs:
        assert opt2.neigen_sector[s.isector] == sl.sectors.count(s.isector) + 1, s


def test_increase_branch_keeps_the_list():
    T = ft.truth()
    opt = DiagOptions(lanc_nstates_total=8, beta=ft.BETA, cutoff=ft.CUTOFF)
    sl = state_list(T.sector_results(6), opt, T.cfg)
    assert sl.size == 8 and np.max(np.abs(np.array(sl.energies) - T.energies[:8])) < 1e-12
    sl2, opt2 = post_diag(sl, opt, T.cfg)
    assert opt2.lanc_nstates_total == 10 and sl2.energies == sl.energies and sl2.sectors == sl.sectors


def test_farm_owner_of_a_twin_entry_is_its_partners():
    """farm_diag with ed_twin: a twin entry names a sector no rank solved; its
    owner is the rank that holds the partner's vector, which the list keeps."""
    from edgpu.farm import farm_diag

    T = ft.truth()
    by = {r.isector: r for r in T.sector_results(6, True, vectors=True)}
    opt = DiagOptions(lanc_nstates_total=ft.NTOTAL, beta=ft.BETA, cutoff=ft.CUTOFF, ed_twin=True)
    fr = farm_diag(T.cfg, opt, solver=lambda cfg, sec, o, dev: by[sec.isector])
    assert sorted(fr.local) == sorted(by) and fr.owners == [0] * fr.states.size
    ref = state_list(by.values(), opt, T.cfg)
    assert fr.states.energies == ref.energies and fr.states.sectors == ref.sectors
    assert fr.states.twin_of == ref.twin_of and any(p is not None for p in ref.twin_of)
    assert fr.states.finite_t and fr.states.beta == ft.BETA
    for k, p in enumerate(fr.states.twin_of):
        assert (fr.states.vectors[k] is None) == (p is not None)


def test_neigen_sector_update_and_clamps():
    sl = StateList([-1.0, -0.9, -0.8, -0.7], [1, 1, 1, 2], [None] * 4, finite_t=True, beta=1.0)
    opt = DiagOptions(lanc_nstates_total=4, beta=1.0, cutoff=1e-9, neigen_sector={1: 2, 2: 5, 3: 1, 4: 3})
    _, o = post_diag(sl, opt)
    # 1: 2+1 = 3 (count 3: no clamp); 2: 5+1 -> count+1 = 2; 3: 1-1 -> 1; 4: 3-1 -> count+1 = 1
    assert o.neigen_sector == {1: 3, 2: 2, 3: 1, 4: 1}
    assert o.lanc_nstates_total == 6 and opt.neigen_sector == {1: 2, 2: 5, 3: 1, 4: 3}


@pytest.mark.parametrize("bath", ["flat", "random"])
def test_defaults_reproduce_the_committed_t0_lists(bath):
    with open(os.path.join(GOLD, f"c4_diag_{bath}.json")) as fh:
        d = json.load(fh)
    res = [SectorResult(int(k), tuple(g["q"]), g["dim"], np.asarray(g["eigenvalues"]), len(g["eigenvalues"]))
           for k, g in d["sectors"].items()]
    sl = state_list(res, DiagOptions())
    assert sl.sectors == d["states"]["sectors"] and sl.energies == d["states"]["energies"]
    assert sl.twin_of == [None] * sl.size and not sl.finite_t
    assert list(sl.weights()) == [1.0] * sl.size and sl.zeta == float(sl.size)

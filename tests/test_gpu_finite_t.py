"""Finite-temperature diagonalisation, Green's function and observables on the
MI355X against the dense thermal sums of finite_t_truth (Ns = 5, beta = 8,
cutoff = 1e-4: 15 states over 8 sectors), with ed_twin off and on.

lanc_dim_threshold = 16 sends the 25-, 50- and 100-row sectors through the
device eigensolver, so their kept vectors are device tensors and the twin
entries of the 50- and 100-row sectors are rebuilt by ed_sector_twin_vector;
the smaller sectors are dense (host vectors, uploaded for the twin map).

Bars: energies 1e-10 (the solver's 1e-12 residual tolerance on |E| < 10);
G(iw) 1e-10 of max|G| (the project's bar for G(iw)); observables 1e-9 (the
end-to-end bar of test_gpu_obs: eigenvectors carry the solver's tolerance).

G(w) on the real axis is held to the project's real-axis bar, 1e-5 of max|G|
(test_gpu_diag_gf), not to 1e-10: the continued fraction comes from the
reference's plain Lanczos without reorthogonalisation (sp_lanc_tridiag,
nlanc = min(dim, lanc_nGFiter) = dim here), whose Ritz values inside the
spectrum are not all eigenvalues once orthogonality is lost, and eps = 0.01
weighs a pole-position error by 1/eps^2.  A numpy replay of that recurrence
on this model's dense blocks (every seed of the 15 kept states, nlanc = dim)
differs from the exact resolvent by up to 1.3e-5 of max|G(w)| per seed and by
1.5e-14 on the Matsubara axis; the same recurrence with full
reorthogonalisation gives 3.0e-13 and 1.5e-14.  So the distance on the real
axis belongs to the algorithm the reference prescribes, and 1e-10 is not
reachable there by any implementation of it.  Measured on the MI355X: G(iw)
8.0e-14 (ed_twin off) and 6.5e-15 (on), G(w) 1.2e-7 both; twin on against off
8.1e-14 and 5.5e-9.
"""
import json
import os

import numpy as np
import pytest

import finite_t_truth as ft
from edgpu.diag import DiagOptions, ed_diag, post_diag, state_vector, to_host
from edgpu.gf import GFOptions, build_gf, matsubara, realaxis
from edgpu.observables import observables
from edgpu.params import make_config
from edgpu.sectors import get_sector

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOPT = GFOptions(Lmats=16, Lreal=16, beta=ft.BETA)
_RUN = {}


def run(ed_twin):
    """ed_diag + post_diag + build_gf + observables, once per ed_twin."""
    if ed_twin not in _RUN:
        T = ft.truth()
        opt = DiagOptions(lanc_dim_threshold=16, lanc_nstates_total=ft.NTOTAL, beta=ft.BETA, cutoff=ft.CUTOFF,
                          ed_twin=ed_twin)
        res, sl = ed_diag(T.cfg, opt)
        sl2, opt2 = post_diag(sl, opt, T.cfg)
        Gm, Gr = build_gf(T.cfg, sl2, GOPT)
        _RUN[ed_twin] = dict(res=res, sl=sl, sl2=sl2, opt2=opt2, Gm=Gm[0, 0, 0, 0], Gr=Gr[0, 0, 0, 0],
                             obs=observables(T.cfg, sl2))
    return _RUN[ed_twin]


@pytest.mark.parametrize("ed_twin", [False, True])
def test_energies_match_the_dense_thermal_set(ed_twin):
    T, r = ft.truth(), run(ed_twin)
    assert len(r["res"]) == (21 if ed_twin else 36)
    assert {x.method for x in r["res"]} == {"dense", "arpack"}
    sl2 = r["sl2"]
    d = np.max(np.abs(np.sort(sl2.energies) - T.energies)) if sl2.size == 15 else np.inf
    print(f"ed_twin={ed_twin}: {r['sl'].size} -> {sl2.size} states, max |E - truth| = {d:.3e}")
    assert sl2.size == 15 and d < 1e-10
    assert sorted(sl2.sectors) == sorted(i for _, i, _ in T.kept)
    assert r["opt2"].lanc_nstates_total == 17 and abs(sl2.zeta - T.zeta) < 1e-8
    ntwin = sum(p is not None for p in sl2.twin_of)
    assert ntwin == (sum(1 for _, i, _ in T.kept if T.secs[i - 1].q1 < T.secs[i - 1].q2) if ed_twin else 0)
    if ed_twin:       # a twin entry's vector is an eigenvector of the twin sector's dense block
        for k, p in enumerate(sl2.twin_of):
            if p is None:
                continue
            assert sl2.vectors[k] is None
            v = to_host(state_vector(T.cfg, sl2, k))
            i = sl2.sectors[k]
            idx = T.maps[i]
            blk = T.H[idx][:, idx].toarray().real
            resid = np.linalg.norm(blk @ v - sl2.energies[k] * v)
            assert abs(np.linalg.norm(v) - 1.0) < 1e-10 and resid < 1e-8, (k, resid)


@pytest.mark.parametrize("ed_twin", [False, True])
def test_gf_matches_the_dense_thermal_sum(ed_twin):
    T, r = ft.truth(), run(ed_twin)
    Gm0, Gr0 = T.gf(matsubara(GOPT.beta, GOPT.Lmats), realaxis(GOPT.wini, GOPT.wfin, GOPT.Lreal), GOPT.eps)
    rel_m = np.max(np.abs(r["Gm"] - Gm0)) / np.max(np.abs(Gm0))
    rel_r = np.max(np.abs(r["Gr"] - Gr0)) / np.max(np.abs(Gr0))
    print(f"ed_twin={ed_twin}: G(iw) rel diff {rel_m:.3e}, G(w) rel diff {rel_r:.3e}")
    assert rel_m < 1e-10
    assert rel_r < 1e-5       # plain-Lanczos continued fraction at eps = 0.01: see the module docstring


def test_twin_on_and_off_agree():
    a, b = run(False), run(True)
    rel_m = np.max(np.abs(a["Gm"] - b["Gm"])) / np.max(np.abs(a["Gm"]))
    rel_r = np.max(np.abs(a["Gr"] - b["Gr"])) / np.max(np.abs(a["Gr"]))
    de = np.max(np.abs(np.sort(a["sl2"].energies) - np.sort(b["sl2"].energies)))
    print(f"twin on/off: G(iw) {rel_m:.3e}, G(w) {rel_r:.3e}, energies {de:.3e}")
    assert rel_m < 1e-10 and de < 1e-10
    assert rel_r < 1e-5       # as above: the two runs' seeds differ in the last bits
    for f in ("dens", "dens_up", "dens_dw", "docc"):
        assert np.max(np.abs(getattr(a["obs"], f) - getattr(b["obs"], f))) < 1e-9


@pytest.mark.parametrize("ed_twin", [False, True])
def test_observables_match_the_dense_thermal_averages(ed_twin):
    T, o = ft.truth(), run(ed_twin)["obs"]
    up, dw, docc = T.observables()
    d = max(abs(o.dens_up[0] - up), abs(o.dens_dw[0] - dw), abs(o.docc[0] - docc), abs(o.dens[0] - up - dw))
    print(f"ed_twin={ed_twin}: dens_up {o.dens_up[0]:.12f} dens_dw {o.dens_dw[0]:.12f} docc {o.docc[0]:.12f}, "
          f"max deviation {d:.3e}")
    assert d < 1e-9
    assert abs(o.egs - T.e0) < 1e-10


def test_beta_mismatch_is_refused():
    T, r = ft.truth(), run(False)
    with pytest.raises(ValueError, match="beta"):
        build_gf(T.cfg, r["sl2"], GFOptions(Lmats=16, Lreal=16))      # beta = 1000


def test_default_options_reproduce_the_t0_green_function():
    """The default (T=0) path did not move: configs[1] with its random bath
    gives the committed E0 (tests/golden/c2_e0.json) and, bit for bit, the G
    recorded from the commit before finite temperature was added
    (tests/golden/c2_gf_t0.npz: ground-state sector (4,4), Lmats = Lreal = 16)."""
    with open(os.path.join(GOLD, "c2_e0.json")) as fh:
        e0 = json.load(fh)["by_seed"]["20251015"]["E0"]
    cfg = make_config(Norb=1, Nbath=7, bath="random", seed=20251015)
    _, sl = ed_diag(cfg, DiagOptions(), sectors=[get_sector(cfg)[(4, 4)].isector])
    assert sl.size == 1 and not sl.finite_t and sl.twin_of == [None]
    assert abs(sl.energies[0] - e0) < 1e-10
    Gm, Gr = build_gf(cfg, sl, GFOptions(Lmats=16, Lreal=16))
    g = np.load(os.path.join(GOLD, "c2_gf_t0.npz"))
    assert sl.energies[0] == float(g["E0"])
    assert np.array_equal(Gm, g["Gm"]) and np.array_equal(Gr, g["Gr"])

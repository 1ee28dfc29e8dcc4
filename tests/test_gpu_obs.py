"""ed_sector_nn_moments / ed_sector_expect (k_nn_moments, k_expect) and
edgpu.observables / local_energy on the MI355X.

Truth: the full-Fock Jordan-Wigner matrices of oracle.jw_dense._ops multiplied
in string order and restricted to the sector (obs_truth.dense_expect), on
random unit vectors.  Tolerance 1e-12 absolute: for a unit vector every sum has
sum_i |terms| <= 1; a thread adds at most dim/grid/256 = 1 term here and the
wave, block and grid stages are pairwise or short fixed-order sums, so the
rounding error is a few eps * log2(dim) = 3e-15, far inside the bound.  End to
end after ed_diag: 1e-9 (the eigenvectors carry the solver's 1e-12 residual
tolerance).
"""
import ctypes

import numpy as np
import pytest

import cases
import obs_truth as ot
from edgpu import _lib
from edgpu.hamiltonian import Sector
from edgpu.params import make_config
from edgpu.sectors import c_sector, cdg_sector, get_sector

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1] for c in cases.CASES}
SMALL = lambda: make_config(Norb=1, Nbath=2)   # noqa: E731
CASES["small"] = SMALL
# (case, sector, vector types): both vector types on the real-H cases
MATRIX = [("normal_jh", (3, 3), (False, True)), ("nonsu2_rand", (5, 0), (True,)),
          ("superc_2orb", (1, 0), (False, True)), ("nonsu2_jz", (5, 1), (True,)),
          ("c2", (4, 4), (False, True)),            # dim 4,900: 20 blocks, second reduction stage
          ("hybrid", (3, 3), (False, True)),        # inter-orbital hops through the shared bath
          ("small", (0, 0), (True,)),               # dim 1: one block, 255 idle lanes
          ("small", (1, 1), (False, True)),         # dim 9: below one wavefront
          ("c2", (3, 5), (True,)),                  # dim 3,136 = 12*256 + 64: partial tail block
          ("c2", (3, 4), (True,))]                  # dim 3,920 = 15*256 + 80: partial tail block


def strings(cfg):
    """Impurity strings plus hops among the first three levels of each spin
    (bath levels included); split into accepted and refused by the dense
    commutator test."""
    Ns = cfg.Ns
    lv = [l for l in (0, 1, 2) if l < Ns] + [Ns + l for l in (0, 1, 2) if l < Ns]
    terms = ot.hop_terms(cfg) + ot.number_terms(cfg) + ot.pair_terms(cfg)
    terms += [[(p, 1), (q, 0)] for p in lv for q in lv if p != q]
    if cfg.Norb > 1:
        terms += ot.exchange_terms(cfg)
    uniq = []
    for t in terms:
        if t not in uniq:
            uniq.append(t)
    ok = [t for t in uniq if ot.dense_term(2 * Ns, t).nnz == 0 or ot.dense_conserves(cfg, t)]
    return ok, [t for t in uniq if t not in ok]


_SPLIT = {}


def split_strings(name):
    if name not in _SPLIT:
        _SPLIT[name] = strings(CASES[name]())
    return _SPLIT[name]


def open_sector(cfg, q, **kw):
    return Sector(cfg, q[0], q[1], stored=False, direct=True, real=cfg.is_real(), **kw)


@pytest.mark.parametrize("name,q,vtypes", MATRIX)
def test_moments_and_expect_match_dense(name, q, vtypes):
    cfg = CASES[name]()
    nlev = 2 * cfg.Ns
    ok, _ = split_strings(name)
    lv = ot.imp_levels(cfg)
    with open_sector(cfg, q) as S:
        hmap = S.map()
        for cplx in vtypes:
            vec = ot.random_state(S.dim, cplx, seed=S.dim + cplx)
            M, norm = S.nn_moments(vec, lv)
            vals = S.expect(vec, ok)
            vc = vec.astype(np.complex128)
            dM = max(abs(M[a, b] - ot.dense_expect(nlev, hmap, vc, [(p, 1), (p, 0), (r, 1), (r, 0)]))
                     for a, p in enumerate(lv) for b, r in enumerate(lv))
            dv = max(abs(v - ot.dense_expect(nlev, hmap, vc, t)) for v, t in zip(vals, ok))
            print(f"{name} {q} dim {S.dim} complex={cplx}: {len(ok)} strings, moments {dM:.3e}, expect {dv:.3e}, "
                  f"norm-1 {norm - 1.0:.3e}")
            assert dM < 1e-12 and dv < 1e-12 and abs(norm - 1.0) < 1e-12
            if not cplx:
                assert np.all(vals.imag == 0.0)
            # one string alone, one more than a register tile, more than one launch's worth
            for n in (1, _lib.OBS_TILE + 3, _lib.OBS_MAX_TERMS + 5):
                rep = [ok[k % len(ok)] for k in range(n)]
                got = S.expect(vec, rep)
                assert np.array_equal(got, np.array([vals[k % len(ok)] for k in range(n)]))
            # hermiticity: <c+_p c_q> = conj <c+_q c_p>
            for t, v in zip(ok, vals):
                if len(t) == 2 and t[0][1] == 1 and t[1][1] == 0 and t[0][0] != t[1][0]:
                    back = [(t[1][0], 1), (t[0][0], 0)]
                    assert abs(v - np.conj(vals[ok.index(back)])) < 1e-13


def _expect_rc(S, x, terms):
    L = _lib.load()
    nops = np.array([len(t) for t in terms], dtype=np.int32)
    lv = np.array([l for t in terms for l, _ in t] or [0], dtype=np.int32)
    op = np.array([o for t in terms for _, o in t] or [0], dtype=np.int32)
    out = np.full(2 * max(len(terms), 1), 7.0)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    rc = L.ed_sector_expect(S.handle, 1, ctypes.c_void_p(x.data_ptr()), len(terms), P(nops), P(lv), P(op), P(out),
                            None)
    return rc, out


def test_refusals_return_codes():
    """Row-split sectors and every string that leaves the sector come back as
    error codes (ED_ERR_UNSUPPORTED = 5, ED_ERR_ARG = 1) with nothing written."""
    import torch

    L = _lib.load()
    for name, q in (("normal_jh", (3, 3)), ("superc_2orb", (1, 0)), ("nonsu2_jz", (5, 1)), ("nonsu2_rand", (5, 0))):
        cfg = CASES[name]()
        ok, bad = split_strings(name)
        assert bad
        with open_sector(cfg, q) as S:
            x = torch.from_numpy(ot.random_state(S.dim, True, 2)).cuda()
            torch.cuda.synchronize()
            for t in bad + [[], [(0, 1), (0, 0)] * 2 + [(0, 1)], [(2 * cfg.Ns, 1), (2 * cfg.Ns, 0)]]:
                rc, out = _expect_rc(S, x, [ok[0], t])
                assert rc == 1 and np.all(out == 7.0), (t, rc)
            lv = np.array([0, 2 * cfg.Ns], dtype=np.int32)
            o = np.zeros(4)
            assert L.ed_sector_nn_moments(S.handle, 1, ctypes.c_void_p(x.data_ptr()), 2,
                                          ctypes.c_void_p(lv.ctypes.data), ctypes.c_void_p(o.ctypes.data), None) == 1
            assert L.ed_sector_nn_moments(S.handle, 1, ctypes.c_void_p(x.data_ptr()), 7,
                                          ctypes.c_void_p(lv.ctypes.data), ctypes.c_void_p(o.ctypes.data), None) == 1
    cfg = CASES["c2"]()
    with Sector(cfg, 4, 4, stored=True, rows=(256, 512)) as R:
        x = torch.from_numpy(ot.random_state(R.dim, True, 2)).cuda()
        torch.cuda.synchronize()
        rc, out = _expect_rc(R, x, [[(0, 1), (0, 0)]])
        assert rc == 5 and np.all(out == 7.0)
        lv = np.array([0], dtype=np.int32)
        o = np.full(2, 7.0)
        assert L.ed_sector_nn_moments(R.handle, 1, ctypes.c_void_p(x.data_ptr()), 1, ctypes.c_void_p(lv.ctypes.data),
                                      ctypes.c_void_p(o.ctypes.data), None) == 5
        assert np.all(o == 7.0)


def test_sum_rule_and_determinism():
    """Normal mode: the occupations of all 2*Ns levels, six at a time, add up
    to nup + ndw; two calls on the same input return the same bytes."""
    cfg = CASES["c2"]()
    ok, _ = split_strings("c2")
    with open_sector(cfg, (4, 4)) as S:
        vec = ot.random_state(S.dim, True, 11)
        tot = 0.0
        for l0 in range(0, 2 * cfg.Ns, 6):
            lv = list(range(l0, min(l0 + 6, 2 * cfg.Ns)))
            M, norm = S.nn_moments(vec, lv)
            M2, norm2 = S.nn_moments(vec, lv)
            assert M.tobytes() == M2.tobytes() and norm == norm2
            tot += float(np.trace(M))
        print(f"sum of occupations - 8 = {tot - 8.0:.3e}")
        assert abs(tot - 8.0) < 1e-12
        a, b = S.expect(vec, ok), S.expect(vec, ok)
        assert a.tobytes() == b.tobytes()
        # a stored sector's handle serves as well as a direct one
        with Sector(cfg, 4, 4, stored=True, real=True) as T:
            assert T.expect(vec, ok).tobytes() == a.tobytes()


def _apply(src, dst, op, level, x, y=None, coef=None):
    import torch

    L = _lib.load()
    vt = 1 if x.is_complex() else 0
    st = torch.cuda.current_stream()
    P = ctypes.c_void_p
    if y is None:
        y = torch.empty(dst.dim, dtype=x.dtype, device=x.device)
        _lib.check(L.ed_sector_apply_op(src.handle, dst.handle, op, level, vt, P(x.data_ptr()), P(y.data_ptr()),
                                        P(st.cuda_stream)), "apply_op")
    else:
        _lib.check(L.ed_sector_apply_op_acc(src.handle, dst.handle, op, level, float(coef.real), float(coef.imag), vt,
                                            P(x.data_ptr()), P(y.data_ptr()), P(st.cuda_stream)), "apply_op_acc")
    return y


def test_cross_check_with_apply_op():
    """<c+_p c_q> = <c_p psi | c_q psi> with the GF seed kernels (k_apply_op)
    in the N-1 sector, and magX / magY / phisc through the reference's
    seed-norm route (ED_OBSERVABLES.f90:166-337) built with ed_sector_apply_op
    / _acc."""
    import torch

    cfg = CASES["normal_jh"]()
    sec = get_sector(cfg)[(3, 3)]
    low = c_sector(cfg, sec, 0)
    with open_sector(cfg, (3, 3)) as S, open_sector(cfg, (low.q1, low.q2)) as T:
        for cplx in (False, True):
            x = torch.from_numpy(ot.random_state(S.dim, cplx, 21)).cuda()
            y0, y1 = _apply(S, T, 0, 0, x), _apply(S, T, 0, 1, x)
            dot = torch.vdot(y0, y1).item() if cplx else torch.dot(y0, y1).item()
            got = S.expect(x, [[(0, 1), (1, 0)]])[0]
            print(f"<c+_0 c_1> complex={cplx}: expect {got}, apply_op dot {dot}, diff {abs(got - dot):.3e}")
            assert abs(got - dot) < 1e-12

    cfg = CASES["nonsu2_rand"]()
    Ns = cfg.Ns
    sec = get_sector(cfg)[(5, 0)]
    low = c_sector(cfg, sec, 0)
    with open_sector(cfg, (5, 0)) as S, open_sector(cfg, (low.q1, low.q2)) as T:
        x = torch.from_numpy(ot.random_state(S.dim, True, 22)).cuda()
        M, _ = S.nn_moments(x, ot.imp_levels(cfg))
        for a in range(cfg.Norb):
            nu, nd = M[a, a], M[cfg.Norb + a, cfg.Norb + a]
            y = _apply(S, T, 0, a, x)
            _apply(S, T, 0, a + Ns, x, y, 1 + 0j)
            magx = 0.5 * (torch.sum(y.abs() ** 2).item() - nu - nd)
            y = torch.zeros(T.dim, dtype=x.dtype, device=x.device)
            _apply(S, T, 0, a, x, y, 1j)
            _apply(S, T, 0, a + Ns, x, y, 1 + 0j)
            magy = 0.5 * (torch.sum(y.abs() ** 2).item() - nu - nd)
            z = S.expect(x, [[(a, 1), (a + Ns, 0)]])[0]
            print(f"orbital {a}: magx {z.real:.15f} (seed norm {magx:.15f}), magy {z.imag:.15f} ({magy:.15f})")
            assert abs(z.real - magx) < 1e-12 and abs(z.imag - magy) < 1e-12

    cfg = CASES["superc_2orb"]()
    Ns = cfg.Ns
    sec = get_sector(cfg)[(1, 0)]
    up = cdg_sector(cfg, sec, 0)
    with open_sector(cfg, (1, 0)) as S, open_sector(cfg, (up.q1, up.q2)) as T:
        x = torch.from_numpy(ot.random_state(S.dim, True, 23)).cuda()
        M, _ = S.nn_moments(x, ot.imp_levels(cfg))
        for a in range(cfg.Norb):
            nu, nd = M[a, a], M[cfg.Norb + a, cfg.Norb + a]
            y = _apply(S, T, 1, a, x)
            _apply(S, T, 0, a + Ns, x, y, 1 + 0j)
            phi_ref = 0.5 * (torch.sum(y.abs() ** 2).item() - nu - (1.0 - nd))
            phi = S.expect(x, [[(a, 0), (a + Ns, 0)]])[0].real + nd - nu
            print(f"orbital {a}: phisc {phi:.15f} (seed norm {phi_ref:.15f})")
            assert abs(phi - phi_ref) < 1e-12


@pytest.mark.parametrize("name", ["normal_jh", "nonsu2_rand", "superc"])
def test_end_to_end_matches_dense_eigh(name):
    """ed_diag (device vectors) -> observables + local_energy against the dense
    eigh of every sector traced over the ground multiplet."""
    from edgpu.diag import DiagOptions, ed_diag
    from edgpu.observables import local_energy, observables

    cfg = CASES[name]()
    _, sl = ed_diag(cfg, DiagOptions())
    ref = ot.dense_ground_states(cfg)
    assert sorted(sl.sectors) == sorted(ref.sectors)
    truth = ot.dense_observables(cfg, ref)
    obs, ene = observables(cfg, sl), local_energy(cfg, sl)
    dev = ot.max_deviation(obs, ene, truth)
    print(f"{name}: {sl.size} kept state(s), dens {obs.dens}, epot {ene.epot:.12f}, eknot {ene.eknot:.12f}, "
          f"max deviation {dev:.3e}")
    assert dev < 1e-9


def test_particle_hole_symmetry_c2():
    """c2 (flat bath, xmu = 0, hfmode): dens = 1 and magz = 0."""
    from edgpu.diag import DiagOptions, ed_diag
    from edgpu.observables import observables

    cfg = CASES["c2"]()
    _, sl = ed_diag(cfg, DiagOptions())
    obs = observables(cfg, sl)
    print(f"c2: {sl.size} kept state(s), dens - 1 = {obs.dens[0] - 1.0:.3e}, magz = {obs.magz[0]:.3e}, "
          f"docc = {obs.docc[0]:.12f}")
    assert abs(obs.dens[0] - 1.0) < 1e-9 and abs(obs.magz[0]) < 1e-9

"""Host restatements for the susceptibility tests (test infrastructure only).

chi_poles_host   the arithmetic of k_chi_poles (csrc/ed_poles.hip) in numpy:
                 the same formulas in the same order of additions, vectorised
                 over the grid points only.
numpy_seeds      the seeds of ed_sector_seed_diag: the factor summed in level
                 order, times the vector.
replay_chi       build_chi with every device piece replaced: numpy seeds, the
                 oracle's plain Lanczos (lanczos_plain_tridiag_c) with the
                 device's breakdown threshold, `tridiag_poles`, chi_poles_host.
"""
import numpy as np

from edgpu.chi import (assemble, bosonic_matsubara, n_components, seed_levels, seed_table, tau_grid)
from edgpu.gf import _peso_bz, realaxis, tridiag_poles
from edgpu.sectors import setup_pointers


def thermal_host(beta, D):
    """(1 - exp(-beta D), s(D)) as chi_thermal (csrc/ed_chi_host.hpp)."""
    D = np.asarray(D, dtype=np.float64)
    f = -np.expm1(-beta * D)
    s = np.where(D == 0.0, beta, f / np.where(D == 0.0, 1.0, D))
    return f, s


def _cdiv(pr, a, b):
    """(pr, 0) / (a, b) by Smith's algorithm, as cdiv of ed_kernels.hpp with p.y = 0."""
    a, b = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float))
    with np.errstate(divide="ignore", invalid="ignore"):
        r1 = b / a
        d1 = a + b * r1
        x1, y1 = (pr + 0.0 * r1) / d1, (0.0 - pr * r1) / d1
        r2 = a / b
        d2 = a * r2 + b
        x2, y2 = (pr * r2 + 0.0) / d2, (0.0 * r2 - pr) / d2
    first = np.abs(b) <= np.abs(a)
    return np.where(first, x1, x2) + 1j * np.where(first, y1, y2)


def chi_poles_host(fracs, beta, vm, tau, wr, eps, ncomp, start=None):
    """fracs: (comp, peso, Ei, E, z) or (comp, peso, Ei, E, z, isign) in queue
    order; isign 0 (both branches, the default), +1 or -1: the selector of
    ed_chi_add_poles_signed, the branch that is not selected left out.  Returns
    (iv, tau, w, (sum |terms| of iv, tau, w)) — the arrays start from `start` =
    (iv, tau, w) (a second flush) or zero."""
    vm, tau, wr = (np.asarray(x, float) for x in (vm, tau, wr))
    civ = np.zeros((ncomp, len(vm)), complex) if start is None else np.array(start[0])
    ctau = np.zeros((ncomp, len(tau))) if start is None else np.array(start[1])
    cw = np.zeros((ncomp, len(wr)), complex) if start is None else np.array(start[2])
    mag = [np.abs(civ), np.abs(ctau), np.abs(cw)]
    tm = beta - tau
    for comp, peso, ei, E, z, *sel in fracs:
        isign = sel[0] if sel else 0
        assert isign in (0, 1, -1)
        E, z = np.asarray(E, float), np.asarray(z, float)
        f, s = thermal_host(beta, E - ei)
        for sg in (0, 1):                      # isign = +1, then -1
            if isign == (1 if sg else -1):     # a one-sign fraction: the other branch is not its
                continue
            for j in range(len(E)):
                de = E[j] - ei
                pj = (peso * z[j]) * z[j]
                t0 = pj * s[j]
                civ[comp, 0] = civ[comp, 0] + t0
                mag[0][comp, 0] += abs(t0)
                tt = pj * np.exp(-(tm if sg else tau) * de)
                ctau[comp] = ctau[comp] + tt
                mag[1][comp] += np.abs(tt)
                num = pj * f[j]
                if sg:
                    ci, cr = _cdiv(num, 0.0 + de, vm[1:]), _cdiv(num, wr + de, np.full(len(wr), eps))
                else:
                    ci, cr = _cdiv(-num, 0.0 - de, vm[1:]), _cdiv(-num, wr - de, np.full(len(wr), eps))
                civ[comp, 1:] = civ[comp, 1:] + ci
                cw[comp] = cw[comp] + cr
                mag[0][comp, 1:] += np.abs(ci)
                mag[2][comp] += np.abs(cr)
    return civ, ctau, cw, tuple(mag)


def row_factor(hmap, levels, w):
    """sum_l w[l] * bit(state, levels[l]), added in level order in double."""
    c = np.zeros(len(hmap))
    for lv, wl in zip(levels, w):
        c = c + wl * ((np.asarray(hmap) >> np.uint32(lv)) & np.uint32(1)).astype(np.float64)
    return c


def numpy_seeds(hmap, levels, weights, x):
    """Unnormalised seeds (nseed, dim) of the vector's type."""
    return np.array([row_factor(hmap, levels, w) * x for w in weights])


def replay_chi(cfg, states, copt, spin=True, dens=True, record=None):
    """build_chi on the host; the same queue order (kept state, then seed)."""
    from oracle.oracle import Oracle, lanc_tridiag
    from oracle_gf_superc import host_state_vector

    orc = Oracle(cfg)
    table, levels = seed_table(cfg, spin, dens), seed_levels(cfg)
    secs = setup_pointers(cfg)
    zeta = states.zeta if states.finite_t else float(states.size)
    fracs = []
    for k, isec in enumerate(states.sectors):
        sec = secs[isec - 1]
        hmap = orc.build_sector(sec.q1, sec.q2)
        # a twin entry's vector from its partner by flip_state, without the superc sign
        vec = host_state_vector(cfg, orc, states, k, sign=False).astype(np.complex128)
        csr = orc.build_csr(hmap)
        nlanc = min(len(hmap), copt.lanc_nGFiter)
        for name, comp, w in table:
            v = row_factor(hmap, levels, w) * vec
            norm2 = float(np.vdot(v, v).real)
            if norm2 == 0.0:
                continue
            a, b, n = lanc_tridiag(csr, v / np.sqrt(norm2), nlanc, copt.threshold)
            E, z = tridiag_poles(a, b, nlanc, first_row=True)
            if record is not None:
                record.append(dict(name=name, comp=comp, state=k, isector=isec, norm2=norm2, alfa=a, beta=b, nlanc=n))
            fracs.append((comp, _peso_bz(states, k, 1.0, norm2, zeta), states.energies[k], E, z))
    vm, tg = bosonic_matsubara(copt.beta, copt.Lmats), tau_grid(copt.beta, copt.ltau)
    wr = realaxis(copt.wini, copt.wfin, copt.Lreal)
    iv, tau, w, _ = chi_poles_host(fracs, copt.beta, vm, tg, wr, copt.eps, n_components(cfg))
    return assemble(cfg, copt, iv, tau, w, spin=spin, dens=dens)
